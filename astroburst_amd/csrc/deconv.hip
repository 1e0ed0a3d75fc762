// Richardson-Lucy deconvolution on gfx950.
//
// Replaces core/analysis/deconvolution.rs: generate_gaussian_psf (:12-33), FftConvolver (:36-124), richardson_lucy (:141-221) and
// apply_deringing (:223-245).
//
// The reference convolves through f32 FFTs over a power-of-two buffer of at least rows + pr - 1 x cols + pc - 1 (math/fft.rs:122-127)
// with PSF tap (y, x) at ((y - pr/2) mod F, (x - pc/2) mod F).  That buffer is wide enough that no tap landing on the kept window
// wraps onto image data, so the product restricted to the window IS the linear convolution with a zero boundary:
//     conv(est)[y,x] = sum_{j,i} psf[j,i] * est[y - (j - pr/2), x - (i - pc/2)]
//     conv_T(r)[y,x] = sum_{j,i} psf[j,i] * r[y + (j - pr/2), x + (i - pc/2)]
// and it is computed here directly: 2 * pr * pc FMA per pixel per iteration against four 8192^2 complex FFTs for a 4096^2 frame.
// Each iteration is three launches on the context's stream:
//   rl_tiled_kernel<true>   conv(est) and ratio = img / (c + 1e-6f), one f32 plane (AB_WS_DECONV)
//   rl_tiled_kernel<false>  conv_T(ratio) fused with the update old * cor * inv_reg -> NaN-to-0 max -> f32 delta -> deringing,
//                           written over `est` in place (a pixel reads only its own old value), f64 delta^2 partial per workgroup
//   rl_finish_kernel        the partials summed in a fixed order -> iterations_run, convergence, converged (RlState)
// Every kernel of a later iteration reads `done` and returns at once (the masked-stretch pattern).  No atomics touch a pixel or a sum:
// two calls are bit-identical.
//
// Tiles: 256 lanes, each computes two adjacent columns x kRows rows (64 x 32 outputs per workgroup); the plane's tile + halo sits in
// LDS (zero outside the image: taps off the image are never read from memory), one LDS row window of 10 floats feeds kRows x 8
// v_pk_fma_f32, the PSF taps are uniform loads (scalar registers), zero-padded to a multiple of 8 columns.  PSFs up to
// kMaxTiledPsf (63) in either dimension, any aspect, even or odd; larger ones take rl_plain_kernel (one lane per pixel, straight
// from memory: correct, slower).
//
// Non-finite input: in the reference one NaN or inf entering an FFT spreads over the whole output.  A forward kernel that reads a
// non-finite estimate sample, or writes a non-finite ratio, raises a flag in RlState; the update then treats the whole correction as
// NaN (estimate -> max(NaN, 0) = 0, then the deringing clamp), as the reference does.  A non-finite PSF tap does the same for every
// iteration.  Finite inputs large enough to overflow the reference's FFT (|x| >= ~1e30) are outside the contract.
#include "entry_host.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kTx = 32, kTy = 8;       // 256 lanes
constexpr int kRows = 4;               // output rows per lane
constexpr int kTileW = 2 * kTx;        // 64 output columns (two adjacent per lane)
constexpr int kTileH = kRows * kTy;    // 32 output rows
constexpr int kTap = 8;                // taps per LDS window; the PSF's columns are zero-padded to a multiple of it
constexpr int kMaxTiledPsf = 63;
constexpr int kFinishBlock = 256;

struct RlState {
    double convergence;
    unsigned long long iterations_run;
    int done;
    int bad_est;    // this iteration's forward convolution read a non-finite estimate sample
    int bad_ratio;  // this iteration's ratio plane holds a non-finite value
    int bad_psf;    // the PSF holds a non-finite tap (every iteration)
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// wt = the PSF, wf = the PSF flipped in both axes; rows of pcp floats, zero beyond pc.  Initialises the chain state.
__global__ __launch_bounds__(kBlock) void rl_prep_kernel(const float *__restrict__ psf, int pr, int pc, int pcp, float *__restrict__ wf,
                                                         float *__restrict__ wt, RlState *__restrict__ st) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < pr * pcp; k += kBlock) {
        const int j = k / pcp, i = k % pcp;
        float plain = 0.0f, flipped = 0.0f;
        if (i < pc) {
            plain = psf[(int64_t)j * pc + i];
            flipped = psf[(int64_t)(pr - 1 - j) * pc + (pc - 1 - i)];
            if (!finite_f(plain)) bad = 1;
        }
        wt[k] = plain;
        wf[k] = flipped;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        st->convergence = DBL_MAX;  // f64::MAX until an iteration has run
        st->iterations_run = 0;
        st->done = 0;
        st->bad_est = 0;
        st->bad_ratio = 0;
        st->bad_psf = bad;
    }
}

// the update of one pixel (deconvolution.rs:171-185) and deringing (:223-245); returns the f32 delta widened to f64
__device__ __forceinline__ double rl_update(float *__restrict__ est, const float *__restrict__ img, int64_t p, float cor, float inv_reg,
                                            int deringing, float t_hi, float t_lo) {
    const float old = est[p];
    float e = old * cor * inv_reg;
    e = e > 0.0f ? e : 0.0f;  // f32::max(_, 0.0): NaN -> 0
    const double d = (double)(e - old);
    if (deringing) {
        const float orig = img[p];
        const float upper = orig * t_hi;
        float lower = orig * t_lo;
        lower = lower > 0.0f ? lower : 0.0f;
        if (e > upper)
            e = upper;
        else if (e < lower)
            e = lower;
    }
    est[p] = e;
    return d * d;
}

// fixed-order sum of one workgroup's f64 values (tree over the lanes)
__device__ __forceinline__ double block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// the lane's contribution of LDS row ty0 + a: taps of PSF row j = a - r to output row r.  kAll: every r has its j inside the PSF
// (no branch, so the four odd-offset pairs are formed once for all kRows rows)
template <bool kAll>
__device__ __forceinline__ void tile_row(const float *__restrict__ row, const float *__restrict__ w, int a, int pr, int pcp, f2 (&acc)[kRows]) {
    for (int c = 0; c < pcp / kTap; ++c) {
        const f2 *p = (const f2 *)(row + c * kTap);  // 8-byte aligned: lw, tx and c * kTap are even
        f2 e[5], o[4];
#pragma unroll
        for (int m = 0; m < 5; ++m) e[m] = p[m];
#pragma unroll
        for (int m = 0; m < 4; ++m) o[m] = (f2){e[m].y, e[m + 1].x};
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int j = a - r;
            if (!kAll && (j < 0 || j >= pr)) continue;
            const float *wr = w + j * pcp + c * kTap;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc[r] = __builtin_elementwise_fma(e[m], (f2)(wr[2 * m]), acc[r]);
                acc[r] = __builtin_elementwise_fma(o[m], (f2)(wr[2 * m + 1]), acc[r]);
            }
        }
    }
}

// kFwd: src = est, w = flipped PSF, halo (pr-1-pr/2, pc-1-pc/2); writes ratio = img / (c + 1e-6f) to dst.
// !kFwd: src = ratio, w = PSF, halo (pr/2, pc/2); updates dst = est in place and writes the workgroup's delta^2 partial.
// In both, out[y0+ty][x0+tx] = sum_j sum_i w[j][i] * T[ty + j][tx + i], T = the plane from (y0 - hy, x0 - hx) with a zero border.
template <bool kFwd>
__global__ __launch_bounds__(kBlock) void rl_tiled_kernel(const float *__restrict__ src, const float *__restrict__ w, int pr, int pcp, int hy,
                                                          int hx, int rows, int cols, const float *__restrict__ img, float *__restrict__ dst,
                                                          RlState *__restrict__ st, float inv_reg, int deringing, float t_hi, float t_lo,
                                                          double *__restrict__ partials) {
    extern __shared__ float tile[];  // (kTileH + pr - 1) x lw
    __shared__ double red[kBlock];
    if (st->done) return;
    const int lw = kTileW + pcp;  // even: every (row, even column) is 8-byte aligned
    const int lh = kTileH + pr - 1;
    const int y0 = blockIdx.y * kTileH, x0 = blockIdx.x * kTileW;
    const int lx = threadIdx.x % kTx, ly = threadIdx.x / kTx;
    const bool poisoned = !kFwd && (st->bad_psf | st->bad_est | st->bad_ratio);
    f2 acc[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) acc[r] = (f2)(0.0f);
    if (!poisoned) {
        int bad = 0;
        for (int a = ly; a < lh; a += kTy) {
            const int gy = y0 - hy + a;
            const bool row_in = gy >= 0 && gy < rows;
            for (int b = lx; b < lw; b += kTx) {
                const int gx = x0 - hx + b;
                float v = 0.0f;
                if (row_in && gx >= 0 && gx < cols) {
                    v = src[(int64_t)gy * cols + gx];
                    if (kFwd && !finite_f(v)) bad = 1;
                }
                tile[a * lw + b] = v;
            }
        }
        if (kFwd && bad) st->bad_est = 1;
        __syncthreads();
        const float *base = tile + (kRows * ly) * lw + 2 * lx;
        // LDS rows a = 0 .. kRows + pr - 2: the first and last kRows - 1 feed only some of the lane's rows
        for (int a = 0; a < kRows - 1; ++a) tile_row<false>(base + a * lw, w, a, pr, pcp, acc);
        for (int a = kRows - 1; a < pr; ++a) tile_row<true>(base + a * lw, w, a, pr, pcp, acc);
        for (int a = max(kRows - 1, pr); a < kRows + pr - 1; ++a) tile_row<false>(base + a * lw, w, a, pr, pcp, acc);
    }
    const int gx = x0 + 2 * lx;
    if (kFwd) {
        int bad = 0;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int gy = y0 + kRows * ly + r;
            if (gy >= rows) break;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (gx + q >= cols) break;
                const int64_t p = (int64_t)gy * cols + gx + q;
                const float ratio = img[p] / (acc[r][q] + 1e-6f);
                if (!finite_f(ratio)) bad = 1;
                dst[p] = ratio;
            }
        }
        if (bad) st->bad_ratio = 1;
    } else {
        double sq = 0.0;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int gy = y0 + kRows * ly + r;
            if (gy >= rows) break;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (gx + q >= cols) break;
                sq += rl_update(dst, img, (int64_t)gy * cols + gx + q, poisoned ? __builtin_nanf("") : acc[r][q], inv_reg, deringing, t_hi, t_lo);
            }
        }
        const double s = block_sum(sq, red);
        if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// PSFs beyond the tiled limit: one lane per pixel, every tap straight from memory (skipped where it falls off the image)
template <bool kFwd>
__global__ __launch_bounds__(kBlock) void rl_plain_kernel(const float *__restrict__ src, const float *__restrict__ w, int pr, int pc, int pcp,
                                                          int hy, int hx, int rows, int cols, const float *__restrict__ img,
                                                          float *__restrict__ dst, RlState *__restrict__ st, float inv_reg, int deringing,
                                                          float t_hi, float t_lo, double *__restrict__ partials) {
    __shared__ double red[kBlock];
    if (st->done) return;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in = p < (int64_t)rows * cols;
    const bool poisoned = !kFwd && (st->bad_psf | st->bad_est | st->bad_ratio);
    float c = 0.0f;
    int y = 0, x = 0;
    if (in) {
        y = (int)(p / cols);
        x = (int)(p % cols);
        if (!poisoned) {
            if (kFwd && !finite_f(src[p])) st->bad_est = 1;  // every sample is some lane's own pixel
            for (int j = 0; j < pr; ++j) {
                const int gy = y - hy + j;
                if (gy < 0 || gy >= rows) continue;
                for (int i = 0; i < pc; ++i) {
                    const int gx = x - hx + i;
                    if (gx < 0 || gx >= cols) continue;
                    c = fmaf(src[(int64_t)gy * cols + gx], w[j * pcp + i], c);
                }
            }
        }
    }
    if (kFwd) {
        if (in) {
            const float ratio = img[p] / (c + 1e-6f);
            if (!finite_f(ratio)) st->bad_ratio = 1;
            dst[p] = ratio;
        }
    } else {
        const double sq = in ? rl_update(dst, img, p, poisoned ? __builtin_nanf("") : c, inv_reg, deringing, t_hi, t_lo) : 0.0;
        const double s = block_sum(sq, red);
        if (threadIdx.x == 0) partials[blockIdx.x] = s;
    }
}

// the iteration's end (deconvolution.rs:187-209): sum_sq over the partials in a fixed order, convergence, the early stop
__global__ __launch_bounds__(kFinishBlock) void rl_finish_kernel(const double *__restrict__ partials, int nparts, double npix,
                                                                 RlState *__restrict__ st) {
    __shared__ double red[kFinishBlock];
    if (st->done) return;
    double v = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kFinishBlock) v += partials[i];
    const double sum_sq = block_sum(v, red);
    if (threadIdx.x == 0) {
        const unsigned long long it = st->iterations_run + 1;
        const double conv = sqrt(sum_sq / npix);
        st->iterations_run = it;
        st->convergence = conv;
        if (conv < 1e-6 && it >= 3) st->done = 1;
        st->bad_est = 0;
        st->bad_ratio = 0;
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool cancelled(ab_ctx *ctx) {
    ab_ctx *root = ctx;
    while (root->parent) root = root->parent;
    return root->cancel.load(std::memory_order_relaxed) != 0;
}

// richardson_lucy (:141-221) on device planes; `est` (rows x cols, not overlapping img) receives the result
int rl_device(ab_ctx *ctx, const float *img, int64_t rows64, int64_t cols64, const float *psf, int pr, int pc, const ab_rl_config &cfg,
              float *est, ab_rl_result *res) {
    const int rows = (int)rows64, cols = (int)cols64;
    const int64_t n = rows64 * cols64;
    AB_HIP(ctx, hipMemcpyAsync(est, img, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));  // estimate = image.clone()
    res->iterations_run = 0;
    res->convergence = DBL_MAX;
    if (cfg.iterations == 0) return AB_OK;
    const bool tiled = pr <= kMaxTiledPsf && pc <= kMaxTiledPsf;
    const int pcp = (pc + kTap - 1) / kTap * kTap;
    const dim3 tgrid(ab_div_up(cols, kTileW), ab_div_up(rows, kTileH));
    const int pgrid = ab_div_up(n, kBlock);
    const int nparts = tiled ? (int)(tgrid.x * tgrid.y) : pgrid;
    const size_t lds = tiled ? (size_t)(kTileH + pr - 1) * (size_t)(kTileW + pcp) * sizeof(float) : 0;
    const size_t wbytes = align256((size_t)pr * pcp * sizeof(float));
    const size_t off_wf = align256(sizeof(RlState)), off_wt = off_wf + wbytes, off_part = off_wt + wbytes;
    const size_t off_ratio = off_part + align256((size_t)nparts * sizeof(double));
    char *ws = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_DECONV, off_ratio + (size_t)n * sizeof(float), (void **)&ws));
    RlState *st = (RlState *)ws;
    float *wf = (float *)(ws + off_wf), *wt = (float *)(ws + off_wt), *ratio = (float *)(ws + off_ratio);
    double *partials = (double *)(ws + off_part);
    hipLaunchKernelGGL(rl_prep_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, psf, pr, pc, pcp, wf, wt, st);
    AB_HIP(ctx, hipGetLastError());

    const float lambda = (float)cfg.regularization;
    const float inv_reg = lambda > 0.0f ? 1.0f / (1.0f + lambda) : 1.0f;
    const float t_hi = 1.0f + cfg.deringing_threshold, t_lo = 1.0f - cfg.deringing_threshold;
    const int dr = cfg.deringing ? 1 : 0;
    const int cy = pr / 2, cx = pc / 2;
    // Iterations are enqueued in chunks of an estimated <= ~25 ms of GPU time (rates well below the measured ones), joined once per
    // chunk: the cancel flag is looked at and the progress callback ticked there, and a converged chain stops the enqueueing.
    const double est_ms = 4.0 * pr * pc * (double)n / (tiled ? 10e12 : 0.5e12) * 1e3;
    const size_t chunk = (size_t)std::max(1.0, std::min(256.0, std::floor(25.0 / std::max(est_ms, 1e-3))));
    void *pin = nullptr;
    AB_TRY(ab_pinned(ctx, sizeof(RlState), &pin));
    const RlState *hs = (const RlState *)pin;
    size_t enq = 0;
    char stage[64];
    while (true) {
        if (cancelled(ctx)) return ab_set_error(ctx, AB_ERR_CANCELLED, "Operation cancelled");  // (:151-155, at the top of an iteration)
        const size_t k_end = enq + std::min(chunk, cfg.iterations - enq);
        for (; enq < k_end; ++enq) {
            if (tiled) {
                hipLaunchKernelGGL(rl_tiled_kernel<true>, tgrid, dim3(kBlock), lds, ctx->stream, (const float *)est, (const float *)wf, pr, pcp,
                                   pr - 1 - cy, pc - 1 - cx, rows, cols, img, ratio, st, inv_reg, dr, t_hi, t_lo, partials);
                hipLaunchKernelGGL(rl_tiled_kernel<false>, tgrid, dim3(kBlock), lds, ctx->stream, (const float *)ratio, (const float *)wt, pr, pcp,
                                   cy, cx, rows, cols, img, est, st, inv_reg, dr, t_hi, t_lo, partials);
            } else {
                hipLaunchKernelGGL(rl_plain_kernel<true>, dim3(pgrid), dim3(kBlock), 0, ctx->stream, (const float *)est, (const float *)wf, pr, pc,
                                   pcp, pr - 1 - cy, pc - 1 - cx, rows, cols, img, ratio, st, inv_reg, dr, t_hi, t_lo, partials);
                hipLaunchKernelGGL(rl_plain_kernel<false>, dim3(pgrid), dim3(kBlock), 0, ctx->stream, (const float *)ratio, (const float *)wt, pr,
                                   pc, pcp, cy, cx, rows, cols, img, est, st, inv_reg, dr, t_hi, t_lo, partials);
            }
            hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(kFinishBlock), 0, ctx->stream, (const double *)partials, nparts, (double)n, st);
        }
        AB_HIP(ctx, hipGetLastError());
        AB_HIP(ctx, hipMemcpyAsync(pin, st, sizeof(RlState), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        res->iterations_run = (size_t)hs->iterations_run;
        res->convergence = hs->convergence;
        const bool last = hs->done || enq == cfg.iterations;
        snprintf(stage, sizeof stage, "iteration %llu/%llu", (unsigned long long)hs->iterations_run, (unsigned long long)cfg.iterations);
        const int rc = ab_progress(ctx, stage, hs->iterations_run, cfg.iterations);
        if (last) return AB_OK;  // (a cancel seen after the last iteration: the reference has no check left either)
        AB_TRY(rc);
    }
}

bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bn && b0 < a0 + an;
}

}  // namespace

extern "C" {

int ab_generate_gaussian_psf(size_t size, float sigma, float *out_host) try {
    if (size == 0 || !out_host) return AB_ERR_INVALID;  // (the reference's `size - 1` underflows)
    const float center = (float)(size - 1) / 2.0f;
    const float sigma2 = 2.0f * sigma * sigma;
    float sum = 0.0f;
    for (size_t y = 0; y < size; ++y) {
        for (size_t x = 0; x < size; ++x) {
            const float dy = (float)y - center;
            const float dx = (float)x - center;
            const float val = ::expf(-((dx * dx + dy * dy) / sigma2));
            out_host[y * size + x] = val;
            sum += val;
        }
    }
    if (sum > 0.0f)
        for (size_t i = 0; i < size * size; ++i) out_host[i] = out_host[i] / sum;
    return AB_OK;
} AB_CATCH_NOCTX

int ab_richardson_lucy(ab_ctx *ctx, const ab_plane *img, const ab_plane *psf, const ab_rl_config *cfg, ab_plane_mut *out,
                       ab_rl_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, img && psf && cfg && out && res, "null argument");
    AB_CHECK(ctx, psf->data && psf->rows > 0 && psf->cols > 0, "the PSF is empty");
    AB_CHECK(ctx, out->rows == img->rows && out->cols == img->cols, "output must have the image's dims");
    AB_CHECK(ctx, img->rows * img->cols < (int64_t(1) << 31) && psf->rows * psf->cols < (int64_t(1) << 31), "image too large for this build");
    if (img->data && out->data && img->rows > 0 && img->cols > 0) {
        const size_t bytes = (size_t)img->rows * (size_t)img->cols * sizeof(float);
        AB_CHECK(ctx, !ranges_overlap(img->data, bytes, out->data, bytes), "output must not overlap the image");
    }
    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    const float *in = nullptr, *kp = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    AB_TRY(sc.stage_in(psf, &kp));
    AB_TRY(sc.stage_out(out, &o));
    AB_TRY(rl_device(ctx, in, img->rows, img->cols, kp, (int)psf->rows, (int)psf->cols, *cfg, o, res));
    return sc.finish_outs();
} AB_CATCH(ctx)

}  // extern "C"
