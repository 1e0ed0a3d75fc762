// A trous (starlet) wavelet denoising on gfx950.
//
// Replaces core/imaging/wavelet.rs: wavelet_denoise (:41-133), atrous_smooth_buffers (:135-186), estimate_noise_sigma (:203-216),
// atrous_noise_scaling (:218-225), soft_threshold_slice (:227-236) and hard_threshold_slice (:238-244).
//
// The reference computes every pixel in f32 with one multiply and one add per tap, taps in the order ki = 0 .. 4, starting from
// 0.0f, and adds the thresholded details to the coarsest plane in the order d_0, d_1, ...  The library is built with
// -ffp-contract=off, every kernel below keeps those orders, and so the whole output plane equals the reference's bit for bit
// (tests/test_wavelet_cpu.py checks that the kernels' ISA holds no f32 fused multiply-add).  Its transposed route for the
// vertical pass (:157-172) stores the same values in another layout and changes no bit.
//
// One call is, on the context's stream:
//   per scale j (step = 2^j)     c_{j+1} = smooth(c_j, step):
//       wt_row_kernel + wt_col_kernel   two streaming launches through one intermediate plane, four adjacent pixels per lane -- or,
//       wt_fused_kernel          selected only through the developer library until it has been measured: one launch, the horizontal
//                                pass of a 64-column tile plus 2*step rows of halo above and below goes straight from memory into
//                                LDS, the vertical pass runs from LDS
//     scale 0 also writes d_0 = c_0 - c_1 (into the output plane, which nothing reads before the reconstruction overwrites it)
//   ab_plane_median_f32          the median of the finite |d_0| (plane_select.hip) -> noise_sigma -> ab_wavelet_scale_thresholds
//   wt_reconstruct_kernel        reads c_0 .. c_S, forms each d_j = c_j - c_{j+1}, thresholds it, adds in the reference's order
//                                from c_S, applies the finite-and-non-negative gate and writes the output: thresholding never
//                                makes a pass of its own (a recomputed c_j - c_{j+1} has the bits of a stored one)
// No atomics touch a pixel: two calls are bit-identical.
#include "entry_host.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxScales = 8;
constexpr int kPx = 4;            // adjacent pixels per lane of the streaming kernels
constexpr int kBx = 64, kBy = 4;  // their workgroup: 64 lanes along a row (256 pixels), 4 rows
constexpr int kTileW = 64;        // fused kernel: output columns per workgroup (one per lane of a wave)
constexpr int kFusedWaves = 4;    // ... and its 4 waves take the tile's rows in turn
constexpr int kFusedStepLimit = 32;       // (64 + 4 * 32) * 256 B = 48 KiB of LDS: within the 64 KiB a launch gets without an attribute
// The hand-over between the two forms.  0: every scale takes the two-pass form.  The fused kernel has not been measured against it
// yet, so the release library never selects it; it stays reachable through the developer switch below.
constexpr int kFusedMaxStepDefault = 0;

// B3_KERNEL_1D (wavelet.rs:35)
#define AB_B3_TAPS {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f}

__device__ __forceinline__ int clamp_idx(int64_t i, int dim) { return (int)(i < 0 ? 0 : (i > dim - 1 ? dim - 1 : i)); }

typedef float f4 __attribute__((ext_vector_type(4)));

// four adjacent floats; `aligned` (uniform): p is 16-byte aligned
__device__ __forceinline__ void load4(const float *__restrict__ p, bool aligned, float (&v)[kPx]) {
    if (aligned) {
        const f4 t = *(const f4 *)p;
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int q = 0; q < kPx; ++q) v[q] = p[q];
    }
}
__device__ __forceinline__ void store4(float *__restrict__ p, bool aligned, const float (&v)[kPx]) {
    if (aligned) {
        *(f4 *)p = (f4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int q = 0; q < kPx; ++q) p[q] = v[q];
    }
}

// the horizontal pass (:144-155).  vec: cols % 4 == 0 and both planes 16-byte aligned (every lane's four pixels are one float4)
__global__ __launch_bounds__(kBlock) void wt_row_kernel(const float *__restrict__ src, float *__restrict__ dst, int rows, int cols, int step,
                                                        int vec) {
    const float k[5] = AB_B3_TAPS;
    const int x0 = (blockIdx.x * kBx + threadIdx.x) * kPx;
    if (x0 >= cols) return;
    const bool whole = x0 + kPx <= cols;
    const bool inner = whole && x0 >= 2 * step && x0 + kPx - 1 < cols - 2 * step;  // no tap of the four pixels is clamped
    const bool tap_vec = vec && (step % kPx) == 0;
    for (int y = blockIdx.y * kBy + threadIdx.y; y < rows; y += gridDim.y * kBy) {
        const float *row = src + (int64_t)y * cols;
        float s[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (inner) {
#pragma unroll
            for (int ki = 0; ki < 5; ++ki) {
                float v[kPx];
                load4(row + x0 + (ki - 2) * step, tap_vec, v);
#pragma unroll
                for (int q = 0; q < kPx; ++q) s[q] = s[q] + v[q] * k[ki];
            }
        } else {
#pragma unroll
            for (int ki = 0; ki < 5; ++ki)
#pragma unroll
                for (int q = 0; q < kPx; ++q) s[q] = s[q] + row[clamp_idx((int64_t)x0 + q + (int64_t)(ki - 2) * step, cols)] * k[ki];
        }
        float *o = dst + (int64_t)y * cols + x0;
        if (whole) {
            store4(o, vec, s);
        } else {
            for (int q = 0; x0 + q < cols; ++q) o[q] = s[q];
        }
    }
}

// the vertical pass (:174-184); kDetail: also detail = prev - out (:72-76), prev = the plane the horizontal pass read
template <bool kDetail>
__global__ __launch_bounds__(kBlock) void wt_col_kernel(const float *__restrict__ src, float *__restrict__ dst, int rows, int cols, int step,
                                                        int vec, const float *__restrict__ prev, float *__restrict__ detail) {
    const float k[5] = AB_B3_TAPS;
    const int x0 = (blockIdx.x * kBx + threadIdx.x) * kPx;
    if (x0 >= cols) return;
    const bool whole = x0 + kPx <= cols;
    for (int y = blockIdx.y * kBy + threadIdx.y; y < rows; y += gridDim.y * kBy) {
        float s[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ki = 0; ki < 5; ++ki) {
            const float *p = src + (int64_t)clamp_idx((int64_t)y + (int64_t)(ki - 2) * step, rows) * cols + x0;
            float v[kPx] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (whole) {
                load4(p, vec, v);
            } else {
                for (int q = 0; x0 + q < cols; ++q) v[q] = p[q];
            }
#pragma unroll
            for (int q = 0; q < kPx; ++q) s[q] = s[q] + v[q] * k[ki];
        }
        const int64_t at = (int64_t)y * cols + x0;
        if (whole) {
            store4(dst + at, vec, s);
            if (kDetail) {
                float c[kPx], d[kPx];
                load4(prev + at, vec, c);
#pragma unroll
                for (int q = 0; q < kPx; ++q) d[q] = c[q] - s[q];
                store4(detail + at, vec, d);
            }
        } else {
            for (int q = 0; x0 + q < cols; ++q) {
                dst[at + q] = s[q];
                if (kDetail) detail[at + q] = prev[at + q] - s[q];
            }
        }
    }
}

// Both passes of one scale in one launch.  A workgroup owns kTileW columns x tile_rows rows.  Its horizontal pass is evaluated for
// those columns on tile_rows + 4 * step rows (LDS row a = plane row clamp(y0 - 2 * step + a, 0, rows - 1): the value the clamped
// vertical tap reads) straight from memory -- a wave reads 64 consecutive floats per tap -- into LDS; the vertical pass then
// reads LDS only (row stride 64 floats: a wave's 64 lanes hit 64 consecutive words).  LDS = (tile_rows + 4 * step) * 256 bytes.
template <bool kDetail>
__global__ __launch_bounds__(kBlock) void wt_fused_kernel(const float *__restrict__ src, float *__restrict__ dst, int rows, int cols, int step,
                                                          int tile_rows, float *__restrict__ detail) {
    extern __shared__ float hbuf[];  // (tile_rows + 4 * step) x kTileW
    const float k[5] = AB_B3_TAPS;
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    const int x = blockIdx.x * kTileW + tx;
    const int64_t y0 = (int64_t)blockIdx.y * tile_rows;
    const int lh = tile_rows + 4 * step;
    const bool col_in = x < cols;
    int cx[5];
#pragma unroll
    for (int ki = 0; ki < 5; ++ki) cx[ki] = clamp_idx((int64_t)x + (int64_t)(ki - 2) * step, cols);
    if (col_in) {
        for (int a = ty; a < lh; a += kFusedWaves) {
            const float *row = src + (int64_t)clamp_idx(y0 - 2 * step + a, rows) * cols;
            float s = 0.0f;
#pragma unroll
            for (int ki = 0; ki < 5; ++ki) s = s + row[cx[ki]] * k[ki];
            hbuf[a * kTileW + tx] = s;
        }
    }
    __syncthreads();
    if (!col_in) return;
    for (int r = ty; r < tile_rows; r += kFusedWaves) {
        const int64_t y = y0 + r;
        if (y >= rows) break;
        float s = 0.0f;
#pragma unroll
        for (int ki = 0; ki < 5; ++ki) s = s + hbuf[(r + ki * step) * kTileW + tx] * k[ki];
        const int64_t at = y * cols + x;
        dst[at] = s;
        if (kDetail) detail[at] = src[at] - s;
    }
}

struct ReconArgs {
    const float *c[kMaxScales + 1];  // c_0 = the image .. c_S
    float t[kMaxScales];             // ab_wavelet_scale_thresholds
    int scales;
    int soft;
};

// soft_threshold_slice (:227-236) / hard_threshold_slice (:238-244) of one value.  signum is +-1 for +-0 and NaN for NaN; a NaN
// fails `<=` and stays NaN either way
__device__ __forceinline__ float wt_threshold(float v, float t, int soft) {
    const float a = fabsf(v);
    if (a <= t) return 0.0f;
    if (!soft) return v;
    const float sg = (v != v) ? v : copysignf(1.0f, v);
    return sg * (a - t);
}

// thresholding (:93-105) and reconstruction (:112-121) of kN adjacent pixels per lane (kN = 4: planes and count 16-byte aligned)
template <int kN>
__global__ __launch_bounds__(kBlock) void wt_reconstruct_kernel(const ReconArgs a, int64_t n, float *__restrict__ out) {
    const int64_t p = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kN;
    if (p >= n) return;
    float hi[kN], sum[kN], lo[kN];  // c_{j+1}, the running sum, c_j
    float det[kMaxScales][kN];
#pragma unroll
    for (int q = 0; q < kN; ++q) hi[q] = 0.0f;
    // the planes are read from c_0 up, the details kept in registers, then added in the reference's order from c_S
    if (kN == 4) {
        float v[4];
        load4(a.c[0] + p, true, v);
#pragma unroll
        for (int q = 0; q < kN; ++q) lo[q] = v[q];
    } else {
        lo[0] = a.c[0][p];
    }
#pragma unroll
    for (int j = 0; j < kMaxScales; ++j) {
        if (j < a.scales) {
            if (kN == 4) {
                float v[4];
                load4(a.c[j + 1] + p, true, v);
#pragma unroll
                for (int q = 0; q < kN; ++q) hi[q] = v[q];
            } else {
                hi[0] = a.c[j + 1][p];
            }
#pragma unroll
            for (int q = 0; q < kN; ++q) {
                det[j][q] = wt_threshold(lo[q] - hi[q], a.t[j], a.soft);
                lo[q] = hi[q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kN; ++q) sum[q] = lo[q];  // c_S
#pragma unroll
    for (int j = 0; j < kMaxScales; ++j) {
        if (j < a.scales) {
#pragma unroll
            for (int q = 0; q < kN; ++q) sum[q] = sum[q] + det[j][q];
        }
    }
    float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < kN; ++q) o[q] = (__builtin_isfinite(sum[q]) && sum[q] >= 0.0f) ? sum[q] : 0.0f;
    if (kN == 4) {
        store4(out + p, true, o);
    } else {
        out[p] = o[0];
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bn && b0 < a0 + an;
}

// atrous_noise_scaling (:218-225)
double noise_scaling(int scale) {
    static const double table[7] = {0.8908, 0.2007, 0.0856, 0.0413, 0.0205, 0.0103, 0.0051};
    if (scale < 7) return table[scale];
    return table[6] / std::ldexp(1.0, scale - 6);  // 2.0f64.powi(scale - 6): a power of two, exact
}

// the fused kernel's grid has one row of workgroups per tile_rows rows: planes beyond the grid's y limit stream
bool takes_fused(int rows, int step, int fused_max_step, int tile_rows) { return step <= fused_max_step && ab_div_up(rows, tile_rows) <= 65535; }

// c_{j+1} = smooth(c_j, step) on the context's stream; detail (nullable) = c_j - c_{j+1}
int smooth_scale(ab_ctx *ctx, const float *cur, float *next, float *hplane, int rows, int cols, int step, int fused_max_step, int tile_rows,
                 float *detail) {
    if (takes_fused(rows, step, fused_max_step, tile_rows)) {
        const dim3 grid(ab_div_up(cols, kTileW), ab_div_up(rows, tile_rows));
        const size_t lds = (size_t)(tile_rows + 4 * step) * kTileW * sizeof(float);
        if (detail)
            hipLaunchKernelGGL(wt_fused_kernel<true>, grid, dim3(kBlock), lds, ctx->stream, cur, next, rows, cols, step, tile_rows, detail);
        else
            hipLaunchKernelGGL(wt_fused_kernel<false>, grid, dim3(kBlock), lds, ctx->stream, cur, next, rows, cols, step, tile_rows, detail);
    } else {
        const dim3 grid(ab_div_up(cols, kBx * kPx), std::min(ab_div_up(rows, kBy), 65535)), block(kBx, kBy);
        const int vec = cols % kPx == 0 && aligned16(cur) && aligned16(next) && aligned16(hplane) && (!detail || aligned16(detail));
        hipLaunchKernelGGL(wt_row_kernel, grid, block, 0, ctx->stream, cur, hplane, rows, cols, step, vec);
        if (detail)
            hipLaunchKernelGGL(wt_col_kernel<true>, grid, block, 0, ctx->stream, (const float *)hplane, next, rows, cols, step, vec, cur, detail);
        else
            hipLaunchKernelGGL(wt_col_kernel<false>, grid, block, 0, ctx->stream, (const float *)hplane, next, rows, cols, step, vec, cur, detail);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// wavelet_denoise (:41-133) on device planes; `out` (rows x cols, not overlapping img) receives the result
int wavelet_device(ab_ctx *ctx, const float *img, int64_t rows64, int64_t cols64, const ab_wavelet_config &cfg, float *out, ab_wavelet_result *res) {
    const int rows = (int)rows64, cols = (int)cols64;
    const int64_t n = rows64 * cols64;
    const int S = (int)std::min<size_t>(std::max<size_t>(cfg.num_scales, 1), kMaxScales);  // (:47)
    const uint64_t total = 2 * (uint64_t)S + 1;                                            // (:51-53)
    // Steps up to fused_max_step take the fused kernel, larger ones the two-pass form.  The developer library can move the hand-over
    // (AB_WAVELET_FUSED_MAX_STEP, up to 32) and change the tile height, to cross-check the two forms against each other and to sweep.
    int fused_max_step = kFusedMaxStepDefault, tile_rows = 64;
    if (const char *v = ab_dev_env("AB_WAVELET_FUSED_MAX_STEP")) fused_max_step = std::max(0, std::min(atoi(v), kFusedStepLimit));
    if (const char *v = ab_dev_env("AB_WAVELET_TILE_ROWS")) tile_rows = std::max(16, std::min(atoi(v), 128)) / kFusedWaves * kFusedWaves;
    // c_1 .. c_S, and the horizontal pass's plane only when some scale takes the two-pass form
    bool two_pass = false;
    for (int j = 0; j < S; ++j) two_pass = two_pass || !takes_fused(rows, 1 << j, fused_max_step, tile_rows);
    const size_t plane = align256((size_t)n * sizeof(float));
    char *ws = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_WAVELET, plane * (size_t)(S + (two_pass ? 1 : 0)), (void **)&ws));
    float *hplane = two_pass ? (float *)(ws + plane * (size_t)S) : nullptr;
    ReconArgs ra = {};
    ra.c[0] = img;
    for (int j = 1; j <= S; ++j) ra.c[j] = (const float *)(ws + plane * (size_t)(j - 1));
    ra.scales = S;
    ra.soft = cfg.linear_denoise ? 1 : 0;

    char stage[64];
    uint64_t tick = 0;
    for (int j = 0; j < S; ++j) {
        snprintf(stage, sizeof stage, "decomposing scale %d/%d", j + 1, S);
        AB_TRY(ab_progress(ctx, stage, ++tick, total));  // (:62-67: the cancel check, then the tick)
        AB_TRY(smooth_scale(ctx, ra.c[j], (float *)ra.c[j + 1], hplane, rows, cols, 1 << j, fused_max_step, tile_rows, j == 0 ? out : nullptr));
    }
    // estimate_noise_sigma (:203-216): the median of the finite |d_0|, even counts averaged in f32; 0 when there is none
    ab_plane_sel sel;
    sel.data = out;
    sel.n = n;
    sel.min_valid = -INFINITY;
    sel.use_dev = 1;
    sel.center = 0.0f;
    float med = 0.0f;
    AB_TRY(ab_plane_median_f32(ctx, sel, &med, nullptr));
    const double noise_sigma = (double)med * 1.4826;  // MAD_TO_SIGMA (types/constants.rs:7)
    AB_TRY(ab_wavelet_scale_thresholds(noise_sigma, &cfg, ra.t));
    for (int j = 0; j < S; ++j) {
        snprintf(stage, sizeof stage, "thresholding scale %d/%d", j + 1, S);
        AB_TRY(ab_progress(ctx, stage, ++tick, total));  // (:86-91)
    }
    (void)ab_progress(ctx, "reconstructing", ++tick, total);  // (:108-110: no cancel check is left in the reference either)
    bool vec = n % 4 == 0 && aligned16(out);
    for (int j = 0; j <= S; ++j) vec = vec && aligned16(ra.c[j]);
    if (vec)
        hipLaunchKernelGGL(wt_reconstruct_kernel<4>, dim3(ab_div_up(n / 4, kBlock)), dim3(kBlock), 0, ctx->stream, ra, n, out);
    else
        hipLaunchKernelGGL(wt_reconstruct_kernel<1>, dim3(ab_div_up(n, kBlock)), dim3(kBlock), 0, ctx->stream, ra, n, out);
    AB_HIP(ctx, hipGetLastError());
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the result is complete on return, as ab_richardson_lucy's is)
    res->scales_processed = (size_t)S;
    res->noise_estimate = noise_sigma;
    return AB_OK;
}

}  // namespace

extern "C" {

int ab_wavelet_scale_thresholds(double noise_sigma, const ab_wavelet_config *cfg, float *out) try {
    if (!cfg || !out || (cfg->num_thresholds > 0 && !cfg->thresholds)) return AB_ERR_INVALID;
    const size_t len = cfg->num_thresholds;
    for (int j = 0; j < kMaxScales; ++j) {
        const float ts = (size_t)j < len ? cfg->thresholds[j] : (len > 0 ? cfg->thresholds[len - 1] : 1.0f);  // (:93-97)
        out[j] = ts * (float)(noise_sigma * noise_scaling(j));                                                 // (:99)
    }
    return AB_OK;
} AB_CATCH_NOCTX

int ab_wavelet_denoise(ab_ctx *ctx, const ab_plane *img, const ab_wavelet_config *cfg, ab_plane_mut *out, ab_wavelet_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, img && cfg && out && res, "null argument");
    AB_CHECK(ctx, img->data && img->rows > 0 && img->cols > 0, "the image is empty");
    AB_CHECK(ctx, out->data, "null output plane");
    AB_CHECK(ctx, out->rows == img->rows && out->cols == img->cols, "output must have the image's dims");
    AB_CHECK(ctx, img->rows < (int64_t(1) << 31) && img->cols < (int64_t(1) << 31) && img->rows * img->cols < (int64_t(1) << 31),
             "image too large for this build");
    AB_CHECK(ctx, cfg->num_thresholds == 0 || cfg->thresholds, "null threshold list");
    const size_t bytes = (size_t)img->rows * (size_t)img->cols * sizeof(float);
    AB_CHECK(ctx, !ranges_overlap(img->data, bytes, out->data, bytes), "output must not overlap the image");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    const float *in = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    AB_TRY(sc.stage_out(out, &o));
    AB_TRY(wavelet_device(ctx, in, img->rows, img->cols, *cfg, o, res));
    return sc.finish_outs();
} AB_CATCH(ctx)

}  // extern "C"
