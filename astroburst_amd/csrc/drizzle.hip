// Drizzle stacking on gfx950.
//
// Replaces core/stacking/drizzle.rs: drizzle_stack (:227-346) = crop to the minimum dims, offsets, DrizzleAccumulator::drizzle_frame
// (:46-122) per frame and finalize (:124-199).
//
// The reference SCATTERS: every finite input pixel pushes its value onto the sample list of each output pixel inside its window whose
// weight exceeds 1e-12, frame after frame, input row after input row, column after column, and `push` (:38-45) drops whatever arrives
// once a list holds max(2 n, 4) samples.  The order in which ONE output pixel receives its samples is therefore fixed -- frame, then
// input row, then input column, and an input pixel pushes to a given output pixel at most once -- so the same lists are rebuilt here
// as a GATHER: one lane per output pixel walks the frames in order and, inside a frame, the few input pixels that can reach it in
// raster order.  No atomics, no n_out x 2 n list storage, and two runs give identical bytes.
//
// Which input pixels can reach output pixel o (per axis; c = (i + d) * scale is the input pixel's centre, half = pixfrac * scale / 2):
//   the reference's window is clamp_index(floor(c - half)) ..= clamp_index(ceil(c + half)).  For 0 < o < n_out - 1 the clamps change
//   nothing about o's membership, and floor(c - half) <= o <= ceil(c + half) needs c - half < o + 1 and c + half > o - 1, i.e.
//   |o + 0.5 - c| < half + 1.5.  clamp_index clamps ONTO the border, so o = 0 and o = n_out - 1 are also in the window of every
//   footprint that lies beyond them: there only the weight bounds the distance.  w > 1e-12 needs
//     Square    both overlaps positive: c - half < o + 1 and c + half > o            -> |o + 0.5 - c| < half + 0.5
//     Gaussian  exp(-d2 / (2 s^2)) > 1e-12, d2 >= (o + 0.5 - c)^2, ln(1e12) = 27.631 -> |o + 0.5 - c| < s * sqrt(2 * 27.64) < 7.44 s
//     Lanczos3  lanczos3(x) = 0 for |x| >= 3                                         -> |o + 0.5 - c| < 3
//   (the weight bound holds for interior pixels too: the smaller of the two is used there).  With that radius B the candidates are
//   the integers i with (o + 0.5 - B) / scale - d - pad <= i <= (o + 0.5 + B) / scale - d + pad, cut to the frame; pad = 1e-9 of the
//   magnitudes involved covers the rounding of c and of this estimate (a few 2^-52 relative) a million times over.  That is at most
//   2 B / scale + 3 indices, and with half / scale = pixfrac / 2 <= 0.5, s = max(half, 0.5) and scale >= 1: 2 B / scale <= 7.44, at
//   most 11 indices per axis (kMaxCand 16); Square at the default scale 2 / pixfrac 0.7: 2 or 3.
//   Each candidate is then put to the reference's EXACT test in the reference's f64 operations and order (-ffp-contract=off):
//   floor / ceil / clamp of the same c -+ half per axis (a bit mask per axis: the window is a product of two intervals), the weight,
//   `w > 1e-12`, and the cap.
//
// finalize: the list never exceeds cap = max(2 n, 4).  Up to kLdsCap (64 samples = 32 frames, the reference's everyday range) the
// lane keeps its list as a column of dynamic LDS (sample k of lane t at [k * 256 + t]: conflict-free) and finishes in the same
// kernel.  Longer lists (33 .. 32 767 frames) take the same kernel body with the column in a global scratch of at most kScratchBytes,
// whatever the image: the output is processed in runs of kScratchBytes / (4 cap) consecutive pixels.  Either way the lane sorts its
// column (LDS path: through registers and the project's sorting network, sortnet_gen.hpp; long lists: heap sort in memory), after which every step of the MAD clip is a walk over a sorted range:
//   median_f32_mut (math/median.rs:46-61) = s[m/2], or (s[m/2 - 1] + s[m/2]) / 2.0f;
//   the deviations |v - median| (f32) grow monotonically away from the median on either side, so their order statistics come from
//   a two-pointer merge outward from the middle;
//   `dev >= -sigma_low * sigma && dev <= sigma_high * sigma` with dev = v - median monotone in v keeps a contiguous range [a, b).
// The survivors' f64 sum runs in ascending order of value (the pin oracle/orc_combine.c documents for what select_nth_unstable
// leaves unspecified).  rejected_pixels: a u64 partial per workgroup, summed in a fixed order by dz_finish_kernel.
#include "entry_host.hpp"

#include <algorithm>
#include <cmath>

// the sorting networks the stacking kernels use (tools/gen_sortnet.py); every sample that reaches one is finite or a +inf pad
#define AB_CE(a, b)                         \
    {                                       \
        T lo_ = fminf(v[a], v[b]);          \
        T hi_ = fmaxf(v[a], v[b]);          \
        v[a] = lo_;                         \
        v[b] = hi_;                         \
    }
#define AB_SORT4(a, b, c, d)                                                         \
    {                                                                                \
        const T x0_ = v[a], x1_ = v[b], x2_ = v[c], x3_ = v[d];                      \
        const T s0_ = fminf(fminf(x0_, x1_), x2_), s1_ = __builtin_amdgcn_fmed3f(x0_, x1_, x2_), \
                s2_ = fmaxf(fmaxf(x0_, x1_), x2_);                                   \
        v[a] = __builtin_amdgcn_fmed3f(-__builtin_inff(), s0_, x3_);                 \
        v[b] = __builtin_amdgcn_fmed3f(s0_, s1_, x3_);                               \
        v[c] = __builtin_amdgcn_fmed3f(s1_, s2_, x3_);                               \
        v[d] = __builtin_amdgcn_fmed3f(__builtin_inff(), s2_, x3_);                  \
    }
#define AB_STACK_CE_XOR 1
#include "sort_ops.hpp"
#include "sortnet_gen.hpp"

namespace {

constexpr int kFinishBlock = 1024;
constexpr int kTileW = 64, kTileH = 4;  // the LDS path's workgroup: 64 x 4 output pixels, a wave per output row
constexpr int kLdsCap = 64;             // lists of up to 64 samples (32 frames) stay in LDS: 256 * 64 * 4 = 64 KiB per workgroup
constexpr int kMaxCand = 16;            // candidate input indices per axis (<= 12, derived above)
constexpr size_t kScratchBytes = (size_t)256 << 20;  // the long-list path's sample columns
constexpr int kMaxFrames = 32767;       // the reference counts samples in a u16: 2 n must fit
constexpr int kBandRows = 1024;         // output rows per launch of the LDS path (progress tick / cancel check between them)

struct DzFrame {
    const float *p;
    int64_t ld;
    double dx, dy;  // what drizzle_frame receives: the NEGATED offsets (drizzle.rs:323)
};

struct DzParams {
    int in_rows, in_cols, out_rows, out_cols;
    int n_frames, cap, iters;
    float sigma_low, sigma_high;
    double scale, inv_scale, half;
    double two_sigma2;  // Gaussian: 2.0 * sigma * sigma, sigma = max(half, 0.5)
    double reach;       // the weight's radius B in output pixels (see above)
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// clamp_index (core/imaging/boundary.rs:9-20) of a floor / ceil result kept in f64 (`as i64` saturates: the clamp gives the same index)
__device__ __forceinline__ double clamp_idx(double v, double last) { return v < 0.0 ? 0.0 : (v > last ? last : v); }

// bit k set: input index lo + k has output index o inside its window on this axis (drizzle.rs:73-80)
__device__ __forceinline__ unsigned axis_mask(int o, int n_in, int n_out, double d, const DzParams &P, int *lo_out) {
    const bool border = o == 0 || o == n_out - 1;
    const double B = border ? P.reach : fmin(P.reach, P.half + 1.5);
    const double ctr = (double)o + 0.5;
    // i + d in ((ctr - B) / scale, (ctr + B) / scale) in exact arithmetic; `pad` (>= 1e-9 of every magnitude involved, against a few
    // 2^-52 of rounding in c and in this estimate) widens it, floor / ceil take the integers around it
    // (capped at half a pixel: a frame whose |d| is beyond 1e9 px either misses the field altogether or is still covered by 0.5)
    const double pad = fmin(1e-9 * (fabs(d) + (double)n_in + (double)n_out + B), 0.5);
    const double lo_d = fmax(floor((ctr - B) * P.inv_scale - d - pad), 0.0);
    const double hi_d = fmin(ceil((ctr + B) * P.inv_scale - d + pad), (double)(n_in - 1));
    *lo_out = 0;
    if (!(lo_d <= hi_d)) return 0u;
    const int lo = (int)lo_d, cnt = min((int)hi_d - lo + 1, kMaxCand);
    *lo_out = lo;
    const double last = (double)(n_out - 1), od = (double)o;
    unsigned m = 0u;
    for (int k = 0; k < cnt; ++k) {
        const double c = ((double)(lo + k) + d) * P.scale;
        const double a = clamp_idx(floor(c - P.half), last), b = clamp_idx(ceil(c + P.half), last);
        if (a <= od && od <= b) m |= 1u << k;
    }
    return m;
}

__device__ __forceinline__ double lanczos3(double x) {  // drizzle.rs:212-221
    if (fabs(x) < 1e-12) return 1.0;
    if (fabs(x) >= 3.0) return 0.0;
    const double pi_x = 3.14159265358979323846 * x;
    const double pi_x_3 = pi_x / 3.0;
    return (sin(pi_x) / pi_x) * (sin(pi_x_3) / pi_x_3);
}

template <int kKernel>
__device__ __forceinline__ double dz_weight(double cx, double cy, int ox, int oy, const DzParams &P) {  // drizzle.rs:84-103
    if (kKernel == 0) {  // overlap_area (:202-209)
        const double w = fmax(fmin(cx + P.half, (double)ox + 1.0) - fmax(cx - P.half, (double)ox), 0.0);
        const double h = fmax(fmin(cy + P.half, (double)oy + 1.0) - fmax(cy - P.half, (double)oy), 0.0);
        return w * h;
    } else if (kKernel == 1) {
        const double ex = (double)ox + 0.5 - cx, ey = (double)oy + 0.5 - cy;
        const double dist2 = ex * ex + ey * ey;
        return exp(-dist2 / P.two_sigma2);
    } else {
        return lanczos3(fabs((double)ox + 0.5 - cx)) * lanczos3(fabs((double)oy + 0.5 - cy));
    }
}

// a lane's sample column: element k at base[k * stride]
struct Column {
    float *base;
    size_t stride;
    __device__ __forceinline__ float get(int k) const { return base[(size_t)k * stride]; }
    __device__ __forceinline__ void set(int k, float v) const { base[(size_t)k * stride] = v; }
};

// the LDS path's sort: the column goes through registers -- kNP wires (the list capacity rounded up to a power of two), +inf beyond
// the pixel's n samples -- and Batcher's network in the rewritten three-input form; every index is a compile-time constant
template <int kNP>
__device__ __forceinline__ void network_sort(const Column &s, int n) {
    float v[kNP];
#pragma unroll
    for (int k = 0; k < kNP; ++k) v[k] = k < n ? s.get(k) : __builtin_inff();
    SortNet<kNP>::sort_fused(v);
#pragma unroll
    for (int k = 0; k < kNP; ++k)
        if (k < n) s.set(k, v[k]);
}

__device__ void sift_down(const Column &s, int root, int n) {
    const float v = s.get(root);
    while (true) {
        int child = 2 * root + 1;
        if (child >= n) break;
        float c = s.get(child);
        if (child + 1 < n) {
            const float c2 = s.get(child + 1);
            if (c2 > c) {
                c = c2;
                ++child;
            }
        }
        if (!(c > v)) break;
        s.set(root, c);
        root = child;
    }
    s.set(root, v);
}

__device__ void heap_sort(const Column &s, int n) {
    for (int i = n / 2 - 1; i >= 0; --i) sift_down(s, i, n);
    for (int end = n - 1; end > 0; --end) {
        const float top = s.get(0);
        s.set(0, s.get(end));
        s.set(end, top);
        sift_down(s, 0, end);
    }
}

// median_f32_mut of |s[i] - med| over the sorted range [a, b), m = b - a >= 3: s[a + m/2 - 1] <= med <= s[a + m/2], so the
// deviations are non-decreasing going down from a + m/2 - 1 and going up from a + m/2; merge the two runs up to rank m/2
__device__ float mad_of_sorted(const Column &s, int a, int b, float med) {
    const int m = b - a, mid = m / 2;
    int l = a + mid - 1, r = a + mid;
    float prev = 0.0f, cur = 0.0f;
    for (int k = 0; k <= mid; ++k) {
        const float dl = l >= a ? fabsf(s.get(l) - med) : 0.0f;
        const float dr = r < b ? fabsf(s.get(r) - med) : 0.0f;
        const bool take_l = l >= a && (r >= b || dl <= dr);
        prev = cur;
        cur = take_l ? dl : dr;
        if (take_l) --l;
        else ++r;
    }
    return (m & 1) ? cur : (prev + cur) / 2.0f;
}

// finalize (drizzle.rs:124-199) of one pixel's n >= 2 samples
template <int kNP>
__device__ float dz_finalize(const Column &s, int n, const DzParams &P, unsigned *rejected) {
    if constexpr (kNP > 0) network_sort<kNP>(s, n);
    else heap_sort(s, n);
    int a = 0, b = n;
    unsigned rej = 0;
    for (int it = 0; it < P.iters; ++it) {
        const int m = b - a;
        if (m < 3) break;
        const int mid = a + m / 2;
        const float med = (m & 1) ? s.get(mid) : (s.get(mid - 1) + s.get(mid)) / 2.0f;
        const float mad = mad_of_sorted(s, a, b, med);
        const float sigma = (float)fmax((double)mad * 1.4826, 1e-10);
        const float t_lo = -P.sigma_low * sigma, t_hi = P.sigma_high * sigma;
        int na = a;
        while (na < b && !(s.get(na) - med >= t_lo)) ++na;
        int nb = b;
        while (nb > na && !(s.get(nb - 1) - med <= t_hi)) --nb;
        const int removed = m - (nb - na);
        a = na;
        b = nb;
        rej += (unsigned)removed;
        if (removed == 0) break;
    }
    *rejected = rej;
    if (a == b) {  // nothing survives (:181-187): the mean of every sample
        a = 0;
        b = n;
    }
    double sum = 0.0;
    for (int k = a; k < b; ++k) sum += (double)s.get(k);
    return (float)(sum / (double)(b - a));
}

// kLds: grid (ceil(out_cols / 64), rows of the band / 4), output rows from row0; the columns live in dynamic LDS (256 * cap floats).
// !kLds: a 1-D grid over the pixels [p0, p0 + count); lane g's column is lists[g + k * lanes] (lanes = gridDim.x * 256).
// kNP: the network's width on the LDS path (8, 16, 32, 64 >= cap), 0 on the long-list path
template <bool kLds, int kKernel, int kNP>
__global__ __launch_bounds__(kBlock) void dz_gather_kernel(const DzFrame *__restrict__ frames, DzParams P, int row0, int64_t p0, int64_t count,
                                                           float *__restrict__ lists, float *__restrict__ img, float *__restrict__ wgt,
                                                           unsigned long long *__restrict__ partials) {
    extern __shared__ float lds[];
    int ox, oy;
    bool valid;
    Column col;
    if (kLds) {
        ox = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1));
        oy = row0 + blockIdx.y * kTileH + (threadIdx.x >> 6);
        valid = ox < P.out_cols && oy < P.out_rows;
        col.base = lds + threadIdx.x;
        col.stride = kBlock;
    } else {
        const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        valid = g < count;
        const int64_t p = p0 + (valid ? g : 0);
        oy = (int)(p / P.out_cols);
        ox = (int)(p - (int64_t)oy * P.out_cols);
        col.base = lists + g;
        col.stride = (size_t)gridDim.x * kBlock;
    }
    int cnt = 0;
    double wsum = 0.0;
    for (int f = 0; f < P.n_frames; ++f) {
        const bool live = valid && cnt < P.cap;
        if (__ballot(live) == 0ull) break;  // every pixel of the wave is full: the remaining frames push nothing
        if (!live) continue;
        const DzFrame fr = frames[f];
        int ylo, xlo;
        const unsigned my = axis_mask(oy, P.in_rows, P.out_rows, fr.dy, P, &ylo);
        if (my == 0u) continue;
        const unsigned mx = axis_mask(ox, P.in_cols, P.out_cols, fr.dx, P, &xlo);
        if (mx == 0u) continue;
        for (unsigned ry = my; ry != 0u && cnt < P.cap; ry &= ry - 1u) {
            const int iy = ylo + __ffs(ry) - 1;
            const double cy = ((double)iy + fr.dy) * P.scale;
            const float *row = fr.p + (int64_t)iy * fr.ld;
            for (unsigned rx = mx; rx != 0u; rx &= rx - 1u) {
                const int ix = xlo + __ffs(rx) - 1;
                const float val = row[ix];
                if (!finite_f(val)) continue;
                const double cx = ((double)ix + fr.dx) * P.scale;
                const double w = dz_weight<kKernel>(cx, cy, ox, oy, P);
                if (w > 1e-12 && cnt < P.cap) {  // push (:38-45)
                    col.set(cnt, val);
                    ++cnt;
                    wsum += w;
                }
            }
        }
    }
    unsigned rej = 0;
    if (valid) {
        float v = 0.0f, w = 0.0f;
        if (cnt == 1) {
            v = col.get(0);
            w = (float)wsum;
        } else if (cnt >= 2) {
            v = dz_finalize<kNP>(col, cnt, P, &rej);
            w = (float)wsum;
        }
        const int64_t p = (int64_t)oy * P.out_cols + ox;
        img[p] = v;
        if (wgt) wgt[p] = w;
    }
    // the workgroup's rejected count: lanes -> wave (shuffles) -> workgroup (four words of LDS, reused once every column is done)
    unsigned long long r = rej;
    for (int off = 32; off > 0; off >>= 1) r += __shfl_down(r, off, 64);
    __syncthreads();
    unsigned long long *red = (unsigned long long *)lds;
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t blk = kLds ? (size_t)blockIdx.y * gridDim.x + blockIdx.x : (size_t)blockIdx.x;
        partials[blk] = red[0] + red[1] + red[2] + red[3];
    }
}

__global__ __launch_bounds__(kFinishBlock) void dz_finish_kernel(const unsigned long long *__restrict__ partials, size_t nparts,
                                                                 unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[kFinishBlock];
    unsigned long long v0 = 0, v1 = 0, v2 = 0, v3 = 0;  // (four loads in flight per lane: 262 144 partials for an 8192^2 output)
    size_t i = threadIdx.x;
    for (; i + 3 * kFinishBlock < nparts; i += 4 * kFinishBlock) {
        v0 += partials[i];
        v1 += partials[i + kFinishBlock];
        v2 += partials[i + 2 * kFinishBlock];
        v3 += partials[i + 3 * kFinishBlock];
    }
    for (; i < nparts; i += kFinishBlock) v0 += partials[i];
    red[threadIdx.x] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    for (int s = kFinishBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

template <bool kLds, int kNP>
void dz_launch_np(int kernel, dim3 grid, size_t lds, hipStream_t stream, const DzFrame *frames, const DzParams &P, int row0, int64_t p0, int64_t count,
                  float *lists, float *img, float *wgt, unsigned long long *partials) {
    if (kernel == 0)
        hipLaunchKernelGGL((dz_gather_kernel<kLds, 0, kNP>), grid, dim3(kBlock), lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
    else if (kernel == 1)
        hipLaunchKernelGGL((dz_gather_kernel<kLds, 1, kNP>), grid, dim3(kBlock), lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
    else
        hipLaunchKernelGGL((dz_gather_kernel<kLds, 2, kNP>), grid, dim3(kBlock), lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
}
template <bool kLds>
void dz_launch(int kernel, dim3 grid, size_t lds, hipStream_t stream, const DzFrame *frames, const DzParams &P, int row0, int64_t p0, int64_t count,
               float *lists, float *img, float *wgt, unsigned long long *partials) {
    if (!kLds) dz_launch_np<false, 0>(kernel, grid, lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
    else if (P.cap <= 8) dz_launch_np<true, 8>(kernel, grid, lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
    else if (P.cap <= 16) dz_launch_np<true, 16>(kernel, grid, lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
    else if (P.cap <= 32) dz_launch_np<true, 32>(kernel, grid, lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
    else dz_launch_np<true, kLdsCap>(kernel, grid, lds, stream, frames, P, row0, p0, count, lists, img, wgt, partials);
}

// steps 1-2 of drizzle_stack (drizzle.rs:231-279): the frame-count and dimension checks, the crop, the clamps, the output dims
struct DzDims {
    int64_t in_rows, in_cols, out_rows, out_cols;
    double scale, pixfrac;
};
int dz_dims(ab_ctx *ctx, const ab_plane *planes, size_t n, const ab_drizzle_config *cfg, DzDims *d) {
    if (n == 0) return ab_set_error(ctx, AB_ERR_INVALID, "No images to drizzle");
    if (n < 2) return ab_set_error(ctx, AB_ERR_INVALID, "Drizzle requires at least 2 frames for sub-pixel reconstruction");
    if (n > (size_t)kMaxFrames) return ab_set_error(ctx, AB_ERR_INVALID, "Drizzle takes at most %d frames (the reference counts 2 n samples in a u16)", kMaxFrames);
    if (!planes || !cfg) return ab_set_error(ctx, AB_ERR_INVALID, "null argument");
    int64_t min_r = planes[0].rows, min_c = planes[0].cols, max_r = min_r, max_c = min_c;
    for (size_t i = 0; i < n; ++i) {
        if (planes[i].rows < 0 || planes[i].cols < 0) return ab_set_error(ctx, AB_ERR_INVALID, "frame %zu has negative dims", i);
        min_r = std::min(min_r, planes[i].rows);
        max_r = std::max(max_r, planes[i].rows);
        min_c = std::min(min_c, planes[i].cols);
        max_c = std::max(max_c, planes[i].cols);
    }
    const int64_t row_diff = max_r - min_r, col_diff = max_c - min_c;
    const int64_t tolerance = (int64_t)((double)std::max(min_r, min_c) * 0.05);
    if (row_diff > tolerance || col_diff > tolerance)
        return ab_set_error(ctx, AB_ERR_INVALID, "Frame dimensions vary too much (rows: %lldpx, cols: %lldpx, tolerance: %lldpx)", (long long)row_diff,
                            (long long)col_diff, (long long)tolerance);
    if (std::isnan(cfg->scale) || std::isnan(cfg->pixfrac)) return ab_set_error(ctx, AB_ERR_INVALID, "scale / pixfrac is NaN");
    d->scale = std::min(std::max(cfg->scale, 1.0), 4.0);
    d->pixfrac = std::min(std::max(cfg->pixfrac, 0.1), 1.0);
    d->in_rows = min_r;
    d->in_cols = min_c;
    d->out_rows = (int64_t)std::ceil((double)min_r * d->scale);
    d->out_cols = (int64_t)std::ceil((double)min_c * d->scale);
    return AB_OK;
}

// steps 4-6 on device planes; dx_dy = n pairs as DrizzleResult.offsets reports them
int dz_device(ab_ctx *ctx, const float *const *dp, const int64_t *ld, size_t n, const double *dx_dy, const DzDims &D, const ab_drizzle_config &cfg,
              float *img, float *wgt, uint64_t *rejected) {
    *rejected = 0;
    const int64_t n_out = D.out_rows * D.out_cols;
    if (n_out == 0) return AB_OK;
    DzParams P;
    P.in_rows = (int)D.in_rows;
    P.in_cols = (int)D.in_cols;
    P.out_rows = (int)D.out_rows;
    P.out_cols = (int)D.out_cols;
    P.n_frames = (int)n;
    P.cap = std::max(2 * (int)n, 4);
    P.iters = (int)std::min<size_t>(cfg.sigma_iterations, (size_t)P.cap);  // (a round that removes nothing ends the loop: no more than cap rounds act)
    P.sigma_low = cfg.sigma_low;
    P.sigma_high = cfg.sigma_high;
    P.scale = D.scale;
    P.inv_scale = 1.0 / D.scale;
    P.half = D.pixfrac * D.scale * 0.5;
    const double sigma = std::max(P.half, 0.5);
    P.two_sigma2 = 2.0 * sigma * sigma;
    P.reach = cfg.kernel == 0 ? P.half + 0.5 : (cfg.kernel == 1 ? 7.44 * sigma : 3.0);

    const bool in_lds = P.cap <= kLdsCap;
    const dim3 tgrid(ab_div_up(D.out_cols, kTileW), 1);
    const int bands = in_lds ? ab_div_up(D.out_rows, kBandRows) : 0;
    // the long-list path: runs of `run` consecutive pixels, a multiple of the workgroup, whose columns fill at most kScratchBytes
    int64_t run = (int64_t)(kScratchBytes / ((size_t)P.cap * sizeof(float))) / kBlock * kBlock;
    run = std::max<int64_t>(run, kBlock);
    run = std::min<int64_t>(run, (n_out + kBlock - 1) / kBlock * kBlock);
    const int64_t runs = in_lds ? 0 : (n_out + run - 1) / run;
    const size_t band_parts = (size_t)tgrid.x * (size_t)(kBandRows / kTileH);
    const size_t nparts = in_lds ? band_parts * (size_t)bands : (size_t)runs * (size_t)(run / kBlock);
    const size_t off_parts = align256(n * sizeof(DzFrame));
    const size_t off_total = off_parts + align256(nparts * sizeof(unsigned long long));
    const size_t off_lists = off_total + 256;
    const size_t bytes = off_lists + (in_lds ? 0 : (size_t)run * (size_t)P.cap * sizeof(float));
    char *ws = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_DRIZZLE, bytes, (void **)&ws));
    DzFrame *frames = (DzFrame *)ws;
    unsigned long long *partials = (unsigned long long *)(ws + off_parts), *total = (unsigned long long *)(ws + off_total);
    float *lists = (float *)(ws + off_lists);
    // the frame table goes through the context's pinned buffer (it outlives an early return); the rejected total comes back through it
    void *pin = nullptr;
    AB_TRY(ab_pinned(ctx, n * sizeof(DzFrame), &pin));
    DzFrame *hf = (DzFrame *)pin;
    for (size_t i = 0; i < n; ++i) hf[i] = DzFrame{dp[i], ld[i], -dx_dy[2 * i], -dx_dy[2 * i + 1]};
    AB_HIP(ctx, hipMemcpyAsync(frames, hf, n * sizeof(DzFrame), hipMemcpyHostToDevice, ctx->stream));
    AB_HIP(ctx, hipMemsetAsync(partials, 0, nparts * sizeof(unsigned long long), ctx->stream));

    const uint64_t steps = in_lds ? (uint64_t)bands : (uint64_t)runs;
    char stage[64];
    for (uint64_t s = 0; s < steps; ++s) {
        snprintf(stage, sizeof stage, "drizzle %llu/%llu", (unsigned long long)s, (unsigned long long)steps);
        AB_TRY(ab_progress(ctx, stage, s, steps));  // (a cancel is seen here, before the next band is enqueued)
        if (in_lds) {
            const int row0 = (int)s * kBandRows;
            const int nrows = std::min<int64_t>(kBandRows, D.out_rows - row0);
            dz_launch<true>(cfg.kernel, dim3(tgrid.x, ab_div_up(nrows, kTileH)), (size_t)kBlock * P.cap * sizeof(float), ctx->stream, frames, P, row0, 0,
                            0, nullptr, img, wgt, partials + s * band_parts);
        } else {
            const int64_t p0 = (int64_t)s * run, cnt = std::min<int64_t>(run, n_out - p0);
            dz_launch<false>(cfg.kernel, dim3((unsigned)(run / kBlock)), 64, ctx->stream, frames, P, 0, p0, cnt, lists, img, wgt,
                             partials + s * (size_t)(run / kBlock));
        }
        AB_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(dz_finish_kernel, dim3(1), dim3(kFinishBlock), 0, ctx->stream, (const unsigned long long *)partials, nparts, total);
    AB_HIP(ctx, hipGetLastError());
    AB_HIP(ctx, hipMemcpyAsync(pin, total, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *rejected = *(const unsigned long long *)pin;
    return AB_OK;
}

// step 3 (drizzle.rs:281-318) on the staged frames: offsets[2 i] = dx, [2 i + 1] = dy
int dz_offsets(ab_ctx *ctx, const float *const *dp, const int64_t *ld, size_t n, const DzDims &D, const ab_drizzle_config &cfg, double *off) {
    const int threads = cfg.num_threads > 0 ? cfg.num_threads : 8;
    // align_channel_affine takes contiguous planes: a cropped frame (ld > cols) is copied once, only when the affine estimate is needed
    float *ref_c = nullptr, *tgt_c = nullptr;
    const size_t plane = (size_t)D.in_rows * (size_t)D.in_cols * sizeof(float);
    int rc = AB_OK;
    auto contiguous = [&](size_t i, float **buf, const float **out) -> int {
        if (ld[i] == D.in_cols) {
            *out = dp[i];
            return AB_OK;
        }
        if (!*buf) AB_HIP(ctx, hipMalloc((void **)buf, plane));
        AB_HIP(ctx, hipMemcpy2DAsync(*buf, (size_t)D.in_cols * sizeof(float), dp[i], (size_t)ld[i] * sizeof(float), (size_t)D.in_cols * sizeof(float),
                                     (size_t)D.in_rows, hipMemcpyDeviceToDevice, ctx->stream));
        *out = *buf;
        return AB_OK;
    };
    const float *ref = nullptr;
    char stage[64];
    for (size_t i = 1; rc == AB_OK && i < n; ++i) {
        snprintf(stage, sizeof stage, "drizzle alignment %zu/%zu", i, n - 1);
        rc = ab_progress(ctx, stage, i - 1, n - 1);
        if (rc != AB_OK) break;
        bool affine = cfg.alignment_method != 0;
        if (!affine) {
            double dx = 0.0, dy = 0.0, conf = 0.0;
            rc = ab_phase_correlate_device(ctx, dp[0], D.in_rows, D.in_cols, ld[0], dp[i], D.in_rows, D.in_cols, ld[i], &dx, &dy, &conf);
            if (rc != AB_OK) break;
            off[2 * i] = dx;
            off[2 * i + 1] = dy;
            affine = conf < 2.0;  // is_low_confidence (phase_correlation.rs:163)
        }
        if (affine) {
            const float *tgt = nullptr;
            if (!ref) rc = contiguous(0, &ref_c, &ref);
            if (rc == AB_OK) rc = contiguous(i, &tgt_c, &tgt);
            ab_affine_align_result r;
            if (rc == AB_OK) rc = ab_align_channel_affine_device(ctx, ref, tgt, D.in_rows, D.in_cols, threads, &r);
            if (rc != AB_OK) break;
            off[2 * i] = r.transform[2];      // tx (align.rs:73-80)
            off[2 * i + 1] = r.transform[5];  // ty
        }
    }
    if (ref_c || tgt_c) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ref_c) (void)hipFree(ref_c);
        if (tgt_c) (void)hipFree(tgt_c);
    }
    return rc;
}

// the body of both entry points: dx_dy_in given (ab_drizzle_frames) or derived (ab_drizzle_stack; written to dx_dy_out if wanted)
int dz_run(ab_ctx *ctx, const ab_plane *planes, size_t n, const double *dx_dy_in, const ab_drizzle_config *cfg, ab_plane_mut *out_image,
           ab_plane_mut *out_weight, double *dx_dy_out, ab_drizzle_result *res) {
    DzDims D;
    AB_TRY(dz_dims(ctx, planes, n, cfg, &D));
    AB_CHECK(ctx, out_image && res, "null argument");
    AB_CHECK(ctx, cfg->kernel >= 0 && cfg->kernel <= 2, "kernel must be 0 (Square), 1 (Gaussian) or 2 (Lanczos3)");
    AB_CHECK(ctx, D.out_rows * D.out_cols < (int64_t(1) << 31), "image too large for this build");
    AB_CHECK(ctx, out_image->rows == D.out_rows && out_image->cols == D.out_cols, "output must be %lldx%lld", (long long)D.out_rows, (long long)D.out_cols);
    const bool want_weight = out_weight && out_weight->data;
    if (want_weight) AB_CHECK(ctx, out_weight->rows == D.out_rows && out_weight->cols == D.out_cols, "weight map must be %lldx%lld", (long long)D.out_rows, (long long)D.out_cols);
    if (dx_dy_in)
        for (size_t i = 0; i < 2 * n; ++i) AB_CHECK(ctx, std::isfinite(dx_dy_in[i]), "offset %zu is not finite", i);
    for (size_t i = 0; i < n; ++i) AB_CHECK(ctx, planes[i].data || planes[i].rows * planes[i].cols == 0, "frame %zu has no data", i);
    AB_TRY(ab_progress(ctx, "drizzle", 0, 1));  // (a cancel requested before the call)
    AB_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<const float *> dp(n);
    std::vector<int64_t> ld(n);
    std::vector<double> off(2 * n, 0.0);
    Scope sc(ctx);
    for (size_t i = 0; i < n; ++i) {
        AB_TRY(sc.stage_in(&planes[i], &dp[i]));
        ld[i] = planes[i].cols;  // the crop to the minimum dims (drizzle.rs:258-272) is only a row stride
    }
    if (dx_dy_in) std::copy(dx_dy_in, dx_dy_in + 2 * n, off.begin());
    else if (cfg->align && D.in_rows > 0 && D.in_cols > 0) AB_TRY(dz_offsets(ctx, dp.data(), ld.data(), n, D, *cfg, off.data()));
    if (!dx_dy_in)
        for (size_t i = 0; i < 2 * n; ++i)
            AB_CHECK(ctx, std::isfinite(off[i]), "the alignment returned a non-finite offset for frame %zu", i / 2);
    float *image = nullptr, *weight = nullptr;
    AB_TRY(sc.stage_out(out_image, &image));
    if (want_weight) AB_TRY(sc.stage_out(out_weight, &weight));
    uint64_t rejected = 0;
    AB_TRY(dz_device(ctx, dp.data(), ld.data(), n, off.data(), D, *cfg, image, weight, &rejected));
    AB_TRY(sc.finish_outs());
    if (dx_dy_out) std::copy(off.begin(), off.end(), dx_dy_out);
    res->frame_count = n;
    res->output_scale = D.scale;
    res->in_rows = D.in_rows;
    res->in_cols = D.in_cols;
    res->out_rows = D.out_rows;
    res->out_cols = D.out_cols;
    res->rejected_pixels = rejected;
    return AB_OK;
}

}  // namespace

extern "C" {

int ab_drizzle_output_dims(const ab_plane *planes, size_t n, const ab_drizzle_config *cfg, int64_t *in_rows, int64_t *in_cols, int64_t *out_rows,
                           int64_t *out_cols) try {
    DzDims D;
    const int rc = dz_dims(nullptr, planes, n, cfg, &D);
    if (rc != AB_OK) return rc;
    if (in_rows) *in_rows = D.in_rows;
    if (in_cols) *in_cols = D.in_cols;
    if (out_rows) *out_rows = D.out_rows;
    if (out_cols) *out_cols = D.out_cols;
    return AB_OK;
} AB_CATCH_NOCTX

int ab_drizzle_frames(ab_ctx *ctx, const ab_plane *planes, size_t n, const double *offsets_dx_dy, const ab_drizzle_config *cfg,
                      ab_plane_mut *out_image, ab_plane_mut *out_weight, ab_drizzle_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, offsets_dx_dy || n == 0, "null offsets");
    return dz_run(ctx, planes, n, offsets_dx_dy, cfg, out_image, out_weight, nullptr, res);
} AB_CATCH(ctx)

int ab_drizzle_stack(ab_ctx *ctx, const ab_plane *planes, size_t n, const ab_drizzle_config *cfg, ab_plane_mut *out_image,
                     ab_plane_mut *out_weight, double *offsets_dx_dy, ab_drizzle_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    return dz_run(ctx, planes, n, nullptr, cfg, out_image, out_weight, offsets_dx_dy, res);
} AB_CATCH(ctx)

}  // extern "C"
