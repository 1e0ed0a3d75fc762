// Spectral (IFU) cubes (gfx950): collapse along z, global robust statistics, asinh normalisation, frame export, spectrum extraction.
//
// Replaces the per-voxel work of core/cube/eager.rs and core/cube/lazy.rs (process_cube_cmd / process_cube_lazy_cmd).  The cube is
// deep and narrow -- 1 000 .. 4 000 planes of 40^2 .. 320^2 pixels in one [z][y][x] block -- and its values are signed, which none
// of the stack / plane kernels of this library serves:
//   mean    one lane per pixel walks its column in ascending z (the reference's f64 additions, in its order: bit for bit); the
//           loads of kMeanAhead planes are issued ahead of the dependent adds.  A column is never split across lanes.
//   median  a workgroup owns 64 adjacent pixels (lane = pixel: every load is one coalesced 256-byte row segment), its waves split z,
//           and a radix select runs along z on the order-preserving key of the bit pattern: 8-bit digits, four passes, an LDS
//           histogram laid out [bin][pixel] (a wave's 64 lanes hit 64 consecutive words: no bank conflicts; waves meet through LDS
//           integer atomics).  The count comes out of pass 0.  Small planes take more waves per workgroup, so a 50^2 cube still
//           spreads over the chip.
//   stats   plane_select.hip's 11/11/10 select in its cube form (signed keys, the two validity rules, a frame stride): three
//           ranks descending together, then the select of |v - median|.
//   frames  normalise -> per-frame min / max -> bytes in two launches for all frames; the asinh is evaluated in f64 (the result is
//           DEFINED as the f32 rounding of the f64 asinh, include/astroburst_hip.h) and recomputed instead of stored.
// No float atomics anywhere: the min / max go through per-block partials.
#include "entry_host.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMeanAhead = 8;    // planes whose loads are in flight ahead of the f64 chain
constexpr int kMedPix = 64;      // pixels of a median workgroup = lanes of a wave
constexpr int kMedBins = 256;    // 8-bit digits
constexpr int kMedMaxWaves = 16;
constexpr int kMedAhead = 4;     // loads in flight per wave in a histogram pass
constexpr int kMaxPartials = 64;  // min / max partials per exported frame

__device__ __forceinline__ bool cube_valid(float v, int rule) {
    return __builtin_isfinite(v) && (rule == AB_CUBE_VALID_NONZERO ? v != 0.0f : v > 1e-7f);
}

// ---- mean ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cube_mean_kernel(const float *__restrict__ cube, int64_t depth, int64_t plane, int rule,
                                                       float *__restrict__ out) {
    const int64_t px = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (px >= plane) return;
    const float *col = cube + px;
    double sum = 0.0;
    uint32_t cnt = 0;
    int64_t z = 0;
    for (; z + kMeanAhead <= depth; z += kMeanAhead) {
        float v[kMeanAhead];
#pragma unroll
        for (int k = 0; k < kMeanAhead; ++k) v[k] = col[(z + k) * plane];
#pragma unroll
        for (int k = 0; k < kMeanAhead; ++k)
            if (cube_valid(v[k], rule)) {
                sum += (double)v[k];
                ++cnt;
            }
    }
    for (; z < depth; ++z) {
        const float v = col[z * plane];
        if (cube_valid(v, rule)) {
            sum += (double)v;
            ++cnt;
        }
    }
    out[px] = cnt > 0 ? (float)(sum / (double)cnt) : 0.0f;
}

// ---- median -------------------------------------------------------------------------------------------------------------------
// blockDim.x = 64 * waves.  hist[bin][pixel]; sel[0][pixel] = the key prefix found so far, sel[1][pixel] = the rank within it.
__global__ __launch_bounds__(kMedPix *kMedMaxWaves) void cube_median_kernel(const float *__restrict__ cube, int64_t depth, int64_t plane,
                                                                            int rule, float *__restrict__ out) {
    __shared__ unsigned int hist[kMedBins * kMedPix];
    __shared__ unsigned int sel[2][kMedPix];
    const int lane = threadIdx.x & (kMedPix - 1);
    const int wave = threadIdx.x / kMedPix;
    const int waves = blockDim.x / kMedPix;
    const int64_t px = (int64_t)blockIdx.x * kMedPix + lane;
    const bool live = px < plane;
    const float *col = cube + (live ? px : 0);
    uint32_t prefix = 0, rank = 0;
    bool empty = false;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = threadIdx.x; i < kMedBins * kMedPix; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        if (live && !empty) {
            for (int64_t z0 = wave; z0 < depth; z0 += (int64_t)waves * kMedAhead) {
                float v[kMedAhead];
#pragma unroll
                for (int k = 0; k < kMedAhead; ++k) {
                    const int64_t z = z0 + (int64_t)k * waves;
                    v[k] = z < depth ? col[z * plane] : __builtin_nanf("");  // (a NaN is invalid under both rules)
                }
#pragma unroll
                for (int k = 0; k < kMedAhead; ++k) {
                    if (!cube_valid(v[k], rule)) continue;
                    const uint32_t b = __float_as_uint(v[k]);
                    const uint32_t key = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
                    // pass 0 takes every valid sample; later passes those that share the digits found so far
                    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[((key >> shift) & 255u) * kMedPix + lane], 1u);
                }
            }
        }
        __syncthreads();
        if (wave == 0) {
            uint32_t r = rank;
            if (pass == 0) {
                uint32_t total = 0;
                for (int b = 0; b < kMedBins; ++b) total += hist[b * kMedPix + lane];
                r = total / 2;  // vals[len / 2]
                if (total == 0) r = 0xFFFFFFFFu;
            }
            uint32_t bin = 0, cum = 0;
            if (r != 0xFFFFFFFFu) {
                bool found = false;
                for (int b = 0; b < kMedBins; ++b) {
                    const uint32_t h = hist[b * kMedPix + lane];
                    if (!found && cum + h > r) {
                        found = true;
                        bin = (uint32_t)b;
                        r -= cum;
                    }
                    if (!found) cum += h;
                }
            }
            sel[0][lane] = r == 0xFFFFFFFFu ? 0u : ((prefix << 8) | bin);
            sel[1][lane] = r;
        }
        __syncthreads();
        prefix = sel[0][lane];
        rank = sel[1][lane];
        empty = rank == 0xFFFFFFFFu;
        // (the next pass's clearing of hist is ordered after these reads of sel by its own barrier; sel is rewritten only after the
        // barrier that follows the histogram loop)
    }
    if (live && wave == 0) {
        const uint32_t bits = (prefix & 0x80000000u) ? (prefix ^ 0x80000000u) : ~prefix;
        out[px] = empty ? 0.0f : __uint_as_float(bits);
    }
}

// ---- normalise / export -------------------------------------------------------------------------------------------------------
struct NormTx {
    float scale, median, low, high;  // scale = 10f32 / sigma
};

__device__ __forceinline__ float cube_normalize(float v, const NormTx t) {
    if (!__builtin_isfinite(v)) return 0.0f;
    const float clamped = v < t.low ? t.low : (v > t.high ? t.high : v);  // f32::clamp(low, high), the sign of a zero included
    const float scaled = t.scale * (clamped - t.median);
    return (float)asinh((double)scaled);
}

__global__ __launch_bounds__(kBlock) void cube_normalize_kernel(const float *__restrict__ in, int64_t n, const NormTx t, float *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = cube_normalize(in[i], t);
}

// grid (parts, min(frames, 65535)): partial[(frame * parts + blockIdx.x) * 2 + {0, 1}] = min, max of the block's share of the frame
__global__ __launch_bounds__(kBlock) void cube_frame_minmax_kernel(const float *__restrict__ cube, int64_t plane, int64_t step, int64_t frames,
                                                                   const NormTx t, float *__restrict__ partial) {
    const int parts = gridDim.x;
    for (int64_t f = blockIdx.y; f < frames; f += gridDim.y) {
        const float *frame = cube + f * step * plane;
        float mn = 3.402823466e+38f, mx = -3.402823466e+38f;  // f32::MAX, f32::MIN (simd.rs:263-264)
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < plane; i += (int64_t)parts * kBlock) {
            const float v = cube_normalize(frame[i], t);
            if (__builtin_isfinite(v)) {
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
        }
        block_minmax(mn, mx);
        if (threadIdx.x == 0) {
            partial[(f * parts + blockIdx.x) * 2] = mn;
            partial[(f * parts + blockIdx.x) * 2 + 1] = mx;
        }
    }
}

// grid (blocks along the frame, min(frames, 65535)); `parts` = the grid.x of the min / max launch
__global__ __launch_bounds__(kBlock) void cube_frame_u8_kernel(const float *__restrict__ cube, int64_t plane, int64_t step, int64_t frames,
                                                               const NormTx t, const float *__restrict__ partial, int parts,
                                                               uint8_t *__restrict__ out) {
    for (int64_t f = blockIdx.y; f < frames; f += gridDim.y) {
        float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
        for (int p = 0; p < parts; ++p) {  // (uniform, <= kMaxPartials pairs: scalar loads)
            mn = fminf(mn, partial[(f * parts + p) * 2]);
            mx = fmaxf(mx, partial[(f * parts + p) * 2 + 1]);
        }
        const float range = fmaxf(mx - mn, 1e-10f);
        const float inv = 255.0f / range;
        const float *frame = cube + f * step * plane;
        uint8_t *dst = out + f * plane;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < plane; i += (int64_t)gridDim.x * kBlock) {
            const float v = cube_normalize(frame[i], t);
            uint8_t b = 0;
            if (__builtin_isfinite(v) && v > 1e-7f) {
                const float s = fminf(fmaxf((v - mn) * inv, 0.0f), 255.0f);
                b = (uint8_t)(int)s;  // `as u8` of a value in [0, 255]: truncation
            }
            dst[i] = b;
        }
    }
}

__global__ __launch_bounds__(kBlock) void cube_spectrum_kernel(const float *__restrict__ cube, int64_t depth, int64_t plane, int64_t at,
                                                               float *__restrict__ out) {
    const int64_t z = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (z < depth) out[z] = cube[z * plane + at];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int cube_check(ab_ctx *ctx, const ab_cube *cube) {
    AB_CHECK(ctx, cube && cube->data, "null cube");
    AB_CHECK(ctx, cube->depth > 0 && cube->rows > 0 && cube->cols > 0, "the cube has a zero dimension (%lld x %lld x %lld)", (long long)cube->depth,
             (long long)cube->rows, (long long)cube->cols);
    AB_CHECK(ctx, cube->rows <= (int64_t(1) << 40) / cube->cols && cube->depth <= (int64_t(1) << 40) / (cube->rows * cube->cols),
             "the cube holds more than 2^40 voxels");
    // (per-pixel counts and ranks are u32, as the reference's `count: u32` is, with 0xFFFFFFFF for "no valid sample")
    AB_CHECK(ctx, cube->depth < (int64_t(1) << 32), "the cube is deeper than 2^32 - 1 planes");
    return AB_OK;
}

int rule_check(ab_ctx *ctx, int32_t rule) {
    AB_CHECK(ctx, rule == AB_CUBE_VALID_NONZERO || rule == AB_CUBE_VALID_ABOVE_PADDING, "unknown validity rule %d", (int)rule);
    return AB_OK;
}

// the cube on the device: in place, or uploaded into the context's cube workspace (exhaustion is AB_ERR_NOMEM)
int cube_stage(ab_ctx *ctx, const ab_cube *cube, const float **dptr) {
    if (cube->on_device) {
        *dptr = cube->data;
        return AB_OK;
    }
    const size_t bytes = (size_t)cube->depth * (size_t)cube->rows * (size_t)cube->cols * sizeof(float);
    void *ws = nullptr;
    AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_CUBE, bytes, &ws));
    AB_HIP(ctx, hipMemcpyAsync(ws, cube->data, bytes, hipMemcpyHostToDevice, ctx->stream));
    *dptr = (const float *)ws;
    return AB_OK;
}

int out_check(ab_ctx *ctx, const ab_cube *cube, const ab_plane_mut *out) {
    AB_CHECK(ctx, out && out->data, "null output plane");
    AB_CHECK(ctx, out->rows == cube->rows && out->cols == cube->cols, "the output plane must be %lld x %lld (got %lld x %lld)", (long long)cube->rows,
             (long long)cube->cols, (long long)out->rows, (long long)out->cols);
    return AB_OK;
}

int stats_tx(ab_ctx *ctx, const ab_cube_stats *g, NormTx *t) {
    AB_CHECK(ctx, g, "null statistics");
    AB_CHECK(ctx, !std::isnan(g->median) && !std::isnan(g->sigma) && !std::isnan(g->low) && !std::isnan(g->high), "a statistic is NaN");
    AB_CHECK(ctx, g->low <= g->high, "low (%g) must not exceed high (%g)", (double)g->low, (double)g->high);
    t->scale = 10.0f / g->sigma;  // alpha / sigma in f32 (eager.rs:211-212)
    t->median = g->median;
    t->low = g->low;
    t->high = g->high;
    return AB_OK;
}

int collapse(ab_ctx *ctx, const ab_cube *cube, int32_t rule, ab_plane_mut *out, bool median) {
    AB_TRY(cube_check(ctx, cube));
    AB_TRY(rule_check(ctx, rule));
    AB_TRY(out_check(ctx, cube, out));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    const float *d = nullptr;
    AB_TRY(cube_stage(ctx, cube, &d));
    Scope sc(ctx);
    float *o = nullptr;
    AB_TRY(sc.stage_out(out, &o));
    const int64_t plane = cube->rows * cube->cols;
    const int64_t groups = (plane + 63) / 64;
    if (!median) {
        hipLaunchKernelGGL(cube_mean_kernel, dim3((unsigned)groups), dim3(64), 0, ctx->stream, d, cube->depth, plane, (int)rule, o);
    } else {
        // waves per workgroup: as many as keep the chip covered when the plane is small, never more than the column can feed
        const int64_t cus = ctx->cu_count > 0 ? ctx->cu_count : 256;
        int waves = groups >= 4 * cus ? 4 : (groups >= 2 * cus ? 8 : kMedMaxWaves);
        while (waves > 1 && (int64_t)waves * kMedAhead > cube->depth) waves /= 2;
        hipLaunchKernelGGL(cube_median_kernel, dim3((unsigned)groups), dim3(kMedPix * waves), 0, ctx->stream, d, cube->depth, plane, (int)rule, o);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "cube collapse launch failed: %s", hipGetErrorString(e));
    return sc.finish_outs();
}

}  // namespace

extern "C" {

int ab_cube_collapse_mean(ab_ctx *ctx, const ab_cube *cube, int32_t rule, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    return collapse(ctx, cube, rule, out, false);
} AB_CATCH(ctx)

int ab_cube_collapse_median(ab_ctx *ctx, const ab_cube *cube, int32_t rule, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    return collapse(ctx, cube, rule, out, true);
} AB_CATCH(ctx)

uint64_t ab_cube_streaming_step(int64_t depth) try {
    if (depth < 1) return 1;
    const int64_t s = std::min<int64_t>(32, depth);  // sample_frames (lazy.rs:334)
    return (uint64_t)(depth > s ? depth / s : 1);
} AB_CATCH_NOCTX_VALUE(1)

int ab_cube_global_stats(ab_ctx *ctx, const ab_cube *cube, int32_t rule, int64_t frame_step, ab_cube_stats *stats, uint64_t *count) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(cube_check(ctx, cube));
    AB_TRY(rule_check(ctx, rule));
    AB_CHECK(ctx, stats, "null statistics");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    const float *d = nullptr;
    AB_TRY(cube_stage(ctx, cube, &d));
    const int64_t step = std::max<int64_t>(1, frame_step);
    const int64_t frames = (cube->depth + step - 1) / step;
    ab_plane_sel s;
    s.data = d;
    s.frame_len = cube->rows * cube->cols;
    s.frame_step = step;
    s.n = frames * s.frame_len;
    s.cube_rule = rule;
    uint64_t n = 0;
    float v[3] = {0.0f, 0.0f, 0.0f};
    // (every histogram pass of the cube's form looks at the cancel flag first: plane_select.hip, run_pass)
    AB_TRY(ab_plane_select_ranks(
        ctx, s, 3,
        [&](uint64_t cnt, uint64_t *ranks) {
            ranks[0] = cnt / 2;
            ranks[1] = (uint64_t)((double)cnt * 0.01);
            ranks[2] = std::min<uint64_t>((uint64_t)((double)cnt * 0.999), cnt - 1);
            return 3;
        },
        &n, v));
    if (count) *count = n;
    if (n == 0) {
        *stats = ab_cube_stats{0.0f, 1.0f, 0.0f, 1.0f};
        return AB_OK;
    }
    s.use_dev = 1;
    s.center = v[0];
    uint64_t n_dev = 0;
    float mad = 0.0f;
    AB_TRY(ab_plane_select_ranks(
        ctx, s, 1,
        [&](uint64_t cnt, uint64_t *ranks) {
            ranks[0] = cnt / 2;
            return 1;
        },
        &n_dev, &mad));
    stats->median = v[0];
    stats->sigma = std::fmax(mad * 1.4826f, 1e-10f);  // (MAD_TO_SIGMA as f32, f32::max)
    stats->low = v[1];
    stats->high = v[2];
    return AB_OK;
} AB_CATCH(ctx)

int ab_cube_normalize_frame(ab_ctx *ctx, const ab_plane *img, const ab_cube_stats *stats, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, img && img->data && out && out->data, "null argument");
    AB_CHECK(ctx, img->rows > 0 && img->cols > 0, "the frame is empty");
    AB_CHECK(ctx, out->rows == img->rows && out->cols == img->cols, "the output plane must be %lld x %lld (got %lld x %lld)", (long long)img->rows,
             (long long)img->cols, (long long)out->rows, (long long)out->cols);
    NormTx t;
    AB_TRY(stats_tx(ctx, stats, &t));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *in = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    AB_TRY(sc.stage_out(out, &o));
    const int64_t n = img->rows * img->cols;
    hipLaunchKernelGGL(cube_normalize_kernel, dim3(ab_stream_grid(ctx, n, kBlock, 16)), dim3(kBlock), 0, ctx->stream, in, n, t, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "cube_normalize_kernel launch failed: %s", hipGetErrorString(e));
    return sc.finish_outs();
} AB_CATCH(ctx)

int ab_cube_export_frames(ab_ctx *ctx, const ab_cube *cube, const ab_cube_stats *stats, int64_t frame_step, uint8_t *out_u8, int32_t out_on_device,
                          int64_t *frame_count) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(cube_check(ctx, cube));
    AB_CHECK(ctx, out_u8, "null output");
    NormTx t;
    AB_TRY(stats_tx(ctx, stats, &t));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    const int64_t step = std::max<int64_t>(1, frame_step);
    const int64_t frames = (cube->depth + step - 1) / step;
    const int64_t plane = cube->rows * cube->cols;
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxPartials, (plane + 4 * kBlock - 1) / (4 * kBlock)));
    // the partials and (host output) the bytes, in the context's scratch arena
    const size_t head = ((size_t)frames * (size_t)parts * 2 * sizeof(float) + 255) & ~(size_t)255;
    const size_t nbytes = (size_t)frames * (size_t)plane;
    char *scratch = nullptr;
    AB_TRY(ab_scratch(ctx, head + (out_on_device ? 0 : nbytes), (void **)&scratch));
    const float *d = nullptr;
    AB_TRY(cube_stage(ctx, cube, &d));
    float *partial = (float *)scratch;
    uint8_t *bytes_dev = out_on_device ? out_u8 : (uint8_t *)(scratch + head);
    const unsigned gy = (unsigned)std::min<int64_t>(frames, 65535);
    hipLaunchKernelGGL(cube_frame_minmax_kernel, dim3(parts, gy), dim3(kBlock), 0, ctx->stream, d, plane, step, frames, t, partial);
    AB_HIP(ctx, hipGetLastError());
    AB_TRY(ab_cancel_point(ctx));
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(256, (plane + 4 * kBlock - 1) / (4 * kBlock)));
    hipLaunchKernelGGL(cube_frame_u8_kernel, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d, plane, step, frames, t, (const float *)partial, parts, bytes_dev);
    AB_HIP(ctx, hipGetLastError());
    if (!out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_u8, bytes_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (frame_count) *frame_count = frames;
    return AB_OK;
} AB_CATCH(ctx)

int ab_cube_extract_spectrum(ab_ctx *ctx, const ab_cube *cube, int64_t y, int64_t x, float *out, int32_t out_on_device) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(cube_check(ctx, cube));
    AB_CHECK(ctx, out, "null output");
    AB_CHECK(ctx, y >= 0 && x >= 0 && y < cube->rows && x < cube->cols, "Pixel (%lld, %lld) out of bounds", (long long)y, (long long)x);
    AB_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t plane = cube->rows * cube->cols, at = y * cube->cols + x;
    if (!cube->on_device) {  // a host cube is read where it lies: one value per plane is no reason to upload it
        if (!out_on_device) {
            for (int64_t z = 0; z < cube->depth; ++z) out[z] = cube->data[z * plane + at];
            return AB_OK;
        }
        void *pin = nullptr;
        AB_TRY(ab_pinned(ctx, (size_t)cube->depth * sizeof(float), &pin));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier call's read-back may still be using the pinned buffer)
        for (int64_t z = 0; z < cube->depth; ++z) ((float *)pin)[z] = cube->data[z * plane + at];
        AB_HIP(ctx, hipMemcpyAsync(out, pin, (size_t)cube->depth * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return AB_OK;
    }
    float *dst = out;
    if (!out_on_device) AB_TRY(ab_scratch(ctx, (size_t)cube->depth * sizeof(float), (void **)&dst));
    hipLaunchKernelGGL(cube_spectrum_kernel, dim3((unsigned)((cube->depth + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, cube->data, cube->depth,
                       plane, at, dst);
    AB_HIP(ctx, hipGetLastError());
    if (!out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out, dst, (size_t)cube->depth * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
