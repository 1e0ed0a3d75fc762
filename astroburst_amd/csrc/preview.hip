// The robust asinh preview and the grayscale / stretched byte renderers (gfx950).
//
// Replaces the per-pixel work of render_asinh_and_save (cmd/common.rs:242-261): robust_asinh_preview = asinh_normalize_simd
// (math/simd.rs:160-214) followed by render_grayscale (infra/render/grayscale.rs:10-29), and of the export command's four renderers
// (grayscale.rs:10-74), each up to the PNG encoder.
//   stats    plane_select.hip's 11/11/10 select: ONE request for the ranks m/2 - 1 (even m), m/2, low and high, which descend
//            together, then one select of |v - median| with the same validity.  No second select lives here.
//   map      elementwise, two routes from one kernel template: the reference's AVX2 route (fast_log_avx2 restated operation for
//            operation, integer steps included) over the 8-pixel chunks counted from flat index 0, and its scalar route (Taylor below
//            0.5, the f64 log above).  The AVX2 route's n % 8 remainder calls the scalar route's own function, outside the loop, so the
//            f64 log is not in that instantiation's body.
//   render   the f32 plane is never written: launch 1 recomputes the map and reduces min / max (wave shuffle -> LDS -> one partial
//            per block, no float atomics), launch 2 finishes the min / max from the partials, recomputes the map, quantises and
//            stores packed bytes.  The plain renderers are the same two launches with the identity in place of the map.
// Every kernel is a grid-stride sweep of four-pixel groups: one 16-byte load where the source allows it, one packed store (four
// bytes, four big-endian u16, four floats) aligned by the DESTINATION; the at most six pixels around the groups and the AVX2
// route's remainder are done one per lane by the first lanes of the grid.  A plane at any float-aligned address is served.
#include "entry_host.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int kOpAvx2 = AB_ASINH_ROUTE_AVX2, kOpScalar = AB_ASINH_ROUTE_SCALAR, kOpIdent = 2;

struct MapTx {
    float median, isa, low, high;  // isa = 10f32 / sigma (simd.rs:179-180)
};

// where the four-pixel groups of a sweep lie
struct Groups {
    int64_t head;   // pixels [0, head) precede the first group
    int64_t quads;  // groups: pixels [head, head + 4 * quads)
    int64_t body;   // pixels [0, body) take the route's formula; [body, n) the scalar one (body == n except on the AVX2 route)
    int64_t n;
    int in16;       // src + head is 16-byte aligned: a group is one dwordx4 load
};

// fast_log_avx2 (simd.rs:28-84): every step as written, mul and add separate (the library is built -ffp-contract=off)
__device__ __forceinline__ float fast_log(float x) {
    const uint32_t xi = __float_as_uint(x);
    float m = __uint_as_float((xi & 0x007FFFFFu) | 0x3F000000u);
    float e = (float)((int32_t)((xi & 0x7F800000u) >> 23) - 0x7E);
    if (m < 0.70710678118654752440f) {  // FRAC_1_SQRT_2
        m = m + m;
        e = e - 1.0f;
    }
    const float f = m - 1.0f;
    const float f2 = f * f;
    const float f3 = f2 * f;
    float r = 7.0376836292e-2f;
    r = r * f + -1.1514610310e-1f;
    r = r * f + 1.1676998740e-1f;
    r = r * f + -1.2420140846e-1f;
    r = r * f + 1.4249322787e-1f;
    r = r * f + -1.6668057665e-1f;
    r = r * f + 2.0000714765e-1f;
    r = r * f + -2.4999993993e-1f;
    r = r * f + 3.3333331174e-1f;
    const float log1pf = (f - 0.5f * f2) + f3 * r;
    return e * 0.69314718055994530942f + log1pf;  // LN_2
}

// one lane of normalize_chunk_avx2's vector loop (simd.rs:133-145); min_ps / max_ps return their second operand on an unordered compare
__device__ __forceinline__ float asinh_avx2(float v, const MapTx t) {
    const bool valid = v == v && v > 1e-7f;  // +inf is valid here
    const float raised = v > t.low ? v : t.low;
    const float clamped = raised < t.high ? raised : t.high;
    const float scaled = (clamped - t.median) * t.isa;
    const float a = fabsf(scaled);
    const float inner = a + sqrtf(a * a + 1.0f);
    const uint32_t bits = __float_as_uint(fast_log(inner)) | (__float_as_uint(scaled) & 0x80000000u);
    return valid ? __uint_as_float(bits) : 0.0f;
}

// the scalar loop (simd.rs:203-211 = the AVX2 route's remainder, :148-157) with fast_asinh_scalar (:9-18)
__device__ __forceinline__ float asinh_scalar(float v, const MapTx t) {
    if (!(__builtin_isfinite(v) && v > 1e-7f)) return 0.0f;
    const float clamped = v < t.low ? t.low : (v > t.high ? t.high : v);
    const float x = t.isa * (clamped - t.median);
    const float ax = fabsf(x);
    if (ax < 0.5f) {
        const float x2 = x * x;
        return x * (1.0f - x2 * (1.0f / 6.0f - x2 * 3.0f / 40.0f));
    }
    // DEFINITION (include/astroburst_hip.h): the f32 rounding of the f64 log of the f32 argument
    const float arg = ax + sqrtf(ax * ax + 1.0f);
    return (x >= 0.0f ? 1.0f : -1.0f) * (float)log((double)arg);
}

template <int OP>
__device__ __forceinline__ float value_of(float v, const MapTx t) {
    if constexpr (OP == kOpAvx2) {
        return asinh_avx2(v, t);
    } else if constexpr (OP == kOpScalar) {
        return asinh_scalar(v, t);
    } else {
        return v;
    }
}

// quad(i, a, b, c, d): the values of pixels i .. i + 3 of a group; one(i, a): a pixel outside the groups
template <int OP, class Quad, class One>
__device__ __forceinline__ void sweep(const float *src, const Groups s, const MapTx t, Quad quad, One one) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < s.quads; q += stride) {
        const int64_t i = s.head + 4 * q;
        const float4 v = s.in16 ? *reinterpret_cast<const float4 *>(src + i) : make_float4(src[i], src[i + 1], src[i + 2], src[i + 3]);
        quad(i, value_of<OP>(v.x, t), value_of<OP>(v.y, t), value_of<OP>(v.z, t), value_of<OP>(v.w, t));
    }
    // the pixels around the groups (at most 3 + 3; every pixel when the destination allows no groups), then the reference's scalar
    // remainder (at most 7, AVX2 route only): one pixel per lane, the first lanes of the grid
    const int64_t after = s.head + 4 * s.quads;
    const int64_t edge = s.head + (s.body - after);
    const int64_t loose = edge + (s.n - s.body);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        if (e < edge) {
            const int64_t i = e < s.head ? e : after + (e - s.head);
            one(i, value_of<OP>(src[i], t));
        } else {
            const int64_t i = s.body + (e - edge);
            one(i, value_of<OP == kOpAvx2 ? kOpScalar : OP>(src[i], t));
        }
    }
}

// (out may be exactly src: a lane reads its pixels before it writes them and no other lane touches them)
template <int OP>
__global__ __launch_bounds__(kBlock) void preview_map_kernel(const float *src, const Groups s, const MapTx t, float *out) {
    sweep<OP>(
        src, s, t, [&](int64_t i, float a, float b, float c, float d) { *reinterpret_cast<float4 *>(out + i) = make_float4(a, b, c, d); },
        [&](int64_t i, float a) { out[i] = a; });
}

// find_minmax_simd's scalar statement (simd.rs:263-271) of the values: part[block] = (min, max) of its finite ones
template <int OP>
__global__ __launch_bounds__(kBlock) void preview_minmax_kernel(const float *__restrict__ src, const Groups s, const MapTx t, float2 *__restrict__ part) {
    float mn = FLT_MAX, mx = -FLT_MAX;  // f32::MAX, f32::MIN
    auto take = [&](float v) {
        if (__builtin_isfinite(v)) {
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    };
    sweep<OP>(
        src, s, t,
        [&](int64_t, float a, float b, float c, float d) {
            take(a);
            take(b);
            take(c);
            take(d);
        },
        [&](int64_t, float a) { take(a); });
    block_minmax(mn, mx);
    if (threadIdx.x == 0) part[blockIdx.x] = make_float2(mn, mx);
}

// UNIT: render_stretched_* (grayscale.rs:52-74), (v.clamp(0, 1) * top) as uN, no validity test.  Otherwise render_grayscale*
// (:10-50): valid ? ((v - min) * inv).clamp(0, top) as uN : 0.  `as` truncates, saturates and sends NaN to 0.
template <int BITS, bool UNIT>
__device__ __forceinline__ uint32_t quantise(float v, float mn, float inv) {
    constexpr float top = BITS == 8 ? 255.0f : 65535.0f;
    if constexpr (UNIT) {
        const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        const float x = c * top;
        return x == x ? (uint32_t)x : 0u;
    } else {
        if (!(__builtin_isfinite(v) && v > 1e-7f)) return 0u;
        const float x = fminf(fmaxf((v - mn) * inv, 0.0f), top);  // (fmaxf drops a NaN: 0, as the cast would give)
        return (uint32_t)x;
    }
}

// 16-bit samples leave as big-endian byte pairs (write_png_l16, grayscale.rs:95)
__device__ __forceinline__ uint32_t be16(uint32_t q) { return (q >> 8) | ((q & 255u) << 8); }

template <int OP, int BITS, bool UNIT>
__global__ __launch_bounds__(kBlock) void preview_bytes_kernel(const float *__restrict__ src, const Groups s, const MapTx t,
                                                               const float2 *__restrict__ part, int parts, uint8_t *__restrict__ out,
                                                               float2 *__restrict__ range_out) {
    float mn = 0.0f, inv = 0.0f;
    if constexpr (!UNIT) {
        float lo = FLT_MAX, hi = -FLT_MAX;
        for (int p = threadIdx.x; p < parts; p += kBlock) {
            const float2 v = part[p];
            lo = fminf(lo, v.x);
            hi = fmaxf(hi, v.y);
        }
        block_minmax(lo, hi);
        if (blockIdx.x == 0 && threadIdx.x == 0) *range_out = make_float2(lo, hi);
        mn = lo;
        inv = (BITS == 8 ? 255.0f : 65535.0f) / fmaxf(hi - lo, 1e-10f);
    }
    sweep<OP>(
        src, s, t,
        [&](int64_t i, float a, float b, float c, float d) {
            const uint32_t qa = quantise<BITS, UNIT>(a, mn, inv), qb = quantise<BITS, UNIT>(b, mn, inv);
            const uint32_t qc = quantise<BITS, UNIT>(c, mn, inv), qd = quantise<BITS, UNIT>(d, mn, inv);
            if constexpr (BITS == 8) {
                *reinterpret_cast<uint32_t *>(out + i) = qa | (qb << 8) | (qc << 16) | (qd << 24);
            } else {
                *reinterpret_cast<uint2 *>(out + 2 * i) = make_uint2(be16(qa) | (be16(qb) << 16), be16(qc) | (be16(qd) << 16));
            }
        },
        [&](int64_t i, float a) {
            const uint32_t q = quantise<BITS, UNIT>(a, mn, inv);
            if constexpr (BITS == 8) {
                out[i] = (uint8_t)q;
            } else {
                out[2 * i] = (uint8_t)(q >> 8);
                out[2 * i + 1] = (uint8_t)(q & 255u);
            }
        });
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// the groups of a sweep over n pixels of `src` under `op`; `align_addr` / `bytes_per_pixel`: the address whose four-pixel stores
// (or, for a sweep that only reads, loads) must be aligned
Groups make_span(const float *src, uintptr_t align_addr, int bytes_per_pixel, int64_t n, int op) {
    Groups s;
    s.n = n;
    s.body = op == kOpAvx2 ? 8 * (n / 8) : n;
    const uintptr_t group = (uintptr_t)(4 * bytes_per_pixel);
    if (align_addr % (uintptr_t)bytes_per_pixel != 0) {
        s.head = s.body;  // (a destination that is not even pixel-aligned: no groups, every pixel on its own)
    } else {
        s.head = std::min<int64_t>(s.body, (int64_t)(((group - align_addr % group) % group) / (uintptr_t)bytes_per_pixel));
    }
    s.quads = (s.body - s.head) / 4;
    s.in16 = ((uintptr_t)(src + s.head) & 15u) == 0 ? 1 : 0;
    return s;
}

// workgroups for a sweep: enough for its groups (or, when it has none, for its pixels), at most per_cu per compute unit
int grid_for(const ab_ctx *ctx, const Groups &s, int per_cu) {
    const int64_t lanes = std::max<int64_t>(s.quads, s.n - 4 * s.quads);
    return ab_stream_grid(ctx, lanes, kBlock, per_cu);
}

int plane_check(ab_ctx *ctx, const ab_plane *img) {
    AB_CHECK(ctx, img && img->data, "null image");
    AB_CHECK(ctx, img->rows > 0 && img->cols > 0, "the image has a zero dimension (%lld x %lld)", (long long)img->rows, (long long)img->cols);
    AB_CHECK(ctx, img->rows <= (int64_t(1) << 40) / img->cols, "the image holds more than 2^40 pixels");
    AB_CHECK(ctx, ((uintptr_t)img->data & 3u) == 0, "the image is not float-aligned");
    return AB_OK;
}

int route_check(ab_ctx *ctx, int32_t route) {
    AB_CHECK(ctx, route == AB_ASINH_ROUTE_AVX2 || route == AB_ASINH_ROUTE_SCALAR, "unknown asinh route %d", (int)route);
    return AB_OK;
}

int out_plane_check(ab_ctx *ctx, const ab_plane *img, const ab_plane_mut *out) {
    AB_CHECK(ctx, out && out->data, "null output plane");
    AB_CHECK(ctx, out->rows == img->rows && out->cols == img->cols, "the output plane must be %lld x %lld (got %lld x %lld)", (long long)img->rows,
             (long long)img->cols, (long long)out->rows, (long long)out->cols);
    AB_CHECK(ctx, ((uintptr_t)out->data & 3u) == 0, "the output plane is not float-aligned");
    if (out->data != img->data && (out->on_device != 0) == (img->on_device != 0)) {
        const uintptr_t a = (uintptr_t)img->data, b = (uintptr_t)out->data, len = (uintptr_t)img->rows * (uintptr_t)img->cols * sizeof(float);
        AB_CHECK(ctx, a + len <= b || b + len <= a, "the output plane must be the image itself or not overlap it");
    }
    return AB_OK;
}

int stats_tx(ab_ctx *ctx, const ab_asinh_stats *st, MapTx *t) {
    AB_CHECK(ctx, st, "null statistics");
    AB_CHECK(ctx, !std::isnan(st->median) && !std::isnan(st->sigma) && !std::isnan(st->low) && !std::isnan(st->high), "a statistic is NaN");
    AB_CHECK(ctx, st->low <= st->high, "low (%g) must not exceed high (%g)", (double)st->low, (double)st->high);
    t->median = st->median;
    t->isa = 10.0f / st->sigma;
    t->low = st->low;
    t->high = st->high;
    return AB_OK;
}

// simd.rs:163-180 of n device-resident pixels
int stats_device(ab_ctx *ctx, const float *d, int64_t n, ab_asinh_stats *out) {
    *out = ab_asinh_stats{0.0f, 0.0f, 0.0f, 0.0f, 0};
    ab_plane_sel s;
    s.data = d;
    s.n = n;
    s.min_valid = 1e-7f;  // is_valid (simd.rs:20-23)
    uint64_t m = 0;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    AB_TRY(ab_plane_select_ranks(
        ctx, s, 4,
        [&](uint64_t cnt, uint64_t *ranks) {
            ranks[0] = cnt / 2;
            ranks[1] = (uint64_t)((double)cnt * 0.01);
            ranks[2] = std::min<uint64_t>((uint64_t)((double)cnt * 0.999), cnt - 1);
            if (cnt % 2 != 0) return 3;
            ranks[3] = cnt / 2 - 1;
            return 4;
        },
        &m, v));
    if (m == 0) return AB_OK;
    const float median = m % 2 == 0 ? (v[3] + v[0]) / 2.0f : v[0];  // median_f32_mut (math/median.rs:46-63)
    s.use_dev = 1;
    s.center = median;
    float mad = 0.0f;
    AB_TRY(ab_plane_median_f32(ctx, s, &mad, nullptr));
    out->median = median;
    out->sigma = std::fmax(mad * 1.4826f, 1e-10f);  // (MAD_TO_SIGMA as f32, f32::max)
    out->low = v[1];
    out->high = v[2];
    out->valid_count = m;
    return AB_OK;
}

int map_launch(ab_ctx *ctx, const float *d, int64_t n, const MapTx t, int route, float *out) {
    const Groups s = make_span(d, (uintptr_t)out, (int)sizeof(float), n, route);
    const int grid = grid_for(ctx, s, 8);
    if (route == kOpAvx2) {
        hipLaunchKernelGGL(preview_map_kernel<kOpAvx2>, dim3(grid), dim3(kBlock), 0, ctx->stream, d, s, t, out);
    } else {
        hipLaunchKernelGGL(preview_map_kernel<kOpScalar>, dim3(grid), dim3(kBlock), 0, ctx->stream, d, s, t, out);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// statistics + map (or, with no valid pixel, the copy) of a staged image into a staged output
int preview_device(ab_ctx *ctx, const float *d, int64_t n, int route, float *out, ab_asinh_stats *st) {
    AB_TRY(stats_device(ctx, d, n, st));
    if (st->valid_count == 0) {
        if (out != d) AB_HIP(ctx, hipMemcpyAsync(out, d, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        return AB_OK;
    }
    MapTx t;
    AB_TRY(stats_tx(ctx, st, &t));
    return map_launch(ctx, d, n, t, route, out);
}

template <int OP>
void launch_minmax(ab_ctx *ctx, int grid, const float *d, const Groups s, const MapTx t, float2 *part) {
    hipLaunchKernelGGL(preview_minmax_kernel<OP>, dim3(grid), dim3(kBlock), 0, ctx->stream, d, s, t, part);
}

template <int OP, bool UNIT>
void launch_bytes(ab_ctx *ctx, int grid, int bits, const float *d, const Groups s, const MapTx t, const float2 *part, int parts, uint8_t *out,
                  float2 *range) {
    if (bits == 8) {
        hipLaunchKernelGGL((preview_bytes_kernel<OP, 8, UNIT>), dim3(grid), dim3(kBlock), 0, ctx->stream, d, s, t, part, parts, out, range);
    } else {
        hipLaunchKernelGGL((preview_bytes_kernel<OP, 16, UNIT>), dim3(grid), dim3(kBlock), 0, ctx->stream, d, s, t, part, parts, out, range);
    }
}

// The values of `op` over the n pixels at d -> bits / 8 bytes per pixel at out (host or device).  unit: the stretched renderers (no
// range pass).  range_host (nullable, !unit): receives (min, max); reading it back synchronises.  zero: every byte is 0 (a preview
// without a valid pixel), nothing is launched.
int bytes_device(ab_ctx *ctx, const float *d, int64_t n, int op, const MapTx t, int bits, bool unit, bool zero, void *out, int32_t out_on_device,
                 float *range_host) {
    const size_t nbytes = (size_t)n * (size_t)(bits / 8);
    if (zero) {
        if (out_on_device) {
            AB_HIP(ctx, hipMemsetAsync(out, 0, nbytes, ctx->stream));
        } else {
            memset(out, 0, nbytes);
        }
        return AB_OK;
    }
    // scratch: the final (min, max) | the partials | (host output) the bytes
    const Groups rs = make_span(d, (uintptr_t)d, (int)sizeof(float), n, op);
    const int parts = grid_for(ctx, rs, 4);
    const size_t head = 256 + (((size_t)parts * sizeof(float2) + 255) & ~(size_t)255);
    char *scratch = nullptr;
    AB_TRY(ab_scratch(ctx, head + (out_on_device ? 0 : nbytes), (void **)&scratch));
    float2 *range = (float2 *)scratch, *part = (float2 *)(scratch + 256);
    uint8_t *bytes_dev = out_on_device ? (uint8_t *)out : (uint8_t *)(scratch + head);
    if (!unit) {
        if (op == kOpAvx2) {
            launch_minmax<kOpAvx2>(ctx, parts, d, rs, t, part);
        } else if (op == kOpScalar) {
            launch_minmax<kOpScalar>(ctx, parts, d, rs, t, part);
        } else {
            launch_minmax<kOpIdent>(ctx, parts, d, rs, t, part);
        }
        AB_HIP(ctx, hipGetLastError());
    }
    const Groups ws = make_span(d, (uintptr_t)bytes_dev, bits / 8, n, op);
    const int grid = grid_for(ctx, ws, 8);
    if (unit) {
        launch_bytes<kOpIdent, true>(ctx, grid, bits, d, ws, t, part, 0, bytes_dev, range);
    } else if (op == kOpAvx2) {
        launch_bytes<kOpAvx2, false>(ctx, grid, bits, d, ws, t, part, parts, bytes_dev, range);
    } else if (op == kOpScalar) {
        launch_bytes<kOpScalar, false>(ctx, grid, bits, d, ws, t, part, parts, bytes_dev, range);
    } else {
        launch_bytes<kOpIdent, false>(ctx, grid, bits, d, ws, t, part, parts, bytes_dev, range);
    }
    AB_HIP(ctx, hipGetLastError());
    if (!out_on_device) AB_HIP(ctx, hipMemcpyAsync(out, bytes_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    if (range_host) AB_HIP(ctx, hipMemcpyAsync(range_host, range, sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    if (!out_on_device || range_host) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AB_OK;
}

int bits_check(ab_ctx *ctx, int32_t bits) {
    AB_CHECK(ctx, bits == 8 || bits == 16, "bits must be 8 or 16 (got %d)", (int)bits);
    return AB_OK;
}

int render_plain(ab_ctx *ctx, const ab_plane *img, int32_t bits, bool unit, void *out, int32_t out_on_device, float *min_out, float *max_out) {
    AB_TRY(plane_check(ctx, img));
    AB_TRY(bits_check(ctx, bits));
    AB_CHECK(ctx, out, "null output");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *in = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    float range[2] = {0.0f, 0.0f};
    const bool want = !unit && (min_out || max_out);
    AB_TRY(bytes_device(ctx, in, img->rows * img->cols, kOpIdent, MapTx{0.0f, 0.0f, 0.0f, 0.0f}, (int)bits, unit, false, out, out_on_device,
                        want ? range : nullptr));
    if (want) {
        if (min_out) *min_out = range[0];
        if (max_out) *max_out = range[1];
    }
    return AB_OK;
}

}  // namespace

extern "C" {

int ab_asinh_preview_stats(ab_ctx *ctx, const ab_plane *img, ab_asinh_stats *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img));
    AB_CHECK(ctx, out, "null statistics");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *in = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    return stats_device(ctx, in, img->rows * img->cols, out);
} AB_CATCH(ctx)

int ab_asinh_normalize_with_stats(ab_ctx *ctx, const ab_plane *img, const ab_asinh_stats *stats, int32_t route, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img));
    AB_TRY(route_check(ctx, route));
    AB_TRY(out_plane_check(ctx, img, out));
    MapTx t;
    AB_TRY(stats_tx(ctx, stats, &t));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *in = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    AB_TRY(sc.stage_out(out, &o));
    const int64_t n = img->rows * img->cols;
    if (stats->valid_count == 0) {  // asinh_normalize_simd returns data.clone() (simd.rs:165-167)
        const hipError_t e = o != in ? hipMemcpyAsync(o, in, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
        if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "the copy of the image failed: %s", hipGetErrorString(e));
    } else {
        AB_TRY(map_launch(ctx, in, n, t, (int)route, o));
    }
    return sc.finish_outs();
} AB_CATCH(ctx)

int ab_robust_asinh_preview(ab_ctx *ctx, const ab_plane *img, int32_t route, ab_plane_mut *out, ab_asinh_stats *stats_out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img));
    AB_TRY(route_check(ctx, route));
    AB_TRY(out_plane_check(ctx, img, out));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *in = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    AB_TRY(sc.stage_out(out, &o));
    ab_asinh_stats st;
    AB_TRY(preview_device(ctx, in, img->rows * img->cols, (int)route, o, &st));
    AB_TRY(sc.finish_outs());
    if (stats_out) *stats_out = st;
    return AB_OK;
} AB_CATCH(ctx)

int ab_render_asinh_preview(ab_ctx *ctx, const ab_plane *img, int32_t route, uint8_t *out_u8, int32_t out_on_device, ab_asinh_stats *stats_out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img));
    AB_TRY(route_check(ctx, route));
    AB_CHECK(ctx, out_u8, "null output");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *in = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    const int64_t n = img->rows * img->cols;
    ab_asinh_stats st;
    AB_TRY(stats_device(ctx, in, n, &st));
    MapTx t{0.0f, 0.0f, 0.0f, 0.0f};
    if (st.valid_count > 0) AB_TRY(stats_tx(ctx, &st, &t));
    // (no valid pixel: the preview is the image itself, and render_grayscale sends every invalid pixel to 0)
    AB_TRY(bytes_device(ctx, in, n, (int)route, t, 8, false, st.valid_count == 0, out_u8, out_on_device, nullptr));
    if (stats_out) *stats_out = st;
    return AB_OK;
} AB_CATCH(ctx)

int ab_render_grayscale(ab_ctx *ctx, const ab_plane *img, int32_t bits, void *out, int32_t out_on_device, float *min_out, float *max_out) try {
    if (!ctx) return AB_ERR_INVALID;
    return render_plain(ctx, img, bits, false, out, out_on_device, min_out, max_out);
} AB_CATCH(ctx)

int ab_render_stretched(ab_ctx *ctx, const ab_plane *img, int32_t bits, void *out, int32_t out_on_device) try {
    if (!ctx) return AB_ERR_INVALID;
    return render_plain(ctx, img, bits, true, out, out_on_device, nullptr, nullptr);
} AB_CATCH(ctx)

}  // extern "C"
