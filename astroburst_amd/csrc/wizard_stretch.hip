// The compose wizard's stretch step on gfx950: apply_arcsinh_stretch_cmd, arcsinh_stretch_composite_cmd and
// masked_stretch_composite_cmd (cmd/processing/stretch.rs:15-43, :94-124, :135-221) from their loaded planes to the encoders' input, and
// arcsinh_stretch_rgb_with_stats (core/imaging/stretch.rs:56-90), the one function of SURVEY row a19 that had no device form.
//
// arcsinh_stretch_rgb keeps two numbers of its three compute_image_stats calls: the smallest minimum and the largest maximum
// (stretch.rs:72-78).  Here that is ONE streaming pass over the three planes and no host round trip:
//   range_kernel     per channel the minimum and maximum of the valid pixels (finite, > 1e-7: stats.rs:11-13), as the pixels' bit patterns
//                    -- positive floats order like unsigned integers.  Reduced in the wave by shuffles, across the four waves through
//                    LDS, then one vector atomic max per workgroup and word (the minimum as its complement, so that zeroed words mean
//                    "no valid pixel": ImageStats::default() contributes 0 to both, stats.rs:46-48).  12 B per pixel.
//   stretch_kernel   prologue: every lane folds the six words (f32::min / max), forms range, the range < 1e-10 decision and
//                    inv_range = 1 / range, correctly rounded (the f64 quotient of two f32 values rounds to the f32 quotient), the values
//                    ab_arcsinh_stretch_with_stats forms on the host.  Body: arcsinh_device.hpp's arcsinh_px, the same function
//                    color.hip's arcsinh_kernel calls, on three planes at once; the stretched pixels are stored (12 B + 12 B per pixel),
//                    packed as the preview's TRUNCATED bytes (helpers.rs:243-245) from registers, or both.  Above max_dim without
//                    planes only the picked pixels are loaded and stretched; with planes the same launch stretches the picks again
//                    from the inputs after its plane pass, so bytes never wait for another workgroup's stores.
// The mono command adds the statistics chain and the STF packer of ab_auto_stretch_preview on the stretched plane.  The masked
// command is a composition of ab_masked_stretch_rgb_shared / ab_masked_stretch with the packer (no stretch) behind it.
// Loads and stores are 16 bytes wide where the address allows it, dwords otherwise; bytes leave as whole dwords behind a head placed by
// the output address.  Persistent grids sized from the context's CU count.  -ffp-contract=off like everything else.
#include "ab_common.hpp"
#include "arcsinh_device.hpp"
#include "entry_host.hpp"

#include <cmath>

namespace {

const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65; common.rs:18-22)

struct StretchState {     // the head of AB_WS_STRETCH
    unsigned int enc[6];  // [2 c]: ~bits of channel c's smallest valid pixel, [2 c + 1]: bits of its largest; 0: no valid pixel
    float gmin, gmax;     // what the stretch's prologue folded (or was given)
    int degenerate;       // range < 1e-10: zeros (stretch.rs:22-24)
    int pad;
};

__device__ __forceinline__ bool valid_px(float v) { return __builtin_isfinite(v) && v > 1e-7f; }  // stats.rs:11-13

struct RangeArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};
    int planes = 3;
    int64_t n = 0;
    int64_t head[3] = {0, 0, 0}, quads[3] = {0, 0, 0};  // per plane: pixels [0, head) precede its 16-byte groups
};

__global__ __launch_bounds__(kBlock) void range_kernel(const RangeArgs a, unsigned int *enc) {
    __shared__ unsigned int part[6][kBlock / 64];
    const int64_t stride = (int64_t)gridDim.x * kBlock, t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < a.planes; ++c) {
        const float *src = a.src[c];
        unsigned int lo = 0xffffffffu, hi = 0u;
        auto take = [&](float v) {
            if (valid_px(v)) {
                const unsigned int u = __float_as_uint(v);
                lo = u < lo ? u : lo;
                hi = u > hi ? u : hi;
            }
        };
        for (int64_t q = t0; q < a.quads[c]; q += stride) {
            const float4 t = *reinterpret_cast<const float4 *>(src + a.head[c] + 4 * q);
            take(t.x), take(t.y), take(t.z), take(t.w);
        }
        const int64_t loose = a.n - 4 * a.quads[c];
        for (int64_t e = t0; e < loose; e += stride) take(src[e < a.head[c] ? e : 4 * a.quads[c] + e]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned int ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if (lane == 0) part[2 * c][wave] = ~lo, part[2 * c + 1][wave] = hi;
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * a.planes) {
        unsigned int m = 0u;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) m = part[threadIdx.x][w] > m ? part[threadIdx.x][w] : m;
        if (m) atomicMax(&enc[threadIdx.x], m);
    }
}

struct StretchArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};
    float *out[3] = {nullptr, nullptr, nullptr};
    uint8_t *bytes = nullptr;
    int64_t n = 0, head = 0, quads = 0;  // the plane pass: pixels [0, head) precede the four-pixel groups
    int vec = 0;                         // bit c: a group of source c is one 16-byte load; bit 3 + c: of output c one 16-byte store
    // the sampled bytes: the preview's pn = ph * pw pixels, grouped by the OUTPUT address
    int64_t rows = 0, cols = 0, pn = 0, pw = 0, bhead = 0, bquads = 0;
    double y_ratio = 1.0, x_ratio = 1.0;
    // the range: given by the caller, or the words range_kernel left
    const unsigned int *enc = nullptr;
    int given = 0;
    float gmin = 0.0f, gmax = 0.0f;
    float factor = 0.0f, inv_denom = 0.0f, gamma = 1.0f;
    int apply_gamma = 0;
    StretchState *state = nullptr;  // nullable: where workgroup 0 leaves what it folded
};

struct Norm {
    float dmin, inv_range;
    int degenerate;
};

template <int CH>
__device__ __forceinline__ Norm norm_of(const StretchArgs &a) {
    float gmin = a.gmin, gmax = a.gmax;
    if (!a.given) {  // (sr.min as f32).min(sg.min as f32).min(sb.min as f32), likewise the maximum (stretch.rs:72-78)
        gmin = a.enc[0] ? __uint_as_float(~a.enc[0]) : 0.0f;
        gmax = __uint_as_float(a.enc[1]);
#pragma unroll
        for (int c = 1; c < CH; ++c) {
            gmin = fminf(gmin, a.enc[2 * c] ? __uint_as_float(~a.enc[2 * c]) : 0.0f);
            gmax = fmaxf(gmax, __uint_as_float(a.enc[2 * c + 1]));
        }
    }
    const float range = gmax - gmin;  // stretch.rs:21-26
    Norm nm;
    nm.dmin = gmin;
    nm.degenerate = range < 1e-10f ? 1 : 0;
    nm.inv_range = (float)(1.0 / (double)range);  // 1.0f / range, correctly rounded
    if (a.state && blockIdx.x == 0 && threadIdx.x == 0) a.state->gmin = gmin, a.state->gmax = gmax, a.state->degenerate = nm.degenerate;
    return nm;
}

// (v.clamp(0, 1) * 255f32) as u8: truncated, NaN -> 0 (helpers.rs:243-245; render.hip's plain map)
__device__ __forceinline__ uint32_t trunc_u8(float v) {
    const float x = (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)) * 255.0f;
    return !(x > 0.0f) ? 0u : (x >= 255.0f ? 255u : (uint32_t)(unsigned char)x);
}

// CH planes; STRETCH: arcsinh_px, else the pixels pass through (the masked route's packer); PLANES: the stretched pixels are stored;
// BYTES: 0 none, 1 of every pixel (rides in the plane pass), 2 of the pixels the preview picks (a pass of its own over the inputs)
template <int CH, bool STRETCH, bool PLANES, int BYTES>
__global__ __launch_bounds__(kBlock) void stretch_kernel(const StretchArgs a) {
    static_assert(BYTES == 0 || CH == 3, "the packer interleaves three channels");
    Norm nm = {0.0f, 0.0f, 0};
    if constexpr (STRETCH) nm = norm_of<CH>(a);
    auto px = [&](float v) -> float {
        if constexpr (STRETCH)
            return nm.degenerate ? 0.0f : arcsinh_px(v, nm.dmin, nm.inv_range, a.factor, a.inv_denom, a.apply_gamma, a.gamma);
        else
            return v;
    };
    const int64_t stride = (int64_t)gridDim.x * kBlock, t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (PLANES || BYTES == 1) {
        for (int64_t q = t0; q < a.quads; q += stride) {
            const int64_t i = a.head + 4 * q;
            float v[CH][4];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                if (a.vec & (1 << c)) {
                    const float4 t = *reinterpret_cast<const float4 *>(a.src[c] + i);
                    v[c][0] = t.x, v[c][1] = t.y, v[c][2] = t.z, v[c][3] = t.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[c][k] = a.src[c][i + k];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) v[c][k] = px(v[c][k]);
                if constexpr (PLANES) {
                    if (a.vec & (8 << c)) {
                        *reinterpret_cast<float4 *>(a.out[c] + i) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) a.out[c][i + k] = v[c][k];
                    }
                }
            }
            if constexpr (BYTES == 1) {
                uint32_t d[3] = {0u, 0u, 0u};  // byte j = 3 k + c: four to a dword
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= trunc_u8(v[c][k]) << (8 * ((3 * k + c) & 3));
                uint32_t *o = reinterpret_cast<uint32_t *>(a.bytes + 3 * i);
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = d[j];
            }
        }
        // the pixels around the groups: one per lane, the first lanes of the grid
        const int64_t loose = a.n - 4 * a.quads;
        for (int64_t e = t0; e < loose; e += stride) {
            const int64_t i = e < a.head ? e : 4 * a.quads + e;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const float r = px(a.src[c][i]);
                if constexpr (PLANES) a.out[c][i] = r;
                if constexpr (BYTES == 1) a.bytes[3 * i + c] = (uint8_t)trunc_u8(r);
            }
        }
    }
    if constexpr (BYTES == 2) {
        auto source_of = [&](int64_t i) -> int64_t {
            const uint32_t dy = (uint32_t)i / (uint32_t)a.pw;  // (pn < 2^31)
            const uint32_t dx = (uint32_t)i - dy * (uint32_t)a.pw;
            return nn_index((int64_t)dy, a.y_ratio, a.rows) * a.cols + nn_index((int64_t)dx, a.x_ratio, a.cols);
        };
        for (int64_t q = t0; q < a.bquads; q += stride) {
            const int64_t i = a.bhead + 4 * q;
            uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t si = source_of(i + k);
#pragma unroll
                for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= trunc_u8(px(a.src[c][si])) << (8 * ((3 * k + c) & 3));
            }
            uint32_t *o = reinterpret_cast<uint32_t *>(a.bytes + 3 * i);
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = d[j];
        }
        const int64_t loose = a.pn - 4 * a.bquads;
        for (int64_t e = t0; e < loose; e += stride) {
            const int64_t i = e < a.bhead ? e : 4 * a.bquads + e;
            const int64_t si = source_of(i);
#pragma unroll
            for (int c = 0; c < 3; ++c) a.bytes[3 * i + c] = (uint8_t)trunc_u8(px(a.src[c][si]));
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int launch_range(ab_ctx *ctx, const float *const *src, int planes, int64_t n, unsigned int *enc) {
    AB_HIP(ctx, hipMemsetAsync(enc, 0, 6 * sizeof(unsigned int), ctx->stream));
    RangeArgs a;
    a.planes = planes, a.n = n;
    for (int c = 0; c < planes; ++c) {
        a.src[c] = src[c];
        a.head[c] = head16(src[c], n);
        a.quads[c] = (n - a.head[c]) / 4;
    }
    hipLaunchKernelGGL(range_kernel, dim3(ab_stream_grid(ctx, (n + 3) / 4)), dim3(kBlock), 0, ctx->stream, a, enc);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// one launch: the planes (a.out, when planes), the bytes (a.bytes, when non-null) or both; a.src / a.n and the stretch's scalars are set
template <int CH, bool STRETCH>
int launch_stretch(ab_ctx *ctx, StretchArgs a, bool planes, const Preview &pv) {
    const int bytes = !a.bytes ? 0 : (pv.sampled ? 2 : 1);
    a.head = bytes == 1 ? head_bytes(a.bytes, a.n) : head16(a.src[0], a.n);
    a.quads = (a.n - a.head) / 4;
    for (int c = 0; c < CH; ++c) {
        if (((uintptr_t)(a.src[c] + a.head) & 15u) == 0) a.vec |= 1 << c;
        if (planes && ((uintptr_t)(a.out[c] + a.head) & 15u) == 0) a.vec |= 8 << c;
    }
    int64_t lanes = (planes || bytes == 1) ? std::max<int64_t>(a.quads, a.n - 4 * a.quads) : 0;
    if (bytes == 2) {
        a.pn = pv.ph * pv.pw, a.pw = pv.pw;
        a.y_ratio = (double)a.rows / (double)pv.ph, a.x_ratio = (double)a.cols / (double)pv.pw;
        a.bhead = head_bytes(a.bytes, a.pn);
        a.bquads = (a.pn - a.bhead) / 4;
        lanes = std::max<int64_t>(lanes, std::max<int64_t>(a.bquads, a.pn - 4 * a.bquads));
    }
    const dim3 grid(ab_stream_grid(ctx, lanes)), block(kBlock);
    if constexpr (CH == 1) {
        hipLaunchKernelGGL((stretch_kernel<1, STRETCH, true, 0>), grid, block, 0, ctx->stream, a);
    } else if (planes) {
        if (bytes == 0) hipLaunchKernelGGL((stretch_kernel<CH, STRETCH, true, 0>), grid, block, 0, ctx->stream, a);
        if (bytes == 1) hipLaunchKernelGGL((stretch_kernel<CH, STRETCH, true, 1>), grid, block, 0, ctx->stream, a);
        if (bytes == 2) hipLaunchKernelGGL((stretch_kernel<CH, STRETCH, true, 2>), grid, block, 0, ctx->stream, a);
    } else {
        if (bytes == 1) hipLaunchKernelGGL((stretch_kernel<CH, STRETCH, false, 1>), grid, block, 0, ctx->stream, a);
        if (bytes == 2) hipLaunchKernelGGL((stretch_kernel<CH, STRETCH, false, 2>), grid, block, 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// AB_WS_STRETCH: the state, then `bytes` bytes bound for the host, then `planes` planes of n pixels nobody asked for
struct Carved {
    StretchState *st = nullptr;
    uint8_t *bytes = nullptr;
    float *plane[3] = {nullptr, nullptr, nullptr};
};
int carve(ab_ctx *ctx, size_t bytes, int planes, int64_t n, Carved *w) {
    constexpr size_t head = 256;
    static_assert(sizeof(StretchState) <= head, "the state fits its slot");
    const size_t bytes_al = (bytes + 255) & ~(size_t)255, plane_al = ((size_t)n * sizeof(float) + 255) & ~(size_t)255;
    void *p = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_STRETCH, head + bytes_al + (size_t)planes * plane_al, &p));
    w->st = (StretchState *)p;
    w->bytes = (uint8_t *)p + head;
    for (int c = 0; c < planes; ++c) w->plane[c] = (float *)((char *)p + head + bytes_al + (size_t)c * plane_al);
    return AB_OK;
}

// (factor as f32).clamp(1.0, 500.0) (stretch.rs:26, :102): f32::clamp keeps a NaN
float clamp_factor(double factor) {
    const float f = (float)factor;
    return f < 1.0f ? 1.0f : (f > 500.0f ? 500.0f : f);
}

void set_stretch_scalars(StretchArgs *a, float factor, float gamma) {  // stretch.rs:27-28 (color.hip:417-418)
    a->factor = factor;
    a->inv_denom = 1.0f / asinhf(factor);
    a->gamma = gamma;
    a->apply_gamma = std::fabs(gamma - 1.0f) > 1e-6f;
}

// what the entry points share once their arguments stand: the copies bound for the host join ONE synchronisation
struct Finish {
    ab_ctx *ctx;
    bool wait = false;
    int host_bytes(uint8_t *dst, const uint8_t *src_dev, size_t len) {
        AB_HIP(ctx, hipMemcpyAsync(dst, src_dev, len, hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
        return AB_OK;
    }
    int host_planes(Scope &sc) { return sc.enqueue_host_outs(&wait); }
    int join() {
        if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return AB_OK;
    }
};

// the checks the three composite calls share, before anything touches the device
int composite_check(ab_ctx *ctx, const ab_plane *const ch[3], int64_t max_dim, const ab_plane_mut *out_planes, const uint8_t *out_rgb8, int32_t out_on_device,
                    Preview *pv) {
    AB_TRY(same_dims_check(ctx, ch));  // (the planes of one composite)
    const int64_t rows = ch[0]->rows, cols = ch[0]->cols;
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    AB_CHECK(ctx, out_planes || out_rgb8, "both outputs are null");
    if (out_planes) AB_TRY(out_planes_check(ctx, out_planes, rows, cols));
    AB_TRY(preview_of(ctx, rows, cols, max_dim, pv));
    std::vector<Span> ins, outs;
    for (int c = 0; c < 3; ++c) ins.push_back(span_of(*ch[c]));
    for (int c = 0; c < 3 && out_planes; ++c) outs.push_back(span_of(out_planes[c]));
    if (out_rgb8) outs.push_back(Span{(uintptr_t)out_rgb8, (size_t)(pv->ph * pv->pw) * 3, out_on_device != 0});
    return overlap_check(ctx, ins, outs);
}

// range pass (unless given) and ONE stretch launch over three staged planes; info's state is fetched by the caller
int arcsinh_rgb_chain(ab_ctx *ctx, Scope &sc, const ab_plane *const ch[3], const float *global_min, const float *global_max, float factor, float gamma,
                      ab_plane_mut *out_planes, uint8_t *bytes_dev, const Preview &pv, StretchState *st) {
    StretchArgs a;
    a.rows = ch[0]->rows, a.cols = ch[0]->cols, a.n = a.rows * a.cols;
    for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_in(ch[c], &a.src[c]));
    for (int c = 0; c < 3 && out_planes; ++c) AB_TRY(sc.stage_out(&out_planes[c], &a.out[c]));
    a.bytes = bytes_dev;
    a.enc = st->enc, a.state = st;
    if (global_min) {
        a.given = 1, a.gmin = *global_min, a.gmax = *global_max;
    } else {
        AB_TRY(launch_range(ctx, a.src, 3, a.n, st->enc));
    }
    set_stretch_scalars(&a, factor, gamma);
    return launch_stretch<3, true>(ctx, a, out_planes != nullptr, pv);
}

}  // namespace

extern "C" {

int ab_arcsinh_rgb_range(const ab_image_stats st[3], float out_min_max[2]) try {
    if (!st || !out_min_max) return AB_ERR_INVALID;
    out_min_max[0] = std::fmin(std::fmin((float)st[0].min, (float)st[1].min), (float)st[2].min);  // stretch.rs:76
    out_min_max[1] = std::fmax(std::fmax((float)st[0].max, (float)st[1].max), (float)st[2].max);  // :77
    return AB_OK;
} AB_CATCH_NOCTX

int ab_arcsinh_stretch_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const float *global_min, const float *global_max, float factor,
                           float gamma, ab_plane_mut *out_planes, float out_min_max[2]) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    Preview pv;
    AB_CHECK(ctx, out_planes, "null output planes");
    AB_TRY(composite_check(ctx, ch, 1, out_planes, nullptr, 0, &pv));
    AB_CHECK(ctx, (global_min != nullptr) == (global_max != nullptr), "global_min and global_max are given together or not at all");
    const int64_t n = r->rows * r->cols;

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    Finish fin{ctx};
    if (std::fabs(factor) < 1e-10f) {  // stretch.rs:65-67: the clones; no range is formed
        for (int c = 0; c < 3; ++c) {
            const float *src = nullptr;
            float *dst = nullptr;
            AB_TRY(sc.stage_in(ch[c], &src));
            AB_TRY(sc.stage_out(&out_planes[c], &dst));
            AB_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        }
        AB_TRY(fin.host_planes(sc));
        AB_TRY(fin.join());
        if (out_min_max) out_min_max[0] = out_min_max[1] = 0.0f;
        return AB_OK;
    }
    Carved w;
    AB_TRY(carve(ctx, 0, 0, n, &w));
    pv = Preview();
    AB_TRY(arcsinh_rgb_chain(ctx, sc, ch, global_min, global_max, factor, gamma, out_planes, nullptr, pv, w.st));
    StretchState *pin = nullptr;
    if (out_min_max) {
        AB_TRY(ab_pinned(ctx, sizeof(StretchState), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, w.st, sizeof(StretchState), hipMemcpyDeviceToHost, ctx->stream));
        fin.wait = true;
    }
    AB_TRY(fin.host_planes(sc));
    AB_TRY(fin.join());
    if (out_min_max) out_min_max[0] = pin->gmin, out_min_max[1] = pin->gmax;
    return AB_OK;
} AB_CATCH(ctx)

int ab_arcsinh_stretch_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, double factor, const float *global_min,
                                 const float *global_max, int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device,
                                 ab_arcsinh_composite_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    Preview pv;
    AB_TRY(composite_check(ctx, ch, max_dim, out_planes, out_rgb8, out_on_device, &pv));
    AB_CHECK(ctx, (global_min != nullptr) == (global_max != nullptr), "global_min and global_max are given together or not at all");
    const int64_t rows = r->rows, cols = r->cols, n = rows * cols;
    const float f = clamp_factor(factor);
    const size_t nbytes = (size_t)(pv.ph * pv.pw) * 3;

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    Finish fin{ctx};
    Carved w;
    AB_TRY(carve(ctx, out_rgb8 && !out_on_device ? nbytes : 0, 0, n, &w));
    uint8_t *bytes_dev = !out_rgb8 ? nullptr : (out_on_device ? out_rgb8 : w.bytes);
    AB_TRY(arcsinh_rgb_chain(ctx, sc, ch, global_min, global_max, f, 1.0f, out_planes, bytes_dev, pv, w.st));  // stretch.rs:53: gamma 1
    StretchState *pin = nullptr;
    if (info) {
        AB_TRY(ab_pinned(ctx, sizeof(StretchState), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, w.st, sizeof(StretchState), hipMemcpyDeviceToHost, ctx->stream));
        fin.wait = true;
    }
    if (out_rgb8 && !out_on_device) AB_TRY(fin.host_bytes(out_rgb8, bytes_dev, nbytes));
    AB_TRY(fin.host_planes(sc));
    AB_TRY(fin.join());
    if (info) {
        memset(info, 0, sizeof *info);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->preview_rows = (uint64_t)pv.ph, info->preview_cols = (uint64_t)pv.pw;
        info->factor = f;
        info->global_min = pin->gmin, info->global_max = pin->gmax;
        info->degenerate = pin->degenerate;
    }
    return AB_OK;
} AB_CATCH(ctx)

int ab_arcsinh_stretch_view(ab_ctx *ctx, const ab_plane *img, double factor, ab_plane_mut *out_plane, uint8_t *out_u8, int32_t out_on_device,
                            ab_arcsinh_view_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img, "image"));
    const int64_t rows = img->rows, cols = img->cols, n = rows * cols;
    AB_CHECK(ctx, out_plane && out_plane->data, "null output plane");
    AB_CHECK(ctx, out_plane->rows == rows && out_plane->cols == cols, "the output plane must be %lld x %lld (got %lld x %lld)", (long long)rows, (long long)cols,
             (long long)out_plane->rows, (long long)out_plane->cols);
    AB_CHECK(ctx, ((uintptr_t)out_plane->data & 3u) == 0, "the output plane is not float-aligned");
    {
        std::vector<Span> ins{span_of(*img)}, outs{span_of(*out_plane)};
        if (out_u8) outs.push_back(Span{(uintptr_t)out_u8, (size_t)n, out_on_device != 0});
        AB_TRY(overlap_check(ctx, ins, outs));
    }
    const float f = clamp_factor(factor);

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    Finish fin{ctx};
    Carved w;
    AB_TRY(carve(ctx, out_u8 && !out_on_device ? (size_t)n : 0, 0, n, &w));
    StretchArgs a;
    a.rows = rows, a.cols = cols, a.n = n;
    AB_TRY(sc.stage_in(img, &a.src[0]));
    AB_TRY(sc.stage_out(out_plane, &a.out[0]));
    a.enc = w.st->enc, a.state = w.st;
    AB_TRY(launch_range(ctx, a.src, 1, n, w.st->enc));  // stretch.rs:6-7: stats.min / .max as f32
    set_stretch_scalars(&a, f, 1.0f);
    AB_TRY((launch_stretch<1, true>(ctx, a, true, Preview())));
    // render_and_save (cmd/common.rs:209-240): auto_stretch_preview of the stretched plane
    const ab_image_stats *res = nullptr;
    const void *tx = nullptr;
    const ab_stf_params *stf = nullptr;
    AB_TRY(ab_stats_enqueue(ctx, nullptr, a.out[0], n, n, 0, 0.0, 0.0, &kStfDefault, &res, &tx, &stf));
    uint8_t *u8_dev = !out_u8 ? nullptr : (out_on_device ? out_u8 : w.bytes);
    if (out_u8) AB_TRY(ab_stf_u8_device_tx(ctx, a.out[0], n, tx, u8_dev));
    char *pin = nullptr;
    constexpr size_t kStatsAt = 64, kStfAt = kStatsAt + sizeof(ab_image_stats);
    static_assert(sizeof(StretchState) <= kStatsAt, "the state fits before the statistics");
    if (info) {
        AB_TRY(ab_pinned(ctx, kStfAt + sizeof(ab_stf_params), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, w.st, sizeof(StretchState), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipMemcpyAsync(pin + kStatsAt, res, sizeof(ab_image_stats), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipMemcpyAsync(pin + kStfAt, stf, sizeof(ab_stf_params), hipMemcpyDeviceToHost, ctx->stream));
        fin.wait = true;
    }
    if (out_u8 && !out_on_device) AB_TRY(fin.host_bytes(out_u8, u8_dev, (size_t)n));
    AB_TRY(fin.host_planes(sc));
    AB_TRY(fin.join());
    if (info) {
        memset(info, 0, sizeof *info);
        StretchState st;
        memcpy(&st, pin, sizeof st);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->factor = f;
        info->data_min = st.gmin, info->data_max = st.gmax;
        info->degenerate = st.degenerate;
        memcpy(&info->stats, pin + kStatsAt, sizeof info->stats);
        memcpy(&info->stf, pin + kStfAt, sizeof info->stf);
    }
    return AB_OK;
} AB_CATCH(ctx)

int ab_masked_stretch_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_masked_stretch_config *cfg, int32_t shared_mask,
                                int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device,
                                ab_masked_stretch_composite_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    Preview pv;
    AB_TRY(composite_check(ctx, ch, max_dim, out_planes, out_rgb8, out_on_device, &pv));
    AB_CHECK(ctx, cfg, "null configuration");
    const int64_t rows = r->rows, cols = r->cols, n = rows * cols;
    const size_t nbytes = (size_t)(pv.ph * pv.pw) * 3;

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    // the stretched planes stay on the device for the packer: in the caller's device planes, else in the workspace
    int spare = 0;
    for (int c = 0; c < 3; ++c) spare += !(out_planes && out_planes[c].on_device);
    Carved w;
    AB_TRY(carve(ctx, out_rgb8 && !out_on_device ? nbytes : 0, spare, n, &w));
    ab_plane_mut dev[3];
    for (int c = 0, s = 0; c < 3; ++c) {
        const bool theirs = out_planes && out_planes[c].on_device;
        dev[c] = ab_plane_mut{theirs ? out_planes[c].data : w.plane[s++], rows, cols, 1};
    }
    ab_masked_stretch_result res[3];
    ab_star_mask_info shared = {0, 0.0};
    if (shared_mask) {  // stretch.rs:163-175
        AB_TRY(ab_masked_stretch_rgb_shared(ctx, r, g, b, cfg, &dev[0], &dev[1], &dev[2], res, &shared));
    } else {  // :177-183
        for (int c = 0; c < 3; ++c) AB_TRY(ab_masked_stretch(ctx, ch[c], cfg, &dev[c], &res[c]));
    }
    Finish fin{ctx};
    uint8_t *bytes_dev = !out_rgb8 ? nullptr : (out_on_device ? out_rgb8 : w.bytes);
    if (out_rgb8) {
        StretchArgs a;
        a.rows = rows, a.cols = cols, a.n = n, a.bytes = bytes_dev;
        for (int c = 0; c < 3; ++c) a.src[c] = dev[c].data;
        AB_TRY((launch_stretch<3, false>(ctx, a, false, pv)));
        if (!out_on_device) AB_TRY(fin.host_bytes(out_rgb8, bytes_dev, nbytes));
    }
    for (int c = 0; c < 3 && out_planes; ++c)
        if (!out_planes[c].on_device) {
            AB_HIP(ctx, hipMemcpyAsync(out_planes[c].data, dev[c].data, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            fin.wait = true;
        }
    AB_TRY(fin.join());
    if (info) {
        memset(info, 0, sizeof *info);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->preview_rows = (uint64_t)pv.ph, info->preview_cols = (uint64_t)pv.pw;
        for (int c = 0; c < 3; ++c) info->channels[c] = res[c];
        if (shared_mask) {
            info->mask_mode = AB_MASK_SHARED_LUMINANCE;
            info->stars_masked = (uint64_t)shared.stars_masked, info->mask_coverage = shared.coverage_fraction;  // :173
        } else {
            info->mask_mode = AB_MASK_PER_CHANNEL;
            info->stars_masked = (uint64_t)(res[0].stars_masked + res[1].stars_masked + res[2].stars_masked);  // :192
            info->mask_coverage = (res[0].mask_coverage + res[1].mask_coverage + res[2].mask_coverage) / 3.0;  // :193
        }
    }
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
