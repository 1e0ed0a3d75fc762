// The compose wizard's blend and colour steps on gfx950: blend_channels_cmd and calibrate_and_scnr_cmd from their loaded channels to
// the encoder's input, and the host-only decisions beside them (the colour step's plan, compute_auto_wb_cmd).
//
// Replaces cmd/compose/blend.rs:143-205 and cmd/compose/color.rs:21-49, :112-169, :187-224 up to the PNG encoder and the JSON.  Both
// commands end alike -- three ImageStats, compute_linked_stf (cmd/helpers.rs:185-202), three make_stf_u8_fn(linked, stats[c])
// (core/imaging/stf.rs:122-145), render_rgb_preview_with_stf (cmd/helpers.rs:264-322) -- and each is ONE chain here that stays in HBM:
//   wb_scnr_kernel      (colour) per pixel: three loads, v * factor[c] as a plain f32 multiply (color.rs:29, :38), scnr_device.hpp's
//                       scnr_px on the three products in registers when SCNR is applied, three stores: 12 B read and 12 B written.
//                       The unfused form -- three scale kernels (8 B each) and SCNR in place (24 B) -- moves 48 B.
//   blend_kernel        (blend) color.hip's, through ab_blend_device, after the bicubic resample of the channels that differ in size.
//   statistics          exactly three chains (stats.hip: ab_stats_enqueue), each of a FINAL plane by the route that yields what the
//                       reference keeps (color_plan below); the statistics the reference computes and overwrites (color.rs:150-154)
//                       are never computed.  Each result is copied out of the chain's state block before the next chain reuses it
//                       (save_stats_device.hpp's save_stats_kernel).
//   linked_stf_kernel   one small workgroup: the combined statistics with extras.hip's expressions in their order, ab_auto_stf_hd,
//                       make_tx x 3 -- the same __host__ __device__ functions the host entry points run, IEEE basic operations only.
//                       With it no host round trip stands between the statistics and the preview.
//   preview_stf_kernel  render_rgb_preview_with_stf with its three transforms read from HBM: the ROUNDED byte of apply_stf
//                       (stf_device.hpp's to_u8), interleaved; above max_dim only the picked pixels are loaded.
// and at most one synchronisation, which fetches info and the host outputs (none with info NULL and device outputs).
// Loads are 16 bytes wide behind a scalar head, so any float-aligned plane works; bytes leave as whole dwords where the output address
// allows it.  Persistent grids sized from the context's CU count.  -ffp-contract=off like everything else: each stage is the
// instruction sequence of the kernel it restates, so planes and bytes equal the library's own unfused calls bit for bit.
#include "ab_common.hpp"
#include "save_stats_device.hpp"
#include "scnr_device.hpp"
#include "stf_device.hpp"
#include "entry_host.hpp"

#include <cfloat>
#include <cmath>

namespace {

constexpr uint64_t kParThreshold = 4000000;  // PAR_THRESHOLD (color.rs:19)
constexpr int kMaxChannels = 16, kMaxWeights = 32;  // ab_blend_channels' limits (color.hip)

struct WizState {  // what the chain leaves in AB_WS_WIZARD
    ab_image_stats stats[3];
    ab_stf_params stf;
    StfTx tx[3];
};

struct WbArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};
    float *out[3] = {nullptr, nullptr, nullptr};
    int64_t n = 0;
    int64_t head = 0, quads = 0;  // pixels [0, head) precede the four-pixel groups [head, head + 4 * quads)
    float factor[3] = {1.0f, 1.0f, 1.0f};
    int method = 0;
    float amount = 0.0f;  // clamped to [0, 1] (scnr.rs:28)
    int preserve = 0;
};

// VEC: every plane is 16-byte aligned behind the head, a group is one 16-byte access (else four dwords)
template <bool SCNR, bool VEC>
__global__ __launch_bounds__(kBlock) void wb_scnr_kernel(const WbArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.quads; q += stride) {
        const int64_t i = a.head + 4 * q;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4 *>(a.src[c] + i);
                v[c][0] = t.x, v[c][1] = t.y, v[c][2] = t.z, v[c][3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[c][k] = a.src[c][i + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = v[c][k] * a.factor[c];  // color.rs:29, :38
        }
        if constexpr (SCNR) {
#pragma unroll
            for (int k = 0; k < 4; ++k) scnr_px(v[0][k], v[1][k], v[2][k], a.method, a.amount, a.preserve);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC) {
                *reinterpret_cast<float4 *>(a.out[c] + i) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) a.out[c][i + k] = v[c][k];
            }
        }
    }
    // the pixels around the groups: one per lane, the first lanes of the grid
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        float rv = a.src[0][i] * a.factor[0], gv = a.src[1][i] * a.factor[1], bv = a.src[2][i] * a.factor[2];
        if constexpr (SCNR) scnr_px(rv, gv, bv, a.method, a.amount, a.preserve);
        a.out[0][i] = rv, a.out[1][i] = gv, a.out[2][i] = bv;
    }
}

// compute_linked_stf_with_stats (cmd/helpers.rs:185-202; extras.hip:178-185, the same expressions in the same order), auto_stf and
// make_stf_u8_fn(&linked, stats[c]) x 3
__global__ __launch_bounds__(64) void linked_stf_kernel(WizState *w, const ab_auto_stf_config cfg) {
    if (threadIdx.x != 0) return;
    const ab_image_stats sr = w->stats[0], sg = w->stats[1], sb = w->stats[2];
    ab_image_stats c;
    c.min = fmin(fmin(sr.min, sg.min), sb.min);
    c.max = fmax(fmax(sr.max, sg.max), sb.max);
    c.mean = (sr.mean + sg.mean + sb.mean) / 3.0;
    c.median = (sr.median + sg.median + sb.median) / 3.0;
    c.sigma = sqrt((sr.sigma * sr.sigma + sg.sigma * sg.sigma + sb.sigma * sb.sigma) / 3.0);
    c.mad = (sr.mad + sg.mad + sb.mad) / 3.0;
    c.valid_count = sr.valid_count;
    ab_stf_params stf;
    ab_auto_stf_hd(&c, &cfg, &stf);
    w->stf = stf;
    w->tx[0] = make_tx(&stf, &sr);
    w->tx[1] = make_tx(&stf, &sg);
    w->tx[2] = make_tx(&stf, &sb);
}

struct PreviewArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};
    int64_t rows = 0, cols = 0;   // of the source planes
    int64_t n = 0;                // output pixels: rows * cols, or the preview's when sampled
    int64_t pw = 0;               // sampled: the preview's columns
    double y_ratio = 1.0, x_ratio = 1.0;
    int64_t head = 0, quads = 0;  // placed by the OUTPUT address: the 12 bytes of a group are three aligned dwords
    int in16 = 0;                 // bit c: a group of source c is one 16-byte load
    const StfTx *tx = nullptr;    // the three transforms linked_stf_kernel left
    uint8_t *out = nullptr;
};

template <bool SAMPLED>
__device__ __forceinline__ int64_t source_of(const PreviewArgs &a, int64_t i) {
    if constexpr (SAMPLED) {
        const uint32_t dy = (uint32_t)i / (uint32_t)a.pw;  // (n < 2^31)
        const uint32_t dx = (uint32_t)i - dy * (uint32_t)a.pw;
        return nn_index((int64_t)dy, a.y_ratio, a.rows) * a.cols + nn_index((int64_t)dx, a.x_ratio, a.cols);
    } else {
        return i;
    }
}

template <bool SAMPLED>
__global__ __launch_bounds__(kBlock) void preview_stf_kernel(const PreviewArgs a) {
    const StfTx tx[3] = {a.tx[0], a.tx[1], a.tx[2]};
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.quads; q += stride) {
        const int64_t i = a.head + 4 * q;
        float s[3][4];
        if constexpr (SAMPLED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t si = source_of<true>(a, i + k);
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c][k] = a.src[c][si];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.in16 & (1 << c)) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.src[c] + i);
                    s[c][0] = v.x, s[c][1] = v.y, s[c][2] = v.z, s[c][3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[c][k] = a.src[c][i + k];
                }
            }
        }
        uint32_t d[3] = {0u, 0u, 0u};  // byte j = 3 k + c: four to a dword
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= (uint32_t)to_u8(s[c][k], tx[c]) << (8 * ((3 * k + c) & 3));
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 3 * i);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = d[j];
    }
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        const int64_t si = source_of<SAMPLED>(a, i);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out[3 * i + c] = to_u8(a.src[c][si], tx[c]);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65; color.rs:163, blend.rs:200)

int launch_wb(ab_ctx *ctx, WbArgs a, bool scnr) {
    a.head = head16(a.src[0], a.n);
    a.quads = (a.n - a.head) / 4;
    uintptr_t bits = 0;
    for (int c = 0; c < 3; ++c) bits |= (uintptr_t)(a.src[c] + a.head) | (uintptr_t)(a.out[c] + a.head);
    const bool vec = (bits & 15u) == 0;
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, a.n - 4 * a.quads));
    if (scnr && vec) {
        hipLaunchKernelGGL((wb_scnr_kernel<true, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else if (scnr) {
        hipLaunchKernelGGL((wb_scnr_kernel<true, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else if (vec) {
        hipLaunchKernelGGL((wb_scnr_kernel<false, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((wb_scnr_kernel<false, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

int launch_preview(ab_ctx *ctx, PreviewArgs a, bool sampled) {
    a.head = head_bytes(a.out, a.n);
    a.quads = (a.n - a.head) / 4;
    for (int c = 0; c < 3 && !sampled; ++c)
        if (((uintptr_t)(a.src[c] + a.head) & 15u) == 0) a.in16 |= 1 << c;
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, a.n - 4 * a.quads));
    if (sampled) {
        hipLaunchKernelGGL(preview_stf_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(preview_stf_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// calibrate_and_scnr_cmd's decisions (color.rs:115-117, :138-159 with calibrate_channel, :21-49)
void color_plan(uint64_t n, const ab_image_stats st[3], const double factors[3], bool has_scnr, const ab_scnr_config *scnr, ab_color_plan *p) {
    memset(p, 0, sizeof *p);
    for (int c = 0; c < 3; ++c) {
        const float f = (float)factors[c];
        p->factors[c] = f > 1e-6f ? f : 1e-6f;  // f32::max: of a NaN and a number, the number
    }
    const bool applied = has_scnr && scnr->amount > 1e-7f;  // :139 (false for a NaN)
    p->scnr_applied = applied ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        const bool recomputed = applied && (c == 1 || scnr->preserve_luminance);  // :142-155
        if (n <= kParThreshold || recomputed) {
            p->route[c] = AB_COLOR_STATS_EXACT_OR_FULL;
            continue;
        }
        p->route[c] = AB_COLOR_STATS_KNOWN_RANGE;  // :41-47
        const float factor = p->factors[c];
        const double f = (double)factor;
        p->known_min[c] = factor >= 0.0f ? st[c].min * f : st[c].max * f;
        p->known_max[c] = factor >= 0.0f ? st[c].max * f : st[c].min * f;
    }
}

// The common tail of the two commands over three device planes: the statistics (known == nullptr: compute_image_stats x 3), the linked
// STF, the preview, the one synchronisation and info's common fields.  outs: the staged output planes behind `planes`.
struct Tail {
    int64_t rows, cols;
    Preview pv;
    uint8_t *out_rgb8;
    int32_t out_on_device;
    bool want_info;
    WizState result;  // valid after run() when want_info
};

int run_tail(ab_ctx *ctx, Scope &sc, WizState *ws, const ab_color_plan *known, Tail *t) {
    const int64_t n = t->rows * t->cols;
    const float *planes[3] = {sc.outs[0].dptr, sc.outs[1].dptr, sc.outs[2].dptr};  // (the step's three planes are staged first)
    for (int c = 0; c < 3; ++c) {
        const ab_image_stats *res = nullptr;
        const bool use_known = known && known->route[c] == AB_COLOR_STATS_KNOWN_RANGE;
        AB_TRY(ab_stats_enqueue(ctx, nullptr, planes[c], n, n, use_known ? 1 : 0, use_known ? known->known_min[c] : 0.0, use_known ? known->known_max[c] : 0.0,
                                &kStfDefault, &res, nullptr, nullptr));
        hipLaunchKernelGGL(save_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, res, &ws->stats[c]);
        AB_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(linked_stf_kernel, dim3(1), dim3(64), 0, ctx->stream, ws, kStfDefault);
    AB_HIP(ctx, hipGetLastError());
    const size_t nbytes = (size_t)(t->pv.ph * t->pv.pw) * 3;
    uint8_t *bytes_dev = t->out_rgb8;  // the caller's buffer, or the scratch arena for a host output (the statistics chain asks for none)
    if (t->out_rgb8) {
        if (!t->out_on_device) AB_TRY(ab_scratch(ctx, nbytes, (void **)&bytes_dev));
        PreviewArgs a;
        a.rows = t->rows, a.cols = t->cols, a.n = n, a.tx = ws->tx, a.out = bytes_dev;
        for (int c = 0; c < 3; ++c) a.src[c] = planes[c];
        if (t->pv.sampled) {
            a.n = t->pv.ph * t->pv.pw, a.pw = t->pv.pw;
            a.y_ratio = (double)t->rows / (double)t->pv.ph, a.x_ratio = (double)t->cols / (double)t->pv.pw;
        }
        AB_TRY(launch_preview(ctx, a, t->pv.sampled));
    }
    char *pin = nullptr;
    bool wait = false;
    if (t->want_info) {
        AB_TRY(ab_pinned(ctx, sizeof(WizState), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, ws, sizeof(WizState), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (t->out_rgb8 && !t->out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(t->out_rgb8, bytes_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    AB_TRY(sc.enqueue_host_outs(&wait));
    if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (t->want_info) memcpy(&t->result, pin, sizeof t->result);
    return AB_OK;
}

int carve(ab_ctx *ctx, size_t extra_bytes, WizState **ws, char **extra) {
    constexpr size_t head = (sizeof(WizState) + 255) & ~(size_t)255;
    void *p = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_WIZARD, head + extra_bytes, &p));
    *ws = (WizState *)p;
    if (extra) *extra = (char *)p + head;
    return AB_OK;
}

}  // namespace

extern "C" {

int ab_color_step_plan(uint64_t n_pixels, const ab_image_stats orig_stats[3], const double factors[3], int32_t has_scnr, const ab_scnr_config *scnr,
                       ab_color_plan *plan) try {
    if (!orig_stats || !factors || !plan || (has_scnr && !scnr)) return AB_ERR_INVALID;
    color_plan(n_pixels, orig_stats, factors, has_scnr != 0, scnr, plan);
    return AB_OK;
} AB_CATCH_NOCTX

int ab_compute_auto_wb(const ab_image_stats *sr, const ab_image_stats *sg, const ab_image_stats *sb, ab_auto_wb *out) try {
    if (!sr || !sg || !sb || !out) return AB_ERR_INVALID;
    memset(out, 0, sizeof *out);
    const ab_image_stats *s[3] = {sr, sg, sb};
    double stab[3], med[3];
    for (int c = 0; c < 3; ++c) {
        stab[c] = s[c]->median > 1e-10 ? s[c]->mad / s[c]->median : DBL_MAX;  // color.rs:196-198
        med[c] = std::fmax(s[c]->median, 1e-10);                              // f64::max
        out->stability[c] = stab[c];
    }
    const int ref = stab[0] <= stab[1] && stab[0] <= stab[2] ? 0 : (stab[2] <= stab[1] ? 2 : 1);  // :203, :206, :221
    for (int c = 0; c < 3; ++c) out->factors[c] = c == ref ? 1.0 : med[ref] / med[c];
    out->ref_channel = ref;
    return AB_OK;
} AB_CATCH_NOCTX

int ab_calibrate_and_scnr(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats orig_stats[3], const double factors[3],
                          int32_t has_scnr, const ab_scnr_config *scnr, int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device,
                          ab_color_step_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    AB_TRY(same_dims_check(ctx, ch));  // (the planes of one composite)
    AB_CHECK(ctx, orig_stats && factors, "null statistics or factors");
    AB_CHECK(ctx, !has_scnr || scnr, "has_scnr is set and the SCNR configuration is null");
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    const int64_t rows = r->rows, cols = r->cols, n = rows * cols;
    AB_TRY(out_planes_check(ctx, out_planes, rows, cols));
    Preview pv;
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    {
        std::vector<Span> ins, outs;
        for (int c = 0; c < 3; ++c) ins.push_back(span_of(*ch[c])), outs.push_back(span_of(out_planes[c]));
        if (out_rgb8) outs.push_back(Span{(uintptr_t)out_rgb8, (size_t)(pv.ph * pv.pw) * 3, out_on_device != 0});
        AB_TRY(overlap_check(ctx, ins, outs));
    }
    ab_color_plan plan;
    color_plan((uint64_t)n, orig_stats, factors, has_scnr != 0, scnr, &plan);

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    WizState *ws = nullptr;
    AB_TRY(carve(ctx, 0, &ws, nullptr));
    WbArgs a;
    a.n = n;
    for (int c = 0; c < 3; ++c) {
        AB_TRY(sc.stage_in(ch[c], &a.src[c]));
        a.factor[c] = plan.factors[c];
    }
    for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_out(&out_planes[c], &a.out[c]));
    if (plan.scnr_applied) {
        a.method = scnr->method;
        a.amount = scnr->amount > 1.0f ? 1.0f : scnr->amount;  // scnr.rs:28 (above 1e-7 already)
        a.preserve = scnr->preserve_luminance;
    }
    AB_TRY(launch_wb(ctx, a, plan.scnr_applied != 0));
    Tail t{rows, cols, pv, out_rgb8, out_on_device, info != nullptr, {}};
    AB_TRY(run_tail(ctx, sc, ws, &plan, &t));
    if (info) {
        memset(info, 0, sizeof *info);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->preview_rows = (uint64_t)pv.ph, info->preview_cols = (uint64_t)pv.pw;
        info->scnr_applied = plan.scnr_applied;
        for (int c = 0; c < 3; ++c) info->factors[c] = plan.factors[c], info->route[c] = plan.route[c], info->stats[c] = t.result.stats[c];
        info->stf = t.result.stf;
    }
    return AB_OK;
} AB_CATCH(ctx)

int ab_blend_composite(ab_ctx *ctx, const ab_plane *channels, size_t n_channels, const ab_blend_weight *weights, size_t n_weights, int64_t max_dim,
                       ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device, ab_blend_composite_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    if (n_channels == 0) return ab_set_error(ctx, AB_ERR_INVALID, "No channel paths provided");  // blend.rs:139-141
    AB_CHECK(ctx, channels, "null channels");
    AB_CHECK(ctx, n_channels <= (size_t)kMaxChannels, "at most %d channels (got %zu)", kMaxChannels, n_channels);
    AB_CHECK(ctx, weights || n_weights == 0, "null weights");
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    size_t in_range = 0;  // (a weight whose channel_idx is out of range is skipped, channel_blend.rs:20-23)
    for (size_t w = 0; w < n_weights; ++w) in_range += weights[w].channel_idx < n_channels;
    AB_CHECK(ctx, in_range <= (size_t)kMaxWeights, "at most %d blend weights (got %zu)", kMaxWeights, in_range);
    int64_t rows = 0, cols = 0;  // :148-150
    for (size_t i = 0; i < n_channels; ++i) {
        AB_TRY(plane_check(ctx, &channels[i], "channel"));
        rows = std::max(rows, channels[i].rows), cols = std::max(cols, channels[i].cols);
    }
    AB_CHECK(ctx, fits31(rows, cols), "the composite of %lld x %lld holds 2^31 pixels or more", (long long)rows, (long long)cols);
    const int64_t n = rows * cols;
    size_t n_resampled = 0;
    for (size_t i = 0; i < n_channels; ++i) n_resampled += channels[i].rows != rows || channels[i].cols != cols;  // :152
    AB_CHECK(ctx, n_resampled == 0 || rows <= 65535, "a resample to %lld rows is not in this build", (long long)rows);
    AB_TRY(out_planes_check(ctx, out_planes, rows, cols));
    Preview pv;
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    {
        std::vector<Span> ins, outs;
        for (size_t i = 0; i < n_channels; ++i) ins.push_back(span_of(channels[i]));
        for (int c = 0; c < 3; ++c) outs.push_back(span_of(out_planes[c]));
        if (out_rgb8) outs.push_back(Span{(uintptr_t)out_rgb8, (size_t)(pv.ph * pv.pw) * 3, out_on_device != 0});
        AB_TRY(overlap_check(ctx, ins, outs));
    }

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    WizState *ws = nullptr;
    char *extra = nullptr;
    const size_t plane_bytes = ((size_t)n * sizeof(float) + 255) & ~(size_t)255;
    AB_TRY(carve(ctx, n_resampled * plane_bytes, &ws, &extra));
    const float *src[kMaxChannels];
    size_t slot = 0;
    for (size_t i = 0; i < n_channels; ++i) {
        AB_TRY(sc.stage_in(&channels[i], &src[i]));
        if (channels[i].rows != rows || channels[i].cols != cols) {  // :160-161; the original is untouched
            float *dst = (float *)(extra + slot++ * plane_bytes);
            AB_TRY(ab_resample_device(ctx, src[i], channels[i].rows, channels[i].cols, rows, cols, dst));
            src[i] = dst;
        }
    }
    float *dst[3];
    for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_out(&out_planes[c], &dst[c]));
    AB_TRY(ab_blend_device(ctx, src, n_channels, weights, n_weights, n, dst[0], dst[1], dst[2]));  // :185
    Tail t{rows, cols, pv, out_rgb8, out_on_device, info != nullptr, {}};
    AB_TRY(run_tail(ctx, sc, ws, nullptr, &t));  // :187-205
    if (info) {
        memset(info, 0, sizeof *info);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->preview_rows = (uint64_t)pv.ph, info->preview_cols = (uint64_t)pv.pw;
        info->resampled = n_resampled ? 1 : 0;
        for (int c = 0; c < 3; ++c) info->stats[c] = t.result.stats[c];
        info->stf = t.result.stf;
    }
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
