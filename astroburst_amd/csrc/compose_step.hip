// The "RGB Compose" panel on gfx950: compose_rgb_cmd from its loaded entries to the PNG encoder's input and the JSON, as one chain.
//
// Replaces the body of cmd/compose/rgb.rs:43-205: process_rgb (core/compose/rgb.rs:209-323), the L branch (:118-151: resample_image,
// stf::analyze = compute_image_stats, auto_stf, apply_stf_f32, apply_lrgb of core/compose/lrgb.rs:4-45) and render_rgb_preview
// (cmd/helpers.rs:204-262).  The command keeps the white-balanced pre-stretch planes with their statistics (:106-116) and the preview's
// bytes (:153-161); the final planes are dropped.  So:
//   front half           ab_compose_front_check / ab_compose_front_device (compose_rgb.hip), the channels landing in out_pre directly
//   statistics           ab_stats_enqueue chains, each result saved beside the others in AB_WS_COMPOSE (save_stats_device.hpp); the
//                        host sees the pre-white-balance ones once, and only for WhiteBalance::Auto (ab_select_wb_reference)
//   wb_merge_kernel      ONE launch: every channel whose (mult as f32 - 1).abs() >= 1e-7 scaled in place (rgb.rs:127-130) and, when
//                        linked, merge_for_stf's plane (rv + gv + bv) * (1.0f / 3.0f) from the rounded products in registers (:157-160)
//   compose_params_kernel one lane: the STF source per configuration (auto_stf per channel, of the combined plane, or the given ones),
//                        the three compose-local transforms, L's StfTx
//   compose_finish_kernel<SAMPLED, LRGB>  per pixel in registers: compose-local STF x 3 (compose_device.hpp), SCNR (scnr_device.hpp),
//                        L through apply_stf_f32's arithmetic (stf_device.hpp's to_f32), apply_lrgb, the truncating byte, the packing
//                        of tone.hip's kernel (twelve bytes as three dwords placed by the OUTPUT address).  SAMPLED: only the pixels
//                        the preview picks are loaded and finished.
// and one final synchronisation for info and the host outputs (none with info NULL and device outputs).  Registration keeps its own.
// -ffp-contract=off like everything else: each stage is the instruction sequence of the kernel it restates, so planes, bytes, STFs and
// statistics equal the library's own chain ab_process_rgb -> ab_resample_image -> ab_compute_image_stats -> ab_auto_stf ->
// ab_apply_stf_f32 -> ab_apply_lrgb -> ab_render_rgb_preview bit for bit (the mean to the statistics routes' 1e-12).
#include "ab_common.hpp"
#include "compose_device.hpp"
#include "save_stats_device.hpp"
#include "scnr_device.hpp"
#include "stf_device.hpp"
#include "entry_host.hpp"

#include <cmath>

namespace {

struct ComposeState {  // what the chain leaves in AB_WS_COMPOSE
    ab_image_stats full[3];  // before white balance
    ab_image_stats wb[3];    // after it: what the STF is applied with
    ab_image_stats comb;     // of merge_for_stf's plane (linked)
    ab_image_stats l;        // of the matched L (auto_stretch)
    ab_stf_params stf[3], l_stf;
    ComposeStf tx[3];
    StfTx ltx;
};

struct WbMergeArgs {
    float *p[3] = {nullptr, nullptr, nullptr};
    float *comb = nullptr;        // merge_for_stf's plane, or nullptr (unlinked)
    int64_t n = 0;
    int64_t head = 0, quads = 0;  // pixels [0, head) precede the four-pixel groups [head, head + 4 * quads)
    float mult[3] = {1.0f, 1.0f, 1.0f};
    int scale[3] = {0, 0, 0};
};

// VEC: every plane is 16-byte aligned behind the head, a group is one 16-byte access (else four dwords)
template <bool VEC>
__global__ __launch_bounds__(kBlock) void wb_merge_kernel(const WbMergeArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.quads; q += stride) {
        const int64_t i = a.head + 4 * q;
        float v[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!a.scale[c] && !a.comb) continue;
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4 *>(a.p[c] + i);
                v[c][0] = t.x, v[c][1] = t.y, v[c][2] = t.z, v[c][3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[c][k] = a.p[c][i + k];
            }
            if (!a.scale[c]) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = v[c][k] * a.mult[c];  // rgb.rs:129
            if constexpr (VEC) {
                *reinterpret_cast<float4 *>(a.p[c] + i) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) a.p[c][i + k] = v[c][k];
            }
        }
        if (a.comb) {  // rgb.rs:157-160
            float m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = (v[0][k] + v[1][k] + v[2][k]) * (1.0f / 3.0f);
            if constexpr (VEC) {
                *reinterpret_cast<float4 *>(a.comb + i) = make_float4(m[0], m[1], m[2], m[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) a.comb[i + k] = m[k];
            }
        }
    }
    // the pixels around the groups: one per lane, the first lanes of the grid
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        float v[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!a.scale[c] && !a.comb) continue;
            v[c] = a.p[c][i];
            if (!a.scale[c]) continue;
            v[c] = v[c] * a.mult[c];
            a.p[c][i] = v[c];
        }
        if (a.comb) a.comb[i] = (v[0] + v[1] + v[2]) * (1.0f / 3.0f);
    }
}

struct ParamArgs {
    int auto_stretch = 0, linked = 0, has_l = 0;
    ab_stf_params given[3] = {};  // cfg->stf[c] or {0, 0.5, 1} (rgb.rs:283-294)
    ab_auto_stf_config stf_cfg = {0.25, -2.8};
};

// process_rgb's STF sources (rgb.rs:265-294), apply_stf_inplace's scalars (:192-197), and the L branch's auto_stf with
// StfTransform::new (cmd/compose/rgb.rs:130-135, stf.rs:69-78): the __host__ __device__ functions the host entry points run
__global__ __launch_bounds__(64) void compose_params_kernel(ComposeState *w, const ParamArgs a) {
    if (threadIdx.x != 0) return;
    ab_stf_params linked = {0.0, 0.5, 1.0};
    if (a.auto_stretch && a.linked) {
        const ab_image_stats comb = w->comb;
        ab_auto_stf_hd(&comb, &a.stf_cfg, &linked);
    }
    for (int c = 0; c < 3; ++c) {
        const ab_image_stats st = w->wb[c];
        ab_stf_params p = a.given[c];
        if (a.auto_stretch && a.linked)
            p = linked;
        else if (a.auto_stretch)
            ab_auto_stf_hd(&st, &a.stf_cfg, &p);
        w->stf[c] = p;
        ComposeStf t;
        t.dmin = st.min;
        t.inv_range = 1.0 / fmax(st.max - st.min, 1e-30);
        t.shadow = p.shadow;
        t.clip_range = fmax(p.highlight - p.shadow, 1e-15);
        t.m = p.midtone;
        w->tx[c] = t;
    }
    ab_stf_params lp = {0.0, 0.0, 0.0};
    StfTx lt = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.has_l && a.auto_stretch) {
        const ab_image_stats ls = w->l;
        ab_auto_stf_hd(&ls, &a.stf_cfg, &lp);
        lt = make_tx(&lp, &ls);
    }
    w->l_stf = lp;
    w->ltx = lt;
}

struct FinishArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};  // the white-balanced planes (plain: planes that are finished already)
    const float *l = nullptr;      // LRGB: the matched L
    int64_t rows = 0, cols = 0;    // of the source planes
    int64_t n = 0;                 // output pixels: rows * cols, or the preview's when sampled
    int64_t pw = 0;                // sampled: the preview's columns
    double y_ratio = 1.0, x_ratio = 1.0;
    int64_t head = 0, quads = 0;   // pixels [0, head) precede the groups [head, head + 4 * quads)
    int in16 = 0, st16 = 0;        // a group of the sources / out_s is one 16-byte access
    const ComposeState *st = nullptr;
    int plain = 0;                 // the pick-and-pack of finished planes: no stage runs
    int scnr = 0, method = 0, preserve = 0;
    float amount = 0.0f;
    int l_stf = 0;                 // L goes through its transform (auto_stretch), else as it is
    float lw = 1.0f, cw = 1.0f;
    float *out_s[3] = {nullptr, nullptr, nullptr};  // all three or none
    uint8_t *out = nullptr;
};

struct FinishTx {
    ComposeStf tx[3];
    StfTx ltx;
};

template <bool SAMPLED>
__device__ __forceinline__ int64_t source_of(const FinishArgs &a, int64_t i) {
    if constexpr (SAMPLED) {
        const uint32_t dy = (uint32_t)i / (uint32_t)a.pw;  // (n < 2^31)
        const uint32_t dx = (uint32_t)i - dy * (uint32_t)a.pw;
        return nn_index((int64_t)dy, a.y_ratio, a.rows) * a.cols + nn_index((int64_t)dx, a.x_ratio, a.cols);
    } else {
        return i;
    }
}

// one pixel from the white-balanced values to the finished ones
template <bool LRGB>
__device__ __forceinline__ void finish_px(const FinishArgs &a, const FinishTx &t, float lv, float (&v)[3]) {
    if (a.plain) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = compose_stf_px(v[c], t.tx[c]);              // rgb.rs:299-304
    if (a.scnr) scnr_px(v[0], v[1], v[2], a.method, a.amount, a.preserve);          // :306-312
    if constexpr (LRGB) {
        const float ls = a.l_stf ? to_f32(lv, t.ltx) : lv;                          // cmd/compose/rgb.rs:130-138
        lrgb_px(ls, v[0], v[1], v[2], a.lw, a.cw);                                  // :140-147
    }
}

template <bool SAMPLED, bool LRGB>
__global__ __launch_bounds__(kBlock) void compose_finish_kernel(const FinishArgs a) {
    FinishTx t = {};
    if (!a.plain) {
#pragma unroll
        for (int c = 0; c < 3; ++c) t.tx[c] = a.st->tx[c];
        t.ltx = a.st->ltx;
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.quads; q += stride) {
        const int64_t i = a.head + 4 * q;
        float s[3][4], lv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (SAMPLED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t si = source_of<true>(a, i + k);
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c][k] = a.src[c][si];
                if constexpr (LRGB) lv[k] = a.l[si];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (a.in16) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.src[c] + i);
                    s[c][0] = v.x, s[c][1] = v.y, s[c][2] = v.z, s[c][3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[c][k] = a.src[c][i + k];
                }
            }
            if constexpr (LRGB) {
                if (a.in16) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.l + i);
                    lv[0] = v.x, lv[1] = v.y, lv[2] = v.z, lv[3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) lv[k] = a.l[i + k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float p[3] = {s[0][k], s[1][k], s[2][k]};
            finish_px<LRGB>(a, t, lv[k], p);
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c][k] = p[c];
        }
        if constexpr (!SAMPLED) {
            if (a.out_s[0]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (a.st16) {
                        *reinterpret_cast<float4 *>(a.out_s[c] + i) = make_float4(s[c][0], s[c][1], s[c][2], s[c][3]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k) a.out_s[c][i + k] = s[c][k];
                    }
                }
            }
        }
        if (a.out) {  // byte j = 3 k + c: four to a dword
            uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= quantise(s[c][k]) << (8 * ((3 * k + c) & 3));
            uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 3 * i);
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = d[j];
        }
    }
    // the pixels around the groups: one per lane, the first lanes of the grid
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        const int64_t si = source_of<SAMPLED>(a, i);
        float p[3], lv = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = a.src[c][si];
        if constexpr (LRGB) lv = a.l[si];
        finish_px<LRGB>(a, t, lv, p);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (!SAMPLED) {
                if (a.out_s[0]) a.out_s[c][i] = p[c];
            }
            if (a.out) a.out[3 * i + c] = (uint8_t)quantise(p[c]);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65)

int launch_wb_merge(ab_ctx *ctx, WbMergeArgs a) {
    a.head = head16(a.p[0], a.n);
    a.quads = (a.n - a.head) / 4;
    uintptr_t bits = a.comb ? (uintptr_t)(a.comb + a.head) : 0;
    for (int c = 0; c < 3; ++c) bits |= (uintptr_t)(a.p[c] + a.head);
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, a.n - 4 * a.quads));
    if ((bits & 15u) == 0) {
        hipLaunchKernelGGL(wb_merge_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(wb_merge_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// places the groups by the byte output's address and launches; everything else in `a` is the caller's
int launch_finish(ab_ctx *ctx, FinishArgs a, bool sampled) {
    a.head = a.out ? head_bytes(a.out, a.n) : 0;
    a.quads = (a.n - a.head) / 4;
    uintptr_t in_bits = a.l ? (uintptr_t)(a.l + a.head) : 0, st_bits = 0;
    for (int c = 0; c < 3; ++c) {
        in_bits |= (uintptr_t)(a.src[c] + a.head);
        if (a.out_s[c]) st_bits |= (uintptr_t)(a.out_s[c] + a.head);
    }
    a.in16 = !sampled && (in_bits & 15u) == 0;
    a.st16 = (st_bits & 15u) == 0;
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, a.n - 4 * a.quads));
    const bool lrgb = a.l != nullptr;
    if (sampled && lrgb) {
        hipLaunchKernelGGL((compose_finish_kernel<true, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else if (sampled) {
        hipLaunchKernelGGL((compose_finish_kernel<true, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else if (lrgb) {
        hipLaunchKernelGGL((compose_finish_kernel<false, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((compose_finish_kernel<false, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// one statistics chain of a device plane, its result saved at dst
int enqueue_stats(ab_ctx *ctx, const float *plane, int64_t n, ab_image_stats *dst) {
    const ab_image_stats *res = nullptr;
    AB_TRY(ab_stats_enqueue(ctx, nullptr, plane, n, n, 0, 0.0, 0.0, &kStfDefault, &res, nullptr, nullptr));
    hipLaunchKernelGGL(save_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, res, dst);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

}  // namespace

extern "C" {

int ab_compose_rgb(ab_ctx *ctx, const ab_plane *l, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_rgb_compose_config *cfg,
                   float lrgb_lightness, float lrgb_chrominance, int64_t max_dim, ab_plane_mut *out_pre, ab_plane_mut *out_planes, uint8_t *out_rgb8,
                   int32_t out_on_device, ab_compose_rgb_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, cfg, "null configuration");
    AB_CHECK(ctx, out_pre, "null pre-stretch output planes");
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    const ab_plane *ch[3] = {r, g, b};
    for (int c = 0; c < 3; ++c)
        if (ch[c]) AB_TRY(plane_check(ctx, ch[c], kChan[c]));
    if (l) AB_TRY(plane_check(ctx, l, "L"));
    ab_compose_dims dm;
    AB_TRY(ab_compose_front_check(ctx, ch, &dm));  // "Need at least 2 channels ...", "Channel dimension ratio ..."
    const int64_t rows = dm.rows, cols = dm.cols;
    AB_CHECK(ctx, fits31(rows, cols), "the composite of %lld x %lld holds 2^31 pixels or more", (long long)rows, (long long)cols);
    const int64_t n = rows * cols;
    AB_TRY(out_planes_check(ctx, out_pre, rows, cols));
    if (out_planes) AB_TRY(out_planes_check(ctx, out_planes, rows, cols));
    Preview pv;
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    const size_t nbytes = (size_t)(pv.ph * pv.pw) * 3;
    {
        std::vector<Span> ins, outs;
        for (int c = 0; c < 3; ++c) {
            if (ch[c]) ins.push_back(span_of(*ch[c]));
            outs.push_back(span_of(out_pre[c]));
            if (out_planes) outs.push_back(span_of(out_planes[c]));
        }
        if (l) ins.push_back(span_of(*l));
        if (out_rgb8) outs.push_back(Span{(uintptr_t)out_rgb8, nbytes, out_on_device != 0});
        AB_TRY(overlap_check(ctx, ins, outs));
    }
    const bool l_resampled = l && (l->rows != rows || l->cols != cols);  // cmd/compose/rgb.rs:124
    const bool auto_stretch = cfg->auto_stretch != 0, linked = auto_stretch && cfg->linked_stf != 0;

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    ComposeState *ws = nullptr;
    uint8_t *bytes_ws = nullptr;  // a host output's bytes on the device
    {
        constexpr size_t head = (sizeof(ComposeState) + 255) & ~(size_t)255;
        void *p = nullptr;
        AB_TRY(ab_workspace(ctx, AB_WS_COMPOSE, head + (out_rgb8 && !out_on_device ? nbytes : 0), &p));
        ws = (ComposeState *)p;
        bytes_ws = (uint8_t *)p + head;
    }
    // the front half: the channels land in out_pre
    const float *src[3] = {nullptr, nullptr, nullptr};
    float *tmp[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < 3; ++c) {
        if (!ch[c]) continue;
        AB_TRY(sc.stage_in(ch[c], &src[c]));
        if (dm.resample && !(ch[c]->rows == rows && ch[c]->cols == cols)) AB_TRY(sc.alloc((void **)&tmp[c], (size_t)n * sizeof(float)));
    }
    float *img[3];
    for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_out(&out_pre[c], &img[c]));
    double offset_g[2] = {0.0, 0.0}, offset_b[2] = {0.0, 0.0};
    AB_TRY(ab_compose_front_device(ctx, ch, src, &dm, tmp, cfg, img, offset_g, offset_b));

    // statistics before white balance (rgb.rs:243-249), the multipliers (:251-255)
    for (int c = 0; c < 3; ++c) AB_TRY(enqueue_stats(ctx, img[c], n, &ws->full[c]));
    double wb[3] = {1.0, 1.0, 1.0};
    ab_image_stats full[3];
    bool have_full = false;
    if (cfg->white_balance == 0) {
        void *pin = nullptr;
        AB_TRY(ab_pinned(ctx, sizeof full, &pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, ws->full, sizeof full, hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(full, pin, sizeof full);
        have_full = true;
        ab_select_wb_reference(&full[0], &full[1], &full[2], wb);
    } else if (cfg->white_balance == 1) {
        memcpy(wb, cfg->wb_manual, sizeof wb);
    }
    WbMergeArgs wa;
    wa.n = n;
    bool any_scaled = false;
    for (int c = 0; c < 3; ++c) {  // apply_multiplier_inplace (:127-130)
        wa.p[c] = img[c];
        wa.mult[c] = (float)wb[c];
        wa.scale[c] = std::fabs(wa.mult[c] - 1.0f) < 1e-7f ? 0 : 1;
        any_scaled = any_scaled || wa.scale[c];
    }
    if (linked) AB_TRY(sc.alloc((void **)&wa.comb, (size_t)n * sizeof(float)));
    if (any_scaled || linked) AB_TRY(launch_wb_merge(ctx, wa));

    // statistics after white balance (:261-291): an unscaled channel's are the ones already taken
    for (int c = 0; c < 3; ++c) {
        if (wa.scale[c]) {
            AB_TRY(enqueue_stats(ctx, img[c], n, &ws->wb[c]));
        } else {
            hipLaunchKernelGGL(save_stats_kernel, dim3(1), dim3(64), 0, ctx->stream, &ws->full[c], &ws->wb[c]);
            AB_HIP(ctx, hipGetLastError());
        }
    }
    if (linked) AB_TRY(enqueue_stats(ctx, wa.comb, n, &ws->comb));
    const float *l_dev = nullptr;
    if (l) {  // cmd/compose/rgb.rs:118-138
        AB_TRY(sc.stage_in(l, &l_dev));
        if (l_resampled) {
            float *lm = nullptr;
            AB_TRY(sc.alloc((void **)&lm, (size_t)n * sizeof(float)));
            AB_TRY(ab_resample_device(ctx, l_dev, l->rows, l->cols, rows, cols, lm));
            l_dev = lm;
        }
        if (auto_stretch) AB_TRY(enqueue_stats(ctx, l_dev, n, &ws->l));
    }
    ParamArgs pa;
    pa.auto_stretch = auto_stretch, pa.linked = linked, pa.has_l = l != nullptr;
    for (int c = 0; c < 3; ++c) pa.given[c] = cfg->has_stf[c] ? cfg->stf[c] : ab_stf_params{0.0, 0.5, 1.0};
    pa.stf_cfg = kStfDefault;
    hipLaunchKernelGGL(compose_params_kernel, dim3(1), dim3(64), 0, ctx->stream, ws, pa);
    AB_HIP(ctx, hipGetLastError());

    // the finish
    FinishArgs a;
    a.rows = rows, a.cols = cols, a.n = n, a.st = ws, a.l = l_dev;
    for (int c = 0; c < 3; ++c) a.src[c] = img[c];
    if (cfg->has_scnr) {  // apply_scnr_inplace's own clamp and threshold (scnr.rs:28-31)
        const float amount = cfg->scnr.amount < 0.0f ? 0.0f : (cfg->scnr.amount > 1.0f ? 1.0f : cfg->scnr.amount);
        if (!(amount < 1e-7f)) a.scnr = 1, a.method = cfg->scnr.method, a.amount = amount, a.preserve = cfg->scnr.preserve_luminance;
    }
    a.l_stf = auto_stretch, a.lw = lrgb_lightness, a.cw = lrgb_chrominance;
    if (out_planes) {
        for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_out(&out_planes[c], &a.out_s[c]));
    }
    uint8_t *bytes_dev = out_rgb8 ? (out_on_device ? out_rgb8 : bytes_ws) : nullptr;
    FinishArgs pick;  // the preview's geometry above max_dim
    pick.rows = rows, pick.cols = cols, pick.n = pv.ph * pv.pw, pick.pw = pv.pw;
    pick.y_ratio = (double)rows / (double)pv.ph, pick.x_ratio = (double)cols / (double)pv.pw;
    if (!pv.sampled) {  // one launch: planes and / or bytes
        a.out = bytes_dev;
        if (a.out || a.out_s[0]) AB_TRY(launch_finish(ctx, a, false));
    } else if (!out_planes) {  // one launch: only the pixels the preview picks
        if (bytes_dev) {
            a.n = pick.n, a.pw = pick.pw, a.y_ratio = pick.y_ratio, a.x_ratio = pick.x_ratio;
            a.out = bytes_dev;
            AB_TRY(launch_finish(ctx, a, true));
        }
    } else {  // the full-size planes, then a plain pick-and-pack of them
        AB_TRY(launch_finish(ctx, a, false));
        if (bytes_dev) {
            pick.plain = 1;
            for (int c = 0; c < 3; ++c) pick.src[c] = a.out_s[c];
            pick.out = bytes_dev;
            AB_TRY(launch_finish(ctx, pick, true));
        }
    }

    // ONE synchronisation: info and the host outputs
    char *pin = nullptr;
    bool wait = false;
    if (info) {
        AB_TRY(ab_pinned(ctx, sizeof(ComposeState), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, ws, sizeof(ComposeState), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (out_rgb8 && !out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_rgb8, bytes_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    AB_TRY(sc.enqueue_host_outs(&wait));
    if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        ComposeState st;
        memcpy(&st, pin, sizeof st);
        memset(info, 0, sizeof *info);
        ab_processed_rgb_info &pi = info->rgb;
        pi.rows = (uint64_t)rows, pi.cols = (uint64_t)cols;
        pi.resampled = dm.resample ? 1 : 0;
        pi.scnr_applied = cfg->has_scnr ? 1 : 0;
        for (int c = 0; c < 3; ++c) {
            const ab_image_stats &f = have_full ? full[c] : st.full[c];
            pi.chan_stats[c][0] = f.min, pi.chan_stats[c][1] = f.max, pi.chan_stats[c][2] = f.median, pi.chan_stats[c][3] = f.mean;
            pi.stf[c] = st.stf[c];
            pi.stats_wb[c] = st.wb[c];
        }
        memcpy(pi.offset_g, offset_g, sizeof offset_g);
        memcpy(pi.offset_b, offset_b, sizeof offset_b);
        info->preview_rows = (uint64_t)pv.ph, info->preview_cols = (uint64_t)pv.pw;
        info->lrgb_applied = l ? 1 : 0;
        info->l_resampled = l_resampled ? 1 : 0;
        if (l && auto_stretch) info->l_stats = st.l, info->l_stf = st.l_stf;
    }
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
