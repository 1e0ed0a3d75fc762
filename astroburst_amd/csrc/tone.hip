// The compose wizard's tone editor on gfx950: STF, levels, curves, SCNR and the preview packer behind one call.
//
// Replaces the pixel work of apply_tone_composite_cmd (cmd/processing/curves.rs:57-191) up to the PNG encoder: apply_stf_f32 x 3
// (:113-119), apply_levels_rgb (:121-131), apply_curve_rgb (:133-146), apply_scnr_inplace (:148-154) and render_rgb_preview
// (cmd/helpers.rs:204-262).  Every stage is pointwise (SCNR mixes the three channels of ONE pixel), and the command keeps no plane:
// only the preview's bytes leave it.  So one kernel family, templated on <LEVELS, CURVES, SAMPLED>, does per pixel
//   1 load      three f32 (SAMPLED: gathered through the preview's nearest-neighbour rule, helpers.rs:306-309)
//   2 STF       stf_device.hpp's to_f32                                        (stf.rs:104-120)
//   3 levels    color.hip's levels_kernel arithmetic, f64 with the same pow    (curves.rs:25-29, :46), a channel whose own
//               parameters are identity passes through untouched               (curves.rs:32-34: data.clone())
//   4 curves    color.hip's curve_kernel index arithmetic into the channel's LUT (curves.rs:105-109, :192)
//   5 SCNR      scnr_device.hpp's scnr_px                                      (scnr.rs:36-52)
//   6 planes    the three finished f32 planes, optionally stored (never when SAMPLED)
//   7 pack      (v.clamp(0, 1) * 255f32) as u8, interleaved R, G, B            (helpers.rs:243-245)
// in registers between the load and the stores: 12 B read and 3 B written per pixel against the 108 B of the eleven launches of the
// unfused chain.  Four pixels per lane, the scheme of rgb_export.hip's rgb_finish_kernel: one 16-byte load per plane where the
// addresses allow it, the 12 output bytes as three dwords placed by the OUTPUT address, the at most six pixels around the groups one
// per lane.  With CURVES the three LUTs (3 x 16 KiB) are staged into LDS once per workgroup of a persistent grid of at most three
// workgroups per CU (160 KiB of LDS per CU / 48 KiB): staging is paid a few hundred times per launch.  Those workgroups are 512 lanes
// wide, so that six waves per SIMD stand behind the three copies (256 lanes: 0.489 ms against 0.430 at 4096^2 with every stage on).
// Without CURVES no LDS is used and the workgroups are the usual 256 lanes, eight per CU.
// SAMPLED (an image above max_dim and no planes wanted) tones only the pixels the preview picks: lanes own four consecutive PREVIEW
// pixels, nothing of full size is read densely or allocated.
// Compiled with -ffp-contract=off like everything else: each stage is the instruction sequence of the kernel it restates, so the
// fused result is bit for bit what the library's own chain of entry points gives.
#include "ab_common.hpp"
#include "entry_host.hpp"
#include "scnr_device.hpp"
#include "stf_device.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kBlockCurves = 512;  // CURVES: twice the waves behind each 48 KiB copy of the LUTs
constexpr int kLut = 4096;
constexpr int kCurveGroupsPerCu = 3;  // 160 KiB of LDS per CU / the 48 KiB of three LUTs

struct ToneArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};
    int64_t rows = 0, cols = 0;    // of the source planes
    int64_t n = 0;                 // output pixels: rows * cols, or the preview's when sampled
    int64_t pw = 0;                // sampled: the preview's columns
    double y_ratio = 1.0, x_ratio = 1.0;
    int64_t head = 0, quads = 0;   // pixels [0, head) precede the groups [head, head + 4 * quads)
    int in16 = 0, st16 = 0;        // a group of the sources / out_s is one 16-byte access
    int stf = 0;                   // 0: the plain pick-and-pack of planes that are toned already
    StfTx tx[3] = {};
    int lev[3] = {0, 0, 0};        // the channel's levels are not identity
    double black[3] = {0.0, 0.0, 0.0}, inv_range[3] = {1.0, 1.0, 1.0}, inv_gamma[3] = {1.0, 1.0, 1.0};
    const float *lut = nullptr;    // CURVES: 3 x 4096 f32 on the device, 16-byte aligned
    int scnr = 0, method = 0, preserve = 0;
    float amount = 0.0f;
    float *out_s[3] = {nullptr, nullptr, nullptr};  // all three or none
    uint8_t *out = nullptr;
};

// where output pixel i is read from
template <bool SAMPLED>
__device__ __forceinline__ int64_t source_of(const ToneArgs &a, int64_t i) {
    if constexpr (SAMPLED) {
        const uint32_t dy = (uint32_t)i / (uint32_t)a.pw;  // (n < 2^31)
        const uint32_t dx = (uint32_t)i - dy * (uint32_t)a.pw;
        return nn_index((int64_t)dy, a.y_ratio, a.rows) * a.cols + nn_index((int64_t)dx, a.x_ratio, a.cols);
    } else {
        return i;
    }
}

// stages 2-5 of one pixel
template <bool LEVELS, bool CURVES>
__device__ __forceinline__ void tone_px(const ToneArgs &a, const float *lut, float (&v)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = a.stf ? to_f32(v[c], a.tx[c]) : v[c];
        if constexpr (LEVELS) {
            if (a.lev[c]) {
                float r = 0.0f;
                if (__builtin_isfinite(s) && !(s < 0.0f)) {                    // curves.rs:46
                    double norm = ((double)s - a.black[c]) * a.inv_range[c];  // curves.rs:27-29
                    norm = norm < 0.0 ? 0.0 : (norm > 1.0 ? 1.0 : norm);
                    r = (float)pow(norm, a.inv_gamma[c]);
                }
                s = r;
            }
        }
        if constexpr (CURVES) {
            float r = 0.0f;
            if (__builtin_isfinite(s) && !(s < 0.0f)) {                  // curves.rs:192
                const float t = fminf(fmaxf(s, 0.0f), 1.0f) * 4095.0f;  // curves.rs:105
                int idx = (int)t;                                       // `as usize` of a value in [0, 4095]
                idx = idx > 4095 ? 4095 : idx;
                r = lut[c * kLut + idx];
            }
            s = r;
        }
        v[c] = s;
    }
    if (a.scnr) scnr_px(v[0], v[1], v[2], a.method, a.amount, a.preserve);
}

template <bool LEVELS, bool CURVES, bool SAMPLED>
__global__ __launch_bounds__(CURVES ? kBlockCurves : kBlock) void tone_kernel(const ToneArgs a) {
    constexpr int kB = CURVES ? kBlockCurves : kBlock;
    const float *lut = nullptr;
    if constexpr (CURVES) {
        __shared__ float s_lut[3 * kLut];
        const float4 *g = reinterpret_cast<const float4 *>(a.lut);
        for (int i = threadIdx.x; i < 3 * kLut / 4; i += kB) reinterpret_cast<float4 *>(s_lut)[i] = g[i];
        __syncthreads();
        lut = s_lut;
    }
    const int64_t stride = (int64_t)gridDim.x * kB;
    for (int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x; q < a.quads; q += stride) {
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
                if (a.in16) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.src[c] + i);
                    s[c][0] = v.x, s[c][1] = v.y, s[c][2] = v.z, s[c][3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[c][k] = a.src[c][i + k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float p[3] = {s[0][k], s[1][k], s[2][k]};
            tone_px<LEVELS, CURVES>(a, lut, p);
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
    for (int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        const int64_t si = source_of<SAMPLED>(a, i);
        float p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = a.src[c][si];
        tone_px<LEVELS, CURVES>(a, lut, p);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (!SAMPLED) {
                if (a.out_s[0]) a.out_s[c][i] = p[c];
            }
            if (a.out) a.out[3 * i + c] = (uint8_t)quantise(p[c]);
        }
    }
}

// ---- host: the command's decisions -------------------------------------------------------------------------------------------
const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65)
const double kIdentityPoints[4] = {0.0, 0.0, 1.0, 1.0};  // identity_lut (cmd/processing/curves.rs:53-55)

bool levels_identity(const ab_levels_params &p) {  // LevelsParams::is_identity (core/imaging/curves.rs:18-22)
    return std::fabs(p.black) < 1e-7 && std::fabs(p.gamma - 1.0) < 1e-7 && std::fabs(p.white - 1.0) < 1e-7;
}

bool curve_identity(const double *xy, size_t n) {  // SplineLut::is_identity (core/imaging/curves.rs:94-103)
    if (n > 2) return false;
    if (n == 0) return true;
    if (n == 1) return std::fabs(xy[0] - xy[1]) < 1e-6;
    const bool near_start = std::fabs(xy[0]) < 1e-6 && std::fabs(xy[1]) < 1e-6;
    const bool near_end = std::fabs(xy[2] - 1.0) < 1e-6 && std::fabs(xy[3] - 1.0) < 1e-6;
    return near_start && near_end;
}

// cmd/processing/curves.rs:86-154 without the pixels; lut3x4096 nullable
int tone_plan(const ab_image_stats stats[3], const ab_tone_config *cfg, ab_tone_info *info, float *lut3x4096) {
    memset(info, 0, sizeof *info);
    if (cfg->linked_stf) {  // :89-91
        ab_stf_params p;
        ab_image_stats combined;
        const int rc = ab_compute_linked_stf(&stats[0], &stats[1], &stats[2], &kStfDefault, &p, &combined);
        if (rc != AB_OK) return rc;
        for (int c = 0; c < 3; ++c) info->stf[c] = p, info->norm[c] = combined;
    } else {  // :92-100
        for (int c = 0; c < 3; ++c) {
            const int rc = ab_auto_stf(&stats[c], &kStfDefault, &info->stf[c]);
            if (rc != AB_OK) return rc;
            info->norm[c] = stats[c];
        }
    }
    for (int c = 0; c < 3; ++c)  // :103-111
        if (cfg->has_stf[c]) info->stf[c] = cfg->stf[c];
    bool lev = false, cur = false;
    for (int c = 0; c < 3; ++c) {
        lev = lev || !levels_identity(cfg->levels[c]);                                      // :125
        cur = cur || (cfg->curve_xy[c] && !curve_identity(cfg->curve_xy[c], cfg->n_curve[c]));  // :133-136
    }
    info->levels_applied = lev ? 1 : 0;
    info->curves_applied = cur ? 1 : 0;
    if (cur && lut3x4096) {  // :139-141
        for (int c = 0; c < 3; ++c) {
            const int rc = cfg->curve_xy[c] ? ab_spline_lut_from_points(cfg->curve_xy[c], cfg->n_curve[c], lut3x4096 + c * kLut)
                                            : ab_spline_lut_from_points(kIdentityPoints, 2, lut3x4096 + c * kLut);
            if (rc != AB_OK) return rc;
        }
    }
    info->scnr_applied = cfg->has_scnr && cfg->scnr.amount > 1e-7f ? 1 : 0;  // :149
    return AB_OK;
}

// ---- host: checks, staging, launches -------------------------------------------------------------------------------------------
template <bool LEVELS, bool CURVES>
void launch_sampled(ab_ctx *ctx, int grid, bool sampled, const ToneArgs &a) {
    constexpr int block = CURVES ? kBlockCurves : kBlock;
    if (sampled) {
        hipLaunchKernelGGL((tone_kernel<LEVELS, CURVES, true>), dim3(grid), dim3(block), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((tone_kernel<LEVELS, CURVES, false>), dim3(grid), dim3(block), 0, ctx->stream, a);
    }
}

// places the groups by the byte output's address and launches; everything else in `a` is the caller's
int launch_tone(ab_ctx *ctx, ToneArgs a, bool levels, bool curves, bool sampled) {
    a.head = a.out ? head_bytes(a.out, a.n) : 0;
    a.quads = (a.n - a.head) / 4;
    uintptr_t in_bits = 0, st_bits = 0;
    for (int c = 0; c < 3; ++c) {
        in_bits |= (uintptr_t)(a.src[c] + a.head);
        if (a.out_s[c]) st_bits |= (uintptr_t)(a.out_s[c] + a.head);
    }
    a.in16 = !sampled && (in_bits & 15u) == 0;
    a.st16 = (st_bits & 15u) == 0;
    const int64_t lanes = std::max<int64_t>(a.quads, a.n - 4 * a.quads);
    // a persistent, grid-strided launch: at most three workgroups per CU hold the LUTs' 48 KiB of LDS each, eight otherwise (sizing the
    // grid by the runtime's occupancy answer per kernel instead -- two per CU where the f64 pow's registers leave room for no more --
    // measured the same within the run-to-run spread, so the fixed counts of the other streaming kernels stay)
    const int grid = ab_stream_grid(ctx, lanes, curves ? kBlockCurves : kBlock, curves ? kCurveGroupsPerCu : 8);
    if (levels && curves) {
        launch_sampled<true, true>(ctx, grid, sampled, a);
    } else if (levels) {
        launch_sampled<true, false>(ctx, grid, sampled, a);
    } else if (curves) {
        launch_sampled<false, true>(ctx, grid, sampled, a);
    } else {
        launch_sampled<false, false>(ctx, grid, sampled, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// The three LUTs on the device, without a synchronisation: they go through a pinned buffer of the context's own, which the host may
// rewrite once the event behind the last upload has passed (it has, long ago, when the next slider move arrives).  LUTs equal to the
// ones already there (an STF or SCNR slider moved) are not uploaded again.
int lut_upload(ab_ctx *ctx, const float *lut, const float **dev) {
    const size_t bytes = 3 * kLut * sizeof(float);
    void *d = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_TONE, bytes, &d));
    if (!ctx->tone_lut_host) AB_HIP(ctx, hipHostMalloc(&ctx->tone_lut_host, bytes, hipHostMallocDefault));
    if (!ctx->tone_lut_ev) AB_HIP(ctx, hipEventCreateWithFlags(&ctx->tone_lut_ev, hipEventDisableTiming));
    const bool current = ctx->tone_lut_ws == d && memcmp(ctx->tone_lut_host, lut, bytes) == 0;  // (the host copy only changes below)
    if (!current) {
        AB_HIP(ctx, hipEventSynchronize(ctx->tone_lut_ev));  // (at once for an event never recorded)
        ctx->tone_lut_ws = nullptr;
        memcpy(ctx->tone_lut_host, lut, bytes);
        AB_HIP(ctx, hipMemcpyAsync(d, ctx->tone_lut_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        AB_HIP(ctx, hipEventRecord(ctx->tone_lut_ev, ctx->stream));
        ctx->tone_lut_ws = d;
    }
    *dev = (const float *)d;
    return AB_OK;
}

// apply_tone_composite_cmd's pixel work.  restretch: restretch_composite_cmd (cmd/compose/rgb.rs:208-241) on the same kernel -- the
// caller has set explicit STFs and identity levels and curves; SCNR is decided by apply_scnr_inplace alone (a config that is present
// reaches it, rgb.rs:232-234; its own clamp and threshold are scnr.rs:28-31), not by the tone command's amount > 1e-7 (curves.rs:149):
// the two differ for a NaN amount, which apply_scnr_inplace lets through.
int tone_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats stats[3], const ab_tone_config *cfg,
                   int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device, ab_tone_info *info, bool restretch) {
    const ab_plane *ch[3] = {r, g, b};
    AB_TRY(same_dims_check(ctx, ch));  // (the command takes its dims from R, :80; its planes are one composite's)
    AB_CHECK(ctx, stats && cfg, "null statistics or configuration");
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    AB_CHECK(ctx, out_planes || out_rgb8, "nothing to do: out_planes and out_rgb8 are both null");
    const int64_t rows = r->rows, cols = r->cols, n = rows * cols;
    Preview pv;
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    const int64_t ph = pv.ph, pw = pv.pw;
    const bool above = pv.sampled;
    const size_t nbytes = (size_t)(ph * pw) * 3;
    if (out_planes) AB_TRY(out_planes_check(ctx, out_planes, rows, cols));
    const std::vector<Span> ins{device_span(*r), device_span(*g), device_span(*b)};
    AB_TRY(overlap_check(ctx, ins, {device_span(out_rgb8, nbytes, out_on_device)}));
    for (int o = 0; out_planes && o < 3; ++o)
        AB_TRY(overlap_check(ctx, ins, {device_span(out_planes[o].data, (size_t)n * sizeof(float), out_planes[o].on_device)}));
    ab_tone_info plan;
    std::vector<float> lut(3 * kLut);
    {
        const int rc = tone_plan(stats, cfg, &plan, lut.data());
        if (rc != AB_OK) return ab_set_error(ctx, rc, "the tone plan could not be computed");
    }
    if (restretch) {
        const float amount = cfg->scnr.amount < 0.0f ? 0.0f : (cfg->scnr.amount > 1.0f ? 1.0f : cfg->scnr.amount);  // scnr.rs:28
        plan.scnr_applied = cfg->has_scnr && !(amount < 1e-7f) ? 1 : 0;                                           // :29-31
    }
    plan.rows = (uint64_t)rows, plan.cols = (uint64_t)cols;
    plan.preview_rows = (uint64_t)ph, plan.preview_cols = (uint64_t)pw;

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    ToneArgs a;
    a.rows = rows, a.cols = cols, a.n = n;
    for (int c = 0; c < 3; ++c) {
        AB_TRY(sc.stage_in(ch[c], &a.src[c]));
        a.tx[c] = make_tx(&plan.stf[c], &plan.norm[c]);
        a.lev[c] = !levels_identity(cfg->levels[c]);
        if (a.lev[c]) {  // core/imaging/curves.rs:36-39
            const ab_levels_params &p = cfg->levels[c];
            const double range = std::fmax(p.white - p.black, 1e-15);
            a.black[c] = p.black;
            a.inv_range[c] = 1.0 / range;
            a.inv_gamma[c] = 1.0 / clampd_hd(p.gamma, 0.01, 10.0);
        }
    }
    a.stf = 1;
    if (plan.curves_applied) AB_TRY(lut_upload(ctx, lut.data(), &a.lut));
    if (plan.scnr_applied) {  // scnr.rs:28
        a.scnr = 1;
        a.method = cfg->scnr.method;
        a.amount = cfg->scnr.amount > 1.0f ? 1.0f : cfg->scnr.amount;
        a.preserve = cfg->scnr.preserve_luminance;
    }
    if (out_planes) {
        for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_out(&out_planes[c], &a.out_s[c]));
    }
    uint8_t *bytes_dev = nullptr;  // the caller's buffer, or the scratch arena for a host output (nothing below asks for scratch)
    if (out_rgb8) {
        if (out_on_device) {
            bytes_dev = out_rgb8;
        } else {
            AB_TRY(ab_scratch(ctx, nbytes, (void **)&bytes_dev));
        }
    }
    const bool lev = plan.levels_applied != 0, cur = plan.curves_applied != 0;
    if (!above) {  // one launch: planes and / or bytes
        a.out = bytes_dev;
        AB_TRY(launch_tone(ctx, a, lev, cur, false));
    } else if (!out_planes) {  // one launch: only the pixels the preview picks
        a.n = ph * pw, a.pw = pw;
        a.y_ratio = (double)rows / (double)ph, a.x_ratio = (double)cols / (double)pw;
        a.out = bytes_dev;
        AB_TRY(launch_tone(ctx, a, lev, cur, true));
    } else {  // the full-size planes, then a plain pick-and-pack of them
        AB_TRY(launch_tone(ctx, a, lev, cur, false));
        if (bytes_dev) {
            ToneArgs p;
            p.rows = rows, p.cols = cols, p.n = ph * pw, p.pw = pw;
            p.y_ratio = (double)rows / (double)ph, p.x_ratio = (double)cols / (double)pw;
            for (int c = 0; c < 3; ++c) p.src[c] = a.out_s[c];
            p.out = bytes_dev;
            AB_TRY(launch_tone(ctx, p, false, false, true));
        }
    }
    if (out_rgb8 && !out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_rgb8, bytes_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    AB_TRY(sc.finish_outs());
    if (info) *info = plan;
    return AB_OK;
}

}  // namespace

extern "C" {

void ab_tone_config_default(ab_tone_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    for (int c = 0; c < 3; ++c) {
        cfg->stf[c] = ab_stf_params{0.0, 0.5, 1.0};
        cfg->levels[c] = ab_levels_params{0.0, 1.0, 1.0};  // LevelsParams::default() (core/imaging/curves.rs:11-15)
    }
    cfg->scnr = ab_scnr_config{0, 1.0f, 0};
}

int ab_tone_plan(const ab_image_stats stats[3], const ab_tone_config *cfg, ab_tone_info *info, float *lut3x4096) try {
    if (!stats || !cfg || !info) return AB_ERR_INVALID;
    return tone_plan(stats, cfg, info, lut3x4096);
} AB_CATCH_NOCTX

int ab_apply_tone_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats stats[3], const ab_tone_config *cfg,
                            int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device, ab_tone_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    return tone_composite(ctx, r, g, b, stats, cfg, max_dim, out_planes, out_rgb8, out_on_device, info, false);
} AB_CATCH(ctx)

int ab_restretch_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats stats[3], const ab_stf_params stf[3],
                           int32_t has_scnr, const ab_scnr_config *scnr, int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8,
                           int32_t out_on_device) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, stf, "null STF parameters");
    AB_CHECK(ctx, !has_scnr || scnr, "has_scnr is set and the SCNR configuration is null");
    ab_tone_config cfg;
    ab_tone_config_default(&cfg);
    for (int c = 0; c < 3; ++c) cfg.has_stf[c] = 1, cfg.stf[c] = stf[c];  // cmd/compose/rgb.rs:224-230
    if (has_scnr) cfg.has_scnr = 1, cfg.scnr = *scnr;                     // :232-234
    return tone_composite(ctx, r, g, b, stats, &cfg, max_dim, out_planes, out_rgb8, out_on_device, nullptr, true);
} AB_CATCH(ctx)

}  // extern "C"
