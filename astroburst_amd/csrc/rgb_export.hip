// The colour finish on gfx950: drizzle RGB compose and the 8 / 16-bit RGB export renderers.
//
// Replaces core/compose/drizzle_rgb.rs (process_drizzle_rgb :41-145, drizzle_rgb :159-286 up to the PNG / FITS writers),
// infra/render/rgb.rs (render_rgb :7-47, render_rgb_16bit :49-91, each up to the encoder) and the pixel work of the export
// command's colour bodies (cmd/export/mod.rs:177-207, :287-328, :357-409).
//
// One kernel family, templated on the packer, does per pixel and channel
//   1 load        v = src[y * ld + x] (ld = the source's own column count: a top-left crop is a stride), 0 for an absent channel
//   2 balance     w = v * (float)wb, optionally stored                                    (drizzle_rgb.rs:82-84)
//   3 stretch     s = stf::apply_stf_f32's value (stf_device.hpp: to_f32, which multiplies by inv_clip -- NOT compose_rgb.hip's
//                 compose_stf_kernel, which divides by clip_range as rgb.rs:199-206 does)
//   4 SCNR        on the three s in registers (scnr_device.hpp)
//   5 planes      the three finished f32 planes, optionally stored
//   6 pack        interleaved R, G, B bytes: truncated u8, rounded u8, truncated big-endian u16
// so the finish of a picture reads its three planes once and writes only what the caller asked for: 12 B read + 3 / 6 B written per
// pixel against the 63 B of apply_stf_f32 x 3 + apply_scnr_inplace + a packer.  Four pixels per lane: one 16-byte load per plane where
// every source is uncropped and aligned, 12 / 24 output bytes as whole dwords wherever the OUTPUT address allows it (the groups are
// placed by it); the at most six pixels around the groups, or every pixel when a 16-bit output sits at an odd address, are done one
// per lane by the first lanes of the grid.  Any float-aligned plane and any byte address of an output are served.
#include "ab_common.hpp"
#include "entry_host.hpp"
#include "scnr_device.hpp"
#include "stf_device.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kPackNone = -1;

struct FinishArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};  // nullptr: an absent channel
    int64_t ld[3] = {0, 0, 0};
    int64_t cols = 0, n = 0;     // of the output
    int64_t head = 0, quads = 0;  // pixels [0, head) precede the groups [head, head + 4 * quads)
    int flat = 0;                 // every present source has ld == cols: pixel i is src[i]
    int in16 = 0, wb16 = 0, st16 = 0;  // a group of the sources / out_wb / out_s is one 16-byte access
    int has_wb = 0;
    float mult[3] = {1.0f, 1.0f, 1.0f};
    float *out_wb[3] = {nullptr, nullptr, nullptr};  // all three or none
    StfTx tx[3] = {};
    int scnr = 0, method = 0, preserve = 0;
    float amount = 0.0f;
    float *out_s[3] = {nullptr, nullptr, nullptr};  // all three or none
    uint8_t *out = nullptr;
};

__device__ __forceinline__ float load_px(const FinishArgs &a, int c, int64_t i) {
    const float *p = a.src[c];
    if (!p) return 0.0f;
    if (a.flat) return p[i];
    const uint32_t y = (uint32_t)i / (uint32_t)a.cols;  // (n < 2^31)
    return p[(int64_t)y * a.ld[c] + (int64_t)((uint32_t)i - y * (uint32_t)a.cols)];
}

// stages 2-4 of one pixel; w = what stage 2 leaves (for out_wb)
template <bool STF>
__device__ __forceinline__ void finish_px(const FinishArgs &a, float (&w)[3], float (&s)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.has_wb) w[c] = w[c] * a.mult[c];
        if constexpr (STF) {
            s[c] = to_f32(w[c], a.tx[c]);
        } else {
            s[c] = w[c];
        }
    }
    if (a.scnr) scnr_px(s[0], s[1], s[2], a.method, a.amount, a.preserve);
}

// (v.clamp(0, 1) * top) [.round()] as uN: f32::clamp keeps a NaN, `as` truncates, saturates and sends NaN to 0 (rgb.rs:29-31, :71-73,
// drizzle_rgb.rs:244-246); f32::round is half away from zero, written out for the x >= 0 that arrives here (x - trunc(x) is exact)
template <int PACK>
__device__ __forceinline__ uint32_t quantise_as(float s) {
    if constexpr (PACK == AB_RGB_PACK_8) return quantise(s);  // the truncated byte is the preview's
    const float c = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
    float x = c * (PACK == AB_RGB_PACK_16BE ? 65535.0f : 255.0f);
    if constexpr (PACK == AB_RGB_PACK_8_ROUND) {
        const float t = truncf(x);
        x = x - t >= 0.5f ? t + 1.0f : t;
    }
    return x == x ? (uint32_t)x : 0u;
}

__device__ __forceinline__ uint32_t be16(uint32_t q) { return (q >> 8) | ((q & 255u) << 8); }

__device__ __forceinline__ void store4(float *p, int wide, const float (&v)[4]) {
    if (wide) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = v[k];
    }
}

template <int PACK, bool STF>
__global__ __launch_bounds__(kBlock) void rgb_finish_kernel(const FinishArgs a) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.quads; q += stride) {
        const int64_t i = a.head + 4 * q;
        float w[3][4], s[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.in16) {
                const float4 v = a.src[c] ? *reinterpret_cast<const float4 *>(a.src[c] + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                w[c][0] = v.x, w[c][1] = v.y, w[c][2] = v.z, w[c][3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) w[c][k] = load_px(a, c, i + k);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pw[3] = {w[0][k], w[1][k], w[2][k]}, ps[3];
            finish_px<STF>(a, pw, ps);
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c][k] = pw[c], s[c][k] = ps[c];
        }
        if (a.out_wb[0]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) store4(a.out_wb[c] + i, a.wb16, w[c]);
        }
        if (a.out_s[0]) {
#pragma unroll
            for (int c = 0; c < 3; ++c) store4(a.out_s[c] + i, a.st16, s[c]);
        }
        if constexpr (PACK == AB_RGB_PACK_16BE) {  // sample j = 3 k + c: two to a dword, high byte first
            uint32_t d[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 1] |= be16(quantise_as<PACK>(s[c][k])) << (16 * ((3 * k + c) & 1));
            uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 6 * i);
#pragma unroll
            for (int j = 0; j < 6; ++j) o[j] = d[j];
        } else if constexpr (PACK != kPackNone) {  // byte j = 3 k + c: four to a dword
            uint32_t d[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= quantise_as<PACK>(s[c][k]) << (8 * ((3 * k + c) & 3));
            uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 3 * i);
#pragma unroll
            for (int j = 0; j < 3; ++j) o[j] = d[j];
        }
    }
    // the pixels around the groups: one per lane, the first lanes of the grid
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        float w[3], s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = load_px(a, c, i);
        finish_px<STF>(a, w, s);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.out_wb[0]) a.out_wb[c][i] = w[c];
            if (a.out_s[0]) a.out_s[c][i] = s[c];
            if constexpr (PACK == AB_RGB_PACK_16BE) {
                const uint32_t q = quantise_as<PACK>(s[c]);
                a.out[6 * i + 2 * c] = (uint8_t)(q >> 8);
                a.out[6 * i + 2 * c + 1] = (uint8_t)(q & 255u);
            } else if constexpr (PACK != kPackNone) {
                a.out[3 * i + c] = (uint8_t)quantise_as<PACK>(s[c]);
            }
        }
    }
}

// combined = ((r + g) + b) / 3.0f (drizzle_rgb.rs:90): a true f32 division, not merge_for_stf's multiplication by 1 / 3
__global__ __launch_bounds__(kBlock) void merge3_div_kernel(const float *__restrict__ r, const float *__restrict__ g, const float *__restrict__ b, int64_t n,
                                                            float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock; i < n; i += stride)
        out[i] = ((r[i] + g[i]) + b[i]) / 3.0f;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int pack_bytes(int32_t pack) { return pack == AB_RGB_PACK_16BE ? 6 : 3; }

int pack_check(ab_ctx *ctx, int32_t pack) {
    AB_CHECK(ctx, pack == AB_RGB_PACK_8 || pack == AB_RGB_PACK_8_ROUND || pack == AB_RGB_PACK_16BE, "unknown RGB packer %d", (int)pack);
    return AB_OK;
}

template <int PACK>
void launch_pack(ab_ctx *ctx, int grid, bool stf, const FinishArgs &a) {
    if (stf) {
        hipLaunchKernelGGL((rgb_finish_kernel<PACK, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((rgb_finish_kernel<PACK, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    }
}

// places the groups by the byte output's address (pack >= 0) and launches; a.src / ld / cols / n and the stage fields are the caller's
int launch_finish(ab_ctx *ctx, FinishArgs a, int pack, bool stf) {
    bool groups = true;
    a.head = 0;
    if (pack != kPackNone) {
        const uintptr_t addr = (uintptr_t)a.out;
        if (pack_bytes(pack) == 3) {
            a.head = head_bytes(a.out, a.n);
        } else if (addr & 1u) {
            groups = false;  // 6 head + addr is odd for every head
        } else {
            a.head = addr % 4 ? 1 : 0;
        }
    }
    a.head = groups ? std::min(a.head, a.n) : 0;
    a.quads = groups ? (a.n - a.head) / 4 : 0;
    a.flat = 1;
    uintptr_t in_bits = 0, wb_bits = 0, st_bits = 0;
    for (int c = 0; c < 3; ++c) {
        if (a.src[c]) {
            if (a.ld[c] != a.cols) a.flat = 0;
            in_bits |= (uintptr_t)(a.src[c] + a.head);
        }
        if (a.out_wb[c]) wb_bits |= (uintptr_t)(a.out_wb[c] + a.head);
        if (a.out_s[c]) st_bits |= (uintptr_t)(a.out_s[c] + a.head);
    }
    a.in16 = a.flat && (in_bits & 15u) == 0;
    a.wb16 = (wb_bits & 15u) == 0;
    a.st16 = (st_bits & 15u) == 0;
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, a.n - 4 * a.quads));
    switch (pack) {
        case AB_RGB_PACK_8: launch_pack<AB_RGB_PACK_8>(ctx, grid, stf, a); break;
        case AB_RGB_PACK_8_ROUND: launch_pack<AB_RGB_PACK_8_ROUND>(ctx, grid, stf, a); break;
        case AB_RGB_PACK_16BE: launch_pack<AB_RGB_PACK_16BE>(ctx, grid, stf, a); break;
        default: launch_pack<kPackNone>(ctx, grid, stf, a); break;
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// where the packed bytes land on the device: the caller's buffer, or the scratch arena for a host output (taken right before the
// launch: nothing after it may ask for scratch)
int bytes_begin(ab_ctx *ctx, void *out, int32_t out_on_device, size_t nbytes, uint8_t **dev) {
    if (out_on_device) {
        *dev = (uint8_t *)out;
        return AB_OK;
    }
    return ab_scratch(ctx, nbytes, (void **)dev);
}
int bytes_finish(ab_ctx *ctx, void *out, int32_t out_on_device, size_t nbytes, const uint8_t *dev) {
    if (out_on_device) return AB_OK;
    AB_HIP(ctx, hipMemcpyAsync(out, dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AB_OK;
}

// stages 3 + 6 (stf != nullptr) or 6 alone over three device planes of rows x cols
int render_device(ab_ctx *ctx, const float *const d[3], int64_t rows, int64_t cols, const ab_stf_params *stf, const ab_image_stats *stats, int32_t pack,
                  void *out, int32_t out_on_device) {
    FinishArgs a;
    a.cols = cols;
    a.n = rows * cols;
    for (int c = 0; c < 3; ++c) {
        a.src[c] = d[c];
        a.ld[c] = cols;
        if (stf) a.tx[c] = make_tx(&stf[c], &stats[c]);
    }
    const size_t nbytes = (size_t)a.n * (size_t)pack_bytes(pack);
    AB_TRY(bytes_begin(ctx, out, out_on_device, nbytes, &a.out));
    AB_TRY(launch_finish(ctx, a, pack, stf != nullptr));
    return bytes_finish(ctx, out, out_on_device, nbytes, a.out);
}

int render_planes(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_stf_params *stf, const ab_image_stats *stats, int32_t pack,
                  void *out, int32_t out_on_device) {
    const ab_plane *ch[3] = {r, g, b};
    AB_TRY(same_dims_check(ctx, ch));
    AB_TRY(pack_check(ctx, pack));
    AB_CHECK(ctx, out, "null output");
    const size_t nbytes = (size_t)(r->rows * r->cols) * (size_t)pack_bytes(pack);
    AB_TRY(overlap_check(ctx, {device_span(*r), device_span(*g), device_span(*b)}, {device_span(out, nbytes, out_on_device)}));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *d[3];
    for (int c = 0; c < 3; ++c) AB_TRY(sc.stage_in(ch[c], &d[c]));
    return render_device(ctx, d, r->rows, r->cols, stf, stats, pack, out, out_on_device);
}

const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65)

int out3_check(ab_ctx *ctx, const ab_plane_mut *o, int64_t rows, int64_t cols, const char *what) {
    if (!o) return AB_OK;
    for (int c = 0; c < 3; ++c) {
        AB_CHECK(ctx, o[c].data, "null %s %s plane", what, kChan[c]);
        AB_CHECK(ctx, o[c].rows == rows && o[c].cols == cols, "the %s %s plane must be %lld x %lld (got %lld x %lld)", what, kChan[c], (long long)rows,
                 (long long)cols, (long long)o[c].rows, (long long)o[c].cols);
        AB_CHECK(ctx, ((uintptr_t)o[c].data & 3u) == 0, "the %s %s plane is not float-aligned", what, kChan[c]);
    }
    return AB_OK;
}

int drizzle_cfg_check(ab_ctx *ctx, const ab_drizzle_rgb_config *cfg) {
    AB_CHECK(ctx, cfg, "null configuration");
    AB_CHECK(ctx, cfg->white_balance >= 0 && cfg->white_balance <= 2, "white_balance must be 0 (Auto), 1 (Manual) or 2 (None)");
    return AB_OK;
}

// process_drizzle_rgb (drizzle_rgb.rs:41-145) of device planes d[c] (nullptr: absent) of rows[c] x cols[c]; the arguments are checked
int process_device(ab_ctx *ctx, Scope &sc, const float *const d[3], const int64_t rows_c[3], const int64_t cols_c[3], const ab_drizzle_rgb_config *cfg,
                   ab_plane_mut *out_stretched, ab_plane_mut *out_wb, uint8_t *out_rgb8, int32_t out_on_device, ab_processed_drizzle_rgb_info *info) {
    int64_t rows = INT64_MAX, cols = INT64_MAX;  // :45-52
    for (int c = 0; c < 3; ++c)
        if (d[c]) rows = std::min(rows, rows_c[c]), cols = std::min(cols, cols_c[c]);
    const int64_t n = rows * cols;
    memset(info, 0, sizeof *info);
    info->rows = (uint64_t)rows;
    info->cols = (uint64_t)cols;
    // the white-balanced planes are materialised: in the caller's planes, else in scope slots
    float *wbp[3];
    for (int c = 0; c < 3; ++c) {
        if (out_wb) {
            AB_TRY(sc.stage_out(&out_wb[c], &wbp[c]));
        } else {
            AB_TRY(sc.alloc((void **)&wbp[c], (size_t)n * sizeof(float)));
        }
    }
    // :54-74 the statistics of the cropped, unscaled planes (they want a contiguous plane: a channel cropped in its columns is gathered
    // into its white-balance plane first, which the pass below then overwrites from the source through its stride)
    ab_image_stats full[3], wbst[3];
    FinishArgs wa;
    wa.cols = cols;
    wa.n = n;
    for (int c = 0; c < 3; ++c) {
        memset(&full[c], 0, sizeof full[c]);
        if (!d[c]) continue;  // :63-66 a zero plane: every statistic 0
        wa.src[c] = d[c];
        wa.ld[c] = cols_c[c];
        const float *contiguous = d[c];
        if (cols_c[c] != cols) {  // (fewer rows alone are a shorter plane, not a stride)
            AB_HIP(ctx, hipMemcpy2DAsync(wbp[c], (size_t)cols * sizeof(float), d[c], (size_t)cols_c[c] * sizeof(float), (size_t)cols * sizeof(float), (size_t)rows,
                                         hipMemcpyDeviceToDevice, ctx->stream));
            contiguous = wbp[c];
        }
        AB_TRY(ab_stats_device(ctx, contiguous, n, 0, 0.0, 0.0, &full[c]));
        info->chan_stats[c][0] = full[c].min, info->chan_stats[c][1] = full[c].max;
        info->chan_stats[c][2] = full[c].median, info->chan_stats[c][3] = full[c].mean;
    }
    double wb[3] = {1.0, 1.0, 1.0};  // :76-80
    if (cfg->white_balance == 0) {
        ab_select_wb_reference(&full[0], &full[1], &full[2], wb);
    } else if (cfg->white_balance == 1) {
        memcpy(wb, cfg->wb_manual, sizeof wb);
    }
    // :82-84 every channel is multiplied, even by 1 (stages 1 + 2)
    wa.has_wb = 1;
    for (int c = 0; c < 3; ++c) {
        info->wb[c] = wb[c];
        wa.mult[c] = (float)wb[c];
        wa.out_wb[c] = wbp[c];
    }
    AB_TRY(launch_finish(ctx, wa, kPackNone, false));
    auto stats_of = [&](int c) -> int {  // v * 1.0f is v: the statistics already taken
        if (wa.mult[c] == 1.0f) {
            wbst[c] = full[c];
            return AB_OK;
        }
        memset(&wbst[c], 0, sizeof wbst[c]);
        return ab_stats_device(ctx, wbp[c], n, 0, 0.0, 0.0, &wbst[c]);
    };
    for (int c = 0; c < 3; ++c) AB_TRY(stats_of(c));
    if (cfg->auto_stretch && cfg->linked_stf) {  // :89-96
        float *comb = nullptr;
        AB_TRY(sc.alloc((void **)&comb, (size_t)n * sizeof(float)));
        hipLaunchKernelGGL(merge3_div_kernel, dim3(ab_stream_grid(ctx, n)), dim3(kBlock), 0, ctx->stream, wbp[0], wbp[1], wbp[2], n, comb);
        AB_HIP(ctx, hipGetLastError());
        ab_image_stats st;
        memset(&st, 0, sizeof st);
        AB_TRY(ab_stats_device(ctx, comb, n, 0, 0.0, 0.0, &st));
        ab_stf_params p;
        ab_auto_stf(&st, &kStfDefault, &p);
        for (int c = 0; c < 3; ++c) info->stf[c] = p;
    } else if (cfg->auto_stretch) {  // :97-105
        for (int c = 0; c < 3; ++c) ab_auto_stf(&wbst[c], &kStfDefault, &info->stf[c]);
    } else {  // :106-116
        for (int c = 0; c < 3; ++c) info->stf[c] = ab_stf_params{0.0, 0.5, 1.0};
    }
    for (int c = 0; c < 3; ++c) info->stats_wb[c] = wbst[c];
    info->scnr_applied = cfg->has_scnr ? 1 : 0;  // :122-127 (true whenever a configuration is given)
    // :118-127 and the packer of :232-248: one launch (stages 1, 3, 4, 5, 6)
    if (out_stretched || out_rgb8) {
        FinishArgs fa;
        fa.cols = cols;
        fa.n = n;
        for (int c = 0; c < 3; ++c) {
            fa.src[c] = wbp[c];
            fa.ld[c] = cols;
            fa.tx[c] = make_tx(&info->stf[c], &wbst[c]);
            if (out_stretched) AB_TRY(sc.stage_out(&out_stretched[c], &fa.out_s[c]));
        }
        if (cfg->has_scnr) {  // scnr.rs:28-31
            const float amount = cfg->scnr.amount < 0.0f ? 0.0f : (cfg->scnr.amount > 1.0f ? 1.0f : cfg->scnr.amount);
            if (!(amount < 1e-7f)) {
                fa.scnr = 1;
                fa.method = cfg->scnr.method;
                fa.amount = amount;
                fa.preserve = cfg->scnr.preserve_luminance;
            }
        }
        const size_t nbytes = (size_t)n * 3;
        if (out_rgb8) AB_TRY(bytes_begin(ctx, out_rgb8, out_on_device, nbytes, &fa.out));
        AB_TRY(launch_finish(ctx, fa, out_rgb8 ? AB_RGB_PACK_8_ROUND : kPackNone, true));
        if (out_rgb8) AB_TRY(bytes_finish(ctx, out_rgb8, out_on_device, nbytes, fa.out));
    }
    return sc.finish_outs();
}

// the checks process_device relies on: output dims = the minimum per axis over the present channels, n < 2^31
int process_check(ab_ctx *ctx, const int64_t rows_c[3], const int64_t cols_c[3], const bool present[3], const ab_drizzle_rgb_config *cfg,
                  const ab_plane_mut *out_stretched, const ab_plane_mut *out_wb, const ab_processed_drizzle_rgb_info *info) {
    AB_TRY(drizzle_cfg_check(ctx, cfg));
    AB_CHECK(ctx, info, "null info");
    int64_t rows = INT64_MAX, cols = INT64_MAX;
    for (int c = 0; c < 3; ++c)
        if (present[c]) rows = std::min(rows, rows_c[c]), cols = std::min(cols, cols_c[c]);
    AB_CHECK(ctx, rows != INT64_MAX, "at least one channel must be present");
    AB_CHECK(ctx, fits31(rows, cols), "the output holds 2^31 pixels or more");
    AB_TRY(out3_check(ctx, out_stretched, rows, cols, "stretched"));
    AB_TRY(out3_check(ctx, out_wb, rows, cols, "white-balanced"));
    return AB_OK;
}

// the output's pixel count (after process_check)
int64_t info_dims(const int64_t rows_c[3], const int64_t cols_c[3], const bool present[3]) {
    int64_t rows = INT64_MAX, cols = INT64_MAX;
    for (int c = 0; c < 3; ++c)
        if (present[c]) rows = std::min(rows, rows_c[c]), cols = std::min(cols, cols_c[c]);
    return rows * cols;
}

}  // namespace

extern "C" {

int ab_rgb_packed_bytes(int64_t rows, int64_t cols, int32_t pack, size_t *bytes) try {
    if (!bytes || rows < 1 || cols < 1 || !fits31(rows, cols)) return AB_ERR_INVALID;
    if (pack != AB_RGB_PACK_8 && pack != AB_RGB_PACK_8_ROUND && pack != AB_RGB_PACK_16BE) return AB_ERR_INVALID;
    *bytes = (size_t)(rows * cols) * (size_t)pack_bytes(pack);
    return AB_OK;
} AB_CATCH_NOCTX

int ab_render_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, int32_t pack, void *out, int32_t out_on_device) try {
    if (!ctx) return AB_ERR_INVALID;
    return render_planes(ctx, r, g, b, nullptr, nullptr, pack, out, out_on_device);
} AB_CATCH(ctx)

int ab_render_rgb_stf(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_stf_params stf[3], const ab_image_stats stats[3],
                      int32_t pack, void *out, int32_t out_on_device) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, stf && stats, "null STF parameters or statistics");
    return render_planes(ctx, r, g, b, stf, stats, pack, out, out_on_device);
} AB_CATCH(ctx)

int ab_export_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_rgb_export_config *cfg, void *out, int32_t out_on_device,
                  ab_rgb_export_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    for (int c = 0; c < 3; ++c) AB_TRY(plane_check(ctx, ch[c], kChan[c]));
    AB_CHECK(ctx, cfg && out && info, "null argument");
    AB_CHECK(ctx, cfg->bits == 8 || cfg->bits == 16, "bits must be 8 or 16 (got %d)", (int)cfg->bits);
    const int32_t pack = cfg->bits == 16 ? AB_RGB_PACK_16BE : AB_RGB_PACK_8;
    int64_t rows = 0, cols = 0;  // export/mod.rs:396-398
    for (int c = 0; c < 3; ++c) rows = std::max(rows, ch[c]->rows), cols = std::max(cols, ch[c]->cols);
    AB_CHECK(ctx, fits31(rows, cols), "the output holds 2^31 pixels or more");
    const int64_t n = rows * cols;
    const size_t nbytes = (size_t)n * (size_t)pack_bytes(pack);
    AB_TRY(overlap_check(ctx, {device_span(*r), device_span(*g), device_span(*b)}, {device_span(out, nbytes, out_on_device)}));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    memset(info, 0, sizeof *info);
    info->rows = (uint64_t)rows;
    info->cols = (uint64_t)cols;
    Scope sc(ctx);
    const float *d[3];
    for (int c = 0; c < 3; ++c) {
        AB_TRY(sc.stage_in(ch[c], &d[c]));
        if (ch[c]->rows != rows || ch[c]->cols != cols) {  // :399-405
            float *h = nullptr;
            AB_TRY(sc.alloc((void **)&h, (size_t)n * sizeof(float)));
            AB_TRY(ab_resample_device(ctx, d[c], ch[c]->rows, ch[c]->cols, rows, cols, h));
            d[c] = h;
            info->resampled = 1;
        }
    }
    for (int c = 0; c < 3; ++c) AB_TRY(ab_stats_device(ctx, d[c], n, 0, 0.0, 0.0, &info->stats[c]));  // :358-360
    if (cfg->has_stf) {  // :362-370
        for (int c = 0; c < 3; ++c) info->stf[c] = cfg->stf[c];
    } else {  // :371-378
        ab_stf_params linked;
        AB_CHECK(ctx, ab_compute_linked_stf(&info->stats[0], &info->stats[1], &info->stats[2], &kStfDefault, &linked, nullptr) == AB_OK,
                 "the linked STF could not be computed");
        for (int c = 0; c < 3; ++c) info->stf[c] = linked;
    }
    return render_device(ctx, d, rows, cols, info->stf, info->stats, pack, out, out_on_device);  // :381-382
} AB_CATCH(ctx)

int ab_process_drizzle_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_drizzle_rgb_config *cfg, ab_plane_mut *out_stretched,
                           ab_plane_mut *out_wb, uint8_t *out_rgb8, int32_t out_on_device, ab_processed_drizzle_rgb_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    int64_t rows_c[3] = {0, 0, 0}, cols_c[3] = {0, 0, 0};
    bool present[3];
    for (int c = 0; c < 3; ++c) {
        present[c] = ch[c] != nullptr;
        if (!present[c]) continue;
        AB_TRY(plane_check(ctx, ch[c], kChan[c]));
        rows_c[c] = ch[c]->rows, cols_c[c] = ch[c]->cols;
    }
    AB_TRY(process_check(ctx, rows_c, cols_c, present, cfg, out_stretched, out_wb, info));
    const size_t on = (size_t)info_dims(rows_c, cols_c, present);
    std::vector<Span> ins;
    for (int c = 0; c < 3; ++c)
        if (present[c]) ins.push_back(device_span(*ch[c]));
    AB_TRY(overlap_check(ctx, ins, {device_span(out_rgb8, on * 3, out_on_device)}));
    for (int o = 0; o < 3; ++o) {
        if (out_stretched) AB_TRY(overlap_check(ctx, ins, {device_span(out_stretched[o].data, on * sizeof(float), out_stretched[o].on_device)}));
        if (out_wb) AB_TRY(overlap_check(ctx, ins, {device_span(out_wb[o].data, on * sizeof(float), out_wb[o].on_device)}));
    }
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *d[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < 3; ++c)
        if (present[c]) AB_TRY(sc.stage_in(ch[c], &d[c]));
    return process_device(ctx, sc, d, rows_c, cols_c, cfg, out_stretched, out_wb, out_rgb8, out_on_device, info);
} AB_CATCH(ctx)

int ab_drizzle_rgb(ab_ctx *ctx, const ab_plane *r_frames, size_t n_r, const ab_plane *g_frames, size_t n_g, const ab_plane *b_frames, size_t n_b,
                   const ab_drizzle_config *dcfg, const ab_drizzle_rgb_config *cfg, ab_plane_mut *out_wb, uint8_t *out_rgb8, int32_t out_on_device,
                   ab_drizzle_result res[3], ab_processed_drizzle_rgb_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, dcfg && res && info, "null argument");
    AB_TRY(drizzle_cfg_check(ctx, cfg));
    const ab_plane *lists[3] = {r_frames, g_frames, b_frames};
    const size_t counts[3] = {n_r, n_g, n_b};
    const int given = (r_frames != nullptr) + (g_frames != nullptr) + (b_frames != nullptr);
    memset(res, 0, 3 * sizeof *res);
    if (given < 2) return ab_set_error(ctx, AB_ERR_INVALID, "Need at least 2 channels for RGB drizzle (got %d)", given);  // :171-173
    bool present[3];
    int64_t rows_c[3] = {0, 0, 0}, cols_c[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {  // :178 a list of fewer than two frames is no channel
        present[c] = lists[c] && counts[c] >= 2;
        if (!present[c]) continue;
        const int rc = ab_drizzle_output_dims(lists[c], counts[c], dcfg, nullptr, nullptr, &rows_c[c], &cols_c[c]);
        if (rc != AB_OK) return ab_set_error(ctx, rc, "the %s frames cannot be drizzled (frame dimensions vary too much, too many frames, or a NaN scale / pixfrac)", kChan[c]);
    }
    if (!present[0] && !present[1] && !present[2]) return ab_set_error(ctx, AB_ERR_INVALID, "All channels failed or have fewer than 2 frames");  // :203-205
    AB_TRY(process_check(ctx, rows_c, cols_c, present, cfg, nullptr, out_wb, info));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    // each channel's drizzle stays in HBM: scope slots 5 .. 7 (process_device takes at most four from slot 0)
    const float *d[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < 3; ++c) {
        if (!present[c]) continue;
        float *img = nullptr;
        AB_TRY(ab_workspace(ctx, AB_WS_SCOPE5 + c, (size_t)(rows_c[c] * cols_c[c]) * sizeof(float), (void **)&img));
        ab_plane_mut pm{img, rows_c[c], cols_c[c], 1};
        AB_TRY(ab_drizzle_stack(ctx, lists[c], counts[c], dcfg, &pm, nullptr, nullptr, &res[c]));
        d[c] = img;
    }
    Scope sc(ctx);
    return process_device(ctx, sc, d, rows_c, cols_c, cfg, nullptr, out_wb, out_rgb8, out_on_device, info);
} AB_CATCH(ctx)

}  // extern "C"
