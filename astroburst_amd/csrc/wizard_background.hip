// The compose wizard's background step on gfx950: extract_background_cmd (cmd/processing/background.rs:17-94) from its loaded plane
// to the two PNG encoders' inputs and the JSON, and the mono preview that ends it and three other commands -- auto_stretch_preview
// (cmd/common.rs:18-22) followed by save_preview_png's nearest-neighbour pick (:152-193).
//
// save_preview_png picks downsample_nn::<1>'s pixels from bytes auto_stretch_preview made of EVERY pixel.  downsample_nn's dims
// (dst = ((n as f64) * scale).round().max(1.0), scale = max_dim / max(width, height), cmd/common.rs:162-164; both kept when both fit,
// :158-160) are cmd/helpers.rs:285-287's rule, which render.hip's preview_dims restates: ab_preview_dims gives a mono preview's dims
// as it gives a composite's.  Its pick, ((d as f64) * ratio).min((n - 1) as f64) as usize with ratio = n as f64 / dst as f64
// (:166-176), is entry_host.hpp's nn_index.
//   mono_preview_kernel  one or two planes of one size, each with its own transform (read from HBM, where the statistics chain left it)
//                        and its own output.  SAMPLED: a lane owns one output byte; a workgroup walks preview rows, the source row is
//                        found once per row (uniform), the source column once per lane for all its rows.  Not SAMPLED (every pixel is
//                        picked): stf.hip's map, four pixels per lane, one 16-byte load where the plane's address allows it, one dword
//                        of bytes stored behind a head placed by the OUTPUT's address.
//   model_range_kernel   background.hip's surface kernel (the same per-pixel body, background_device.hpp) that also reduces the minimum
//                        and maximum of the model's valid pixels (finite, > 1e-7: stats.rs:11-13) as bit patterns -- positive floats
//                        order like unsigned integers -- and counts them: shuffles in the wave, LDS across the four waves, one atomic
//                        per workgroup and word (the minimum as its complement, so that zeroed words mean "no valid pixel").  A
//                        workgroup walks rows, so the atomics number a few thousand whatever the plane's size.
// The step's chain: sampling and fit (background.hip), model_range_kernel, the model's median (its first synchronisation also lands
// the range words), the correction, the corrected plane's statistics chain, the model's with the range known (stats.rs:36-38: above
// 4 000 000 px it has no range pass), ONE mono_preview_kernel launch for both previews, one final synchronisation.
// -ffp-contract=off like everything else.
#include "ab_common.hpp"
#include "background_device.hpp"
#include "stf_device.hpp"
#include "entry_host.hpp"

#include <cmath>

namespace {

struct BgChan {  // what a statistics chain left in the context's state block, saved before the next chain overwrites it
    ab_image_stats stats;
    ab_stf_params stf;
    StfTx tx;
};

struct BgState {           // the head of AB_WS_BACKGROUND
    unsigned int enc[2];   // ~bits of the model's smallest valid pixel, bits of its largest; 0: no valid pixel
    unsigned int count;    // its valid pixels
    unsigned int pad;
    BgChan chan[2];        // [0] the corrected plane, [1] the model
};

__global__ void save_chan_kernel(const ab_image_stats *res, const ab_stf_params *stf, const StfTx *tx, BgChan *out) {
    if (threadIdx.x == 0) out->stats = *res, out->stf = *stf, out->tx = *tx;
}

// ---- the surface with its range -----------------------------------------------------------------------------------------------------
template <int DEG>
__global__ __launch_bounds__(kPolyBlock) void model_range_kernel(const PolyArgs p, float *__restrict__ model, int pow2_cols, double inv_cols,
                                                                 BgState *__restrict__ st) {
    __shared__ unsigned int part[3][kPolyBlock / 64];
    unsigned int lo = 0xffffffffu, hi = 0u, cnt = 0u;
    for (int y = blockIdx.y; y < p.rows; y += gridDim.y) {
        double cy[(DEG + 1) * (DEG + 2) / 2];
        poly_row_table<DEG>(p, y, cy);
#pragma unroll
        for (int u = 0; u < kPolyPx; ++u) {
            const int x = (blockIdx.x * kPolyPx + u) * kPolyBlock + threadIdx.x;
            if (x >= p.cols) continue;
            const float v = poly_px<DEG>(p, cy, x, pow2_cols, inv_cols);
            model[(size_t)y * p.cols + x] = v;
            if (is_valid_pixel(v)) {
                const unsigned int b = __float_as_uint(v);
                lo = b < lo ? b : lo;
                hi = b > hi ? b : hi;
                ++cnt;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
        cnt += __shfl_xor(cnt, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[0][wave] = ~lo, part[1][wave] = hi, part[2][wave] = cnt;
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned int m = 0u;
#pragma unroll
        for (int w = 0; w < kPolyBlock / 64; ++w) m = threadIdx.x == 2 ? m + part[2][w] : (part[threadIdx.x][w] > m ? part[threadIdx.x][w] : m);
        if (m) {
            if (threadIdx.x == 2)
                atomicAdd(&st->count, m);
            else
                atomicMax(&st->enc[threadIdx.x], m);
        }
    }
}

__global__ __launch_bounds__(kBlock) void correct_kernel(const float *__restrict__ img, const float *__restrict__ model, int64_t n, int mode,
                                                         float model_median, float *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = bg_apply_px(img[i], model[i], mode, model_median);
}

// ---- the mono preview ---------------------------------------------------------------------------------------------------------------
struct PreviewArgs {
    const float *src[2] = {nullptr, nullptr};
    const StfTx *tx[2] = {nullptr, nullptr};
    uint8_t *out[2] = {nullptr, nullptr};
    int planes = 1;
    int64_t rows = 0, cols = 0, ph = 0, pw = 0;  // SAMPLED: the pick
    double y_ratio = 1.0, x_ratio = 1.0;
    int64_t n = 0;                               // every pixel: pixels [0, head) precede the four-pixel groups of a plane
    int64_t head[2] = {0, 0}, quads[2] = {0, 0};
    int vec = 0;                                 // bit p: a group of plane p is one 16-byte load
};

template <bool SAMPLED>
__global__ __launch_bounds__(kBlock) void mono_preview_kernel(const PreviewArgs a) {
    if constexpr (SAMPLED) {
        const int64_t dx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        if (dx >= a.pw) return;
        const int64_t sx = nn_index(dx, a.x_ratio, a.cols);
        for (int p = 0; p < a.planes; ++p) {
            const StfTx t = *a.tx[p];
            const float *__restrict__ src = a.src[p];
            uint8_t *__restrict__ out = a.out[p];
            for (int64_t dy = blockIdx.y; dy < a.ph; dy += gridDim.y) {
                const int64_t sy = nn_index(dy, a.y_ratio, a.rows);  // (uniform: once per row of lanes)
                out[dy * a.pw + dx] = to_u8(src[sy * a.cols + sx], t);
            }
        }
    } else {
        const int64_t stride = (int64_t)gridDim.x * kBlock, t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        for (int p = 0; p < a.planes; ++p) {
            const StfTx t = *a.tx[p];
            const float *__restrict__ src = a.src[p];
            uint8_t *__restrict__ out = a.out[p];
            const int64_t head = a.head[p], quads = a.quads[p];
            for (int64_t q = t0; q < quads; q += stride) {
                const int64_t i = head + 4 * q;
                float v[4];
                if (a.vec & (1 << p)) {
                    const float4 f = *reinterpret_cast<const float4 *>(src + i);
                    v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = src[i + k];
                }
                uint32_t d = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) d |= (uint32_t)to_u8(v[k], t) << (8 * k);
                *reinterpret_cast<uint32_t *>(out + i) = d;
            }
            const int64_t loose = a.n - 4 * quads;  // the pixels around the groups: one per lane, the first lanes of the grid
            for (int64_t e = t0; e < loose; e += stride) {
                const int64_t i = e < head ? e : 4 * quads + e;
                out[i] = to_u8(src[i], t);
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65; common.rs:18-22)

// one launch for a.planes planes; a.src / a.tx / a.out are set
int launch_preview(ab_ctx *ctx, PreviewArgs a, int64_t rows, int64_t cols, const Preview &pv) {
    a.rows = rows, a.cols = cols, a.n = rows * cols;
    if (pv.sampled) {
        a.ph = pv.ph, a.pw = pv.pw;
        a.y_ratio = (double)rows / (double)pv.ph, a.x_ratio = (double)cols / (double)pv.pw;
        const int64_t gx = (pv.pw + kBlock - 1) / kBlock, cap = ab_stream_cap(ctx);
        const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(pv.ph, (cap + gx - 1) / gx));
        hipLaunchKernelGGL(mono_preview_kernel<true>, dim3((unsigned)gx, (unsigned)gy), dim3(kBlock), 0, ctx->stream, a);
    } else {
        int64_t lanes = 1;
        for (int p = 0; p < a.planes; ++p) {
            a.head[p] = std::min<int64_t>(a.n, (int64_t)((4 - (uintptr_t)a.out[p] % 4) % 4));  // the bytes before the output's first dword
            a.quads[p] = (a.n - a.head[p]) / 4;
            if (((uintptr_t)(a.src[p] + a.head[p]) & 15u) == 0) a.vec |= 1 << p;
            lanes = std::max<int64_t>(lanes, std::max<int64_t>(a.quads[p], a.n - 4 * a.quads[p]));
        }
        hipLaunchKernelGGL(mono_preview_kernel<false>, dim3(ab_stream_grid(ctx, lanes)), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// AB_WS_BACKGROUND: the state, then two previews' bytes bound for the host, then a model of n pixels nobody asked for
struct Carved {
    BgState *st = nullptr;
    uint8_t *bytes[2] = {nullptr, nullptr};
    float *model = nullptr;
};
int carve(ab_ctx *ctx, size_t bytes_each, bool want_model, int64_t n, Carved *w) {
    constexpr size_t head = 512;
    static_assert(sizeof(BgState) <= head, "the state fits its slot");
    const size_t bytes_al = (bytes_each + 255) & ~(size_t)255, plane_al = want_model ? (((size_t)n * sizeof(float) + 255) & ~(size_t)255) : 0;
    void *p = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_BACKGROUND, head + 2 * bytes_al + plane_al, &p));
    w->st = (BgState *)p;
    w->bytes[0] = (uint8_t *)p + head;
    w->bytes[1] = w->bytes[0] + bytes_al;
    w->model = want_model ? (float *)((char *)p + head + 2 * bytes_al) : nullptr;
    return AB_OK;
}

// plane_select.hip keeps its three 2048-bin histograms at the start of the context's pinned buffer; the model's range words land
// behind them, so the median's first synchronisation delivers both
constexpr size_t kSelectPinned = 3 * 2048 * sizeof(unsigned int);

template <int DEG>
void launch_model(ab_ctx *ctx, const PolyArgs &pa, float *model, int pow2_cols, double inv_cols, BgState *st) {
    const int64_t gx = ((int64_t)pa.cols + kPolyBlock * kPolyPx - 1) / (kPolyBlock * kPolyPx), cap = ab_stream_cap(ctx);
    const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(pa.rows, (cap + gx - 1) / gx));
    hipLaunchKernelGGL(model_range_kernel<DEG>, dim3((unsigned)gx, (unsigned)gy), dim3(kPolyBlock), 0, ctx->stream, pa, model, pow2_cols, inv_cols, st);
}

}  // namespace

extern "C" {

int ab_auto_stretch_preview_sampled(ab_ctx *ctx, const ab_plane *img, const ab_auto_stf_config *cfg, int64_t max_dim, uint8_t *out_u8, int32_t out_on_device,
                                    ab_image_stats *out_stats, ab_stf_params *out_stf) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img, "image"));
    AB_CHECK(ctx, out_u8, "null output bytes");
    const int64_t rows = img->rows, cols = img->cols, n = rows * cols;
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    Preview pv;  // (the image exceeds max_dim: the preview is a pick, cmd/common.rs:158-160)
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    const size_t nbytes = (size_t)(pv.ph * pv.pw);
    {
        std::vector<Span> ins{span_of(*img)}, outs{Span{(uintptr_t)out_u8, nbytes, out_on_device != 0}};
        AB_TRY(overlap_check(ctx, ins, outs));
    }

    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    Carved w;
    AB_TRY(carve(ctx, out_on_device ? 0 : nbytes, false, n, &w));
    PreviewArgs a;
    AB_TRY(sc.stage_in(img, &a.src[0]));
    const ab_image_stats *res = nullptr;
    const void *tx = nullptr;
    const ab_stf_params *stf = nullptr;
    AB_TRY(ab_stats_enqueue(ctx, nullptr, a.src[0], n, n, 0, 0.0, 0.0, cfg ? cfg : &kStfDefault, &res, &tx, &stf));
    a.tx[0] = (const StfTx *)tx;
    a.out[0] = out_on_device ? out_u8 : w.bytes[0];
    AB_TRY(launch_preview(ctx, a, rows, cols, pv));
    bool wait = false;
    char *pin = nullptr;
    if (out_stats || out_stf) {
        AB_TRY(ab_pinned(ctx, sizeof(ab_image_stats) + sizeof(ab_stf_params), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, res, sizeof(ab_image_stats), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipMemcpyAsync(pin + sizeof(ab_image_stats), stf, sizeof(ab_stf_params), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (!out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_u8, a.out[0], nbytes, hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out_stats) memcpy(out_stats, pin, sizeof *out_stats);
    if (out_stf) memcpy(out_stf, pin + sizeof(ab_image_stats), sizeof *out_stf);
    return AB_OK;
} AB_CATCH(ctx)

int ab_background_step(ab_ctx *ctx, const ab_plane *img, const ab_background_config *cfg, int64_t max_dim, ab_plane_mut *out_corrected, ab_plane_mut *out_model,
                       uint8_t *out_corrected_u8, uint8_t *out_model_u8, int32_t out_on_device, ab_background_step_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img, "image"));
    AB_CHECK(ctx, cfg, "null configuration");
    AB_CHECK(ctx, out_corrected && out_corrected->data, "null corrected plane");
    AB_CHECK(ctx, !out_model || out_model->data, "null model plane");
    const int64_t rows = img->rows, cols = img->cols, n = rows * cols;
    const ab_plane_mut *outs_p[2] = {out_corrected, out_model};
    const char *const what[2] = {"corrected", "model"};
    for (int k = 0; k < 2; ++k) {
        if (!outs_p[k]) continue;
        AB_CHECK(ctx, outs_p[k]->rows == rows && outs_p[k]->cols == cols, "the %s plane must be %lld x %lld (got %lld x %lld)", what[k], (long long)rows,
                 (long long)cols, (long long)outs_p[k]->rows, (long long)outs_p[k]->cols);
        AB_CHECK(ctx, ((uintptr_t)outs_p[k]->data & 3u) == 0, "the %s plane is not float-aligned", what[k]);
    }
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    Preview pv;  // (the image exceeds max_dim: the preview is a pick, cmd/common.rs:158-160)
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    const size_t nbytes = (size_t)(pv.ph * pv.pw);
    {
        std::vector<Span> ins{span_of(*img)}, outs;
        for (int k = 0; k < 2; ++k)
            if (outs_p[k]) outs.push_back(span_of(*outs_p[k]));
        if (out_corrected_u8) outs.push_back(Span{(uintptr_t)out_corrected_u8, nbytes, out_on_device != 0});
        if (out_model_u8) outs.push_back(Span{(uintptr_t)out_model_u8, nbytes, out_on_device != 0});
        AB_TRY(overlap_check(ctx, ins, outs));
    }
    AB_TRY(ab_background_check(ctx, rows, cols, cfg));
    const int degree = (int)cfg->poly_degree;

    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    Carved w;
    AB_TRY(carve(ctx, out_on_device ? 0 : nbytes, out_model == nullptr, n, &w));
    char *pin = nullptr;  // (the largest request first: the buffer is not reallocated under the copies below)
    AB_TRY(ab_pinned(ctx, kSelectPinned + std::max(sizeof(BgState), (size_t)64), (void **)&pin));
    const float *src = nullptr;
    AB_TRY(sc.stage_in(img, &src));

    // 1. sampling and fit: ab_extract_background's (ticks 1 and 2, its cancel points and errors)
    ab_background_fit fit;
    const int rc_fit = ab_background_sample_fit(ctx, src, rows, cols, cfg, &fit);
    if (rc_fit != AB_OK) {
        if (info) info->bg.sample_count = fit.sample_count;
        return rc_fit;
    }
    PolyArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.degree = degree;
    pa.rows = (int)rows;
    pa.cols = (int)cols;
    pa.row_scale = (double)rows;
    pa.col_scale = (double)cols;
    memcpy(pa.coeffs, fit.coeffs, sizeof pa.coeffs);

    // 2. the surface, with the range of its valid pixels
    AB_TRY(ab_progress(ctx, "generating model", 3, 4));  // background.rs:88-93
    float *model = w.model;
    if (out_model) {
        AB_TRY(sc.stage_out(out_model, &model));
    }
    AB_HIP(ctx, hipMemsetAsync(w.st, 0, 4 * sizeof(unsigned int), ctx->stream));
    {
        const int pow2_cols = (cols & (cols - 1)) == 0 ? 1 : 0;
        const double inv_cols = 1.0 / (double)cols;  // exact when cols is a power of two
        switch (degree) {  // 0 .. 5 (ab_background_check)
        case 0: launch_model<0>(ctx, pa, model, pow2_cols, inv_cols, w.st); break;
        case 1: launch_model<1>(ctx, pa, model, pow2_cols, inv_cols, w.st); break;
        case 2: launch_model<2>(ctx, pa, model, pow2_cols, inv_cols, w.st); break;
        case 3: launch_model<3>(ctx, pa, model, pow2_cols, inv_cols, w.st); break;
        case 4: launch_model<4>(ctx, pa, model, pow2_cols, inv_cols, w.st); break;
        default: launch_model<5>(ctx, pa, model, pow2_cols, inv_cols, w.st); break;
        }
    }
    AB_HIP(ctx, hipGetLastError());
    unsigned int *range_pin = (unsigned int *)(pin + kSelectPinned);
    AB_HIP(ctx, hipMemcpyAsync(range_pin, w.st, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    float model_median = 0.0f;
    ab_plane_sel msel;
    msel.data = model;
    msel.n = n;
    AB_TRY(ab_plane_median_f32(ctx, msel, &model_median, nullptr));  // (synchronises: the range words have landed)
    unsigned int enc[3];
    memcpy(enc, range_pin, sizeof enc);
    const bool has_valid = enc[2] != 0 && enc[0] != 0;
    const double known_min = has_valid ? (double)__builtin_bit_cast(float, ~enc[0]) : 0.0, known_max = has_valid ? (double)__builtin_bit_cast(float, enc[1]) : 0.0;
    const int use_known = has_valid && known_min < known_max ? 1 : 0;  // (a degenerate range: the statistics scan, stats.rs:36-38)

    // 3. the correction
    AB_TRY(ab_progress(ctx, "applying correction", 4, 4));  // background.rs:97-99
    float *corrected = nullptr;
    AB_TRY(sc.stage_out(out_corrected, &corrected));
    hipLaunchKernelGGL(correct_kernel, dim3(ab_stream_grid(ctx, n)), dim3(kBlock), 0, ctx->stream, src, model, n, (int)cfg->mode, model_median, corrected);
    AB_HIP(ctx, hipGetLastError());

    // 4. the statistics, once each: the corrected plane's (what :53 and :73 both compute), then the model's with its range known
    const float *plane[2] = {corrected, model};
    for (int k = 0; k < 2; ++k) {
        const ab_image_stats *res = nullptr;
        const void *tx = nullptr;
        const ab_stf_params *stf = nullptr;
        AB_TRY(ab_stats_enqueue(ctx, nullptr, plane[k], n, n, k == 1 ? use_known : 0, k == 1 ? known_min : 0.0, k == 1 ? known_max : 0.0, &kStfDefault, &res, &tx,
                                &stf));
        hipLaunchKernelGGL(save_chan_kernel, dim3(1), dim3(64), 0, ctx->stream, res, stf, (const StfTx *)tx, &w.st->chan[k]);
        AB_HIP(ctx, hipGetLastError());
    }

    // 5. both previews in one launch
    uint8_t *const u8_out[2] = {out_corrected_u8, out_model_u8};
    uint8_t *u8_dev[2] = {nullptr, nullptr};
    {
        PreviewArgs a;
        a.planes = 0;
        for (int k = 0; k < 2; ++k) {
            if (!u8_out[k]) continue;
            u8_dev[k] = out_on_device ? u8_out[k] : w.bytes[k];
            a.src[a.planes] = plane[k], a.tx[a.planes] = &w.st->chan[k].tx, a.out[a.planes] = u8_dev[k];
            ++a.planes;
        }
        if (a.planes) AB_TRY(launch_preview(ctx, a, rows, cols, pv));
    }

    // 6. one synchronisation for info and whatever is bound for the host
    bool wait = false;
    if (info) {
        AB_HIP(ctx, hipMemcpyAsync(pin, w.st, sizeof(BgState), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    for (int k = 0; k < 2; ++k)
        if (u8_out[k] && !out_on_device) {
            AB_HIP(ctx, hipMemcpyAsync(u8_out[k], u8_dev[k], nbytes, hipMemcpyDeviceToHost, ctx->stream));
            wait = true;
        }
    AB_TRY(sc.enqueue_host_outs(&wait));
    if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        BgState st;
        memcpy(&st, pin, sizeof st);
        memset(info, 0, sizeof *info);
        info->bg.sample_count = fit.sample_count;
        info->bg.rms_residual = fit.rms_residual;
        memcpy(info->bg.coeffs, fit.coeffs, sizeof info->bg.coeffs);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->preview_rows = (uint64_t)pv.ph, info->preview_cols = (uint64_t)pv.pw;
        info->corrected_stats = st.chan[0].stats, info->model_stats = st.chan[1].stats;
        info->corrected_stf = st.chan[0].stf, info->model_stf = st.chan[1].stf;
    }
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
