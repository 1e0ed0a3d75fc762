// Opening a file on gfx950: the preview bytes and the display histogram of process_fits / process_fits_full / process_rgb_fits.
//
// Replaces the pixel work of cmd/io/mod.rs:33-172 (and of compute_histogram, cmd/analysis/mod.rs:22-53) up to the PNG encoder and the
// JSON: compute_image_stats -> auto_stf -> apply_stf (cmd/io/mod.rs:25-27), compute_histogram_with_stats (stats.rs:373-376) ->
// downsample_histogram (:423-444), and for an RGB file compute_image_stats x 3 -> auto_stf x 3 -> apply_stf_f32 x 3 ->
// render_rgb_preview (cmd/io/mod.rs:44-62, cmd/helpers.rs:204-262) with the display histogram of R.
//
// The statistics chain (stats.hip: ab_stats_enqueue) leaves ImageStats, the STF parameters and the StfTx in the context's state block
// in HBM without a synchronisation.  The kernels here read them from there, so a whole command is one chain and at most one
// synchronisation (none when every output stays on the device and the caller wants no scalars):
//   view_mono_kernel  per pixel: one load, the apply_stf byte (stf_device.hpp's to_u8) and / or one more count in the display
//                     histogram.  4 B read and 1 B written per pixel.
//   view_rgb_kernel   per pixel: three loads, apply_stf_f32 per channel (to_f32), the preview's byte (v.clamp(0, 1) * 255f32) as u8
//                     interleaved, and -- when every pixel is visited -- R's count in the display histogram.  12 B read, 3 B written.
//                     An image above max_dim tones only the pixels the preview picks (tone.hip's SAMPLED form); R's histogram is
//                     then one view_mono_kernel pass over R.
// The display histogram.  The reference builds 65 536 bins and folds them (downsample_histogram).  When the display count T divides
// 65 536 the fold is a shift of the bin index, so the T bins are accumulated directly: in LDS, one copy per wave up to 1024 bins (one
// copy per workgroup up to 16 384), flushed with one global add per non-empty bin and workgroup.  No 65 536-bin intermediate exists and
// the plane is read once.  Any other T < 65 536 (and the divisors 32 768 and 65 536, which do not fit in LDS as u32) counts the 65 536
// bins on the device with global adds and folds them there with the reference's own index arithmetic, dropped top bin included
// (fold_kernel).  Hot bins: view_hist.hpp.
// Loads are 16 bytes wide behind a scalar head, so any float-aligned plane works; bytes leave as whole dwords where the output
// address allows it.  Persistent grids sized from the context's CU count.  -ffp-contract=off like everything else: each stage is the
// instruction sequence of the kernel it restates, so bytes and bins equal the library's own unfused calls bit for bit.
#include "ab_common.hpp"
#include "entry_host.hpp"
#include "stf_device.hpp"
#include "view_hist.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kPerWaveMax = 1024;  // display bins up to which every wave owns a copy (4 x 4 KiB)
constexpr int kLdsMax = 16384;     // ... up to which the workgroup owns one (64 KiB)
// how lanes that share a bin are added (view_hist.hpp; LABNOTES.md has the measurement behind the choice)
constexpr int kHistMode = 1;

struct ViewChan {  // what one channel's statistics chain left in the state block, saved before the next chain overwrites it
    ab_image_stats stats;
    ab_stf_params stf;
    StfTx tx;
};

struct HistArgs {
    const ab_image_stats *st_dev = nullptr;  // [dmin, dmax] = the statistics' min / max read from HBM; else the two below
    double dmin = 0.0, dmax = 0.0;
    unsigned int *bins = nullptr;  // the t display bins, or the 65 536 when t == 0 (both cleared before the launch)
    int t = 0;                     // display bins accumulated in LDS; 0: the 65 536 bins, global adds
    int copies = 1;                // LDS copies of the t bins: one per wave or one
    int shift = 0;                 // display bin = 65 536-bin index >> shift
};

// false: the reference returns zero bins (stats.rs:379-387), decided here from what the statistics chain left
__device__ __forceinline__ bool hist_begin(const HistArgs &h, unsigned int *lds, double *dmin, double *inv) {
    const double lo = h.st_dev ? h.st_dev->min : h.dmin, hi = h.st_dev ? h.st_dev->max : h.dmax;
    const double range = hi - lo;
    if (range < 1e-10) return false;
    *dmin = lo;
    *inv = (double)kViewSrcBins / range;  // stats.rs:389
    if (h.t) {
        for (int i = threadIdx.x; i < h.t * h.copies; i += kBlock) lds[i] = 0;
        __syncthreads();
    }
    return true;
}

__device__ __forceinline__ void hist_px(const HistArgs &h, unsigned int *mine, float v, double dmin, double inv) {
    const bool valid = is_valid_pixel(v);  // stats.rs:397
    const uint32_t b = view_bin(v, dmin, inv);
    if (h.t) {
        view_hist_add<kHistMode>(mine, valid, b >> h.shift);
    } else if (valid) {
        atomicAdd(&h.bins[b], 1u);
    }
}

__device__ __forceinline__ void hist_end(const HistArgs &h, const unsigned int *lds) {
    if (!h.t) return;
    __syncthreads();
    for (int i = threadIdx.x; i < h.t; i += kBlock) {
        unsigned int s = 0;
        for (int c = 0; c < h.copies; ++c) s += lds[c * h.t + i];
        if (s) atomicAdd(&h.bins[i], s);
    }
}

struct MonoArgs {
    const float *src = nullptr;
    int64_t n = 0;
    int64_t head = 0, quads = 0;  // pixels [0, head) precede the 16-byte groups [head, head + 4 * quads)
    const StfTx *tx_dev = nullptr;
    uint8_t *out = nullptr;
    int out4 = 0;  // a group's four bytes are one aligned dword
    HistArgs hist;
};

template <bool U8, bool HIST>
__global__ __launch_bounds__(kBlock) void view_mono_kernel(const MonoArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
    StfTx t = {};
    if constexpr (U8) t = *a.tx_dev;
    bool hist = false;
    double dmin = 0.0, inv = 0.0;
    if constexpr (HIST) hist = hist_begin(a.hist, lds, &dmin, &inv);
    if (!U8 && !hist) return;
    unsigned int *mine = lds + (a.hist.copies > 1 ? (threadIdx.x >> 6) * a.hist.t : 0);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < a.quads; q += stride) {
        const int64_t i = a.head + 4 * q;
        const float4 v4 = *reinterpret_cast<const float4 *>(a.src + i);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        if constexpr (U8) {
            if (a.out4) {
                uchar4 r;
                r.x = to_u8(v[0], t), r.y = to_u8(v[1], t), r.z = to_u8(v[2], t), r.w = to_u8(v[3], t);
                *reinterpret_cast<uchar4 *>(a.out + i) = r;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) a.out[i + k] = to_u8(v[k], t);
            }
        }
        if constexpr (HIST) {
            if (hist) {
#pragma unroll
                for (int k = 0; k < 4; ++k) hist_px(a.hist, mine, v[k], dmin, inv);
            }
        }
    }
    // the pixels around the groups: one per lane, the first lanes of the grid
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        const float v = a.src[i];
        if constexpr (U8) a.out[i] = to_u8(v, t);
        if constexpr (HIST) {
            if (hist) hist_px(a.hist, mine, v, dmin, inv);
        }
    }
    if constexpr (HIST) {
        if (hist) hist_end(a.hist, lds);
    }
}

// downsample_histogram (stats.rs:430-441) of the 65 536 bins: out[i] = the saturating sum of src[(i as f64 * ratio) as usize ..
// min(((i + 1) as f64 * ratio) as usize, 65536))
__global__ __launch_bounds__(kBlock) void fold_kernel(const unsigned int *__restrict__ src, uint32_t target, unsigned int *__restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= target) return;
    const double ratio = (double)kViewSrcBins / (double)target;
    const uint32_t start = (uint32_t)((double)i * ratio);
    uint32_t end = (uint32_t)((double)(i + 1) * ratio);
    end = end < (uint32_t)kViewSrcBins ? end : (uint32_t)kViewSrcBins;
    unsigned long long s = 0;
    for (uint32_t j = start; j < end; ++j) s += src[j];
    out[i] = s > 0xffffffffull ? 0xffffffffu : (unsigned int)s;
}

// the device-to-device copy of one channel's result out of the state block
__global__ void save_chan_kernel(const ab_image_stats *st, const ab_stf_params *stf, const StfTx *tx, ViewChan *dst) {
    if (threadIdx.x == 0) {
        dst->stats = *st;
        dst->stf = *stf;
        dst->tx = *tx;
    }
}

struct RgbArgs {
    const float *src[3] = {nullptr, nullptr, nullptr};
    int64_t rows = 0, cols = 0;   // of the source planes
    int64_t n = 0;                // output pixels: rows * cols, or the preview's when sampled
    int64_t pw = 0;               // sampled: the preview's columns
    double y_ratio = 1.0, x_ratio = 1.0;
    int64_t head = 0, quads = 0;  // placed by the OUTPUT address: the 12 bytes of a group are three aligned dwords
    int in16 = 0;                 // a group of every source is one 16-byte load
    const ViewChan *chan = nullptr;
    uint8_t *out = nullptr;
    HistArgs hist;
};

template <bool SAMPLED>
__device__ __forceinline__ int64_t source_of(const RgbArgs &a, int64_t i) {
    if constexpr (SAMPLED) {
        const uint32_t dy = (uint32_t)i / (uint32_t)a.pw;  // (n < 2^31)
        const uint32_t dx = (uint32_t)i - dy * (uint32_t)a.pw;
        return nn_index((int64_t)dy, a.y_ratio, a.rows) * a.cols + nn_index((int64_t)dx, a.x_ratio, a.cols);
    } else {
        return i;
    }
}

template <bool SAMPLED, bool HIST>
__global__ __launch_bounds__(kBlock) void view_rgb_kernel(const RgbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned int lds[];
    const StfTx tx[3] = {a.chan[0].tx, a.chan[1].tx, a.chan[2].tx};
    bool hist = false;
    double dmin = 0.0, inv = 0.0;
    if constexpr (HIST) hist = hist_begin(a.hist, lds, &dmin, &inv);
    unsigned int *mine = lds + (a.hist.copies > 1 ? (threadIdx.x >> 6) * a.hist.t : 0);
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
                if (a.in16) {
                    const float4 v = *reinterpret_cast<const float4 *>(a.src[c] + i);
                    s[c][0] = v.x, s[c][1] = v.y, s[c][2] = v.z, s[c][3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[c][k] = a.src[c][i + k];
                }
            }
        }
        if constexpr (HIST) {
            if (hist) {
#pragma unroll
                for (int k = 0; k < 4; ++k) hist_px(a.hist, mine, s[0][k], dmin, inv);
            }
        }
        uint32_t d[3] = {0u, 0u, 0u};  // byte j = 3 k + c: four to a dword
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= quantise(to_f32(s[c][k], tx[c])) << (8 * ((3 * k + c) & 3));
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 3 * i);
#pragma unroll
        for (int j = 0; j < 3; ++j) o[j] = d[j];
    }
    const int64_t loose = a.n - 4 * a.quads;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < loose; e += stride) {
        const int64_t i = e < a.head ? e : 4 * a.quads + e;
        const int64_t si = source_of<SAMPLED>(a, i);
        float p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = a.src[c][si];
        if constexpr (HIST) {
            if (hist) hist_px(a.hist, mine, p[0], dmin, inv);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) a.out[3 * i + c] = (uint8_t)quantise(to_f32(p[c], tx[c]));
    }
    if constexpr (HIST) {
        if (hist) hist_end(a.hist, lds);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct ViewWs {  // carved from AB_WS_VIEW
    unsigned int *src_bins;  // the 65 536 bins of the two-step route
    unsigned int *out_bins;  // up to 65 536 display bins on their way to a host output
    ViewChan *chan;          // the three channels' saved results
};

int carve(ab_ctx *ctx, ViewWs *w) {
    void *p = nullptr;
    const size_t bins = (size_t)kViewSrcBins * sizeof(unsigned int);
    AB_TRY(ab_workspace(ctx, AB_WS_VIEW, 2 * bins + 3 * sizeof(ViewChan), &p));
    w->src_bins = (unsigned int *)p;
    w->out_bins = (unsigned int *)((char *)p + bins);
    w->chan = (ViewChan *)((char *)p + 2 * bins);
    return AB_OK;
}

enum HistRoute { ROUTE_NONE = 0, ROUTE_LDS, ROUTE_FOLD, ROUTE_COPY };
struct HistPlan {
    HistRoute route = ROUTE_NONE;
    size_t target = 0, out_len = 0;
    int copies = 1, shift = 0;
    size_t lds_bytes = 0;
};

HistPlan plan_hist(size_t target) {
    HistPlan p;
    p.target = target;
    if (target == 0) return p;
    if (target >= (size_t)kViewSrcBins) {  // stats.rs:426-428: the 65 536 bins themselves
        p.route = ROUTE_COPY, p.out_len = kViewSrcBins;
        return p;
    }
    p.out_len = target;
    if ((target & (target - 1)) == 0 && target <= (size_t)kLdsMax) {
        p.route = ROUTE_LDS;
        p.copies = target <= (size_t)kPerWaveMax ? kWaves : 1;
        for (size_t t = target; t < (size_t)kViewSrcBins; t <<= 1) ++p.shift;
        p.lds_bytes = target * (size_t)p.copies * sizeof(unsigned int);
    } else {
        p.route = ROUTE_FOLD;
    }
    return p;
}

// clears what the pass adds into and points `h` at it; out_dev: the display bins on the device
int hist_prepare(ab_ctx *ctx, const HistPlan &p, const ViewWs &w, unsigned int *out_dev, HistArgs *h) {
    h->t = 0, h->copies = 1, h->shift = 0;
    if (p.route == ROUTE_LDS) {
        h->bins = out_dev, h->t = (int)p.target, h->copies = p.copies, h->shift = p.shift;
        AB_HIP(ctx, hipMemsetAsync(out_dev, 0, p.target * sizeof(unsigned int), ctx->stream));
    } else if (p.route == ROUTE_COPY) {
        h->bins = out_dev;
        AB_HIP(ctx, hipMemsetAsync(out_dev, 0, (size_t)kViewSrcBins * sizeof(unsigned int), ctx->stream));
    } else {
        h->bins = w.src_bins;
        AB_HIP(ctx, hipMemsetAsync(w.src_bins, 0, (size_t)kViewSrcBins * sizeof(unsigned int), ctx->stream));
    }
    return AB_OK;
}

int hist_finish(ab_ctx *ctx, const HistPlan &p, const ViewWs &w, unsigned int *out_dev) {
    if (p.route != ROUTE_FOLD) return AB_OK;
    hipLaunchKernelGGL(fold_kernel, dim3(ab_div_up((int64_t)p.target, kBlock)), dim3(kBlock), 0, ctx->stream, w.src_bins, (uint32_t)p.target, out_dev);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// one pass over a plane: the apply_stf bytes (tx_dev, out; both or neither) and / or the histogram (hist nullable)
int launch_mono(ab_ctx *ctx, const float *src, int64_t n, const StfTx *tx_dev, uint8_t *out, const HistArgs *hist, size_t lds_bytes) {
    MonoArgs a;
    a.src = src, a.n = n, a.tx_dev = tx_dev, a.out = out;
    a.head = head16(src, n);
    a.quads = (n - a.head) / 4;
    a.out4 = out && ((uintptr_t)(out + a.head) & 3u) == 0;
    if (hist) a.hist = *hist;
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, n - 4 * a.quads));
    if (out && hist) {
        hipLaunchKernelGGL((view_mono_kernel<true, true>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, a);
    } else if (out) {
        hipLaunchKernelGGL((view_mono_kernel<true, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else if (hist) {
        hipLaunchKernelGGL((view_mono_kernel<false, true>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

int launch_rgb(ab_ctx *ctx, RgbArgs a, bool sampled, const HistArgs *hist, size_t lds_bytes) {
    a.head = head_bytes(a.out, a.n);
    a.quads = (a.n - a.head) / 4;
    uintptr_t in_bits = 0;
    for (int c = 0; c < 3; ++c) in_bits |= (uintptr_t)(a.src[c] + a.head);
    a.in16 = !sampled && (in_bits & 15u) == 0;
    if (hist) a.hist = *hist;
    const int grid = ab_stream_grid(ctx, std::max<int64_t>(a.quads, a.n - 4 * a.quads));
    if (sampled) {
        hipLaunchKernelGGL((view_rgb_kernel<true, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else if (hist) {
        hipLaunchKernelGGL((view_rgb_kernel<false, true>), dim3(grid), dim3(kBlock), lds_bytes, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((view_rgb_kernel<false, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

const ab_auto_stf_config kStfDefault = {0.25, -2.8};  // AutoStfConfig::default() (types/image.rs:52-65)
constexpr size_t kHistBinsDisplay = 512;              // HISTOGRAM_BINS_DISPLAY (types/constants.rs)

}  // namespace

extern "C" {

int ab_downsample_histogram(const uint32_t *bins, size_t n_bins, size_t target_bins, uint32_t *out, size_t *out_len) try {
    if (!bins || !out || !out_len || n_bins == 0 || target_bins == 0) return AB_ERR_INVALID;
    if (target_bins >= n_bins) {  // stats.rs:426-428
        memcpy(out, bins, n_bins * sizeof(uint32_t));
        *out_len = n_bins;
        return AB_OK;
    }
    const double ratio = (double)n_bins / (double)target_bins;  // :431
    for (size_t i = 0; i < target_bins; ++i) {
        const size_t start = (size_t)((double)i * ratio);  // :434 (a finite value of at most n_bins: `as usize` is the truncation)
        const size_t end = std::min((size_t)((double)(i + 1) * ratio), n_bins);
        uint64_t sum = 0;  // saturating_add in sequence (:438) = the exact sum clamped, taken 2^16 bins at a time so that it cannot wrap
        for (size_t j = start; j < end && sum <= 0xffffffffull; j += 65536) {
            const size_t stop = std::min(end, j + 65536);
            for (size_t k = j; k < stop; ++k) sum += bins[k];
        }
        out[i] = (uint32_t)std::min<uint64_t>(sum, 0xffffffffull);
    }
    *out_len = target_bins;
    return AB_OK;
} AB_CATCH_NOCTX

int ab_histogram_bin_edges(double dmin, double dmax, size_t bins, double *edges) try {
    if (!edges || bins == 0) return AB_ERR_INVALID;
    const double range = dmax - dmin;
    if (range < 1e-10) {  // stats.rs:380-387
        for (size_t i = 0; i <= bins; ++i) edges[i] = dmin;
        return AB_OK;
    }
    const double step = range / (double)bins;  // :412-413
    for (size_t i = 0; i <= bins; ++i) edges[i] = dmin + (double)i * step;
    return AB_OK;
} AB_CATCH_NOCTX

int ab_display_histogram(ab_ctx *ctx, const ab_plane *img, double dmin, double dmax, size_t target_bins, uint32_t *out_bins, int32_t out_on_device,
                         size_t *out_len) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img, "image"));
    AB_CHECK(ctx, out_bins, "null output");
    AB_CHECK(ctx, target_bins >= 1, "target_bins must be >= 1");
    const HistPlan plan = plan_hist(target_bins);
    AB_TRY(overlap_check(ctx, {device_span(*img)}, {device_span(out_bins, plan.out_len * sizeof(uint32_t), out_on_device)}));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *src = nullptr;
    AB_TRY(sc.stage_in(img, &src));
    ViewWs w;
    AB_TRY(carve(ctx, &w));
    unsigned int *out_dev = out_on_device ? out_bins : w.out_bins;
    HistArgs h;
    h.dmin = dmin, h.dmax = dmax;
    AB_TRY(hist_prepare(ctx, plan, w, out_dev, &h));
    AB_TRY(launch_mono(ctx, src, img->rows * img->cols, nullptr, nullptr, &h, plan.lds_bytes));
    AB_TRY(hist_finish(ctx, plan, w, out_dev));
    if (!out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_bins, out_dev, plan.out_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (out_len) *out_len = plan.out_len;
    return AB_OK;
} AB_CATCH(ctx)

void ab_fits_view_config_default(ab_fits_view_config *cfg) {
    if (!cfg) return;
    cfg->stf = kStfDefault;
    cfg->hist_bins = kHistBinsDisplay;
}

int ab_process_fits_view(ab_ctx *ctx, const ab_plane *img, const ab_fits_view_config *cfg, uint8_t *out_u8, int32_t out_on_device, uint32_t *out_bins,
                         int32_t bins_on_device, ab_fits_view_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_TRY(plane_check(ctx, img, "image"));
    AB_CHECK(ctx, cfg && out_u8, "null configuration or byte output");
    AB_CHECK(ctx, cfg->hist_bins == 0 || out_bins, "hist_bins is %zu and out_bins is null", cfg->hist_bins);
    const int64_t n = img->rows * img->cols;
    const HistPlan plan = plan_hist(cfg->hist_bins);
    AB_TRY(overlap_check(ctx, {device_span(*img)}, {device_span(out_u8, (size_t)n, out_on_device)}));
    AB_TRY(overlap_check(ctx, {device_span(*img)}, {device_span(out_bins, plan.out_len * sizeof(uint32_t), bins_on_device)}));  // (no bins: no bytes)
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    const float *src = nullptr;
    AB_TRY(sc.stage_in(img, &src));
    ViewWs w;
    AB_TRY(carve(ctx, &w));
    uint8_t *bytes_dev = out_u8;  // the caller's buffer, or the scratch arena for a host output (the statistics chain asks for none)
    if (!out_on_device) AB_TRY(ab_scratch(ctx, (size_t)n, (void **)&bytes_dev));
    const ab_image_stats *res = nullptr;
    const void *tx = nullptr;
    const ab_stf_params *stf = nullptr;
    AB_TRY(ab_stats_enqueue(ctx, nullptr, src, n, n, 0, 0.0, 0.0, &cfg->stf, &res, &tx, &stf));
    unsigned int *bins_dev = bins_on_device ? out_bins : w.out_bins;
    HistArgs h;
    h.st_dev = res;
    if (plan.route != ROUTE_NONE) AB_TRY(hist_prepare(ctx, plan, w, bins_dev, &h));
    AB_TRY(launch_mono(ctx, src, n, (const StfTx *)tx, bytes_dev, plan.route != ROUTE_NONE ? &h : nullptr, plan.lds_bytes));
    AB_TRY(hist_finish(ctx, plan, w, bins_dev));
    char *pin = nullptr;
    bool wait = false;
    if (info) {
        AB_TRY(ab_pinned(ctx, sizeof(ab_image_stats) + sizeof(ab_stf_params), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, res, sizeof(ab_image_stats), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipMemcpyAsync(pin + sizeof(ab_image_stats), stf, sizeof(ab_stf_params), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (!out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_u8, bytes_dev, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (plan.route != ROUTE_NONE && !bins_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_bins, bins_dev, plan.out_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        memset(info, 0, sizeof *info);
        info->rows = (uint64_t)img->rows, info->cols = (uint64_t)img->cols;
        memcpy(&info->stats, pin, sizeof info->stats);
        memcpy(&info->stf, pin + sizeof(ab_image_stats), sizeof info->stf);
        info->hist_len = (uint64_t)plan.out_len;
    }
    return AB_OK;
} AB_CATCH(ctx)

int ab_process_rgb_fits_view(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_fits_view_config *cfg, int64_t max_dim,
                             uint8_t *out_rgb8, int32_t out_on_device, uint32_t *out_bins, int32_t bins_on_device, ab_rgb_fits_view_info *info) try {
    if (!ctx) return AB_ERR_INVALID;
    const ab_plane *ch[3] = {r, g, b};
    AB_TRY(same_dims_check(ctx, ch));  // (the command takes its dims from R, cmd/io/mod.rs:56)
    AB_CHECK(ctx, cfg, "null configuration");
    AB_CHECK(ctx, max_dim >= 1, "max_dim must be >= 1 (got %lld)", (long long)max_dim);
    AB_CHECK(ctx, out_rgb8 || cfg->hist_bins > 0, "nothing to do: out_rgb8 is null and hist_bins is 0");
    AB_CHECK(ctx, cfg->hist_bins == 0 || out_bins, "hist_bins is %zu and out_bins is null", cfg->hist_bins);
    const int64_t rows = r->rows, cols = r->cols, n = rows * cols;
    Preview pv;
    AB_TRY(preview_of(ctx, rows, cols, max_dim, &pv));
    const int64_t ph = pv.ph, pw = pv.pw;
    const bool above = pv.sampled;
    const size_t nbytes = (size_t)(ph * pw) * 3;
    const HistPlan plan = plan_hist(cfg->hist_bins);
    const std::vector<Span> ins{device_span(*r), device_span(*g), device_span(*b)};
    AB_TRY(overlap_check(ctx, ins, {device_span(out_rgb8, nbytes, out_on_device)}));
    AB_TRY(overlap_check(ctx, ins, {device_span(out_bins, plan.out_len * sizeof(uint32_t), bins_on_device)}));  // (no bins: no bytes)
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    ViewWs w;
    AB_TRY(carve(ctx, &w));
    uint8_t *bytes_dev = out_rgb8;
    if (out_rgb8 && !out_on_device) AB_TRY(ab_scratch(ctx, nbytes, (void **)&bytes_dev));
    RgbArgs a;
    a.rows = rows, a.cols = cols, a.n = n, a.chan = w.chan, a.out = bytes_dev;
    for (int c = 0; c < 3; ++c) {  // cmd/io/mod.rs:44-50, one chain per channel; its result leaves the state block before the next
        AB_TRY(sc.stage_in(ch[c], &a.src[c]));
        const ab_image_stats *res = nullptr;
        const void *tx = nullptr;
        const ab_stf_params *stf = nullptr;
        AB_TRY(ab_stats_enqueue(ctx, nullptr, a.src[c], n, n, 0, 0.0, 0.0, &cfg->stf, &res, &tx, &stf));
        hipLaunchKernelGGL(save_chan_kernel, dim3(1), dim3(64), 0, ctx->stream, res, stf, (const StfTx *)tx, w.chan + c);
        AB_HIP(ctx, hipGetLastError());
    }
    unsigned int *bins_dev = bins_on_device ? out_bins : w.out_bins;
    HistArgs h;
    h.st_dev = &w.chan[0].stats;  // compute_histogram_with_stats(&rgb.r, &stats_r), :61
    const bool want_hist = plan.route != ROUTE_NONE;
    if (want_hist) AB_TRY(hist_prepare(ctx, plan, w, bins_dev, &h));
    const bool ride = want_hist && bytes_dev && !above;  // every pixel of R is visited by the packer
    if (bytes_dev) {
        if (above) {
            a.n = ph * pw, a.pw = pw;
            a.y_ratio = (double)rows / (double)ph, a.x_ratio = (double)cols / (double)pw;
        }
        AB_TRY(launch_rgb(ctx, a, above, ride ? &h : nullptr, plan.lds_bytes));
    }
    if (want_hist && !ride) AB_TRY(launch_mono(ctx, a.src[0], n, nullptr, nullptr, &h, plan.lds_bytes));
    AB_TRY(hist_finish(ctx, plan, w, bins_dev));
    char *pin = nullptr;
    bool wait = false;
    if (info) {
        AB_TRY(ab_pinned(ctx, 3 * sizeof(ViewChan), (void **)&pin));
        AB_HIP(ctx, hipMemcpyAsync(pin, w.chan, 3 * sizeof(ViewChan), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (out_rgb8 && !out_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_rgb8, bytes_dev, nbytes, hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (want_hist && !bins_on_device) {
        AB_HIP(ctx, hipMemcpyAsync(out_bins, bins_dev, plan.out_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        wait = true;
    }
    if (wait) AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) {
        memset(info, 0, sizeof *info);
        info->rows = (uint64_t)rows, info->cols = (uint64_t)cols;
        info->preview_rows = (uint64_t)ph, info->preview_cols = (uint64_t)pw;
        for (int c = 0; c < 3; ++c) {
            ViewChan vc;
            memcpy(&vc, pin + c * sizeof(ViewChan), sizeof vc);
            info->stats[c] = vc.stats, info->stf[c] = vc.stf;
        }
        info->hist_len = (uint64_t)plan.out_len;
    }
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
