// The weighted, normalised sigma-clip stack (ab_stack_weighted) and the parameters it takes from the subframe scores
// (ab_stack_params_from_metrics).  The reference has no weighted stack (core/stacking/combine.rs:14-92 ends in an unweighted mean of
// the survivors); the definition is this library's own, in include/astroburst_hip.h: every frame is brought to a common level first
// (s = p * scale + offset in f32), the REJECTION is sigma_clip_combine's on those samples, and only the final mean changes -- the
// survivors are weighted per frame.
//
// Mapping: stack_sigma_clip.hip's.  One lane per output pixel, a wave reads 64 consecutive pixels of every frame (one 256-byte segment
// per frame, every load issued before the first is consumed), up to 64 frames per lane.  What is new is that the lane keeps TWO
// copies of its samples in registers:
//   s[NP]   the normalised samples in FRAME order (non-finite ones replaced by +inf),
//   v[NP]   the same values sorted (the network of sortnet_gen.hpp), which median / MAD and the exact clipping engine work on
//           (stack_clip.hpp: clip_exact, the arithmetic of ab_stack_sigma_clip under AB_STACK_EXACT=1).
// The survivors are an interval [a, b] of the sorted order and equal values share their fate, so frame f survives exactly when
// v[a] <= s[f] <= v[b]: the two bounds are fetched with an unrolled select chain (a run-time index would send the array to scratch
// memory) and ONE sweep over s[] in frame order accumulates sum(w s) and sum(w) in f64 -- a multiply and an add per frame, rounded
// separately (-ffp-contract=off).  The weights, scales and offsets are wave-uniform kernel arguments next to the plane pointers, read
// through the scalar cache (at NP = 32 / 64 the compiler parks part of the table in VGPR lanes).  Frames of weight 0 never reach the
// kernel (the host drops them from the table), and the slots between the active frames and NP read the context's +inf plane
// (ab_stack_inf_plane) with weight 0, so every load is unconditional.
//
// HBM traffic: 4 N P bytes read once, 4 P (image) or 8 P (image + weight plane) written.  128 registers of samples at NP = 64: one
// wave per SIMD, as the exact engine of stack_sigma_clip.hip.
#include "entry_host.hpp"
#include "stack_clip.hpp"

#include <cmath>

namespace {

constexpr int kMaxActive = AB_STACK_MAX_ACTIVE;  // 64: a pixel's samples live in one lane's registers, twice

struct WeightedArgs {
    const float *p[kMaxActive];
    int64_t ld[kMaxActive];  // row stride (= cols of that plane): the top-left crop
    double w[kMaxActive];    // > 0 for the active frames, 0 for the pads
    float scale[kMaxActive], offset[kMaxActive];
    int contiguous;          // all ld == cols: the linear pixel index is the element offset
    int64_t rows, cols;      // output dims
    float sigma_low, sigma_high;
    uint32_t max_iter;
    float *out;
    float *out_w;                  // nullable
    unsigned long long *rejected;  // AB_REJ_SLOTS device counters
};

template <int NP>
__global__ __launch_bounds__(256, 1) void stack_weighted_kernel(const WeightedArgs args) {
    const int64_t total = args.rows * args.cols;
    int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = g < total;
    if (!valid) g = total - 1;  // no lane reads out of range; it writes and counts nothing
    int64_t y = 0, x = g;
    if (!args.contiguous) {
        y = g / args.cols;
        x = g - y * args.cols;
    }

    // ---- load (all NP loads in flight), then normalise: s = p * scale + offset, an f32 multiply and an f32 add ----
    float s[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) s[f] = args.p[f][args.contiguous ? g : (y * args.ld[f] + x)];
    int n = 0;  // finite samples of this pixel
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        // (a frame of scale 1 and offset 0 is read as it is: -0.0 * 1 + 0 would be +0.0)
        const bool as_is = args.scale[f] == 1.0f && args.offset[f] == 0.0f;
        const float t = as_is ? s[f] : s[f] * args.scale[f] + args.offset[f];
        // finiteness is judged on the normalised sample; what is not finite becomes a +inf pad that sorts to the top (combine.rs:170-175)
        const bool fin = __builtin_isfinite(t);
        s[f] = fin ? t : __builtin_inff();
        n += fin ? 1 : 0;
    }

    float v[NP];
#pragma unroll
    for (int f = 0; f < NP; ++f) v[f] = s[f];
    if constexpr (NP >= 8)
        SortNet<NP>::sort_fused(v);
    else
        SortNet<NP>::sort(v);

    // ---- iteration 0's median / MAD (combine.rs:37-48), as stack_sigma_clip.hip's stack_pixel takes them ----
    const int m = n >> 1;
    float med = 0.0f, mad = 0.0f;
    if (__all(m == NP / 2)) {
        med_mad_at<NP, NP / 2>(v, med, mad);  // every lane has all NP samples
    } else if (__all(m == __builtin_amdgcn_readfirstlane(m))) {
        med_mad_dispatch<NP, 0, NP / 2>(v, m, __builtin_amdgcn_readfirstlane(m), med, mad);  // one position for the whole wave (a padded stack)
    } else {
        float w[NP];  // (a copy: launder() makes the vector look rewritten)
#pragma unroll
        for (int f = 0; f < NP; ++f) w[f] = v[f];
        unsigned long long todo = __ballot(1);
        while (todo) {
            launder<NP>(w);  // or LICM evaluates all NP/2+1 candidate positions up front and spills
            const int cur = __builtin_amdgcn_readlane(m, (int)__builtin_ctzll(todo));
            med_mad_dispatch<NP, 0, NP / 2>(w, m, cur, med, mad);
            todo &= ~__ballot(m == cur);
        }
    }

    // ---- the reference's rejection, down to the surviving interval ----
    const ClipResult r = clip_exact<NP>(v, n, med, mad, args.sigma_low, args.sigma_high, args.max_iter);

    // the bounds of the interval (nothing survived, or no sample at all: the sweep's sums are not used)
    float va = 0.0f, vb = 0.0f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        va = (i == r.a) ? v[i] : va;
        vb = (i == r.b) ? v[i] : vb;
    }
    // ---- one sweep in frame order: sum(w s) and sum(w) over the surviving frames (a pad is +inf, above every finite bound) ----
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int f = 0; f < NP; ++f) {
        const bool keep = s[f] >= va && s[f] <= vb;
        const double ws = args.w[f] * (double)s[f];
        num += keep ? ws : 0.0;  // (x + 0.0 == x: a frame that does not survive adds nothing)
        den += keep ? args.w[f] : 0.0;
    }

    float value, wsum;
    if (n == 0) {
        value = 0.0f;
        wsum = 0.0f;
    } else if (n == 1) {
        value = med;  // the single finite sample, bit for bit (v[0] = v[n / 2])
        wsum = (float)den;
    } else if (r.len == 0) {
        value = __builtin_isfinite(r.last_center) ? r.last_center : 0.0f;  // combine.rs:85-88
        wsum = 0.0f;
    } else {
        value = (float)(num / den);
        wsum = (float)den;
    }
    uint32_t rej = r.rej;
    if (valid) {
        args.out[g] = value;
        if (args.out_w) args.out_w[g] = wsum;
    } else {
        rej = 0;
    }
    // rejection count: wave reduction, then one atomic per wave spread over AB_REJ_SLOTS counters (stack_sigma_clip.hip's epilogue)
    rej = (uint32_t)wave_reduce_i32<0>((int)rej);
    if ((threadIdx.x & 63) == 0 && rej != 0)
        atomicAdd(&args.rejected[(blockIdx.x * 4u + (threadIdx.x >> 6)) & (AB_REJ_SLOTS - 1)], (unsigned long long)rej);
}

template <int NP>
void launch_weighted(ab_ctx *ctx, const WeightedArgs &args, int64_t total) {
    hipLaunchKernelGGL(stack_weighted_kernel<NP>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, args);
}

}  // namespace

extern "C" {

int ab_stack_weighted(ab_ctx *ctx, const ab_plane *planes, const ab_stack_frame_param *params, size_t n, const ab_stack_config *cfg, ab_plane_mut *out,
                      ab_plane_mut *out_weight, uint64_t *out_rejected) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, planes && params && n >= 1, "No images to stack");
    AB_CHECK(ctx, cfg && out && out->data, "null config or output");
    AB_CHECK(ctx, out->rows > 0 && out->cols > 0, "stack output has a zero dimension");
    AB_CHECK(ctx, fits31(out->rows, out->cols), "the stack output holds 2^31 pixels or more");  // (pixel counts, byte spans and the grid stay in range)
    AB_CHECK(ctx, !out_weight || (out_weight->data && out_weight->rows == out->rows && out_weight->cols == out->cols),
             "the weight plane is null or not %lld x %lld", (long long)out->rows, (long long)out->cols);
    std::vector<size_t> active;
    for (size_t i = 0; i < n; ++i) {
        AB_CHECK(ctx, std::isfinite(params[i].weight) && params[i].weight >= 0.0, "frame %zu has a negative or non-finite weight", i);
        AB_CHECK(ctx, std::isfinite(params[i].scale) && std::isfinite(params[i].offset), "frame %zu has a non-finite scale or offset", i);
        AB_CHECK(ctx, planes[i].rows >= out->rows && planes[i].cols >= out->cols, "frame %zu (%lldx%lld) is smaller than the output (%lldx%lld)", i,
                 (long long)planes[i].rows, (long long)planes[i].cols, (long long)out->rows, (long long)out->cols);
        if (params[i].weight > 0.0) active.push_back(i);
    }
    AB_CHECK(ctx, !active.empty(), "No images to stack");
    if (active.size() > (size_t)kMaxActive)
        return ab_set_error(ctx, AB_ERR_UNSUPPORTED, "weighted stack of %zu active frames (at most %d frames of weight > 0 per call)", active.size(),
                            kMaxActive);
    std::vector<Span> ins, outs{device_span(out->data, (size_t)out->rows * (size_t)out->cols * sizeof(float), out->on_device)};
    if (out_weight) outs.push_back(device_span(out_weight->data, (size_t)out->rows * (size_t)out->cols * sizeof(float), out_weight->on_device));
    for (size_t i : active) {
        AB_CHECK(ctx, planes[i].data, "frame %zu is null", i);
        AB_CHECK(ctx, fits31(planes[i].rows, planes[i].cols), "frame %zu holds 2^31 pixels or more", i);
        ins.push_back(device_span(planes[i]));
    }
    AB_TRY(overlap_check(ctx, ins, outs));
    AB_HIP(ctx, hipSetDevice(ctx->device));

    const int64_t total = out->rows * out->cols;
    int np = 2;
    while (np < (int)active.size()) np *= 2;
    Scope sc(ctx);
    WeightedArgs args;
    memset(&args, 0, sizeof args);
    args.contiguous = 1;
    for (size_t k = 0; k < active.size(); ++k) {
        const size_t i = active[k];
        AB_TRY(sc.stage_in(&planes[i], &args.p[k]));
        args.ld[k] = planes[i].cols;
        if (planes[i].cols != out->cols) args.contiguous = 0;
        args.w[k] = params[i].weight;
        args.scale[k] = params[i].scale;
        args.offset[k] = params[i].offset;
    }
    if ((int)active.size() < np) {  // the pads: a plane of +inf, read as it is, weight 0
        const float *inf_plane = nullptr;
        AB_TRY(ab_stack_inf_plane(ctx, total, &inf_plane));
        for (int k = (int)active.size(); k < np; ++k) {
            args.p[k] = inf_plane;
            args.ld[k] = out->cols;
            args.scale[k] = 1.0f;
        }
    }
    args.rows = out->rows;
    args.cols = out->cols;
    args.sigma_low = cfg->sigma_low;
    args.sigma_high = cfg->sigma_high;
    args.max_iter = cfg->max_iterations;
    AB_TRY(sc.stage_out(out, &args.out));
    if (out_weight) AB_TRY(sc.stage_out(out_weight, &args.out_w));
    args.rejected = ctx->counters;

    AB_HIP(ctx, hipMemsetAsync(ctx->counters, 0, AB_REJ_SLOTS * sizeof(unsigned long long), ctx->stream));
    for (hipEvent_t &e : ctx->stack_ev)
        if (!e) AB_HIP(ctx, hipEventCreate(&e));
    ctx->stack_ev_valid = false;
    AB_HIP(ctx, hipEventRecord(ctx->stack_ev[0], ctx->stream));
    switch (np) {
        case 2: launch_weighted<2>(ctx, args, total); break;
        case 4: launch_weighted<4>(ctx, args, total); break;
        case 8: launch_weighted<8>(ctx, args, total); break;
        case 16: launch_weighted<16>(ctx, args, total); break;
        case 32: launch_weighted<32>(ctx, args, total); break;
        default: launch_weighted<64>(ctx, args, total); break;
    }
    AB_HIP(ctx, hipGetLastError());
    AB_HIP(ctx, hipEventRecord(ctx->stack_ev[1], ctx->stream));
    ctx->stack_ev_valid = true;
    AB_TRY(sc.finish_outs());
    if (out_rejected) AB_TRY(ab_stack_last_rejected(ctx, out_rejected));
    return AB_OK;
} AB_CATCH(ctx)

int ab_stack_params_from_metrics(const ab_subframe_metrics *metrics, size_t n, int32_t normalize, ab_stack_frame_param *out, size_t *out_reference) try {
    if (!metrics || !out) return AB_ERR_INVALID;
    if (normalize != AB_STACK_NORM_NONE && normalize != AB_STACK_NORM_ADDITIVE && normalize != AB_STACK_NORM_MULTIPLICATIVE) return AB_ERR_INVALID;
    // a background a frame can be normalised with (AB_STACK_NORM_NONE does not look at it)
    const auto usable = [normalize](double bg) {
        if (normalize == AB_STACK_NORM_NONE) return true;
        return std::isfinite(bg) && (normalize != AB_STACK_NORM_MULTIPLICATIVE || bg > 0.0);
    };
    size_t ref = n;
    for (size_t i = 0; i < n; ++i) {
        const double w = metrics[i].weight;
        out[i] = ab_stack_frame_param{metrics[i].accepted && std::isfinite(w) && w > 0.0 ? w : 0.0, 1.0f, 0.0f};
        if (out[i].weight > 0.0 && (ref == n || out[i].weight > out[ref].weight)) ref = i;  // the largest weight, the lowest index on a tie
    }
    if (ref == n || !usable(metrics[ref].background_median)) return AB_ERR_INVALID;
    const double bg_ref = metrics[ref].background_median;
    for (size_t i = 0; i < n; ++i) {
        if (out[i].weight == 0.0) continue;
        const double bg = metrics[i].background_median;
        if (!usable(bg)) {
            out[i].weight = 0.0;
        } else if (normalize == AB_STACK_NORM_ADDITIVE) {
            out[i].offset = (float)(bg_ref - bg);
        } else if (normalize == AB_STACK_NORM_MULTIPLICATIVE) {
            out[i].scale = (float)(bg_ref / bg);
        }
    }
    if (out_reference) *out_reference = ref;
    return AB_OK;
} AB_CATCH_NOCTX

}  // extern "C"
