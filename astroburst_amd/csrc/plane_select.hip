// Exact order statistics over a whole plane (gfx950): 11/11/10-bit radix select on f32 bit patterns.
//
// Serves every place the reference collects the valid pixels of a full image into a Vec and calls
// select_nth_unstable on it: background.rs:135-146 (global median / MAD), :350-361 (model median),
// tiles.rs:149-178 (percentile bounds), wavelet.rs:203-216 (the median of the finite |d_0|).  (The masked
// stretch has its own device-resident chain of the same 11/11/10 select: masked_stretch.hip.)  The keys
// are non-negative -- candidates are > min_valid >= 0, or the keys are absolute deviations -- so their
// bit patterns order like the values.  Pass 0 histograms the top 11 bits and yields the candidate count;
// each requested rank then costs two more streaming passes.  All passes are HBM-bound reads of the plane.
//
// The spectral cube's global statistics (cube.hip; eager.rs:168-208, lazy.rs:331-370) take the same select over SIGNED values:
// ab_plane_sel::cube_rule >= 0 instantiates the histogram kernel a second time, with the cube's two validity rules, the
// order-preserving key bits ^ (sign ? 0xFFFFFFFF : 0x80000000), and the candidates laid out as every frame_step-th frame of
// frame_len values.  The host descent is shared; the callers above keep the first instantiation, their arguments and results.
// The PSF estimation's image median (psf.hip) is the signed form over one frame with AB_SEL_VALID_FINITE: every finite pixel counts.
#include "ab_common.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = 256;

struct SelArgs {
    const float *data;
    int64_t n;
    float min_valid;
    int use_dev;
    float center;
    uint32_t prefix_mask, prefix_val;
    int shift, nbits;
    unsigned int *hist;
    // the cube's form only (kCube): validity rule, frame geometry -- frame k of `frames` starts at data + k * frame_step * frame_len
    int cube_rule;
    int64_t frame_len, frame_step, frames;
};

// kCube = false: the planes' form, exactly as every caller before the cube had it.  kCube = true: blockIdx.y strides the frames.
template <bool kCube>
__global__ __launch_bounds__(kBlock) void plane_select_hist_kernel(const SelArgs a) {
    __shared__ unsigned int lds[2048];
    const uint32_t nb = 1u << a.nbits;
    for (uint32_t i = threadIdx.x; i < nb; i += kBlock) lds[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    if constexpr (!kCube) {
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
            const float v = a.data[i];
            if (__builtin_isfinite(v) && v > a.min_valid) {
                const float k = a.use_dev ? fabsf(v - a.center) : v;
                const uint32_t key = __float_as_uint(k);
                if ((key & a.prefix_mask) == a.prefix_val) atomicAdd(&lds[(key >> a.shift) & (nb - 1)], 1u);
            }
        }
    } else {
        for (int64_t f = blockIdx.y; f < a.frames; f += gridDim.y) {
            const float *frame = a.data + f * a.frame_step * a.frame_len;
            for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.frame_len; i += stride) {
                const float v = frame[i];
                if (__builtin_isfinite(v) && (a.cube_rule == AB_SEL_VALID_FINITE || (a.cube_rule == AB_CUBE_VALID_NONZERO ? v != 0.0f : v > 1e-7f))) {
                    uint32_t key;
                    if (a.use_dev) {
                        key = __float_as_uint(fabsf(v - a.center));
                    } else {
                        const uint32_t b = __float_as_uint(v);
                        key = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
                    }
                    if ((key & a.prefix_mask) == a.prefix_val) atomicAdd(&lds[(key >> a.shift) & (nb - 1)], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += kBlock)
        if (lds[i]) atomicAdd(&a.hist[i], lds[i]);
}

int run_pass(ab_ctx *ctx, const ab_plane_sel &s, uint32_t mask, uint32_t val, int shift, int nbits, unsigned int *host) {
    const uint32_t nb = 1u << nbits;
    AB_HIP(ctx, hipMemsetAsync(ctx->sel_hist, 0, nb * sizeof(unsigned int), ctx->stream));
    const int64_t target = (int64_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 8;
    if (s.cube_rule < 0) {
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((s.n + kBlock - 1) / kBlock, target));
        SelArgs a{s.data, s.n, s.min_valid, s.use_dev, s.center, mask, val, shift, nbits, ctx->sel_hist, -1, 0, 1, 0};
        hipLaunchKernelGGL(plane_select_hist_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, a);
    } else {
        AB_TRY(ab_cancel_point(ctx));  // the cube's contract: the cancel flag is looked at before every pass over the cube
        // frames along y (at most `target` rows of blocks: the kernel strides the rest), enough blocks along x to fill the chip
        const int64_t frames = (s.n + s.frame_len - 1) / s.frame_len;
        const int gy = (int)std::min<int64_t>(frames, target);
        const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((s.frame_len + kBlock - 1) / kBlock, (target + gy - 1) / gy));
        SelArgs a{s.data, s.n, s.min_valid, s.use_dev, s.center, mask, val, shift, nbits, ctx->sel_hist, s.cube_rule, s.frame_len, s.frame_step, frames};
        hipLaunchKernelGGL(plane_select_hist_kernel<true>, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    AB_HIP(ctx, hipMemcpyAsync(host, ctx->sel_hist, nb * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AB_OK;
}

// bin containing 0-based rank; rank becomes the rank within the bin
uint32_t locate(const unsigned int *h, uint32_t nb, uint64_t *rank) {
    uint64_t cum = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        if (cum + h[i] > *rank) {
            *rank -= cum;
            return i;
        }
        cum += h[i];
    }
    *rank = 0;
    return nb - 1;
}

}  // namespace

int ab_plane_select_ranks(ab_ctx *ctx, const ab_plane_sel &s, int max_ranks, const std::function<int(uint64_t, uint64_t *)> &ranks_of,
                          uint64_t *count_out, float *vals) {
    *count_out = 0;
    AB_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->sel_hist) AB_HIP(ctx, hipMalloc((void **)&ctx->sel_hist, 2048 * sizeof(unsigned int)));
    void *pin = nullptr;
    AB_TRY(ab_pinned(ctx, 3 * 2048 * sizeof(unsigned int), &pin));
    unsigned int *h0 = (unsigned int *)pin, *h1 = h0 + 2048, *h2 = h1 + 2048;
    if (s.n <= 0) return AB_OK;
    AB_TRY(run_pass(ctx, s, 0, 0, 21, 11, h0));
    uint64_t count = 0;
    for (int i = 0; i < 2048; ++i) count += h0[i];
    *count_out = count;
    if (count == 0) return AB_OK;
    std::vector<uint64_t> ranks((size_t)max_ranks);
    const int n_ranks = std::min(max_ranks, ranks_of(count, ranks.data()));
    // The ranks descend TOGETHER: a level is histogrammed once per distinct prefix, and the two middle ranks of an even count (the
    // usual request) share their prefix all the way down except when they straddle a bin edge -- 3 passes instead of 5.
    struct Item {
        int r;
        uint64_t rank;  // within the current prefix
    };
    const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    std::function<int(int, uint32_t, uint32_t, const unsigned int *, std::vector<Item>)> descend =
        [&](int level, uint32_t mask, uint32_t val, const unsigned int *h, std::vector<Item> items) -> int {
        // h = the histogram of `level` under (mask, val); split the items by the bin their rank falls into
        const uint32_t nb = 1u << bits[level];
        std::vector<std::pair<uint32_t, std::vector<Item>>> groups;
        for (Item it : items) {
            const uint32_t b = locate(h, nb, &it.rank);
            if (groups.empty() || groups.back().first != b) groups.push_back({b, {}});
            groups.back().second.push_back(it);
        }
        for (auto &g : groups) {
            const uint32_t v = val | (g.first << shifts[level]);
            if (level == 2) {
                // (the cube's signed keys go back through their own inverse; its deviation keys are plain bit patterns like the planes')
                const uint32_t bits_out = (s.cube_rule >= 0 && !s.use_dev) ? ((v & 0x80000000u) ? (v ^ 0x80000000u) : ~v) : v;
                for (const Item &it : g.second) memcpy(&vals[it.r], &bits_out, sizeof(float));
                continue;
            }
            const uint32_t m = mask | (((1u << bits[level]) - 1u) << shifts[level]);
            // Every item of this level has been located in `h` above, before the first child pass: a level's histogram is never read
            // again once its groups exist.  So no histogram can be overwritten while it is still needed, whichever buffer a child
            // pass fills -- level 2 could reuse h1; h2 only keeps the two levels' counts apart.
            unsigned int *hn = level == 0 ? h1 : h2;
            AB_TRY(run_pass(ctx, s, m, v, shifts[level + 1], bits[level + 1], hn));
            AB_TRY(descend(level + 1, m, v, hn, g.second));
        }
        return AB_OK;
    };
    std::vector<Item> items;
    for (int r = 0; r < n_ranks; ++r) items.push_back({r, std::min(ranks[r], count - 1)});
    std::stable_sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.rank < b.rank; });  // equal bins become neighbours
    return descend(0, 0u, 0u, h0, items);
}

int ab_plane_order_stats(ab_ctx *ctx, const ab_plane_sel &s, int want_lower, uint64_t *count_out, float *mid_out, float *lower_out) {
    *mid_out = 0.0f;
    if (lower_out) *lower_out = 0.0f;
    float v[2] = {0.0f, 0.0f};
    int got = 0;
    AB_TRY(ab_plane_select_ranks(
        ctx, s, 2,
        [&](uint64_t count, uint64_t *ranks) {
            ranks[0] = count / 2;
            ranks[1] = count / 2 - (count > 1 ? 1 : 0);
            return got = (want_lower && count % 2 == 0) ? 2 : 1;
        },
        count_out, v));
    if (*count_out == 0) return AB_OK;
    *mid_out = v[0];
    if (lower_out) *lower_out = got == 2 ? v[1] : v[0];
    return AB_OK;
}

int ab_plane_median_f32(ab_ctx *ctx, const ab_plane_sel &s, float *out, uint64_t *count_out) {
    uint64_t cnt;
    float mid, lower;
    AB_TRY(ab_plane_order_stats(ctx, s, 1, &cnt, &mid, &lower));
    if (count_out) *count_out = cnt;
    *out = cnt == 0 ? 0.0f : (cnt % 2 == 0 ? (lower + mid) / 2.0f : mid);
    return AB_OK;
}
