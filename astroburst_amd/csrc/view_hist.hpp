// The display histogram's bin arithmetic and its LDS accumulation (view.hip; tools/view_hist_bench.hip measures the choices).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kViewSrcBins = 65536;  // HISTOGRAM_BINS (stats.rs:8): what compute_histogram_with_stats builds before the fold

// build_histogram's index (stats.rs:398-399) at 65 536 bins: ((v as f64 - dmin) * inv) as usize, then .min(65535).  Rust's cast
// saturates and sends NaN to 0; the same three IEEE operations as stats.hip's bin_index, so every pixel lands where
// ab_build_histogram(65536) puts it.
__device__ __forceinline__ uint32_t view_bin(float v, double dmin, double inv) {
    const double t = ((double)v - dmin) * inv;
    if (!(t > 0.0)) return 0;
    if (t >= (double)(kViewSrcBins - 1)) return kViewSrcBins - 1;
    return (uint32_t)t;
}

// One more pixel in `bins[bin]` for every lane with `valid`.  A sky frame sends most of a wave's lanes to the same one or two display
// bins.  MODE 0: one add per lane.  MODE 1: the lanes that share the first valid lane's bin are counted with one ballot and that lane
// adds the count, in the same instruction in which every other valid lane adds its 1.  MODE 2: the same with two instructions (the
// leader's add, then the others').  Every lane of the wave that is still in the loop calls this together (a ballot sees the active
// lanes only).  tools/view_hist_bench.hip measures the three.
template <int MODE>
__device__ __forceinline__ void view_hist_add(unsigned int *bins, bool valid, uint32_t bin) {
    if constexpr (MODE == 0) {
        if (valid) atomicAdd(&bins[bin], 1u);
    } else {
        const unsigned long long m = __ballot(valid);
        if (m == 0) return;  // (uniform)
        const int first = __ffsll(m) - 1;
        const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
        const bool mine = valid && bin == lead;
        const unsigned int same = (unsigned int)__popcll(__ballot(mine));
        const bool leader = (int)__lane_id() == first;
        if constexpr (MODE == 1) {
            if (leader || (valid && !mine)) atomicAdd(&bins[bin], leader ? same : 1u);
        } else {
            if (leader) atomicAdd(&bins[lead], same);
            if (valid && !mine) atomicAdd(&bins[bin], 1u);
        }
    }
}

}  // namespace
