// Device helpers the stacking engines share (stack_sigma_clip.hip and, through stack_pair.hpp, stack_pair.hip and
// stack_lanes.hip): one copy each, all of them inlined into the kernels that use them.
#pragma once
#include "ab_common.hpp"

namespace abstack {

// Compiler fences (no instructions).  launder() makes the sample vector look rewritten so LLVM
// does not hoist 64 f32->f64 conversions (128 VGPRs) out of the clipping loop; opaque() stops it
// from keeping 64 interval masks alive in SGPRs across the passes of one iteration.
template <int NP>
__device__ __forceinline__ void launder(float (&v)[NP]) {
    if constexpr (NP >= 8) {
#pragma unroll
        for (int i = 0; i < NP; i += 8)
            asm volatile("" : "+v"(v[i]), "+v"(v[i + 1]), "+v"(v[i + 2]), "+v"(v[i + 3]), "+v"(v[i + 4]),
                         "+v"(v[i + 5]), "+v"(v[i + 6]), "+v"(v[i + 7]));
    } else {
#pragma unroll
        for (int i = 0; i < NP; ++i) asm volatile("" : "+v"(v[i]));
    }
}
__device__ __forceinline__ void opaque(int &a, int &b) { asm volatile("" : "+v"(a), "+v"(b)); }

// between a value written inside an asm statement and the DPP instruction that reads it: the wait states the compiler cannot see (dpp_fence)
__device__ __forceinline__ void nop_fence(float &x) { asm volatile("s_nop 1" : "+v"(x)); }

// wave reductions on DPP moves (row_shr 1/2/4/8, row_bcast 15 / 31; lanes without a source take the identity) and one v_readlane:
// VALU only, where the __shfl_xor butterfly is six dependent ds_bpermute round trips
template <int OP>  // 0 sum, 1 min, 2 max (signed)
__device__ __forceinline__ int wave_reduce_i32(int x) {
    constexpr int id = OP == 1 ? 0x7fffffff : (OP == 2 ? (int)0x80000000 : 0);
    auto op = [](int a, int b) { return OP == 0 ? a + b : (OP == 1 ? min(a, b) : max(a, b)); };
    x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x111, 0xf, 0xf, false));
    x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x112, 0xf, 0xf, false));
    x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x114, 0xf, 0xf, false));
    x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x118, 0xf, 0xf, false));
    x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x142, 0xa, 0xf, false));
    x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(x, 63);
}

// sqrt(v) for the iteration's sigma, which only its f32 rounding is used of.  v_rsq_f64 is good to ~2^-27; g = v y, one residual
// step g + (v - g^2) y / 2 brings it to ~2^-52 -- a few ulp(f64) short of the correctly rounded root, which the compiler's 15-
// instruction expansion (scaling, three refinement pairs, class fix-up) delivers.  That is the same order as the fast engine's
// running-sum variance itself (a few ulp(f64) from the two-pass value), 28 binary orders below the f32 the result is
// rounded to: the f32 sigma differs from the oracle's with probability ~1e-8 per pixel, as before.  No scaling: a variance of f32
// samples lies between 2^-298 and 2^+262 or is 0 (-> 0: the caller's max with 1e-10 takes over).  (AB_STACK_IEEE_SQRT: the library call.)
__device__ __forceinline__ double sqrt_for_sigma(double v) {
#ifdef AB_STACK_IEEE_SQRT
    return sqrt(v);
#else
    const double y = __builtin_amdgcn_rsq(v);
    const double g = v * y;
    const double e = __builtin_fma(-g, g, v);
    const double r = __builtin_fma(e, 0.5 * y, g);
    return v > 0.0 ? r : 0.0;
#endif
}

}  // namespace abstack

// The epilogue of the one-wave workgroups (pair, duo, quad): the wave's rejected samples through a shuffle tree, then ONE atomic per
// wave spread over AB_REJ_SLOTS counters that the host sums.  A macro on purpose: an inlined function changes the block order of
// the multi-lane fast kernels (LABNOTES.md section 12).
#define AB_TALLY_REJECTED(rejected, r)                                                                                               \
    do {                                                                                                                             \
        int tally_ = (r);                                                                                                            \
        _Pragma("unroll") for (int off = 32; off >= 1; off >>= 1) tally_ += __shfl_xor(tally_, off, 64);                             \
        if (threadIdx.x == 0 && tally_ != 0) atomicAdd(&(rejected)[blockIdx.x & (AB_REJ_SLOTS - 1)], (unsigned long long)tally_);   \
    } while (0)
