// Shared by the multi-lane stacking kernels (stack_pair.hip: two lanes per pixel, the oracle's arithmetic word for word; stack_lanes.hip:
// two, four or eight lanes per pixel, the fast engine's running sums): H samples per lane, the lanes of a pixel adjacent in the wave
// (lanes 2k and 2k + 1 share pixel k of the wave's 32; four or eight lanes pixel k of 16 or 8).
#pragma once
#include "stack_shared.hpp"

#include "sort_ops.hpp"
#define AB_CE(a, b)                       \
    {                                     \
        T lo_ = ab_v_min(v[a], v[b]);     \
        T hi_ = ab_v_max(v[a], v[b]);     \
        v[a] = lo_;                       \
        v[b] = hi_;                       \
    }
#define AB_SORT4(a, b, c, d)                                                                          \
    {                                                                                                 \
        const T x0_ = v[a], x1_ = v[b], x2_ = v[c], x3_ = v[d];                                       \
        const T s0_ = ab_v_min3(x0_, x1_, x2_), s1_ = ab_v_med3(x0_, x1_, x2_), s2_ = ab_v_max3(x0_, x1_, x2_); \
        v[a] = ab_v_min(s0_, x3_);                                                                    \
        v[b] = ab_v_med3(s0_, s1_, x3_);                                                              \
        v[c] = ab_v_med3(s1_, s2_, x3_);                                                              \
        v[d] = ab_v_max(s2_, x3_);                                                                    \
    }
#include "sortnet_gen.hpp"

namespace abpair {

using namespace abstack;

constexpr double kMadToSigma = 1.4826;  // types/constants.rs:7
// pixels the fast kernel hands to the oracle-arithmetic kernel: lists by wave index (one same-address atomic per deferring wave
// would serialise at ~12 ns each: stack_sigma_clip.hip), kListWaves one-wave workgroups walking each list
constexpr int kListSlots = AB_STACK_LIST_SLOTS;
constexpr int kListWaves = 2;

struct PairArgs {
    const float *const *p;  // plane pointers (device array): the even lane's slot f is p[f], the odd lane's p[half + f]
    int n;                  // frames
    int half;               // frames per lane (the table's stride): H for the exact kernels, the frame-count class R <= H for the fast ones
    int64_t total;          // pixels
    float sigma_low, sigma_high;
    uint32_t max_iter;
    float *out;
    unsigned long long *rejected;
    int median_only;  // median_combine_row_major (calibration.rs:84-125): [len/2] of the finite samples
    // the fast kernel appends to these; the exact kernel in LIST mode (list != nullptr in its copy of the arguments) walks them
    unsigned int *list_count, *list_ticket;
    int *list;
    unsigned int list_cap;
    int walk_lists;
};

// another lane's value through DPP: quad_perm, row_half_mirror or row_shl by a compile-time control word
template <int CTRL>
__device__ __forceinline__ int dppi(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dppf(float x) {
    return __builtin_bit_cast(float, dppi<CTRL>(__builtin_bit_cast(int, x)));
}
template <int CTRL>
__device__ __forceinline__ double dppd(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned int lo = (unsigned int)dppi<CTRL>((int)(unsigned int)u), hi = (unsigned int)dppi<CTRL>((int)(unsigned int)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
constexpr int kSwap1 = 0xB1;        // quad_perm [1,0,3,2]: lane q ^ 1
constexpr int kSwap2 = 0x4E;        // quad_perm [2,3,0,1]: lane q ^ 2
constexpr int kRev = 0x1B;          // quad_perm [3,2,1,0]: lane q ^ 3
constexpr int kHalfMirror = 0x141;  // row_half_mirror: lane 7 - i of every 8
// the partner lane's value (lanes 2k <-> 2k+1)
__device__ __forceinline__ float swapf(float x) { return dppf<kSwap1>(x); }
__device__ __forceinline__ int swapi(int x) { return dppi<kSwap1>(x); }
__device__ __forceinline__ double swapd(double x) { return dppd<kSwap1>(x); }

// The network's min / max are inline assembly, and the compiler's hazard recogniser does not see a VALU write inside an asm
// statement: a DPP read of such a register within two wait states returns the OLD value.  Every sample therefore passes through
// one of these (volatile, `s_nop 1` inside, the sample an in/out operand) between the network that wrote it and the first DPP
// that reads it.
template <int H>
__device__ __forceinline__ void dpp_fence(float (&v)[H]) {
#pragma unroll
    for (int i = 0; i < H; i += 8)
        asm volatile("s_nop 1" : "+v"(v[i]), "+v"(v[i + 1]), "+v"(v[i + 2]), "+v"(v[i + 3]), "+v"(v[i + 4]), "+v"(v[i + 5]), "+v"(v[i + 6]),
                     "+v"(v[i + 7]));
}

// hand the pixel to the list pass: one atomic per wave, kListSlots counters (here, not in stack_shared.hpp: it writes through PairArgs)
__device__ __forceinline__ void hand_over(const PairArgs &a, bool d, int lane, int64_t g) {
    const unsigned long long m = __ballot(d);
    if (m) {
        const int leader = (int)__builtin_ctzll(m);
        const unsigned int w = blockIdx.x;
        const unsigned int slot = (w + (w / kListSlots) * 977u) & (kListSlots - 1);
        unsigned int base = 0;
        if (lane == leader) base = atomicAdd(&a.list_count[slot], (unsigned int)__builtin_popcountll(m));
        base = __shfl(base, leader, 64);
        if (d) a.list[(size_t)slot * a.list_cap + base + (unsigned int)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (int)g;
    }
}

// in-lane bitonic merge of a bitonic sequence of H (ascending result): log2 H half-cleaner stages.  (One function per stage: as
// two nested `#pragma unroll` loops the body exceeds the pragma's size limit, the outer loop stays a loop, and the samples live
// in scratch memory.)
template <int H, int D>
__device__ __forceinline__ void half_cleaner(float (&v)[H]) {
    using T = float;
#pragma unroll
    for (int i = 0; i < H; ++i)
        if ((i & D) == 0) AB_CE(i, i + D)
}
template <int H>
__device__ __forceinline__ void bitonic_merge(float (&v)[H]) {
    static_assert(H == 128 || H == 256, "two lanes per pixel: 128 or 256 samples each");
    if constexpr (H == 256) half_cleaner<H, 128>(v);
    half_cleaner<H, 64>(v);
    half_cleaner<H, 32>(v);
    half_cleaner<H, 16>(v);
    half_cleaner<H, 8>(v);
    half_cleaner<H, 4>(v);
    half_cleaner<H, 2>(v);
    half_cleaner<H, 1>(v);
}

// One cross step -- v[i] against the partner lane's v[H - 1 - i] -- leaves the H smallest of two lanes' 2H sorted samples in the one
// lane and the H largest in the other, each a bitonic sequence.  An exchange keeps v_med3(x, partner, sel): the minimum where sel = -inf,
// the maximum where sel = +inf -- one instruction by a per-lane constant instead of min, max and a select.
template <int CTRL, int H>
__device__ __forceinline__ void cross_rev(float (&v)[H], float sel) {
#pragma unroll
    for (int i = 0; i < H / 2; ++i) {
        const float t1 = dppf<CTRL>(v[H - 1 - i]), t2 = dppf<CTRL>(v[i]);
        const float a = ab_v_med3(v[i], t1, sel), b = ab_v_med3(v[H - 1 - i], t2, sel);
        v[i] = a;
        v[H - 1 - i] = b;
    }
}
// v[i] against the partner lane's v[i]: the half-cleaner stage of distance H of a bitonic merge over two lanes
template <int CTRL, int H>
__device__ __forceinline__ void cross_same(float (&v)[H], float sel) {
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float t = dppf<CTRL>(v[i]);
        v[i] = ab_v_med3(v[i], t, sel);
    }
}
// the pair's cross step: the smaller half to the even lane, the larger to the odd lane
template <int H>
__device__ __forceinline__ void cross_step(float (&v)[H], bool odd) {
    cross_rev<kSwap1>(v, odd ? __builtin_inff() : -__builtin_inff());
}

}  // namespace abpair

// stack_lanes.hip: the fast pass of a 129 .. 1024-frame stack on L = 2, 4 or 8 lanes per pixel (129 .. 256, 257 .. 512, 513 .. 1024 frames),
// 128 samples per lane (class R of frames per lane); the arguments' table holds L R pointers
int ab_stack_lanes_launch(ab_ctx *ctx, int L, int R, const abpair::PairArgs &args);
