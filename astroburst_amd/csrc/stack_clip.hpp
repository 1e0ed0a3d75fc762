// What the one-lane-per-pixel stacking kernels share (stack_sigma_clip.hip, stack_weighted.hip): the compare-exchange forms the sorting
// networks are built from, median / MAD off the sorted samples, and the exact clipping engine.  Moved here from stack_sigma_clip.hip
// word for word; all of it is inlined into the kernels that use it.
#pragma once
#include "stack_shared.hpp"

#include <cmath>

// -inf / +inf the optimiser cannot see through (one SGPR each): v_med3_f32(x, y, -inf) IS min(x, y), but spelled fminf() -- or as
// a med3 with a literal infinity, which instcombine folds back to fminf() -- it is preceded by a canonicalising v_max_f32 x, x, x
// whenever the compiler cannot prove an operand is not a signalling NaN (a freshly loaded sample, the result of an integer
// operation).  No NaN reaches the network (non-finite samples are replaced by +inf above it).
__device__ __forceinline__ float ab_ninf() {
    float x = -__builtin_inff();
    asm("" : "+s"(x));
    return x;
}
__device__ __forceinline__ float ab_pinf() {
    float x = __builtin_inff();
    asm("" : "+s"(x));
    return x;
}
// Compare-exchange.  v_min_f32 / v_max_f32 / v_med3_f32 are half-rate on gfx950 (4.3 cycles per wave64 instruction,
// tools/valu_rate.hip), and a sorting network is nothing else.  AB_STACK_CE_XOR: the larger element is not compared for a second
// time -- the minimum is one of the two inputs bit for bit (no NaN reaches the network, denormals are not flushed), so the other
// one is a ^ b ^ min, a single v_bitop3_b32.
#if !defined(AB_STACK_NO_CE_XOR) && !defined(AB_STACK_CE_XOR)
#define AB_STACK_CE_XOR 1
#endif
#ifdef AB_STACK_CE_XOR
#define AB_CE(a, b)                                                                                                   \
    {                                                                                                                 \
        const T lo_ = __builtin_amdgcn_fmed3f(v[a], v[b], ab_ninf());                                                 \
        v[b] = __uint_as_float(__builtin_amdgcn_bitop3_b32(__float_as_uint(v[a]), __float_as_uint(v[b]), __float_as_uint(lo_), 0x96)); \
        v[a] = lo_;                                                                                                   \
    }
#else
#define AB_CE(a, b)                         \
    {                                       \
        T lo_ = fminf(v[a], v[b]);          \
        T hi_ = fmaxf(v[a], v[b]);          \
        v[a] = lo_;                         \
        v[b] = hi_;                         \
    }
#endif
// The base case of the network on four unsorted samples with the three-input operations: sort three (min3 / med3 / max3), then
// place the fourth (min, med3, med3, max) -- 7 instructions where Batcher's five compare-exchanges take 10, all of them at the
// same half rate as a two-input min / max (tools/valu_rate.hip): 48 of the sort's 1086 instructions, 1.18 -> 1.14 ms on the bench
// stack (same box, AB_LIB_PATH A/B).
#ifndef AB_STACK_NO_SORT4  // (A/B switch for tools/time_stack_bench_data.py)
#define AB_SORT4(a, b, c, d)                                                         \
    {                                                                                \
        const T x0_ = v[a], x1_ = v[b], x2_ = v[c], x3_ = v[d];                      \
        const T s0_ = fminf(fminf(x0_, x1_), x2_), s1_ = __builtin_amdgcn_fmed3f(x0_, x1_, x2_), \
                s2_ = fmaxf(fmaxf(x0_, x1_), x2_);                                   \
        v[a] = __builtin_amdgcn_fmed3f(AB_SORT4_NINF, s0_, x3_); /* = min */         \
        v[b] = __builtin_amdgcn_fmed3f(s0_, s1_, x3_);                               \
        v[c] = __builtin_amdgcn_fmed3f(s1_, s2_, x3_);                               \
        v[d] = __builtin_amdgcn_fmed3f(AB_SORT4_PINF, s2_, x3_); /* = max */         \
    }
#endif
#ifdef AB_STACK_LITERAL_INF  // (A/B: round 2's form -- the compiler turns these two into v_min / v_max + one canonicalising v_max per base case)
#define AB_SORT4_NINF (-__builtin_inff())
#define AB_SORT4_PINF (__builtin_inff())
#else
#define AB_SORT4_NINF ab_ninf()
#define AB_SORT4_PINF ab_pinf()
#endif
#include "sort_ops.hpp"  // the min / max / min3 / med3 / max3 of SortNet<NP>::sort_fused as inline assembly, AB_SN_* macros
#include "sortnet_gen.hpp"

namespace {

using namespace abstack;  // launder, opaque, wave_reduce_i32, sqrt_for_sigma

constexpr double kMadToSigma = 1.4826;  // types/constants.rs:7

// sum over sorted positions a..b of (double)v[i], ascending, one f64 add per element; the f32
// select happens before the conversion (x + 0.0 is exact).
template <int NP>
__device__ __forceinline__ double masked_sum(const float (&v)[NP], int a, int b) {
    double S = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const bool in = (unsigned)(i - a) <= (unsigned)(b - a);
        const float xs = in ? v[i] : 0.0f;
        S += (double)xs;
    }
    return S;
}

// Median and MAD of the n finite samples of one pixel from the SORTED vector v (pads = +inf on
// top), for the wave-uniform candidate median position MM = n/2 (n = 2MM or 2MM+1):
//   med = v[MM]                                                        (combine.rs:38-40)
//   MAD = (n/2)-th smallest of |v_i - med|                              (combine.rs:42-46)
// The deviations left of the median (A[j] = med - v[MM-j], ascending in j) and right of it
// (B[j] = v[MM+1+j] - med) are two sorted runs, and the k-th element of their merge is
//   min over splits i + j = k + 1 of max(A[i-1], B[j-1]);
// with k = MM the splits pair v[p] with v[p+MM]: term(p) = max(med - v[p], v[p+MM] - med),
// p = 1 .. n-MM-1, plus the p = 0 term med - v[0].  For even n the p = MM term reads the +inf pad
// at v[2MM] and drops out by itself, so one instruction stream serves both parities.
// ~2N min/max/sub instead of a second selection, and every register index is a constant.
template <int NP, int MM>
__device__ __forceinline__ void med_mad_at(const float (&v)[NP], float &med_out, float &mad_out) {
    const float med = v[MM];
    float best = med - v[0];
#pragma unroll
    for (int p = 1; p <= MM; ++p) {
        if (p + MM < NP) {
            const float a = med - v[p];
            const float b = v[p + MM] - med;
            best = fminf(best, fmaxf(a, b));
        }
    }
    med_out = med;
    mad_out = best;
}

// lanes of one wave can disagree on n/2 (non-finite samples): evaluate each position present.  `cur` is wave-uniform;
// the positions [LO, HI] are bisected (a linear chain of NP/2 compares hops over as many cold code blocks, one
// instruction-cache miss each: a padded 200-frame stack spent a quarter of its time there).
template <int NP, int LO, int HI>
__device__ __forceinline__ void med_mad_dispatch(const float (&v)[NP], int m, int cur, float &med, float &mad) {
    if constexpr (LO == HI) {
        float md, ma;
        med_mad_at<NP, LO>(v, md, ma);
        if (m == LO) {
            med = md;
            mad = ma;
        }
    } else {
        constexpr int MID = (LO + HI) / 2;
        if (cur <= MID)
            med_mad_dispatch<NP, LO, MID>(v, m, cur, med, mad);
        else
            med_mad_dispatch<NP, MID + 1, HI>(v, m, cur, med, mad);
    }
}

// Per-lane state handed from the prologue (gather + sort + median/MAD) to a clipping engine.
struct ClipResult {
    float value;   // sigma_clip_combine's f32 result
    double sum;    // f64 sum of the survivors   (partial mode)
    int len;       // number of survivors        (partial mode)
    uint32_t rej;  // rejected samples of this pixel
    bool defer = false;  // fast pass only: this pixel needs the general pass
    // exact engine only, for a caller that weighs the survivors itself (stack_weighted.hip): they are the sorted positions [a, b]
    // (len == 0: nothing survived), and last_center is what the reference falls back to then
    int a, b;
    float last_center;
};

// ---- clipping engine A: "exact" -- every iteration re-sums the survivors directly --------------
// Bit-for-bit the oracle's ORC_ORDER_ASCENDING arithmetic (two-pass mean / sum of squared
// deviations over the interval, ascending).  ~1500 VALU slots per iteration; kept as the
// in-library cross-check of the fast engine (AB_STACK_EXACT=1) and for its provable order.
template <int NP>
__device__ __forceinline__ ClipResult clip_exact(float (&v)[NP], int n, float med, float mad,
                                                 float sigma_low, float sigma_high, uint32_t max_iter) {
    float sigma = (float)fmax((double)mad * kMadToSigma, 1e-10);
    float center = med;
    int a = 0, b = n - 1, len = n;
    uint32_t rej = 0;
    float last_center = __builtin_nanf("");
    bool active = (n >= 2);

    for (uint32_t it = 0; it < max_iter; ++it) {
        if (!__any(active)) break;
        launder<NP>(v);  // keep f32->f64 conversions inside the iteration (VGPR pressure)
        if (it > 0) {
            // mean / sample variance of the survivors in f64, ascending order (combine.rs:50-60)
            const double S = masked_sum<NP>(v, a, b);
            const double nn = (double)len;
            const double mean = S / nn;
            opaque(a, b);
            double Q = 0.0;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const bool in = (unsigned)(i - a) <= (unsigned)(b - a);
                const double dd = (double)v[i] - mean;
                const double sq = dd * dd;
                Q += in ? sq : 0.0;
            }
            const double variance = Q / fmax(nn - 1.0, 1.0);
            center = (float)mean;
            sigma = (float)fmax(sqrt(variance), 1e-10);
            opaque(a, b);
        }
        const bool go = active && (len >= 2);  // `if len < 2 { break }` (combine.rs:33-35)
        if (go) last_center = center;          // combine.rs:63

        const float lo = -sigma_low * sigma;  // combine.rs:65-66
        const float hi = sigma_high * sigma;
        // survivors stay an interval of the sorted order: count what falls off either end
        int cl = 0, ch = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const bool in = (unsigned)(i - a) <= (unsigned)(b - a);
            const float dev = v[i] - center;
            cl += (in && !(dev >= lo)) ? 1 : 0;
            ch += (in && !(dev <= hi)) ? 1 : 0;
        }
        // a sample can fail both tests only if nothing survives (lo > hi or NaN thresholds)
        const int removed = (cl + ch > len) ? len : (cl + ch);
        if (go) {
            rej += (uint32_t)removed;  // combine.rs:76-78
            len -= removed;
            if (len > 0) {
                a += cl;
                b -= ch;
            } else {
                a = 1;
                b = 0;
            }
        }
        active = go && (removed != 0);  // combine.rs:80-82
    }

    // ---- result (combine.rs:20-26,85-91) ----
    launder<NP>(v);
    opaque(a, b);
    const double S = masked_sum<NP>(v, a, b);  // empty interval (a=1,b=0 or n=0) sums to 0
    ClipResult r;
    if (n == 0) {
        r.value = 0.0f;
    } else if (n == 1) {
        r.value = med;  // the single finite sample is v[0] = v[n/2]
    } else if (len == 0) {
        r.value = __builtin_isfinite(last_center) ? last_center : 0.0f;
    } else {
        r.value = (float)(S / (double)len);
    }
    r.sum = (len > 0) ? S : 0.0;
    r.len = len > 0 ? len : 0;
    r.rej = rej;
    r.a = a;
    r.b = b;
    r.last_center = last_center;
    return r;
}

}  // namespace
