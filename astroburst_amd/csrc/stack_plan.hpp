// Where a kappa-sigma stack (or median combine) of n frames goes: the one place that chooses between the six stacking engines.
// Pure host arithmetic on <cstdint> / <cstddef> alone (tests/test_stack_plan_cpu.py builds it for the CPU and holds it to the table
// below).  ab_stack_device plans once; ab_stack_pair_device and ab_stack_wide_device launch what the plan says.
// "plain" = every plane contiguous (ld == cols), fewer than 2^30 pixels, full output (no partial sums).  np = the next power of two.
//
//   n            condition                                  route
//   1            any                                        stack_single_kernel
//   2 .. 64      n == np >= 8, contiguous, < 2^30 px,       two-pass: <NP, .., DIRECT, kFastPass>, then kGeneralPass over the lists
//                default engine, not the median
//   2 .. 64      n < np, np >= 8, contiguous, < 2^30 px     one plane of +inf pads the table up to np: single-pass DIRECT kernel
//   2 .. 64      otherwise                                  launch_stack<PARTIAL, EXACT, STAGE>, DIRECT iff n == np, contiguous, < 2^30 px
//   65 .. 128    plain, not exact                           NP = 128 DIRECT (pads up to 128): two-pass when n == 128 and not the median
//   129 .. 256   plain, default or median                   stack_lanes_fast_kernel<2, R>, then stack_pair_kernel<128> in list mode
//   257 .. 512   plain, default or median                   stack_lanes_fast_kernel<4, R>, then stack_pair_kernel<256> in list mode
//   513 .. 1024  plain, default or median                   stack_lanes_fast_kernel<8, R>, then stack_wide_list_kernel<16>
//   129 .. 512   plain, exact                               stack_pair_kernel<128 or 256> over all pixels
//   65 .. 4096   everything else                            stack_wide_*: K = 2, 4, 8, 16, 32, 64 registers per lane by n
//   > deep_from  everything that is not the NP = 128 route  stack_deep_kernel
//
// R: the frame-count class of a multi-lane fast pass, frames per lane rounded up to a multiple of 16 (the pads' loads and network
// operations vanish at compile time): 129 and 160 frames give 80, 161 gives 96, 256 / 512 / 1024 give 128, 257 and 513 give 80.
//
// Why these routes (LABNOTES.md has the measurements): 129 .. 256 samples in one lane (VGPRs + AGPRs, one wave per SIMD) took 10.6 ms
// for 256 x 4096^2, two lanes of 128 take 7.1 and the pair kernel serves the exact engine (15.5 ms, was 151 one wave per pixel); 512
// frames on two lanes of 256 samples took 36 ms, four lanes of 128 take 15; 513 x 2048^2 took 43.7 ms one wave per pixel, eight lanes
// take 9.7.  The superseded forms are retired; their A/B numbers: profiles/r05_deep_stacks.txt, profiles/r06_duo_deep_stacks.txt.
#pragma once
#include <cstddef>
#include <cstdint>

enum StackEngine {
    kEngineSingle,  // stack_sigma_clip.hip: stack_single_kernel
    kEngineLane,    // stack_sigma_clip.hip: one lane per pixel, NP = 2 .. 128 samples in registers
    kEnginePair,    // stack_pair.hip over all pixels: two lanes per pixel, the oracle's arithmetic
    kEngineLanes,   // stack_lanes.hip's fast pass (`lanes` = two, four or eight lanes per pixel), then a list pass
    kEngineWide,    // stack_wide.hip: one wave per pixel
    kEngineDeep,    // stack_deep.hip: one workgroup per pixel
};
enum StackListKernel {  // which kernel walks the lists of pixels a fast pass hands over
    kListNone,
    kListGeneral,  // stack_sigma_clip_kernel<NP, .., kGeneralPass>
    kListPair128,  // stack_pair_kernel<128> in list mode
    kListPair256,  // stack_pair_kernel<256> in list mode
    kListWide16,   // stack_wide_list_kernel<16>
};
enum StackGather { kGatherScalar, kGatherQuad, kGatherTiled };  // stack_wide.hip: stack_wide_kernel / _quad_kernel / _tile_kernel

struct StackPlan {
    int engine;    // StackEngine
    int lanes;     // lanes per pixel: 1, 2, 4, 8; 64 for the wave-per-pixel engine; 0 for the workgroup-per-pixel engine
    int np;        // kEngineLane: samples per lane (NP)
    int h;         // kEnginePair / Lanes: samples per lane of stack_pair.hip's kernel (H)
    int k;         // kEngineWide: registers per lane (K)
    int r;         // kEnginePair / Lanes: frames per lane in the pointer table (the class R of a fast pass, H for the exact kernel)
    bool pad_inf;  // a plane of +inf stands in for the frames the table is short of
    bool direct;   // kEngineLane: the DIRECT gather (all np slots filled, one row stride, byte offsets fit 32 bits)
    bool two_pass; // a fast pass over every pixel, then `list` over the pixels it handed over
    int list;      // StackListKernel
    int gather;    // kEngineWide: StackGather
    bool tree;     // kEngineWide: tree sums (the chain of ascending f64 additions otherwise)
};

// contiguous: every row stride equals cols.  partial: (sum, count) planes instead of the image.  aligned16: every plane pointer is.
inline StackPlan ab_stack_plan(size_t n, int64_t total, bool contiguous, bool partial, bool median_only, bool exact, int deep_from, bool aligned16) {
    StackPlan p = {};
    const bool small = total < (int64_t(1) << 30);  // byte offsets fit 32 bits
    const bool plain = contiguous && small && !partial;
    if (n == 1) {
        p.engine = kEngineSingle;
        p.lanes = 1;
        return p;
    }
    if (n <= 64 || (n <= 128 && plain && !exact)) {
        p.engine = kEngineLane;
        p.lanes = 1;
        p.np = 2;
        while ((size_t)p.np < n) p.np <<= 1;
        // A frame count between two powers of two would run the strided kernel, whose `f < n` predicates make it 2-3x slower (37 frames:
        // 2.7 ms against 1.3 for 64).  Contiguous planes alias one plane of +inf instead: what the algorithm ignores (combine.rs:170-175)
        p.pad_inf = n < (size_t)p.np && p.np >= 8 && contiguous && small;
        p.direct = (p.pad_inf || n == (size_t)p.np) && contiguous && small;
        // (the fast pass only looks at sorted positions NP-4 .. NP-1 for the high end: on a padded stack those are pads and every
        // pixel would be deferred, so padded stacks take the single-pass kernel)
        p.two_pass = n == (size_t)p.np && p.np >= 8 && contiguous && small && !median_only && !exact;
        p.list = p.two_pass ? kListGeneral : kListNone;
        return p;
    }
    if (n > (size_t)deep_from) {
        p.engine = kEngineDeep;
        return p;
    }
    if (plain && n > 128 && n <= 512 && exact) {
        p.engine = kEnginePair;
        p.lanes = 2;
        p.h = n > 256 ? 256 : 128;
        p.r = p.h;
        p.pad_inf = true;
        return p;
    }
    if (plain && n > 128 && n <= 1024 && !exact) {  // (the median combine too: a pixel with every sample finite needs the sort and one register)
        p.engine = kEngineLanes;
        p.lanes = n > 512 ? 8 : (n > 256 ? 4 : 2);
        p.h = n > 256 ? 256 : 128;
        p.r = (int)(((n + (size_t)p.lanes - 1) / (size_t)p.lanes + 15) / 16) * 16;
        p.pad_inf = true;
        p.two_pass = true;
        p.list = n > 512 ? kListWide16 : (p.h == 128 ? kListPair128 : kListPair256);
        return p;
    }
    p.engine = kEngineWide;
    p.lanes = 64;
    p.k = n > 2048 ? 64 : (n > 1024 ? 32 : (n > 512 ? 16 : (n > 256 ? 8 : (n > 128 ? 4 : 2))));
    // 16-byte loads: contiguous 16-byte aligned planes of 4 k pixels.  The LDS-staged form (257 frames and more) takes whole groups
    // of 256 / K adjacent pixels; 513 frames and more have no four-pixel form (four pixels' worth of 16-byte loads would not fit
    // the register file beside two sort arrays)
    const bool quad = contiguous && (total & 3) == 0 && aligned16;
    if (quad && n > 256 && total % (256 / p.k) == 0)
        p.gather = kGatherTiled;
    else if (quad && n <= 512)
        p.gather = kGatherQuad;
    else
        p.gather = kGatherScalar;
    // the tree sums: the default engine here; the partial sums of the sharded estimator and the exact engine keep the ascending chain
    p.tree = !exact && !partial;
    return p;
}

// The grid of kEngineLanes' fast pass: one wave per 64 / lanes pixels, the wave count a multiple of 8 (the kernel deals neighbouring
// pixel groups to the workgroup ids of one XCD).  The launch takes its grid from here and the list set-up its capacity.
struct StackLanesGrid {
    int64_t waves;
    int64_t px_wave;  // pixels per wave
};
inline StackLanesGrid ab_stack_lanes_grid(int lanes, int64_t total) {
    const int64_t px_wave = 64 / lanes;
    return {((total + px_wave - 1) / px_wave + 7) / 8 * 8, px_wave};
}
