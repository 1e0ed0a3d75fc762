// The per-pixel bodies of the RGB compose panel shared by compose_rgb.hip (compose_stf_kernel), extras.hip (lrgb_kernel) and
// compose_step.hip (compose_finish_kernel, in registers): the compose-local apply_stf_inplace (core/compose/rgb.rs:191-207 -- NOT
// apply_stf_f32: it divides by the clip range and has its own validity test) and the closure of apply_lrgb (core/compose/lrgb.rs:25-42).
// Compiled with -ffp-contract=off like everything else; each caller gets the same instruction sequence.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct ComposeStf {  // rgb.rs:192-197
    double dmin, inv_range, shadow, clip_range, m;
};

__device__ __forceinline__ float compose_stf_px(float v, const ComposeStf &t) {  // rgb.rs:199-206
    if (!__builtin_isfinite(v) || v <= 1e-7f) return 0.0f;
    const double norm = ((double)v - t.dmin) * t.inv_range;
    double clipped = (norm - t.shadow) / t.clip_range;
    clipped = clipped < 0.0 ? 0.0 : (clipped > 1.0 ? 1.0 : clipped);
    if (clipped <= 0.0) return 0.0f;
    if (clipped >= 1.0) return 1.0f;
    return (float)((t.m - 1.0) * clipped / ((2.0 * t.m - 1.0) * clipped - t.m));
}

__device__ __forceinline__ float lrgb_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__device__ __forceinline__ void lrgb_px(float lum_new, float &rv, float &gv, float &bv, float lw, float cw) {  // lrgb.rs:25-42
    const float lum_old = rv * 0.2126f + gv * 0.7152f + bv * 0.0722f;
    if (lum_old < 1e-10f) {
        const float blended = lum_new * lw;
        rv = blended, gv = blended, bv = blended;
        return;
    }
    const float ratio = (lum_new * lw + lum_old * (1.0f - lw)) / lum_old;
    const float rn = lrgb_clamp01(rv * ratio * cw + lum_new * (1.0f - cw));
    const float gn = lrgb_clamp01(gv * ratio * cw + lum_new * (1.0f - cw));
    const float bn = lrgb_clamp01(bv * ratio * cw + lum_new * (1.0f - cw));
    rv = rn, gv = gn, bv = bn;
}

}  // namespace
