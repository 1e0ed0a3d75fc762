// The per-pixel SCNR shared by color.hip (in place, over three planes) and rgb_export.hip (in registers, between the stretch and
// the packer): the closure of apply_scnr_inplace (core/imaging/scnr.rs:36-52).  fminf / fmaxf follow f32::min / max: of a NaN and a
// number, the number.  `amount` is already clamped to [0, 1] (:28) and the caller has skipped the call below 1e-7 (:29-31).
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void scnr_px(float &rv, float &gv, float &bv, int method, float amount, int preserve) {
    const float LUM_R = 0.2126f, LUM_G = 0.7152f, LUM_B = 0.0722f;
    const float INV_RB_WEIGHT = 1.0f / (LUM_R + LUM_B);
    const float limit = method == 0 ? (rv + bv) * 0.5f : fmaxf(rv, bv);
    const float g_corrected = fminf(gv, limit);
    const float g_new = gv + amount * (g_corrected - gv);
    const float delta_g = gv - g_new;
    if (preserve && delta_g > 1e-10f && rv <= 1.0f && bv <= 1.0f) {
        const float lum_lost = LUM_G * delta_g;
        const float boost = lum_lost * INV_RB_WEIGHT;
        const float rn = rv + boost, bn = bv + boost;
        rv = rn > 1.0f ? 1.0f : rn;
        bv = bn > 1.0f ? 1.0f : bn;
    }
    gv = g_new;
}

}  // namespace
