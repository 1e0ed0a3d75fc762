// The per-pixel arcsinh stretch shared by color.hip (one plane, scalars formed on the host) and wizard_stretch.hip (three planes, range
// and inv_range formed on the device): the closure of arcsinh_stretch_with_stats (core/imaging/stretch.rs:34-42).  Both callers pass the
// same f32 scalars, so the fused route equals the unfused one bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float arcsinh_px(float val, float dmin, float inv_range, float factor, float inv_denom, int apply_gamma, float gamma) {
    float r = 0.0f;
    if (__builtin_isfinite(val)) {  // stretch.rs:35-41
        float norm = (val - dmin) * inv_range;
        norm = norm < 0.0f ? 0.0f : (norm > 1.0f ? 1.0f : norm);
        const float stretched = asinhf(norm * factor) * inv_denom;
        r = apply_gamma ? powf(stretched, gamma) : stretched;
    }
    return r;
}

}  // namespace
