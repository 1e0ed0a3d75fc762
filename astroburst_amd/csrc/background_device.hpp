// The per-pixel body of the background surface and its correction, shared by background.hip (ab_extract_background) and
// wizard_background.hip (ab_background_step): evaluate_polynomial_surface (core/imaging/background.rs:307-341) with eval_poly_inline's
// term order (:230-249) and apply_correction (:343-383).
#pragma once
#include "ab_common.hpp"

namespace {

constexpr int kMaxPolyTerms = 21;
constexpr int kPolyBlock = 256;
constexpr int kPolyPx = 4;  // pixels of a row per thread

struct PolyArgs {
    double coeffs[kMaxPolyTerms];
    int degree;
    int rows, cols;
    double row_scale, col_scale;
};

// The reference's term is (coeffs[idx] * y_pows[yp]) * x_pows[xp]: the first product is the same for every pixel of a row, so a thread
// forms the row's DEG-dependent table once and spends one multiply and one add per term and pixel -- the same operations in the same
// order, bit for bit.  DEG is a template parameter: with a run-time degree the power tables were indexed dynamically and lived in
// scratch memory (459 us for 8192^2, 0.58 TB/s of model written; round 4).
template <int DEG>
__device__ __forceinline__ void poly_row_table(const PolyArgs &p, int y, double (&cy)[(DEG + 1) * (DEG + 2) / 2]) {
    const double ny = (double)y / p.row_scale - 0.5;
    double y_pows[DEG + 1];
    y_pows[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= DEG; ++i) y_pows[i] = y_pows[i - 1] * ny;
    int idx = 0;  // coeffs[idx] * y_pows[yp] in eval_poly_inline's term order (:230-249)
#pragma unroll
    for (int total = 0; total <= DEG; ++total)
#pragma unroll
        for (int yp = total; yp >= 0; --yp) {
            cy[idx] = p.coeffs[idx] * y_pows[yp];
            ++idx;
        }
}

// `x / col_scale` stays an IEEE division unless col_scale is a power of two, where multiplying by its reciprocal is the same exact
// scaling.
template <int DEG>
__device__ __forceinline__ float poly_px(const PolyArgs &p, const double (&cy)[(DEG + 1) * (DEG + 2) / 2], int x, int pow2_cols, double inv_cols) {
    const double nx = (pow2_cols ? (double)x * inv_cols : (double)x / p.col_scale) - 0.5;
    double x_pows[DEG + 1];
    x_pows[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= DEG; ++i) x_pows[i] = x_pows[i - 1] * nx;
    double val = 0.0;
    int idx = 0;
#pragma unroll
    for (int total = 0; total <= DEG; ++total)
#pragma unroll
        for (int yp = total; yp >= 0; --yp) {
            val += cy[idx] * x_pows[total - yp];
            ++idx;
        }
    return (float)val;
}

// apply_correction (:343-383): mode 0 Subtract, 1 Divide, re-centred on the model's median
__device__ __forceinline__ float bg_apply_px(float v, float bg, int mode, float model_median) {
    if (mode == 0) return v - bg + model_median;                   // :367-369
    return fabsf(bg) > 1e-10f ? (v / bg) * model_median : v;       // :370-376
}

}  // namespace
