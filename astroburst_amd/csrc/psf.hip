// Empirical PSF estimation (gfx950): core/imaging/psf_estimation.rs, estimate_psf (:52-134) + psf_to_kernel (:136-149).
//
// The image stays in HBM; candidate lists, per-star records and a handful of scalars are all that crosses to the host.
//   1  psf_stats_kernel / psf_stats_finish_kernel   f64 sum and sum_sq, f32 max: one read of the plane, a fixed reduction tree
//                                                   (1024 partials whatever the device: the same bits from run to run)
//   2  plane_select.hip, signed keys                the [n / 2] order statistic: three histogram reads of the plane
//   3  psf_candidates_kernel                        val >= threshold and val == max of the clipped 11 x 11 window (separable
//                                                   row-max / column-max over an LDS tile with a 5-pixel halo): one read of the
//                                                   plane, a compacted list of linear indices (rerun once when the list was short)
//   4  host                                         the `visited` suppression (:203, :208, :237-245) walks the sorted list
//   5  psf_measure_kernel                           one workgroup per surviving peak: the reference's measurements, operation for
//                                                   operation (:247-274)
//   6  host                                         filter, score, stable sort, take (ab_psf_select_stars)
//   7  psf_cutout_kernel / psf_final_kernel         one workgroup per selected star, then the average (:94-113, :117-123)
// EXACTNESS: a sum the reference forms sequentially is formed sequentially here, by one lane, over values the other lanes staged (and
// sorted) in LDS -- raster order over a window, ascending order over a sorted slice.  Products and quotients are per-element and
// unfused (-ffp-contract=off); f64 sqrt and division are IEEE.  Only stddev (pass 1) is summed in another order than the reference's.
#include "entry_host.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kStatBlocks = 1024;  // fixed: the reduction tree must not depend on the device
constexpr int kTileW = 64, kTileH = 32, kHalo = 5;
constexpr int kSortCap = 15360;  // floats of LDS per workgroup: the 2 f .. 3 f annulus at f = 30 holds pi * 4500 = 14 137 lattice points
constexpr int kMaxRadius = AB_PSF_MAX_CUTOUT_RADIUS, kMaxSize = 2 * kMaxRadius + 1;

struct PsfPartial {
    double sum, sum_sq;
    float mx, pad;
};

// ---- pass 1: whole-plane statistics (:165-176) ----------------------------------------------------------------------------------
__device__ inline void block_reduce_stats(double &a, double &b, float &m, double *s1, double *s2, float *sm) {
    const int t = threadIdx.x;
    s1[t] = a;
    s2[t] = b;
    sm[t] = m;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
            s1[t] += s1[t + s];
            s2[t] += s2[t + s];
            sm[t] = sm[t + s] > sm[t] ? sm[t + s] : sm[t];
        }
        __syncthreads();
    }
    a = s1[0];
    b = s2[0];
    m = sm[0];
}

__global__ __launch_bounds__(kBlock) void psf_stats_kernel(const float *__restrict__ img, int64_t n, PsfPartial *__restrict__ parts) {
    __shared__ double s1[kBlock], s2[kBlock];
    __shared__ float sm[kBlock];
    double a = 0.0, b = 0.0;
    float m = -INFINITY;
    const int64_t stride = (int64_t)kStatBlocks * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float v = img[i];
        const double vf = (double)v;
        a += vf;
        b += vf * vf;
        if (v > m) m = v;
    }
    block_reduce_stats(a, b, m, s1, s2, sm);
    if (threadIdx.x == 0) parts[blockIdx.x] = PsfPartial{a, b, m, 0.0f};
}

__global__ __launch_bounds__(kBlock) void psf_stats_finish_kernel(const PsfPartial *__restrict__ parts, PsfPartial *__restrict__ out) {
    __shared__ double s1[kBlock], s2[kBlock];
    __shared__ float sm[kBlock];
    double a = 0.0, b = 0.0;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < kStatBlocks; i += kBlock) {
        a += parts[i].sum;
        b += parts[i].sum_sq;
        if (parts[i].mx > m) m = parts[i].mx;
    }
    block_reduce_stats(a, b, m, s1, s2, sm);
    if (threadIdx.x == 0) *out = PsfPartial{a, b, m, 0.0f};
}

// ---- pass 3: candidates (:205-235 without `visited`) ----------------------------------------------------------------------------
// A pixel inside the margins is a peak when val >= threshold and no pixel of the 11 x 11 window, clipped at the image edge, is
// strictly greater: val == max of the window.  count keeps counting past cap: the host reruns with a list of that size.
__global__ __launch_bounds__(kBlock) void psf_candidates_kernel(const float *__restrict__ img, int rows, int cols, int margin, double threshold,
                                                                unsigned int *__restrict__ list, unsigned int cap, unsigned int *__restrict__ count) {
    constexpr int LW = kTileW + 2 * kHalo, LH = kTileH + 2 * kHalo;
    __shared__ float in[LH][LW];
    __shared__ float rmax[LH][kTileW];
    __shared__ unsigned int found[kTileW * kTileH];
    __shared__ unsigned int nfound, base;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    if (threadIdx.x == 0) nfound = 0;
    for (int i = threadIdx.x; i < LH * LW; i += kBlock) {
        const int ly = i / LW, lx = i % LW;
        const int y = y0 + ly - kHalo, x = x0 + lx - kHalo;
        in[ly][lx] = (y >= 0 && y < rows && x >= 0 && x < cols) ? img[(int64_t)y * cols + x] : -INFINITY;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LH * kTileW; i += kBlock) {
        const int ly = i / kTileW, lx = i % kTileW;
        float m = in[ly][lx];
#pragma unroll
        for (int k = 1; k <= 2 * kHalo; ++k) m = fmaxf(m, in[ly][lx + k]);
        rmax[ly][lx] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTileH * kTileW; i += kBlock) {
        const int ly = i / kTileW, lx = i % kTileW;
        const int y = y0 + ly, x = x0 + lx;
        if (y < margin || y >= rows - margin || x < margin || x >= cols - margin) continue;
        const float v = in[ly + kHalo][lx + kHalo];
        if ((double)v < threshold) continue;
        float m = rmax[ly][lx];
#pragma unroll
        for (int k = 1; k <= 2 * kHalo; ++k) m = fmaxf(m, rmax[ly + k][lx]);
        if (v == m) found[atomicAdd(&nfound, 1u)] = (unsigned int)((int64_t)y * cols + x);
    }
    __syncthreads();
    if (threadIdx.x == 0) base = nfound ? atomicAdd(count, nfound) : 0u;
    __syncthreads();
    for (unsigned int i = threadIdx.x; i < nfound; i += kBlock)
        if ((uint64_t)base + i < cap) list[base + i] = found[i];
}

// ---- pass 5: measurement (:247-274) ------------------------------------------------------------------------------------------------
struct PsfMeasure {
    double x, y, peak, flux, fwhm, ellipticity, dist, snr;
    int keep;  // fwhm > 1.5 && fwhm < 20.0 && snr > 10.0 (:263)
    int err;   // an annulus larger than kSortCap (cannot happen while fwhm <= 30)
};

// f64 -> usize / i64 as Rust's `as` (saturating, NaN -> 0); values past 2^62 only ever compare as "outside the image"
__device__ inline int64_t sat_usize(double v) {
    if (!(v > 0.0)) return 0;
    return v >= 4.0e18 ? (int64_t)4000000000000000000LL : (int64_t)v;
}
__device__ inline int64_t sat_i64(double v) {
    if (v != v) return 0;
    if (v >= 4.0e18) return (int64_t)4000000000000000000LL;
    if (v <= -4.0e18) return -(int64_t)4000000000000000000LL;
    return (int64_t)v;
}

// subpixel_peak (:377-407)
__device__ inline double subpixel_peak(const float *img, int64_t h, int64_t w, int64_t ix, int64_t iy) {
    if (ix < 1 || iy < 1 || ix + 1 >= w || iy + 1 >= h) return (double)img[iy * w + ix];
    auto v = [&](int dy, int dx) { return (double)img[(iy + dy) * w + (ix + dx)]; };
    const double c = v(0, 0);
    const double dx_val = (v(0, 1) - v(0, -1)) * 0.5;
    const double dy_val = (v(1, 0) - v(-1, 0)) * 0.5;
    const double dxx = v(0, 1) + v(0, -1) - 2.0 * c;
    const double dyy = v(1, 0) + v(-1, 0) - 2.0 * c;
    const double dxy = (v(1, 1) + v(-1, -1) - v(1, -1) - v(-1, 1)) * 0.25;
    const double det = dxx * dyy - dxy * dxy;
    if (fabs(det) < 1e-12 || det < 0.0) return c;
    const double sx = -(dyy * dx_val - dxy * dy_val) / det;
    const double sy = -(dxx * dy_val - dxy * dx_val) / det;
    if (fabs(sx) > 1.0 || fabs(sy) > 1.0) return c;
    return c + 0.5 * (dx_val * sx + dy_val * sy);
}

// The pixels of rows y0 .. y1, columns x0 .. x1 (inclusive, inside the image; may be empty) that satisfy pred(px, py), appended to buf
// in RASTER order; every thread of the workgroup calls it and gets the count (entries past cap are counted, not stored).
template <class Pred>
__device__ inline int block_compact(const float *__restrict__ img, int64_t w, int64_t y0, int64_t y1, int64_t x0, int64_t x1, Pred pred,
                                    float *buf, int cap, int *wave_cnt) {
    if (y1 < y0 || x1 < x0) return 0;
    const int64_t ww = x1 - x0 + 1, total = ww * (y1 - y0 + 1);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int running = 0;
    for (int64_t b = 0; b < total; b += kBlock) {
        const int64_t i = b + threadIdx.x;
        bool in = false;
        float v = 0.0f;
        if (i < total) {
            const int64_t py = y0 + i / ww, px = x0 + i % ww;
            if (pred(px, py)) {
                in = true;
                v = img[py * w + px];
            }
        }
        const unsigned long long mask = __ballot(in);
        const int prefix = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(mask);
        __syncthreads();
        int off = running, tot = 0;
        for (int k = 0; k < kBlock / 64; ++k) {
            if (k < wv) off += wave_cnt[k];
            tot += wave_cnt[k];
        }
        if (in && off + prefix < cap) buf[off + prefix] = v;
        running += tot;
        __syncthreads();
    }
    return running;
}

// Ascending sort of x[0 .. n) in LDS, any n, no NaNs: the bitonic network in its all-ascending form (the first stage of a merge
// compares mirror images), so wires n .. 2^k - 1 can stand for +inf without being stored: an exchange with one of them never swaps.
__device__ inline void block_sort_ascending(float *x, int n) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    const int half = np2 >> 1;
    auto cmpx = [&](int lo, int hi) {
        if (hi < n) {
            const float a = x[lo], b = x[hi];
            if (b < a) {
                x[lo] = b;
                x[hi] = a;
            }
        }
    };
    for (int size = 2; size <= np2; size <<= 1) {
        __syncthreads();
        const int hs = size >> 1;
        for (int i = threadIdx.x; i < half; i += kBlock) {
            const int blk = i / hs, j = i % hs;
            cmpx(blk * size + j, blk * size + size - 1 - j);
        }
        for (int stride = size >> 2; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < half; i += kBlock) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1));
                cmpx(lo, lo | stride);
            }
        }
    }
    __syncthreads();
}

// mean of the sorted middle half (:434-441, :499-506): one lane, ascending order
__device__ inline double middle_half_mean(const float *sorted, int n) {
    if (n == 0) return 0.0;
    const int lo = n / 4;
    int hi = 3 * n / 4;
    hi = hi > lo + 1 ? hi : lo + 1;
    hi = hi < n ? hi : n;
    if (hi <= lo) return 0.0;
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += (double)sorted[i];
    return s / (double)(hi - lo);
}

__device__ inline double clamp_1_30(double v) { return v < 1.0 ? 1.0 : (v > 30.0 ? 30.0 : v); }  // f64::clamp: NaN stays NaN

__global__ __launch_bounds__(kBlock) void psf_measure_kernel(const float *__restrict__ img, int rows, int cols, const unsigned int *__restrict__ peaks,
                                                             int npeaks, double fwhm_factor, PsfMeasure *__restrict__ out) {
    __shared__ float buf[kSortCap];
    __shared__ int wave_cnt[kBlock / 64];
    __shared__ double shd[8];
    __shared__ int64_t shi[6];
    const int64_t h = rows, w = cols;
    const int tid = threadIdx.x;
    const double cx = (double)w / 2.0, cy = (double)h / 2.0;
    for (int p = blockIdx.x; p < npeaks; p += gridDim.x) {
        const int64_t x = peaks[p] % (unsigned int)cols, y = peaks[p] / (unsigned int)cols;
        // ---- centroid_subpixel radius 3 (:281-306), subpixel_peak at the peak, the rounding of measure_fwhm (:310-315)
        if (tid == 0) {
            double sum_x = 0.0, sum_y = 0.0, sum_w = 0.0;
            for (int dy = -3; dy <= 3; ++dy)
                for (int dx = -3; dx <= 3; ++dx) {
                    const int64_t ny = y + dy, nx = x + dx;
                    if (ny >= 0 && ny < h && nx >= 0 && nx < w) {
                        const double val = (double)img[ny * w + nx];
                        sum_x += (double)nx * val;
                        sum_y += (double)ny * val;
                        sum_w += val;
                    }
                }
            const double sub_x = sum_w > 0.0 ? sum_x / sum_w : (double)x;
            const double sub_y = sum_w > 0.0 ? sum_y / sum_w : (double)y;
            shd[0] = sub_x;
            shd[1] = sub_y;
            shd[2] = subpixel_peak(img, h, w, x, y);
            shi[0] = sat_usize(round(sub_x));
            shi[1] = sat_usize(round(sub_y));
        }
        __syncthreads();
        const double sub_x = shd[0], sub_y = shd[1];
        const int64_t ix = shi[0], iy = shi[1];
        const bool inside = !(ix >= w || iy >= h);
        __syncthreads();
        // ---- measure_fwhm (:308-375)
        double fwhm_major = 4.0, fwhm_minor = 4.0;  // (only lane 0's copy is meaningful)
        if (inside) {
            // estimate_local_bg radius 10 (:409-442)
            const double inner_r2 = (10.0 * 0.6) * (10.0 * 0.6), outer_r2 = 10.0 * 10.0;
            const int nbg = block_compact(
                img, w, std::max<int64_t>(iy - 10, 0), std::min<int64_t>(iy + 10, h - 1), std::max<int64_t>(ix - 10, 0), std::min<int64_t>(ix + 10, w - 1),
                [&](int64_t px, int64_t py) {
                    const int64_t dx = px - ix, dy = py - iy;
                    const double d2 = (double)(dx * dx + dy * dy);
                    return d2 >= inner_r2 && d2 <= outer_r2;
                },
                buf, kSortCap, wave_cnt);
            block_sort_ascending(buf, nbg);
            if (tid == 0) {
                const double bg = middle_half_mean(buf, nbg);
                const double peak = subpixel_peak(img, h, w, ix, iy);
                const double net_peak = peak - bg;
                shd[3] = bg;
                shd[4] = bg + net_peak * 0.5;
                shi[2] = net_peak <= 0.0 ? 0 : 1;
            }
            __syncthreads();
            const bool positive = shi[2] != 0;
            if (positive) {
                // the 25 x 25 window staged in raster order (NaN = outside the image; pixels are finite)
                for (int i = tid; i < 625; i += kBlock) {
                    const int64_t py = iy + i / 25 - 12, px = ix + i % 25 - 12;
                    buf[i] = (py < 0 || py >= h || px < 0 || px >= w) ? __builtin_nanf("") : img[py * w + px];
                }
            }
            __syncthreads();
            if (positive && tid == 0) {
                const double bg = shd[3], threshold = shd[4];
                double m_xx = 0.0, m_yy = 0.0, m_xy = 0.0, sum_w = 0.0;
                for (int i = 0; i < 625; ++i) {
                    const float pv = buf[i];
                    if (pv != pv) continue;
                    const double val = (double)pv;
                    if (val < threshold) continue;
                    const int64_t py = iy + i / 25 - 12, px = ix + i % 25 - 12;
                    const double weight = val - bg;
                    const double fx = (double)px - sub_x;
                    const double fy = (double)py - sub_y;
                    m_xx += fx * fx * weight;
                    m_yy += fy * fy * weight;
                    m_xy += fx * fy * weight;
                    sum_w += weight;
                }
                if (!(sum_w <= 0.0)) {
                    const double sigma_xx = m_xx / sum_w, sigma_yy = m_yy / sum_w, sigma_xy = m_xy / sum_w;
                    const double trace = sigma_xx + sigma_yy;
                    const double det = sigma_xx * sigma_yy - sigma_xy * sigma_xy;
                    const double disc = sqrt(fmax(trace * trace - 4.0 * det, 0.0));
                    const double lambda1 = fmax((trace + disc) / 2.0, 0.0);
                    const double lambda2 = fmax((trace - disc) / 2.0, 0.0);
                    fwhm_major = clamp_1_30(fwhm_factor * sqrt(lambda1));
                    fwhm_minor = clamp_1_30(fwhm_factor * sqrt(lambda2));
                }
            }
            __syncthreads();
        }
        // ---- fwhm, ellipticity, the two windows (:250-258, :449-452, :479-482)
        if (tid == 0) {
            const double fwhm = (fwhm_major + fwhm_minor) / 2.0;
            const double big = fmax(fwhm_major, fwhm_minor), small = fmin(fwhm_minor, fwhm_major);
            shd[3] = fwhm;
            shd[4] = big > 1e-10 ? 1.0 - small / big : 0.0;
        }
        __syncthreads();
        const double fwhm = shd[3];
        double flux = 0.0, bg_flux = 0.0;
        int err = 0;
        {   // aperture_flux (:444-465)
            const double radius = fwhm * 1.5, r2 = radius * radius;
            const int64_t y_min = sat_usize(fmax(floor(sub_y - radius), 0.0)), y_max = std::min<int64_t>(sat_usize(ceil(sub_y + radius)), h - 1);
            const int64_t x_min = sat_usize(fmax(floor(sub_x - radius), 0.0)), x_max = std::min<int64_t>(sat_usize(ceil(sub_x + radius)), w - 1);
            const int na = block_compact(
                img, w, y_min, y_max, x_min, x_max,
                [&](int64_t px, int64_t py) {
                    const double dx = (double)px - sub_x, dy = (double)py - sub_y;
                    return dx * dx + dy * dy <= r2;
                },
                buf, kSortCap, wave_cnt);
            if (na > kSortCap) err = 1;
            if (tid == 0 && !err)
                for (int i = 0; i < na; ++i) flux += (double)buf[i];
            __syncthreads();
        }
        {   // annulus_background (:467-507)
            const double inner_r = fwhm * 2.0, outer_r = fwhm * 3.0, ir2 = inner_r * inner_r, or2 = outer_r * outer_r;
            const int64_t y_min = sat_usize(fmax(floor(sub_y - outer_r), 0.0)), y_max = std::min<int64_t>(sat_usize(ceil(sub_y + outer_r)), h - 1);
            const int64_t x_min = sat_usize(fmax(floor(sub_x - outer_r), 0.0)), x_max = std::min<int64_t>(sat_usize(ceil(sub_x + outer_r)), w - 1);
            const int nb = block_compact(
                img, w, y_min, y_max, x_min, x_max,
                [&](int64_t px, int64_t py) {
                    const double dx = (double)px - sub_x, dy = (double)py - sub_y;
                    const double d2 = dx * dx + dy * dy;
                    return d2 >= ir2 && d2 <= or2;
                },
                buf, kSortCap, wave_cnt);
            if (nb > kSortCap) err = 1;
            if (!err) {
                block_sort_ascending(buf, nb);
                if (tid == 0) bg_flux = middle_half_mean(buf, nb);
            }
            __syncthreads();
        }
        if (tid == 0) {
            const double snr = bg_flux > 0.0 ? flux / sqrt(bg_flux) : flux;
            const double dist = sqrt((sub_x - cx) * (sub_x - cx) + (sub_y - cy) * (sub_y - cy));
            PsfMeasure m;
            m.x = sub_x;
            m.y = sub_y;
            m.peak = shd[2];
            m.flux = flux;
            m.fwhm = fwhm;
            m.ellipticity = shd[4];
            m.dist = dist;
            m.snr = snr;
            m.keep = (fwhm > 1.5 && fwhm < 20.0 && snr > 10.0) ? 1 : 0;
            m.err = err;
            out[p] = m;
        }
        __syncthreads();
    }
}

// ---- pass 7: cutouts and their average (:94-113, :518-619) ---------------------------------------------------------------------------
// One workgroup per selected star: extract_cutout (ok = 0: None), subpixel_center, bilinear_shift, normalize_cutout -> norm[s].
__global__ __launch_bounds__(kBlock) void psf_cutout_kernel(const float *__restrict__ img, int rows, int cols, const double *__restrict__ xy, int radius,
                                                            double *__restrict__ norm, int *__restrict__ ok) {
    __shared__ double cut[kMaxSize * kMaxSize];
    __shared__ double shifted[kMaxSize * kMaxSize];
    __shared__ double shd[3];
    __shared__ int64_t shi[3];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t h = rows, w = cols;
    const int size = 2 * radius + 1, n = size * size;
    if (tid == 0) {
        const int64_t ix = sat_i64(round(xy[2 * s])), iy = sat_i64(round(xy[2 * s + 1]));
        const int64_t x_start = ix - radius, y_start = iy - radius;
        const bool none = x_start < 0 || y_start < 0 || x_start + size > w || y_start + size > h;
        shi[0] = none ? 0 : 1;
        shi[1] = x_start;
        shi[2] = y_start;
        ok[s] = none ? 0 : 1;
    }
    __syncthreads();
    if (!shi[0]) return;
    const int64_t xs = shi[1], ys = shi[2];
    for (int i = tid; i < n; i += kBlock) cut[i] = (double)img[(ys + i / size) * w + xs + i % size];
    __syncthreads();
    if (tid == 0) {  // subpixel_center's moments, raster order (:551-562)
        double sum_x = 0.0, sum_y = 0.0, sum_w = 0.0;
        for (int yy = 0; yy < size; ++yy)
            for (int xx = 0; xx < size; ++xx) {
                const double val = cut[yy * size + xx];
                sum_x += (double)xx * val;
                sum_y += (double)yy * val;
                sum_w += val;
            }
        if (sum_w <= 0.0) {
            shi[0] = 0;  // cutout.clone()
        } else {
            const double ccx = sum_x / sum_w, ccy = sum_y / sum_w;
            shd[0] = ((double)size - 1.0) / 2.0 - ccx;
            shd[1] = ((double)size - 1.0) / 2.0 - ccy;
        }
    }
    __syncthreads();
    if (shi[0]) {  // bilinear_shift (:578-610)
        const double dx = shd[0], dy = shd[1];
        auto sample = [&](int64_t yy, int64_t xx) { return (yy >= 0 && yy < size && xx >= 0 && xx < size) ? cut[yy * size + xx] : 0.0; };
        for (int i = tid; i < n; i += kBlock) {
            const double sx = (double)(i % size) - dx, sy = (double)(i / size) - dy;
            const int64_t x0 = sat_i64(floor(sx)), y0 = sat_i64(floor(sy));
            const double fx = sx - (double)x0, fy = sy - (double)y0;
            shifted[i] = sample(y0, x0) * (1.0 - fx) * (1.0 - fy) + sample(y0, x0 + 1) * fx * (1.0 - fy) + sample(y0 + 1, x0) * (1.0 - fx) * fy +
                         sample(y0 + 1, x0 + 1) * fx * fy;
        }
    } else {
        for (int i = tid; i < n; i += kBlock) shifted[i] = cut[i];
    }
    __syncthreads();
    if (tid == 0) {  // normalize_cutout (:612-619)
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += shifted[i];
        shd[2] = sum;
    }
    __syncthreads();
    const double sum = shd[2];
    double *o = norm + (size_t)s * n;
    for (int i = tid; i < n; i += kBlock) o[i] = sum > 0.0 ? shifted[i] / sum : shifted[i];
}

struct PsfFinal {
    double spread;
    unsigned long long count;
};

// psf_sum over the extracted stars in selection order, / count, normalize_cutout, compute_spread_radius, the cast (:98-123, :621-643)
__global__ __launch_bounds__(kBlock) void psf_final_kernel(const double *__restrict__ norm, const int *__restrict__ ok, int nsel, int size,
                                                           float *__restrict__ kernel, PsfFinal *__restrict__ fin) {
    __shared__ double acc[kMaxSize * kMaxSize];
    __shared__ double shd[1];
    __shared__ int cnt;
    const int tid = threadIdx.x, n = size * size;
    if (tid == 0) {
        int c = 0;
        for (int k = 0; k < nsel; ++k) c += ok[k] ? 1 : 0;
        cnt = c;
    }
    __syncthreads();
    const int count = cnt;
    if (count == 0) {
        if (tid == 0) *fin = PsfFinal{0.0, 0ull};
        return;
    }
    for (int e = tid; e < n; e += kBlock) {
        double s = 0.0;
        for (int k = 0; k < nsel; ++k)
            if (ok[k]) s += norm[(size_t)k * n + e];
        acc[e] = s / (double)count;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += acc[i];
        shd[0] = sum;
    }
    __syncthreads();
    const double sum = shd[0];
    if (sum > 0.0)
        for (int e = tid; e < n; e += kBlock) acc[e] = acc[e] / sum;
    __syncthreads();
    if (tid == 0) {
        const double c = ((double)size - 1.0) / 2.0;
        double sum_r2_w = 0.0, sum_w = 0.0;
        for (int yy = 0; yy < size; ++yy)
            for (int xx = 0; xx < size; ++xx) {
                const double val = acc[yy * size + xx];
                const double r2 = ((double)xx - c) * ((double)xx - c) + ((double)yy - c) * ((double)yy - c);
                sum_r2_w += r2 * val;
                sum_w += val;
            }
        *fin = PsfFinal{sum_w > 0.0 ? sqrt(sum_r2_w / sum_w) : 0.0, (unsigned long long)count};
    }
    for (int e = tid; e < n; e += kBlock) kernel[e] = (float)acc[e];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// score_star (:509-516)
double score_star(const ab_psf_star &s) {
    const double roundness_score = 1.0 - s.ellipticity;
    const double snr_score = std::fmin(s.snr / 100.0, 1.0);
    const double center_score = 1.0 / (1.0 + s.distance_from_center / 500.0);
    const double fwhm_consistency = 1.0 / (1.0 + std::fabs(s.fwhm - 4.0) / 4.0);
    return roundness_score * 0.35 + snr_score * 0.30 + center_score * 0.15 + fwhm_consistency * 0.20;
}

// the filter (:68-84), the stable descending sort (:90): indices of every star that passed, best first
std::vector<size_t> select_stars(const ab_psf_star *stars, size_t n, const ab_psf_estimation_config &cfg, double max_val, int64_t rows, int64_t cols) {
    const double cx = (double)cols / 2.0, cy = (double)rows / 2.0;
    const double max_dist = std::sqrt(cx * cx + cy * cy) * cfg.max_center_distance_fraction;
    const double margin = (double)cfg.edge_margin;
    // (w - margin in usize wraps in the reference when margin > w; ab_estimate_psf refuses that case, here the difference is signed)
    const double x_hi = (double)(cols - (int64_t)cfg.edge_margin), y_hi = (double)(rows - (int64_t)cfg.edge_margin);
    std::vector<size_t> idx;
    std::vector<double> score;
    for (size_t i = 0; i < n; ++i) {
        const ab_psf_star &s = stars[i];
        const double norm_peak = s.peak / max_val;
        const bool in_bounds = s.x >= margin && s.y >= margin && s.x < x_hi && s.y < y_hi;
        const bool not_saturated = norm_peak < cfg.saturation_threshold;
        const bool bright_enough = norm_peak > cfg.min_peak_fraction;
        const bool round_enough = s.ellipticity < cfg.max_ellipticity;
        const bool close_enough = s.distance_from_center < max_dist;
        if (in_bounds && not_saturated && bright_enough && round_enough && close_enough) {
            idx.push_back(i);
            score.push_back(score_star(s));
        }
    }
    std::vector<size_t> order(idx.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    // score_star(b).partial_cmp(&score_star(a)).unwrap_or(Equal): a before b iff score(b) < score(a); NaN compares Equal
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return score[b] < score[a]; });
    std::vector<size_t> out(order.size());
    for (size_t i = 0; i < order.size(); ++i) out[i] = idx[order[i]];
    return out;
}

int estimate_device(ab_ctx *ctx, const float *img, int64_t rows, int64_t cols, const ab_psf_estimation_config &cfg, ab_plane_mut *kernel_out,
                    ab_psf_star *stars_out, size_t stars_cap, ab_psf_result *res) {
    const int64_t n = rows * cols;
    const int radius = (int)cfg.cutout_radius, size = 2 * radius + 1, ksz = size * size;
    const int margin = (int)cfg.edge_margin;
    // ---- fixed block: partials, the reduced statistics, the candidate counter, the final scalars, the f32 kernel
    const size_t off_stat = align256(sizeof(PsfPartial) * kStatBlocks), off_cnt = off_stat + 256, off_fin = off_cnt + 256, off_k = off_fin + 256;
    char *ws = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_PSF, off_k + sizeof(float) * kMaxSize * kMaxSize, (void **)&ws));
    PsfPartial *parts = (PsfPartial *)ws, *stat_dev = (PsfPartial *)(ws + off_stat);
    unsigned int *count_dev = (unsigned int *)(ws + off_cnt);
    PsfFinal *fin_dev = (PsfFinal *)(ws + off_fin);
    float *kernel_dev = (float *)(ws + off_k);

    // ---- compute_image_stats (:158-188)
    hipLaunchKernelGGL(psf_stats_kernel, dim3(kStatBlocks), dim3(kBlock), 0, ctx->stream, img, n, parts);
    hipLaunchKernelGGL(psf_stats_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, (const PsfPartial *)parts, stat_dev);
    AB_HIP(ctx, hipGetLastError());
    PsfPartial st;
    AB_HIP(ctx, hipMemcpyAsync(&st, stat_dev, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // (a finite f32 squared and summed 2^31 times stays far below DBL_MAX: sum_sq is non-finite iff a pixel is)
    AB_CHECK(ctx, std::isfinite(st.sum_sq), "the image holds a non-finite pixel");
    const double nf = (double)n;
    const double mean = st.sum / nf;
    const double var = (st.sum_sq / nf) - mean * mean;
    const double stddev = var > 0.0 ? std::sqrt(var) : 0.0;
    const double max_val = (double)st.mx;
    ab_plane_sel sel;
    sel.data = img;
    sel.n = n;
    sel.cube_rule = AB_SEL_VALID_FINITE;  // signed keys, no pixel dropped
    sel.frame_len = n;
    sel.frame_step = 1;
    float median_f = 0.0f;
    uint64_t counted = 0;
    AB_TRY(ab_plane_select_ranks(
        ctx, sel, 1,
        [](uint64_t count, uint64_t *ranks) {
            ranks[0] = count / 2;
            return 1;
        },
        &counted, &median_f));
    if (counted != (uint64_t)n) return ab_set_error(ctx, AB_ERR_INVALID, "the image holds a non-finite pixel");
    const double threshold = (double)median_f + 5.0 * stddev;

    // ---- candidates: a list sized for a sparse field first, the exact size when that was short (a constant plane: every pixel)
    const dim3 cgrid(ab_div_up(cols, kTileW), ab_div_up(rows, kTileH));
    unsigned int cap = (unsigned int)std::max<int64_t>(4096, n / 1024), found = 0;
    unsigned int *list_dev = nullptr;
    for (int attempt = 0; attempt < 2; ++attempt) {
        AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SCOPE0, (size_t)cap * sizeof(unsigned int), (void **)&list_dev));
        AB_HIP(ctx, hipMemsetAsync(count_dev, 0, sizeof(unsigned int), ctx->stream));
        hipLaunchKernelGGL(psf_candidates_kernel, cgrid, dim3(kBlock), 0, ctx->stream, img, (int)rows, (int)cols, margin, threshold, list_dev, cap, count_dev);
        AB_HIP(ctx, hipGetLastError());
        AB_HIP(ctx, hipMemcpyAsync(&found, count_dev, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (found <= cap) break;
        if (attempt == 1) return ab_set_error(ctx, AB_ERR_HIP, "the candidate count changed between two passes over the same plane");
        cap = found;
    }
    std::vector<unsigned int> cand(found);
    if (found) {
        AB_HIP(ctx, hipMemcpyAsync(cand.data(), list_dev, (size_t)found * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    // ---- `visited` (:203, :208, :237-245): raster order; a kept peak marks rows y .. y + 5 of columns x - 5 .. x + 5 for the pixels still to
    // come, whether or not it passes the fwhm / snr gate later.  vis_until[x] = the last marked row of column x.
    std::sort(cand.begin(), cand.end());
    std::vector<int64_t> vis_until((size_t)cols, -1);
    std::vector<unsigned int> peaks;
    for (unsigned int idx : cand) {
        const int64_t y = idx / (unsigned int)cols, x = idx % (unsigned int)cols;
        if (vis_until[(size_t)x] >= y) continue;
        peaks.push_back(idx);
        for (int64_t xx = std::max<int64_t>(0, x - 5); xx <= std::min<int64_t>(cols - 1, x + 5); ++xx) vis_until[(size_t)xx] = y + 5;
    }
    AB_TRY(ab_cancel_point(ctx));

    // ---- measurement
    std::vector<ab_psf_star> stars;
    if (!peaks.empty()) {
        const size_t np = peaks.size();
        AB_CHECK(ctx, np < ((size_t)1 << 31), "too many peaks");
        const size_t off_rec = align256(np * sizeof(unsigned int));
        char *mws = nullptr;
        AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SCOPE1, off_rec + np * sizeof(PsfMeasure), (void **)&mws));
        unsigned int *peaks_dev = (unsigned int *)mws;
        PsfMeasure *rec_dev = (PsfMeasure *)(mws + off_rec);
        AB_HIP(ctx, hipMemcpyAsync(peaks_dev, peaks.data(), np * sizeof(unsigned int), hipMemcpyHostToDevice, ctx->stream));
        const double fwhm_factor = 2.0 * std::sqrt(std::log(2.0) * 2.0);  // (:367)
        const int grid = (int)std::min<size_t>(np, (size_t)1 << 20);
        hipLaunchKernelGGL(psf_measure_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, img, (int)rows, (int)cols, (const unsigned int *)peaks_dev, (int)np,
                           fwhm_factor, rec_dev);
        AB_HIP(ctx, hipGetLastError());
        std::vector<PsfMeasure> rec(np);
        AB_HIP(ctx, hipMemcpyAsync(rec.data(), rec_dev, np * sizeof(PsfMeasure), hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (const PsfMeasure &m : rec) {
            if (m.err) return ab_set_error(ctx, AB_ERR_UNSUPPORTED, "a star's background annulus holds more than %d pixels", kSortCap);
            if (m.keep) stars.push_back(ab_psf_star{m.x, m.y, m.peak, m.flux, m.fwhm, m.ellipticity, m.dist, m.snr});
        }
    }
    res->stars_detected = stars.size();
    if (stars.empty()) {
        res->outcome = AB_PSF_NO_STARS_DETECTED;
        return AB_OK;
    }
    // ---- selection (:68-92)
    const std::vector<size_t> order = select_stars(stars.data(), stars.size(), cfg, max_val, rows, cols);
    res->stars_filtered = order.size();
    if (order.empty()) {
        res->outcome = AB_PSF_NO_STARS_PASSED;
        return AB_OK;
    }
    const size_t nsel = std::min(order.size(), cfg.num_stars);
    AB_CHECK(ctx, nsel < ((size_t)1 << 24), "num_stars is too large for this build");

    // ---- cutouts and their average (:94-123)
    std::vector<double> xy(2 * nsel);
    for (size_t k = 0; k < nsel; ++k) {
        xy[2 * k] = stars[order[k]].x;
        xy[2 * k + 1] = stars[order[k]].y;
    }
    const size_t off_ok = align256(2 * nsel * sizeof(double)), off_norm = off_ok + align256(nsel * sizeof(int));
    char *aws = nullptr;
    AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SCOPE2, off_norm + nsel * (size_t)ksz * sizeof(double), (void **)&aws));
    double *xy_dev = (double *)aws, *norm_dev = (double *)(aws + off_norm);
    int *ok_dev = (int *)(aws + off_ok);
    AB_HIP(ctx, hipMemcpyAsync(xy_dev, xy.data(), 2 * nsel * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(psf_cutout_kernel, dim3((unsigned int)nsel), dim3(kBlock), 0, ctx->stream, img, (int)rows, (int)cols, (const double *)xy_dev, radius,
                       norm_dev, ok_dev);
    hipLaunchKernelGGL(psf_final_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, (const double *)norm_dev, (const int *)ok_dev, (int)nsel, size, kernel_dev,
                       fin_dev);
    AB_HIP(ctx, hipGetLastError());
    PsfFinal fin;
    AB_HIP(ctx, hipMemcpyAsync(&fin, fin_dev, sizeof fin, hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (fin.count == 0) {
        res->outcome = AB_PSF_NO_CUTOUTS;
        return AB_OK;
    }
    AB_HIP(ctx, hipMemcpyAsync(kernel_out->data, kernel_dev, (size_t)ksz * sizeof(float), kernel_out->on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                               ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double sum_fwhm = 0.0, sum_ell = 0.0;
    for (size_t k = 0; k < nsel; ++k) {
        sum_fwhm += stars[order[k]].fwhm;
        sum_ell += stars[order[k]].ellipticity;
        if (k < stars_cap) stars_out[k] = stars[order[k]];
    }
    res->outcome = AB_PSF_OK;
    res->average_fwhm = sum_fwhm / (double)nsel;
    res->average_ellipticity = sum_ell / (double)nsel;
    res->spread_pixels = fin.spread;
    res->stars_used = nsel;
    res->stars_rejected = order.size() >= (size_t)fin.count ? order.size() - (size_t)fin.count : 0;  // saturating_sub (:131)
    return AB_OK;
}

}  // namespace

extern "C" {

void ab_psf_estimation_config_default(ab_psf_estimation_config *cfg) {
    if (!cfg) return;
    cfg->num_stars = 30;
    cfg->cutout_radius = 15;
    cfg->saturation_threshold = 0.95;
    cfg->min_peak_fraction = 0.10;
    cfg->max_ellipticity = 0.3;
    cfg->edge_margin = 30;
    cfg->max_center_distance_fraction = 0.7;
}

int ab_psf_select_stars(const ab_psf_star *stars, size_t n, const ab_psf_estimation_config *cfg, double max_val, int64_t rows, int64_t cols,
                        size_t *out_idx, size_t cap, size_t *out_selected, size_t *out_filtered) try {
    if (!cfg || (!stars && n > 0) || (!out_idx && cap > 0)) return AB_ERR_INVALID;
    const std::vector<size_t> order = select_stars(stars, n, *cfg, max_val, rows, cols);
    const size_t take = std::min(std::min(order.size(), cfg->num_stars), cap);
    for (size_t k = 0; k < take; ++k) out_idx[k] = order[k];
    if (out_selected) *out_selected = take;
    if (out_filtered) *out_filtered = order.size();
    return AB_OK;
} AB_CATCH_NOCTX

int ab_estimate_psf(ab_ctx *ctx, const ab_plane *img, const ab_psf_estimation_config *cfg, ab_plane_mut *kernel_out, ab_psf_star *stars_out,
                    size_t stars_cap, ab_psf_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, img && cfg && kernel_out && res && (stars_out || stars_cap == 0), "null argument");
    AB_CHECK(ctx, img->data && img->rows > 0 && img->cols > 0, "the image is empty");
    AB_CHECK(ctx, img->rows * img->cols < (int64_t(1) << 31), "image too large for this build");
    AB_CHECK(ctx, cfg->num_stars > 0, "num_stars must be at least 1");
    AB_CHECK(ctx, cfg->edge_margin < ((size_t)1 << 30) && img->rows > 2 * (int64_t)cfg->edge_margin && img->cols > 2 * (int64_t)cfg->edge_margin,
             "rows and cols must exceed 2 * edge_margin (%zu): the image is %lld x %lld", cfg->edge_margin, (long long)img->rows, (long long)img->cols);
    if (cfg->cutout_radius > (size_t)AB_PSF_MAX_CUTOUT_RADIUS)
        return ab_set_error(ctx, AB_ERR_UNSUPPORTED, "cutout_radius %zu exceeds AB_PSF_MAX_CUTOUT_RADIUS (%d)", cfg->cutout_radius, AB_PSF_MAX_CUTOUT_RADIUS);
    const int64_t size = 2 * (int64_t)cfg->cutout_radius + 1;
    AB_CHECK(ctx, kernel_out->data && kernel_out->rows == size && kernel_out->cols == size, "the kernel plane must be %lld x %lld", (long long)size,
             (long long)size);
    *res = ab_psf_result{};
    res->kernel_size = (size_t)size;
    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    const float *in = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    return estimate_device(ctx, in, img->rows, img->cols, *cfg, kernel_out, stars_out, stars_cap, res);
} AB_CATCH(ctx)

}  // extern "C"
