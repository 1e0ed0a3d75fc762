// The synthetic star-field generator, core/synth/{star_field,psf,noise,pipeline}.rs (generate_synth_cmd, generate_synth_stack_cmd).
//
// Every random number of the reference comes from StdRng::seed_from_u64 = ChaCha12 (chacha12.hpp): a draw's position in the stream
// decides its value, so wherever the number of draws per pixel is fixed each lane computes its own block of the stream.
//   star fields       host loops of scalar maths over one stream (glibc pow / cos / sin / log, as Rust's f64 methods)
//   render_stars      pass A: one workgroup per star sums evaluate() over the clamped window (fixed tree) -> norm = flux / psf_sum and
//                     the skip flag; the stars are binned on the host into 16 x 16 output tiles, each list in ascending star index;
//                     pass B: one lane per output pixel walks its tile's list in order and accumulates the f32 addends -- the
//                     reference's order of additions, no atomics, no dependence on launch order
//   flat field        pixel i takes draw i: one lane per ChaCha block = eight pixels
//   apply_noise       fast route: every pixel with signal_e >= 30 takes four draws: one lane per block = two adjacent pixels; the
//                     kernel raises a flag when a pixel is below 30 or non-finite, and the frame is then recomputed on the host by
//                     the reference's serial walk (Knuth's loop draws a data-dependent number of times)
// The host parts (stream, star fields, binning, the serial walks) use no device code.  The exactness contract is in the header.
#include <algorithm>
#include <cmath>

#include "entry_host.hpp"

#include "chacha12.hpp"

namespace {

constexpr int kTile = 16;  // pass B: 16 x 16 pixels per workgroup
constexpr double kTwoPi = 2.0 * 3.14159265358979323846;

// ---- host scalar parts -------------------------------------------------------------------------------------------------------------

// power_law_flux (star_field.rs:44-50)
double power_law_flux(ab_chacha_stream &rng, double flux_min, double flux_max) {
    const double alpha = 2.5;
    const double f_min_inv = std::pow(flux_min, 1.0 - alpha);
    const double f_max_inv = std::pow(flux_max, 1.0 - alpha);
    const double u = rng.draw();
    return std::pow(f_min_inv + u * (f_max_inv - f_min_inv), 1.0 / (1.0 - alpha));
}

// gen_field (pipeline.rs:126-138); AB_ERR_INVALID (message in *why) for what would not terminate
int star_field(const ab_synth_config &cfg, std::vector<ab_synth_star> *out, const char **why) {
    const ab_synth_field_config &f = cfg.field;
    const double a = cfg.field_type.a, b = cfg.field_type.b;
    const double width = (double)f.width, height = (double)f.height;
    ab_chacha_stream rng(f.seed);
    out->clear();
    switch (cfg.field_type.kind) {
    case AB_SYNTH_FIELD_UNIFORM:  // (:52-66)
        out->reserve(f.n_stars);
        for (size_t i = 0; i < f.n_stars; ++i) {
            ab_synth_star s;
            s.flux = power_law_flux(rng, f.flux_min, f.flux_max);
            s.x = rng.draw() * width;
            s.y = rng.draw() * height;
            s.z = 0.0;
            s.temperature = 3000.0 + rng.draw() * 27000.0;
            out->push_back(s);
        }
        return AB_OK;
    case AB_SYNTH_FIELD_KING_CLUSTER: {  // (:68-93) a = core_radius, b = tidal_radius
        if (!(std::isfinite(a) && a > 0.0 && std::isfinite(b) && b > 0.0)) {
            *why = "king_cluster: core_radius and tidal_radius must be positive and finite";
            return AB_ERR_INVALID;
        }
        const double cx = width * 0.5, cy = height * 0.5;
        const double c = b / a;
        const double king_norm = 1.0 / std::sqrt(1.0 + c * c);
        if (!(1.0 - king_norm > 0.0)) {  // the profile's maximum (r = 0): nothing is ever accepted
            *why = "king_cluster: tidal_radius / core_radius is too small for the profile to accept a star";
            return AB_ERR_INVALID;
        }
        out->reserve(f.n_stars);
        while (out->size() < f.n_stars) {
            const double r = rng.draw() * b;
            const double q = r / a;
            double d = 1.0 / std::sqrt(1.0 + q * q) - king_norm;
            d = d > 0.0 ? d : 0.0;  // f64::max(0.0)
            const double profile = d * d;
            if (rng.draw() < profile) {
                const double theta = rng.draw() * 2.0 * M_PI;
                ab_synth_star s;
                s.flux = power_law_flux(rng, f.flux_min, f.flux_max);
                s.x = cx + r * std::cos(theta);
                s.y = cy + r * std::sin(theta);
                s.z = 0.0;
                s.temperature = 3000.0 + rng.draw() * 27000.0;
                out->push_back(s);
            }
        }
        return AB_OK;
    }
    case AB_SYNTH_FIELD_EXPONENTIAL_DISK: {  // (:95-119) a = scale_length, b = inclination_deg
        const double cx = width * 0.5, cy = height * 0.5;
        const double cos_i = std::cos(b * M_PI / 180.0);
        out->reserve(f.n_stars);
        for (size_t i = 0; i < f.n_stars; ++i) {
            const double d = rng.draw();
            const double u = d < 1.0 - 1e-10 ? d : 1.0 - 1e-10;  // f64::min
            const double r = -a * std::log(1.0 - u);
            const double theta = rng.draw() * 2.0 * M_PI;
            ab_synth_star s;
            s.flux = power_law_flux(rng, f.flux_min, f.flux_max);
            s.x = cx + r * std::cos(theta);
            s.y = cy + r * std::sin(theta) * cos_i;
            s.z = rng.draw() * a * 0.1;
            s.temperature = 3000.0 + rng.draw() * 27000.0;
            out->push_back(s);
        }
        return AB_OK;
    }
    default:
        *why = "unknown field_type.kind";
        return AB_ERR_INVALID;
    }
}

struct NoiseP {
    double gain, readout, sky, dark, exposure, bias;
};
NoiseP noise_p(const ab_synth_noise_params &p) { return NoiseP{p.gain, p.readout_noise, p.sky_background, p.dark_current, p.exposure_time, p.bias_level}; }

// `as u64` of a rounded, non-negative sample, back `as f64`: saturates at u64::MAX, which rounds to 2^64
__host__ __device__ __forceinline__ double photon_count(double sample) { return fmin(fmax(round(sample), 0.0), 0x1p64); }

// BoxMullerNormal::sample (noise.rs:34-40)
double box_muller(ab_chacha_stream &rng, double mean, double sd) {
    const double u1 = std::fmax(rng.draw(), 1e-30);
    const double u2 = rng.draw();
    return mean + sd * std::sqrt(-2.0 * std::log(u1)) * std::cos(kTwoPi * u2);
}

// apply_noise (noise.rs:62-79), the serial walk: any input
void host_apply_noise(const float *img, int64_t n, uint64_t seed, const NoiseP &p, float *out) {
    ab_chacha_stream rng(seed);
    for (int64_t i = 0; i < n; ++i) {
        const double flux = (double)img[i];
        const double signal_e = (flux + p.sky) * p.gain * p.exposure + p.dark * p.exposure;
        const double lambda = std::fmax(signal_e, 0.0);  // f64::max: NaN -> 0.0
        double photon = 0.0;
        if (lambda <= 0.0) {
        } else if (lambda < 30.0) {  // Knuth (:46-55)
            const double l = std::exp(-lambda);
            uint64_t k = 0;
            double prod = 1.0;
            for (;;) {
                ++k;
                prod *= rng.draw();
                if (prod <= l) break;
            }
            photon = (double)(k - 1);
        } else {
            photon = photon_count(lambda + std::sqrt(lambda) * box_muller(rng, 0.0, 1.0));
        }
        const double read_e = box_muller(rng, 0.0, p.readout);
        out[i] = (float)std::fmax((photon + read_e + p.bias) / p.gain, 0.0);
    }
}

// generate_flat_field (noise.rs:81-99)
void host_flat_field(int64_t rows, int64_t cols, uint64_t seed, double vs, float *out) {
    ab_chacha_stream rng(seed);
    const double cx = (double)cols * 0.5, cy = (double)rows * 0.5;
    const double max_r = std::sqrt(cx * cx + cy * cy);
    for (int64_t y = 0; y < rows; ++y)
        for (int64_t x = 0; x < cols; ++x) {
            const double dx = (double)x - cx, dy = (double)y - cy;
            const double r = std::sqrt(dx * dx + dy * dy) / max_r;
            out[y * cols + x] = (float)std::fmax((1.0 - vs * r * r) * (1.0 + rng.draw() * 0.02 - 0.01), 0.01);
        }
}

void host_apply_flat(float *img, const float *flat, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (flat[i] > 1e-6f) img[i] /= flat[i];
}

// make_psf (pipeline.rs:140-146) + the constructors of psf.rs: evaluate()'s constants and psf_r = radius().ceil()
struct PsfParams {
    int kind;
    double p0;  // Gaussian: inv_2sigma_sq; Moffat: inv_alpha_sq; Airy: scale
    double p1;  // Moffat: beta
};

int make_psf(ab_ctx *ctx, const ab_synth_psf_type &t, PsfParams *p, int64_t *psf_r) {
    double radius = 0.0;
    p->kind = t.kind;
    p->p1 = 0.0;
    switch (t.kind) {
    case AB_SYNTH_PSF_GAUSSIAN: {
        AB_CHECK(ctx, std::isfinite(t.fwhm) && t.fwhm > 0.0, "Gaussian PSF: fwhm must be positive and finite");
        const double sigma = t.fwhm / 2.3548;
        p->p0 = 1.0 / (2.0 * sigma * sigma);
        radius = sigma * 4.0;
        break;
    }
    case AB_SYNTH_PSF_MOFFAT: {
        AB_CHECK(ctx, std::isfinite(t.fwhm) && t.fwhm > 0.0 && std::isfinite(t.beta) && t.beta > 0.0, "Moffat PSF: fwhm and beta must be positive and finite");
        const double alpha = t.fwhm / (2.0 * std::sqrt(std::pow(2.0, 1.0 / t.beta) - 1.0));
        p->p0 = 1.0 / (alpha * alpha);
        p->p1 = t.beta;
        radius = alpha * 5.0;
        break;
    }
    case AB_SYNTH_PSF_AIRY:
        AB_CHECK(ctx, std::isfinite(t.fwhm) && t.fwhm > 0.0, "Airy PSF: lambda_over_d must be positive and finite");
        p->p0 = M_PI / t.fwhm;
        radius = t.fwhm * 4.0;
        break;
    default:
        return ab_set_error(ctx, AB_ERR_INVALID, "unknown psf_type.kind %d", t.kind);
    }
    AB_CHECK(ctx, std::isfinite(radius) && std::isfinite(p->p0) && p->p0 > 0.0, "the PSF parameters give a non-finite radius or scale");
    if (std::ceil(radius) > (double)AB_SYNTH_MAX_PSF_RADIUS)
        return ab_set_error(ctx, AB_ERR_UNSUPPORTED, "psf_r = %.0f exceeds AB_SYNTH_MAX_PSF_RADIUS (%d)", std::ceil(radius), AB_SYNTH_MAX_PSF_RADIUS);
    *psf_r = (int64_t)std::ceil(radius);
    return AB_OK;
}

// a star with its window clamped to the image (psf.rs:136-139): x0 <= x1 and y0 <= y1 for every record that reaches the device
struct StarRec {
    double sx, sy, flux;
    int x0, x1, y0, y1;
};
struct StarNorm {
    double norm;
    int skip, pad;
};

// the window's bounds along one axis; false when it is empty -- wholly beyond the far edge (the reference's empty range) or wholly
// before the near one (where the reference's `as usize` wraps: the deliberate difference named in the header)
bool window(double s, int64_t psf_r, int64_t extent, int *lo, int *hi) {
    const double r = (double)psf_r;
    const double l = std::floor(s - r), h = std::ceil(s + r);
    if (!(l <= (double)(extent - 1)) || !(h >= 0.0)) return false;
    *lo = (int)std::fmax(l, 0.0);
    *hi = (int)std::fmin(h, (double)(extent - 1));
    return *lo <= *hi;
}

// the stars whose windows meet the image, in list order
std::vector<StarRec> clamp_stars(const ab_synth_star *stars, size_t n, int64_t psf_r, int64_t rows, int64_t cols) {
    std::vector<StarRec> recs;
    for (size_t i = 0; i < n; ++i) {
        StarRec r;
        r.sx = stars[i].x, r.sy = stars[i].y, r.flux = stars[i].flux;
        if (window(r.sx, psf_r, cols, &r.x0, &r.x1) && window(r.sy, psf_r, rows, &r.y0, &r.y1)) recs.push_back(r);
    }
    return recs;
}

// CSR lists of the records whose windows touch each kTile x kTile tile (tx x ty tiles): count, prefix, fill in record order -> every
// list ascending.  Returns the number of entries; at 2^31 or more nothing is filled.
uint64_t bin_stars(const std::vector<StarRec> &recs, int tx, int ty, std::vector<unsigned int> *off, std::vector<int> *idx) {
    const size_t ntiles = (size_t)tx * (size_t)ty;
    off->assign(ntiles + 1, 0u);
    idx->clear();
    uint64_t entries = 0;
    for (const StarRec &r : recs)
        for (int y = r.y0 / kTile; y <= r.y1 / kTile; ++y)
            for (int x = r.x0 / kTile; x <= r.x1 / kTile; ++x) ++(*off)[(size_t)y * tx + x + 1], ++entries;
    if (entries >= ((uint64_t)1 << 31)) return entries;
    for (size_t t = 0; t < ntiles; ++t) (*off)[t + 1] += (*off)[t];
    idx->resize((size_t)entries);
    std::vector<unsigned int> cur(off->begin(), off->end() - 1);
    for (size_t s = 0; s < recs.size(); ++s)
        for (int y = recs[s].y0 / kTile; y <= recs[s].y1 / kTile; ++y)
            for (int x = recs[s].x0 / kTile; x <= recs[s].x1 / kTile; ++x) (*idx)[cur[(size_t)y * tx + x]++] = (int)s;
    return entries;
}

// ---- device ------------------------------------------------------------------------------------------------------------------------

// bessel_j1 (psf.rs:91-121)
__device__ double synth_j1(double x) {
    const double ax = fabs(x);
    if (ax < 8.0) {
        const double y = x * x;
        const double num = x * (72362614232.0 + y * (-7895059235.0 + y * (242396853.1 + y * (-2972611.439 + y * (15704.4826 + y * (-30.16036606))))));
        const double den = 144725228442.0 + y * (2300535178.0 + y * (18583304.74 + y * (99447.43394 + y * (376.9991397 + y))));
        return num / den;
    }
    const double z = 8.0 / ax;
    const double y = z * z;
    const double xx = ax - 2.356194491;
    const double p = 1.0 + y * (0.183105e-2 + y * (-0.3516396496e-4 + y * (0.2457520174e-5 + y * (-0.240337019e-6))));
    const double q = 0.04687499995 + y * (-0.2002690873e-3 + y * (0.8449199096e-5 + y * (-0.88228987e-6 + y * 0.105787412e-6)));
    const double ans = (0.5641895835 / sqrt(ax)) * (cos(xx) * p - z * sin(xx) * q);
    return x < 0.0 ? -ans : ans;
}

// PsfModel::evaluate (psf.rs:26-29, :52-55, :75-85)
__device__ __forceinline__ double psf_eval(const PsfParams &p, double dx, double dy) {
    const double r2 = dx * dx + dy * dy;
    if (p.kind == AB_SYNTH_PSF_GAUSSIAN) return exp(-r2 * p.p0);
    if (p.kind == AB_SYNTH_PSF_MOFFAT) return pow(1.0 + r2 * p.p0, -p.p1);
    const double r = sqrt(r2);
    if (r < 1e-10) return 1.0;
    const double x = r * p.p0;
    const double v = 2.0 * synth_j1(x) / x;
    return v * v;
}

// pass A: psf_sum of star blockIdx.x over its window.  Lane t sums the window's pixels t, t + 256, ... (raster numbering) in that
// order; the 256 partial sums meet in a fixed tree.
__global__ __launch_bounds__(kBlock) void synth_norm_kernel(const StarRec *recs, PsfParams psf, StarNorm *norms) {
    __shared__ double sh[kBlock];
    const StarRec rec = recs[blockIdx.x];
    const int w = rec.x1 - rec.x0 + 1, h = rec.y1 - rec.y0 + 1;
    const int total = w * h;  // <= (2 * 512 + 2)^2
    double acc = 0.0;
    for (int i = (int)threadIdx.x; i < total; i += kBlock) {
        const int py = rec.y0 + i / w, px = rec.x0 + i % w;
        acc += psf_eval(psf, (double)px - rec.sx, (double)py - rec.sy);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double psf_sum = sh[0];
        StarNorm o;
        o.skip = psf_sum < 1e-20 ? 1 : 0;
        o.norm = o.skip ? 0.0 : rec.flux / psf_sum;
        o.pad = 0;
        norms[blockIdx.x] = o;
    }
}

// pass B: one lane per output pixel; tile_off / tile_idx = CSR lists of the stars whose windows touch the tile, ascending
__global__ __launch_bounds__(kBlock) void synth_render_kernel(const StarRec *recs, const StarNorm *norms, const unsigned int *tile_off, const int *tile_idx,
                                                              PsfParams psf, int rows, int cols, int tiles_x, float *out) {
    const int tile = (int)blockIdx.x, tile_x = tile % tiles_x, tile_y = tile / tiles_x;
    const int px = tile_x * kTile + (int)(threadIdx.x % kTile), py = tile_y * kTile + (int)(threadIdx.x / kTile);
    const bool inside = px < cols && py < rows;
    const unsigned int beg = tile_off[tile], end = tile_off[tile + 1];
    float acc = 0.0f;
    for (unsigned int j = beg; j < end; ++j) {
        const int s = tile_idx[j];
        const StarNorm nm = norms[s];
        if (nm.skip) continue;
        const StarRec rec = recs[s];
        if (inside && px >= rec.x0 && px <= rec.x1 && py >= rec.y0 && py <= rec.y1)
            acc += (float)(psf_eval(psf, (double)px - rec.sx, (double)py - rec.sy) * nm.norm);
    }
    if (inside) out[(int64_t)py * cols + px] = acc;
}

// generate_flat_field: lane b computes block b of the stream = the draws of pixels 8 b .. 8 b + 7
__global__ __launch_bounds__(kBlock) void synth_flat_kernel(int64_t rows, int64_t cols, ab_chacha_key key, double vs, float *out) {
    const int64_t n = rows * cols;
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t first = 8 * b;
    if (first >= n) return;
    uint32_t w[16];
    ab_chacha_block<12>(key, (uint64_t)b, w);
    const double cx = (double)cols * 0.5, cy = (double)rows * 0.5;
    const double max_r = sqrt(cx * cx + cy * cy);
    int64_t y = first / cols, x = first - y * cols;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (first + j < n) {
            const double dx = (double)x - cx, dy = (double)y - cy;
            const double r = sqrt(dx * dx + dy * dy) / max_r;
            out[first + j] = (float)fmax((1.0 - vs * r * r) * (1.0 + ab_chacha_f64(w, j) * 0.02 - 0.01), 0.01);
            if (++x == cols) x = 0, ++y;
        }
    }
}

__global__ __launch_bounds__(kBlock) void synth_apply_flat_kernel(float *img, const float *flat, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float f = flat[i];
    if (f > 1e-6f) img[i] = img[i] / f;
}

// apply_noise, fast route: lane b computes block b of the stream = the four draws each of pixels 2 b and 2 b + 1 (raster order, across
// row ends).  *flag is raised when a pixel's draw count is not four (lambda below 30) or its lambda is not finite; what the lanes
// wrote is then discarded by the host.
__global__ __launch_bounds__(kBlock) void synth_noise_kernel(const float *img, int64_t n, ab_chacha_key key, NoiseP p, float *out, unsigned int *flag) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t first = 2 * b;
    if (first >= n) return;
    uint32_t w[16];
    ab_chacha_block<12>(key, (uint64_t)b, w);
    bool general = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t i = first + h;
        if (i < n) {
            const double flux = (double)img[i];
            const double signal_e = (flux + p.sky) * p.gain * p.exposure + p.dark * p.exposure;
            const double lambda = fmax(signal_e, 0.0);
            if (!(lambda >= 30.0 && lambda < INFINITY)) general = true;
            double u1 = fmax(ab_chacha_f64(w, 4 * h), 1e-30), u2 = ab_chacha_f64(w, 4 * h + 1);
            const double unit = 0.0 + 1.0 * sqrt(-2.0 * log(u1)) * cos(kTwoPi * u2);
            const double photon = photon_count(lambda + sqrt(lambda) * unit);
            u1 = fmax(ab_chacha_f64(w, 4 * h + 2), 1e-30), u2 = ab_chacha_f64(w, 4 * h + 3);
            const double read_e = 0.0 + p.readout * sqrt(-2.0 * log(u1)) * cos(kTwoPi * u2);
            out[i] = (float)fmax((photon + read_e + p.bias) / p.gain, 0.0);
        }
    }
    if (general) *flag = 1u;
}

// ---- host drivers ------------------------------------------------------------------------------------------------------------------

static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int launch_flat(ab_ctx *ctx, int64_t rows, int64_t cols, uint64_t seed, double vs, float *out_dev) {
    AB_CHECK(ctx, rows * cols < (int64_t(1) << 32), "image too large for this build");
    const int64_t blocks = (rows * cols + 7) / 8;
    hipLaunchKernelGGL(synth_flat_kernel, dim3((unsigned int)ab_div_up(blocks, kBlock)), dim3(kBlock), 0, ctx->stream, rows, cols, ab_chacha_key_from_u64(seed), vs,
                       out_dev);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

int launch_apply_flat(ab_ctx *ctx, float *img_dev, const float *flat_dev, int64_t n) {
    AB_CHECK(ctx, n < (int64_t(1) << 32), "image too large for this build");
    hipLaunchKernelGGL(synth_apply_flat_kernel, dim3((unsigned int)ab_div_up(n, kBlock)), dim3(kBlock), 0, ctx->stream, img_dev, flat_dev, n);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

int launch_noise(ab_ctx *ctx, const float *img_dev, int64_t n, uint64_t seed, const NoiseP &p, float *out_dev, unsigned int *flag_dev) {
    AB_CHECK(ctx, n < (int64_t(1) << 32), "image too large for this build");
    const int64_t blocks = (n + 1) / 2;
    hipLaunchKernelGGL(synth_noise_kernel, dim3((unsigned int)ab_div_up(blocks, kBlock)), dim3(kBlock), 0, ctx->stream, img_dev, n, ab_chacha_key_from_u64(seed), p,
                       out_dev, flag_dev);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// render_stars into out_dev (rows x cols, every pixel written); stars are host data
int render_device(ab_ctx *ctx, const ab_synth_star *stars, size_t n, const ab_synth_psf_type &psf_type, int64_t rows, int64_t cols, float *out_dev) {
    PsfParams psf;
    int64_t psf_r = 0;
    AB_TRY(make_psf(ctx, psf_type, &psf, &psf_r));
    AB_CHECK(ctx, rows < (int64_t(1) << 30) && cols < (int64_t(1) << 30), "image too large for this build");
    for (size_t i = 0; i < n; ++i)
        AB_CHECK(ctx, std::isfinite(stars[i].x) && std::isfinite(stars[i].y) && std::isfinite(stars[i].flux), "star %zu has a non-finite x, y or flux", i);
    const std::vector<StarRec> recs = clamp_stars(stars, n, psf_r, rows, cols);
    const int tx = ab_div_up(cols, kTile), ty = ab_div_up(rows, kTile);
    const size_t ntiles = (size_t)tx * (size_t)ty;
    AB_CHECK(ctx, recs.size() < ((size_t)1 << 31), "too many stars");
    AB_CHECK(ctx, ntiles < ((size_t)1 << 24), "image too large for this build");  // (a launch holds fewer than 2^32 lanes)
    std::vector<unsigned int> off;
    std::vector<int> idx;
    const uint64_t entries = bin_stars(recs, tx, ty, &off, &idx);
    if (entries >= ((uint64_t)1 << 31)) return ab_set_error(ctx, AB_ERR_UNSUPPORTED, "the stars' windows cover %llu tiles in all: more than 2^31", (unsigned long long)entries);
    const size_t nrec = recs.size();
    const size_t off_norm = align256(std::max<size_t>(nrec, 1) * sizeof(StarRec)), off_off = off_norm + align256(std::max<size_t>(nrec, 1) * sizeof(StarNorm)),
                 off_idx = off_off + align256((ntiles + 1) * sizeof(unsigned int)), bytes = off_idx + align256(std::max<size_t>(idx.size(), 1) * sizeof(int));
    char *ws = nullptr;
    AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SYNTH, bytes, (void **)&ws));
    StarRec *recs_dev = (StarRec *)ws;
    StarNorm *norms_dev = (StarNorm *)(ws + off_norm);
    unsigned int *off_dev = (unsigned int *)(ws + off_off);
    int *idx_dev = (int *)(ws + off_idx);
    if (nrec) AB_HIP(ctx, hipMemcpyAsync(recs_dev, recs.data(), nrec * sizeof(StarRec), hipMemcpyHostToDevice, ctx->stream));
    AB_HIP(ctx, hipMemcpyAsync(off_dev, off.data(), (ntiles + 1) * sizeof(unsigned int), hipMemcpyHostToDevice, ctx->stream));
    if (!idx.empty()) AB_HIP(ctx, hipMemcpyAsync(idx_dev, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the tables are pageable host vectors that end with this function)
    if (nrec) hipLaunchKernelGGL(synth_norm_kernel, dim3((unsigned int)nrec), dim3(kBlock), 0, ctx->stream, (const StarRec *)recs_dev, psf, norms_dev);
    hipLaunchKernelGGL(synth_render_kernel, dim3((unsigned int)ntiles), dim3(kBlock), 0, ctx->stream, (const StarRec *)recs_dev, (const StarNorm *)norms_dev,
                       (const unsigned int *)off_dev, (const int *)idx_dev, psf, (int)rows, (int)cols, tx, out_dev);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// a frame's bytes to its plane, host or device (synchronous)
int store_plane(ab_ctx *ctx, const ab_plane_mut *p, const float *src_host, size_t bytes) {
    if (!p->on_device) {
        memcpy(p->data, src_host, bytes);
        return AB_OK;
    }
    AB_HIP(ctx, hipMemcpyAsync(p->data, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AB_OK;
}

// generate / generate_stack: n planes in frames_out; `stack` selects the per-frame seeds of generate_stack
int generate_impl(ab_ctx *ctx, const ab_synth_config &cfg, ab_plane_mut *frames_out, size_t n, bool stack, ab_plane_mut *truth_out, ab_synth_star *stars_out,
                  size_t cap, ab_synth_result *res) {
    const int64_t rows = (int64_t)cfg.field.height, cols = (int64_t)cfg.field.width;
    AB_CHECK(ctx, rows > 0 && cols > 0, "width and height must be at least 1");
    for (size_t i = 0; i < n; ++i)
        AB_CHECK(ctx, frames_out[i].data && frames_out[i].rows == rows && frames_out[i].cols == cols, "output plane %zu must be %lld x %lld (height x width)", i,
                 (long long)rows, (long long)cols);
    if (truth_out) AB_CHECK(ctx, truth_out->data && truth_out->rows == rows && truth_out->cols == cols, "the truth plane must be %lld x %lld", (long long)rows, (long long)cols);
    std::vector<ab_synth_star> stars;
    const char *why = "";
    if (star_field(cfg, &stars, &why) != AB_OK) return ab_set_error(ctx, AB_ERR_INVALID, "%s", why);
    for (size_t i = 0; i < std::min(stars.size(), cap); ++i) stars_out[i] = stars[i];
    if (res) res->star_count = stars.size(), res->frames_on_host = 0;
    AB_TRY(ab_cancel_point(ctx));
    AB_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t npx = rows * cols;
    const size_t bytes = (size_t)npx * sizeof(float);
    // ground truth: rendered once, straight into the caller's plane when that is on the device
    float *truth_dev = nullptr;
    if (truth_out && truth_out->on_device)
        truth_dev = truth_out->data;
    else
        AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SCOPE0, bytes, (void **)&truth_dev));
    AB_TRY(render_device(ctx, stars.data(), stars.size(), cfg.psf_type, rows, cols, truth_dev));
    if (truth_out && !truth_out->on_device) {
        AB_HIP(ctx, hipMemcpyAsync(truth_out->data, truth_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    float *img_dev = nullptr, *flat_dev = nullptr;
    if (cfg.apply_vignette) {
        AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SCOPE1, bytes, (void **)&img_dev));
        AB_TRY(ab_workspace_or_nomem(ctx, AB_WS_SCOPE2, bytes, (void **)&flat_dev));
    }
    unsigned int *flags_dev = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_SCOPE3, n * sizeof(unsigned int), (void **)&flags_dev));
    AB_HIP(ctx, hipMemsetAsync(flags_dev, 0, n * sizeof(unsigned int), ctx->stream));
    const NoiseP np = noise_p(cfg.noise);
    const uint64_t seed = cfg.noise.seed;
    auto flat_seed = [&](size_t i) { return seed + 999ull + (stack ? (uint64_t)i : 0ull); };       // wrapping
    auto noise_seed = [&](size_t i) { return seed + (stack ? (uint64_t)i * 7919ull : 0ull); };  // wrapping
    for (size_t i = 0; i < n; ++i) {
        const float *src = truth_dev;
        if (cfg.apply_vignette) {
            AB_TRY(launch_flat(ctx, rows, cols, flat_seed(i), cfg.vignette_strength, flat_dev));
            AB_HIP(ctx, hipMemcpyAsync(img_dev, truth_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
            AB_TRY(launch_apply_flat(ctx, img_dev, flat_dev, npx));
            src = img_dev;
        }
        Scope frame(ctx);  // (stages only: an inner scope's alloc() would start at slot 0 again)
        float *o = nullptr;
        AB_TRY(frame.stage_out(&frames_out[i], &o));
        AB_TRY(launch_noise(ctx, src, npx, noise_seed(i), np, o, flags_dev + i));
        AB_TRY(frame.finish_outs());
        AB_TRY(ab_progress(ctx, "synth", (uint64_t)i + 1, (uint64_t)n));
    }
    // the frames' routes, read once
    std::vector<unsigned int> flags(n);
    AB_HIP(ctx, hipMemcpyAsync(flags.data(), flags_dev, n * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> truth, img, flat, out;
    size_t on_host = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!flags[i]) continue;
        if (truth.empty()) {
            truth.resize((size_t)npx);
            out.resize((size_t)npx);
            AB_HIP(ctx, hipMemcpyAsync(truth.data(), truth_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
            AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        const float *src = truth.data();
        if (cfg.apply_vignette) {
            img = truth;
            flat.resize((size_t)npx);
            host_flat_field(rows, cols, flat_seed(i), cfg.vignette_strength, flat.data());
            host_apply_flat(img.data(), flat.data(), npx);
            src = img.data();
        }
        host_apply_noise(src, npx, noise_seed(i), np, out.data());
        AB_TRY(store_plane(ctx, &frames_out[i], out.data(), bytes));
        ++on_host;
    }
    if (res) res->frames_on_host = on_host;
    return AB_OK;
}

}  // namespace

extern "C" {

void ab_synth_config_default(ab_synth_config *cfg) {
    if (!cfg) return;
    *cfg = ab_synth_config{};
    cfg->field.width = 2048;
    cfg->field.height = 2048;
    cfg->field.n_stars = 500;
    cfg->field.flux_min = 100.0;
    cfg->field.flux_max = 50000.0;
    cfg->field.seed = 42;
    cfg->field_type.kind = AB_SYNTH_FIELD_UNIFORM;
    cfg->psf_type.kind = AB_SYNTH_PSF_GAUSSIAN;
    cfg->psf_type.fwhm = 3.0;
    cfg->noise.gain = 1.5;
    cfg->noise.readout_noise = 8.0;
    cfg->noise.sky_background = 200.0;
    cfg->noise.dark_current = 0.05;
    cfg->noise.exposure_time = 300.0;
    cfg->noise.bias_level = 1000.0;
    cfg->noise.seed = 123;
    cfg->apply_vignette = 0;
    cfg->vignette_strength = 0.3;
    cfg->n_frames = 1;
}

int ab_synth_rng_f64(uint64_t seed, uint64_t skip, size_t n, double *out) try {
    if (!out && n > 0) return AB_ERR_INVALID;
    ab_chacha_stream rng(seed, skip);
    for (size_t i = 0; i < n; ++i) out[i] = rng.draw();
    return AB_OK;
} AB_CATCH_NOCTX

int ab_synth_chacha_block(const uint32_t *key, uint64_t counter, int rounds, uint32_t *out16) try {
    if (!key || !out16 || (rounds != 12 && rounds != 20)) return AB_ERR_INVALID;
    ab_chacha_key k;
    for (int i = 0; i < 8; ++i) k.k[i] = key[i];
    if (rounds == 12)
        ab_chacha_block<12>(k, counter, out16);
    else
        ab_chacha_block<20>(k, counter, out16);
    return AB_OK;
} AB_CATCH_NOCTX

int ab_synth_star_field(const ab_synth_config *cfg, ab_synth_star *stars_out, size_t cap, size_t *n_out) try {
    if (!cfg || (!stars_out && cap > 0)) return AB_ERR_INVALID;
    std::vector<ab_synth_star> stars;
    const char *why = "";
    const int rc = star_field(*cfg, &stars, &why);
    if (rc != AB_OK) return rc;
    for (size_t i = 0; i < std::min(stars.size(), cap); ++i) stars_out[i] = stars[i];
    if (n_out) *n_out = stars.size();
    return AB_OK;
} AB_CATCH_NOCTX

int ab_synth_render_stars(ab_ctx *ctx, const ab_synth_star *stars, size_t n, const ab_synth_psf_type *psf, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, psf && out && (stars || n == 0), "null argument");
    AB_CHECK(ctx, out->data && out->rows > 0 && out->cols > 0, "the output plane is empty");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    float *o = nullptr;
    AB_TRY(sc.stage_out(out, &o));
    AB_TRY(render_device(ctx, stars, n, *psf, out->rows, out->cols, o));
    return sc.finish_outs();
} AB_CATCH(ctx)

int ab_synth_flat_field(ab_ctx *ctx, uint64_t seed, double vignette_strength, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, out, "null argument");
    AB_CHECK(ctx, out->data && out->rows > 0 && out->cols > 0, "the output plane is empty");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    float *o = nullptr;
    AB_TRY(sc.stage_out(out, &o));
    AB_TRY(launch_flat(ctx, out->rows, out->cols, seed, vignette_strength, o));
    return sc.finish_outs();
} AB_CATCH(ctx)

int ab_synth_apply_flat_field(ab_ctx *ctx, ab_plane_mut *img_inout, const ab_plane *flat) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, img_inout && flat, "null argument");
    AB_CHECK(ctx, img_inout->data && flat->data && img_inout->rows > 0 && img_inout->cols > 0, "the image is empty");
    AB_CHECK(ctx, img_inout->rows == flat->rows && img_inout->cols == flat->cols, "the image and the flat must have equal dims");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    const ab_plane view{img_inout->data, img_inout->rows, img_inout->cols, img_inout->on_device};
    Scope sc(ctx);
    const float *img = nullptr, *fl = nullptr;
    AB_TRY(sc.stage_in(&view, &img));
    AB_TRY(sc.stage_in(flat, &fl));
    const int64_t n = view.rows * view.cols;
    float *img_dev = const_cast<float *>(img);  // (the caller's own mutable plane, or the staged copy of it)
    AB_TRY(launch_apply_flat(ctx, img_dev, fl, n));
    if (!view.on_device) {
        hipError_t e = hipMemcpyAsync(img_inout->data, img_dev, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "D2H copy failed: %s", hipGetErrorString(e));
    }
    return AB_OK;
} AB_CATCH(ctx)

int ab_synth_apply_noise(ab_ctx *ctx, const ab_plane *img, const ab_synth_noise_params *params, ab_plane_mut *out, ab_synth_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, img && params && out, "null argument");
    AB_CHECK(ctx, img->data && out->data && img->rows > 0 && img->cols > 0, "the image is empty");
    AB_CHECK(ctx, img->rows == out->rows && img->cols == out->cols, "img and out must have equal dims");
    if (res) *res = ab_synth_result{};
    AB_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = img->rows * img->cols;
    const size_t bytes = (size_t)n * sizeof(float);
    const NoiseP np = noise_p(*params);
    unsigned int *flag_dev = nullptr;
    AB_TRY(ab_workspace(ctx, AB_WS_SCOPE3, sizeof(unsigned int), (void **)&flag_dev));
    AB_HIP(ctx, hipMemsetAsync(flag_dev, 0, sizeof(unsigned int), ctx->stream));
    Scope sc(ctx);
    const float *in = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(img, &in));
    AB_TRY(sc.stage_out(out, &o));
    AB_TRY(launch_noise(ctx, in, n, params->seed, np, o, flag_dev));
    AB_TRY(sc.finish_outs());
    unsigned int flag = 0;
    hipError_t e = hipMemcpyAsync(&flag, flag_dev, sizeof flag, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "reading the route flag failed: %s", hipGetErrorString(e));
    if (!flag) return AB_OK;
    // the general route: the reference's serial walk on the host
    std::vector<float> host_in, host_out((size_t)n);
    const float *src = img->data;
    if (img->on_device) {
        host_in.resize((size_t)n);
        e = hipMemcpyAsync(host_in.data(), in, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "D2H copy failed: %s", hipGetErrorString(e));
        src = host_in.data();
    }
    host_apply_noise(src, n, params->seed, np, host_out.data());
    AB_TRY(store_plane(ctx, out, host_out.data(), bytes));
    if (res) res->frames_on_host = 1;
    return AB_OK;
} AB_CATCH(ctx)

int ab_synth_generate(ab_ctx *ctx, const ab_synth_config *cfg, ab_plane_mut *noisy_out, ab_plane_mut *truth_out, ab_synth_star *stars_out, size_t cap,
                      ab_synth_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, cfg && noisy_out && (stars_out || cap == 0), "null argument");
    if (res) *res = ab_synth_result{};
    return generate_impl(ctx, *cfg, noisy_out, 1, false, truth_out, stars_out, cap, res);
} AB_CATCH(ctx)

int ab_synth_generate_stack(ab_ctx *ctx, const ab_synth_config *cfg, ab_plane_mut *frames_out, ab_plane_mut *truth_out, ab_synth_star *stars_out, size_t cap,
                            ab_synth_result *res) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, cfg && frames_out && (stars_out || cap == 0), "null argument");
    AB_CHECK(ctx, cfg->n_frames > 0, "n_frames must be at least 1");
    if (res) *res = ab_synth_result{};
    return generate_impl(ctx, *cfg, frames_out, (size_t)cfg->n_frames, true, truth_out, stars_out, cap, res);
} AB_CATCH(ctx)

}  // extern "C"
