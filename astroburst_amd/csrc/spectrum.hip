// The FFT power spectrum on gfx950: a forward complex f32 2-D FFT built from one batched line kernel.
//
// Replaces core/analysis/fft.rs (compute_power_spectrum_opts :23-68, downsample_area_average :70-97), math/fft.rs
// (FftEngine2D::<f32>::forward_2d :137-148, prepare_windowed_buffer / prepare_buffer_no_window :202-245), math/window.rs
// (hann_symmetric :20-35) and the per-pixel part of compute_fft_spectrum (cmd/analysis/mod.rs:66-96).
//
// One 2-D transform is, on the context's stream (A, B: two fft_rows x fft_cols complex workspaces):
//   fft_lines_kernel<image>   one launch over the image's rows only: the finite filter, the window multiply (v * wy) * wx and the
//                             zero padding happen in the loads, the row's FFT runs in LDS, the result goes to A.  Rows of pure
//                             padding are neither transformed nor written
//   fft_transpose_kernel      A -> B (32 x 32 tiles through LDS); rows of A beyond the image are read as zero, not from memory
//   fft_lines_kernel          the fft_cols lines of B, each fft_rows long, in place
// then either
//   fft_transpose_kernel      B -> natural row-major order (ab_fft2_forward_f32), or
//   spectrum_log_kernel       fftshift, sqrtf(re^2 + im^2), logf(1 + mag) and the s x s block mean straight from the transposed B
//                             (ab_compute_power_spectrum): the size^2 log plane is never written
//
// The line kernel: a workgroup holds kTile points in LDS (split re / im planes, XOR-swizzled banks) -- one line of 4096, 8192 or
// 16384 points, or 2048 / n lines of n <= 2048 points -- and runs an in-place decimation-in-frequency radix-2 FFT on them, three
// butterfly layers per LDS round trip (eight points per lane in registers; a 16384-point line takes five rounds).  The output of
// an in-place DIF is bit-reversed: the store reads LDS at brev(k).  Every twiddle is W_n^p = exp(-2 pi i p / n) evaluated in f64
// and rounded once to f32, from a table per line length cached in the context; no sincosf in a kernel.
// No atomics anywhere: two calls are bit-identical.
#include "entry_host.hpp"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kMaxLog = 14;             // lines of up to 16384 points
constexpr int kMaxLine = 1 << kMaxLog;
constexpr int kSmallTile = 2048;        // lines of up to 2048 points share a workgroup: 2048 / n of them
constexpr int kTwiddleCount = kMaxLine; // the tables of n = 2, 4 .. 16384 hold n / 2 entries each, n's at [n / 2 - 1, n - 1)
constexpr int kMaxDisplay = 1024;       // MAX_DISPLAY_SIZE (fft.rs:9)

// LDS index of tile point q: the three 5-bit fields of q XORed into the bank, so that 32 lanes whose addresses differ in ANY five
// consecutive bits (the contiguous loads, a butterfly round of any stride, the bit-reversed store) hit 32 banks
__device__ __forceinline__ int sw(int q) { return q ^ ((q >> 5) & 31) ^ ((q >> 10) & 31); }

struct LineArgs {
    // image mode: line r is row r of the image, zero-padded to n
    const float *img;
    int img_cols;
    const float *wy, *wx;  // both null: no window
    // complex mode: line r is src[r * n .. + n)
    const float2 *src;
    float2 *dst;        // line r goes to dst[r * n .. + n) (may be src)
    const float2 *tw;   // W_n^p, p < n / 2
    int n, logn;
    int lines;
};

// kLayers butterfly layers of the blocks of length m (= n >> done) on the eight / four / two points base + t * s, s = m >> kLayers
template <int kLayers>
__device__ __forceinline__ void fft_round(float *__restrict__ sre, float *__restrict__ sim, const float2 *__restrict__ tw, int base, int j, int s,
                                          int done) {
    constexpr int kP = 1 << kLayers;
    float xr[kP], xi[kP];
#pragma unroll
    for (int t = 0; t < kP; ++t) {
        const int q = sw(base + t * s);
        xr[t] = sre[q];
        xi[t] = sim[q];
    }
#pragma unroll
    for (int l = 0; l < kLayers; ++l) {
        constexpr int kTop = kLayers - 1;
        const int half = 1 << (kTop - l);
#pragma unroll
        for (int t = 0; t < kP; ++t) {
            if (t & half) continue;
            // position p of point t in its block of length m >> l; the twiddle W_{m >> l}^p = W_n^{p << (done + l)}
            const int p = j + (t & (half - 1)) * s;
            const float2 w = tw[p << (done + l)];
            const float ar = xr[t], ai = xi[t], br = xr[t + half], bi = xi[t + half];
            xr[t] = ar + br;
            xi[t] = ai + bi;
            const float dr = ar - br, di = ai - bi;
            xr[t + half] = dr * w.x - di * w.y;
            xi[t + half] = dr * w.y + di * w.x;
        }
    }
#pragma unroll
    for (int t = 0; t < kP; ++t) {
        const int q = sw(base + t * s);
        sre[q] = xr[t];
        sim[q] = xi[t];
    }
}

template <int kTile, int kThreads, bool kImage>
__global__ __launch_bounds__(kThreads) void fft_lines_kernel(const LineArgs a) {
    __shared__ float sre[kTile], sim[kTile];
    const int n = a.n, logn = a.logn;
    const int tid = threadIdx.x;
    const int64_t line0 = (int64_t)blockIdx.x * (kTile >> logn);
    for (int q = tid; q < kTile; q += kThreads) {
        const int k = q & (n - 1);
        const int64_t line = line0 + (q >> logn);
        float re = 0.0f, im = 0.0f;
        if (line < a.lines) {
            if (kImage) {
                if (k < a.img_cols) {
                    const float v = a.img[line * a.img_cols + k];
                    if (__builtin_isfinite(v)) re = a.wy ? (v * a.wy[line]) * a.wx[k] : v;  // (fft.rs:216-222, :239-241)
                }
            } else {
                const float2 c = a.src[line * n + k];
                re = c.x, im = c.y;
            }
        }
        const int p = sw(q);
        sre[p] = re;
        sim[p] = im;
    }
    __syncthreads();
    for (int done = 0; done < logn;) {
        const int layers = min(3, logn - done);
        const int logs = logn - done - layers;  // s = 2^logs: the distance between a lane's points
        const int s = 1 << logs;
        for (int i = tid; i < (kTile >> layers); i += kThreads) {
            const int g = i & ((n >> layers) - 1);  // the lane's group inside its line
            const int j = g & (s - 1);
            const int base = ((i >> (logn - layers)) << logn) + ((g >> logs) << (logs + layers)) + j;
            if (layers == 3) fft_round<3>(sre, sim, a.tw, base, j, s, done);
            else if (layers == 2) fft_round<2>(sre, sim, a.tw, base, j, s, done);
            else fft_round<1>(sre, sim, a.tw, base, j, s, done);
        }
        done += layers;
        __syncthreads();
    }
    for (int q = tid; q < kTile; q += kThreads) {
        const int k = q & (n - 1);
        const int64_t line = line0 + (q >> logn);
        if (line >= a.lines) continue;
        const int rev = logn ? (int)(__brev((unsigned)k) >> (32 - logn)) : 0;
        const int p = sw(((q >> logn) << logn) + rev);
        a.dst[line * n + k] = make_float2(sre[p], sim[p]);
    }
}

// dst[c][r] = src[r][c] of a rows x cols complex plane; rows >= valid_rows of src are zero and are not read
__global__ __launch_bounds__(256) void fft_transpose_kernel(const float2 *__restrict__ src, float2 *__restrict__ dst, int rows, int cols,
                                                            int valid_rows) {
    __shared__ float2 tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x = blockIdx.x * 32 + tx;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int y = blockIdx.y * 32 + ty + k;
        float2 v = make_float2(0.0f, 0.0f);
        if (x < cols && y < valid_rows) v = src[(int64_t)y * cols + x];
        tile[ty + k][tx] = v;
    }
    __syncthreads();
    const int x2 = blockIdx.y * 32 + tx;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int y2 = blockIdx.x * 32 + ty + k;
        if (x2 < rows && y2 < cols) dst[(int64_t)y2 * rows + x2] = tile[tx][ty + k];
    }
}

// fft.rs:39-57 from the TRANSPOSED spectrum ft (F[r][c] = ft[c * size + r]): out[dy][dx] = the mean over the s x s block of
// ln(1 + |F[(y + half) % size][(x + half) % size]|).  half is a multiple of s, so a block is an aligned s x s block of F too.  Lanes
// run along y (contiguous in ft); a 32 x 32 tile of results turns through LDS so that the store runs along x.  The block is summed
// column by column, then the s column sums: all f32
__global__ __launch_bounds__(256) void spectrum_log_kernel(const float2 *__restrict__ ft, int size, int s, float *__restrict__ out, int disp) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int half = size / 2;
    const int dy = blockIdx.y * 32 + tx;
    const float inv = 1.0f / (float)(s * s);  // (a power of two: the division of :92 is exact either way)
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int dx = blockIdx.x * 32 + ty + k;
        float total = 0.0f;
        if (dy < disp && dx < disp) {
            const int r0 = (dy * s + half) & (size - 1), c0 = (dx * s + half) & (size - 1);
            for (int xx = 0; xx < s; ++xx) {
                const float2 *col = ft + (int64_t)(c0 + xx) * size + r0;
                float cs = 0.0f;
                for (int yy = 0; yy < s; ++yy) {
                    const float2 c = col[yy];
                    const float mag = sqrtf(c.x * c.x + c.y * c.y);  // complex::norm (math/complex.rs:7-9)
                    cs = cs + logf(1.0f + mag);
                }
                total = total + cs;
            }
        }
        tile[ty + k][tx] = s == 1 ? total : total * inv;
    }
    __syncthreads();
    const int ox = blockIdx.x * 32 + tx;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int oy = blockIdx.y * 32 + ty + k;
        if (oy < disp && ox < disp) out[(int64_t)oy * disp + ox] = tile[tx][ty + k];
    }
}

// ---- compute_fft_spectrum's per-pixel part ----
constexpr int kRedBlock = 256;
constexpr int kRedBlocks = 1024;

__device__ __forceinline__ void tree_minmax(float &mn, float &mx) {
    __shared__ float smn[kRedBlock], smx[kRedBlock];
    smn[threadIdx.x] = mn;
    smx[threadIdx.x] = mx;
    __syncthreads();
    for (int d = kRedBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + d]);  // f32::min / f32::max: a NaN operand is skipped
            smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + d]);
        }
        __syncthreads();
    }
    mn = smn[0];
    mx = smx[0];
}

// partial[2 b], [2 b + 1] = min, max of block b's share
__global__ __launch_bounds__(kRedBlock) void u8_minmax_kernel(const float *__restrict__ v, int64_t n, float *__restrict__ partial) {
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kRedBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRedBlock) {
        mn = fminf(mn, v[i]);
        mx = fmaxf(mx, v[i]);
    }
    tree_minmax(mn, mx);
    if (threadIdx.x == 0) partial[2 * blockIdx.x] = mn, partial[2 * blockIdx.x + 1] = mx;
}

// result = {min, max, v[dc_at]}
__global__ __launch_bounds__(kRedBlock) void u8_minmax_final_kernel(const float *__restrict__ partial, int blocks, const float *__restrict__ v,
                                                                    int64_t dc_at, float *__restrict__ result) {
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < blocks; i += kRedBlock) {
        mn = fminf(mn, partial[2 * i]);
        mx = fmaxf(mx, partial[2 * i + 1]);
    }
    tree_minmax(mn, mx);
    if (threadIdx.x == 0) result[0] = mn, result[1] = mx, result[2] = v[dc_at];
}

// ((v - min) * inv) as u8 (mod.rs:93-95): truncating, saturating, NaN -> 0
__global__ __launch_bounds__(kRedBlock) void u8_scale_kernel(const float *__restrict__ v, int64_t n, float mn, float inv, uint8_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kRedBlock + threadIdx.x;
    if (i >= n) return;
    const float x = (v[i] - mn) * inv;
    out[i] = x != x ? 0 : (x <= 0.0f ? 0 : (x >= 255.0f ? 255 : (uint8_t)x));
}

// ---- host ----
bool is_pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }
int log2_of(int64_t v) {
    int l = 0;
    while ((int64_t(1) << l) < v) ++l;
    return l;
}

// ab_workspace, with exhaustion reported as AB_ERR_NOMEM (a 16384^2 transform asks for two 2 GiB planes)
int fft_workspace(ab_ctx *ctx, int slot, size_t bytes, void **out) {
    if (bytes > ctx->ws_bytes[slot]) {
        void *p = nullptr;
        if (ctx->ws[slot]) {
            AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
            p = ctx->ws[slot];
            ctx->ws[slot] = nullptr;
            ctx->ws_bytes[slot] = 0;
            AB_HIP(ctx, hipFree(p));
        }
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return ab_set_error(ctx, AB_ERR_NOMEM, "cannot allocate %zu bytes of device memory for the FFT workspace", bytes);
        }
        AB_HIP(ctx, e);
        ctx->ws[slot] = p;
        ctx->ws_bytes[slot] = bytes;
    }
    *out = ctx->ws[slot];
    return AB_OK;
}

struct FftTables {
    const float2 *tw;  // kTwiddleCount entries
    float *wy, *wx;    // kMaxLine floats each
};

// the twiddle tables of every line length, built once per workspace: exp(-2 pi i p / n) in f64, rounded once to f32
int fft_tables(ab_ctx *ctx, FftTables *t) {
    const size_t tw_bytes = (size_t)kTwiddleCount * sizeof(float2), win_bytes = (size_t)kMaxLine * sizeof(float);
    char *ws = nullptr;
    AB_TRY(fft_workspace(ctx, AB_WS_FFT_TABLES, tw_bytes + 2 * win_bytes, (void **)&ws));
    if (ctx->fft_tab_ws != ws) {
        std::vector<float2> host((size_t)kTwiddleCount, make_float2(0.0f, 0.0f));
        for (int logn = 1; logn <= kMaxLog; ++logn) {
            const int n = 1 << logn;
            float2 *tab = host.data() + (n / 2 - 1);
            for (int p = 0; p < n / 2; ++p) {
                const double ang = -2.0 * M_PI * (double)p / (double)n;
                tab[p] = make_float2((float)std::cos(ang), (float)std::sin(ang));
            }
        }
        AB_HIP(ctx, hipMemcpyAsync(ws, host.data(), tw_bytes, hipMemcpyHostToDevice, ctx->stream));
        AB_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (`host` dies with this scope)
        ctx->fft_tab_ws = ws;
    }
    t->tw = (const float2 *)ws;
    t->wy = (float *)(ws + tw_bytes);
    t->wx = t->wy + kMaxLine;
    return AB_OK;
}

template <bool kImage>
int launch_lines(ab_ctx *ctx, const LineArgs &a) {
    if (a.lines <= 0) return AB_OK;
    const int n = a.n;
    if (n <= kSmallTile) {
        const int per = kSmallTile / n;
        hipLaunchKernelGGL((fft_lines_kernel<kSmallTile, 256, kImage>), dim3(ab_div_up(a.lines, per)), dim3(256), 0, ctx->stream, a);
    } else if (n == 4096) {
        hipLaunchKernelGGL((fft_lines_kernel<4096, 512, kImage>), dim3(a.lines), dim3(512), 0, ctx->stream, a);
    } else if (n == 8192) {
        hipLaunchKernelGGL((fft_lines_kernel<8192, 1024, kImage>), dim3(a.lines), dim3(1024), 0, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((fft_lines_kernel<16384, 1024, kImage>), dim3(a.lines), dim3(1024), 0, ctx->stream, a);
    }
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

int launch_transpose(ab_ctx *ctx, const float2 *src, float2 *dst, int rows, int cols, int valid_rows) {
    hipLaunchKernelGGL(fft_transpose_kernel, dim3(ab_div_up(cols, 32), ab_div_up(rows, 32)), dim3(32, 8), 0, ctx->stream, src, dst, rows, cols,
                       valid_rows);
    AB_HIP(ctx, hipGetLastError());
    return AB_OK;
}

// prepare_*_buffer + forward_2d of a device image, enqueued on the context's stream.  Leaves the TRANSPOSED spectrum (fft_cols lines
// of fft_rows points) in *bt and the other workspace plane, free to reuse, in *spare.  win_y / win_x: host tables or both null
int fft2_device(ab_ctx *ctx, const float *img, int rows, int cols, const float *win_y, const float *win_x, int fft_rows, int fft_cols, float2 **bt,
                float2 **spare) {
    FftTables tab;
    AB_TRY(fft_tables(ctx, &tab));
    const size_t plane = (size_t)fft_rows * (size_t)fft_cols * sizeof(float2);
    float2 *A = nullptr, *B = nullptr;
    AB_TRY(fft_workspace(ctx, AB_WS_FFT_A, plane, (void **)&A));
    AB_TRY(fft_workspace(ctx, AB_WS_FFT_B, plane, (void **)&B));
    if (win_y) {
        // (pageable host memory: the copies have read their source when they return)
        AB_HIP(ctx, hipMemcpyAsync(tab.wy, win_y, (size_t)rows * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        AB_HIP(ctx, hipMemcpyAsync(tab.wx, win_x, (size_t)cols * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    LineArgs a = {};
    a.img = img;
    a.img_cols = cols;
    a.wy = win_y ? tab.wy : nullptr;
    a.wx = win_y ? tab.wx : nullptr;
    a.dst = A;
    a.n = fft_cols;
    a.logn = log2_of(fft_cols);
    a.tw = tab.tw + (fft_cols / 2 - (fft_cols > 1 ? 1 : 0));
    a.lines = rows;  // the image's rows only: a row of padding transforms to zeros, which the transpose supplies
    AB_TRY(launch_lines<true>(ctx, a));
    AB_TRY(launch_transpose(ctx, A, B, fft_rows, fft_cols, rows));
    LineArgs b = {};
    b.src = B;
    b.dst = B;
    b.n = fft_rows;
    b.logn = log2_of(fft_rows);
    b.tw = tab.tw + (fft_rows / 2 - (fft_rows > 1 ? 1 : 0));
    b.lines = fft_cols;
    AB_TRY(launch_lines<false>(ctx, b));
    *bt = B;
    *spare = A;
    return AB_OK;
}

void hann_symmetric_f32(size_t n, float *out) {
    if (n == 0) return;
    if (n == 1) {
        out[0] = 1.0f;
        return;
    }
    const float two_pi = 2.0f * 3.14159265358979323846f;  // T::two() * T::pi()
    const float denom = std::max((float)(n - 1), 1.0f);
    for (size_t i = 0; i < n; ++i) {
        const float phase = two_pi * (float)i / denom;
        out[i] = 0.5f * (1.0f - cosf(phase));
    }
}

int spectrum_dims(int64_t rows, int64_t cols, int64_t *original, int64_t *display) {
    if (rows < 1 || cols < 1) return AB_ERR_INVALID;
    const int64_t m = std::max(rows, cols);
    if (m > kMaxLine) return AB_ERR_UNSUPPORTED;
    int64_t size = 1;
    while (size < m) size <<= 1;
    if (original) *original = size;
    if (display) *display = std::min<int64_t>(size, kMaxDisplay);
    return AB_OK;
}

}  // namespace

extern "C" {

int ab_power_spectrum_dims(int64_t rows, int64_t cols, int64_t *original_size, int64_t *display_size) try {
    return spectrum_dims(rows, cols, original_size, display_size);
} AB_CATCH_NOCTX

int ab_hann_symmetric_f32(size_t n, float *out) try {
    if (n > 0 && !out) return AB_ERR_INVALID;
    hann_symmetric_f32(n, out);
    return AB_OK;
} AB_CATCH_NOCTX

int ab_fft2_forward_f32(ab_ctx *ctx, const ab_plane *image, const float *win_y, const float *win_x, int64_t fft_rows, int64_t fft_cols, float *out,
                        int32_t out_on_device) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, image && out, "null argument");
    AB_CHECK(ctx, image->data && image->rows > 0 && image->cols > 0, "the image is empty");
    AB_CHECK(ctx, is_pow2(fft_rows) && is_pow2(fft_cols) && fft_rows <= kMaxLine && fft_cols <= kMaxLine,
             "fft_rows and fft_cols must be powers of two in 1 .. 16384 (got %lld x %lld)", (long long)fft_rows, (long long)fft_cols);
    AB_CHECK(ctx, image->rows <= fft_rows && image->cols <= fft_cols, "the image (%lld x %lld) is larger than the FFT buffer (%lld x %lld)",
             (long long)image->rows, (long long)image->cols, (long long)fft_rows, (long long)fft_cols);
    AB_CHECK(ctx, (win_y == nullptr) == (win_x == nullptr), "win_y and win_x must both be given or both be NULL");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    Scope sc(ctx);
    const float *in = nullptr;
    AB_TRY(sc.stage_in(image, &in));
    float2 *bt = nullptr, *spare = nullptr;
    int rc = fft2_device(ctx, in, (int)image->rows, (int)image->cols, win_y, win_x, (int)fft_rows, (int)fft_cols, &bt, &spare);
    if (rc == AB_OK) rc = launch_transpose(ctx, bt, out_on_device ? (float2 *)out : spare, (int)fft_cols, (int)fft_rows, (int)fft_cols);
    if (rc == AB_OK && !out_on_device) {
        const hipError_t e = hipMemcpyAsync(out, spare, (size_t)fft_rows * (size_t)fft_cols * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = ab_set_error(ctx, AB_ERR_HIP, "D2H copy failed: %s", hipGetErrorString(e));
    }
    {
        const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the result is complete, and the caller's windows are read, on return)
        if (e != hipSuccess && rc == AB_OK) rc = ab_set_error(ctx, AB_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    return rc;
} AB_CATCH(ctx)

int ab_compute_power_spectrum(ab_ctx *ctx, const ab_plane *image, int32_t apply_window, ab_plane_mut *spectrum, ab_fft_result *result) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, image && spectrum && result, "null argument");
    AB_CHECK(ctx, image->data && image->rows > 0 && image->cols > 0, "the image is empty");
    int64_t size = 0, disp = 0;
    const int drc = spectrum_dims(image->rows, image->cols, &size, &disp);
    if (drc != AB_OK) return ab_set_error(ctx, drc, "images beyond 16384 pixels a side are not supported (got %lld x %lld)", (long long)image->rows,
                                          (long long)image->cols);
    AB_CHECK(ctx, spectrum->data, "null output plane");
    AB_CHECK(ctx, spectrum->rows == disp && spectrum->cols == disp, "the spectrum plane must be %lld x %lld (got %lld x %lld)", (long long)disp,
             (long long)disp, (long long)spectrum->rows, (long long)spectrum->cols);
    AB_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<float> wy, wx;
    if (apply_window) {  // (fft.rs:29-32)
        wy.resize((size_t)image->rows);
        wx.resize((size_t)image->cols);
        hann_symmetric_f32(wy.size(), wy.data());
        hann_symmetric_f32(wx.size(), wx.data());
    }
    Scope sc(ctx);
    const float *in = nullptr;
    float *o = nullptr;
    AB_TRY(sc.stage_in(image, &in));
    AB_TRY(sc.stage_out(spectrum, &o));
    float2 *bt = nullptr, *spare = nullptr;
    int rc = fft2_device(ctx, in, (int)image->rows, (int)image->cols, apply_window ? wy.data() : nullptr, apply_window ? wx.data() : nullptr, (int)size,
                     (int)size, &bt, &spare);
    if (rc == AB_OK) {
        const int s = (int)(size / disp);
        hipLaunchKernelGGL(spectrum_log_kernel, dim3(ab_div_up(disp, 32), ab_div_up(disp, 32)), dim3(32, 8), 0, ctx->stream, (const float2 *)bt,
                           (int)size, s, o, (int)disp);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = ab_set_error(ctx, AB_ERR_HIP, "spectrum_log_kernel launch failed: %s", hipGetErrorString(e));
    }
    {
        const hipError_t e = hipStreamSynchronize(ctx->stream);  // (the window tables are this call's: read before they go)
        if (e != hipSuccess && rc == AB_OK) rc = ab_set_error(ctx, AB_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    if (rc == AB_OK) rc = sc.finish_outs();
    if (rc == AB_OK) {
        result->display_rows = disp;
        result->display_cols = disp;
        result->original_size = size;
        result->windowed = apply_window ? 1 : 0;
    }
    return rc;
} AB_CATCH(ctx)

int ab_spectrum_to_u8(ab_ctx *ctx, const ab_plane *spectrum, uint8_t *out_u8, int32_t out_on_device, float *min_val, float *max_val, float *dc) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, spectrum && out_u8, "null argument");
    AB_CHECK(ctx, spectrum->data && spectrum->rows > 0 && spectrum->cols > 0, "the spectrum is empty");
    AB_CHECK(ctx, spectrum->rows < (int64_t(1) << 31) && spectrum->cols < (int64_t(1) << 31), "spectrum too large for this build");
    AB_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = spectrum->rows * spectrum->cols;
    const int blocks = (int)std::min<int64_t>(kRedBlocks, (n + kRedBlock - 1) / kRedBlock);
    // the partials, the result triple and (host output) the bytes, in the context's scratch arena
    const size_t head = (size_t)(2 * kRedBlocks + 4) * sizeof(float);
    char *scratch = nullptr;
    AB_TRY(ab_scratch(ctx, head + (out_on_device ? 0 : (size_t)n), (void **)&scratch));
    float *partial = (float *)scratch, *triple = partial + 2 * kRedBlocks;
    uint8_t *bytes_dev = out_on_device ? out_u8 : (uint8_t *)(scratch + head);
    Scope sc(ctx);
    const float *in = nullptr;
    AB_TRY(sc.stage_in(spectrum, &in));
    const int64_t dc_at = (spectrum->rows / 2) * spectrum->cols + spectrum->cols / 2;  // (mod.rs:77)
    hipLaunchKernelGGL(u8_minmax_kernel, dim3(blocks), dim3(kRedBlock), 0, ctx->stream, in, n, partial);
    hipLaunchKernelGGL(u8_minmax_final_kernel, dim3(1), dim3(kRedBlock), 0, ctx->stream, (const float *)partial, blocks, in, dc_at, triple);
    float host[3] = {0.0f, 0.0f, 0.0f};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, triple, sizeof host, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) {
        const float range = std::fmax(host[1] - host[0], 1e-10f);  // (mod.rs:75-76), in f32
        const float inv = 255.0f / range;
        hipLaunchKernelGGL(u8_scale_kernel, dim3((unsigned)((n + kRedBlock - 1) / kRedBlock)), dim3(kRedBlock), 0, ctx->stream, in, n, host[0], inv,
                           bytes_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !out_on_device) e = hipMemcpyAsync(out_u8, bytes_dev, (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return ab_set_error(ctx, AB_ERR_HIP, "ab_spectrum_to_u8 failed: %s", hipGetErrorString(e));
    if (min_val) *min_val = host[0];
    if (max_val) *max_val = host[1];
    if (dc) *dc = host[2];
    return AB_OK;
} AB_CATCH(ctx)

}  // extern "C"
