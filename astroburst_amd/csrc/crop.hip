// The compose wizard's crop step on gfx950: valid-region detection and the channel crop.
//
// Replaces cmd/compose/crop.rs: detect_valid_region (:14-62), crop_array (:64-71) and the pixel work of crop_channels_cmd -- the loop
// over the planes and the intersection (:103-122), the manual margins (:123-126), the per-plane crop and statistics (:133-168) and the
// reported dimensions and margins (:170-183).  Files, the image cache and JSON stay with the host.
//
// Two kernels, both indexed by the FLAT pixel index of a dense plane (the input of the detection, the output of the crop), so one
// peeled head of at most three pixels puts every later group of four on a 16-byte boundary whatever the base address and `cols`:
//
//   bbox_kernel   one streaming pass, 4 B per pixel.  A lane loads one dwordx4, evaluates |v| > threshold on the four values in
//                 registers and folds the hits into its own (first row, last row + 1, first column, last column + 1); a group that
//                 lies inside one row costs a ctz / clz of the 4-bit hit mask, one that wraps walks its pixels.  The lane's (row,
//                 column) advances by a precomputed step, there is one division per lane and launch.  The four bounds are folded
//                 across the wave by shuffles, across the workgroup's sixteen waves through LDS, and the workgroup issues one
//                 atomicMin / atomicMax per bound on the plane's slot of four u32, which an init launch set to (rows, 0, cols, 0).
//                 Integer min / max commute: the result does not depend on arrival order.  A workgroup that found nothing issues
//                 nothing (its bounds are the slot's identities).
//   crop_kernel   the window copy.  The source is read through its own row stride, the output is dense: whole dwordx4 stores at
//                 every group, a dwordx4 load where the group lies in one row and its source address is 16-byte aligned, dword
//                 loads otherwise; the at most six pixels around the groups are moved one per lane.  Values move as u32: NaN
//                 payloads survive.
//
// Both take up to kBatch planes of any dims in ONE launch: the kernel argument holds a table of (pointer, dims, first workgroup) and
// a workgroup finds its plane by its index.  More than kBatch planes are served kBatch at a time.
#include "ab_common.hpp"
#include "entry_host.hpp"

#include <algorithm>
#include <climits>
#include <cmath>

namespace {

// (the copy's workgroup is entry_host.hpp's kBlock, at most 8 per CU)
// The detection's workgroups each end in four atomics on one 16-byte slot, which the L2 serialises (about 5.5 ns each): with 2048
// workgroups of 256 lanes a 4096^2 plane took 55 us, 45 of them that queue.  Sixteen waves per workgroup and two workgroups per CU keep
// the same waves in flight with a quarter of the atomics: 22 us; one per CU loses bandwidth on large planes, four gain nothing there
// and cost 8 us here.
constexpr int kBoxBlock = 1024;
constexpr int kBoxPerCu = 2;
constexpr int kBatch = 16;                  // planes per launch
constexpr int kUnroll = 4;                  // groups a lane of the detection has in flight
constexpr int kWorth = 4;                   // groups per lane below which one more workgroup is not worth having: sizes both kernels' grids

struct BoxEnt {
    const float *src;
    uint32_t rows, cols, n;
    uint32_t head, quads;     // pixels [0, head) precede the groups [head, head + 4 * quads)
    uint32_t wg0, per;        // the plane's first workgroup; groups per workgroup (a multiple of its lanes)
    uint32_t step_r, step_c;  // 4 kBoxBlock / cols, 4 kBoxBlock % cols: what a lane advances by from group to group
};
struct BoxArgs {
    BoxEnt e[kBatch];
    int count;
    float threshold;
    uint32_t *slots;  // 4 u32 per plane: top, bottom, left, right
};

struct CropEnt {
    const uint32_t *src;  // the window's first pixel
    uint32_t *dst;
    uint32_t ld, ocols, n;
    uint32_t head, quads;
    uint32_t wg0, per;
    uint32_t step_r, step_c;  // 4 kBlock / ocols, 4 kBlock % ocols
};
struct CropArgs {
    CropEnt e[kBatch];
    int count;
};

struct Fold {
    uint32_t top, bottom, left, right;
    __device__ __forceinline__ void hit(uint32_t r, uint32_t c_first, uint32_t c_end) {
        top = min(top, r);
        bottom = max(bottom, r + 1u);
        left = min(left, c_first);
        right = max(right, c_end);
    }
};

// detect_valid_region's test (:20): strict, in f32; a NaN pixel or a NaN threshold compares false
__device__ __forceinline__ bool valid_px(float v, float threshold) { return fabsf(v) > threshold; }

// the pixels of one group, (r, c) = its first pixel's place
__device__ __forceinline__ void fold_group(Fold &f, const float4 v, float thr, uint32_t r, uint32_t c, uint32_t cols) {
    const uint32_t m = (valid_px(v.x, thr) ? 1u : 0u) | (valid_px(v.y, thr) ? 2u : 0u) | (valid_px(v.z, thr) ? 4u : 0u) | (valid_px(v.w, thr) ? 8u : 0u);
    if (!m) return;
    if (c + 3u < cols) {  // inside one row
        f.hit(r, c + (uint32_t)__builtin_ctz(m), c + 32u - (uint32_t)__builtin_clz(m));
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (m & (1u << k)) f.hit(r, c, c + 1u);
        if (++c == cols) c = 0u, ++r;
    }
}

template <class Args>
__device__ __forceinline__ int plane_of(const Args &a) {
    int p = 0;
    for (int k = 1; k < a.count; ++k)
        if (blockIdx.x >= a.e[k].wg0) p = k;
    return p;
}

__global__ __launch_bounds__(64) void bbox_init_kernel(const BoxArgs a) {
    const int p = threadIdx.x >> 2, w = threadIdx.x & 3;
    if (p < a.count) a.slots[4 * p + w] = w == 0 ? a.e[p].rows : (w == 2 ? a.e[p].cols : 0u);
}

__global__ __launch_bounds__(kBoxBlock) void bbox_kernel(const BoxArgs a) {
    const int p = plane_of(a);
    const BoxEnt &e = a.e[p];
    const float thr = a.threshold;
    const uint32_t rows = e.rows, cols = e.cols;
    const uint32_t j = blockIdx.x - e.wg0, tid = threadIdx.x;
    Fold f{rows, 0u, cols, 0u};
    const uint32_t begin = j * e.per, end = min(begin + e.per, e.quads);  // (j * per < quads + per: no overflow, n < 2^31)
    if (begin < end) {
        const float4 *src4 = reinterpret_cast<const float4 *>(e.src + e.head);
        const uint32_t i0 = e.head + 4u * (begin + tid);
        uint32_t r = i0 / cols, c = i0 - r * cols;
        for (uint32_t base = begin; base < end; base += kBoxBlock * kUnroll) {
            float4 v[kUnroll];
            bool ok[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const uint32_t q = base + (uint32_t)u * kBoxBlock + tid;
                ok[u] = q < end;
                if (ok[u]) v[u] = src4[q];
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (ok[u]) fold_group(f, v[u], thr, r, c, cols);
                r += e.step_r;
                c += e.step_c;
                if (c >= cols) c -= cols, ++r;
            }
        }
    }
    if (j == 0u) {  // the pixels around the groups
        const uint32_t loose = e.n - 4u * e.quads;
        if (tid < loose) {
            const uint32_t i = tid < e.head ? tid : 4u * e.quads + tid;
            const uint32_t r = i / cols, c = i - r * cols;
            if (valid_px(e.src[i], thr)) f.hit(r, c, c + 1u);
        }
    }
    // across the wave, then across the workgroup's waves
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        f.top = min(f.top, (uint32_t)__shfl_xor((int)f.top, off));
        f.bottom = max(f.bottom, (uint32_t)__shfl_xor((int)f.bottom, off));
        f.left = min(f.left, (uint32_t)__shfl_xor((int)f.left, off));
        f.right = max(f.right, (uint32_t)__shfl_xor((int)f.right, off));
    }
    __shared__ uint32_t part[kBoxBlock / 64][4];
    if ((tid & 63u) == 0u) {
        uint32_t *w = part[tid >> 6];
        w[0] = f.top, w[1] = f.bottom, w[2] = f.left, w[3] = f.right;
    }
    __syncthreads();
    if (tid < 4u) {
        const bool is_min = (tid & 1u) == 0u;  // top and left
        uint32_t v = part[0][tid];
#pragma unroll
        for (int w = 1; w < kBoxBlock / 64; ++w) v = is_min ? min(v, part[w][tid]) : max(v, part[w][tid]);
        uint32_t *slot = a.slots + 4 * p + tid;
        const uint32_t identity = tid == 0u ? rows : (tid == 2u ? cols : 0u);
        if (v != identity) {
            if (is_min) {
                atomicMin(slot, v);
            } else {
                atomicMax(slot, v);
            }
        }
    }
}

__device__ __forceinline__ uint32_t crop_load(const CropEnt &e, uint32_t y, uint32_t x) { return e.src[y * e.ld + x]; }

__global__ __launch_bounds__(kBlock) void crop_kernel(const CropArgs a) {
    const CropEnt &e = a.e[plane_of(a)];
    const uint32_t ocols = e.ocols;
    const uint32_t j = blockIdx.x - e.wg0, tid = threadIdx.x;
    const uint32_t begin = j * e.per, end = min(begin + e.per, e.quads);
    if (begin < end) {
        uint4 *dst4 = reinterpret_cast<uint4 *>(e.dst + e.head);
        const uint32_t i0 = e.head + 4u * (begin + tid);
        uint32_t y = i0 / ocols, x = i0 - y * ocols;
        for (uint32_t q = begin + tid; q < end; q += kBlock) {
            uint4 v;
            if (x + 3u < ocols) {  // inside one row
                const uint32_t *s = e.src + y * e.ld + x;
                if (((uintptr_t)s & 15u) == 0u) {
                    v = *reinterpret_cast<const uint4 *>(s);
                } else {
                    v = make_uint4(s[0], s[1], s[2], s[3]);
                }
            } else {
                uint32_t w[4], yy = y, xx = x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[k] = crop_load(e, yy, xx);
                    if (++xx == ocols) xx = 0u, ++yy;
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            dst4[q] = v;
            y += e.step_r;
            x += e.step_c;
            if (x >= ocols) x -= ocols, ++y;
        }
    }
    if (j == 0u) {
        const uint32_t loose = e.n - 4u * e.quads;
        if (tid < loose) {
            const uint32_t i = tid < e.head ? tid : 4u * e.quads + tid;
            const uint32_t y = i / ocols;
            e.dst[i] = crop_load(e, y, i - y * ocols);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int plane_check(ab_ctx *ctx, const ab_plane *p, size_t i) {
    AB_CHECK(ctx, p && p->data, "null plane %zu", i);
    AB_CHECK(ctx, p->rows >= 1 && p->cols >= 1, "plane %zu has a zero dimension (%lld x %lld)", i, (long long)p->rows, (long long)p->cols);
    AB_CHECK(ctx, fits31(p->rows, p->cols), "plane %zu holds 2^31 pixels or more", i);
    AB_CHECK(ctx, ((uintptr_t)p->data & 3u) == 0, "plane %zu is not float-aligned", i);
    return AB_OK;
}

// how a dense plane of n pixels at `addr` splits into head, groups and workgroups of `block` lanes: as many workgroups as leave each
// about kWorth groups per lane, at most wg_cap; a workgroup's span is a multiple of `block` groups and at least `block` (the last
// workgroup takes what is left).  Returns the workgroup count.
uint32_t split(uintptr_t addr, uint32_t n, int block, int64_t wg_cap, uint32_t *head, uint32_t *quads, uint32_t *per) {
    *head = std::min<uint32_t>((uint32_t)((16u - (addr & 15u)) & 15u) / 4u, n);
    *quads = (n - *head) / 4u;
    const int64_t worth = (int64_t)block * kWorth;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(((int64_t)*quads + worth - 1) / worth, wg_cap));
    const int64_t each = (((int64_t)*quads + want - 1) / want + block - 1) / block * block;
    *per = (uint32_t)std::max<int64_t>(each, block);
    return (uint32_t)std::max<int64_t>(1, ((int64_t)*quads + *per - 1) / *per);
}

// the workgroups each of `planes` planes may have when the launch holds per_cu workgroups per compute unit
int64_t wg_cap(const ab_ctx *ctx, size_t planes, int per_cu) {
    const int64_t cap = (int64_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * per_cu;
    return std::max<int64_t>(1, cap / (int64_t)std::max<size_t>(planes, 1));
}

// the boxes of n checked planes: boxes[4 i ..] = (top, bottom, left, right) of plane i
int detect_boxes(ab_ctx *ctx, const ab_plane *imgs, size_t n, float threshold, std::vector<uint32_t> *boxes) {
    boxes->assign(4 * n, 0u);
    if (n == 0) return AB_OK;
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    std::vector<const float *> src(n, nullptr);
    for (size_t i = 0; i < n; ++i) AB_TRY(sc.stage_in(&imgs[i], &src[i]));
    uint32_t *slots = nullptr;
    AB_TRY(ab_scratch(ctx, 4 * n * sizeof(uint32_t), (void **)&slots));
    for (size_t first = 0; first < n; first += kBatch) {
        const size_t count = std::min<size_t>(kBatch, n - first);
        BoxArgs a;
        memset(&a, 0, sizeof a);
        a.count = (int)count;
        a.threshold = threshold;
        a.slots = slots + 4 * first;
        uint32_t wgs = 0;
        const int64_t cap = wg_cap(ctx, count, kBoxPerCu);
        for (size_t k = 0; k < count; ++k) {
            const ab_plane &p = imgs[first + k];
            BoxEnt &e = a.e[k];
            e.src = src[first + k];
            e.rows = (uint32_t)p.rows, e.cols = (uint32_t)p.cols, e.n = (uint32_t)(p.rows * p.cols);
            e.wg0 = wgs;
            wgs += split((uintptr_t)e.src, e.n, kBoxBlock, cap, &e.head, &e.quads, &e.per);
            e.step_r = 4u * kBoxBlock / e.cols, e.step_c = 4u * kBoxBlock % e.cols;
        }
        hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(bbox_kernel, dim3(wgs), dim3(kBoxBlock), 0, ctx->stream, a);
        AB_HIP(ctx, hipGetLastError());
    }
    void *pin = nullptr;
    AB_TRY(ab_pinned(ctx, 4 * n * sizeof(uint32_t), &pin));
    AB_HIP(ctx, hipMemcpyAsync(pin, slots, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    AB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(boxes->data(), pin, 4 * n * sizeof(uint32_t));
    return AB_OK;
}

ab_crop_box box_of(const uint32_t *b) { return ab_crop_box{b[0], b[1], b[2], b[3]}; }

// the running (max top, min bottom, max left, min right) of :104-116
ab_crop_box common_box(const std::vector<uint32_t> &boxes, size_t n) {
    ab_crop_box c{0, UINT64_MAX, 0, UINT64_MAX};
    for (size_t i = 0; i < n; ++i) {
        c.top = std::max<uint64_t>(c.top, boxes[4 * i]);
        c.bottom = std::min<uint64_t>(c.bottom, boxes[4 * i + 1]);
        c.left = std::max<uint64_t>(c.left, boxes[4 * i + 2]);
        c.right = std::min<uint64_t>(c.right, boxes[4 * i + 3]);
    }
    return c;
}

struct Window {
    int64_t t, b, l, r;
    int64_t rows() const { return b - t; }
    int64_t cols() const { return r - l; }
    int64_t area() const { return rows() * cols(); }
};

// crop_array's clamp (:65-69)
Window clamp_window(const ab_crop_box *box, int64_t rows, int64_t cols) {
    Window w;
    w.t = (int64_t)std::min<uint64_t>(box->top, (uint64_t)rows);
    w.b = std::max<int64_t>((int64_t)std::min<uint64_t>(box->bottom, (uint64_t)rows), w.t);
    w.l = (int64_t)std::min<uint64_t>(box->left, (uint64_t)cols);
    w.r = std::max<int64_t>((int64_t)std::min<uint64_t>(box->right, (uint64_t)cols), w.l);
    return w;
}

uint64_t sat_sub(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }

int out_check(ab_ctx *ctx, const ab_plane *src, const Window &w, const ab_plane_mut *out, size_t i) {
    AB_CHECK(ctx, out, "null output plane %zu", i);
    AB_CHECK(ctx, out->rows == w.rows() && out->cols == w.cols(), "output plane %zu must be %lld x %lld (got %lld x %lld)", i, (long long)w.rows(),
             (long long)w.cols(), (long long)out->rows, (long long)out->cols);
    if (w.area() == 0) return AB_OK;  // nothing is written
    AB_CHECK(ctx, out->data, "null output plane %zu", i);
    AB_CHECK(ctx, ((uintptr_t)out->data & 3u) == 0, "output plane %zu is not float-aligned", i);
    if (src->on_device && out->on_device) {
        const uintptr_t a = (uintptr_t)src->data, al = (uintptr_t)src->rows * (uintptr_t)src->cols * sizeof(float);
        const uintptr_t b = (uintptr_t)out->data, bl = (uintptr_t)w.area() * sizeof(float);
        AB_CHECK(ctx, a + al <= b || b + bl <= a, "output plane %zu overlaps its input", i);
    }
    return AB_OK;
}

// crop_array of n checked planes through their windows into their checked outputs, one launch per kBatch planes; a host plane is
// staged as its window's rows only; stats (nullable): compute_image_stats of each cropped plane, ImageStats::default() for an empty one
int crop_planes(ab_ctx *ctx, const ab_plane *imgs, size_t n, const Window *win, ab_plane_mut *outs, ab_image_stats *stats) {
    AB_HIP(ctx, hipSetDevice(ctx->device));
    AB_TRY(ab_cancel_point(ctx));
    Scope sc(ctx);
    std::vector<float *> dst(n, nullptr);
    std::vector<size_t> live;  // the planes with something to copy
    for (size_t i = 0; i < n; ++i)
        if (win[i].area() > 0) live.push_back(i);
    std::vector<const uint32_t *> origin(n, nullptr);
    for (size_t i : live) {
        const Window &w = win[i];
        if (imgs[i].on_device) {
            origin[i] = reinterpret_cast<const uint32_t *>(imgs[i].data) + w.t * imgs[i].cols + w.l;
        } else {  // rows [t, b) of a host plane are one contiguous block
            const ab_plane band{imgs[i].data + w.t * imgs[i].cols, w.rows(), imgs[i].cols, 0};
            const float *staged = nullptr;
            AB_TRY(sc.stage_in(&band, &staged));
            origin[i] = reinterpret_cast<const uint32_t *>(staged) + w.l;
        }
        AB_TRY(sc.stage_out(&outs[i], &dst[i]));
    }
    for (size_t first = 0; first < live.size(); first += kBatch) {
        const size_t count = std::min<size_t>(kBatch, live.size() - first);
        CropArgs a;
        memset(&a, 0, sizeof a);
        a.count = (int)count;
        uint32_t wgs = 0;
        const int64_t cap = wg_cap(ctx, count, 8);
        for (size_t k = 0; k < count; ++k) {
            const size_t i = live[first + k];
            CropEnt &e = a.e[k];
            e.src = origin[i];
            e.dst = reinterpret_cast<uint32_t *>(dst[i]);
            e.ld = (uint32_t)imgs[i].cols, e.ocols = (uint32_t)win[i].cols(), e.n = (uint32_t)win[i].area();
            e.wg0 = wgs;
            wgs += split((uintptr_t)e.dst, e.n, kBlock, cap, &e.head, &e.quads, &e.per);
            e.step_r = 4u * kBlock / e.ocols, e.step_c = 4u * kBlock % e.ocols;
        }
        hipLaunchKernelGGL(crop_kernel, dim3(wgs), dim3(kBlock), 0, ctx->stream, a);
        AB_HIP(ctx, hipGetLastError());
    }
    if (stats) {
        for (size_t i = 0; i < n; ++i) {
            memset(&stats[i], 0, sizeof stats[i]);  // ImageStats::default()
            if (win[i].area() > 0) AB_TRY(ab_stats_device(ctx, dst[i], win[i].area(), 0, 0.0, 0.0, &stats[i]));
        }
    }
    return sc.finish_outs();
}

}  // namespace

extern "C" {

int ab_detect_valid_region(ab_ctx *ctx, const ab_plane *img, float threshold, ab_crop_box *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, out, "null output");
    AB_TRY(plane_check(ctx, img, size_t(0)));
    std::vector<uint32_t> boxes;
    AB_TRY(detect_boxes(ctx, img, 1, threshold, &boxes));
    *out = box_of(boxes.data());
    return AB_OK;
} AB_CATCH(ctx)

int ab_detect_valid_regions(ab_ctx *ctx, const ab_plane *imgs, size_t n, float threshold, ab_crop_box *out_each, ab_crop_box *out_common) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, imgs || n == 0, "null planes");
    for (size_t i = 0; i < n; ++i) AB_TRY(plane_check(ctx, &imgs[i], i));
    std::vector<uint32_t> boxes;
    AB_TRY(detect_boxes(ctx, imgs, n, threshold, &boxes));
    if (out_each)
        for (size_t i = 0; i < n; ++i) out_each[i] = box_of(&boxes[4 * i]);
    if (out_common) *out_common = common_box(boxes, n);
    return AB_OK;
} AB_CATCH(ctx)

int ab_crop_array(ab_ctx *ctx, const ab_plane *src, const ab_crop_box *box, ab_plane_mut *out) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, box, "null box");
    AB_TRY(plane_check(ctx, src, size_t(0)));
    const Window w = clamp_window(box, src->rows, src->cols);
    AB_TRY(out_check(ctx, src, w, out, 0));
    return crop_planes(ctx, src, 1, &w, out, nullptr);
} AB_CATCH(ctx)

void ab_crop_config_default(ab_crop_config *cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    cfg->auto_detect = 1;
    cfg->threshold = 1e-6f;  // AUTO_THRESHOLD (:12)
}

int ab_crop_channels_plan(ab_ctx *ctx, const ab_plane *imgs, size_t n, const ab_crop_config *cfg, ab_crop_plan *plan, uint64_t *out_dims) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, cfg && plan, "null configuration or plan");
    if (n == 0) return ab_set_error(ctx, AB_ERR_INVALID, "No paths provided for cropping");  // :92-94
    AB_CHECK(ctx, imgs, "null planes");
    for (size_t i = 0; i < n; ++i) AB_TRY(plane_check(ctx, &imgs[i], i));
    memset(plan, 0, sizeof *plan);
    const uint64_t rows0 = (uint64_t)imgs[0].rows, cols0 = (uint64_t)imgs[0].cols;
    if (cfg->auto_detect) {  // :103-122
        std::vector<uint32_t> boxes;
        AB_TRY(detect_boxes(ctx, imgs, n, cfg->threshold, &boxes));
        const ab_crop_box c = common_box(boxes, n);
        if (c.bottom <= c.top || c.right <= c.left) return ab_set_error(ctx, AB_ERR_INVALID, "Auto-crop found no valid overlapping region");
        plan->crop_box = c;
    } else {  // :123-126
        plan->crop_box = ab_crop_box{cfg->top, sat_sub(rows0, cfg->bottom), cfg->left, sat_sub(cols0, cfg->right)};
    }
    plan->auto_detected = cfg->auto_detect ? 1 : 0;
    const Window w0 = clamp_window(&plan->crop_box, imgs[0].rows, imgs[0].cols);  // :170-175
    plan->out_rows = (uint64_t)w0.rows();
    plan->out_cols = (uint64_t)w0.cols();
    plan->actual_top = plan->crop_box.top;  // :179-183
    plan->actual_bottom = sat_sub(rows0, plan->crop_box.bottom);
    plan->actual_left = plan->crop_box.left;
    plan->actual_right = sat_sub(cols0, plan->crop_box.right);
    if (out_dims) {
        for (size_t i = 0; i < n; ++i) {
            const Window w = clamp_window(&plan->crop_box, imgs[i].rows, imgs[i].cols);
            out_dims[2 * i] = (uint64_t)w.rows();
            out_dims[2 * i + 1] = (uint64_t)w.cols();
        }
    }
    return AB_OK;
} AB_CATCH(ctx)

int ab_crop_channels(ab_ctx *ctx, const ab_plane *imgs, size_t n, const ab_crop_plan *plan, ab_plane_mut *outs, ab_image_stats *stats) try {
    if (!ctx) return AB_ERR_INVALID;
    AB_CHECK(ctx, plan, "null plan");
    if (n == 0) return ab_set_error(ctx, AB_ERR_INVALID, "No paths provided for cropping");
    AB_CHECK(ctx, imgs && outs, "null planes");
    std::vector<Window> win(n);
    for (size_t i = 0; i < n; ++i) {
        AB_TRY(plane_check(ctx, &imgs[i], i));
        win[i] = clamp_window(&plan->crop_box, imgs[i].rows, imgs[i].cols);
        AB_TRY(out_check(ctx, &imgs[i], win[i], &outs[i], i));
    }
    return crop_planes(ctx, imgs, n, win.data(), outs, stats);
} AB_CATCH(ctx)

}  // extern "C"
