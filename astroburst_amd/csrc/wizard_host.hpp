// Host plumbing shared by the compose wizard's steps (wizard_color.hip, wizard_stretch.hip): argument checks that run before anything
// touches the device, the overlap test of outputs against inputs, the scope that releases staged planes, the persistent grid's size,
// and the preview's nearest-neighbour pick.
#pragma once
#include "ab_common.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = 256;

const char *const kChan[3] = {"R", "G", "B"};

bool fits31(int64_t rows, int64_t cols) { return rows <= ((int64_t(1) << 31) - 1) / cols; }  // rows * cols < 2^31 (cols >= 1)

int plane_check(ab_ctx *ctx, const ab_plane *p, const char *what) {
    AB_CHECK(ctx, p && p->data, "null %s plane", what);
    AB_CHECK(ctx, p->rows >= 1 && p->cols >= 1, "the %s plane has a zero dimension (%lld x %lld)", what, (long long)p->rows, (long long)p->cols);
    AB_CHECK(ctx, fits31(p->rows, p->cols), "the %s plane holds 2^31 pixels or more", what);
    AB_CHECK(ctx, ((uintptr_t)p->data & 3u) == 0, "the %s plane is not float-aligned", what);
    return AB_OK;
}

int out_planes_check(ab_ctx *ctx, const ab_plane_mut *out_planes, int64_t rows, int64_t cols) {
    AB_CHECK(ctx, out_planes, "null output planes");
    for (int c = 0; c < 3; ++c) {
        AB_CHECK(ctx, out_planes[c].data, "null output %s plane", kChan[c]);
        AB_CHECK(ctx, out_planes[c].rows == rows && out_planes[c].cols == cols, "the output %s plane must be %lld x %lld (got %lld x %lld)", kChan[c],
                 (long long)rows, (long long)cols, (long long)out_planes[c].rows, (long long)out_planes[c].cols);
        AB_CHECK(ctx, ((uintptr_t)out_planes[c].data & 3u) == 0, "the output %s plane is not float-aligned", kChan[c]);
    }
    return AB_OK;
}

struct Span {  // bytes [at, at + len) on the host or the device
    uintptr_t at;
    size_t len;
    bool dev;
};
bool overlaps(const Span &a, const Span &b) { return a.dev == b.dev && a.len && b.len && a.at < b.at + b.len && b.at < a.at + a.len; }

// no output may overlap an input or another output
int overlap_check(ab_ctx *ctx, const std::vector<Span> &ins, const std::vector<Span> &outs) {
    for (size_t o = 0; o < outs.size(); ++o) {
        for (const Span &i : ins) AB_CHECK(ctx, !overlaps(outs[o], i), "an output overlaps an input plane");
        for (size_t p = o + 1; p < outs.size(); ++p) AB_CHECK(ctx, !overlaps(outs[o], outs[p]), "two outputs overlap");
    }
    return AB_OK;
}

Span span_of(const ab_plane &p) { return Span{(uintptr_t)p.data, (size_t)p.rows * (size_t)p.cols * sizeof(float), p.on_device != 0}; }
Span span_of(const ab_plane_mut &p) { return Span{(uintptr_t)p.data, (size_t)p.rows * (size_t)p.cols * sizeof(float), p.on_device != 0}; }

struct Scope {  // releases / aborts everything registered with it when the entry point returns
    ab_ctx *ctx;
    std::vector<StagedPlane> ins;
    StagedOut outs[3];
    int n_outs = 0;
    explicit Scope(ab_ctx *c) : ctx(c) {}
    ~Scope() {
        for (int i = 0; i < n_outs; ++i) ab_stage_out_abort(ctx, &outs[i]);
        for (StagedPlane &p : ins) ab_stage_release(ctx, &p);
    }
    int stage_in(const ab_plane *p, const float **dptr) {
        ins.emplace_back();
        AB_TRY(ab_stage_in(ctx, p, &ins.back()));
        *dptr = ins.back().dptr;
        return AB_OK;
    }
};

int persistent_grid(ab_ctx *ctx, int64_t lanes) {
    const int64_t cap = (int64_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>((lanes + kBlock - 1) / kBlock, cap));
}

// ((d as f64) * ratio).min((len - 1) as f64) as usize (helpers.rs:297, :300)
__device__ __forceinline__ int64_t nn_index(int64_t d, double ratio, int64_t len) {
    const double s = (double)d * ratio, hi = (double)(len - 1);
    return (int64_t)(s < hi ? s : hi);
}

}  // namespace
