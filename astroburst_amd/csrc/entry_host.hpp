// Host plumbing of the entry points that take host or device planes: what is released when an entry point returns, on an error exit
// or an exception included, and what the display-side ones refuse before anything touches the device.  Included, checks and all, by
// view.hip, tone.hip, rgb_export.hip, render.hip, compose_rgb.hip, masked_stretch.hip, wizard_color.hip, wizard_stretch.hip,
// wizard_background.hip and compose_step.hip; crop.hip takes fits31 and the scope only (it words its messages by plane number).  The
// scope only, with checks worded by themselves: spcc.hip, color.hip, extras.hip, stf.hip, fits.hip, resample.hip, background.hip,
// subframe.hip, phase_corr.hip, psf.hip, deconv.hip, wavelet.hip, spectrum.hip, synth.hip, drizzle.hip; preview.hip and cube.hip take
// block_minmax too (preview.hip's four-pixel groups of a sweep are its Groups, not a Span); stack_weighted.hip takes the scope and
// device_span / overlap_check (its other checks are worded like stack_sigma_clip.hip's).  Not included by the benchmark's path
// and the multi-rank code (stats, detect, affine, batch_pipeline, stack_*, sharded, comm), whose plumbing is workspaces and child contexts.
//   checks      fits31, plane_check, same_dims_check, out_planes_check, preview_of
//   overlap     overlap_check over Spans.  Two forms of a span, kept apart because the entry points answer differently today:
//               span_of -- the wizard's steps (wizard_*.hip): host memory counts too, and outputs may not overlap each other;
//               device_span -- view.hip, tone.hip, rgb_export.hip: only a DEVICE output over a DEVICE input is refused.  They stage a
//               host output through a temporary, so a host call in place works and must keep working; they hand over one output
//               at a time, so no output / output pair is tested that was not tested before.
//   scope       Scope: staged inputs, staged outputs and the call's device planes, released in that order's reverse on return
//   placement   head16, head_bytes: the pixels before the four-pixel groups
//   device      nn_index (the preview's nearest-neighbour pick), quantise (its byte), block_minmax (wave shuffle, then kBlock / 64 LDS words)
// The streaming grid's size is ab_common.hpp's ab_stream_grid.  A new entry-point file includes this header; it does not copy it.
#pragma once
#include "ab_common.hpp"

#include <algorithm>
#include <deque>

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

// three present channels of one size, dims taken from R (rgb.rs:13, curves.rs:80, cmd/io/mod.rs:56)
int same_dims_check(ab_ctx *ctx, const ab_plane *const ch[3]) {
    for (int c = 0; c < 3; ++c) AB_TRY(plane_check(ctx, ch[c], kChan[c]));
    for (int c = 1; c < 3; ++c)
        AB_CHECK(ctx, ch[c]->rows == ch[0]->rows && ch[c]->cols == ch[0]->cols, "the %s plane is %lld x %lld, R is %lld x %lld", kChan[c],
                 (long long)ch[c]->rows, (long long)ch[c]->cols, (long long)ch[0]->rows, (long long)ch[0]->cols);
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

struct Preview {  // the preview of ab_preview_dims
    int64_t ph = 0, pw = 0;
    bool sampled = false;  // the image exceeds max_dim: the preview is a pick (helpers.rs:283-290)
};
int preview_of(ab_ctx *ctx, int64_t rows, int64_t cols, int64_t max_dim, Preview *pv) {
    AB_CHECK(ctx, ab_preview_dims(rows, cols, max_dim, &pv->ph, &pv->pw) == AB_OK, "the preview's dimensions could not be computed");
    pv->sampled = pv->ph != rows || pv->pw != cols;
    return AB_OK;
}

struct Span {  // bytes [at, at + len) on the host or the device; a span of no bytes overlaps nothing
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
// the form that counts device-resident memory only: host memory and a null pointer give a span of no bytes
Span device_span(const void *p, size_t len, int32_t on_device) { return Span{(uintptr_t)p, p && on_device ? len : 0, true}; }
Span device_span(const ab_plane &p) { return device_span(p.data, (size_t)p.rows * (size_t)p.cols * sizeof(float), p.on_device); }

// Releases / aborts everything registered with it when the entry point returns.  The deques never move an element, so a pointer to a
// staged plane or output stays good for the length of the call, however many follow it.  A loop that stages one plane per iteration
// opens a Scope per iteration, inside the call's own; such an inner Scope stages and adopts but must not alloc(): slot numbering starts
// at zero in each Scope, so its first plane would be the outer one's.
struct Scope {
    ab_ctx *ctx;
    std::deque<StagedPlane> ins;
    std::deque<StagedOut> outs;
    std::vector<void *> dev;  // the planes past the eight scope slots, and what adopt() took
    int next_slot = 0;
    explicit Scope(ab_ctx *c) : ctx(c) {}
    ~Scope() {
        for (StagedOut &o : outs) ab_stage_out_abort(ctx, &o);  // (a finished output owns nothing any more)
        if (!dev.empty()) (void)hipStreamSynchronize(ctx->stream);
        for (void *p : dev) (void)hipFree(p);
        for (StagedPlane &p : ins) ab_stage_release(ctx, &p);
    }
    int stage_in(const ab_plane *p, const float **dptr) {
        ins.emplace_back();
        AB_TRY(ab_stage_in(ctx, p, &ins.back()));
        *dptr = ins.back().dptr;
        return AB_OK;
    }
    int stage_out(const ab_plane_mut *p, float **dptr) {
        outs.emplace_back();
        AB_TRY(ab_stage_out_begin(ctx, p, &outs.back()));
        *dptr = outs.back().dptr;
        return AB_OK;
    }
    int finish_outs() {  // downloads the host outputs, in the order they were staged; what an error leaves is the destructor's
        for (StagedOut &o : outs) AB_TRY(ab_stage_out_finish(ctx, &o));
        return AB_OK;
    }
    // the wizard's steps instead enqueue the host outputs' copies, which join the step's ONE synchronisation (*wait: there is something
    // to wait for); the destructor frees the staging buffers
    int enqueue_host_outs(bool *wait) {
        for (const StagedOut &o : outs)
            if (o.owned) {
                AB_HIP(ctx, hipMemcpyAsync(o.host, o.dptr, o.bytes, hipMemcpyDeviceToHost, ctx->stream));
                *wait = true;
            }
        return AB_OK;
    }
    // a device plane for the length of the call, out of the context's scope slots (kept between calls); a ninth one is allocated,
    // and freed once the stream has drained
    int alloc(void **p, size_t bytes) {
        if (next_slot < 8) return ab_workspace(ctx, AB_WS_SCOPE0 + next_slot++, std::max<size_t>(bytes, 16), p);
        AB_HIP(ctx, hipMalloc(p, std::max<size_t>(bytes, 16)));
        dev.push_back(*p);
        return AB_OK;
    }
    // a per-call hipMalloc of the entry point's own, freed with the rest once the stream has drained
    void adopt(void *p) { dev.push_back(p); }
};

// the pixels before the first 16-byte group of a float plane
int64_t head16(const void *p, int64_t n) { return std::min<int64_t>(n, (int64_t)(((16 - (uintptr_t)p % 16) % 16) / sizeof(float))); }
// the pixels before the first one whose byte triple starts a dword: 3 head = -addr (mod 4)
int64_t head_bytes(const uint8_t *out, int64_t n) { return std::min<int64_t>(n, (int64_t)((3 * ((4 - (uintptr_t)out % 4) % 4)) % 4)); }

// ((d as f64) * ratio).min((len - 1) as f64) as usize (helpers.rs:306, :309)
__device__ __forceinline__ int64_t nn_index(int64_t d, double ratio, int64_t len) {
    const double s = (double)d * ratio, hi = (double)(len - 1);
    return (int64_t)(s < hi ? s : hi);
}

// (v.clamp(0, 1) * 255f32) as u8: f32::clamp keeps a NaN, `as` truncates and sends NaN to 0 (helpers.rs:243-245)
__device__ __forceinline__ uint32_t quantise(float s) {
    const float c = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
    const float x = c * 255.0f;
    return x == x ? (uint32_t)x : 0u;
}

// wave reduce -> LDS -> every lane holds the block's min / max
__device__ __forceinline__ void block_minmax(float &mn, float &mx) {
    __shared__ float smn[kBlock / 64], smx[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x / 64] = mn;
        smx[threadIdx.x / 64] = mx;
    }
    __syncthreads();
    mn = smn[0];
    mx = smx[0];
    for (int w = 1; w < kBlock / 64; ++w) {
        mn = fminf(mn, smn[w]);
        mx = fmaxf(mx, smx[w]);
    }
    __syncthreads();
}

}  // namespace
