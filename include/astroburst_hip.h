/*
 * astroburst_hip.h -- C ABI of libastroburst_hip.so, the MI355X (gfx950) implementation of
 * AstroBurst's pixel-compute hot path.
 *
 * The reference (Rust, src-tauri/) has no FFI seam of its own; the replaceable edge is the
 * internal call `cmd::* -> core::*`.  Every entry point below replaces one
 * `core::*` function and cites it (paths relative to src-tauri/src/).  INTEGRATION.md shows the
 * Rust `extern "C"` block and the safe wrappers a maintainer would add.
 *
 * Conventions
 *  - plain C types only; all functions return an ab_status (0 = ok) and never abort/throw
 *    (the app is built panic="abort", Cargo.toml:64).  ab_last_error(ctx) returns the message,
 *    worded like the reference's anyhow strings where one exists (e.g. "No images to stack").
 *  - planes are contiguous row-major f32, dims (rows, cols), exactly ndarray::Array2<f32>'s
 *    standard layout (`.as_slice().expect("contiguous")`, combine.rs:152-155).
 *  - an ab_plane may point at HOST memory (on_device = 0: staged through HBM by the library)
 *    or at DEVICE memory (on_device = 1: used in place, nothing is copied).  Inputs are
 *    borrowed and never modified; outputs are caller-allocated.
 *  - a context owns one HIP stream (or borrows the caller's, ab_ctx_set_stream) and a scratch
 *    arena; it is not shared between threads -- create one per calling thread (the Tauri
 *    commands run concurrently on tokio blocking threads, cmd/common.rs:345-352).
 *  - device-plane calls are asynchronous on the context's stream unless they return scalars.
 *
 * Environment
 *  The library reads these eight variables and no others (each when a context / communicator is created, AB_TRACE per call).
 *  None changes a result: every engine they select is held to the same oracle by the tests.
 *    AB_TRACE=1              stage stamps, deferred-pixel and redone-frame notes on stderr (also fills AB_FB_STACK_GENERAL_PIXELS)
 *    AB_STACK_EXACT=1        ab_stack_*: the direct two-pass clipping engine instead of the running-sum one (bit-exact cross-check
 *                            of the default engine's contract -- rejected count exact, every value within 1e-5 relative, see
 *                            ab_stack_sigma_clip; this engine: bit for bit on every pixel; ~1.3x slower)
 *    AB_STATS_CHAIN=1        ab_compute_image_stats*: the histogram chain instead of the register-resident kernel (identical results;
 *                            what a resident launch falls back to by itself when its grid barrier times out)
 *    AB_REGISTER_WORKERS=n   host threads (= frame groups in flight) of ab_register_frames / ab_align_pairs_affine (default 12)
 *    AB_STACK_DEEP_FROM=n    stacks of more than n frames (64 <= n <= 4096, default 4096) take the workgroup-per-pixel kernel
 *    AB_BATCH_DEEP_FROM=n    the same for ab_sigma_clipped_mean_stack (64 <= n <= 2048, default 2048)
 *    AB_COMM_TIMEOUT_MS=n    how long a rank waits on a collective (either transport) before AB_ERR_COMM (default 300000)
 *    AB_COMM_HOST_SLOT_MB=n  host-staged communicator: size of a rank's shared-memory slot, 1 .. 1024 (default 4)
 *  Superseded kernel forms, sweep knobs, stage cuts and fault injection exist only in the developer build
 *  (`make -C astroburst_amd/csrc dev` -> libastroburst_hip_dev.so, ab_version() ends in "+dev"); the release library does not
 *  contain their names (tests/test_abi_cpu.py checks both lists against the sources and the built library).
 */
#ifndef ASTROBURST_HIP_H
#define ASTROBURST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AB_API __attribute__((visibility("default")))

typedef enum {
    AB_OK = 0,
    AB_ERR_INVALID = 1,     /* bad argument (message says which) */
    AB_ERR_HIP = 2,         /* HIP runtime error (message carries hipGetErrorString) */
    AB_ERR_NO_DEVICE = 3,   /* no gfx950 device / wrong architecture */
    AB_ERR_UNSUPPORTED = 4, /* valid request this build cannot serve yet */
    AB_ERR_NOMEM = 5,
    AB_ERR_COMM = 6,      /* RCCL unavailable or a collective failed (message carries ncclGetErrorString) */
    AB_ERR_CANCELLED = 7  /* the host set the context's cancel flag (AppError::Cancelled, core/imaging/background.rs:80-82) */
} ab_status;

typedef struct ab_ctx ab_ctx;
typedef struct ab_comm ab_comm; /* one RCCL rank bound to a context's GPU: section (e) at the end of this header */

typedef struct {
    const float *data;
    int64_t rows, cols;
    int32_t on_device; /* 0 host, 1 device (HBM) */
} ab_plane;

typedef struct {
    float *data;
    int64_t rows, cols;
    int32_t on_device;
} ab_plane_mut;

/* ---- context / memory ------------------------------------------------------------------- */
AB_API int ab_ctx_create(int device_id, ab_ctx **out);
AB_API void ab_ctx_destroy(ab_ctx *ctx);
AB_API const char *ab_last_error(const ab_ctx *ctx);
AB_API const char *ab_version(void);
/* borrow an existing hipStream_t (e.g. PyTorch's current stream).  A NULL handle means HIP's
 * default stream, which is what PyTorch runs on unless told otherwise. */
AB_API int ab_ctx_set_stream(ab_ctx *ctx, void *hip_stream);
/* go back to the context's own (non-blocking) stream */
AB_API int ab_ctx_reset_stream(ab_ctx *ctx);
AB_API void *ab_ctx_get_stream(ab_ctx *ctx);
AB_API int ab_ctx_synchronize(ab_ctx *ctx);
AB_API int ab_device_alloc(ab_ctx *ctx, size_t bytes, void **out_dptr);
AB_API int ab_device_free(ab_ctx *ctx, void *dptr);
AB_API int ab_upload(ab_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
AB_API int ab_download(ab_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);
/* Progress / cancel (infra/progress.rs:39-74; taken as Option<&ProgressHandle> by core/imaging/background.rs:55-59).
 * cb(stage, current, total, user) is called on the calling thread at the reference's own stage boundaries with its stage
 * strings ("sampling background", "fitting polynomial surface", "generating model", "applying correction") and once per
 * frame by the frame loops (stage "registration" for ab_register_frames / ab_align_pairs_affine, "subframe" for
 * ab_analyze_subframes); NULL removes it.  ab_ctx_request_cancel may be called from any
 * thread: the next stage boundary returns AB_ERR_CANCELLED ("Operation cancelled") and leaves the flag set until
 * ab_ctx_clear_cancel. */
typedef void (*ab_progress_cb)(const char *stage, uint64_t current, uint64_t total, void *user);
AB_API int ab_ctx_set_progress_cb(ab_ctx *ctx, ab_progress_cb cb, void *user);
AB_API int ab_ctx_request_cancel(ab_ctx *ctx);
AB_API int ab_ctx_clear_cancel(ab_ctx *ctx);
/* device properties the bench prints: name, CU count, HBM bytes */
AB_API int ab_device_info(ab_ctx *ctx, char *name, size_t name_cap, int *cu_count, uint64_t *hbm_bytes);
/* Release what the context has grown for its calls: the scratch arena, every workspace, the HBM staging area of host-resident
 * frames (as large as the largest frame set it was given), the pinned read-back buffers and the declined-tile lists -- its frame
 * workers' too.  The context stays usable: the next call allocates what it needs again.  Blocks until the context's streams are
 * idle.  Every buffer is released whatever an earlier release returned; the first failure is the return code, its text in
 * ab_last_error(ctx).  A long-lived host (one ab_ctx per command thread, infra/cache.rs keeps the planes) calls it after a large
 * batch.  (ab_stack_images(align) gives its registered copies back by itself when they exceed 1 GiB.) */
AB_API int ab_ctx_trim(ab_ctx *ctx);
/* Every fast path of the library has an exact fallback that gives the SAME result (a frame redone through the full component list,
 * a background tile settled by the resident kernel, a statistics launch repeated as the histogram chain).  They are silent in the
 * results and not in the run time, so the context counts them (its frame workers' too): out[k] = events of kind k since the
 * context was created (or since the last call with reset != 0), for k < min(cap, AB_FB_COUNT).  Thread-safe. */
typedef enum {
    AB_FB_FRAMES_REDONE = 0,  /* detect_stars of a registration frame redone through the full path (any of the four reasons below) */
    AB_FB_TILE_SLOTS,         /* ... a 32 x 128 labelling tile held more components than its record slots */
    AB_FB_COMPONENT_TABLE,    /* ... more components than the chained table holds */
    AB_FB_SELECTION_SHORT,    /* ... the brightest 480 components did not yield the matcher's 120 stars and fainter ones exist */
    AB_FB_SELECTION_CUT,      /* ... the faintest kept star lay within two key steps of the selection's cut */
    AB_FB_TILES_DECLINED,     /* background tiles the streaming kernel declined (settled by the resident tile kernel) */
    AB_FB_STATS_CHAIN,        /* compute_image_stats launches whose resident kernel aborted and were repeated as the chain */
    AB_FB_STACK_GENERAL_PIXELS, /* pixels the stack's fast pass handed to its general pass (counted only under AB_TRACE=1) */
    AB_FB_LABEL_TILES_DENSE,  /* 256 x 256 labelling tiles of registration frames read from the frame: no usable candidate list from the tile pass
                                 (a partial tile, a tile brighter than the frame's threshold, an overflowed list, a tile the streaming kernel declined) */
    AB_FB_COUNT
} ab_fallback_kind;
AB_API int ab_ctx_fallback_counts(ab_ctx *ctx, uint64_t *out, size_t cap, int reset);

/* ---- a1/a2  core/stacking/combine.rs ------------------------------------------------------ */
/* StackConfig, types/stacking.rs:3-20 (defaults 3.0, 3.0, 5, align=true) */
typedef struct {
    float sigma_low;
    float sigma_high;
    uint32_t max_iterations;
    int32_t align; /* bool */
} ab_stack_config;

/* The per-pixel kernel of stack_images (combine.rs:160-182 + sigma_clip_combine :14-92):
 * out[y][x] = sigma_clip_combine({planes[k][y][x] finite}, sigma_low, sigma_high, max_iter).
 * All planes must be at least out->rows x out->cols; each is read with its own row stride
 * (= its cols), i.e. the reference's top-left crop to the minimum dims (combine.rs:104-113)
 * costs nothing.  *out_rejected receives StackResult.rejected_pixels (sum of per-pixel
 * rejection counts, combine.rs:158,181).  Any frame count the reference takes (it gathers a Vec per pixel: no limit; here up to
 * 2^24 per call): up to 256 contiguous frames a pixel's samples live in one lane's registers (64: the HBM-bound kernel; 65 .. 128:
 * ~4 ms and 129 .. 256: ~10-16 ms for 4096^2), 257 .. 512 in two lanes', up to 4096 -- or with ragged strides -- in one wave's
 * (stack_wide.hip), beyond that a workgroup sorts a pixel's samples in a scratch segment (stack_deep.hip): same results, slower.
 * Floating-point contract.  The reference's result depends on the order select_nth_unstable leaves the survivors in (SURVEY.md 7
 * hard part 2); the definition here: the f64 sums of iterations >= 1 run over the survivors in ascending value order.
 *   - DEFAULT ENGINE (2 .. 64 frames): within 1e-5 relative of that definition on every pixel -- north_star's tolerance.  Its
 *     iterations >= 1 take mean and variance from running sums about the median (E = sum(x - c0), Q = sum(x - c0)^2 in f64: mean =
 *     (n c0 + E) / n, sum(x - mean)^2 = Q - n (mean - c0)^2), a few ulp(f64) away from the two-pass sums; an ulp can flip the
 *     clipping decision of a sample that sits exactly on a bound.  The same contract holds from 129 to 4096 frames (fast multi-lane
 *     passes with running moments; above 512 frames the survivors are summed as a tree).  Guaranteed: the rejected count equals the
 *     oracle's exactly; every value within 1e-5 relative; pixels whose arithmetic is exact (samples exactly on a threshold, sums exact
 *     in f64) bit for bit -- tests/test_gpu_stack_adversarial.py holds all three on adversarial pixels at 3 .. 4100 frames.  Outside
 *     any relative bound: a kept sample whose deviation from the median overflows f32 (sigma inf): every route but AB_STACK_EXACT=1
 *     holds only its rejected count.  MEASURED: 0 of 16.7 M pixels of
 *     the bench stack differ; the older tests allow 1e-4 of the pixels of natural data to differ at all (tests/test_gpu_stack.py).
 *   - AB_STACK_EXACT=1 when the context is created: the direct two-pass engine, bit-identical BY CONSTRUCTION (the tests run both).
 *   - 65 .. 128 frames and row bands (ab_stack_sigma_clip_rows / _rowband) run the same fast engine under the same contract.
 *   - more than 4096 frames (or AB_STACK_DEEP_FROM: the workgroup-per-pixel kernel, ascending sums): bit-identical but for the
 *     sigma-inf pixels above; median combine: bit-identical. */
AB_API int ab_stack_sigma_clip(ab_ctx *ctx, const ab_plane *planes, size_t n, const ab_stack_config *cfg,
                               ab_plane_mut *out, uint64_t *out_rejected);

/* Passing out_rejected = NULL to ab_stack_sigma_clip keeps the call fully asynchronous on the
 * context's stream; the count of that last stack can be fetched later (synchronises). */
AB_API int ab_stack_last_rejected(ab_ctx *ctx, uint64_t *out_rejected);
/* milliseconds between the HIP events the library records on the context's stream immediately before the first and
 * after the last stack kernel of the most recent multi-frame ab_stack_* call (blocks until that call has finished):
 * the kernels' own duration, free of the caller's launch overhead (bench.py's roofline) */
AB_API int ab_stack_last_kernel_ms(ab_ctx *ctx, float *out_ms);

/* stack_images (combine.rs:94-193): crops to the minimum dims, optionally registers frames
 * 1..n-1 on frame 0 (PhaseCorrelation, combine.rs:126-138), then sigma-clip combines.
 * out must be min_rows x min_cols.  offsets (nullable) receives n (dy, dx) pairs rounded to
 * i32 as the reference reports them (combine.rs:135-137).  Errors: n == 0 -> AB_ERR_INVALID
 * "No images to stack" (combine.rs:98-100). */
AB_API int ab_stack_images(ab_ctx *ctx, const ab_plane *planes, size_t n, const ab_stack_config *cfg,
                           ab_plane_mut *out, int32_t *offsets_dy_dx, uint64_t *out_rejected);

/* Frame-sharded partial: per pixel the f64 sum and the u32 count of
 * the survivors of THIS shard's frames; ranks all-reduce (sum, count) and divide.  This is a
 * two-level estimator, not the reference's single-level one; its CPU checker is
 * orc_stack_partial_noalign.  out_sum/out_cnt are device pointers of rows*cols elements. */
AB_API int ab_stack_sigma_clip_partial(ab_ctx *ctx, const ab_plane *planes, size_t n,
                                       const ab_stack_config *cfg, int64_t rows, int64_t cols,
                                       double *out_sum_dev, uint32_t *out_cnt_dev, uint64_t *out_rejected);
/* out[i] = cnt[i] ? (float)(sum[i] / cnt[i]) : 0  -- the divide after the all-reduce */
AB_API int ab_stack_finalize_partial(ab_ctx *ctx, const double *sum_dev, const uint32_t *cnt_dev, int64_t n,
                                     float *out_dev);

/* ---- a3/a5  core/stacking/align.rs:36-57, core/alignment/affine.rs:663-690 ---------------- */
/* shift_image_subpixel(image, dy, dx): out(y,x) = bicubic(src, y+dy, x+dx), 0.0 where the
 * sample centre leaves [-0.5, dim-0.5]; |dy|,|dx| < 1e-12 is a copy. */
AB_API int ab_shift_image_subpixel(ab_ctx *ctx, const ab_plane *src, double dy, double dx, ab_plane_mut *out);
/* warp_image(image, &AffineTransform{a,b,tx,c,d,ty}, out_rows, out_cols): the transform maps
 * OUTPUT (x,y) to SOURCE (sx,sy) (affine.rs:74-80); 0.0 outside 0<=sx<cols-1, 0<=sy<rows-1. */
AB_API int ab_warp_image(ab_ctx *ctx, const ab_plane *src, const double transform[6], ab_plane_mut *out);

/* rows [row0, row0 + out_band->rows) of warp_image(src, transform, out_rows, out_band->cols): the band of a row-sharded
 * registration; coordinates are those of the whole output, so the band equals the same rows of ab_warp_image. */
AB_API int ab_warp_image_rows(ab_ctx *ctx, const ab_plane *src, const double transform[6], int64_t out_rows, int64_t row0,
                              ab_plane_mut *out_band);
/* The same with the SOURCE given as a band (a rank of the row-band scheme ingests its rows of every frame + a
 * halo, not the frame set): src_band = rows [src_row0, src_row0 + src_band->rows) of a frame of src_rows rows.  The band must
 * cover ab_warp_source_rows of the request (AB_ERR_INVALID names the rows otherwise); the result equals the same rows of
 * ab_warp_image on the whole frame bit for bit.  Device planes. */
AB_API int ab_warp_image_rows_from_band(ab_ctx *ctx, const ab_plane *src_band, int64_t src_row0, int64_t src_rows, const double transform[6],
                                        int64_t out_rows, int64_t row0, ab_plane_mut *out_band);
/* source rows [*src_row0, *src_row0 + *src_nrows) that rows [row0, row0 + nrows) of warp_image(src, transform, .., out_cols) read
 * from a src_rows x src_cols frame (affine.rs:663-690: sy = c x + d y + ty at the band's corners; sampling.rs:48-80: rows
 * floor(sy) - 1 .. floor(sy) + 2, clamped): exact, not a bound with a margin; 0 rows when the band maps outside the frame */
AB_API int ab_warp_source_rows(const double transform[6], int64_t src_rows, int64_t src_cols, int64_t out_cols, int64_t row0, int64_t nrows,
                               int64_t *src_row0, int64_t *src_nrows);

/* ---- a8  core/alignment/phase_correlation.rs ------------------------------------------------- */
typedef struct { double dx, dy, confidence; } ab_phase_correlation_result; /* PhaseCorrelationResult, :15-20 */
/* phase_correlate(reference, target) (phase_correlation.rs:22-89): crops both to the common dims,
 * returns (0, 0, 0) for constant / nearly empty images, correlates directly up to 512 x 512 and
 * coarse (area-averaged 512 x 512) + fine (centred 512 x 512 crop) above.  The FFT arithmetic is
 * ours (the reference uses rustfft); the reference's own tests pin the shift to +-1 px. */
AB_API int ab_phase_correlate(ab_ctx *ctx, const ab_plane *reference, const ab_plane *target,
                              ab_phase_correlation_result *out);
/* correlate_single (phase_correlation.rs:105-141) for two equal planes of at most 512 x 512;
 * surface_host (nullable) receives the fft_rows x fft_cols correlation surface (parity tests) */
AB_API int ab_correlate_single(ab_ctx *ctx, const ab_plane *a, const ab_plane *b, ab_phase_correlation_result *out,
                               double *surface_host);

/* ---- a7  core/analysis/star_detection.rs ------------------------------------------------------ */
typedef struct { /* DetectedStar, star_detection.rs:10-20 */
    double x, y, flux, fwhm, eccentricity, peak, snr;
    uint64_t npix;
} ab_detected_star;
/* estimate_background (star_detection.rs:32-84): per-tile sigma-clipped median / sigma, then the
 * [len/2] element of the sorted tile medians and sigmas; (0, 1) if no tile has 8 valid pixels */
AB_API int ab_estimate_background(ab_ctx *ctx, const ab_plane *img, int64_t tile_size, double *out_median,
                                  double *out_sigma);
/* the tile map behind estimate_background (star_detection.rs:36-68): tiles in row-major order, step = max(tile_size, 16);
 * per tile sigma_clipped_stats(valid pixels, 3.0, 2) = (median, sigma) and valid = the tile had >= 8 valid pixels.
 * Writes at most cap tiles; *out_tiles = tile count, *out_tiles_x = tiles per row. */
AB_API int ab_background_tile_stats(ab_ctx *ctx, const ab_plane *img, int64_t tile_size, double *out_median, double *out_sigma,
                                    int32_t *out_valid, size_t cap, size_t *out_tiles, size_t *out_tiles_x);
/* detect_stars(image, sigma) (star_detection.rs:86-258): threshold at median + sigma * bg_sigma,
 * 8-connected components seeded from interior pixels, 3 <= npix <= 5000, flux-weighted moments,
 * FWHM in [0.5, 30], sorted by flux (descending), deduplicated within 3 px.  Writes at most cap
 * stars; *out_total (nullable) is the number found.  Segmentation (component set, npix, order)
 * is exact; the f64 moments are summed in raster instead of BFS order (~1e-15 relative). */
AB_API int ab_detect_stars(ab_ctx *ctx, const ab_plane *img, double sigma_threshold, ab_detected_star *out, size_t cap,
                           size_t *out_count, size_t *out_total, double *bg_median, double *bg_sigma);

/* ---- a6  core/alignment/affine.rs -------------------------------------------------------------- */
typedef struct { /* AffineAlignResult, affine.rs:82-89 */
    double transform[6]; /* AffineTransform a, b, tx, c, d, ty: output (x, y) -> source (affine.rs:55-80) */
    uint64_t matched_stars, inliers;
    double residual_px;
    int32_t method; /* 0 affine, 1 rigid, 2 phase_correlation, 3 identity (AffineAlignMethod, :91-97) */
} ab_affine_align_result;
/* normalize_for_detection (affine.rs:24-53): clamp((v - p1) / (p99.9 - p1), 0, 1) on a <= 100 k subsample's percentiles */
AB_API int ab_normalize_for_detection(ab_ctx *ctx, const ab_plane *img, ab_plane_mut *out);
/* align_channel_affine(reference, target) (affine.rs:129-212): normalise, detect at 3.5 sigma, top 120
 * stars, triangle voting, RANSAC affine then rigid (2000 draws, 3 px inliers), sanity limits, else
 * phase correlation (confidence >= 1.5), else identity.  num_threads pins what the reference takes
 * from rayon::current_num_threads() (the draws are partitioned and seeded per worker, :410-416);
 * vote ties are broken by (ref, tgt) index (the reference iterates a HashMap). */
AB_API int ab_align_channel_affine(ab_ctx *ctx, const ab_plane *reference, const ab_plane *target, int num_threads,
                                   ab_affine_align_result *out);
/* align_channel_affine(reference, targets[i]) for i < n in one call: the loop a stacking / compose caller runs
 * (cmd/compose/blend.rs:226-232, rgb.rs:165-189).  The reference frame's normalisation, detection and triangle
 * table are computed once; each out[i] equals what ab_align_channel_affine(reference, targets[i]) returns. */
AB_API int ab_register_frames(ab_ctx *ctx, const ab_plane *reference, const ab_plane *targets, size_t n, int num_threads,
                              ab_affine_align_result *out);
/* align_pair(reference, targets[i], AlignMethod::Affine) for i < n (core/alignment/pair.rs:41-77): the estimate above
 * followed by warp_image(target, transform) into aligned[i] (device planes); each worker warps its frame right after
 * estimating it, so the warps overlap the other frames' detection.  The reference and any target may be HOST planes
 * (on_device = 0), as the application holds its frames (core/stacking/calibration.rs:306-315, infra/cache.rs:306-310):
 * the library copies them into HBM on its own stream, one event per frame, and registers each frame as it lands -- the
 * call costs the upload plus one group's registration, not upload + registration.  Pinned host memory keeps the copies
 * asynchronous; results do not depend on where a frame started. */
AB_API int ab_align_pairs_affine(ab_ctx *ctx, const ab_plane *reference, const ab_plane *targets, size_t n, int num_threads,
                                 ab_affine_align_result *out, ab_plane_mut *aligned);
/* the star-list half (triangles -> votes -> RANSAC -> sanity) on given centroids; host only */
AB_API int ab_affine_from_stars(const double *ref_xy, size_t n_ref, const double *tgt_xy, size_t n_tgt, int64_t rows,
                                int64_t cols, int num_threads, ab_affine_align_result *out, int *found);
/* The matcher's seam (test hooks; nothing in the reference corresponds to them as functions).  Vote matrices are 64 x 64 uint32_t,
 * row = reference star index, column = target star index; only the first 60 stars of a list form triangles and collect votes
 * (build_triangles' limit, :285), a list is cut to its first 120 (top_n_stars), and a pair with a list of fewer than 4 stars
 * has an all-zero matrix (:162-168).  A coordinate that is not finite is AB_ERR_INVALID (the reference panics on it).
 *   ab_triangle_votes_host    the vote half of match_triangles (:320-350) on the host; no context
 *   ab_matches_from_votes     the greedy half (:351-384) on a given matrix: the accepted (ref, tgt) index pairs in acceptance order,
 *                             the first `cap` of them written, *n_out = how many there are; no context
 *   ab_triangle_votes_device  the GPU matcher registration runs, on given lists: the targets' lists are concatenated in tgt_xy
 *                             (n_tgt[k] stars each), votes_out holds n_targets matrices; the reference table is built once per call;
 *                             grouped = 0 takes the targets one after another (a batch's frame-by-frame form), grouped = 1 in groups
 *                             of up to 8 in the given order (its grouped form), a list of fewer than 4 stars holding its slot as an
 *                             empty one */
AB_API int ab_triangle_votes_host(const double *ref_xy, size_t n_ref, const double *tgt_xy, size_t n_tgt, uint32_t *votes_out);
AB_API int ab_matches_from_votes(size_t n_ref, size_t n_tgt, const uint32_t *votes, size_t *out_ref_idx, size_t *out_tgt_idx, size_t cap,
                                 size_t *n_out);
AB_API int ab_triangle_votes_device(ab_ctx *ctx, const double *ref_xy, size_t n_ref, const double *tgt_xy, const size_t *n_tgt,
                                    size_t n_targets, int grouped, uint32_t *votes_out);

/* ---- a9  core/imaging/stats.rs ------------------------------------------------------------- */
typedef struct { /* ImageStats, types/image.rs:2-10 */
    double min, max, median, mad, sigma, mean;
    uint64_t valid_count;
} ab_image_stats;

/* compute_image_stats (stats.rs:15-23): exact select for <= 4 000 000 px, 65 536-bin
 * histogram refinement above.  Synchronous (returns scalars). */
AB_API int ab_compute_image_stats(ab_ctx *ctx, const ab_plane *img, ab_image_stats *out);
/* compute_image_stats_with_known_range (stats.rs:25-41) */
AB_API int ab_compute_image_stats_with_known_range(ab_ctx *ctx, const ab_plane *img, double known_min,
                                                   double known_max, ab_image_stats *out);
/* build_histogram (stats.rs:378-421): bins u32[bins] on the HOST; range < 1e-10 -> zeros */
AB_API int ab_build_histogram(ab_ctx *ctx, const ab_plane *img, size_t bins, double dmin, double dmax,
                              uint32_t *out_bins_host);
/* pass-2 histogram of the >4M-px path (stats.rs:260-300), exposed for bin-for-bin parity
 * tests and for the multi-GPU all-reduce of row-band partial histograms. */
AB_API int ab_stats_value_hist(ab_ctx *ctx, const ab_plane *img, double gmin, double gmax,
                               uint64_t *hist65536_host, double *out_sum, uint64_t *out_cnt);

/* ---- a10/a11  core/imaging/stf.rs ----------------------------------------------------------- */
typedef struct { double shadow, midtone, highlight; } ab_stf_params;        /* types/image.rs:36-40 */
typedef struct { double target_bg, shadow_k; } ab_auto_stf_config;          /* types/image.rs:52-65 */
/* auto_stf (stf.rs:13-39) -- host scalar maths, kept in the library so callers get one ABI */
AB_API int ab_auto_stf(const ab_image_stats *stats, const ab_auto_stf_config *cfg, ab_stf_params *out);
/* apply_stf -> Vec<u8> (stf.rs:89-102).  Device planes need no alignment beyond their element's: any 4-byte aligned f32 plane and
 * any u8 pointer are accepted, here, in ab_apply_stf_f32 and in ab_auto_stretch_preview (16-byte aligned f32 planes and 4-byte
 * aligned u8 planes take the wide accesses, the rest is read and written pixel by pixel -- the same bytes either way). */
AB_API int ab_apply_stf_u8(ab_ctx *ctx, const ab_plane *img, const ab_stf_params *p, const ab_image_stats *st,
                           uint8_t *out, int32_t out_on_device);
/* apply_stf_f32 (stf.rs:104-120); out may alias img.data (apply_stf_inplace, stf.rs:147-155) */
AB_API int ab_apply_stf_f32(ab_ctx *ctx, const ab_plane *img, const ab_stf_params *p, const ab_image_stats *st,
                            ab_plane_mut *out);

/* auto_stretch_preview (cmd/common.rs:18-22): compute_image_stats -> auto_stf -> apply_stf as ONE asynchronous chain on the
 * device (the percentile bookkeeping between the histogram passes runs in one-workgroup kernels; the STF kernel reads its
 * transform from HBM).  img, out_u8_dev: device.  cfg NULL = AutoStfConfig::default().  out_stats / out_stf (nullable) are
 * fetched with the call's only synchronisation; both NULL keeps it fully asynchronous.  With a communicator, img is this
 * rank's row band of an image of total_rows rows (0 = img->rows) and the statistics are the whole image's. */
AB_API int ab_auto_stretch_preview(ab_ctx *ctx, ab_comm *comm, const ab_plane *img, int64_t total_rows, const ab_auto_stf_config *cfg,
                                   uint8_t *out_u8_dev, ab_image_stats *out_stats, ab_stf_params *out_stf);

/* ---- a14  core/imaging/scnr.rs ----------------------------------------------------------------- */
typedef struct { /* ScnrConfig, types/image.rs:82-100 */
    int32_t method; /* 0 AverageNeutral, 1 MaximumNeutral */
    float amount;
    int32_t preserve_luminance;
} ab_scnr_config;
/* apply_scnr_inplace (scnr.rs:18-53): mutates the three caller-owned planes; mismatched dims or
 * amount < 1e-7 is a silent no-op exactly as in the reference. */
AB_API int ab_apply_scnr_inplace(ab_ctx *ctx, ab_plane_mut *r, ab_plane_mut *g, ab_plane_mut *b,
                                 const ab_scnr_config *cfg);

/* ---- a16  core/compose/channel_blend.rs ------------------------------------------------------------ */
typedef struct { /* BlendWeight, channel_blend.rs:5-11 */
    uint64_t channel_idx;
    double r_weight, g_weight, b_weight;
} ab_blend_weight;
/* blend_channels (channel_blend.rs:13-70): out_c[i] = sum over weights (list order) of ch[idx][i] * w_c,
 * f32 multiply then add; weights whose channel_idx >= n_channels are skipped. */
AB_API int ab_blend_channels(ab_ctx *ctx, const ab_plane *channels, size_t n_channels, const ab_blend_weight *weights,
                             size_t n_weights, ab_plane_mut *r, ab_plane_mut *g, ab_plane_mut *b);

/* ---- a15  core/imaging/curves.rs ----------------------------------------------------------------------- */
typedef struct { double black, gamma, white; } ab_levels_params; /* LevelsParams, curves.rs:4-9 */
/* SplineLut::from_points (curves.rs:69-95): Fritsch-Carlson monotone cubic -> 4096-entry LUT (host maths) */
AB_API int ab_spline_lut_from_points(const double *points_xy, size_t n_points, float *lut4096);
/* apply_curve (curves.rs:186-197): truncating LUT lookup, non-finite or negative -> 0 */
AB_API int ab_apply_curve(ab_ctx *ctx, const ab_plane *img, const float *lut4096_host, ab_plane_mut *out);
/* apply_levels (curves.rs:31-52): clamp((v-black)/(white-black))^(1/gamma) in f64 */
AB_API int ab_apply_levels(ab_ctx *ctx, const ab_plane *img, const ab_levels_params *p, ab_plane_mut *out);

/* ---- a19  core/imaging/stretch.rs:10-45 ------------------------------------------------------------------ */
AB_API int ab_arcsinh_stretch_with_stats(ab_ctx *ctx, const ab_plane *img, float dmin, float dmax, float factor,
                                         float gamma, ab_plane_mut *out);

/* ---- helpers of a13/a17/a18: luminance (masked_stretch.rs:143-154), WB scale (cmd/compose/color.rs:28-40) */
AB_API int ab_luminance(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, ab_plane_mut *out);
AB_API int ab_scale(ab_ctx *ctx, const ab_plane *img, float factor, ab_plane_mut *out);

/* ---- a20  core/stacking/calibration.rs ---------------------------------------------------------------------- */
/* calibrate_image (calibration.rs:47-82): (raw - bias - dark*ratio) / flat (flat finite, |f| > 1e-4), clamped
 * at 0; any of bias/dark/flat may be NULL. */
AB_API int ab_calibrate_image(ab_ctx *ctx, const ab_plane *raw, const ab_plane *bias, const ab_plane *dark,
                              const ab_plane *flat, float dark_exposure_ratio, ab_plane_mut *out);
/* median_combine_row_major (calibration.rs:84-125), the per-pixel combine of create_master_{bias,dark,flat}:
 * element [len/2] of the finite samples (upper median), 0 if none.  Any n >= 1 (as ab_stack_sigma_clip). */
AB_API int ab_median_combine(ab_ctx *ctx, const ab_plane *planes, size_t n, ab_plane_mut *out);

/* ---- a12  core/imaging/background.rs ---------------------------------------------------------------------------- */
typedef struct { /* BackgroundConfig, background.rs:14-33 (defaults 8, 3, 2.5, 3, Subtract) */
    size_t grid_size, poly_degree;
    float sigma_clip;
    size_t iterations;
    int mode; /* CorrectionMode: 0 Subtract, 1 Divide */
} ab_background_config;
typedef struct { /* BackgroundResult's scalars (:35-42) + the fitted coefficients */
    size_t sample_count;
    double rms_residual;
    double coeffs[21];
} ab_background_info;
/* extract_background(image, config) (background.rs:55-116): grid of cell medians clipped against the global
 * median / MAD -> polynomial surface (degree <= 5) by ridge least squares -> model and corrected image.
 * out_model may be NULL.  Error strings follow the reference ("Image too small for grid_size=..",
 * "Not enough background samples (..) for polynomial degree ..", "Failed to solve polynomial fit: ..."). */
AB_API int ab_extract_background(ab_ctx *ctx, const ab_plane *img, const ab_background_config *cfg, ab_plane_mut *out_model,
                                 ab_plane_mut *out_corrected, ab_background_info *info);

/* ---- a13  core/imaging/star_mask.rs, masked_stretch.rs --------------------------------------------------------- */
typedef struct { /* StarMaskConfig, star_mask.rs:6-30 (defaults 2.5, 4.0, 5.0, 1.5, 30.0, false, 0.85) */
    double growth_factor, softness, detection_sigma, min_fwhm, max_fwhm;
    int luminance_protect;
    double luminance_ceiling;
} ab_star_mask_config;
typedef struct { size_t stars_masked; double coverage_fraction; } ab_star_mask_info; /* StarMaskResult scalars, :32-37 */
/* generate_star_mask (star_mask.rs:38-44) = detect_stars(image, detection_sigma) + the painter below */
AB_API int ab_generate_star_mask(ab_ctx *ctx, const ab_plane *img, const ab_star_mask_config *cfg, ab_plane_mut *out_mask,
                                 ab_star_mask_info *info);
/* generate_star_mask_from_detection (star_mask.rs:46-138): stars with min_fwhm <= fwhm <= max_fwhm paint a disc of
 * radius fwhm * growth_factor plus a smoothstep skirt `softness` wide (max-combined); optional luminance protection
 * above luminance_ceiling; coverage = fraction of mask > 0.01.  Only x, y, fwhm of each star are read. */
AB_API int ab_generate_star_mask_from_stars(ab_ctx *ctx, const ab_plane *img, const ab_detected_star *stars, size_t n_stars,
                                            const ab_star_mask_config *cfg, ab_plane_mut *out_mask, ab_star_mask_info *info);
typedef struct { /* MaskedStretchConfig, masked_stretch.rs:7-32 (defaults 10, 0.25, 2.5, 4.0, true, 0.85, 0.85, 1e-5) */
    size_t iterations;
    double target_background, mask_growth, mask_softness;
    int luminance_protect;
    double luminance_ceiling, protection_amount, convergence_threshold;
} ab_masked_stretch_config;
typedef struct { /* MaskedStretchResult scalars, masked_stretch.rs:34-42 */
    size_t iterations_run;
    double final_background;
    size_t stars_masked;
    double mask_coverage;
    int converged;
} ab_masked_stretch_result;
/* masked_stretch (masked_stretch.rs:44-58): star mask from the image itself, then the loop below */
AB_API int ab_masked_stretch(ab_ctx *ctx, const ab_plane *img, const ab_masked_stretch_config *cfg, ab_plane_mut *out,
                             ab_masked_stretch_result *res);
/* masked_stretch_with_mask (:60-118): normalise to [0,1]; up to `iterations` times: bg = [len/2] element of the
 * unmasked (mask < 0.5) positive pixels, stop at target / stagnation, else blend the MTF-stretched image in with
 * weight 1 - mask * protection; clamp.  mask_info (nullable) is echoed into res (stars_masked, mask_coverage). */
AB_API int ab_masked_stretch_with_mask(ab_ctx *ctx, const ab_plane *img, const ab_plane *mask,
                                       const ab_star_mask_info *mask_info, const ab_masked_stretch_config *cfg,
                                       ab_plane_mut *out, ab_masked_stretch_result *res);
/* masked_stretch_rgb_shared (:155-193): one mask from the luminance (:120-153), applied to r, g, b; res3[0..3] */
AB_API int ab_masked_stretch_rgb_shared(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b,
                                        const ab_masked_stretch_config *cfg, ab_plane_mut *out_r, ab_plane_mut *out_g,
                                        ab_plane_mut *out_b, ab_masked_stretch_result *res3, ab_star_mask_info *shared);

/* ---- a17  core/compose/rgb.rs, white_balance.rs, core/imaging/resample.rs ----------------------------------------- */
/* resample_image(image, target_rows, target_cols) (resample.rs:25-61): bicubic resize to out's dims */
AB_API int ab_resample_image(ab_ctx *ctx, const ab_plane *src, ab_plane_mut *out);
/* select_wb_reference (white_balance.rs:3-20): multipliers (r, g, b) against the most stable channel (host maths) */
AB_API int ab_select_wb_reference(const ab_image_stats *sr, const ab_image_stats *sg, const ab_image_stats *sb,
                                  double out_rgb[3]);
typedef struct { /* RgbComposeConfig, types/compose.rs:47-75 */
    int32_t white_balance;      /* WhiteBalance: 0 Auto, 1 Manual(wb_manual), 2 None */
    double wb_manual[3];
    int32_t auto_stretch, linked_stf;
    int32_t has_stf[3];         /* Option<StfParams> stf_r / stf_g / stf_b (used when !auto_stretch) */
    ab_stf_params stf[3];
    int32_t align, align_method; /* AlignMethod: 0 PhaseCorrelation, 1 Affine */
    int32_t has_scnr;           /* Option<ScnrConfig> */
    ab_scnr_config scnr;
    int32_t num_threads;        /* rayon::current_num_threads() of the host being replaced (affine RANSAC seeds) */
} ab_rgb_compose_config;
typedef struct { /* scalars of ProcessedRgb, rgb.rs:18-40 */
    uint64_t rows, cols;
    ab_stf_params stf[3];
    double chan_stats[3][4];    /* ChannelStats {min, max, median, mean} per channel, before white balance */
    double offset_g[2], offset_b[2]; /* (dy, dx) resp. (ty, tx) */
    int32_t scnr_applied, resampled;
    ab_image_stats stats_wb[3]; /* stats after white balance (the ones the STF is applied with) */
} ab_processed_rgb_info;
/* process_rgb(r?, g?, b?, &config) (rgb.rs:209-323): harmonise dims (bicubic up to the largest), synthesise a missing
 * channel, align G and B to the first present channel, white balance, (linked) auto-STF, compose-local STF
 * (rgb.rs:191-207), SCNR.  Absent channels are NULL; at least two must be present.  out_* (and the nullable
 * pre_* = white-balanced, pre-stretch copies) must have the largest channel's dims. */
AB_API int ab_process_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b,
                          const ab_rgb_compose_config *cfg, ab_plane_mut *out_r, ab_plane_mut *out_g, ab_plane_mut *out_b,
                          ab_plane_mut *pre_r, ab_plane_mut *pre_g, ab_plane_mut *pre_b, ab_processed_rgb_info *info);

/* ---- a18  core/astrometry/spcc.rs -------------------------------------------------------------------------------- */
typedef struct { /* SpccConfig, spcc.rs:9-28 (defaults 20.0, 200, 0.90, AverageSpiral; catalog = BuiltinBpRp) */
    double min_snr;
    uint64_t max_stars;
    double saturation_limit;
    int32_t white_reference; /* WhiteReference: 0 AverageSpiral, 1 G2V, 2 Photopic, 3 Custom(custom) */
    double custom[3];
} ab_spcc_config;
typedef struct { /* the numbers of SpccResult, spcc.rs:45-56 */
    double r_factor, g_factor, b_factor;
    uint64_t stars_matched, stars_total;
    double avg_color_index;
} ab_spcc_result;
/* spcc_calibrate_rgb(r, g, b, header, config) (spcc.rs:73-183) with the built-in Bp-Rp catalogue.  The header's
 * WCS enters that path only through its pixel scale (the catalogue is synthesised from the detections' own
 * sky positions, :257-273, so the cross-match is the identity whenever pixel_scale > 0): the caller passes
 * WcsTransform::pixel_scale_arcsec().  Err strings as the reference ("Only N stars passed quality filters
 * (need 5+). Try lowering min_snr." / "Only N stars cross-matched (need 3+). Check WCS solution quality."). */
AB_API int ab_spcc_calibrate_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b,
                                 double pixel_scale_arcsec, const ab_spcc_config *cfg, ab_spcc_result *res);
/* the part after detection (spcc.rs:90-183) on a given detect_stars() result and luminance maximum */
AB_API int ab_spcc_from_detection(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b,
                                  const ab_detected_star *stars, size_t n_stars, double lum_max, double pixel_scale_arcsec,
                                  const ab_spcc_config *cfg, ab_spcc_result *res);
/* white_reference_rgb (spcc.rs:245-255); host maths */
AB_API int ab_spcc_white_reference_rgb(int32_t kind, const double custom[3], double out_rgb[3]);

/* ---- caller-side helpers of a17 / a20 ---------------------------------------------------------------------------- */
/* apply_lrgb(l, &mut r, &mut g, &mut b, lightness_weight, chrominance_weight) (core/compose/lrgb.rs:4-45); mutates
 * r, g, b; Err "L dimensions .. do not match RGB (..)" on mismatched dims */
AB_API int ab_apply_lrgb(ab_ctx *ctx, const ab_plane *l, ab_plane_mut *r, ab_plane_mut *g, ab_plane_mut *b,
                         float lightness_weight, float chrominance_weight);
/* lrgb.rs:47-64 synthesize_luminance (= spcc.rs:185-196): r*0.2126 + g*0.7152 + b*0.0722, NO finite guard
 * (ab_luminance is the guarded masked_stretch.rs variant) */
AB_API int ab_synthesize_luminance(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, ab_plane_mut *out);
/* compute_linked_stf_with_stats (cmd/helpers.rs:185-202): auto_stf of the channel-averaged statistics (host maths);
 * out_combined nullable */
AB_API int ab_compute_linked_stf(const ab_image_stats *sr, const ab_image_stats *sg, const ab_image_stats *sb,
                                 const ab_auto_stf_config *cfg, ab_stf_params *out_stf, ab_image_stats *out_combined);
/* calibrate_channel (cmd/compose/color.rs:21-49): out = orig * factor, statistics of the result (known-range fast
 * path above 4 000 000 px) */
AB_API int ab_calibrate_channel(ab_ctx *ctx, const ab_plane *orig, float factor, const ab_image_stats *orig_stats,
                                ab_plane_mut *out, ab_image_stats *out_stats);
/* create_master_bias / _dark / _flat on in-memory frames (calibration.rs:127-255): kind 0 bias = median combine;
 * 1 dark = median of (frame - bias?); 2 flat = median of (frame - bias? - dark?), normalised to mean 1 over its
 * finite positive pixels (others -> 1.0).  Err strings as the reference ("No bias frames provided", "Dimension
 * mismatch: expected (..), got (..)").  Any n_frames >= 1. */
AB_API int ab_create_master(ab_ctx *ctx, int32_t kind, const ab_plane *frames, size_t n_frames, const ab_plane *master_bias,
                            const ab_plane *master_dark, ab_plane_mut *out);

/* ---- the compose wizard's crop step, cmd/compose/crop.rs (crop_channels_cmd: between align_channels_cmd and blend_channels_cmd) -- */
/* Boxes are half open: rows [top, bottom), columns [left, right).  Inputs may be host or device planes of any float-aligned
 * address and any dims with rows * cols < 2^31; a device plane is never downloaded, only the boxes (4 x u32 per plane) cross to the
 * host.  Nothing here rounds: every result is the reference's, bit for bit. */
typedef struct { uint64_t top, bottom, left, right; } ab_crop_box;
/* detect_valid_region(arr, threshold) (crop.rs:14-62).  A pixel is valid iff |v| > threshold, strictly and in f32 (:20): a NaN
 * pixel never is, +-inf are (unless the threshold is +inf), -0.0 only for a negative threshold; a NaN threshold makes nothing
 * valid, a negative one every non-NaN pixel.  top = the first row holding a valid pixel (rows if none), bottom = the last such
 * row + 1 (0 if none), left / right the same over the columns: a plane without a valid pixel gives (rows, 0, cols, 0), which is
 * what the reference's four loops leave.  Synchronous (returns scalars). */
AB_API int ab_detect_valid_region(ab_ctx *ctx, const ab_plane *img, float threshold, ab_crop_box *out);
/* the loop crop.rs:109-116 over n planes, each measured with its own dims, up to 16 planes per launch: out_each[n] (nullable) and
 * the running (max top, min bottom, max left, min right) out_common (nullable; (0, UINT64_MAX, 0, UINT64_MAX) for n = 0, :104-107).
 * Synchronous. */
AB_API int ab_detect_valid_regions(ab_ctx *ctx, const ab_plane *imgs, size_t n, float threshold, ab_crop_box *out_each,
                                   ab_crop_box *out_common);
/* crop_array(arr, top, bottom, left, right) (crop.rs:64-71): the box is clamped to src's dims as the reference clamps it,
 * t = min(top, rows), b = max(min(bottom, rows), t), l = min(left, cols), r = max(min(right, cols), l); out must be
 * (b - t) x (r - l) and dense.  A zero-area window is legal: nothing is written (out->data may then be NULL).  A host source is
 * staged as the window's rows only.  Asynchronous on the context's stream for device planes. */
AB_API int ab_crop_array(ab_ctx *ctx, const ab_plane *src, const ab_crop_box *box, ab_plane_mut *out);
typedef struct { /* crop_channels_cmd's arguments (crop.rs:77-81) + the threshold */
    int32_t auto_detect;               /* auto_detect.unwrap_or(true) (:101) */
    uint64_t top, bottom, left, right; /* manual MARGINS: pixels removed from each side (:123-126) */
    float threshold;                   /* AUTO_THRESHOLD (:12) */
} ab_crop_config;
AB_API void ab_crop_config_default(ab_crop_config *cfg); /* auto_detect 1, margins 0, threshold 1e-6f */
typedef struct {
    ab_crop_box crop_box;        /* (crop_top, crop_bottom, crop_left, crop_right), crop.rs:103-126 */
    uint64_t out_rows, out_cols; /* plane 0's cropped dims, crop.rs:170-175 (the JSON's "dimensions" is [out_cols, out_rows]) */
    uint64_t actual_top, actual_bottom, actual_left, actual_right; /* crop.rs:179-183: crop_box.top, rows0 - crop_box.bottom, crop_box.left,
                                                                      cols0 - crop_box.right, the subtractions saturating */
    int32_t auto_detected;
} ab_crop_plan;
/* crop.rs:92-126: decide the box.  Auto mode intersects the planes' valid regions (ab_detect_valid_regions with cfg->threshold):
 * AB_ERR_INVALID "Auto-crop found no valid overlapping region" when min_bottom <= max_top || min_right <= max_left (:118-120).
 * Manual mode: (top, rows0.saturating_sub(bottom), left, cols0.saturating_sub(right)) with plane 0's dims and no emptiness check.
 * n = 0: AB_ERR_INVALID "No paths provided for cropping" (:92-94).  out_dims (nullable) [2 n] = (rows, cols) of each plane's
 * cropped output (crop_array clamps per plane: planes of different dims give outputs of different dims), so that the caller can
 * allocate.  Synchronous in auto mode; host arithmetic in manual mode. */
AB_API int ab_crop_channels_plan(ab_ctx *ctx, const ab_plane *imgs, size_t n, const ab_crop_config *cfg, ab_crop_plan *plan,
                                 uint64_t *out_dims);
/* crop.rs:133-168 without the file and cache traffic: outs[i] = crop_array(imgs[i], plan->crop_box), up to 16 planes per launch;
 * stats (nullable, n entries) = compute_image_stats(&cropped) through ab_compute_image_stats' own engine (exact select at
 * <= 4 000 000 cropped pixels, the histogram route above), ImageStats::default() -- all zero -- for a zero-area plane, without a
 * launch.  With stats = NULL and device planes the call is asynchronous on the context's stream. */
AB_API int ab_crop_channels(ab_ctx *ctx, const ab_plane *imgs, size_t n, const ab_crop_plan *plan, ab_plane_mut *outs,
                            ab_image_stats *stats);

/* ---- FITS pixel codecs, infra/fits/reader.rs + writer.rs ------------------------------------------- */
/* decode_pixels(data, bitpix, bscale, bzero) (reader.rs:42-101): big-endian BITPIX 8 / 16 / 32 / -32 / -64 -> f32,
 * `v as f64 * bscale + bzero` unless is_identity_scaling (:36-39).  `data` = the HDU's data unit as it sits in the
 * file (host or device); out must hold nbytes / bytes-per-pixel pixels. */
AB_API int ab_fits_decode_pixels(ab_ctx *ctx, const void *data, size_t nbytes, int32_t data_on_device, int64_t bitpix, double bscale,
                                 double bzero, ab_plane_mut *out);
/* compute_bzero_bscale (writer.rs:143-159): i16 scaling from the finite min / max */
AB_API int ab_fits_compute_bzero_bscale(ab_ctx *ctx, const ab_plane *img, double *bzero, double *bscale);
/* write_f32 / i16 / f64_slice_as_be (writer.rs:82-135): the data unit for BITPIX -32, 16 (with bzero / bscale) or -64 */
AB_API int ab_fits_encode_pixels(ab_ctx *ctx, const ab_plane *img, int32_t bitpix, double bzero, double bscale, void *out,
                                 int32_t out_on_device);
/* stack_images' per-pixel loop (combine.rs:160-182) fed straight from n device-resident data units (BITPIX -32 or 16,
 * all rows x cols of `out`): decode_pixels is fused into the kernel's gather, so BITPIX 16 stacks read 2 bytes per
 * sample from HBM and no decoded copy exists.  Result = ab_fits_decode_pixels + ab_stack_sigma_clip, bit for bit.
 * n must be 8, 16, 32 or 64.  Every plane must hold rows x cols samples and be readable up to the next 4-byte boundary
 * (BITPIX 16 with an odd pixel count: the last sample is fetched inside an aligned dword; a FITS data unit is padded to
 * 2880 bytes, so a whole data unit always qualifies). */
AB_API int ab_stack_sigma_clip_raw(ab_ctx *ctx, const void *const *raw_planes_dev, size_t n, int64_t bitpix, double bscale,
                                   double bzero, const ab_stack_config *cfg, ab_plane_mut *out, uint64_t *out_rejected);

/* ---- batch calibration pipeline, core/imaging/calibration_pipeline.rs ------------------------------- */
typedef struct { /* BatchStackConfig (:20-37); defaults 2.5, 3.0, 5, true */
    float sigma_low, sigma_high;
    uint64_t max_iterations;
    int32_t normalize_before_stack; /* bool */
} ab_batch_stack_config;
typedef struct { /* CalibrationMasters (:6-11); NULL = None.  A master whose rows * cols differs from the light's is skipped (:87-89) */
    const ab_plane *bias, *dark, *flat;
} ab_calibration_masters;
typedef struct { /* BatchChannelStats (:65-72) without the label; lights_after_rejection is the rejection_counts array */
    uint64_t lights_input;
    double mean, stddev;
} ab_batch_channel_stats;
typedef struct { /* ChannelInput (:13-17) + where the channel's per-frame rejection counts go (n_lights entries, nullable) */
    const char *label;
    const ab_plane *lights;
    size_t n_lights;
    uint64_t *rejection_counts;
} ab_batch_channel_input;
AB_API void ab_batch_stack_config_default(ab_batch_stack_config *cfg);
/* calibrate_light (:74-118): ((light - bias) - dark) / flat where flat is finite and |flat| > 1e-4, negatives -> 0 */
AB_API int ab_calibrate_light(ab_ctx *ctx, const ab_plane *light, const ab_calibration_masters *masters, ab_plane_mut *out);
/* normalize_frames (:309-319): frame * (1 / (mean as f32)) where the f64 mean is > 0, else a copy.  outs[i] may alias frames[i].
 * The f64 mean is a fixed-shape tree sum (the reference's is sequential): equal to ~1e-13 relative. */
AB_API int ab_normalize_frames(ab_ctx *ctx, const ab_plane *frames, size_t n, ab_plane_mut *outs);
/* sigma_clipped_mean_stack (:321-378): per pixel, up to max_iterations passes of { median, MAD -> sigma = 1.4826 MAD (f32);
 * stop if sigma < 1e-10; keep -sigma_low < (v - median) / sigma < sigma_high }, NaN samples included and rejected by the
 * first pass; result = f32 sum of the survivors in frame order / count (0 if none).  rejection_counts[f] (nullable) =
 * samples of frame f rejected over the whole image.  Any n >= 1 frames of identical dims (65 .. 2048: one wave per
 * pixel instead of one lane, ~40x slower per sample; beyond: one workgroup per pixel, samples in a scratch segment).  Bit-exact. */
AB_API int ab_sigma_clipped_mean_stack(ab_ctx *ctx, const ab_plane *frames, size_t n, const ab_batch_stack_config *config, ab_plane_mut *out,
                                       uint64_t *rejection_counts);
/* one channel of run_batch_pipeline (:157-190): calibrate_light on every light, normalize_frames (if configured),
 * sigma_clipped_mean_stack, mean / stddev of the master.  Fused: the lights are read twice (frame means, stack) and no
 * calibrated or normalised frame is ever written; the stacked samples are bit-identical to the reference's. */
AB_API int ab_run_batch_channel(ab_ctx *ctx, const ab_plane *lights, size_t n, const ab_calibration_masters *masters,
                                const ab_batch_stack_config *config, ab_plane_mut *out_master, uint64_t *rejection_counts,
                                ab_batch_channel_stats *stats);
/* compose_rgb_from_masters (:201-267) for the R, G, B (and optional L) masters: normalize_channel (:291-307) on the common
 * top-left crop, apply_luminance (:269-289) when all four share their dims; out_rgb = rows x cols x 3 interleaved f32
 * (Array3), host or device.  out_rgb == NULL only reports the dims. */
AB_API int ab_compose_rgb_from_masters(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_plane *l,
                                       float *out_rgb, int32_t out_on_device, int64_t *out_rows, int64_t *out_cols);
/* run_batch_pipeline (:120-199): validation with the reference's messages, every channel through ab_run_batch_channel into
 * out_masters[c] (dims of the channel's lights), stats[c] (nullable), then compose_rgb_from_masters when channels labelled
 * R, G and B exist (ASCII case-insensitive): out_rgb must then hold min-rows x min-cols x 3 floats; *rgb_rows = 0 = None. */
AB_API int ab_run_batch_pipeline(ab_ctx *ctx, const ab_batch_channel_input *channels, size_t n_channels,
                                 const ab_calibration_masters *masters, const ab_batch_stack_config *config, ab_plane_mut *out_masters,
                                 ab_batch_channel_stats *stats, float *out_rgb, int32_t rgb_on_device, int64_t *rgb_rows,
                                 int64_t *rgb_cols);

/* ---- subframe scoring, core/analysis/subframe.rs -------------------------------------------------- */
typedef struct { /* SubframeWeightConfig (subframe.rs:24-49) */
    double fwhm_weight, eccentricity_weight, snr_weight, noise_weight, max_fwhm, max_eccentricity, min_snr;
    uint64_t min_stars;
} ab_subframe_weight_config;
typedef struct { /* the numbers of SubframeMetrics (subframe.rs:9-22); file_path stays with the caller */
    uint64_t star_count;
    double median_fwhm, median_eccentricity, median_snr, background_median, background_sigma, noise_ratio, weight;
    int32_t accepted;
} ab_subframe_metrics;
AB_API void ab_subframe_weight_config_default(ab_subframe_weight_config *cfg);      /* Default, :36-49 */
/* analyze_subframe(image, _, config) (subframe.rs:51-121): detect_stars(image, 4.0), medians of the finite fwhm /
 * eccentricity / snr, noise_ratio, compute_weight (:123-146) and the accept flags.  config == NULL -> defaults. */
AB_API int ab_analyze_subframe(ab_ctx *ctx, const ab_plane *image, const ab_subframe_weight_config *config, ab_subframe_metrics *out);
/* the caller's loop over a night's subframes: n frames scored frame-parallel on the context's worker streams */
AB_API int ab_analyze_subframes(ab_ctx *ctx, const ab_plane *images, size_t n, const ab_subframe_weight_config *config,
                                ab_subframe_metrics *out);
AB_API void ab_normalize_subframe_weights(ab_subframe_metrics *metrics, size_t n);  /* normalize_weights, :148-159 */

/* ---- the weighted, normalised sigma-clip stack: what consumes the subframe scores ------------------------------------ */
/* The reference has no weighted stack (core/stacking/combine.rs:14-92 ends in an unweighted mean of the survivors); this definition
 * is the library's own, built so that the rejection is exactly the reference's and only the final mean changes.
 *   Active frames.  A frame takes part iff weight > 0.  A frame of weight 0 takes part in nothing -- not in the clipping, not in the
 *     mean, not in the rejected count -- and its plane is never read.  A negative or non-finite weight, a non-finite scale or offset
 *     -> AB_ERR_INVALID; no active frame -> AB_ERR_INVALID "No images to stack"; more than AB_STACK_MAX_ACTIVE (64) active frames ->
 *     AB_ERR_UNSUPPORTED (a pixel's samples live in one lane's registers, twice; the engines for deeper stacks do not hand out the
 *     surviving interval yet).  Any number of frames of weight 0 may sit between the active ones.
 *   Samples.  s_f = p_f * scale_f + offset_f, an f32 multiply and then an f32 add (never fused); a frame with scale == 1 and
 *     offset == 0 is read as it is (-0.0 stays -0.0).  Finiteness is judged on s_f: a sample the normalisation sends to +-inf is
 *     dropped like a NaN (combine.rs:170-175).
 *   Rejection.  sigma_clip_combine on the finite s_f of the active frames, with the library's documented ascending-order f64 sums in
 *     iterations >= 1 and the correctly rounded sqrt: the arithmetic of ab_stack_sigma_clip under AB_STACK_EXACT=1.  The survivors
 *     are an interval of the sorted samples and equal values share their fate: frame f survives iff s_f is finite and lies between
 *     the smallest and the largest surviving value.
 *   Result per pixel, m = number of finite samples.  m = 0: image 0.0, weight sum 0.  m = 1: that sample, that frame's weight.
 *     Nothing survives: the reference's fallback (last_center if finite, else 0.0; combine.rs:85-88), weight sum 0.  Otherwise
 *     image = (float)(sum w_f (double)s_f / sum w_f) over the surviving frames, both sums in f64 in ascending FRAME INDEX order, one
 *     multiply and one add per frame, each rounded; weight plane = (float)sum w_f.  *out_rejected = the reference's count
 *     (combine.rs:76-78) summed over the pixels.
 * With all weights 1, scale 1 and offset 0 this is ab_stack_sigma_clip under AB_STACK_EXACT=1 but for the order of the final sum
 * (frame order, not ascending value): identical whenever that sum is exact in f64.  cfg->align is ignored.
 * planes: host or device, each at least out->rows x out->cols, read with its own row stride (the top-left crop, as
 * ab_stack_sigma_clip).  out, out_weight (nullable; same dims as out): host or device; a device output may not overlap a device
 * input or the other output; the output and every active plane hold fewer than 2^31 pixels (AB_ERR_INVALID).  The call records the events behind ab_stack_last_kernel_ms, and ab_stack_last_rejected answers after
 * it; out_rejected == NULL keeps it asynchronous on the context's stream (device planes). */
#define AB_STACK_MAX_ACTIVE 64
typedef struct {
    double weight; /* >= 0; 0 = the frame takes no part */
    float scale;
    float offset;
} ab_stack_frame_param;
AB_API int ab_stack_weighted(ab_ctx *ctx, const ab_plane *planes, const ab_stack_frame_param *params, size_t n,
                             const ab_stack_config *cfg, ab_plane_mut *out, ab_plane_mut *out_weight, uint64_t *out_rejected);
/* The parameters of ab_stack_weighted from the scores of ab_analyze_subframes (+ ab_normalize_subframe_weights).  Host-only
 * arithmetic: no context, usable without a GPU.
 *   weight_f = metrics[f].weight when metrics[f].accepted is set and the weight is finite and > 0, else 0.
 *   The reference frame is the active frame of the largest weight, the lowest index on a tie (*out_reference, nullable).
 *   AB_STACK_NORM_NONE: scale 1, offset 0; the backgrounds are not looked at.
 *   AB_STACK_NORM_ADDITIVE: scale 1, offset = (float)(bg_ref - bg_f), bg = background_median.
 *   AB_STACK_NORM_MULTIPLICATIVE: scale = (float)(bg_ref / bg_f), offset 0.
 *   In the two normalising modes an active frame whose background_median is not finite (multiplicative: or <= 0) gets weight 0.
 * AB_ERR_INVALID: a NULL metrics or out, an unknown mode, no active frame, or a reference frame whose own background fails that test. */
typedef enum { AB_STACK_NORM_NONE = 0, AB_STACK_NORM_ADDITIVE = 1, AB_STACK_NORM_MULTIPLICATIVE = 2 } ab_stack_norm;
AB_API int ab_stack_params_from_metrics(const ab_subframe_metrics *metrics, size_t n, int32_t normalize, ab_stack_frame_param *out,
                                        size_t *out_reference);

/* ---- preview / tile renderers up to the PNG encoder ---------------------------------------------- */
/* preview size for max_dim (cmd/helpers.rs:283-290, infra/ipc.rs:100-103): the plane's own dims when both fit */
AB_API int ab_preview_dims(int64_t rows, int64_t cols, int64_t max_dim, int64_t *out_rows, int64_t *out_cols);
/* render_rgb_preview (helpers.rs:204-262; == render_rgb, infra/render/rgb.rs:7-34, when the planes fit max_dim) with
 * stf == NULL: nearest-neighbour pick, (v.clamp(0, 1) * 255.0) as u8.  render_rgb_preview_with_stf (:264-322) with
 * stf / stats = 3 entries (R, G, B): make_stf_u8_fn(stf[c], stats[c]) (core/imaging/stf.rs:122-145) per channel.
 * out_rgb = preview_rows x preview_cols x 3 interleaved bytes (host or device), i.e. the encoder's input. */
AB_API int ab_render_rgb_preview(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, int64_t max_dim,
                                 const ab_stf_params *stf, const ab_image_stats *stats, uint8_t *out_rgb, int32_t out_on_device);
/* encode_with_header (infra/ipc.rs:93-103; max_dim == 0) / encode_with_header_downsampled (:105-148): 16-byte header
 * (u32 width, u32 height, f32 data_min, f32 data_max, little-endian) + cleaned f32 pixels (non-finite -> 0).
 * out holds 16 + 4 * preview_rows * preview_cols bytes; *out_len (nullable) = the length written.
 * The SIGN of a data_min / data_max that is zero is unspecified: on a plane that holds both +0.0 and -0.0 the reference keeps
 * the first zero of each 65536-pixel chunk and merges the chunks with f32::min / f32::max, which fix no sign either.  Compare
 * those two header fields by value; the pixel bytes keep every -0.0 as it is. */
AB_API int ab_ipc_encode_with_header(ab_ctx *ctx, const ab_plane *img, int64_t max_dim, void *out, int32_t out_on_device, size_t *out_len);
#define AB_MAX_TILE_LEVELS 32
typedef struct { /* TileLevel (infra/render/tiles.rs:21-29) + where the level's tiles start in the packed buffer */
    uint64_t level, width, height, cols, rows;
    double scale_factor;
    uint64_t offset;
} ab_tile_level;
AB_API int ab_tile_compute_num_levels(int64_t width, int64_t height, int64_t tile_size);   /* tiles.rs:137-147; 0 = bad args */
/* the pyramid's levels (level 0 = coarsest, tiles.rs:203-246) and the packed size: per level, tiles in (tile_y, tile_x)
 * order, each tile_size x tile_size x channels bytes.  levels holds AB_MAX_TILE_LEVELS entries. */
AB_API int ab_tile_pyramid_layout(int64_t rows, int64_t cols, int64_t tile_size, int32_t channels, ab_tile_level *levels,
                                  int32_t *num_levels, size_t *total_bytes);
AB_API int ab_tile_downsample_2x(ab_ctx *ctx, const ab_plane *img, ab_plane_mut *out);      /* downsample_2x, tiles.rs:41-70 */
/* percentile_bounds (tiles.rs:149-178): order statistics of the finite pixels > 1e-7; finite min / max if there are none.
 * The ranks are `((n as f64 * pct) as usize).min(n - 1)`, a saturating conversion: a negative or NaN pct selects the smallest
 * valid pixel, a pct past 1 the largest. */
AB_API int ab_tile_percentile_bounds(ab_ctx *ctx, const ab_plane *img, double low_pct, double high_pct, float *lo, float *hi);
/* generate_tile_pyramid (tiles.rs:180-255) up to the encoder: percentile_bounds(0.001, 0.999), the 2x chain, and every
 * render_tile buffer (:72-113) into `tiles` (layout above, channels = 1; zero outside the image). */
AB_API int ab_generate_tile_pyramid(ab_ctx *ctx, const ab_plane *normalized, int64_t tile_size, uint8_t *tiles, int32_t tiles_on_device,
                                    ab_tile_level *levels, int32_t *num_levels, float *global_min, float *global_max);
/* generate_tile_pyramid_rgb / _rgb_stf (tiles.rs:363-481): stf == NULL -> render_tile_rgb (:257-298, rounded), else
 * render_tile_rgb_stf (:300-341) with make_stf_u8_fn(stf[c], stats[c]); channels = 3 */
AB_API int ab_generate_tile_pyramid_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, int64_t tile_size,
                                        const ab_stf_params *stf, const ab_image_stats *stats, uint8_t *tiles, int32_t tiles_on_device,
                                        ab_tile_level *levels, int32_t *num_levels);

/* ---- Richardson-Lucy deconvolution, core/analysis/deconvolution.rs (deconvolve_rl_cmd) ------------------------------- */
typedef struct { /* RLConfig (types/stacking.rs) without the PSF's own size / sigma: the PSF is passed as a plane */
    size_t iterations;
    double regularization;
    int32_t deringing; /* bool */
    float deringing_threshold;
} ab_rl_config;
typedef struct { /* RLResult's scalars; elapsed_ms is the host's to measure */
    size_t iterations_run;
    double convergence;
} ab_rl_result;
/* generate_gaussian_psf (deconvolution.rs:12-33): size x size f32, row-major, exp = libm expf in the reference's order and
 * f32 running sum (bit-identical to the reference on glibc).  Host-only; size 0 -> AB_ERR_INVALID. */
AB_API int ab_generate_gaussian_psf(size_t size, float sigma, float *out_host);
/* richardson_lucy (:141-221) with apply_deringing (:223-245); img, psf and out host or device, out = img's dims and not
 * overlapping it; an empty PSF -> AB_ERR_INVALID.  The reference's FFT convolution over the padded power-of-two buffer equals
 * the linear convolution with a zero boundary on the kept window, computed here directly in f32 (not bit-identical to the
 * reference's FFTs: ~1e-5 relative, as its own f32 FFT against f64).  The iteration stops early once convergence < 1e-6 after
 * >= 3 iterations: near that threshold a stop may differ from the reference's by one iteration.  iterations = 0 returns
 * the image with iterations_run = 0 and convergence = DBL_MAX.  A NaN / inf pixel or PSF tap poisons the whole convolution as
 * in the reference; |x| >= 1e30 (FFT overflow in the reference) is outside the contract.  PSFs up to 63 x 63 take the LDS-tiled
 * kernels, larger ones a plain direct kernel (correct, slower).  Iterations are enqueued in chunks of <= ~25 ms of GPU work:
 * cancellation is seen, and the progress callback ticked ("iteration k/n"), once per chunk. */
AB_API int ab_richardson_lucy(ab_ctx *ctx, const ab_plane *img, const ab_plane *psf, const ab_rl_config *cfg, ab_plane_mut *out,
                              ab_rl_result *res);

/* ---- empirical PSF estimation, core/imaging/psf_estimation.rs (deconvolve_rl_cmd with use_empirical_psf) -------------------- */
typedef struct { /* PsfEstimationConfig (psf_estimation.rs:16-25); Default (:27-39): 30 / 15 / 0.95 / 0.10 / 0.3 / 30 / 0.7 */
    size_t num_stars;
    size_t cutout_radius;
    double saturation_threshold;
    double min_peak_fraction;
    double max_ellipticity;
    size_t edge_margin;
    double max_center_distance_fraction;
} ab_psf_estimation_config;
typedef struct { /* StarCandidate (:4-14) */
    double x, y, peak, flux, fwhm, ellipticity, distance_from_center, snr;
} ab_psf_star;
typedef enum { /* estimate_psf's Ok and its three Err strings (:64-66, :86-88, :107-109) */
    AB_PSF_OK = 0,
    AB_PSF_NO_STARS_DETECTED = 1,      /* "No stars detected in image" */
    AB_PSF_NO_STARS_PASSED = 2,        /* "No stars passed quality filters" */
    AB_PSF_NO_CUTOUTS = 3              /* "Failed to extract star cutouts" */
} ab_psf_outcome;
typedef struct { /* PsfResult's scalars (:41-50); the kernel and stars_used are arguments of their own */
    int32_t outcome; /* an ab_psf_outcome; the fields below are meaningful for AB_PSF_OK only (the two counts always) */
    size_t kernel_size; /* 2 * cutout_radius + 1 */
    double average_fwhm, average_ellipticity, spread_pixels;
    size_t stars_used;     /* min(num_stars, stars_filtered): the length of PsfResult.stars_used */
    size_t stars_rejected; /* the reference's candidates.len() - count (:131): filtered stars minus extracted cutouts */
    size_t stars_detected; /* detect_stars_for_psf's list (:62) */
    size_t stars_filtered; /* after the quality filter (:68-84) */
} ab_psf_result;
#define AB_PSF_MAX_CUTOUT_RADIUS 31
AB_API void ab_psf_estimation_config_default(ab_psf_estimation_config *cfg);
/* The quality filter (:68-84), score_star (:509-516), the stable descending sort (:90) and take(num_stars) (:92) over n stars,
 * host-only scalar maths, bit for bit the reference's: out_idx (cap entries) receives the indices of the selected stars in
 * selection order, *out_selected their number (min(num_stars, filtered, cap)), *out_filtered how many passed the filter.
 * max_val = the image's maximum as f64 (LocalStats.max_val), rows / cols its dims.  NULL stars with n > 0, NULL cfg -> AB_ERR_INVALID;
 * out_idx may be NULL when cap = 0. */
AB_API int ab_psf_select_stars(const ab_psf_star *stars, size_t n, const ab_psf_estimation_config *cfg, double max_val, int64_t rows,
                               int64_t cols, size_t *out_idx, size_t cap, size_t *out_selected, size_t *out_filtered);
/* estimate_psf (:52-134) followed by psf_to_kernel (:136-149).  img host or device (a device plane is never downloaded: candidate
 * lists, per-star records and nothing else cross to the host); kernel_out host or device, (2 * cutout_radius + 1)^2 f32 -- a device
 * kernel_out can be handed straight to ab_richardson_lucy; stars_out (nullable when stars_cap = 0) receives the first
 * min(stars_used, stars_cap) entries of PsfResult.stars_used.
 * The reference's three Err returns are RESULTS: the call returns AB_OK, res->outcome names the case and kernel_out is untouched.
 * AB_ERR_INVALID: NULL arguments; rows or cols <= 2 * edge_margin (the reference's `h - margin` loop bounds wrap or are empty);
 * num_stars = 0 (the reference divides 0 / 0); a kernel plane that is not (2 r + 1)^2; 2^31 pixels or more; a non-finite pixel
 * (the reference's behaviour on NaN is an accident of partial_cmp; found by the statistics pass at no extra cost).
 * AB_ERR_UNSUPPORTED: cutout_radius > AB_PSF_MAX_CUTOUT_RADIUS (31: the cutout is kept in LDS as f64).
 * EXACTNESS.  Given the same detection threshold (:198) everything is reproduced bit for bit: every f64 field of every star, the
 * selection order, the f32 kernel and the three scalars -- every f64 accumulation chain is summed in the reference's order (raster
 * order over a window, ascending order over a sorted slice), unfused, with IEEE sqrt and division.  The ONE exception is stddev
 * (:178-180): sum and sum_sq are formed by a fixed parallel reduction tree (identical from run to run), which cannot reproduce the
 * rounding of the reference's sequential sums.  The relative error of either sum is bounded by about n * 2^-53, amplified in var by
 * mean^2 / var; it changes the result only if a pixel lies inside that band around threshold = median + 5 * stddev.  Where the pixels
 * are integer-valued (raw ADU) and sum_sq < 2^53 both sums are exact in any order and the result is bit-identical without
 * qualification.  max_val and the median (the [n / 2] order statistic, negative pixels included) are exact.
 * Not asynchronous: lists and records are read back. */
AB_API int ab_estimate_psf(ab_ctx *ctx, const ab_plane *img, const ab_psf_estimation_config *cfg, ab_plane_mut *kernel_out,
                           ab_psf_star *stars_out, size_t stars_cap, ab_psf_result *res);

/* ---- the synthetic star-field generator, core/synth/{star_field,psf,noise,pipeline}.rs (generate_synth_cmd, generate_synth_stack_cmd) -- */
typedef struct { /* Star (star_field.rs:4-10) */
    double x, y, z, flux, temperature;
} ab_synth_star;
typedef struct { /* FieldConfig (star_field.rs:13-20); Default (:22-33): 2048 x 2048, 500 stars, flux 100 .. 50000, seed 42 */
    uint32_t width, height;
    size_t n_stars;
    double flux_min, flux_max;
    uint64_t seed;
} ab_synth_field_config;
typedef enum { /* FieldType (pipeline.rs:11-21) */
    AB_SYNTH_FIELD_UNIFORM = 0,
    AB_SYNTH_FIELD_KING_CLUSTER = 1,     /* a = core_radius, b = tidal_radius */
    AB_SYNTH_FIELD_EXPONENTIAL_DISK = 2  /* a = scale_length, b = inclination_deg */
} ab_synth_field_kind;
typedef struct {
    int32_t kind; /* an ab_synth_field_kind */
    double a, b;  /* the variant's two parameters (ignored for Uniform) */
} ab_synth_field_type;
typedef enum { /* PsfType (pipeline.rs:24-28) */
    AB_SYNTH_PSF_GAUSSIAN = 0, /* fwhm */
    AB_SYNTH_PSF_MOFFAT = 1,   /* fwhm, beta */
    AB_SYNTH_PSF_AIRY = 2      /* fwhm holds lambda_over_d */
} ab_synth_psf_kind;
typedef struct {
    int32_t kind; /* an ab_synth_psf_kind */
    double fwhm;  /* Gaussian / Moffat: fwhm; Airy: lambda_over_d (pixels) */
    double beta;  /* Moffat only */
} ab_synth_psf_type;
typedef struct { /* NoiseParams (noise.rs:8-16); Default (:18-30): 1.5, 8.0, 200.0, 0.05, 300.0, 1000.0, seed 123 */
    double gain, readout_noise, sky_background, dark_current, exposure_time, bias_level;
    uint64_t seed;
} ab_synth_noise_params;
typedef struct { /* SynthConfig (pipeline.rs:31-39); Default (:41-53): Uniform, Gaussian fwhm 3, no vignette, strength 0.3, 1 frame */
    ab_synth_field_config field;
    ab_synth_field_type field_type;
    ab_synth_psf_type psf_type;
    ab_synth_noise_params noise;
    int32_t apply_vignette; /* bool */
    double vignette_strength;
    uint32_t n_frames;
} ab_synth_config;
typedef struct {
    size_t star_count;     /* SynthResult.star_count */
    size_t frames_on_host; /* frames whose noise took the general (host) route, see ab_synth_apply_noise */
} ab_synth_result;
#define AB_SYNTH_MAX_PSF_RADIUS 512
/* EXACTNESS of this section.  Every generator of the reference is StdRng::seed_from_u64(seed) of rand 0.8.5: ChaCha with 12 rounds
 * (rand_chacha 0.3.1), keyed by eight PCG32 outputs over the seed (rand_core 0.6.4), 64-bit block counter from 0, stream id 0,
 * words consumed in block order, gen::<f64>() = (next_u64() >> 11) * 2^-53.  A draw's position in the stream decides its value, so
 * each pixel computes its own draws wherever the number of draws per pixel is fixed.
 *   - the stream, the star fields, the flat field and apply_flat_field: bit for bit the reference's algorithm (IEEE + - * / sqrt on
 *     the device, glibc pow / cos / sin / log on the host -- what Rust's f64 methods call on Linux).
 *   - ab_synth_render_stars: the device's f64 exp / pow / sin / cos are not glibc's and psf_sum is a fixed tree sum, not a raster-order
 *     one.  Relative differences of a few 2^-53 are far below half an f32 ulp, so each f32 addend is the reference's or its neighbour:
 *     a pixel covered by k stars differs by at most 2 k ulp of its accumulated value, a pixel covered by none is exactly 0.0.  The
 *     addends are accumulated in star order (a gather over per-tile lists in ascending star index, no atomics).
 *   - ab_synth_apply_noise, fast route: given the same input plane the photon count is the reference's whenever
 *     lambda + sqrt(lambda) * N(0, 1) is further from a half-integer than the f64 error of that product (below about 1e-9 for lambda up
 *     to 1e6); the output is then within one f32 ulp.  General route: bit for bit.
 *   - run to run every output is bit-identical.
 *   - agreement with frames the reference actually writes rests on rand 0.8.5's published algorithms and has NOT been checked
 *     against a Rust build (there is no rustc where this library is built, and the reference has no test or fixture for this
 *     module) -- as for rustfft in ab_phase_correlate.  The ChaCha block function passes the published 20-round vector.
 * One DELIBERATE difference: a star whose window lies wholly left of or above the image (x + psf_r < 0; king_cluster and
 * exponential_disk can produce one) makes the reference's `as usize` bound wrap, and render_stars then loops over ~2^64 pixels and
 * does not return.  The library skips such a star, as the reference itself skips one wholly right of or below the image. */
AB_API void ab_synth_config_default(ab_synth_config *cfg);
/* draws skip .. skip + n - 1 (as gen::<f64>()) of StdRng::seed_from_u64(seed); host-only */
AB_API int ab_synth_rng_f64(uint64_t seed, uint64_t skip, size_t n, double *out);
/* test hook: one 64-byte block of the ChaCha block function behind the stream -- key of eight u32 words, 64-bit counter, zero stream
 * id; rounds = 12 (the generator's) or 20 (RFC 7539's known answers with a zero nonce); any other count -> AB_ERR_INVALID.  Host-only. */
AB_API int ab_synth_chacha_block(const uint32_t *key, uint64_t counter, int rounds, uint32_t *out16);
/* gen_field (pipeline.rs:126-138): uniform_field (star_field.rs:52-66), king_cluster (:68-93) or exponential_disk (:95-119) of
 * cfg->field / cfg->field_type, in the reference's draw order; host-only scalar maths.  stars_out receives the first
 * min(n_stars, cap) stars (nullable when cap = 0), *n_out = n_stars.  AB_ERR_INVALID for what would not terminate in the reference:
 * king_cluster with a non-positive or non-finite core or tidal radius, or a profile that can never accept (its maximum, at r = 0,
 * is not positive); also for an unknown kind. */
AB_API int ab_synth_star_field(const ab_synth_config *cfg, ab_synth_star *stars_out, size_t cap, size_t *n_out);
/* render_stars (psf.rs:123-158) of n host-side stars into out (host or device; its dims are the image's; every pixel is written).
 * AB_ERR_INVALID: a non-finite x, y or flux (the reference writes NaN into pixel (0, 0) for those); a non-positive or non-finite
 * PSF parameter.  AB_ERR_UNSUPPORTED: psf_r = ceil(radius) above AB_SYNTH_MAX_PSF_RADIUS (512 px: a star's window is then over a
 * million pixels -- the default Gaussian has psf_r = 6).  Stars wholly outside the image on any side are skipped (see above). */
AB_API int ab_synth_render_stars(ab_ctx *ctx, const ab_synth_star *stars, size_t n, const ab_synth_psf_type *psf, ab_plane_mut *out);
/* generate_flat_field (noise.rs:81-99): pixel i (raster order) takes draw i of the seed's stream.  out host or device. */
AB_API int ab_synth_flat_field(ab_ctx *ctx, uint64_t seed, double vignette_strength, ab_plane_mut *out);
/* apply_flat_field (noise.rs:101-111): img /= flat where flat > 1e-6 (f32 division), in place; both host or device, equal dims. */
AB_API int ab_synth_apply_flat_field(ab_ctx *ctx, ab_plane_mut *img_inout, const ab_plane *flat);
/* apply_noise (noise.rs:62-79).  img and out host or device, equal dims, not overlapping.
 * FAST ROUTE: where every pixel's signal_e.max(0) is finite and >= 30 (the default parameters give 90 015) each pixel takes
 * exactly four draws, and one lane computes the ChaCha block of two adjacent pixels in raster order.  GENERAL ROUTE: the kernel
 * raises a flag if any pixel is below 30 or non-finite; the frame is then recomputed on the host by the reference's serial walk
 * (Knuth's product loop takes a data-dependent number of draws) over the same stream code.  Reading the flag makes the call
 * synchronous.  res (nullable): frames_on_host = 1 if the general route ran, else 0.  The route is not an ab_fallback_kind. */
AB_API int ab_synth_apply_noise(ab_ctx *ctx, const ab_plane *img, const ab_synth_noise_params *params, ab_plane_mut *out,
                                ab_synth_result *res);
/* generate (pipeline.rs:63-82): star field, render, optional flat (seed noise.seed + 999, wrapping), noise -- chained on the device.
 * noisy_out and truth_out (nullable) host or device, height x width; stars_out receives min(star_count, cap) stars (nullable
 * when cap = 0).  res (nullable).  The errors of the steps above, and AB_ERR_INVALID for planes that are not height x width. */
AB_API int ab_synth_generate(ab_ctx *ctx, const ab_synth_config *cfg, ab_plane_mut *noisy_out, ab_plane_mut *truth_out,
                             ab_synth_star *stars_out, size_t cap, ab_synth_result *res);
/* generate_stack (pipeline.rs:84-108): rendered once; frame i uses flat seed noise.seed + 999 + i and noise seed
 * noise.seed + i * 7919 (both wrapping, as a release build of the reference).  frames_out: cfg->n_frames planes (n_frames = 0 ->
 * AB_ERR_INVALID); device frames can be handed straight to ab_stack_sigma_clip.  The progress callback is ticked ("synth", k, n)
 * and cancellation seen before each frame; the frames' route flags are read once at the end. */
AB_API int ab_synth_generate_stack(ab_ctx *ctx, const ab_synth_config *cfg, ab_plane_mut *frames_out, ab_plane_mut *truth_out,
                                   ab_synth_star *stars_out, size_t cap, ab_synth_result *res);

/* ---- drizzle stacking, core/stacking/drizzle.rs (calibration.rs:320 drizzle_from_paths, drizzle_rgb_cmd) ------------------- */
typedef struct { /* DrizzleConfig (types/stacking.rs) */
    double scale;   /* clamped to [1, 4] (drizzle.rs:274) */
    double pixfrac; /* clamped to [0.1, 1] (:275) */
    int32_t kernel; /* DrizzleKernel: 0 Square, 1 Gaussian, 2 Lanczos3 */
    float sigma_low, sigma_high;
    size_t sigma_iterations;
    int32_t align;            /* bool */
    int32_t alignment_method; /* AlignmentMethod: 0 PhaseCorrelation, 1 Zncc (routed to the affine estimate, :300-313) */
    int32_t num_threads;      /* what the affine estimate takes from rayon::current_num_threads() (ab_align_channel_affine); <= 0: 8 */
} ab_drizzle_config;
typedef struct { /* DrizzleResult's scalars (:335-344); the offsets are an argument of their own */
    size_t frame_count;
    double output_scale;
    int64_t in_rows, in_cols, out_rows, out_cols;
    uint64_t rejected_pixels;
} ab_drizzle_result;
/* drizzle_stack's checks and dims (:231-279), host-only: n = 0 ("No images to drizzle"), n < 2 ("Drizzle requires at least 2
 * frames ..."), rows or cols varying by more than (max(min_rows, min_cols) as f64 * 0.05) as usize ("Frame dimensions vary too
 * much ..."), n > 32 767 (the reference counts 2 n samples per pixel in a u16) or a NaN scale / pixfrac -> AB_ERR_INVALID;
 * otherwise the cropped input dims and out = ceil(in * clamp(scale, 1, 4)) per axis.  Any output pointer may be NULL. */
AB_API int ab_drizzle_output_dims(const ab_plane *planes, size_t n, const ab_drizzle_config *cfg, int64_t *in_rows, int64_t *in_cols,
                                  int64_t *out_rows, int64_t *out_cols);
/* The checks above, then drizzle_frame (:46-122) per frame and finalize (:124-199) with the caller's offsets: n (dx, dy) pairs
 * as DrizzleResult.offsets reports them (the negation of :323 happens inside; all finite, else AB_ERR_INVALID); cfg->align and
 * alignment_method are not read.  Frames host or device, of differing dims within the tolerance (cropped by stride, not
 * copied); out_image and out_weight host or device, ab_drizzle_output_dims' out dims; out_weight NULL (or with NULL data) = not
 * wanted.  The reference's scatter is computed as a gather, one lane per output pixel, which rebuilds each pixel's sample list in
 * the reference's order (frame, input row, input column) with its cap of max(2 n, 4) samples and its `w > 1e-12` test in the
 * reference's f64 operations.  Square: weight map and rejected_pixels bit for bit; image bit for bit where the survivors' f64 sum
 * is exact, else within 1 f32 ulp (the sum runs in ascending order of value; the reference's order after select_nth_unstable is
 * unspecified).  Gaussian / Lanczos3: the device's f64 exp / sin are not glibc's, so a weight may differ in its last bits (the
 * f32 weight map: 1e-6 relative) and a candidate whose weight lies within that of 1e-12 may fall on the other side.  Up to 32
 * frames the lists stay on chip; 33 .. 32 767 frames take a general path (correct, slower).  Not asynchronous: rejected_pixels is
 * read back.  The output is enqueued in bands: cancellation is seen, and the progress callback ticked ("drizzle k/n"), per band. */
AB_API int ab_drizzle_frames(ab_ctx *ctx, const ab_plane *planes, size_t n, const double *offsets_dx_dy, const ab_drizzle_config *cfg,
                             ab_plane_mut *out_image, ab_plane_mut *out_weight, ab_drizzle_result *res);
/* drizzle_stack whole (:227-346): offsets of frames 1 .. n - 1 against frame 0 (:281-318) -- align = 0: zeros; PhaseCorrelation:
 * ab_phase_correlate's (dx, dy), and where its confidence < 2.0 (phase_correlation.rs:163) the affine estimate's (tx, ty)
 * (align.rs:73-80 = ab_align_channel_affine's transform[2], [5]); Zncc: always the affine estimate -- then ab_drizzle_frames.
 * offsets_dx_dy (nullable) receives the n pairs. */
AB_API int ab_drizzle_stack(ab_ctx *ctx, const ab_plane *planes, size_t n, const ab_drizzle_config *cfg, ab_plane_mut *out_image,
                            ab_plane_mut *out_weight, double *offsets_dx_dy, ab_drizzle_result *res);

/* ---- a trous wavelet denoising, core/imaging/wavelet.rs (wavelet_denoise_cmd) ------------------------------------------------ */
typedef struct { /* WaveletConfig (wavelet.rs:10-15); Default (:17-25): 5 scales, {3.0, 2.5, 2.0, 1.5, 1.0}, linear_denoise = true */
    size_t num_scales;       /* clamped to [1, 8] (:47), not rejected */
    const float *thresholds; /* per-scale sigma multipliers: num_thresholds entries (NULL when 0); scale j takes entry j, beyond the
                              * list its last entry, of an empty list 1.0 (:93-97) -- entries past the eighth are never read */
    size_t num_thresholds;
    int32_t linear_denoise;  /* bool: soft thresholding (:227-236), else hard (:238-244) */
} ab_wavelet_config;
typedef struct { /* WaveletResult's scalars (:27-33); elapsed_ms is the host's to measure */
    size_t scales_processed;
    double noise_estimate;
} ab_wavelet_result;
/* The per-scale thresholds of wavelet_denoise (:93-99) for all eight scales: out[j] = ts_j * (f32)(noise_sigma *
 * atrous_noise_scaling(j)) (:218-225) -- the product in f64, the cast, then the f32 multiply.  Host-only scalar maths, bit for bit
 * the reference's; the GPU path takes its thresholds from this function.  cfg->num_scales is not read. */
AB_API int ab_wavelet_scale_thresholds(double noise_sigma, const ab_wavelet_config *cfg, float out[8]);
/* wavelet_denoise (:41-133): the B3-spline a trous decomposition (atrous_smooth_buffers, :135-186; clamped borders, step 2^j),
 * noise_sigma = 1.4826 * median of the finite |d_0| (estimate_noise_sigma, :203-216), soft or hard thresholding of every detail
 * plane and the reconstruction with its finite-and-non-negative gate (:112-121).  img and out host or device, out = img's dims
 * and not overlapping it; NULL arguments, an empty image, or 2^31 pixels or more -> AB_ERR_INVALID.  Every f32 operation is the
 * reference's, in its order and unfused: `out`, noise_estimate and scales_processed equal the reference's bit for bit, NaN / inf
 * pixels included.  Every scale is two streaming launches (a horizontal and a vertical pass).
 * Progress: 2 * S + 1 ticks ("decomposing scale i/S", "thresholding scale i/S", "reconstructing"); cancellation is seen before
 * every decomposing and every thresholding tick (:62-67, :86-91).  Not asynchronous: the median is read back. */
AB_API int ab_wavelet_denoise(ab_ctx *ctx, const ab_plane *img, const ab_wavelet_config *cfg, ab_plane_mut *out, ab_wavelet_result *res);

/* ---- FFT power spectrum, core/analysis/fft.rs (compute_fft_spectrum: cmd/analysis/mod.rs:66-96) ------------------------------ */
/* math/fft.rs:137-148 (FftEngine2D::<f32>::forward_2d), :202-245 (prepare_windowed_buffer, prepare_buffer_no_window),
 * math/window.rs:20-35 (hann_symmetric).  The transform is this library's own f32 FFT (radix-2 butterflies, twiddles evaluated in
 * f64 and rounded once to f32), not rustfft's: results agree with the reference to single-precision FFT accuracy, not bit for bit.
 * Two calls on the same input return the same bits.  |pixel| >= 1e30 is outside the contract. */
typedef struct { /* FftResult's scalars (fft.rs:11-17) */
    int64_t display_rows, display_cols; /* display_height, display_width */
    int64_t original_size;
    int32_t windowed;
} ab_fft_result;
/* compute_power_spectrum's dims (fft.rs:24-25, :53-57), host-only: original_size = max(rows, cols).next_power_of_two(),
 * display_size = min(original_size, 1024).  rows or cols < 1 -> AB_ERR_INVALID; original_size > 16384 -> AB_ERR_UNSUPPORTED.
 * Either output pointer may be NULL. */
AB_API int ab_power_spectrum_dims(int64_t rows, int64_t cols, int64_t *original_size, int64_t *display_size);
/* hann_symmetric::<f32>(n) (window.rs:20-35), host-only: n == 1 -> 1; else 0.5 * (1 - cosf((2f * PIf) * (i as f32) / max(n - 1, 1)))
 * in f32.  n == 0 writes nothing.  The GPU path takes its windows from this function. */
AB_API int ab_hann_symmetric_f32(size_t n, float *out);
/* prepare_windowed_buffer / prepare_buffer_no_window + forward_2d on an fft_rows x fft_cols buffer (each a power of two in
 * 1 .. 16384): pixel (y, x) enters as (v * win_y[y]) * win_x[x] in f32 (v alone when both windows are NULL), a non-finite pixel as
 * 0, everything beyond the image as 0.  image (host or device): rows <= fft_rows, cols <= fft_cols; win_y / win_x: HOST tables of
 * image->rows / image->cols floats, both NULL or both given; out: fft_rows * fft_cols interleaved (re, im) f32 in natural
 * row-major order, host or device (out_on_device).  The padded buffer is never materialised and rows of padding are not transformed.
 * Workspace: 16 * fft_rows * fft_cols bytes of the context (released by ab_ctx_trim); AB_ERR_NOMEM when it cannot be had. */
AB_API int ab_fft2_forward_f32(ab_ctx *ctx, const ab_plane *image, const float *win_y, const float *win_x, int64_t fft_rows, int64_t fft_cols,
                               float *out, int32_t out_on_device);
/* compute_power_spectrum_opts (fft.rs:23-68): the (windowed) image zero-padded to original_size^2, forward_2d, fftshift,
 * ln(1 + |F|), and beyond 1024^2 the s x s block mean (s = original_size / 1024, downsample_area_average :70-97) -- shift,
 * magnitude, log and mean in one kernel, the original_size^2 log plane is never written.  spectrum: display_size^2
 * (ab_power_spectrum_dims), host or device. */
AB_API int ab_compute_power_spectrum(ab_ctx *ctx, const ab_plane *image, int32_t apply_window, ab_plane_mut *spectrum, ab_fft_result *result);
/* The per-pixel part of compute_fft_spectrum (cmd/analysis/mod.rs:66-96): min / max with f32::min / f32::max (a NaN is skipped),
 * range = max(max - min, 1e-10), inv = 255 / range, pixel = ((v - min) * inv) as u8 (truncating, saturating, NaN -> 0), all in f32;
 * dc = spectrum[rows / 2, cols / 2].  spectrum host or device; out_u8: rows * cols bytes, host or device (out_on_device).
 * min_val / max_val / dc may be NULL.  Not asynchronous: the range is read back. */
AB_API int ab_spectrum_to_u8(ab_ctx *ctx, const ab_plane *spectrum, uint8_t *out_u8, int32_t out_on_device, float *min_val, float *max_val,
                             float *dc);

/* ---- spectral (IFU) cubes, core/cube/{eager,lazy}.rs (process_cube_cmd, process_cube_lazy_cmd: cmd/cube.rs) ------------------- */
/* A cube is one contiguous [z][y][x] block of f32, exactly ndarray::Array3<f32>'s standard layout (eager) or the decoded frames
 * of the mmap'ed file one after another (lazy): voxel (z, y, x) at data[(z * rows + y) * cols + x].  All voxel indexing is 64-bit.
 * A host-resident cube (on_device = 0) is uploaded once per call into a workspace of the context (depth * rows * cols * 4 bytes,
 * released by ab_ctx_trim; AB_ERR_NOMEM when it cannot be had).  Every entry: NULL arguments, depth / rows / cols < 1 or output
 * dims that do not match -> AB_ERR_INVALID; so does depth >= 2^32 or more than 2^40 voxels (per-pixel counts and ranks are u32, as
 * the reference's are).  Cancellation (ab_ctx_request_cancel) is looked at before each pass over the cube;
 * there are no progress ticks (the reference has none here).  The collapsed previews (eager.rs:288-295, lazy.rs:388-397) are a
 * collapse into a device plane followed by ab_render_asinh_preview of that plane (the next section).  The host keeps the PNG
 * encoder, the mmap, the header parsing, classify_spectral_cube, build_wavelength_axis and the LRU frame cache. */
typedef struct {
    const float *data;
    int64_t depth, rows, cols;
    int32_t on_device; /* 0 host, 1 device (HBM) */
} ab_cube;
typedef enum {
    AB_CUBE_VALID_NONZERO = 0,      /* finite && v != 0.0: the eager path (eager.rs:39, :171; math/simd.rs:227) */
    AB_CUBE_VALID_ABOVE_PADDING = 1 /* finite && v > 1e-7f: the lazy path, stats::is_valid_pixel (core/imaging/stats.rs:11-13) */
} ab_cube_valid_rule;
typedef struct { /* GlobalCubeStats (eager.rs:160-166) */
    float median, sigma, low, high;
} ab_cube_stats;
/* collapse_mean_simd (math/simd.rs:216-253) = collapse_mean (eager.rs:24-26), rule 0; collapse_mean_lazy (lazy.rs:246-284), rule 1.
 * Per pixel: the f64 sum of the valid samples in ascending z, their u32 count, (sum / count as f64) as f32; no valid sample -> 0.
 * One lane owns a pixel's whole column, so the additions happen in the reference's order: bit for bit.  out: rows x cols, host or
 * device; asynchronous on the context's stream when it is a device plane.  rule: an ab_cube_valid_rule. */
AB_API int ab_cube_collapse_mean(ab_ctx *ctx, const ab_cube *cube, int32_t rule, ab_plane_mut *out);
/* collapse_median (eager.rs:28-55), rule 0; collapse_median_lazy (lazy.rs:286-329), rule 1: element [len / 2] -- the upper median --
 * of the column's valid samples under f32_cmp (math/median.rs:4-13); no valid sample -> 0.  A radix select along z on the
 * order-preserving key of the bit pattern (8-bit digits, four passes over the column): bit for bit, negative values and ties
 * included.  out as above. */
AB_API int ab_cube_collapse_median(ab_ctx *ctx, const ab_cube *cube, int32_t rule, ab_plane_mut *out);
/* The frame stride of compute_global_stats_streaming (lazy.rs:334-335), host-only: s = min(32, depth); depth > s ? depth / s : 1.
 * depth < 1 -> 1. */
AB_API uint64_t ab_cube_streaming_step(int64_t depth);
/* compute_global_stats (eager.rs:168-208): rule 0, frame_step 1.  compute_global_stats_streaming (lazy.rs:331-370): rule 1,
 * frame_step = ab_cube_streaming_step(depth).  The frames used are z = 0, step, 2 * step, ... (step_by; frame_step < 1 is taken as
 * 1).  With the n valid values of those frames sorted into s: median = s[n / 2], low = s[(n as f64 * 0.01) as usize],
 * high = s[min((n as f64 * 0.999) as usize, n - 1)] (the rank products in f64 on the host, as written), sigma =
 * max(d[n / 2] * 1.4826f32, 1e-10f32) with d the sorted |v - median| computed in f32.  n = 0 -> {0, 1, 0, 1}.  count (nullable)
 * receives n.  An 11/11/10-bit radix select over signed keys, the three ranks descending together, then the select of the
 * deviations: all four values bit for bit.  Not asynchronous: the histograms are read back. */
AB_API int ab_cube_global_stats(ab_ctx *ctx, const ab_cube *cube, int32_t rule, int64_t frame_step, ab_cube_stats *stats, uint64_t *count);
/* normalize_with_global (eager.rs:210-222) = normalize_frame_with_stats (lazy.rs:87-99): a non-finite pixel -> 0, otherwise
 * asinh((10f32 / sigma) * (clamp(v, low, high) - median)), the argument formed in f32 in that order.  !(low <= high) or a NaN
 * statistic -> AB_ERR_INVALID (the reference panics in f32::clamp).
 * DEFINITION of the result: the f32 rounding of the f64 asinh of that f32 argument (computed in f64 on the device).  Rust's
 * f32::asinh is ln_1p(ax + ax / (hypot(1, 1 / ax) + 1 / ax)) through the platform libm's f32 functions, so its bits depend on the
 * libm and are not a target: this result is within 2 f32 ulp of the reference's own formula (that formula evaluated in f32 differs
 * from the definition on 5 - 14 % of values, depending on their distribution, by at most 2 ulp).  An argument that overflows f32 is outside the contract.
 * img and out: the same dims, host or device; asynchronous for device planes. */
AB_API int ab_cube_normalize_frame(ab_ctx *ctx, const ab_plane *img, const ab_cube_stats *stats, ab_plane_mut *out);
/* The per-pixel work of export_cube_frames_sampled (eager.rs:224-246) and of process_cube_lazy's frame loop (lazy.rs:414-420) up
 * to the PNG encoder: for every z = k * step (frame_step < 1 is taken as 1) the frame normalised as above, its (min, max)
 * (find_minmax_simd, math/simd.rs:263-271), range = max(max - min, 1e-10), inv = 255f32 / range and byte = (v.is_finite() &&
 * v > 1e-7) ? ((v - min) * inv).clamp(0, 255) as u8 : 0 (infra/render/grayscale.rs:10-29; everything at or below the median renders
 * 0).  Frame k lands at out_u8 + k * rows * cols (host or device: out_on_device), frame_count (nullable) = ceil(depth / step).
 * Two launches for all frames: the normalised f32 frames are never written, the per-frame ranges stay on the device.
 * Asynchronous for a device output. */
AB_API int ab_cube_export_frames(ab_ctx *ctx, const ab_cube *cube, const ab_cube_stats *stats, int64_t frame_step, uint8_t *out_u8,
                                 int32_t out_on_device, int64_t *frame_count);
/* extract_spectrum (eager.rs:57-60), LazyCube::extract_spectrum_at (lazy.rs:222-239): the depth values at (y, x) into out (host or
 * device: out_on_device).  y >= rows or x >= cols (or negative) -> AB_ERR_INVALID, "Pixel (y, x) out of bounds".  Asynchronous
 * for a device cube with a device output.  A host cube is read where it lies (nothing is uploaded): its column is gathered on
 * the host, and with a device output the call has synchronised the stream and finished the copy when it returns. */
AB_API int ab_cube_extract_spectrum(ab_ctx *ctx, const ab_cube *cube, int64_t y, int64_t x, float *out, int32_t out_on_device);

/* ---- the robust asinh preview and the byte renderers: render_asinh_and_save (cmd/common.rs:242-261), infra/render/grayscale.rs -- */
/* robust_asinh_preview = math::simd::asinh_normalize_simd (math/simd.rs:160-214), then render_grayscale (grayscale.rs:10-29): how
 * the stack, calibrate and resample commands and both cube commands finish; the export command's four renderers (grayscale.rs:10-74,
 * cmd/export/mod.rs:233-240).  Everything stops at the PNG encoder.  Pixels are indexed flat, i = y * cols + x, n = rows * cols.
 * Every entry: a NULL argument (the ones marked nullable excepted), rows / cols < 1, an output whose dims do not match, a route
 * outside ab_asinh_route or bits outside {8, 16} -> AB_ERR_INVALID.  Planes host or device; a device plane at any float-aligned
 * address is served (the kernels peel to their 16-byte groups themselves).
 *
 * Statistics (simd.rs:163-180) over the m pixels with is_finite() && v > 1e-7f, sorted into s:
 *   median = median_f32_mut (math/median.rs:46-63): s[m / 2], or for even m (s[m / 2 - 1] + s[m / 2]) / 2.0 in f32 (NOT the cube's
 *            upper median);
 *   sigma  = max(median_f32_mut(|v - median| in f32) * 1.4826f32, 1e-10f32);
 *   low    = s[(m as f64 * 0.01) as usize], high = s[min((m as f64 * 0.999) as usize, m - 1)].
 * All four bit for bit: exact order statistics by radix select, no sort.  m == 0: all four are 0, and the preview is a copy of the
 * input (simd.rs:165-167).
 *
 * The map, with isa = 10f32 / sigma.  The reference has two routes; both are here, selected by `route`:
 *   AB_ASINH_ROUTE_AVX2 (simd.rs:115-158, what an x86-64 host with AVX2 runs).  For i < 8 * (n / 8), counted from flat index 0:
 *     valid = v == v && v > 1e-7f (so +inf IS valid; NaN and -inf are not); clamped = min(max(v, low), high); scaled = (clamped -
 *     median) * isa; a = |scaled|; inner = a + sqrt(a * a + 1); the result is fast_log_avx2(inner) (simd.rs:28-84: mantissa | 0x3F000000,
 *     e = exponent field - 0x7E, the doubling below FRAC_1_SQRT_2, the nine-coefficient Horner chain with separate mul and add,
 *     (f - 0.5 f^2) + f^3 r, e * LN_2 + that) with scaled's sign bit OR-ed in; an invalid pixel gives 0.  Every operation is f32 and
 *     unfused, the sqrt correctly rounded, subnormals kept: BIT FOR BIT for every input, quirks included (a * a overflowing gives
 *     +-128 * LN_2 = +-88.72284; |scaled| below 2^-24 gives +-0 because inner rounds to 1).  The last n % 8 pixels take the
 *     scalar route's formula.
 *   AB_ASINH_ROUTE_SCALAR (simd.rs:203-211 with fast_asinh_scalar :9-18, what every pixel takes on a host without AVX2, e.g. aarch64).
 *     valid = is_finite() && v > 1e-7f (+inf is NOT valid); x = isa * (clamp(v, low, high) - median); for |x| < 0.5 the result is
 *     x * (1 - x2 * (1f32 / 6f32 - (x2 * 3) / 40)) with x2 = x * x, in f32 in that order: bit for bit.  Otherwise sign * ln(|x| +
 *     sqrt(|x| * |x| + 1)), the argument formed in f32.  ln is the platform libm's logf, whose bits are not a target: the result is
 *     DEFINED (as ab_cube_normalize_frame defines its asinh) as the f32 rounding of the f64 log of that f32 argument, computed in f64
 *     on the device.  An overflowing |x|^2 gives +-inf, as in the reference.
 * These are the two places where the contract is a definition and not a particular host's bits: the scalar route's ln, and
 * infinities in find_minmax (below). */
typedef enum {
    AB_ASINH_ROUTE_AVX2 = 0,  /* normalize_chunk_avx2 + the scalar remainder */
    AB_ASINH_ROUTE_SCALAR = 1 /* the scalar loop for every pixel */
} ab_asinh_route;
typedef struct {
    float median, sigma, low, high;
    uint64_t valid_count; /* m */
} ab_asinh_stats;
/* The statistics above.  One select request for the ranks m / 2 - 1 (even m), m / 2, low and high, which descend together, then one
 * select of the deviations.  Not asynchronous: the histograms are read back. */
AB_API int ab_asinh_preview_stats(ab_ctx *ctx, const ab_plane *img, ab_asinh_stats *out);
/* The map alone, with the caller's statistics (isa = 10f32 / stats->sigma).  A NaN statistic or !(low <= high) -> AB_ERR_INVALID (the
 * scalar route's f32::clamp would panic).  stats->valid_count == 0 copies the input.  out: img's dims; exactly img (in place), or
 * not overlapping it.  Asynchronous for device planes. */
AB_API int ab_asinh_normalize_with_stats(ab_ctx *ctx, const ab_plane *img, const ab_asinh_stats *stats, int32_t route, ab_plane_mut *out);
/* asinh_normalize_simd itself: the statistics, then the map (or the copy).  out as above; stats_out nullable. */
AB_API int ab_robust_asinh_preview(ab_ctx *ctx, const ab_plane *img, int32_t route, ab_plane_mut *out, ab_asinh_stats *stats_out);
/* render_asinh_and_save up to the PNG encoder: out_u8 (rows * cols bytes, host or device: out_on_device) = render_grayscale's bytes of
 * robust_asinh_preview(img).  The f32 preview is never written: after the statistics, one launch recomputes the map and reduces
 * the min / max (an invalid pixel contributes its 0), a second finishes the range, recomputes the map, quantises and stores packed
 * bytes.  Byte for byte what ab_robust_asinh_preview followed by ab_render_grayscale gives.  valid_count == 0: every byte is 0.
 * stats_out nullable.  The statistics synchronise; the two launches (and nothing after them) are asynchronous for a device output. */
AB_API int ab_render_asinh_preview(ab_ctx *ctx, const ab_plane *img, int32_t route, uint8_t *out_u8, int32_t out_on_device,
                                   ab_asinh_stats *stats_out);
/* render_grayscale (bits = 8, grayscale.rs:10-29) and render_grayscale_16bit (bits = 16, :31-50).  (min, max) over the pixels with
 * is_finite(): find_minmax_simd's scalar statement (simd.rs:263-271), the one ab_cube_export_frames cites.  range = max(max - min,
 * 1e-10), inv = 255f32 / range (65535f32), sample = (is_finite() && v > 1e-7f) ? ((v - min) * inv).clamp(0, top) as u8 / u16 : 0
 * (`as` truncates and saturates; NaN -> 0).  16-bit samples are written as BIG-ENDIAN byte pairs, which is what write_png_l16 hands
 * the encoder (:95).  out: rows * cols * bits / 8 bytes, host or device.  min_out / max_out nullable; asking for either synchronises.
 * With no finite pixel min = f32::MAX and max = f32::MIN = -f32::MAX: max - min is -inf, range is 1e-10, no pixel passes the validity
 * test and every sample is 0; min_out / max_out receive those two values.
 * Infinities: the reference's AVX2 find_minmax (simd.rs:274-315) masks with v == v, so it COUNTS +-inf among the first 8 * (n / 8)
 * values; the range becomes inf, inv 0 (or the difference NaN), and the whole plane renders 0.  Here, as in the scalar statement,
 * an infinity is skipped.  A plane holding +-inf is therefore outside the bit-for-bit claim against an AVX2 host. */
AB_API int ab_render_grayscale(ab_ctx *ctx, const ab_plane *img, int32_t bits, void *out, int32_t out_on_device, float *min_out, float *max_out);
/* render_stretched_8bit / _16bit (grayscale.rs:52-74): (v.clamp(0, 1) * 255f32) as u8 (65535f32, u16; big-endian pairs).  There is no
 * validity test: NaN -> 0, +inf -> top, -inf -> 0.  One launch; asynchronous for a device plane with a device output. */
AB_API int ab_render_stretched(ab_ctx *ctx, const ab_plane *img, int32_t bits, void *out, int32_t out_on_device);

/* ---- the colour finish: core/compose/drizzle_rgb.rs, infra/render/rgb.rs, cmd/export/mod.rs (export_png, export_rgb_png) ------ */
/* What the export and drizzle commands do to three channels once they exist, up to the PNG / FITS writers.  One fused kernel family
 * (csrc/rgb_export.hip) computes per pixel and channel: the load through the source's own row stride (a top-left crop costs no
 * copy; an absent channel reads as 0), the white-balance multiply v * (wb as f32) (drizzle_rgb.rs:82-84), stf::apply_stf_f32's value
 * (stf.rs:104-120, which MULTIPLIES by inv_clip: not process_rgb's compose-local stretch, which divides by clip_range, rgb.rs:199-206 --
 * the two differ in the last bit), SCNR on the three stretched values in registers (scnr.rs:28-52), and one of three packers:
 *   AB_RGB_PACK_8        (v.clamp(0, 1) * 255f32) as u8              render_rgb, rgb.rs:29-31
 *   AB_RGB_PACK_8_ROUND  (v.clamp(0, 1) * 255f32).round() as u8      drizzle_rgb.rs:244-246 (half away from zero)
 *   AB_RGB_PACK_16BE     (v.clamp(0, 1) * 65535f32) as u16           render_rgb_16bit, rgb.rs:71-77: high byte first
 * interleaved R, G, B.  f32::clamp keeps a NaN and `as` truncates, saturates and sends NaN to 0: NaN -> 0, -inf -> 0, +inf -> top.
 * Every operation is an IEEE basic operation, unfused: every plane and every byte is the reference's, bit for bit.  Planes host or
 * device at any float-aligned address; a device byte output at ANY address (whole dwords are stored wherever it allows).  An output
 * may not overlap an input.  rows * cols >= 2^31 -> AB_ERR_INVALID. */
typedef enum { AB_RGB_PACK_8 = 0, AB_RGB_PACK_8_ROUND = 1, AB_RGB_PACK_16BE = 2 } ab_rgb_pack;
/* host-only: rows * cols * 3 * (pack == AB_RGB_PACK_16BE ? 2 : 1); a pack outside the enum, rows or cols < 1 or rows * cols >= 2^31
 * -> AB_ERR_INVALID */
AB_API int ab_rgb_packed_bytes(int64_t rows, int64_t cols, int32_t pack, size_t *bytes);
/* render_rgb (rgb.rs:7-47) at full size, render_rgb_16bit (:49-91) and the drizzle packer (drizzle_rgb.rs:232-248) on planes that are
 * already stretched: the packer alone.  r, g, b of one size; out: ab_rgb_packed_bytes.  One launch, asynchronous for device planes
 * with a device output.  AB_RGB_PACK_8 gives what ab_render_rgb_preview gives when max_dim covers the image. */
AB_API int ab_render_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, int32_t pack, void *out, int32_t out_on_device);
/* apply_stf_f32(c, &stf[c], &stats[c]) x 3 and then the packer, fused: what export/mod.rs:189-207, :321-328 and :362-382 do once their
 * statistics and STF are known.  One launch; the three stretched f32 planes are never written.  Byte for byte ab_apply_stf_f32 x 3
 * followed by ab_render_rgb. */
AB_API int ab_render_rgb_stf(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_stf_params stf[3],
                             const ab_image_stats stats[3], int32_t pack, void *out, int32_t out_on_device);
typedef struct {
    int32_t bits;    /* 8 (render_rgb) | 16 (render_rgb_16bit); anything else -> AB_ERR_INVALID */
    int32_t has_stf; /* 1: stf[3] as given (the explicit branch, :362-370); 0: compute_linked_stf of the three statistics with
                        AutoStfConfig::default() for all three channels (:371-378) */
    ab_stf_params stf[3];
} ab_rgb_export_config;
typedef struct {
    uint64_t rows, cols;
    int32_t resampled;
    ab_image_stats stats[3]; /* compute_image_stats per channel (after the resampling) */
    ab_stf_params stf[3];    /* what was applied */
} ab_rgb_export_info;
/* stretch_and_render whole (export/mod.rs:357-409): channels of differing dims are first resampled (bicubic, ab_resample_image) to
 * the largest rows and the largest cols (:396-407); compute_image_stats per channel; the STF choice; ab_render_rgb_stf with
 * AB_RGB_PACK_8 / AB_RGB_PACK_16BE.  out: the largest dims.  Not asynchronous: the statistics are read back. */
AB_API int ab_export_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_rgb_export_config *cfg, void *out,
                         int32_t out_on_device, ab_rgb_export_info *info);
typedef struct { /* DrizzleRgbConfig (types/compose.rs) without its DrizzleConfig, which is an argument of its own */
    int32_t white_balance; /* as ab_rgb_compose_config: 0 Auto, 1 Manual(wb_manual), 2 None */
    double wb_manual[3];
    int32_t auto_stretch, linked_stf;
    int32_t has_scnr; /* Option<ScnrConfig> */
    ab_scnr_config scnr;
} ab_drizzle_rgb_config;
typedef struct { /* the scalars of ProcessedDrizzleRgb (drizzle_rgb.rs:24-39) */
    uint64_t rows, cols;
    double wb[3];               /* the multipliers (:76-80), applied as f32 */
    ab_stf_params stf[3];
    double chan_stats[3][4];    /* ChannelStats {min, max, median, mean} BEFORE white balance (:72-74) */
    ab_image_stats stats_wb[3]; /* the statistics the STF is applied with */
    int32_t scnr_applied;       /* a configuration was given (:122-127), whether or not its amount did anything */
} ab_processed_drizzle_rgb_info;
/* process_drizzle_rgb (drizzle_rgb.rs:41-145).  Absent channels NULL (a zero plane, :63-66: its statistics are all 0); at least one
 * present.  Output dims = the minimum rows and the minimum cols over the present channels (a top-left crop, :54-61).  Statistics of
 * the cropped planes; white balance (every channel is multiplied, even by 1; where (float)wb == 1 the second statistics are the
 * first); auto_stretch && linked_stf: auto_stf of the statistics of ((r + g) + b) / 3f32 -- a true division, not process_rgb's
 * multiplication by 1 / 3 -- shared by the channels, each applied with its OWN statistics (:89-96); auto_stretch alone: per channel
 * (:97-105); neither: {0, 0.5, 1} (:106-116); apply_stf_f32; SCNR.  out_stretched[3], out_wb[3] (arrays of three planes of the
 * output dims, host or device) and out_rgb8 (rows * cols * 3 bytes, AB_RGB_PACK_8_ROUND of the stretched planes, :232-248) are each
 * nullable.  After the statistics the white-balanced planes are written by one launch and everything else by one more. */
AB_API int ab_process_drizzle_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_drizzle_rgb_config *cfg,
                                  ab_plane_mut *out_stretched, ab_plane_mut *out_wb, uint8_t *out_rgb8, int32_t out_on_device,
                                  ab_processed_drizzle_rgb_info *info);
/* drizzle_rgb (drizzle_rgb.rs:159-286) up to the PNG / FITS writers, with frames in place of paths.  Fewer than two of the three
 * lists non-NULL: AB_ERR_INVALID "Need at least 2 channels for RGB drizzle (got N)" (:171-173); a list of fewer than two frames is
 * no channel (:178); none left: "All channels failed or have fewer than 2 frames" (:203-205).  Each remaining channel goes through
 * ab_drizzle_stack into an image that stays on the device (its error is returned as it is), then ab_process_drizzle_rgb.  res[c]
 * is zeroed for a channel that is not there.  out_wb[3] (what write_fits_rgb receives) and out_rgb8 (what RgbImage::from_raw
 * receives) are nullable and sized by ab_drizzle_output_dims per channel, the minimum per axis. */
AB_API int ab_drizzle_rgb(ab_ctx *ctx, const ab_plane *r_frames, size_t n_r, const ab_plane *g_frames, size_t n_g, const ab_plane *b_frames,
                          size_t n_b, const ab_drizzle_config *dcfg, const ab_drizzle_rgb_config *cfg, ab_plane_mut *out_wb, uint8_t *out_rgb8,
                          int32_t out_on_device, ab_drizzle_result res[3], ab_processed_drizzle_rgb_info *info);

/* ---- the compose wizard's tone editor: cmd/processing/curves.rs (apply_tone_composite_cmd :57-191) up to the PNG encoder ------- */
/* Every move of an STF, levels, curves or SCNR slider runs apply_stf_f32 x 3 (:113-119), apply_levels_rgb (:121-131), apply_curve_rgb
 * (:133-146), apply_scnr_inplace (:148-154) and render_rgb_preview(.., MAX_PREVIEW_DIM) (:161, cmd/helpers.rs:204-262) over the whole
 * composite and keeps only the preview's bytes.  Every stage is pointwise, so one kernel family (csrc/tone.hip) runs the chain in
 * registers: 12 B read and 3 B written per pixel.  When the composite exceeds max_dim on a side and no plane is wanted, only the pixels
 * the preview picks are toned at all.  Each stage is the arithmetic of the entry point it stands for (ab_apply_stf_f32, ab_apply_levels,
 * ab_apply_curve, ab_apply_scnr_inplace, ab_render_rgb_preview with stf == NULL): planes and bytes are bit for bit that chain's. */
typedef struct {                /* apply_tone_composite_cmd's arguments, cmd/processing/curves.rs:58-71 */
    int32_t has_stf[3];         /* stf_r / stf_g / stf_b: Option<[f64; 3]> (:60-62) */
    ab_stf_params stf[3];       /* {shadow, midtone, highlight} = a[0], a[1], a[2] (:103-111) */
    int32_t linked_stf;         /* Option<bool>.unwrap_or(false) (:87) */
    ab_levels_params levels[3]; /* levels_r / _g / _b (:64-66); absent = LevelsParams::default() = {0, 1, 1} (:121-123) */
    const double *curve_xy[3];  /* curves_r / _g / _b: Option<ToneCurveInput> (:67-69): NULL = None; else n_curve[c] (x, y) pairs (n may be 0) */
    size_t n_curve[3];
    int32_t has_scnr;           /* Option<ScnrConfig> (:70) */
    ab_scnr_config scnr;
} ab_tone_config;
typedef struct {
    ab_stf_params stf[3];       /* what was applied (RES_STF, :171-187) */
    ab_image_stats norm[3];     /* the statistics each channel was normalised with (:89-101; the combined ones x 3 when linked) */
    int32_t levels_applied, curves_applied, scnr_applied; /* RES_LEVELS_APPLIED, RES_CURVES_APPLIED, RES_SCNR_APPLIED (:168-170) */
    uint64_t rows, cols, preview_rows, preview_cols;      /* 0 from ab_tone_plan, which sees no plane */
} ab_tone_info;
AB_API void ab_tone_config_default(ab_tone_config *cfg); /* nothing explicit, unlinked, levels {0, 1, 1}, no curves, no SCNR */
/* Host only: the command's decisions, and the three LUTs it would apply (lut3x4096 nullable; written only when curves_applied).
 *   STF     unlinked: auto_stf(stats[c], AutoStfConfig::default()), normalised with stats[c] (:92-100).  linked: the combined statistics
 *           and the one STF of compute_linked_stf_with_stats (:89-91, helpers.rs:185-202 = ab_compute_linked_stf) for all three.  An
 *           explicit stf[c] replaces channel c's parameters, never the statistics it is normalised with (:103-111).
 *   levels  applied when any channel is not LevelsParams::is_identity (:125; core/imaging/curves.rs:18-22: |black|, |gamma - 1| and
 *           |white - 1| all below 1e-7).  apply_levels then runs per channel (:127): a channel that is itself identity is CLONED
 *           (core/imaging/curves.rs:32-34) and keeps the NaN, infinity or negative value another channel sends to 0 (:46).
 *   curves  a channel is identity when it is None or SplineLut::is_identity(points) (:133-135; core/imaging/curves.rs:94-103: more
 *           than two points never; none always; one when |x - y| < 1e-6; two when they lie within 1e-6 of (0, 0) and (1, 1)).  All
 *           three identity: no curve runs (:136-138).  Else EVERY channel is looked up (:139-142): Some(points) in
 *           from_points(points) -- "identity" points included -- and None in from_points([(0, 0), (1, 1)]) (:53-55), which is no
 *           identity map: it truncates to 4096 levels and sends non-finite and negative values to 0 (core/imaging/curves.rs:105-109, :192).
 *   SCNR    has_scnr && amount > 1e-7 (:149). */
AB_API int ab_tone_plan(const ab_image_stats stats[3], const ab_tone_config *cfg, ab_tone_info *info, float *lut3x4096);
/* The command from its loaded channels (:76-84: r, g, b and their ImageStats) to the encoder's input.  r, g, b: one size, host or
 * device, any float-aligned address.  out_planes (nullable): three planes of that size, host or device -- the r_img, g_img, b_img the
 * command drops.  out_rgb8 (nullable): preview_rows x preview_cols x 3 bytes with the dims of ab_preview_dims(rows, cols, max_dim), host
 * or device (out_on_device) at ANY byte address: the pick ((d as f64) * ratio).min((n - 1) as f64) as usize (helpers.rs:306-309) and
 * the byte (v.clamp(0, 1) * 255f32) as u8 (helpers.rs:243-245; NaN -> 0) of ab_render_rgb_preview with stf == NULL.  An output may
 * not overlap an input.  A mismatch of the planes' dims, rows * cols >= 2^31, max_dim < 1 or both outputs NULL -> AB_ERR_INVALID
 * before anything touches the device.  One launch; two (full-size planes, then the pick) when out_planes is given and the image
 * exceeds max_dim.  Asynchronous when inputs and outputs are on the device (the LUTs travel through a pinned buffer of the context). */
AB_API int ab_apply_tone_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats stats[3],
                                   const ab_tone_config *cfg, int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8,
                                   int32_t out_on_device, ab_tone_info *info);
/* restretch_composite_cmd (cmd/compose/rgb.rs:208-241), the STF slider loop of the RGB Compose panel, on the tone editor's kernel:
 * apply_stf_f32 x 3 with the explicit stf[c] normalised with the cached stats[c] (:224-230), no levels, no curves,
 * apply_scnr_inplace whenever a config is present (has_scnr, :232-234) and render_rgb_preview (:237).  The command has no amount test
 * of its own; what remains is apply_scnr_inplace's (scnr.rs:28-31: clamp to 0 ..= 1, return below 1e-7), which lets a NaN amount
 * through where ab_apply_tone_composite's amount > 1e-7 (curves.rs:149) does not.  Planes and bytes are bit for bit ab_apply_stf_f32
 * x 3 + ab_apply_scnr_inplace + ab_render_rgb_preview with stf NULL; for amount > 1e-7, ab_apply_tone_composite's with the same
 * explicit STFs.  Arguments, outputs, launches and the AB_ERR_INVALID cases are ab_apply_tone_composite's, and a NULL stf, or has_scnr
 * with a NULL scnr.  update_composite_channel_cmd (:255-293) beside it is ab_resample_image + ab_compute_image_stats. */
AB_API int ab_restretch_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats stats[3],
                                  const ab_stf_params stf[3], int32_t has_scnr, const ab_scnr_config *scnr, int64_t max_dim,
                                  ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device);

/* ---- opening a file: cmd/io/mod.rs (process_fits :105-126, process_fits_full :129-172, process_rgb_fits :33-102) and the histogram
 * panel's compute_histogram (cmd/analysis/mod.rs:22-53), up to the PNG encoder and the JSON --------------------------------------- */
/* Host only.  downsample_histogram (core/imaging/stats.rs:423-444): target_bins >= n_bins copies (*out_len = n_bins); else
 * ratio = n_bins as f64 / target_bins as f64 and out[i] = the SATURATING u32 sum of bins[(i as f64 * ratio) as usize ..
 * min(((i + 1) as f64 * ratio) as usize, n_bins)), *out_len = target_bins.  out holds min(target_bins, n_bins) words.  The rule is
 * no clean partition: for 9841 of the targets below 65 536 (49, 98, 103, 107, 161, ...) (target as f64 * ratio) as usize is 65 535
 * and the LAST source bin -- the one that holds the image's maximum -- is dropped.  Reproduced.  n_bins == 0, target_bins == 0 or a
 * NULL pointer -> AB_ERR_INVALID. */
AB_API int ab_downsample_histogram(const uint32_t *bins, size_t n_bins, size_t target_bins, uint32_t *out, size_t *out_len);
/* Host only.  Histogram.bin_edges of build_histogram (stats.rs:379-387, :412-413): bins + 1 doubles, every one dmin when
 * dmax - dmin < 1e-10, else dmin + i as f64 * (range / bins as f64).  bins == 0 or NULL -> AB_ERR_INVALID. */
AB_API int ab_histogram_bin_edges(double dmin, double dmax, size_t bins, double *edges);
/* downsample_histogram(compute_histogram_with_stats(img, {min: dmin, max: dmax}), target_bins) (stats.rs:373-376, :423-444) in one
 * pass: bin for bin ab_downsample_histogram(ab_build_histogram(img, 65536, dmin, dmax), 65536, target_bins), for every pair of
 * doubles, target_bins >= 1, a host or device plane at any float-aligned address.  *out_len (nullable) = min(target_bins, 65536) =
 * the words written to out_bins (host, or device with out_on_device).  A target that divides 65 536 (up to 16 384; the product's
 * 512) accumulates the display bins in LDS: no 65 536-bin intermediate, the plane is read once.  Other targets count the 65 536
 * bins on the device and fold them there.  rows * cols >= 2^31 -> AB_ERR_INVALID (no count can wrap).  Device plane and device
 * output: asynchronous. */
AB_API int ab_display_histogram(ab_ctx *ctx, const ab_plane *img, double dmin, double dmax, size_t target_bins, uint32_t *out_bins,
                                int32_t out_on_device, size_t *out_len);
typedef struct {
    ab_auto_stf_config stf; /* AutoStfConfig::default() = {0.25, -2.8} (cmd/io/mod.rs:26, :48-50) */
    size_t hist_bins;       /* HISTOGRAM_BINS_DISPLAY = 512 (types/constants.rs:9); 0: no histogram (process_fits) */
} ab_fits_view_config;
typedef struct {
    uint64_t rows, cols;    /* RES_DIMENSIONS = [cols, rows] */
    ab_image_stats stats;   /* RES_STATS */
    ab_stf_params stf;      /* RES_STF */
    uint64_t hist_len;      /* RES_BIN_COUNT: min(hist_bins, 65536) */
} ab_fits_view_info;
typedef struct {
    uint64_t rows, cols, preview_rows, preview_cols;
    ab_image_stats stats[3]; /* stats_r, stats_g, stats_b (cmd/io/mod.rs:44-46) */
    ab_stf_params stf[3];    /* stf_r, stf_g, stf_b (:48-50) */
    uint64_t hist_len;
} ab_rgb_fits_view_info;
AB_API void ab_fits_view_config_default(ab_fits_view_config *cfg);
/* The mono branch of process_fits_full (cmd/io/mod.rs:138-144; hist_bins = 0: of process_fits, :114-116): compute_image_stats ->
 * auto_stf(cfg->stf) -> apply_stf, and downsample_histogram(compute_histogram_with_stats(img, stats), hist_bins), as ONE chain: the
 * statistics, then one kernel that reads the transform and the statistics' min / max from HBM, writes every pixel's byte and counts
 * the same pixel into the display histogram, then at most one synchronisation, which fetches info and the host outputs (info NULL
 * and device outputs: none).  img: host or device, any float-aligned address.  out_u8: rows x cols bytes at any address, host or
 * device.  out_bins: min(hist_bins, 65536) words, host or device (bins_on_device); may be NULL when hist_bins == 0.  The bytes are
 * ab_auto_stretch_preview's, the statistics and stf what it returns, the bins ab_display_histogram(img, stats.min, stats.max,
 * hist_bins)'s: max - min < 1e-10 (decided on the device; so also when no pixel is valid) -> zero bins. */
AB_API int ab_process_fits_view(ab_ctx *ctx, const ab_plane *img, const ab_fits_view_config *cfg, uint8_t *out_u8, int32_t out_on_device,
                                uint32_t *out_bins, int32_t bins_on_device, ab_fits_view_info *info);
/* process_rgb_fits from its three planes on (cmd/io/mod.rs:44-62): compute_image_stats x 3, auto_stf(cfg->stf) x 3 (unlinked),
 * apply_stf_f32 per channel, render_rgb_preview(.., max_dim) (cmd/helpers.rs:204-262) and, with hist_bins > 0, the display histogram
 * of R with R's statistics (:61-62).  One chain: three statistics chains, each followed by a small device-to-device copy of its
 * result, then one kernel that reads the three transforms from HBM and packs the preview (an image above max_dim tones only the
 * pixels the preview picks); R's histogram rides in it when every pixel is visited and is one more pass over R otherwise; one
 * synchronisation at the end, none with info NULL and device outputs.  out_rgb8 (nullable when hist_bins > 0): preview_rows x
 * preview_cols x 3 bytes with the dims of ab_preview_dims, any address.  With the default cfg->stf the bytes are
 * ab_apply_tone_composite's with ab_tone_config_default and the same statistics.  Mismatched dims, rows * cols >= 2^31, max_dim < 1,
 * out_rgb8 NULL with hist_bins == 0 or out_bins NULL with hist_bins > 0 -> AB_ERR_INVALID before anything touches the device. */
AB_API int ab_process_rgb_fits_view(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_fits_view_config *cfg,
                                    int64_t max_dim, uint8_t *out_rgb8, int32_t out_on_device, uint32_t *out_bins, int32_t bins_on_device,
                                    ab_rgb_fits_view_info *info);

/* ---- the compose wizard's blend and colour steps: cmd/compose/blend.rs (blend_channels_cmd :128-223) and cmd/compose/color.rs
 * (calibrate_and_scnr_cmd :97-184, compute_auto_wb_cmd :187-224, reset_wb_cmd :51-95), up to the PNG encoder and the JSON ---------- */
/* Both commands end alike: three ImageStats, compute_linked_stf (cmd/helpers.rs:185-202), three make_stf_u8_fn(linked, stats[c])
 * (core/imaging/stf.rs:122-145) and render_rgb_preview_with_stf (cmd/helpers.rs:264-322).  csrc/wizard_color.hip runs each as ONE chain
 * that stays in HBM: the planes' kernel, three statistics chains whose results are saved side by side on the device, one small
 * workgroup that forms the linked STF and the three transforms there (linked_stf_kernel), the preview's packer reading them from HBM
 * (preview_stf_kernel), and at most one synchronisation, which fetches info and the host outputs (info NULL and device outputs: none).
 * reset_wb_cmd needs no entry point of its own: it is ab_compute_linked_stf of the originals' cached statistics followed by
 * ab_render_rgb_preview with stf (the linked one three times) and stats given. */
typedef enum {
    AB_COLOR_STATS_EXACT_OR_FULL = 0, /* compute_image_stats of the final plane (color.rs:30, :144-154) */
    AB_COLOR_STATS_KNOWN_RANGE = 1    /* compute_image_stats_with_known_range of the final plane (color.rs:41-47) */
} ab_color_stats_route;
typedef struct {
    float factors[3];        /* (factor as f32).max(1e-6) (color.rs:115-117; f32::max: a NaN gives 1e-6) */
    int32_t scnr_applied;    /* has_scnr && amount > 1e-7 (:139; a NaN amount is not applied) */
    int32_t route[3];        /* ab_color_stats_route of R, G, B */
    double known_min[3];     /* KNOWN_RANGE: orig.min * factor as f64 and orig.max * factor as f64 (swapped for a negative factor, */
    double known_max[3];     /* :41-45); 0 on the other route */
} ab_color_plan;
typedef struct {
    uint64_t rows, cols, preview_rows, preview_cols;
    float factors[3];        /* the f32 factors applied */
    int32_t scnr_applied;    /* "scnr_applied" (:180) */
    int32_t route[3];        /* the statistics route each channel took */
    ab_image_stats stats[3]; /* stats_r, stats_g, stats_b as insert_composite_rgb receives them (:169) */
    ab_stf_params stf;       /* the linked STF: "auto_stf" (:171) */
} ab_color_step_info;
typedef struct {
    uint64_t rows, cols, preview_rows, preview_cols; /* RES_DIMENSIONS = [cols, rows] (blend.rs:213) */
    int32_t resampled;       /* needs_resample (:152) */
    ab_image_stats stats[3]; /* RES_STATS_R / _G / _B (:216-218) */
    ab_stf_params stf;       /* "auto_stf" (:219) */
} ab_blend_composite_info;
typedef struct {
    double factors[3];       /* RES_R_FACTOR, RES_G_FACTOR, RES_B_FACTOR (color.rs:203-212) */
    double stability[3];     /* stab_r, stab_g, stab_b: mad / median, f64::MAX when median <= 1e-10 (:196-201) */
    int32_t ref_channel;     /* 0 R, 1 G, 2 B (:221) */
} ab_auto_wb;
/* Host only: what calibrate_and_scnr_cmd decides for a composite of n_pixels pixels.  A channel's statistics are taken ONCE, of its
 * final plane, by the route that yields what the reference keeps: EXACT_OR_FULL when n_pixels <= 4 000 000 (PAR_THRESHOLD, :19), for
 * G when SCNR is applied (:154) and for every channel when SCNR is applied with preserve_luminance (:142-152); KNOWN_RANGE otherwise
 * (a channel SCNR does not change: its final plane is its scaled plane).  The statistics the reference computes and overwrites are
 * never computed.  scnr may be NULL when has_scnr == 0.  A NULL orig_stats, factors or plan -> AB_ERR_INVALID. */
AB_API int ab_color_step_plan(uint64_t n_pixels, const ab_image_stats orig_stats[3], const double factors[3], int32_t has_scnr,
                              const ab_scnr_config *scnr, ab_color_plan *plan);
/* calibrate_and_scnr_cmd from its loaded originals (:112: orig_r, orig_g, orig_b and their ImageStats) to the encoder's input.
 * r, g, b: one size, host or device, any float-aligned address.  out_planes (required): three planes of that size, host or device,
 * any float-aligned address -- what becomes __composite_r / _g / _b: bit for bit ab_calibrate_channel's planes followed by
 * ab_apply_scnr_inplace, written by one kernel that multiplies and runs SCNR in registers (12 B read and 12 B written per pixel).
 * out_rgb8 (nullable): preview_rows x preview_cols x 3 bytes with the dims of ab_preview_dims(rows, cols, max_dim), host or device
 * (out_on_device) at ANY byte address: ab_render_rgb_preview's bytes with the linked stf x 3 and info->stats given (the ROUNDED byte
 * of apply_stf, stf.rs:96-100).  Above max_dim only the picked pixels are loaded.  An output may not overlap an input or another
 * output.  Mismatched dims, rows * cols >= 2^31, max_dim < 1 or a NULL out_planes -> AB_ERR_INVALID before anything touches the
 * device. */
AB_API int ab_calibrate_and_scnr(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_image_stats orig_stats[3],
                                 const double factors[3], int32_t has_scnr, const ab_scnr_config *scnr, int64_t max_dim, ab_plane_mut *out_planes,
                                 uint8_t *out_rgb8, int32_t out_on_device, ab_color_step_info *info);
/* blend_channels_cmd from its loaded channels on (blend.rs:143-205).  n_channels == 0 -> AB_ERR_INVALID "No channel paths provided"
 * (:139-141).  Channels of differing dims are resampled (bicubic, ab_resample_image) to the largest rows and the largest cols
 * (:148-169) into a workspace of the context: the originals are untouched.  out_planes (required): three planes of those dims
 * written by ab_blend_channels' kernel (:185; a weight whose channel_idx is out of range is skipped, a NaN reaches the planes), then
 * three statistics chains without a known range (:187-193), the linked STF and the preview as above.  Planes, statistics, STF and
 * bytes equal ab_blend_channels -> ab_compute_image_stats x 3 -> ab_compute_linked_stf -> ab_render_rgb_preview(stf x 3, stats).
 * At most 16 channels and 32 weights in range, as ab_blend_channels. */
AB_API int ab_blend_composite(ab_ctx *ctx, const ab_plane *channels, size_t n_channels, const ab_blend_weight *weights, size_t n_weights,
                              int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device, ab_blend_composite_info *info);
/* Host only: compute_auto_wb_cmd (color.rs:187-224) of the three channels' statistics.  The reference channel is R when stab_r <=
 * stab_g && stab_r <= stab_b, else B when stab_b <= stab_g, else G; the others are scaled to its median.max(1e-10).  It
 * restates the command, not rgb.rs: ab_select_wb_reference stays its own function (tests/test_color_step_cpu.py holds the factors of
 * the two equal on every branch and tie, which is a property of today's reference, not a contract). */
AB_API int ab_compute_auto_wb(const ab_image_stats *sr, const ab_image_stats *sg, const ab_image_stats *sb, ab_auto_wb *out);

/* ---- the compose wizard's stretch step: cmd/processing/stretch.rs (apply_arcsinh_stretch_cmd :15-43, arcsinh_stretch_composite_cmd
 * :94-124, masked_stretch_composite_cmd :135-221) and core/imaging/stretch.rs (arcsinh_stretch_rgb_with_stats :56-90) ------------------ */
/* arcsinh_stretch_rgb keeps two numbers of its three compute_image_stats calls: the smallest minimum and the largest maximum
 * (stretch.rs:72-78).  csrc/wizard_stretch.hip finds them in ONE streaming pass over the three planes (12 B per pixel: per channel the
 * extremes of the valid pixels, finite and > 1e-7, stats.rs:11-13; a channel without one contributes 0 to both, :46-48) and forms range,
 * the range < 1e-10 -> zeros decision and the correctly rounded 1 / range on the device, so no host round trip stands between the pass
 * and the stretch.  The per-pixel arithmetic is ab_arcsinh_stretch_with_stats' own (csrc/arcsinh_device.hpp).
 * masked_stretch_cmd (:46-91) needs no entry point of its own: it is ab_masked_stretch followed by ab_auto_stretch_preview of the
 * result.
 * The factor of the two commands is (factor as f32).clamp(1.0, 500.0) (:26, :102).  f32::clamp keeps a NaN; with a NaN factor
 * arcsinh_stretch_with_stats (core/imaging/stretch.rs:17-42) passes its early return (NaN.abs() < 1e-10 is false), forms
 * inv_denom = 1 / asinh(NaN) = NaN, and every FINITE pixel becomes NaN while a non-finite pixel becomes 0 (:35-36); a degenerate range
 * still yields zeros (:22-24).  The preview's bytes are then all 0 (NaN as u8) and the mono view's statistics are
 * ImageStats::default(). */
typedef struct {
    uint64_t rows, cols, preview_rows, preview_cols; /* RES_DIMENSIONS = [cols, rows] (stretch.rs:121) */
    float factor;                                    /* clamped_factor: RES_STRETCH_FACTOR (:119) */
    float global_min, global_max;                    /* what the three channels were normalised with */
    int32_t degenerate;                              /* global_max - global_min < 1e-10: planes and bytes are zeros */
} ab_arcsinh_composite_info;
typedef struct {
    uint64_t rows, cols;     /* RES_DIMENSIONS = [cols, rows] (stretch.rs:40) */
    float factor;            /* clamped_factor: RES_STRETCH_FACTOR (:38) */
    float data_min, data_max; /* stats.min as f32, stats.max as f32 of the input (core/imaging/stretch.rs:6-7) */
    int32_t degenerate;
    ab_image_stats stats;    /* of the STRETCHED plane: what render_and_save's auto_stretch_preview computes (cmd/common.rs:18-22) */
    ab_stf_params stf;       /* auto_stf(stats, default) */
} ab_arcsinh_view_info;
typedef enum {
    AB_MASK_PER_CHANNEL = 0,     /* "per_channel" (stretch.rs:197) */
    AB_MASK_SHARED_LUMINANCE = 1 /* "shared_luminance" (:174) */
} ab_mask_mode;
typedef struct {
    uint64_t rows, cols, preview_rows, preview_cols; /* RES_DIMENSIONS = [cols, rows] (stretch.rs:218) */
    ab_masked_stretch_result channels[3];            /* "channels": r, g, b (:166-170, :187-191) */
    uint64_t stars_masked;                           /* RES_STARS_MASKED: the shared mask's, or the sum of the three (:192) */
    double mask_coverage;                            /* RES_MASK_COVERAGE: the shared mask's, or (cr + cg + cb) / 3.0 (:193) */
    int32_t mask_mode;                               /* ab_mask_mode */
} ab_masked_stretch_composite_info;
/* Host only: the fold of stretch.rs:72-78 over three channels' statistics -- out_min_max[0] = (sr.min as f32).min(sg.min as f32)
 * .min(sb.min as f32), [1] likewise with max.  A caller that holds cached statistics passes the two values to the calls below and
 * skips their range pass.  A NULL argument -> AB_ERR_INVALID. */
AB_API int ab_arcsinh_rgb_range(const ab_image_stats st[3], float out_min_max[2]);
/* arcsinh_stretch_rgb_with_stats (core/imaging/stretch.rs:56-90).  r, g, b: one size, host or device, any float-aligned address.
 * global_min / global_max: both given (Some, Some) or both NULL (the range pass computes them: they equal
 * (float)ab_compute_image_stats(c).min / .max folded by ab_arcsinh_rgb_range).  |factor| < 1e-10: the outputs are copies of the inputs
 * (:65-67).  out_planes (required): three planes of that size, written by ONE kernel, bit for bit ab_arcsinh_stretch_with_stats x 3
 * with the global range.  out_min_max (nullable): the range used (0, 0 for the copies); fetching it is the call's one synchronisation
 * (device outputs and out_min_max NULL: none).  An output may not overlap an input or another output.  Mismatched dims,
 * rows * cols >= 2^31, a NULL out_planes or exactly one of global_min / global_max -> AB_ERR_INVALID before anything touches the
 * device. */
AB_API int ab_arcsinh_stretch_rgb(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const float *global_min, const float *global_max,
                                  float factor, float gamma, ab_plane_mut *out_planes, float out_min_max[2]);
/* arcsinh_stretch_composite_cmd (stretch.rs:94-124) from the loaded composite to the PNG encoder's input.  factor is clamped as the
 * command clamps it (a NaN: see above); gamma is 1.  out_planes (nullable: the command discards them): three planes as above.
 * out_rgb8 (nullable): preview_rows x preview_cols x 3 bytes with the dims of ab_preview_dims(rows, cols, max_dim), host or device
 * (out_on_device) at ANY byte address: ab_render_rgb_preview's bytes with stf NULL of the stretched planes, (v.clamp(0, 1) * 255f32)
 * as u8 (cmd/helpers.rs:243-245), stretched and packed in registers.  Above max_dim without out_planes only the picked pixels are
 * loaded and stretched after the range pass; with out_planes one kernel writes the planes and the bytes.  At most one
 * synchronisation, at the end; none with info NULL and device outputs.  Mismatched dims, rows * cols >= 2^31, max_dim < 1, both
 * outputs NULL, exactly one of global_min / global_max, or an output that overlaps an input or another output -> AB_ERR_INVALID
 * before anything touches the device. */
AB_API int ab_arcsinh_stretch_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, double factor, const float *global_min,
                                        const float *global_max, int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device,
                                        ab_arcsinh_composite_info *info);
/* apply_arcsinh_stretch_cmd (stretch.rs:15-43) with render_and_save (cmd/common.rs:209-240) up to the encoders, as one chain with one
 * synchronisation: the range pass on the plane, the stretch, then ab_auto_stretch_preview's device chain on the stretched plane.
 * out_plane (required): what write_fits_mono receives (ab_fits_encode_pixels encodes it).  out_u8 (nullable): rows x cols bytes, host
 * or device (out_on_device), any address -- render_and_save has no max_dim.  info (nullable). */
AB_API int ab_arcsinh_stretch_view(ab_ctx *ctx, const ab_plane *img, double factor, ab_plane_mut *out_plane, uint8_t *out_u8, int32_t out_on_device,
                                   ab_arcsinh_view_info *info);
/* masked_stretch_composite_cmd (stretch.rs:135-221) from the loaded composite to the PNG encoder's input: a composition.
 * shared_mask != 0 takes ab_masked_stretch_rgb_shared's route, otherwise ab_masked_stretch's three times; the stretched planes go to
 * out_planes (nullable) or into a workspace of the context, and the packer above turns them into out_rgb8 (nullable; not both).
 * Planes, results and bytes are bit for bit those calls followed by ab_render_rgb_preview with stf NULL.  The AB_ERR_INVALID cases
 * of ab_arcsinh_stretch_composite, and a NULL cfg. */
AB_API int ab_masked_stretch_composite(ab_ctx *ctx, const ab_plane *r, const ab_plane *g, const ab_plane *b, const ab_masked_stretch_config *cfg,
                                       int32_t shared_mask, int64_t max_dim, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device,
                                       ab_masked_stretch_composite_info *info);

/* ---- the compose wizard's background step: cmd/processing/background.rs (extract_background_cmd :17-94) and the mono preview of
 * cmd/common.rs (auto_stretch_preview :18-22 followed by save_preview_png :190-193) ------------------------------------------------------ */
/* save_preview_png picks downsample_nn::<1>'s pixels from auto_stretch_preview's bytes (cmd/common.rs:152-184): above max_dim every
 * pixel of the plane is stretched to a byte and all but the picked ones are dropped.  csrc/wizard_background.hip stretches only the
 * picked pixels.  downsample_nn's dims (dst = ((n as f64) * scale).round().max(1.0), scale = max_dim / max(width, height), :162-164;
 * both dims kept when both fit, :158-160) are cmd/helpers.rs:285-287's rule, so the preview's dims are ab_preview_dims' for a mono plane
 * as for a composite; its pick ((d as f64) * ratio).min((n - 1) as f64) as usize with ratio = n as f64 / dst as f64 (:166-176) is
 * helpers.rs:297-300's too. */
/* auto_stretch_preview (cmd/common.rs:18-22) followed by save_preview_png's pick (:190-193), as one chain: the statistics chain of
 * ab_auto_stretch_preview, then ONE kernel that reads the transform from HBM, loads only the picked pixels and writes their apply_stf
 * bytes (stf.rs:89-102).  img: host or device, any float-aligned address.  cfg NULL = AutoStfConfig::default().  out_u8 (required):
 * preview_rows x preview_cols bytes with the dims of ab_preview_dims(rows, cols, max_dim), host or device (out_on_device), ANY byte
 * address: byte for byte ab_auto_stretch_preview's output at the picked pixels.  out_stats / out_stf (nullable): what
 * ab_auto_stretch_preview returns.  At most one synchronisation, at the end; none with both NULL and a device output.  A NULL img or
 * out_u8, rows * cols >= 2^31, max_dim < 1 or an output that overlaps the input -> AB_ERR_INVALID before anything touches the device. */
AB_API int ab_auto_stretch_preview_sampled(ab_ctx *ctx, const ab_plane *img, const ab_auto_stf_config *cfg, int64_t max_dim, uint8_t *out_u8,
                                           int32_t out_on_device, ab_image_stats *out_stats, ab_stf_params *out_stf);
typedef struct {
    ab_background_info bg;                            /* RES_SAMPLE_COUNT, RES_RMS_RESIDUAL (background.rs:88-89) and the fitted coefficients */
    uint64_t rows, cols, preview_rows, preview_cols;  /* RES_DIMENSIONS = [cols, rows] (:91) */
    ab_image_stats corrected_stats; /* what the command caches with the plane (:73), which is what the preview computed (:53) */
    ab_image_stats model_stats;     /* of the model (:54) */
    ab_stf_params corrected_stf, model_stf; /* auto_stf(stats, default) of each */
} ab_background_step_info;
/* extract_background_cmd (background.rs:17-94) from its loaded plane to the two PNG encoders' inputs and the JSON, as one chain.
 * The command clamps grid_size to 3 ..= 32, poly_degree to 1 ..= 5 and iterations to 1 ..= 10 (:44-47, types/constants.rs:11-16) and
 * casts sigma_clip to f32; that stays on the caller's side, like ab_crop_config_default's defaults: cfg is taken as
 * ab_extract_background takes it (grid_size 1 .. 64, poly_degree 0 .. 5).
 * Sampling and fit are ab_extract_background's.  The surface kernel also reduces the minimum and maximum of the model's valid pixels
 * (finite, > 1e-7) and counts them; the copy that fetches the model's median carries them, and the model's statistics receive them as
 * compute_image_stats_with_known_range does (stats.rs:36-38), so above 4 000 000 pixels that chain has no range pass.  A degenerate
 * range (a constant model, no valid pixel) falls back to the scan inside the statistics; either way the result is bit for bit the
 * unknown-range chain's.  The corrected plane's statistics are computed ONCE (the command computes them at :53 and again at :73).
 * One launch writes both previews' bytes, only the picked pixels above max_dim.
 * out_corrected (required) and out_model (nullable: the model then lives in a workspace of the context): planes of the image's dims,
 * host or device.  out_corrected_u8 / out_model_u8 (each nullable): preview_rows x preview_cols bytes with the dims of
 * ab_preview_dims(rows, cols, max_dim), both host or both device (out_on_device), any byte address.  Planes, bytes, sample_count,
 * coeffs, statistics and STF parameters are bit for bit ab_extract_background followed by ab_auto_stretch_preview of each plane and
 * the pick.  Synchronisations: the cell medians, the global median and MAD, the model's median, and one at the end for info and the
 * host outputs; with a device image and device outputs nothing is staged through the host.
 * Progress ticks, cancel points and error strings are ab_extract_background's.  A NULL img, cfg or out_corrected, mismatched dims,
 * rows * cols >= 2^31, max_dim < 1 or an output that overlaps the input or another output -> AB_ERR_INVALID before anything touches
 * the device. */
AB_API int ab_background_step(ab_ctx *ctx, const ab_plane *img, const ab_background_config *cfg, int64_t max_dim, ab_plane_mut *out_corrected,
                              ab_plane_mut *out_model, uint8_t *out_corrected_u8, uint8_t *out_model_u8, int32_t out_on_device,
                              ab_background_step_info *info);

/* ---- the RGB Compose panel: cmd/compose/rgb.rs (compose_rgb_cmd :43-205) ----------------------------------------------------------------- */
typedef struct {
    ab_processed_rgb_info rgb;          /* what ab_process_rgb reports: dims, STFs, ChannelStats, offsets, scnr_applied, resampled, stats_wb */
    uint64_t preview_rows, preview_cols;
    int32_t lrgb_applied, l_resampled;  /* LRGB_APPLIED (:118-151); L was resampled to the composite's dims (:124-128) */
    ab_image_stats l_stats;             /* stf::analyze of the matched L (:133) and auto_stf of it (:134); zeros when L is absent or */
    ab_stf_params l_stf;                /* auto_stretch == 0 */
} ab_compose_rgb_info;
/* compose_rgb_cmd (cmd/compose/rgb.rs:43-205) from its loaded entries to the PNG encoder's input and the JSON, as one chain:
 * process_rgb (:99-104), the L branch (:118-151: resample_image when L's dims differ, stf::analyze + auto_stf + apply_stf_f32 when
 * auto_stretch, apply_lrgb with lrgb_lightness / lrgb_chrominance) and render_rgb_preview (:155-161).
 * l, r, g, b: nullable, host or device, any float-aligned address; at least two of r / g / b.  out_pre (required, [3]): what becomes
 * __composite_* / __composite_orig_* (:106-116) -- the white-balanced, aligned, pre-stretch planes at the largest channel's dims; the
 * channels land there directly.  out_planes (nullable, [3]): the final processed.r / g / b the command drops.  out_rgb8 (nullable):
 * preview_rows x preview_cols x 3 bytes with the dims of ab_preview_dims(rows, cols, max_dim), host or device (out_on_device), ANY
 * byte address.  info (nullable).
 * The pre-white-balance statistics visit the host once and only for WhiteBalance::Auto (ab_select_wb_reference); every other
 * statistic, the (linked) auto-STF, the compose-local transforms and L's transform are formed on the device.  One launch scales the
 * channels whose (mult as f32 - 1).abs() >= 1e-7 and writes merge_for_stf's plane when linked; one launch does the compose-local STF,
 * SCNR, L's stretch, apply_lrgb and the packing in registers -- only the picked pixels when out_planes is NULL on an image above
 * max_dim, two launches (planes, then the pick) when it is given there.  One final synchronisation fetches info and the host outputs
 * (none with info NULL and device outputs); registration keeps its own.
 * out_pre, out_planes, bytes, offsets, STFs and statistics are bit for bit ab_process_rgb -> ab_resample_image ->
 * ab_compute_image_stats -> ab_auto_stf -> ab_apply_stf_f32 -> ab_apply_lrgb -> ab_render_rgb_preview (stf NULL), except the
 * statistics' mean, which agrees to 1e-12 relative (the statistics routes sum in different orders).
 * Errors: "Need at least 2 channels for RGB compose (got N)" (rgb.rs:217) and "Channel dimension ratio ...x exceeds 8x limit..."
 * (:61-75) as ab_process_rgb; apply_lrgb's dims error cannot occur (L is resampled first).  A NULL cfg or out_pre, wrong output dims,
 * rows * cols >= 2^31, max_dim < 1 or an output that overlaps an input or another output -> AB_ERR_INVALID before anything touches
 * the device. */
AB_API int ab_compose_rgb(ab_ctx *ctx, const ab_plane *l, const ab_plane *r, const ab_plane *g, const ab_plane *b,
                          const ab_rgb_compose_config *cfg, float lrgb_lightness, float lrgb_chrominance, int64_t max_dim,
                          ab_plane_mut *out_pre, ab_plane_mut *out_planes, uint8_t *out_rgb8, int32_t out_on_device,
                          ab_compose_rgb_info *info);

/* ---- bench support: a plain float4 device copy, the measured HBM ceiling ---- */
AB_API int ab_bench_copy(ab_ctx *ctx, const float *src_dev, float *dst_dev, size_t n_floats);

/* ---- (e) multi-GPU: SURVEY.md 8e -------------------------------------------------------------- */
/* The reference is one process on one machine (rayon); what shards is its per-pixel loop (combine.rs:160-182, rows are
 * independent) and its frame list.  One ab_ctx + one ab_comm rank per GPU; collectives are RCCL (xGMI inside a node),
 * enqueued on the context's stream.  librccl is dlopen'ed on first use: the rest of the library works without it. */
#define AB_COMM_ID_BYTES 128
typedef enum { AB_DT_I32 = 0, AB_DT_U32 = 1, AB_DT_I64 = 2, AB_DT_U64 = 3, AB_DT_F32 = 4, AB_DT_F64 = 5 } ab_dtype;
typedef enum { AB_RED_SUM = 0, AB_RED_MAX = 1, AB_RED_MIN = 2 } ab_redop;
/* multi-process: rank 0 makes the id, the host carries it to the other processes, every rank joins */
AB_API int ab_comm_get_unique_id(uint8_t id[AB_COMM_ID_BYTES]);
AB_API int ab_comm_init_rank(ab_ctx *ctx, const uint8_t id[AB_COMM_ID_BYTES], int nranks, int rank, ab_comm **out);
/* single process, n contexts on n distinct devices: out_comms[i] is rank i, bound to ctxs[i]'s device.  Drive each
 * context from its own host thread, or bracket the per-device calls with ab_comm_group_start / _end. */
AB_API int ab_comm_init_all(ab_ctx *const *ctxs, int n, ab_comm **out_comms);
/* HOST-STAGED transport (no RCCL, ranks may share a device): collectives go through the POSIX shared-memory segment
 * /abcomm_<name> -- every rank of the job passes the same name; blocks until all nranks joined.  The same entry points
 * work on it; a collective then returns when its result is in device memory.  What a one-GPU box runs the N > 1 paths
 * on (tests/test_gpu_multirank.py) and a host without librccl falls back to.  AB_COMM_HOST_SLOT_MB (default 4) = the
 * per-rank staging window. */
AB_API int ab_comm_init_rank_host(ab_ctx *ctx, const char *name, int nranks, int rank, ab_comm **out);
AB_API int ab_comm_is_host(const ab_comm *comm);
/* Failure handling.  ab_comm_agree: every rank passes the status of its local work; AB_OK comes back only if every rank
 * passed AB_OK -- a failed rank gets its own status, the others AB_ERR_CANCELLED (a peer was cancelled) or AB_ERR_COMM.
 * Every sharded entry point below calls it BEFORE its data collectives, so one failing rank fails the call everywhere and
 * the communicator stays usable.  Waits on collectives are bounded by ab_comm_set_timeout_ms (default: AB_COMM_TIMEOUT_MS
 * or 300 000): a peer that died turns into AB_ERR_COMM and a dead communicator, not a hang.  ab_comm_abort gives up at
 * once (host transport: peers blocked in a collective return AB_ERR_COMM immediately; RCCL: ncclCommAbort); afterwards
 * every collective on the handle fails with AB_ERR_COMM and only ab_comm_destroy is useful. */
AB_API int ab_comm_agree(ab_ctx *ctx, ab_comm *comm, int local_status);
AB_API int ab_comm_abort(ab_comm *comm);
AB_API int ab_comm_set_timeout_ms(ab_comm *comm, int64_t ms);
AB_API void ab_comm_destroy(ab_comm *comm);
AB_API int ab_comm_rank(const ab_comm *comm);  /* a NULL communicator is a world of one: rank 0 */
AB_API int ab_comm_size(const ab_comm *comm);  /* ... of size 1 */
AB_API uint64_t ab_comm_collectives_issued(const ab_comm *comm);
AB_API int ab_comm_group_start(void);
AB_API int ab_comm_group_end(void);
/* in-place all-reduce of `count` elements on the context's stream (RCCL: asynchronous; host-staged: done on return) */
AB_API int ab_comm_allreduce(ab_ctx *ctx, ab_comm *comm, void *buf_dev, size_t count, int dtype /* ab_dtype */, int op /* ab_redop */);
/* recv_dev = size x bytes_per_rank bytes, rank r's block at r * bytes_per_rank */
AB_API int ab_comm_allgather(ab_ctx *ctx, ab_comm *comm, const void *send_dev, void *recv_dev, size_t bytes_per_rank);
AB_API int ab_comm_broadcast(ab_ctx *ctx, ab_comm *comm, void *buf_dev, size_t bytes, int root);

/* partitions: rows [row0, row0 + nrows) (ceil(rows / nranks) per rank, trailing bands shorter or empty) and frames
 * [f0, f0 + nf) (contiguous, balanced) of rank `rank` */
AB_API int ab_shard_rows(int64_t rows, int nranks, int rank, int64_t *row0, int64_t *nrows);
AB_API int ab_shard_frames(size_t n_frames, int nranks, int rank, size_t *f0, size_t *nf);
/* what rank `rank` must hold of every TARGET frame to warp its band (ab_shard_rows over out_rows) with the n transforms
 * (n x 6 doubles, e.g. ab_register_frames_sharded's estimates): the hull of ab_warp_source_rows = its rows + the halo the
 * transform set needs (about max |ty| + |c| cols + 2 rows either side) */
AB_API int ab_shard_source_rows(const double *transforms, size_t n, int64_t src_rows, int64_t src_cols, int64_t out_rows, int64_t out_cols,
                                int nranks, int rank, int64_t *src_row0, int64_t *src_nrows);

/* ROW-BAND (exact) sharding of stack_images' per-pixel loop (combine.rs:160-182): rows [row0, row0 + out_band->rows) of
 * the stack of ALL n frames -- the reference's single-level estimator restricted to a band, bit for bit.  Device planes. */
AB_API int ab_stack_sigma_clip_rows(ab_ctx *ctx, const ab_plane *planes, size_t n, const ab_stack_config *cfg, int64_t row0,
                                    ab_plane_mut *out_band, uint64_t *out_rejected);
/* the same with the band = this rank's share (ab_shard_rows over the minimum frame dims, combine.rs:104-113) and
 * StackResult.rejected_pixels summed over the ranks (one u64 all-reduce) */
AB_API int ab_stack_sigma_clip_rowband(ab_ctx *ctx, ab_comm *comm, const ab_plane *planes, size_t n, const ab_stack_config *cfg,
                                       ab_plane_mut *out_band, uint64_t *out_rejected_total);
/* FRAME-SHARDED two-level stack (BASELINE configs[3]): ab_stack_sigma_clip_partial over this rank's frames ->
 * all-reduce(sum f64, count u32) -> ab_stack_finalize_partial.  `out` (device) is the full image on every rank.  NOT the
 * reference's estimator (a median over all frames is not decomposable); checker: orc_stack_partial_noalign. */
AB_API int ab_stack_sigma_clip_sharded(ab_ctx *ctx, ab_comm *comm, const ab_plane *local_planes, size_t n_local,
                                       const ab_stack_config *cfg, ab_plane_mut *out, uint64_t *out_rejected_total);
/* the last ab_stack_sigma_clip_sharded of this context: the span of its partial stacks on the context's stream, and the time inside
 * its all-reduces + divisions (they run chunk by chunk on a second stream while the next chunk is stacked: with overlap the two add
 * up to more than the call took).  Blocks until that call's work is done.  bench.py: stage_ms.comm_* */
AB_API int ab_stack_sharded_last_ms(ab_ctx *ctx, float *stack_ms, float *comm_ms);
/* every rank's band -> the full image on every rank (one broadcast per rank inside one RCCL group) */
AB_API int ab_allgather_rows(ab_ctx *ctx, ab_comm *comm, const ab_plane *band, ab_plane_mut *full);
/* align_channel_affine(reference, targets[i]) for i < n, target i estimated on rank i mod size, all n results on every
 * rank (exchanged bit for bit as integer words); targets a rank does not own are not read there */
AB_API int ab_register_frames_sharded(ab_ctx *ctx, ab_comm *comm, const ab_plane *reference, const ab_plane *targets, size_t n,
                                      int num_threads, ab_affine_align_result *out);
/* The row-band scheme's registration as ONE call (pair.rs:41-77 per target): this rank's rows [row0, row0 + out_bands[i].rows)
 * of warp_image(target i, its transform) for every i.  targets[i] holds rows [target_row0[i], + targets[i].rows) of target i
 * (target_row0 NULL = whole frames): whole for the targets this rank estimates (i mod size == rank), of the others at least the rows
 * its band reads (ab_shard_source_rows).  Own frames are warped as they are fitted, overlapped with the remaining estimates; then the
 * estimates are exchanged and the other frames warped from their bands.  out[i] / the pixels equal ab_register_frames_sharded +
 * ab_warp_image_rows(_from_band) bit for bit. */
AB_API int ab_align_pairs_affine_rowband(ab_ctx *ctx, ab_comm *comm, const ab_plane *reference, const ab_plane *targets, const int64_t *target_row0,
                                         size_t n, int num_threads, int64_t row0, ab_affine_align_result *out, ab_plane_mut *out_bands);
/* compute_image_stats (stats.rs:15-210) of an image whose rows are spread over the ranks: `band` = this rank's rows,
 * total_rows = the whole image's.  min / max, counts and the 65 536-bin histograms are all-reduced between the passes
 * (integers: every bin equals the single-GPU bin); every rank receives the whole image's statistics. */
AB_API int ab_compute_image_stats_sharded(ab_ctx *ctx, ab_comm *comm, const ab_plane *band, int64_t total_rows, ab_image_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* ASTROBURST_HIP_H */
