//! Safe wrappers over `sys` (bindings/sys.rs, generated from include/astroburst_hip.h) for the AstroBurst backend:
//! drop-ins for the `core::*` functions the Tauri commands call.  Place this directory at `src-tauri/src/hip/`.
//!
//! NOT compiled in the repository that ships it (that image has no Rust toolchain); `sys.rs` is checked field by field
//! against the C header and this file is checked to wrap every entry point of the header (tests/test_abi_cpu.py); the rest is
//! reviewed source.  Every function keeps the argument meaning, the result type and the error strings of the `core::*`
//! function it replaces (cited per function) and takes the calling thread's `&Hip` first, so a command body changes by one
//! path (`core::imaging::curves::apply_curve(..)` -> `hip::apply_curve(h, ..)`); INTEGRATION.md holds the command hunks.
//!
//! Host or device: every plane argument is `&impl PlaneSrc` -- an `Array2<f32>` (staged through the library's pinned buffer,
//! one PCIe crossing each way) or a `DevicePlane` already in HBM -- and every `*_into` variant writes an `impl PlaneDst`.
//! `device::DEVICE_CACHE` mirrors the pinned keys of GLOBAL_IMAGE_CACHE so that consecutive commands keep their planes in HBM.
//!
//! Threading: one `Hip` per blocking thread (`blocking_cmd!`, cmd/common.rs:345-352) -- an `ab_ctx` owns a stream and
//! scratch and is not shared.  The library never unwinds into Rust (every entry point is a C++ function-try-block) and
//! never aborts; failures are status codes + `ab_last_error`.
#![allow(dead_code)]
pub mod device;
pub mod sys;

use anyhow::{anyhow, bail, Result};
use ndarray::{Array2, Array3};
use std::cell::RefCell;
use std::ffi::{c_void, CStr, CString};
use std::os::raw::c_char;

pub use device::{DevicePlane, PlaneDst, PlaneSrc, DEVICE_CACHE};

use crate::core::alignment::affine::{AffineAlignMethod, AffineAlignResult, AffineTransform};
use crate::core::alignment::pair::AlignPairResult;
use crate::core::alignment::phase_correlation::PhaseCorrelationResult;
use crate::core::analysis::fft::FftResult;
use crate::core::analysis::star_detection::{DetectedStar, DetectionResult};
use crate::core::analysis::subframe::{SubframeMetrics, SubframeWeightConfig};
use crate::core::astrometry::spcc::{SpccConfig, SpccResult, WhiteReference};
use crate::core::compose::channel_blend::BlendWeight;
use crate::core::cube::eager::GlobalCubeStats;
use crate::core::compose::drizzle_rgb::ProcessedDrizzleRgb;
use crate::core::compose::rgb::ProcessedRgb;
use crate::core::imaging::background::{BackgroundConfig, BackgroundResult};
use crate::core::imaging::calibration_pipeline::{
    BatchChannelStats, BatchPipelineConfig, BatchPipelineResult, BatchPipelineStats, BatchStackConfig, CalibrationMasters, ChannelInput,
};
use crate::core::imaging::curves::LevelsParams;
use crate::core::imaging::masked_stretch::{MaskedStretchConfig, MaskedStretchResult, MaskedStretchRgbResult};
use crate::core::imaging::psf_estimation::{PsfEstimationConfig, PsfResult, StarCandidate};
use crate::core::imaging::star_mask::{StarMaskConfig, StarMaskResult};
use crate::core::imaging::wavelet::{WaveletConfig, WaveletResult};
use crate::core::stacking::calibration::CalibrationConfig;
use crate::core::synth::noise::NoiseParams;
use crate::core::synth::pipeline::{FieldType, PsfType, SynthConfig};
use crate::core::synth::star_field::{FieldConfig, Star};
use crate::infra::progress::ProgressHandle;
use crate::types::compose::{AlignMethod, ChannelStats, DimensionHarmonize, DrizzleRgbConfig, RgbComposeConfig, WhiteBalance};
use crate::types::image::{AutoStfConfig, ImageStats, ScnrConfig, ScnrMethod, StfParams};
use crate::types::stacking::{AlignmentMethod, DrizzleConfig, DrizzleKernel, DrizzleResult, RLConfig, RLResult, StackConfig, StackResult};

pub struct Hip {
    pub(crate) ctx: *mut sys::ab_ctx,
}
unsafe impl Send for Hip {}
// `&Hip` crosses into the scoped rank threads of `on_all_gpus`; each rank only ever touches its OWN context there
unsafe impl Sync for Hip {}

thread_local! { static HIP: RefCell<Option<Hip>> = RefCell::new(None); }

/// the calling thread's context on device 0 (created on first use)
pub fn with_hip<T>(f: impl FnOnce(&Hip) -> Result<T>) -> Result<T> {
    HIP.with(|slot| {
        let mut slot = slot.borrow_mut();
        if slot.is_none() {
            *slot = Some(Hip::new(0)?);
        }
        f(slot.as_ref().unwrap())
    })
}

impl Hip {
    pub fn new(device: i32) -> Result<Self> {
        let mut ctx = std::ptr::null_mut();
        match unsafe { sys::ab_ctx_create(device, &mut ctx) } {
            sys::AB_OK => Ok(Self { ctx }),
            sys::AB_ERR_NO_DEVICE => bail!("no gfx950 (MI355X) device"),
            rc => bail!("ab_ctx_create failed ({rc})"),
        }
    }

    pub(crate) fn check(&self, rc: i32) -> Result<()> {
        if rc == sys::AB_OK {
            return Ok(());
        }
        let msg = unsafe { CStr::from_ptr(sys::ab_last_error(self.ctx)) }.to_string_lossy().into_owned();
        if rc == sys::AB_ERR_CANCELLED {
            return Err(crate::types::error::AppError::Cancelled.into()); // background.rs:80-82
        }
        Err(anyhow!(msg)) // the reference's own strings, e.g. "No images to stack"
    }

    /// (name, compute units, HBM bytes)
    pub fn device_info(&self) -> Result<(String, i32, u64)> {
        let mut name = [0 as c_char; 128];
        let (mut cus, mut hbm) = (0i32, 0u64);
        self.check(unsafe { sys::ab_device_info(self.ctx, name.as_mut_ptr(), name.len(), &mut cus, &mut hbm) })?;
        Ok((unsafe { CStr::from_ptr(name.as_ptr()) }.to_string_lossy().into_owned(), cus, hbm))
    }

    /// release the device memory the context has grown for its calls (workspaces, scratch, the staging area of host frames);
    /// the context stays usable -- for a long-lived command thread after a large batch
    pub fn trim(&self) -> Result<()> {
        self.check(unsafe { sys::ab_ctx_trim(self.ctx) })
    }

    /// how often a fast path handed over to its exact fallback (same results, more time) since the context was created or last
    /// reset, indexed by the `sys::AB_FB_*` constants (frames redone in full, crowded tiles, short / close selections, declined
    /// background tiles, aborted resident statistics) -- for the host's log: a session whose registration suddenly takes twice as
    /// long shows up here, not in the pixels
    pub fn fallback_counts(&self, reset: bool) -> Result<[u64; sys::AB_FB_COUNT as usize]> {
        let mut out = [0u64; sys::AB_FB_COUNT as usize];
        self.check(unsafe { sys::ab_ctx_fallback_counts(self.ctx, out.as_mut_ptr(), out.len(), reset as i32) })?;
        Ok(out)
    }

    pub fn synchronize(&self) -> Result<()> {
        self.check(unsafe { sys::ab_ctx_synchronize(self.ctx) })
    }
    /// run on a HIP stream the host owns (e.g. one shared with another library); `reset_stream` returns to the context's own
    pub fn set_stream(&self, hip_stream: *mut c_void) -> Result<()> {
        self.check(unsafe { sys::ab_ctx_set_stream(self.ctx, hip_stream) })
    }
    pub fn reset_stream(&self) -> Result<()> {
        self.check(unsafe { sys::ab_ctx_reset_stream(self.ctx) })
    }
    pub fn stream(&self) -> *mut c_void {
        unsafe { sys::ab_ctx_get_stream(self.ctx) }
    }
    /// duration of the stack kernels of the last stack call on this context (HIP events around the launches)
    pub fn stack_last_kernel_ms(&self) -> Result<f32> {
        let mut ms = 0f32;
        self.check(unsafe { sys::ab_stack_last_kernel_ms(self.ctx, &mut ms) })?;
        Ok(ms)
    }

    /// Forward the library's stage ticks to a `ProgressHandle` (infra/progress.rs:39-74) for the duration of `f`, and the
    /// handle's cancel flag to the library: the reference polls `p.is_cancelled()` between stages (background.rs:80-91); here
    /// every tick -- the library ticks at those same stage boundaries -- forwards a pending cancel, and the library's own
    /// check at the next boundary returns AB_ERR_CANCELLED.
    pub fn with_progress<T>(&self, progress: Option<&ProgressHandle>, f: impl FnOnce() -> Result<T>) -> Result<T> {
        struct User<'a> {
            ctx: *mut sys::ab_ctx,
            p: &'a ProgressHandle,
        }
        unsafe extern "C" fn tick(stage: *const c_char, _cur: u64, total: u64, user: *mut c_void) {
            let u = &*(user as *const User);
            if u.p.is_cancelled() {
                sys::ab_ctx_request_cancel(u.ctx);
            }
            u.p.set_total(total);
            u.p.tick_with_stage(&CStr::from_ptr(stage).to_string_lossy());
        }
        let user = progress.map(|p| User { ctx: self.ctx, p });
        if let Some(u) = user.as_ref() {
            if u.p.is_cancelled() {
                unsafe { sys::ab_ctx_request_cancel(self.ctx) };
            }
            unsafe { sys::ab_ctx_set_progress_cb(self.ctx, Some(tick), u as *const User as *mut c_void) };
        }
        let r = f();
        unsafe {
            sys::ab_ctx_set_progress_cb(self.ctx, None, std::ptr::null_mut());
            sys::ab_ctx_clear_cancel(self.ctx);
        }
        r
    }
}

impl Drop for Hip {
    fn drop(&mut self) {
        unsafe { sys::ab_ctx_destroy(self.ctx) }
    }
}

/// "astroburst-hip x.y (gfx950)"
pub fn version() -> String {
    unsafe { CStr::from_ptr(sys::ab_version()) }.to_string_lossy().into_owned()
}
/// BatchStackConfig::default() / SubframeWeightConfig::default() as the LIBRARY holds them (calibration_pipeline.rs:27-37,
/// subframe.rs:36-49): a start-up assertion that both sides agree costs nothing and catches a drifted default
pub fn library_defaults_match() -> bool {
    let mut b: sys::ab_batch_stack_config = unsafe { std::mem::zeroed() };
    let mut w: sys::ab_subframe_weight_config = unsafe { std::mem::zeroed() };
    unsafe {
        sys::ab_batch_stack_config_default(&mut b);
        sys::ab_subframe_weight_config_default(&mut w);
    }
    let (db, dw) = (BatchStackConfig::default(), SubframeWeightConfig::default());
    b.sigma_low == db.sigma_low && b.sigma_high == db.sigma_high && b.max_iterations == db.max_iterations as u64 && (b.normalize_before_stack != 0) == db.normalize_before_stack
        && w.fwhm_weight == dw.fwhm_weight && w.eccentricity_weight == dw.eccentricity_weight && w.snr_weight == dw.snr_weight && w.noise_weight == dw.noise_weight
        && w.max_fwhm == dw.max_fwhm && w.max_eccentricity == dw.max_eccentricity && w.min_snr == dw.min_snr && w.min_stars == dw.min_stars as u64
}

// ---- small conversions -------------------------------------------------------------------------------------------------------
fn stats_to_sys(st: &ImageStats) -> sys::ab_image_stats {
    sys::ab_image_stats { min: st.min, max: st.max, median: st.median, mad: st.mad, sigma: st.sigma, mean: st.mean, valid_count: st.valid_count }
}
fn stats_from_sys(st: &sys::ab_image_stats) -> ImageStats {
    ImageStats { min: st.min, max: st.max, median: st.median, mad: st.mad, sigma: st.sigma, mean: st.mean, valid_count: st.valid_count }
}
fn stf_to_sys(p: &StfParams) -> sys::ab_stf_params {
    sys::ab_stf_params { shadow: p.shadow, midtone: p.midtone, highlight: p.highlight }
}
fn stf_from_sys(p: &sys::ab_stf_params) -> StfParams {
    StfParams { shadow: p.shadow, midtone: p.midtone, highlight: p.highlight }
}
fn stack_cfg(c: &StackConfig) -> sys::ab_stack_config {
    sys::ab_stack_config { sigma_low: c.sigma_low, sigma_high: c.sigma_high, max_iterations: c.max_iterations as u32, align: c.align as i32 }
}
fn scnr_to_sys(c: &ScnrConfig) -> sys::ab_scnr_config {
    sys::ab_scnr_config { method: matches!(c.method, ScnrMethod::MaximumNeutral) as i32, amount: c.amount, preserve_luminance: c.preserve_luminance as i32 }
}
fn star_from_sys(s: &sys::ab_detected_star) -> DetectedStar {
    DetectedStar { x: s.x, y: s.y, flux: s.flux, fwhm: s.fwhm, eccentricity: s.eccentricity, peak: s.peak, npix: s.npix as usize, snr: s.snr }
}
fn star_to_sys(s: &DetectedStar) -> sys::ab_detected_star {
    sys::ab_detected_star { x: s.x, y: s.y, flux: s.flux, fwhm: s.fwhm, eccentricity: s.eccentricity, peak: s.peak, snr: s.snr, npix: s.npix as u64 }
}
fn align_from_sys(r: &sys::ab_affine_align_result) -> AffineAlignResult {
    let t = r.transform;
    AffineAlignResult {
        transform: AffineTransform { a: t[0], b: t[1], tx: t[2], c: t[3], d: t[4], ty: t[5] },
        matched_stars: r.matched_stars as usize,
        inliers: r.inliers as usize,
        residual_px: r.residual_px,
        method: match r.method {
            0 => AffineAlignMethod::Affine,
            1 => AffineAlignMethod::Rigid,
            2 => AffineAlignMethod::PhaseCorrelation,
            _ => AffineAlignMethod::Identity,
        },
    }
}
fn num_threads() -> i32 {
    rayon::current_num_threads() as i32 // the RANSAC draws are partitioned and seeded per rayon worker (affine.rs:410-416)
}
fn opt_plane<P: PlaneSrc>(p: Option<&P>) -> Option<sys::ab_plane> {
    p.map(|x| x.ab())
}
fn opt_ptr(p: &Option<sys::ab_plane>) -> *const sys::ab_plane {
    p.as_ref().map_or(std::ptr::null(), |x| x as *const _)
}
fn masked_cfg(c: &MaskedStretchConfig) -> sys::ab_masked_stretch_config {
    sys::ab_masked_stretch_config {
        iterations: c.iterations,
        target_background: c.target_background,
        mask_growth: c.mask_growth,
        mask_softness: c.mask_softness,
        luminance_protect: c.luminance_protect as i32,
        luminance_ceiling: c.luminance_ceiling,
        protection_amount: c.protection_amount,
        convergence_threshold: c.convergence_threshold,
    }
}
fn masked_res(image: Array2<f32>, r: &sys::ab_masked_stretch_result) -> MaskedStretchResult {
    MaskedStretchResult {
        image,
        iterations_run: r.iterations_run,
        final_background: r.final_background,
        stars_masked: r.stars_masked,
        mask_coverage: r.mask_coverage,
        converged: r.converged != 0,
    }
}
fn mask_cfg(c: &StarMaskConfig) -> sys::ab_star_mask_config {
    sys::ab_star_mask_config {
        growth_factor: c.growth_factor,
        softness: c.softness,
        detection_sigma: c.detection_sigma,
        min_fwhm: c.min_fwhm,
        max_fwhm: c.max_fwhm,
        luminance_protect: c.luminance_protect as i32,
        luminance_ceiling: c.luminance_ceiling,
    }
}

// ---- a1 / a2  core/stacking/combine.rs -----------------------------------------------------------------------------------------
/// drop-in for core::stacking::combine::stack_images (combine.rs:94-193)
pub fn stack_images(hip: &Hip, images: &[Array2<f32>], config: &StackConfig) -> Result<StackResult> {
    if images.is_empty() {
        bail!("No images to stack"); // combine.rs:98-100
    }
    let rows = images.iter().map(|i| i.nrows()).min().unwrap();
    let cols = images.iter().map(|i| i.ncols()).min().unwrap();
    let planes: Vec<_> = images.iter().map(|i| i.ab()).collect();
    let mut out = Array2::<f32>::zeros((rows, cols));
    let mut po = out.ab_mut();
    let mut offs = vec![0i32; 2 * images.len()];
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_images(hip.ctx, planes.as_ptr(), planes.len(), &stack_cfg(config), &mut po, offs.as_mut_ptr(), &mut rejected) })?;
    Ok(StackResult { image: out, frame_count: images.len(), rejected_pixels: rejected, offsets: offs.chunks(2).map(|c| (c[0], c[1])).collect() })
}

/// the per-pixel loop of stack_images alone (combine.rs:160-182; `sigma_clip_combine` :14-92 per pixel) on frames that are
/// already registered, host or device, into a host or device plane; returns StackResult.rejected_pixels
pub fn stack_sigma_clip_into<P: PlaneSrc>(hip: &Hip, frames: &[P], config: &StackConfig, out: &mut impl PlaneDst) -> Result<u64> {
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_sigma_clip(hip.ctx, planes.as_ptr(), planes.len(), &stack_cfg(config), &mut out.ab_mut(), &mut rejected) })?;
    Ok(rejected)
}
/// rejected_pixels of the last stack on this context when the call itself was made without waiting for it
pub fn stack_last_rejected(hip: &Hip) -> Result<u64> {
    let mut r = 0u64;
    hip.check(unsafe { sys::ab_stack_last_rejected(hip.ctx, &mut r) })?;
    Ok(r)
}
/// two-level estimator for more frames than one GPU holds: per-shard survivor sums and counts, then one divide
pub fn stack_sigma_clip_partial(hip: &Hip, frames: &[DevicePlane], config: &StackConfig, rows: usize, cols: usize, sum_dev: *mut f64, cnt_dev: *mut u32) -> Result<u64> {
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_sigma_clip_partial(hip.ctx, planes.as_ptr(), planes.len(), &stack_cfg(config), rows as i64, cols as i64, sum_dev, cnt_dev, &mut rejected) })?;
    Ok(rejected)
}
pub fn stack_finalize_partial(hip: &Hip, sum_dev: *const f64, cnt_dev: *const u32, out: &mut DevicePlane) -> Result<()> {
    let (r, c) = out.dims();
    hip.check(unsafe { sys::ab_stack_finalize_partial(hip.ctx, sum_dev, cnt_dev, (r * c) as i64, out.ab_mut().data) })
}
/// stack_images' per-pixel loop fed straight from FITS data units in HBM (decode_pixels fused into the gather, reader.rs:36-83)
pub fn stack_sigma_clip_raw(hip: &Hip, raw_planes_dev: &[*const c_void], bitpix: i64, bscale: f64, bzero: f64, config: &StackConfig, out: &mut DevicePlane) -> Result<u64> {
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_sigma_clip_raw(hip.ctx, raw_planes_dev.as_ptr(), raw_planes_dev.len(), bitpix, bscale, bzero, &stack_cfg(config), &mut out.ab_mut(), &mut rejected) })?;
    Ok(rejected)
}

// ---- a3 / a4 / a5  core/stacking/align.rs, core/alignment/affine.rs --------------------------------------------------------------
/// drop-in for core::stacking::align::shift_image_subpixel (align.rs:36-70)
pub fn shift_image_subpixel(hip: &Hip, image: &impl PlaneSrc, dy: f64, dx: f64) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(image.dims());
    hip.check(unsafe { sys::ab_shift_image_subpixel(hip.ctx, &image.ab(), dy, dx, &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for core::alignment::affine::warp_image (affine.rs:663-690)
pub fn warp_image(hip: &Hip, image: &impl PlaneSrc, t: &AffineTransform, out_rows: usize, out_cols: usize) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros((out_rows, out_cols));
    warp_image_into(hip, image, t, &mut out)?;
    Ok(out)
}
pub fn warp_image_into(hip: &Hip, image: &impl PlaneSrc, t: &AffineTransform, out: &mut impl PlaneDst) -> Result<()> {
    let m = [t.a, t.b, t.tx, t.c, t.d, t.ty];
    hip.check(unsafe { sys::ab_warp_image(hip.ctx, &image.ab(), m.as_ptr(), &mut out.ab_mut()) })
}
/// rows [row0, row0 + band.rows) of warp_image's output (a GPU's row band of a registered frame)
pub fn warp_image_rows(hip: &Hip, image: &impl PlaneSrc, t: &AffineTransform, out_rows: usize, row0: usize, band: &mut impl PlaneDst) -> Result<()> {
    let m = [t.a, t.b, t.tx, t.c, t.d, t.ty];
    hip.check(unsafe { sys::ab_warp_image_rows(hip.ctx, &image.ab(), m.as_ptr(), out_rows as i64, row0 as i64, &mut band.ab_mut()) })
}

/// the same with the source given as rows [src_row0, src_row0 + src_band.rows) of a `src_rows`-row frame: a GPU of the row-band
/// scheme holds its rows of every target + the halo `shard_source_rows` names, not the frame set
pub fn warp_image_rows_from_band(hip: &Hip, src_band: &impl PlaneSrc, src_row0: usize, src_rows: usize, t: &AffineTransform, out_rows: usize,
                                 row0: usize, band: &mut impl PlaneDst) -> Result<()> {
    let m = [t.a, t.b, t.tx, t.c, t.d, t.ty];
    hip.check(unsafe {
        sys::ab_warp_image_rows_from_band(hip.ctx, &src_band.ab(), src_row0 as i64, src_rows as i64, m.as_ptr(), out_rows as i64, row0 as i64, &mut band.ab_mut())
    })
}
/// source rows (first, count) that output rows [row0, row0 + nrows) of warp_image read (affine.rs:663-690, sampling.rs:48-80)
/// (context-free: a non-zero status -- negative dimensions, a band outside the output -- has no message to fetch, so it is named here;
/// it must not become "(0, 0): no source rows needed")
pub fn warp_source_rows(t: &AffineTransform, src_rows: usize, src_cols: usize, out_cols: usize, row0: usize, nrows: usize) -> Result<(usize, usize)> {
    let m = [t.a, t.b, t.tx, t.c, t.d, t.ty];
    let (mut s0, mut sn) = (0i64, 0i64);
    let rc = unsafe { sys::ab_warp_source_rows(m.as_ptr(), src_rows as i64, src_cols as i64, out_cols as i64, row0 as i64, nrows as i64, &mut s0, &mut sn) };
    if rc != 0 {
        bail!("warp_source_rows: invalid arguments (status {rc}: src {src_rows}x{src_cols}, out cols {out_cols}, rows {row0}+{nrows})");
    }
    Ok((s0 as usize, sn as usize))
}

// ---- a8  core/alignment/phase_correlation.rs --------------------------------------------------------------------------------------
/// drop-in for phase_correlate (phase_correlation.rs:22-89)
pub fn phase_correlate(hip: &Hip, reference: &impl PlaneSrc, target: &impl PlaneSrc) -> Result<PhaseCorrelationResult> {
    let mut r = sys::ab_phase_correlation_result { dx: 0.0, dy: 0.0, confidence: 0.0 };
    hip.check(unsafe { sys::ab_phase_correlate(hip.ctx, &reference.ab(), &target.ab(), &mut r) })?;
    Ok(PhaseCorrelationResult { dx: r.dx, dy: r.dy, confidence: r.confidence })
}

// ---- a7  core/analysis/star_detection.rs -----------------------------------------------------------------------------------------
/// drop-in for estimate_background (star_detection.rs:32-84)
pub fn estimate_background(hip: &Hip, image: &impl PlaneSrc, tile_size: usize) -> Result<(f64, f64)> {
    let (mut med, mut sig) = (0.0, 1.0);
    hip.check(unsafe { sys::ab_estimate_background(hip.ctx, &image.ab(), tile_size as i64, &mut med, &mut sig) })?;
    Ok((med, sig))
}
/// drop-in for detect_stars (star_detection.rs:86-258)
pub fn detect_stars(hip: &Hip, image: &impl PlaneSrc, sigma_threshold: f64) -> Result<DetectionResult> {
    let (rows, cols) = image.dims();
    let mut cap = 4096usize;
    loop {
        let mut buf: Vec<sys::ab_detected_star> = Vec::with_capacity(cap);
        let (mut count, mut total) = (0usize, 0usize);
        let (mut bg_median, mut bg_sigma) = (0.0, 1.0);
        hip.check(unsafe { sys::ab_detect_stars(hip.ctx, &image.ab(), sigma_threshold, buf.as_mut_ptr(), cap, &mut count, &mut total, &mut bg_median, &mut bg_sigma) })?;
        if total > cap {
            cap = total; // a crowded field: once more with room for every star
            continue;
        }
        unsafe { buf.set_len(count) };
        return Ok(DetectionResult {
            stars: buf.iter().map(star_from_sys).collect(),
            background_median: bg_median,
            background_sigma: bg_sigma,
            threshold_sigma: sigma_threshold,
            image_width: cols,
            image_height: rows,
        });
    }
}

// ---- a6  core/alignment/affine.rs, pair.rs ------------------------------------------------------------------------------------------
/// drop-in for normalize_for_detection (affine.rs:24-53)
pub fn normalize_for_detection(hip: &Hip, image: &impl PlaneSrc) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(image.dims());
    hip.check(unsafe { sys::ab_normalize_for_detection(hip.ctx, &image.ab(), &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for align_channel_affine (affine.rs:129-212)
pub fn align_channel_affine(hip: &Hip, reference: &impl PlaneSrc, target: &impl PlaneSrc) -> Result<AffineAlignResult> {
    let mut r: sys::ab_affine_align_result = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_align_channel_affine(hip.ctx, &reference.ab(), &target.ab(), num_threads(), &mut r) })?;
    Ok(align_from_sys(&r))
}
/// align_channel_affine(reference, targets[i]) for every i in one call: the loop of align_channels_cmd (cmd/compose/blend.rs:226-232)
/// and of compose::rgb::align_channels (rgb.rs:165-189); the reference frame is detected once
pub fn register_frames<P: PlaneSrc>(hip: &Hip, reference: &impl PlaneSrc, targets: &[P]) -> Result<Vec<AffineAlignResult>> {
    let planes: Vec<_> = targets.iter().map(|t| t.ab()).collect();
    let mut out: Vec<sys::ab_affine_align_result> = vec![unsafe { std::mem::zeroed() }; targets.len()];
    hip.check(unsafe { sys::ab_register_frames(hip.ctx, &reference.ab(), planes.as_ptr(), planes.len(), num_threads(), out.as_mut_ptr()) })?;
    Ok(out.iter().map(align_from_sys).collect())
}
/// align_pair(reference, targets[i], Affine) for every i (pair.rs:41-77): estimate + warp into HBM.  The reference and the targets
/// may be host arrays (`&Array2<f32>` as GLOBAL_IMAGE_CACHE holds them) or DevicePlanes: host frames are uploaded by the library
/// on its own stream and registered as they land (one call for the whole set -- do not chunk it)
pub fn align_pairs_affine<P: PlaneSrc>(hip: &Hip, reference: &impl PlaneSrc, targets: &[P], aligned: &mut [DevicePlane]) -> Result<Vec<AffineAlignResult>> {
    let planes: Vec<_> = targets.iter().map(|t| t.ab()).collect();
    let mut outs: Vec<_> = aligned.iter_mut().map(|a| a.ab_mut()).collect();
    let mut res: Vec<sys::ab_affine_align_result> = vec![unsafe { std::mem::zeroed() }; targets.len()];
    hip.check(unsafe { sys::ab_align_pairs_affine(hip.ctx, &reference.ab(), planes.as_ptr(), planes.len(), num_threads(), res.as_mut_ptr(), outs.as_mut_ptr()) })?;
    Ok(res.iter().map(align_from_sys).collect())
}
/// the star-list half of align_channel_affine on given centroids (host arithmetic inside the library)
pub fn affine_from_stars(ref_xy: &[(f64, f64)], tgt_xy: &[(f64, f64)], rows: usize, cols: usize) -> Option<AffineAlignResult> {
    let r: Vec<f64> = ref_xy.iter().flat_map(|p| [p.0, p.1]).collect();
    let t: Vec<f64> = tgt_xy.iter().flat_map(|p| [p.0, p.1]).collect();
    let mut out: sys::ab_affine_align_result = unsafe { std::mem::zeroed() };
    let mut found = 0i32;
    let rc = unsafe { sys::ab_affine_from_stars(r.as_ptr(), ref_xy.len(), t.as_ptr(), tgt_xy.len(), rows as i64, cols as i64, num_threads(), &mut out, &mut found) };
    (rc == sys::AB_OK && found != 0).then(|| align_from_sys(&out))
}
/// side of a vote matrix: row = reference star index, column = target star index
pub const VOTE_DIM: usize = 64;
fn flat_xy(xy: &[(f64, f64)]) -> Vec<f64> {
    xy.iter().flat_map(|p| [p.0, p.1]).collect()
}
/// the vote half of match_triangles (affine.rs:320-350) of the library's host matcher: VOTE_DIM x VOTE_DIM counts, row-major
pub fn triangle_votes_host(ref_xy: &[(f64, f64)], tgt_xy: &[(f64, f64)]) -> Option<Vec<u32>> {
    let (r, t) = (flat_xy(ref_xy), flat_xy(tgt_xy));
    let mut votes = vec![0u32; VOTE_DIM * VOTE_DIM];
    let rc = unsafe { sys::ab_triangle_votes_host(r.as_ptr(), ref_xy.len(), t.as_ptr(), tgt_xy.len(), votes.as_mut_ptr()) };
    (rc == sys::AB_OK).then_some(votes)
}
/// the greedy half of match_triangles (affine.rs:351-384) on a given vote matrix: (ref index, tgt index) in acceptance order
pub fn matches_from_votes(votes: &[u32], n_ref: usize, n_tgt: usize) -> Option<Vec<(usize, usize)>> {
    if votes.len() != VOTE_DIM * VOTE_DIM {
        return None;
    }
    let (mut ri, mut ti, mut n) = (vec![0usize; VOTE_DIM], vec![0usize; VOTE_DIM], 0usize);
    let rc = unsafe { sys::ab_matches_from_votes(n_ref, n_tgt, votes.as_ptr(), ri.as_mut_ptr(), ti.as_mut_ptr(), VOTE_DIM, &mut n) };
    (rc == sys::AB_OK).then(|| ri.into_iter().zip(ti).take(n.min(VOTE_DIM)).collect())
}
/// the GPU matcher's vote matrices for given star lists (one reference list, many target lists): VOTE_DIM x VOTE_DIM counts per target;
/// grouped = false takes the targets one after another, true in groups of up to eight, as a batch's two forms do
pub fn triangle_votes(hip: &Hip, ref_xy: &[(f64, f64)], targets: &[Vec<(f64, f64)>], grouped: bool) -> Result<Vec<Vec<u32>>> {
    let r = flat_xy(ref_xy);
    let t: Vec<f64> = targets.iter().flat_map(|l| flat_xy(l)).collect();
    let counts: Vec<usize> = targets.iter().map(|l| l.len()).collect();
    let mut votes = vec![0u32; targets.len() * VOTE_DIM * VOTE_DIM];
    hip.check(unsafe {
        sys::ab_triangle_votes_device(hip.ctx, r.as_ptr(), ref_xy.len(), t.as_ptr(), counts.as_ptr(), counts.len(), grouped as i32, votes.as_mut_ptr())
    })?;
    Ok(votes.chunks(VOTE_DIM * VOTE_DIM).map(|m| m.to_vec()).collect())
}
/// drop-in for core::alignment::pair::align_pair (pair.rs:41-77)
pub fn align_pair(hip: &Hip, reference: &impl PlaneSrc, target: &impl PlaneSrc, method: AlignMethod, rows: usize, cols: usize) -> Result<AlignPairResult> {
    match method {
        AlignMethod::PhaseCorrelation => {
            let pc = phase_correlate(hip, reference, target)?;
            Ok(AlignPairResult {
                aligned: shift_image_subpixel(hip, target, pc.dy, pc.dx)?,
                offset: (pc.dy, pc.dx),
                confidence: pc.confidence,
                method_used: "phase_correlation".into(),
                matched_stars: 0,
                inliers: 0,
                residual_px: 0.0,
            })
        }
        AlignMethod::Affine => {
            let r = align_channel_affine(hip, reference, target)?;
            Ok(AlignPairResult {
                aligned: warp_image(hip, target, &r.transform, rows, cols)?,
                offset: (r.transform.ty, r.transform.tx),
                confidence: if r.inliers > 0 { 1.0 } else { 0.0 },
                method_used: r.method.to_string(),
                matched_stars: r.matched_stars,
                inliers: r.inliers,
                residual_px: r.residual_px,
            })
        }
    }
}

// ---- a9 / a10 / a11  core/imaging/stats.rs, stf.rs ----------------------------------------------------------------------------------
/// drop-in for compute_image_stats (stats.rs:15-23)
pub fn compute_image_stats(hip: &Hip, data: &impl PlaneSrc) -> Result<ImageStats> {
    let mut st: sys::ab_image_stats = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_compute_image_stats(hip.ctx, &data.ab(), &mut st) })?;
    Ok(stats_from_sys(&st))
}
/// drop-in for compute_image_stats_with_known_range (stats.rs:25-83)
pub fn compute_image_stats_with_known_range(hip: &Hip, data: &impl PlaneSrc, known_min: f64, known_max: f64) -> Result<ImageStats> {
    let mut st: sys::ab_image_stats = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_compute_image_stats_with_known_range(hip.ctx, &data.ab(), known_min, known_max, &mut st) })?;
    Ok(stats_from_sys(&st))
}
/// drop-in for build_histogram (stats.rs:212-240)
pub fn build_histogram(hip: &Hip, data: &impl PlaneSrc, bins: usize, dmin: f64, dmax: f64) -> Result<Vec<u32>> {
    let mut out = vec![0u32; bins];
    hip.check(unsafe { sys::ab_build_histogram(hip.ctx, &data.ab(), bins, dmin, dmax, out.as_mut_ptr()) })?;
    Ok(out)
}
/// the 65 536-bin value histogram + sum + count behind the large-image statistics (stats.rs:85-210), for callers that merge shards
pub fn stats_value_hist(hip: &Hip, data: &impl PlaneSrc, gmin: f64, gmax: f64) -> Result<(Vec<u64>, f64, u64)> {
    let mut hist = vec![0u64; 65536];
    let (mut sum, mut cnt) = (0.0f64, 0u64);
    hip.check(unsafe { sys::ab_stats_value_hist(hip.ctx, &data.ab(), gmin, gmax, hist.as_mut_ptr(), &mut sum, &mut cnt) })?;
    Ok((hist, sum, cnt))
}
/// drop-in for auto_stf (stf.rs:13-47): host arithmetic inside the library
pub fn auto_stf(stats: &ImageStats, config: &AutoStfConfig) -> StfParams {
    let cfg = sys::ab_auto_stf_config { target_bg: config.target_bg, shadow_k: config.shadow_k };
    let mut p = sys::ab_stf_params { shadow: 0.0, midtone: 0.5, highlight: 1.0 };
    unsafe { sys::ab_auto_stf(&stats_to_sys(stats), &cfg, &mut p) };
    stf_from_sys(&p)
}
/// drop-in for apply_stf (stf.rs:89-102)
pub fn apply_stf(hip: &Hip, data: &impl PlaneSrc, p: &StfParams, st: &ImageStats) -> Result<Vec<u8>> {
    let (r, c) = data.dims();
    let mut out = vec![0u8; r * c];
    hip.check(unsafe { sys::ab_apply_stf_u8(hip.ctx, &data.ab(), &stf_to_sys(p), &stats_to_sys(st), out.as_mut_ptr(), 0) })?;
    Ok(out)
}
/// drop-in for apply_stf_f32 (stf.rs:104-118)
pub fn apply_stf_f32(hip: &Hip, data: &impl PlaneSrc, p: &StfParams, st: &ImageStats) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(data.dims());
    apply_stf_f32_into(hip, data, p, st, &mut out)?;
    Ok(out)
}
pub fn apply_stf_f32_into(hip: &Hip, data: &impl PlaneSrc, p: &StfParams, st: &ImageStats, out: &mut impl PlaneDst) -> Result<()> {
    hip.check(unsafe { sys::ab_apply_stf_f32(hip.ctx, &data.ab(), &stf_to_sys(p), &stats_to_sys(st), &mut out.ab_mut()) })
}
/// drop-in for cmd::common::auto_stretch_preview (cmd/common.rs:18-22): stats -> auto_stf -> apply_stf as one device chain.
/// A host plane is uploaded once and never read back; only the u8 preview and 80 bytes of scalars return.
pub fn auto_stretch_preview(hip: &Hip, arr: &impl PlaneSrc) -> Result<(Vec<u8>, ImageStats, StfParams)> {
    let (rows, cols) = arr.dims();
    let src = arr.ab();
    let staged = if src.on_device == 0 { Some(DevicePlane::alloc(rows, cols)?) } else { None };
    if let Some(d) = staged.as_ref() {
        hip.check(unsafe { sys::ab_upload(hip.ctx, d.as_ptr() as *mut c_void, src.data as *const c_void, rows * cols * 4) })?;
    }
    let p = staged.as_ref().map_or(src, |d| d.ab());
    let mut du8 = std::ptr::null_mut();
    hip.check(unsafe { sys::ab_device_alloc(hip.ctx, rows * cols, &mut du8) })?;
    let r = (|| {
        let mut st: sys::ab_image_stats = unsafe { std::mem::zeroed() };
        let mut stf = sys::ab_stf_params { shadow: 0.0, midtone: 0.5, highlight: 1.0 };
        hip.check(unsafe { sys::ab_auto_stretch_preview(hip.ctx, std::ptr::null_mut(), &p, 0, std::ptr::null(), du8 as *mut u8, &mut st, &mut stf) })?;
        let mut out = vec![0u8; rows * cols];
        hip.check(unsafe { sys::ab_download(hip.ctx, out.as_mut_ptr() as *mut c_void, du8, rows * cols) })?;
        Ok((out, stats_from_sys(&st), stf_from_sys(&stf)))
    })();
    unsafe { sys::ab_device_free(hip.ctx, du8) };
    r
}

// ---- a14  core/imaging/scnr.rs ---------------------------------------------------------------------------------------------------------
/// drop-in for apply_scnr_inplace (scnr.rs:18-53); mismatched dims or amount < 1e-7: a silent no-op, as in the reference
pub fn apply_scnr_inplace(hip: &Hip, r: &mut impl PlaneDst, g: &mut impl PlaneDst, b: &mut impl PlaneDst, config: &ScnrConfig) -> Result<()> {
    hip.check(unsafe { sys::ab_apply_scnr_inplace(hip.ctx, &mut r.ab_mut(), &mut g.ab_mut(), &mut b.ab_mut(), &scnr_to_sys(config)) })
}

// ---- a16  core/compose/channel_blend.rs ----------------------------------------------------------------------------------------------------
fn blend_weights(w: &[BlendWeight]) -> Vec<sys::ab_blend_weight> {
    w.iter().map(|x| sys::ab_blend_weight { channel_idx: x.channel_idx as u64, r_weight: x.r_weight, g_weight: x.g_weight, b_weight: x.b_weight }).collect()
}
/// drop-in for blend_channels (channel_blend.rs:13-70)
pub fn blend_channels<P: PlaneSrc>(hip: &Hip, channels: &[P], weights: &[BlendWeight], rows: usize, cols: usize) -> Result<(Array2<f32>, Array2<f32>, Array2<f32>)> {
    let (mut r, mut g, mut b) = (Array2::<f32>::zeros((rows, cols)), Array2::<f32>::zeros((rows, cols)), Array2::<f32>::zeros((rows, cols)));
    blend_channels_into(hip, channels, weights, &mut r, &mut g, &mut b)?;
    Ok((r, g, b))
}
pub fn blend_channels_into<P: PlaneSrc>(hip: &Hip, channels: &[P], weights: &[BlendWeight], r: &mut impl PlaneDst, g: &mut impl PlaneDst, b: &mut impl PlaneDst) -> Result<()> {
    let planes: Vec<_> = channels.iter().map(|c| c.ab()).collect();
    let w = blend_weights(weights);
    hip.check(unsafe { sys::ab_blend_channels(hip.ctx, planes.as_ptr(), planes.len(), w.as_ptr(), w.len(), &mut r.ab_mut(), &mut g.ab_mut(), &mut b.ab_mut()) })
}

// ---- a15  core/imaging/curves.rs -------------------------------------------------------------------------------------------------------------
/// SplineLut (curves.rs:64-184): the 4096-entry table of SplineLut::from_points (Fritsch-Carlson monotone cubic)
pub struct SplineLut {
    lut: [f32; 4096],
}
impl SplineLut {
    pub fn from_points(points: &[(f64, f64)]) -> Self {
        let flat: Vec<f64> = points.iter().flat_map(|p| [p.0, p.1]).collect();
        let mut lut = [0f32; 4096];
        unsafe { sys::ab_spline_lut_from_points(flat.as_ptr(), points.len(), lut.as_mut_ptr()) };
        Self { lut }
    }
}
/// drop-in for apply_curve (curves.rs:186-197)
pub fn apply_curve(hip: &Hip, data: &impl PlaneSrc, lut: &SplineLut) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(data.dims());
    apply_curve_into(hip, data, lut, &mut out)?;
    Ok(out)
}
pub fn apply_curve_into(hip: &Hip, data: &impl PlaneSrc, lut: &SplineLut, out: &mut impl PlaneDst) -> Result<()> {
    hip.check(unsafe { sys::ab_apply_curve(hip.ctx, &data.ab(), lut.lut.as_ptr(), &mut out.ab_mut()) })
}
/// drop-in for apply_levels (curves.rs:31-52)
pub fn apply_levels(hip: &Hip, data: &impl PlaneSrc, p: &LevelsParams) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(data.dims());
    apply_levels_into(hip, data, p, &mut out)?;
    Ok(out)
}
pub fn apply_levels_into(hip: &Hip, data: &impl PlaneSrc, p: &LevelsParams, out: &mut impl PlaneDst) -> Result<()> {
    let lp = sys::ab_levels_params { black: p.black, gamma: p.gamma, white: p.white };
    hip.check(unsafe { sys::ab_apply_levels(hip.ctx, &data.ab(), &lp, &mut out.ab_mut()) })
}
/// drop-ins for apply_levels_rgb / apply_curve_rgb (curves.rs:54-62,199-207): three launches on one stream
pub fn apply_levels_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, lr: &LevelsParams, lg: &LevelsParams, lb: &LevelsParams) -> Result<(Array2<f32>, Array2<f32>, Array2<f32>)> {
    Ok((apply_levels(hip, r, lr)?, apply_levels(hip, g, lg)?, apply_levels(hip, b, lb)?))
}
pub fn apply_curve_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, lr: &SplineLut, lg: &SplineLut, lb: &SplineLut) -> Result<(Array2<f32>, Array2<f32>, Array2<f32>)> {
    Ok((apply_curve(hip, r, lr)?, apply_curve(hip, g, lg)?, apply_curve(hip, b, lb)?))
}

// ---- a19  core/imaging/stretch.rs ---------------------------------------------------------------------------------------------------------------
/// drop-in for arcsinh_stretch_with_stats (stretch.rs:10-45)
pub fn arcsinh_stretch_with_stats(hip: &Hip, data: &impl PlaneSrc, dmin: f32, dmax: f32, factor: f32, gamma: f32) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(data.dims());
    hip.check(unsafe { sys::ab_arcsinh_stretch_with_stats(hip.ctx, &data.ab(), dmin, dmax, factor, gamma, &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for arcsinh_stretch (stretch.rs:5-8)
pub fn arcsinh_stretch(hip: &Hip, data: &impl PlaneSrc, factor: f32) -> Result<Array2<f32>> {
    let st = compute_image_stats(hip, data)?;
    arcsinh_stretch_with_stats(hip, data, st.min as f32, st.max as f32, factor, 1.0)
}
/// compute_luminance (masked_stretch.rs:128-154: the finite-guarded Rec.709 luminance)
pub fn compute_luminance(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(r.dims());
    hip.check(unsafe { sys::ab_luminance(hip.ctx, &r.ab(), &g.ab(), &b.ab(), &mut out.ab_mut()) })?;
    Ok(out)
}
/// `orig * factor` of calibrate_channel (cmd/compose/color.rs:28-40)
pub fn scale_into(hip: &Hip, data: &impl PlaneSrc, factor: f32, out: &mut impl PlaneDst) -> Result<()> {
    hip.check(unsafe { sys::ab_scale(hip.ctx, &data.ab(), factor, &mut out.ab_mut()) })
}

// ---- a20  core/stacking/calibration.rs ------------------------------------------------------------------------------------------------------------
/// drop-in for calibrate_image (calibration.rs:47-82)
pub fn calibrate_image(hip: &Hip, raw: &impl PlaneSrc, config: &CalibrationConfig) -> Result<Array2<f32>> {
    let (bias, dark, flat) = (opt_plane(config.master_bias.as_ref()), opt_plane(config.master_dark.as_ref()), opt_plane(config.master_flat.as_ref()));
    let mut out = Array2::<f32>::zeros(raw.dims());
    hip.check(unsafe { sys::ab_calibrate_image(hip.ctx, &raw.ab(), opt_ptr(&bias), opt_ptr(&dark), opt_ptr(&flat), config.dark_exposure_ratio, &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for median_combine_row_major on in-memory frames (calibration.rs:84-125)
pub fn median_combine<P: PlaneSrc>(hip: &Hip, frames: &[P]) -> Result<Array2<f32>> {
    if frames.is_empty() {
        bail!("No images to stack");
    }
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let mut out = Array2::<f32>::zeros(frames[0].dims());
    hip.check(unsafe { sys::ab_median_combine(hip.ctx, planes.as_ptr(), planes.len(), &mut out.ab_mut()) })?;
    Ok(out)
}
pub enum MasterKind {
    Bias = 0,
    Dark = 1,
    Flat = 2,
}
/// create_master_bias / _dark / _flat after their loader (calibration.rs:127-255): the frames are already in memory
pub fn create_master<P: PlaneSrc>(hip: &Hip, kind: MasterKind, frames: &[P], master_bias: Option<&Array2<f32>>, master_dark: Option<&Array2<f32>>) -> Result<Array2<f32>> {
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let (bias, dark) = (opt_plane(master_bias), opt_plane(master_dark));
    let dims = frames.first().map_or((0, 0), |f| f.dims());
    let mut out = Array2::<f32>::zeros(dims);
    hip.check(unsafe { sys::ab_create_master(hip.ctx, kind as i32, planes.as_ptr(), planes.len(), opt_ptr(&bias), opt_ptr(&dark), &mut out.ab_mut()) })?;
    Ok(out)
}

// ---- a12  core/imaging/background.rs -----------------------------------------------------------------------------------------------------------------
/// drop-in for extract_background (background.rs:55-116), progress and cancel included
pub fn extract_background(hip: &Hip, image: &impl PlaneSrc, config: &BackgroundConfig, progress: Option<&ProgressHandle>) -> Result<BackgroundResult> {
    let start = std::time::Instant::now();
    let (rows, cols) = image.dims();
    let (mut model, mut corrected) = (Array2::<f32>::zeros((rows, cols)), Array2::<f32>::zeros((rows, cols)));
    let cfg = sys::ab_background_config { grid_size: config.grid_size, poly_degree: config.poly_degree, sigma_clip: config.sigma_clip, iterations: config.iterations, mode: config.mode as i32 };
    let mut info: sys::ab_background_info = unsafe { std::mem::zeroed() };
    let (mut pm, mut pc) = (model.ab_mut(), corrected.ab_mut());
    hip.with_progress(progress, || hip.check(unsafe { sys::ab_extract_background(hip.ctx, &image.ab(), &cfg, &mut pm, &mut pc, &mut info) }))?;
    if let Some(p) = progress {
        p.emit_complete(); // background.rs:105-107
    }
    Ok(BackgroundResult { model, corrected, sample_count: info.sample_count, rms_residual: info.rms_residual, elapsed_ms: start.elapsed().as_millis() as u64 })
}

// ---- core/analysis/deconvolution.rs (deconvolve_rl_cmd) -------------------------------------------------------------------------------------------------
/// drop-in for generate_gaussian_psf (deconvolution.rs:12-33): host maths in the library, bit-identical on glibc
pub fn generate_gaussian_psf(size: usize, sigma: f32) -> Array2<f32> {
    let mut psf = Array2::<f32>::zeros((size, size));
    if size > 0 {
        unsafe { sys::ab_generate_gaussian_psf(size, sigma, psf.as_mut_ptr()) };
    }
    psf
}
/// drop-in for richardson_lucy (deconvolution.rs:141-221), progress and cancel included (one tick per chunk of iterations)
pub fn richardson_lucy(hip: &Hip, image: &impl PlaneSrc, psf: &impl PlaneSrc, config: &RLConfig, progress: Option<&ProgressHandle>) -> Result<RLResult> {
    let start = std::time::Instant::now();
    let mut out = Array2::<f32>::zeros(image.dims());
    let cfg = sys::ab_rl_config {
        iterations: config.iterations,
        regularization: config.regularization,
        deringing: config.deringing as i32,
        deringing_threshold: config.deringing_threshold,
    };
    let mut res: sys::ab_rl_result = unsafe { std::mem::zeroed() };
    let mut po = out.ab_mut();
    hip.with_progress(progress, || hip.check(unsafe { sys::ab_richardson_lucy(hip.ctx, &image.ab(), &psf.ab(), &cfg, &mut po, &mut res) }))?;
    Ok(RLResult { image: out, iterations_run: res.iterations_run, convergence: res.convergence, elapsed_ms: start.elapsed().as_millis() as u64 })
}

// ---- core/imaging/psf_estimation.rs (deconvolve_rl_cmd with use_empirical_psf) ---------------------------------------------------------------------------
fn psf_cfg(config: &PsfEstimationConfig) -> sys::ab_psf_estimation_config {
    sys::ab_psf_estimation_config {
        num_stars: config.num_stars,
        cutout_radius: config.cutout_radius,
        saturation_threshold: config.saturation_threshold,
        min_peak_fraction: config.min_peak_fraction,
        max_ellipticity: config.max_ellipticity,
        edge_margin: config.edge_margin,
        max_center_distance_fraction: config.max_center_distance_fraction,
    }
}
fn psf_star(s: &sys::ab_psf_star) -> StarCandidate {
    StarCandidate { x: s.x, y: s.y, peak: s.peak, flux: s.flux, fwhm: s.fwhm, ellipticity: s.ellipticity, distance_from_center: s.distance_from_center, snr: s.snr }
}
/// PsfEstimationConfig::default() (psf_estimation.rs:27-39) as the library fills it in
pub fn psf_estimation_config_default() -> PsfEstimationConfig {
    let mut c: sys::ab_psf_estimation_config = unsafe { std::mem::zeroed() };
    unsafe { sys::ab_psf_estimation_config_default(&mut c) };
    PsfEstimationConfig {
        num_stars: c.num_stars,
        cutout_radius: c.cutout_radius,
        saturation_threshold: c.saturation_threshold,
        min_peak_fraction: c.min_peak_fraction,
        max_ellipticity: c.max_ellipticity,
        edge_margin: c.edge_margin,
        max_center_distance_fraction: c.max_center_distance_fraction,
    }
}
/// the quality filter, score_star, the stable descending sort and take(num_stars) of estimate_psf (psf_estimation.rs:68-92, :509-516):
/// (indices of the selected stars in selection order, how many passed the filter); host maths in the library
pub fn psf_select_stars(stars: &[StarCandidate], config: &PsfEstimationConfig, max_val: f64, rows: usize, cols: usize) -> Result<(Vec<usize>, usize)> {
    let c: Vec<sys::ab_psf_star> = stars
        .iter()
        .map(|s| sys::ab_psf_star { x: s.x, y: s.y, peak: s.peak, flux: s.flux, fwhm: s.fwhm, ellipticity: s.ellipticity, distance_from_center: s.distance_from_center, snr: s.snr })
        .collect();
    let mut idx = vec![0usize; stars.len()];
    let (mut selected, mut filtered) = (0usize, 0usize);
    let rc = unsafe {
        sys::ab_psf_select_stars(c.as_ptr(), c.len(), &psf_cfg(config), max_val, rows as i64, cols as i64, idx.as_mut_ptr(), idx.len(), &mut selected, &mut filtered)
    };
    if rc != sys::AB_OK {
        bail!("psf_select_stars: invalid arguments (status {rc})");
    }
    idx.truncate(selected);
    Ok((idx, filtered))
}
/// estimate_psf (psf_estimation.rs:52-134) with the kernel left where `kernel` lies -- a device plane goes straight into
/// richardson_lucy; PsfResult.kernel stays empty in that case.  The reference's three Err strings come back as errors.
pub fn estimate_psf_into(hip: &Hip, image: &impl PlaneSrc, config: &PsfEstimationConfig, kernel: &mut impl PlaneDst) -> Result<PsfResult> {
    let cap = config.num_stars.min(1 << 20);
    let mut stars: Vec<sys::ab_psf_star> = vec![unsafe { std::mem::zeroed() }; cap.max(1)];
    let mut res: sys::ab_psf_result = unsafe { std::mem::zeroed() };
    let mut pk = kernel.ab_mut();
    hip.check(unsafe { sys::ab_estimate_psf(hip.ctx, &image.ab(), &psf_cfg(config), &mut pk, stars.as_mut_ptr(), cap, &mut res) })?;
    match res.outcome {
        sys::AB_PSF_OK => {}
        sys::AB_PSF_NO_STARS_DETECTED => bail!("No stars detected in image"),
        sys::AB_PSF_NO_STARS_PASSED => bail!("No stars passed quality filters"),
        _ => bail!("Failed to extract star cutouts"),
    }
    Ok(PsfResult {
        kernel: Vec::new(),
        kernel_size: res.kernel_size,
        average_fwhm: res.average_fwhm,
        average_ellipticity: res.average_ellipticity,
        stars_used: stars[..res.stars_used.min(cap)].iter().map(psf_star).collect(),
        stars_rejected: res.stars_rejected,
        spread_pixels: res.spread_pixels,
    })
}
/// drop-in for estimate_psf (psf_estimation.rs:52-134): the image is never downloaded when it is a device plane
pub fn estimate_psf(hip: &Hip, image: &impl PlaneSrc, config: &PsfEstimationConfig) -> Result<PsfResult> {
    let size = config.cutout_radius * 2 + 1;
    let mut kernel = Array2::<f32>::zeros((size, size));
    let mut res = estimate_psf_into(hip, image, config, &mut kernel)?;
    res.kernel = kernel.rows().into_iter().map(|row| row.to_vec()).collect();
    Ok(res)
}
/// drop-in for psf_to_kernel (psf_estimation.rs:136-149): host-only, the reference's own loop
pub fn psf_to_kernel(psf: &PsfResult) -> Array2<f32> {
    let size = psf.kernel_size;
    let mut kernel = Array2::<f32>::zeros((size, size));
    for (y, row) in psf.kernel.iter().enumerate() {
        for (x, &val) in row.iter().enumerate() {
            if y < size && x < size {
                kernel[[y, x]] = val;
            }
        }
    }
    kernel
}

// ---- core/synth (generate_synth_cmd, generate_synth_stack_cmd) --------------------------------------------------------------------------------------------
fn synth_psf(p: &PsfType) -> sys::ab_synth_psf_type {
    match *p {
        PsfType::Gaussian { fwhm } => sys::ab_synth_psf_type { kind: sys::AB_SYNTH_PSF_GAUSSIAN, fwhm, beta: 0.0 },
        PsfType::Moffat { fwhm, beta } => sys::ab_synth_psf_type { kind: sys::AB_SYNTH_PSF_MOFFAT, fwhm, beta },
        PsfType::Airy { lambda_over_d } => sys::ab_synth_psf_type { kind: sys::AB_SYNTH_PSF_AIRY, fwhm: lambda_over_d, beta: 0.0 },
    }
}
fn synth_noise(n: &NoiseParams) -> sys::ab_synth_noise_params {
    sys::ab_synth_noise_params {
        gain: n.gain,
        readout_noise: n.readout_noise,
        sky_background: n.sky_background,
        dark_current: n.dark_current,
        exposure_time: n.exposure_time,
        bias_level: n.bias_level,
        seed: n.seed,
    }
}
fn synth_cfg(c: &SynthConfig) -> sys::ab_synth_config {
    let field_type = match c.field_type {
        FieldType::Uniform => sys::ab_synth_field_type { kind: sys::AB_SYNTH_FIELD_UNIFORM, a: 0.0, b: 0.0 },
        FieldType::KingCluster { core_radius, tidal_radius } => sys::ab_synth_field_type { kind: sys::AB_SYNTH_FIELD_KING_CLUSTER, a: core_radius, b: tidal_radius },
        FieldType::ExponentialDisk { scale_length, inclination_deg } => {
            sys::ab_synth_field_type { kind: sys::AB_SYNTH_FIELD_EXPONENTIAL_DISK, a: scale_length, b: inclination_deg }
        }
    };
    sys::ab_synth_config {
        field: sys::ab_synth_field_config {
            width: c.field.width,
            height: c.field.height,
            n_stars: c.field.n_stars,
            flux_min: c.field.flux_min,
            flux_max: c.field.flux_max,
            seed: c.field.seed,
        },
        field_type,
        psf_type: synth_psf(&c.psf_type),
        noise: synth_noise(&c.noise),
        apply_vignette: c.apply_vignette as i32,
        vignette_strength: c.vignette_strength,
        n_frames: c.n_frames,
    }
}
fn synth_stars_in(stars: &[Star]) -> Vec<sys::ab_synth_star> {
    stars.iter().map(|s| sys::ab_synth_star { x: s.x, y: s.y, z: s.z, flux: s.flux, temperature: s.temperature }).collect()
}
fn synth_stars_out(stars: &[sys::ab_synth_star]) -> Vec<Star> {
    stars.iter().map(|s| Star { x: s.x, y: s.y, z: s.z, flux: s.flux, temperature: s.temperature }).collect()
}
/// SynthConfig::default() (pipeline.rs:41-53) as the library fills it in
pub fn synth_config_default() -> SynthConfig {
    let mut c: sys::ab_synth_config = unsafe { std::mem::zeroed() };
    unsafe { sys::ab_synth_config_default(&mut c) };
    SynthConfig {
        field: FieldConfig { width: c.field.width, height: c.field.height, n_stars: c.field.n_stars, flux_min: c.field.flux_min, flux_max: c.field.flux_max, seed: c.field.seed },
        field_type: FieldType::Uniform,
        psf_type: PsfType::Gaussian { fwhm: c.psf_type.fwhm },
        noise: NoiseParams {
            gain: c.noise.gain,
            readout_noise: c.noise.readout_noise,
            sky_background: c.noise.sky_background,
            dark_current: c.noise.dark_current,
            exposure_time: c.noise.exposure_time,
            bias_level: c.noise.bias_level,
            seed: c.noise.seed,
        },
        apply_vignette: c.apply_vignette != 0,
        vignette_strength: c.vignette_strength,
        n_frames: c.n_frames,
    }
}
/// draws skip .. skip + n - 1 of StdRng::seed_from_u64(seed) as gen::<f64>(): what the generator's kernels compute per pixel
pub fn synth_rng_f64(seed: u64, skip: u64, n: usize) -> Vec<f64> {
    let mut out = vec![0.0f64; n];
    unsafe { sys::ab_synth_rng_f64(seed, skip, n, out.as_mut_ptr()) };
    out
}
/// test hook: one block of the ChaCha block function behind the stream (rounds = 12 or 20)
pub fn synth_chacha_block(key: &[u32; 8], counter: u64, rounds: i32) -> Result<[u32; 16]> {
    let mut out = [0u32; 16];
    let rc = unsafe { sys::ab_synth_chacha_block(key.as_ptr(), counter, rounds, out.as_mut_ptr()) };
    if rc != sys::AB_OK {
        bail!("synth_chacha_block: rounds must be 12 or 20");
    }
    Ok(out)
}
/// drop-in for gen_field (pipeline.rs:126-138): uniform_field / king_cluster / exponential_disk; an Err where the reference would not return
pub fn synth_star_field(config: &SynthConfig) -> Result<Vec<Star>> {
    let cap = config.field.n_stars;
    let mut stars: Vec<sys::ab_synth_star> = vec![unsafe { std::mem::zeroed() }; cap.max(1)];
    let mut n = 0usize;
    let rc = unsafe { sys::ab_synth_star_field(&synth_cfg(config), stars.as_mut_ptr(), cap, &mut n) };
    if rc != sys::AB_OK {
        bail!("star field: king_cluster needs positive finite radii and a profile that can accept (status {rc})");
    }
    Ok(synth_stars_out(&stars[..n.min(cap)]))
}
/// drop-in for render_stars (psf.rs:123-158)
pub fn render_stars(hip: &Hip, stars: &[Star], psf: &PsfType, width: u32, height: u32) -> Result<Array2<f32>> {
    let mut image = Array2::<f32>::zeros((height as usize, width as usize));
    let c = synth_stars_in(stars);
    let mut po = image.ab_mut();
    hip.check(unsafe { sys::ab_synth_render_stars(hip.ctx, c.as_ptr(), c.len(), &synth_psf(psf), &mut po) })?;
    Ok(image)
}
/// drop-in for generate_flat_field (noise.rs:81-99)
pub fn generate_flat_field(hip: &Hip, width: u32, height: u32, seed: u64, vignette_strength: f64) -> Result<Array2<f32>> {
    let mut flat = Array2::<f32>::zeros((height as usize, width as usize));
    let mut po = flat.ab_mut();
    hip.check(unsafe { sys::ab_synth_flat_field(hip.ctx, seed, vignette_strength, &mut po) })?;
    Ok(flat)
}
/// drop-in for apply_flat_field (noise.rs:101-111)
pub fn apply_flat_field(hip: &Hip, image: &mut impl PlaneDst, flat: &impl PlaneSrc) -> Result<()> {
    let mut pi = image.ab_mut();
    hip.check(unsafe { sys::ab_synth_apply_flat_field(hip.ctx, &mut pi, &flat.ab()) })
}
/// drop-in for apply_noise (noise.rs:62-79)
pub fn apply_noise(hip: &Hip, image: &impl PlaneSrc, params: &NoiseParams) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(image.dims());
    let mut po = out.ab_mut();
    hip.check(unsafe { sys::ab_synth_apply_noise(hip.ctx, &image.ab(), &synth_noise(params), &mut po, std::ptr::null_mut()) })?;
    Ok(out)
}
/// drop-in for generate (pipeline.rs:63-82): (noisy, ground_truth, stars)
pub fn synth_generate(hip: &Hip, config: &SynthConfig) -> Result<(Array2<f32>, Array2<f32>, Vec<Star>)> {
    let dims = (config.field.height as usize, config.field.width as usize);
    let (mut noisy, mut truth) = (Array2::<f32>::zeros(dims), Array2::<f32>::zeros(dims));
    let cap = config.field.n_stars;
    let mut stars: Vec<sys::ab_synth_star> = vec![unsafe { std::mem::zeroed() }; cap.max(1)];
    let mut res: sys::ab_synth_result = unsafe { std::mem::zeroed() };
    let (mut pn, mut pt) = (noisy.ab_mut(), truth.ab_mut());
    hip.check(unsafe { sys::ab_synth_generate(hip.ctx, &synth_cfg(config), &mut pn, &mut pt, stars.as_mut_ptr(), cap, &mut res) })?;
    Ok((noisy, truth, synth_stars_out(&stars[..res.star_count.min(cap)])))
}
/// drop-in for generate_stack (pipeline.rs:84-108), progress ("synth", k, n) and cancel per frame: (frames, ground_truth, stars)
pub fn synth_generate_stack(hip: &Hip, config: &SynthConfig, progress: Option<&ProgressHandle>) -> Result<(Vec<Array2<f32>>, Array2<f32>, Vec<Star>)> {
    let dims = (config.field.height as usize, config.field.width as usize);
    let mut frames: Vec<Array2<f32>> = (0..config.n_frames).map(|_| Array2::<f32>::zeros(dims)).collect();
    let mut truth = Array2::<f32>::zeros(dims);
    let cap = config.field.n_stars;
    let mut stars: Vec<sys::ab_synth_star> = vec![unsafe { std::mem::zeroed() }; cap.max(1)];
    let mut res: sys::ab_synth_result = unsafe { std::mem::zeroed() };
    let mut planes: Vec<sys::ab_plane_mut> = frames.iter_mut().map(|f| f.ab_mut()).collect();
    let mut pt = truth.ab_mut();
    hip.with_progress(progress, || {
        hip.check(unsafe { sys::ab_synth_generate_stack(hip.ctx, &synth_cfg(config), planes.as_mut_ptr(), &mut pt, stars.as_mut_ptr(), cap, &mut res) })
    })?;
    Ok((frames, truth, synth_stars_out(&stars[..res.star_count.min(cap)])))
}

// ---- core/imaging/wavelet.rs (wavelet_denoise_cmd) ------------------------------------------------------------------------------------------------------
/// the C view of a WaveletConfig; it borrows the threshold list, so it must not outlive `config`
fn wavelet_cfg(config: &WaveletConfig) -> sys::ab_wavelet_config {
    sys::ab_wavelet_config {
        num_scales: config.num_scales,
        // (the generated struct drops C's const: the library only reads the list)
        thresholds: if config.thresholds.is_empty() { std::ptr::null_mut() } else { config.thresholds.as_ptr() as *mut f32 },
        num_thresholds: config.thresholds.len(),
        linear_denoise: config.linear_denoise as i32,
    }
}
/// drop-in for wavelet_denoise (wavelet.rs:41-133), bit for bit; progress (2 S + 1 ticks, the reference's stage strings) and cancel included
pub fn wavelet_denoise(hip: &Hip, image: &impl PlaneSrc, config: &WaveletConfig, progress: Option<&ProgressHandle>) -> Result<WaveletResult> {
    let start = std::time::Instant::now();
    let mut out = Array2::<f32>::zeros(image.dims());
    let cfg = wavelet_cfg(config);
    let mut res: sys::ab_wavelet_result = unsafe { std::mem::zeroed() };
    let mut po = out.ab_mut();
    hip.with_progress(progress, || hip.check(unsafe { sys::ab_wavelet_denoise(hip.ctx, &image.ab(), &cfg, &mut po, &mut res) }))?;
    Ok(WaveletResult { denoised: out, scales_processed: res.scales_processed, noise_estimate: res.noise_estimate, elapsed_ms: start.elapsed().as_millis() as u64 })
}
/// the eight per-scale f32 thresholds wavelet_denoise derives from noise_sigma (wavelet.rs:93-99, :218-225): host maths in the library
pub fn wavelet_scale_thresholds(noise_sigma: f64, config: &WaveletConfig) -> Result<[f32; 8]> {
    let cfg = wavelet_cfg(config);
    let mut out = [0.0f32; 8];
    let rc = unsafe { sys::ab_wavelet_scale_thresholds(noise_sigma, &cfg, out.as_mut_ptr()) };
    if rc != sys::AB_OK {
        bail!("wavelet_scale_thresholds: invalid arguments (status {rc})");
    }
    Ok(out)
}

// ---- core/analysis/fft.rs (compute_fft_spectrum) --------------------------------------------------------------------------------------------------------
/// (original_size, display_size) of compute_power_spectrum (fft.rs:24-25, :53-57): host maths in the library
pub fn power_spectrum_dims(rows: usize, cols: usize) -> Result<(usize, usize)> {
    let (mut size, mut disp) = (0i64, 0i64);
    let rc = unsafe { sys::ab_power_spectrum_dims(rows as i64, cols as i64, &mut size, &mut disp) };
    if rc != sys::AB_OK {
        bail!("power_spectrum_dims: {rows} x {cols} is empty or beyond 16384 a side (status {rc})");
    }
    Ok((size as usize, disp as usize))
}
/// drop-in for window::hann_symmetric::<f32> (math/window.rs:20-35): host maths in the library
pub fn hann_symmetric_f32(n: usize) -> Vec<f32> {
    let mut w = vec![0.0f32; n];
    if n > 0 {
        unsafe { sys::ab_hann_symmetric_f32(n, w.as_mut_ptr()) };
    }
    w
}
/// prepare_windowed_buffer / prepare_buffer_no_window + FftEngine2D::<f32>::forward_2d (math/fft.rs:137-148, :202-245): the
/// fft_rows x fft_cols spectrum as interleaved (re, im) f32 in natural row-major order; `windows` = (win_y, win_x) or None
pub fn fft2_forward_f32(hip: &Hip, image: &impl PlaneSrc, windows: Option<(&[f32], &[f32])>, fft_rows: usize, fft_cols: usize) -> Result<Vec<f32>> {
    let (rows, cols) = image.dims();
    if let Some((wy, wx)) = windows {
        if wy.len() != rows || wx.len() != cols {
            bail!("fft2_forward_f32: the windows must hold {rows} and {cols} values");
        }
    }
    let mut out = vec![0.0f32; 2 * fft_rows * fft_cols];
    let (wy, wx) = windows.map_or((std::ptr::null(), std::ptr::null()), |(y, x)| (y.as_ptr(), x.as_ptr()));
    hip.check(unsafe { sys::ab_fft2_forward_f32(hip.ctx, &image.ab(), wy, wx, fft_rows as i64, fft_cols as i64, out.as_mut_ptr(), 0) })?;
    Ok(out)
}
/// drop-in for compute_power_spectrum_opts (fft.rs:23-68)
pub fn compute_power_spectrum_opts(hip: &Hip, data: &impl PlaneSrc, apply_window: bool) -> Result<FftResult> {
    let (rows, cols) = data.dims();
    let (_, disp) = power_spectrum_dims(rows, cols)?;
    let mut spectrum = Array2::<f32>::zeros((disp, disp));
    let mut res: sys::ab_fft_result = unsafe { std::mem::zeroed() };
    let mut po = spectrum.ab_mut();
    hip.check(unsafe { sys::ab_compute_power_spectrum(hip.ctx, &data.ab(), apply_window as i32, &mut po, &mut res) })?;
    Ok(FftResult {
        spectrum,
        display_width: res.display_cols as usize,
        display_height: res.display_rows as usize,
        original_size: res.original_size as usize,
        windowed: res.windowed != 0,
    })
}
/// drop-in for compute_power_spectrum (fft.rs:19-21)
pub fn compute_power_spectrum(hip: &Hip, data: &impl PlaneSrc) -> Result<FftResult> {
    compute_power_spectrum_opts(hip, data, true)
}
/// the per-pixel part of compute_fft_spectrum (cmd/analysis/mod.rs:66-96): (pixels, min_val, max_val, dc)
pub fn spectrum_to_u8(hip: &Hip, spectrum: &impl PlaneSrc) -> Result<(Vec<u8>, f32, f32, f32)> {
    let (r, c) = spectrum.dims();
    let mut out = vec![0u8; r * c];
    let (mut mn, mut mx, mut dc) = (0.0f32, 0.0f32, 0.0f32);
    hip.check(unsafe { sys::ab_spectrum_to_u8(hip.ctx, &spectrum.ab(), out.as_mut_ptr(), 0, &mut mn, &mut mx, &mut dc) })?;
    Ok((out, mn, mx, dc))
}

// ---- core/cube/{eager,lazy}.rs (process_cube_cmd, process_cube_lazy_cmd: cmd/cube.rs) --------------------------------------------------------------------
/// The two validity rules of the cube paths: eager (`finite && != 0.0`) and lazy (`stats::is_valid_pixel`)
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum CubeValidRule {
    NonZero = 0,
    AbovePadding = 1,
}
fn cube_ab(cube: &Array3<f32>) -> sys::ab_cube {
    let (depth, rows, cols) = cube.dim();
    let s = cube.as_slice().expect("contiguous");
    sys::ab_cube { data: s.as_ptr(), depth: depth as i64, rows: rows as i64, cols: cols as i64, on_device: 0 }
}
fn cube_stats_ab(g: &GlobalCubeStats) -> sys::ab_cube_stats {
    sys::ab_cube_stats { median: g.median, sigma: g.sigma, low: g.low, high: g.high }
}
/// collapse_mean under either rule (rule 1 = LazyCube::collapse_mean_lazy, lazy.rs:246-284, over the decoded frames)
pub fn collapse_mean_rule(hip: &Hip, cube: &Array3<f32>, rule: CubeValidRule) -> Result<Array2<f32>> {
    let (_, rows, cols) = cube.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    let mut po = out.ab_mut();
    hip.check(unsafe { sys::ab_cube_collapse_mean(hip.ctx, &cube_ab(cube), rule as i32, &mut po) })?;
    Ok(out)
}
/// drop-in for collapse_mean (eager.rs:24-26 = math/simd.rs:216-253): bit for bit
pub fn collapse_mean(hip: &Hip, cube: &Array3<f32>) -> Result<Array2<f32>> {
    collapse_mean_rule(hip, cube, CubeValidRule::NonZero)
}
/// collapse_median under either rule (rule 1 = LazyCube::collapse_median_lazy, lazy.rs:286-329)
pub fn collapse_median_rule(hip: &Hip, cube: &Array3<f32>, rule: CubeValidRule) -> Result<Array2<f32>> {
    let (_, rows, cols) = cube.dim();
    let mut out = Array2::<f32>::zeros((rows, cols));
    let mut po = out.ab_mut();
    hip.check(unsafe { sys::ab_cube_collapse_median(hip.ctx, &cube_ab(cube), rule as i32, &mut po) })?;
    Ok(out)
}
/// drop-in for collapse_median (eager.rs:28-55): bit for bit
pub fn collapse_median(hip: &Hip, cube: &Array3<f32>) -> Result<Array2<f32>> {
    collapse_median_rule(hip, cube, CubeValidRule::NonZero)
}
/// the frame stride of compute_global_stats_streaming (lazy.rs:334-335): host maths in the library
pub fn cube_streaming_step(depth: usize) -> usize {
    unsafe { sys::ab_cube_streaming_step(depth as i64) as usize }
}
/// the global statistics over every `frame_step`-th frame under `rule`, and the number of valid values they were taken from
pub fn compute_global_stats_sampled(hip: &Hip, cube: &Array3<f32>, rule: CubeValidRule, frame_step: usize) -> Result<(GlobalCubeStats, u64)> {
    let mut st: sys::ab_cube_stats = unsafe { std::mem::zeroed() };
    let mut n = 0u64;
    hip.check(unsafe { sys::ab_cube_global_stats(hip.ctx, &cube_ab(cube), rule as i32, frame_step as i64, &mut st, &mut n) })?;
    Ok((GlobalCubeStats { median: st.median, sigma: st.sigma, low: st.low, high: st.high }, n))
}
/// drop-in for compute_global_stats (eager.rs:168-208): bit for bit
pub fn compute_global_stats(hip: &Hip, cube: &Array3<f32>) -> Result<GlobalCubeStats> {
    Ok(compute_global_stats_sampled(hip, cube, CubeValidRule::NonZero, 1)?.0)
}
/// drop-in for LazyCube::compute_global_stats_streaming (lazy.rs:331-370) over the decoded frames: bit for bit
pub fn compute_global_stats_streaming(hip: &Hip, cube: &Array3<f32>) -> Result<GlobalCubeStats> {
    Ok(compute_global_stats_sampled(hip, cube, CubeValidRule::AbovePadding, cube_streaming_step(cube.dim().0))?.0)
}
/// drop-in for normalize_with_global (eager.rs:210-222): the f32 rounding of the f64 asinh, within 2 f32 ulp of f32::asinh
pub fn normalize_with_global(hip: &Hip, data: &impl PlaneSrc, g: &GlobalCubeStats) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(data.dims());
    let mut po = out.ab_mut();
    hip.check(unsafe { sys::ab_cube_normalize_frame(hip.ctx, &data.ab(), &cube_stats_ab(g), &mut po) })?;
    Ok(out)
}
/// drop-in for normalize_frame_with_stats (lazy.rs:87-99)
pub fn normalize_frame_with_stats(hip: &Hip, data: &impl PlaneSrc, stats: &GlobalCubeStats) -> Result<Array2<f32>> {
    normalize_with_global(hip, data, stats)
}
/// the per-pixel work of export_cube_frames_sampled (eager.rs:224-246) / process_cube_lazy's frame loop (lazy.rs:414-420): the L8
/// bytes of every `step`-th frame, frame k at [k * rows * cols ..], and the frame count; the caller encodes the PNGs
pub fn export_cube_frames(hip: &Hip, cube: &Array3<f32>, g: &GlobalCubeStats, step: usize) -> Result<(Vec<u8>, usize)> {
    let (depth, rows, cols) = cube.dim();
    let step = step.max(1);
    let frames = (depth + step - 1) / step;
    let mut out = vec![0u8; frames * rows * cols];
    let mut count = 0i64;
    hip.check(unsafe { sys::ab_cube_export_frames(hip.ctx, &cube_ab(cube), &cube_stats_ab(g), step as i64, out.as_mut_ptr(), 0, &mut count) })?;
    Ok((out, count as usize))
}
/// drop-in for extract_spectrum (eager.rs:57-60) with LazyCube::extract_spectrum_at's bounds error (lazy.rs:222-239)
pub fn extract_spectrum(hip: &Hip, cube: &Array3<f32>, y: usize, x: usize) -> Result<Vec<f32>> {
    let mut out = vec![0.0f32; cube.dim().0];
    hip.check(unsafe { sys::ab_cube_extract_spectrum(hip.ctx, &cube_ab(cube), y as i64, x as i64, out.as_mut_ptr(), 0) })?;
    Ok(out)
}

// ---- render_asinh_and_save (cmd/common.rs:242-261), math/simd.rs:160-214, infra/render/grayscale.rs -------------------------------------------------------------
/// The two routes of asinh_normalize_simd: what an x86-64 host with AVX2 runs (the default: the reference's published hardware), and
/// the scalar loop every other host runs
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum AsinhRoute {
    Avx2 = 0,
    Scalar = 1,
}
/// what asinh_normalize_simd takes from the valid pixels (simd.rs:163-180)
#[derive(Clone, Copy, Debug)]
pub struct AsinhStats {
    pub median: f32,
    pub sigma: f32,
    pub low: f32,
    pub high: f32,
    pub valid_count: u64,
}
fn asinh_stats_zeroed() -> sys::ab_asinh_stats {
    sys::ab_asinh_stats { median: 0.0, sigma: 0.0, low: 0.0, high: 0.0, valid_count: 0 }
}
fn asinh_stats_from(st: &sys::ab_asinh_stats) -> AsinhStats {
    AsinhStats { median: st.median, sigma: st.sigma, low: st.low, high: st.high, valid_count: st.valid_count }
}
/// the statistics alone: median, MAD sigma, the 1 % and 99.9 % order statistics; bit for bit
pub fn asinh_preview_stats(hip: &Hip, data: &impl PlaneSrc) -> Result<AsinhStats> {
    let mut st = asinh_stats_zeroed();
    hip.check(unsafe { sys::ab_asinh_preview_stats(hip.ctx, &data.ab(), &mut st) })?;
    Ok(asinh_stats_from(&st))
}
/// the map alone, with the caller's statistics
pub fn asinh_normalize_with_stats(hip: &Hip, data: &impl PlaneSrc, stats: &AsinhStats, route: AsinhRoute) -> Result<Array2<f32>> {
    let st = sys::ab_asinh_stats { median: stats.median, sigma: stats.sigma, low: stats.low, high: stats.high, valid_count: stats.valid_count };
    let mut out = Array2::<f32>::zeros(data.dims());
    let mut po = out.ab_mut();
    hip.check(unsafe { sys::ab_asinh_normalize_with_stats(hip.ctx, &data.ab(), &st, route as i32, &mut po) })?;
    Ok(out)
}
/// asinh_normalize_simd under either route
pub fn robust_asinh_preview_route(hip: &Hip, data: &impl PlaneSrc, route: AsinhRoute) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(data.dims());
    let mut po = out.ab_mut();
    hip.check(unsafe { sys::ab_robust_asinh_preview(hip.ctx, &data.ab(), route as i32, &mut po, std::ptr::null_mut()) })?;
    Ok(out)
}
/// drop-in for robust_asinh_preview (core/imaging/normalize.rs = math::simd::asinh_normalize_simd, simd.rs:160-214), the AVX2 route:
/// bit for bit
pub fn robust_asinh_preview(hip: &Hip, data: &impl PlaneSrc) -> Result<Array2<f32>> {
    robust_asinh_preview_route(hip, data, AsinhRoute::Avx2)
}
/// render_asinh_and_save (cmd/common.rs:242-261) up to the encoder: the L8 bytes of render_grayscale(robust_asinh_preview(data)), the
/// f32 preview never written; the caller hands them to write_png_l8.  `data` is typically the DevicePlane a stack or a collapse left.
pub fn render_asinh_preview(hip: &Hip, data: &impl PlaneSrc, route: AsinhRoute) -> Result<Vec<u8>> {
    let (r, c) = data.dims();
    let mut out = vec![0u8; r * c];
    hip.check(unsafe { sys::ab_render_asinh_preview(hip.ctx, &data.ab(), route as i32, out.as_mut_ptr(), 0, std::ptr::null_mut()) })?;
    Ok(out)
}
fn render_bytes(hip: &Hip, data: &impl PlaneSrc, bits: i32, stretched: bool) -> Result<Vec<u8>> {
    let (r, c) = data.dims();
    let mut out = vec![0u8; r * c * (bits as usize / 8)];
    let p = out.as_mut_ptr() as *mut c_void;
    hip.check(unsafe {
        if stretched {
            sys::ab_render_stretched(hip.ctx, &data.ab(), bits, p, 0)
        } else {
            sys::ab_render_grayscale(hip.ctx, &data.ab(), bits, p, 0, std::ptr::null_mut(), std::ptr::null_mut())
        }
    })?;
    Ok(out)
}
/// drop-in for render_grayscale (grayscale.rs:10-29) up to write_png_l8: the L8 bytes
pub fn render_grayscale(hip: &Hip, data: &impl PlaneSrc) -> Result<Vec<u8>> {
    render_bytes(hip, data, 8, false)
}
/// drop-in for render_grayscale_16bit (grayscale.rs:31-50) up to the encoder: the big-endian byte pairs write_png_l16 builds
pub fn render_grayscale_16bit(hip: &Hip, data: &impl PlaneSrc) -> Result<Vec<u8>> {
    render_bytes(hip, data, 16, false)
}
/// drop-in for render_stretched_8bit (grayscale.rs:52-62) up to write_png_l8
pub fn render_stretched_8bit(hip: &Hip, data: &impl PlaneSrc) -> Result<Vec<u8>> {
    render_bytes(hip, data, 8, true)
}
/// drop-in for render_stretched_16bit (grayscale.rs:64-74) up to the encoder: big-endian byte pairs
pub fn render_stretched_16bit(hip: &Hip, data: &impl PlaneSrc) -> Result<Vec<u8>> {
    render_bytes(hip, data, 16, true)
}

// ---- core/stacking/drizzle.rs (calibration.rs:320 drizzle_from_paths, drizzle_rgb_cmd) ----------------------------------------------------------------------
fn drizzle_cfg(config: &DrizzleConfig) -> sys::ab_drizzle_config {
    sys::ab_drizzle_config {
        scale: config.scale,
        pixfrac: config.pixfrac,
        kernel: match config.kernel { DrizzleKernel::Square => 0, DrizzleKernel::Gaussian => 1, DrizzleKernel::Lanczos3 => 2 },
        sigma_low: config.sigma_low,
        sigma_high: config.sigma_high,
        sigma_iterations: config.sigma_iterations,
        align: config.align as i32,
        alignment_method: match config.alignment_method { AlignmentMethod::PhaseCorrelation => 0, AlignmentMethod::Zncc => 1 },
        num_threads: rayon::current_num_threads() as i32,
    }
}
fn drizzle_fail(n: usize) -> anyhow::Error {
    // (the host-only entry point has no context to carry the message: the reference's own strings, drizzle.rs:231-254)
    match n {
        0 => anyhow::anyhow!("No images to drizzle"),
        1 => anyhow::anyhow!("Drizzle requires at least 2 frames for sub-pixel reconstruction"),
        _ => anyhow::anyhow!("Frame dimensions vary too much"),
    }
}
/// the checks and dims of drizzle_stack (drizzle.rs:231-279): ((in_rows, in_cols), (out_rows, out_cols)); host-only
pub fn drizzle_output_dims<P: PlaneSrc>(images: &[P], config: &DrizzleConfig) -> Result<((usize, usize), (usize, usize))> {
    let planes: Vec<_> = images.iter().map(|i| i.ab()).collect();
    let (mut ir, mut ic, mut or, mut oc) = (0i64, 0i64, 0i64, 0i64);
    if unsafe { sys::ab_drizzle_output_dims(planes.as_ptr(), planes.len(), &drizzle_cfg(config), &mut ir, &mut ic, &mut or, &mut oc) } != 0 {
        return Err(drizzle_fail(images.len()));
    }
    Ok(((ir as usize, ic as usize), (or as usize, oc as usize)))
}
fn drizzle_run<P: PlaneSrc>(hip: &Hip, images: &[P], offsets: Option<&[(f64, f64)]>, config: &DrizzleConfig) -> Result<DrizzleResult> {
    let (_, (out_rows, out_cols)) = drizzle_output_dims(images, config)?;
    let planes: Vec<_> = images.iter().map(|i| i.ab()).collect();
    let mut image = Array2::<f32>::zeros((out_rows, out_cols));
    let mut weight_map = Array2::<f32>::zeros((out_rows, out_cols));
    let (mut pi, mut pw) = (image.ab_mut(), weight_map.ab_mut());
    let mut res: sys::ab_drizzle_result = unsafe { std::mem::zeroed() };
    let mut off = vec![0f64; 2 * images.len()];
    let cfg = drizzle_cfg(config);
    match offsets {
        Some(o) => {
            if o.len() != images.len() {
                bail!("drizzle_frames: one (dx, dy) per frame");
            }
            for (k, (dx, dy)) in o.iter().enumerate() {
                off[2 * k] = *dx;
                off[2 * k + 1] = *dy;
            }
            hip.check(unsafe { sys::ab_drizzle_frames(hip.ctx, planes.as_ptr(), planes.len(), off.as_ptr(), &cfg, &mut pi, &mut pw, &mut res) })?
        }
        None => hip.check(unsafe { sys::ab_drizzle_stack(hip.ctx, planes.as_ptr(), planes.len(), &cfg, &mut pi, &mut pw, off.as_mut_ptr(), &mut res) })?,
    }
    Ok(DrizzleResult {
        image,
        weight_map,
        frame_count: res.frame_count,
        output_scale: res.output_scale,
        input_dims: (res.in_rows as usize, res.in_cols as usize),
        output_dims: (res.out_rows as usize, res.out_cols as usize),
        offsets: off.chunks(2).map(|c| (c[0], c[1])).collect(),
        rejected_pixels: res.rejected_pixels,
    })
}
/// drop-in for core::stacking::drizzle::drizzle_stack (drizzle.rs:227-346); frames host or device
pub fn drizzle_stack<P: PlaneSrc>(hip: &Hip, images: &[P], config: &DrizzleConfig) -> Result<DrizzleResult> {
    drizzle_run(hip, images, None, config)
}
/// drizzle_stack with offsets the caller already has (one (dx, dy) per frame, as DrizzleResult.offsets reports them): the
/// registration of an earlier run, a plate solution, a dither log
pub fn drizzle_frames<P: PlaneSrc>(hip: &Hip, images: &[P], offsets: &[(f64, f64)], config: &DrizzleConfig) -> Result<DrizzleResult> {
    drizzle_run(hip, images, Some(offsets), config)
}

// ---- the colour finish: core/compose/drizzle_rgb.rs, infra/render/rgb.rs, cmd/export/mod.rs (export_png, export_rgb_png) --------------------------------------
/// the three packers of the reference's colour writers: render_rgb's truncation, drizzle_rgb's rounding, render_rgb_16bit's big-endian pairs
#[derive(Clone, Copy, PartialEq, Eq, Debug)]
pub enum RgbPack {
    U8 = 0,
    U8Round = 1,
    U16Be = 2,
}
/// rows * cols * 3 bytes, twice that for RgbPack::U16Be; host-only
pub fn rgb_packed_bytes(rows: usize, cols: usize, pack: RgbPack) -> Result<usize> {
    let mut n = 0usize;
    if unsafe { sys::ab_rgb_packed_bytes(rows as i64, cols as i64, pack as i32, &mut n) } != 0 {
        bail!("an RGB buffer of {} x {} pixels cannot be sized (an empty image, or 2^31 pixels or more)", cols, rows);
    }
    Ok(n)
}
/// the packer alone on three stretched planes of one size: the interleaved bytes the reference hands its encoder
pub fn render_rgb_packed(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, pack: RgbPack) -> Result<Vec<u8>> {
    let (rows, cols) = r.dims();
    let mut out = vec![0u8; rgb_packed_bytes(rows, cols, pack)?];
    hip.check(unsafe { sys::ab_render_rgb(hip.ctx, &r.ab(), &g.ab(), &b.ab(), pack as i32, out.as_mut_ptr() as *mut c_void, 0) })?;
    Ok(out)
}
/// drop-in for render_rgb (infra/render/rgb.rs:7-47) up to the encoder: Rgb8 bytes at full size
pub fn render_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc) -> Result<Vec<u8>> {
    render_rgb_packed(hip, r, g, b, RgbPack::U8)
}
/// drop-in for render_rgb_16bit (rgb.rs:49-91) up to the encoder: the big-endian byte pairs its flat_map(to_be_bytes) builds
pub fn render_rgb_16bit(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc) -> Result<Vec<u8>> {
    render_rgb_packed(hip, r, g, b, RgbPack::U16Be)
}
/// apply_stf_f32 x 3 and the packer in one launch (export/mod.rs:189-207, :321-328): the three stretched planes are never written
pub fn render_rgb_stf(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, stf: &[StfParams; 3], stats: &[ImageStats; 3], pack: RgbPack) -> Result<Vec<u8>> {
    let (rows, cols) = r.dims();
    let mut out = vec![0u8; rgb_packed_bytes(rows, cols, pack)?];
    let p = [stf_to_sys(&stf[0]), stf_to_sys(&stf[1]), stf_to_sys(&stf[2])];
    let s = [stats_to_sys(&stats[0]), stats_to_sys(&stats[1]), stats_to_sys(&stats[2])];
    hip.check(unsafe { sys::ab_render_rgb_stf(hip.ctx, &r.ab(), &g.ab(), &b.ab(), p.as_ptr(), s.as_ptr(), pack as i32, out.as_mut_ptr() as *mut c_void, 0) })?;
    Ok(out)
}
/// what export_rgb_png's stretch_and_render (cmd/export/mod.rs:357-409) derives on its way to the encoder
pub struct RgbExport {
    pub pixels: Vec<u8>,
    pub rows: usize,
    pub cols: usize,
    pub resampled: bool,
    pub stats: [ImageStats; 3],
    pub stf: [StfParams; 3],
}
/// stretch_and_render whole: resample to the largest dims where they differ, statistics, the explicit STF or the linked one, the bytes
/// of render_rgb (bit_depth 8) / render_rgb_16bit (16)
pub fn export_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, bit_depth: u8, explicit_stf: Option<&[StfParams; 3]>) -> Result<RgbExport> {
    let dims = [r.dims(), g.dims(), b.dims()];
    let rows = dims.iter().map(|d| d.0).max().unwrap();
    let cols = dims.iter().map(|d| d.1).max().unwrap();
    let mut cfg: sys::ab_rgb_export_config = unsafe { std::mem::zeroed() };
    cfg.bits = bit_depth as i32;
    if let Some(p) = explicit_stf {
        cfg.has_stf = 1;
        cfg.stf = [stf_to_sys(&p[0]), stf_to_sys(&p[1]), stf_to_sys(&p[2])];
    }
    let mut pixels = vec![0u8; rgb_packed_bytes(rows, cols, if bit_depth == 16 { RgbPack::U16Be } else { RgbPack::U8 })?];
    let mut info: sys::ab_rgb_export_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_export_rgb(hip.ctx, &r.ab(), &g.ab(), &b.ab(), &cfg, pixels.as_mut_ptr() as *mut c_void, 0, &mut info) })?;
    Ok(RgbExport {
        pixels,
        rows: info.rows as usize,
        cols: info.cols as usize,
        resampled: info.resampled != 0,
        stats: [stats_from_sys(&info.stats[0]), stats_from_sys(&info.stats[1]), stats_from_sys(&info.stats[2])],
        stf: [stf_from_sys(&info.stf[0]), stf_from_sys(&info.stf[1]), stf_from_sys(&info.stf[2])],
    })
}
fn drizzle_rgb_cfg(config: &DrizzleRgbConfig) -> sys::ab_drizzle_rgb_config {
    let mut cfg: sys::ab_drizzle_rgb_config = unsafe { std::mem::zeroed() };
    match config.white_balance {
        WhiteBalance::Auto => cfg.white_balance = 0,
        WhiteBalance::Manual(x, y, z) => {
            cfg.white_balance = 1;
            cfg.wb_manual = [x, y, z];
        }
        WhiteBalance::None => cfg.white_balance = 2,
    }
    cfg.auto_stretch = config.auto_stretch as i32;
    cfg.linked_stf = config.linked_stf as i32;
    if let Some(s) = config.scnr.as_ref() {
        cfg.has_scnr = 1;
        cfg.scnr = scnr_to_sys(s);
    }
    cfg
}
fn planes3(rows: usize, cols: usize) -> [Array2<f32>; 3] {
    [Array2::<f32>::zeros((rows, cols)), Array2::<f32>::zeros((rows, cols)), Array2::<f32>::zeros((rows, cols))]
}
fn processed_drizzle_rgb(stretched: [Array2<f32>; 3], wb: [Array2<f32>; 3], info: &sys::ab_processed_drizzle_rgb_info) -> ProcessedDrizzleRgb {
    let cs = |i: usize| ChannelStats { min: info.chan_stats[i][0], max: info.chan_stats[i][1], median: info.chan_stats[i][2], mean: info.chan_stats[i][3] };
    let [r_stretched, g_stretched, b_stretched] = stretched;
    let [r_wb, g_wb, b_wb] = wb;
    ProcessedDrizzleRgb {
        r_stretched,
        g_stretched,
        b_stretched,
        r_wb,
        g_wb,
        b_wb,
        output_dims: (info.rows as usize, info.cols as usize),
        stf_r: stf_from_sys(&info.stf[0]),
        stf_g: stf_from_sys(&info.stf[1]),
        stf_b: stf_from_sys(&info.stf[2]),
        stats_r: cs(0),
        stats_g: cs(1),
        stats_b: cs(2),
        scnr_applied: info.scnr_applied != 0,
    }
}
/// drop-in for process_drizzle_rgb (core/compose/drizzle_rgb.rs:41-145) on the three optional channel images (the reference takes them
/// inside DrizzleRgbChannels, whose other fields it does not read) -- and the Rgb8 bytes drizzle_rgb builds from the result (:232-248)
pub fn process_drizzle_rgb(hip: &Hip, r: Option<&Array2<f32>>, g: Option<&Array2<f32>>, b: Option<&Array2<f32>>, config: &DrizzleRgbConfig) -> Result<(ProcessedDrizzleRgb, Vec<u8>)> {
    if r.is_none() && g.is_none() && b.is_none() {
        bail!("process_drizzle_rgb: at least one channel must be present");
    }
    let rows = [r, g, b].iter().flatten().map(|a| a.nrows()).min().unwrap();
    let cols = [r, g, b].iter().flatten().map(|a| a.ncols()).min().unwrap();
    let (pr, pg, pb) = (opt_plane(r), opt_plane(g), opt_plane(b));
    let (mut s, mut w) = (planes3(rows, cols), planes3(rows, cols));
    let mut ps = [s[0].ab_mut(), s[1].ab_mut(), s[2].ab_mut()];
    let mut pw = [w[0].ab_mut(), w[1].ab_mut(), w[2].ab_mut()];
    let mut pixels = vec![0u8; rgb_packed_bytes(rows, cols, RgbPack::U8Round)?];
    let mut info: sys::ab_processed_drizzle_rgb_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_process_drizzle_rgb(hip.ctx, opt_ptr(&pr), opt_ptr(&pg), opt_ptr(&pb), &drizzle_rgb_cfg(config), ps.as_mut_ptr(), pw.as_mut_ptr(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    Ok((processed_drizzle_rgb(s, w, &info), pixels))
}
/// what drizzle_rgb (drizzle_rgb.rs:159-286) holds when it reaches its writers: the Rgb8 bytes for RgbImage::from_raw, the three
/// white-balanced planes for write_fits_rgb, and DrizzleRgbResult's scalars
pub struct DrizzleRgbOutput {
    pub pixels: Vec<u8>,
    pub wb: [Array2<f32>; 3],
    pub input_dims: (usize, usize),
    pub output_dims: (usize, usize),
    pub scale: f64,
    pub frame_counts: [usize; 3],
    pub rejected_pixels: u64,
    pub stf: [StfParams; 3],
    pub stats: [ChannelStats; 3],
    pub scnr_applied: bool,
}
/// drop-in for drizzle_rgb (drizzle_rgb.rs:159-286) up to the PNG / FITS writers, with the channels' frames in place of their paths: each
/// channel's drizzle stays on the device and only the bytes and the white-balanced planes come back
pub fn drizzle_rgb<P: PlaneSrc>(hip: &Hip, r: Option<&[P]>, g: Option<&[P]>, b: Option<&[P]>, config: &DrizzleRgbConfig) -> Result<DrizzleRgbOutput> {
    let lists = [r, g, b];
    let given = lists.iter().filter(|l| l.is_some()).count();
    if given < 2 {
        bail!("Need at least 2 channels for RGB drizzle (got {})", given); // :171-173
    }
    let mut dims = Vec::new();
    for l in lists.iter().flatten().filter(|l| l.len() >= 2) {
        dims.push(drizzle_output_dims(l, &config.drizzle)?.1);
    }
    if dims.is_empty() {
        bail!("All channels failed or have fewer than 2 frames"); // :203-205
    }
    let rows = dims.iter().map(|d| d.0).min().unwrap();
    let cols = dims.iter().map(|d| d.1).min().unwrap();
    let planes: Vec<Option<Vec<sys::ab_plane>>> = lists.iter().map(|l| l.map(|f| f.iter().map(|i| i.ab()).collect())).collect();
    let ptr = |i: usize| planes[i].as_ref().map_or(std::ptr::null(), |v| v.as_ptr());
    let len = |i: usize| planes[i].as_ref().map_or(0, |v| v.len());
    let mut w = planes3(rows, cols);
    let mut pw = [w[0].ab_mut(), w[1].ab_mut(), w[2].ab_mut()];
    let mut pixels = vec![0u8; rgb_packed_bytes(rows, cols, RgbPack::U8Round)?];
    let mut res: [sys::ab_drizzle_result; 3] = unsafe { std::mem::zeroed() };
    let mut info: sys::ab_processed_drizzle_rgb_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_drizzle_rgb(hip.ctx, ptr(0), len(0), ptr(1), len(1), ptr(2), len(2), &drizzle_cfg(&config.drizzle), &drizzle_rgb_cfg(config), pw.as_mut_ptr(), pixels.as_mut_ptr(), 0, res.as_mut_ptr(), &mut info)
    })?;
    let first = res.iter().find(|x| x.frame_count > 0).unwrap(); // :207-213
    let cs = |i: usize| ChannelStats { min: info.chan_stats[i][0], max: info.chan_stats[i][1], median: info.chan_stats[i][2], mean: info.chan_stats[i][3] };
    Ok(DrizzleRgbOutput {
        pixels,
        wb: w,
        input_dims: (first.in_rows as usize, first.in_cols as usize),
        output_dims: (info.rows as usize, info.cols as usize),
        scale: first.output_scale,
        frame_counts: [res[0].frame_count, res[1].frame_count, res[2].frame_count],
        rejected_pixels: res.iter().map(|x| x.rejected_pixels).sum(),
        stf: [stf_from_sys(&info.stf[0]), stf_from_sys(&info.stf[1]), stf_from_sys(&info.stf[2])],
        stats: [cs(0), cs(1), cs(2)],
        scnr_applied: info.scnr_applied != 0,
    })
}

// ---- the compose wizard's tone editor: cmd/processing/curves.rs (apply_tone_composite_cmd) ---------------------------------------------------------------------
/// apply_tone_composite_cmd's arguments (cmd/processing/curves.rs:58-71) as the command receives them, (r, g, b) each
#[derive(Clone, Debug, Default)]
pub struct ToneConfig {
    pub stf: [Option<[f64; 3]>; 3],
    pub linked_stf: Option<bool>,
    pub levels: [Option<LevelsParams>; 3],
    pub curves: [Option<Vec<[f64; 2]>>; 3],
    pub scnr: Option<ScnrConfig>,
}
/// what the command decided and reports (RES_STF, RES_LEVELS_APPLIED, RES_CURVES_APPLIED, RES_SCNR_APPLIED, :163-189)
#[derive(Clone, Debug)]
pub struct ToneInfo {
    pub stf: [StfParams; 3],
    pub norm: [ImageStats; 3],
    pub levels_applied: bool,
    pub curves_applied: bool,
    pub scnr_applied: bool,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
}
/// the preview the command encodes: preview_dims.0 x preview_dims.1 x 3 interleaved bytes (RgbImage::from_raw's input)
pub struct TonePreview {
    pub pixels: Vec<u8>,
    pub info: ToneInfo,
}
// `flat` holds the curves' points for as long as the configuration that points into it is in use
fn tone_cfg(config: &ToneConfig, flat: &mut [Vec<f64>; 3]) -> sys::ab_tone_config {
    let mut cfg: sys::ab_tone_config = unsafe { std::mem::zeroed() };
    unsafe { sys::ab_tone_config_default(&mut cfg) };
    for c in 0..3 {
        if let Some(a) = config.stf[c] {
            cfg.has_stf[c] = 1;
            cfg.stf[c] = sys::ab_stf_params { shadow: a[0], midtone: a[1], highlight: a[2] };
        }
        if let Some(l) = config.levels[c].as_ref() {
            cfg.levels[c] = sys::ab_levels_params { black: l.black, gamma: l.gamma, white: l.white };
        }
        if let Some(points) = config.curves[c].as_ref() {
            flat[c] = points.iter().flat_map(|p| [p[0], p[1]]).collect();
            flat[c].reserve(1); // Some(vec![]) is a pointer all the same: NULL means None
            cfg.curve_xy[c] = flat[c].as_mut_ptr();
            cfg.n_curve[c] = points.len();
        }
    }
    cfg.linked_stf = config.linked_stf.unwrap_or(false) as i32;
    if let Some(s) = config.scnr.as_ref() {
        cfg.has_scnr = 1;
        cfg.scnr = scnr_to_sys(s);
    }
    cfg
}
fn tone_info(info: &sys::ab_tone_info) -> ToneInfo {
    ToneInfo {
        stf: [stf_from_sys(&info.stf[0]), stf_from_sys(&info.stf[1]), stf_from_sys(&info.stf[2])],
        norm: [stats_from_sys(&info.norm[0]), stats_from_sys(&info.norm[1]), stats_from_sys(&info.norm[2])],
        levels_applied: info.levels_applied != 0,
        curves_applied: info.curves_applied != 0,
        scnr_applied: info.scnr_applied != 0,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
    }
}
/// the command's decisions without its pixels (:86-154); host-only
pub fn tone_plan(stats: &[ImageStats; 3], config: &ToneConfig) -> Result<ToneInfo> {
    let mut flat: [Vec<f64>; 3] = Default::default();
    let cfg = tone_cfg(config, &mut flat);
    let s = [stats_to_sys(&stats[0]), stats_to_sys(&stats[1]), stats_to_sys(&stats[2])];
    let mut info: sys::ab_tone_info = unsafe { std::mem::zeroed() };
    if unsafe { sys::ab_tone_plan(s.as_ptr(), &cfg, &mut info, std::ptr::null_mut()) } != 0 {
        bail!("the tone plan could not be computed");
    }
    Ok(tone_info(&info))
}
/// apply_tone_composite_cmd (cmd/processing/curves.rs:57-191) from its loaded channels to the encoder's input in one launch: STF, levels,
/// curves, SCNR and render_rgb_preview's pick and pack, only at the pixels the preview shows when the composite exceeds max_dim
pub fn apply_tone_composite(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, stats: &[ImageStats; 3], config: &ToneConfig, max_dim: usize) -> Result<TonePreview> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let mut flat: [Vec<f64>; 3] = Default::default();
    let cfg = tone_cfg(config, &mut flat);
    let s = [stats_to_sys(&stats[0]), stats_to_sys(&stats[1]), stats_to_sys(&stats[2])];
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_tone_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_apply_tone_composite(hip.ctx, &r.ab(), &g.ab(), &b.ab(), s.as_ptr(), &cfg, max_dim as i64, std::ptr::null_mut(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    Ok(TonePreview { pixels, info: tone_info(&info) })
}
/// the same with the three toned planes the command drops (r_img, g_img, b_img) as well: two launches when the composite exceeds max_dim
pub fn apply_tone_composite_planes(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, stats: &[ImageStats; 3], config: &ToneConfig, max_dim: usize) -> Result<([Array2<f32>; 3], TonePreview)> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let mut flat: [Vec<f64>; 3] = Default::default();
    let cfg = tone_cfg(config, &mut flat);
    let s = [stats_to_sys(&stats[0]), stats_to_sys(&stats[1]), stats_to_sys(&stats[2])];
    let mut planes = planes3(rows, cols);
    let mut pp = [planes[0].ab_mut(), planes[1].ab_mut(), planes[2].ab_mut()];
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_tone_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_apply_tone_composite(hip.ctx, &r.ab(), &g.ab(), &b.ab(), s.as_ptr(), &cfg, max_dim as i64, pp.as_mut_ptr(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    Ok((planes, TonePreview { pixels, info: tone_info(&info) }))
}

// ---- opening a file: cmd/io/mod.rs (process_fits, process_fits_full, process_rgb_fits), cmd/analysis/mod.rs (compute_histogram) ------------------------
/// drop-in for downsample_histogram (stats.rs:423-444) on the bins themselves; host-only
pub fn downsample_histogram(bins: &[u32], target_bins: usize) -> Result<Vec<u32>> {
    let mut out = vec![0u32; target_bins.min(bins.len())];
    let mut len = 0usize;
    if unsafe { sys::ab_downsample_histogram(bins.as_ptr(), bins.len(), target_bins, out.as_mut_ptr(), &mut len) } != 0 {
        bail!("downsample_histogram: no source bins or target_bins == 0");
    }
    out.truncate(len);
    Ok(out)
}
/// Histogram.bin_edges of build_histogram (stats.rs:379-387, :412-413); host-only
pub fn histogram_bin_edges(dmin: f64, dmax: f64, bins: usize) -> Result<Vec<f64>> {
    let mut out = vec![0.0f64; bins + 1];
    if unsafe { sys::ab_histogram_bin_edges(dmin, dmax, bins, out.as_mut_ptr()) } != 0 {
        bail!("histogram_bin_edges: bins == 0");
    }
    Ok(out)
}
/// downsample_histogram(&compute_histogram_with_stats(data, stats), target_bins) (stats.rs:373-376, :423-444) in one pass over the plane
pub fn display_histogram(hip: &Hip, data: &impl PlaneSrc, dmin: f64, dmax: f64, target_bins: usize) -> Result<Vec<u32>> {
    let mut out = vec![0u32; target_bins.clamp(1, 65536)];
    let mut len = 0usize;
    hip.check(unsafe { sys::ab_display_histogram(hip.ctx, &data.ab(), dmin, dmax, target_bins, out.as_mut_ptr(), 0, &mut len) })?;
    out.truncate(len);
    Ok(out)
}
/// what process_fits_full hands to the encoder and the JSON (cmd/io/mod.rs:138-170)
pub struct FitsView {
    pub pixels: Vec<u8>,
    pub display_bins: Vec<u32>,
    pub dims: (usize, usize),
    pub stats: ImageStats,
    pub stf: StfParams,
}
/// what process_rgb_fits hands over (cmd/io/mod.rs:44-99): preview_dims.0 x preview_dims.1 x 3 interleaved bytes, R's display bins
pub struct RgbFitsView {
    pub pixels: Vec<u8>,
    pub display_bins: Vec<u32>,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
    pub stats: [ImageStats; 3],
    pub stf: [StfParams; 3],
}
fn fits_view_cfg(config: &AutoStfConfig, hist_bins: usize) -> sys::ab_fits_view_config {
    let mut cfg: sys::ab_fits_view_config = unsafe { std::mem::zeroed() };
    unsafe { sys::ab_fits_view_config_default(&mut cfg) };
    cfg.stf = sys::ab_auto_stf_config { target_bg: config.target_bg, shadow_k: config.shadow_k };
    cfg.hist_bins = hist_bins;
    cfg
}
/// the mono branch of process_fits_full (hist_bins = 0: of process_fits) from the loaded plane to the encoder's input: statistics, auto_stf,
/// apply_stf and the display histogram as one device chain with one synchronisation
pub fn process_fits_view(hip: &Hip, arr: &impl PlaneSrc, config: &AutoStfConfig, hist_bins: usize) -> Result<FitsView> {
    let (rows, cols) = arr.dims();
    let cfg = fits_view_cfg(config, hist_bins);
    let mut pixels = vec![0u8; rows * cols];
    let mut bins = vec![0u32; hist_bins.min(65536)];
    let mut info: sys::ab_fits_view_info = unsafe { std::mem::zeroed() };
    let bins_ptr = if bins.is_empty() { std::ptr::null_mut() } else { bins.as_mut_ptr() };
    hip.check(unsafe { sys::ab_process_fits_view(hip.ctx, &arr.ab(), &cfg, pixels.as_mut_ptr(), 0, bins_ptr, 0, &mut info) })?;
    Ok(FitsView { pixels, display_bins: bins, dims: (info.rows as usize, info.cols as usize), stats: stats_from_sys(&info.stats), stf: stf_from_sys(&info.stf) })
}
/// process_rgb_fits from its three planes on (cmd/io/mod.rs:44-62): per-channel statistics and auto_stf, apply_stf_f32, render_rgb_preview and
/// R's display histogram as one device chain with one synchronisation
pub fn process_rgb_fits_view(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, config: &AutoStfConfig, hist_bins: usize, max_dim: usize) -> Result<RgbFitsView> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let cfg = fits_view_cfg(config, hist_bins);
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut bins = vec![0u32; hist_bins.min(65536)];
    let mut info: sys::ab_rgb_fits_view_info = unsafe { std::mem::zeroed() };
    let bins_ptr = if bins.is_empty() { std::ptr::null_mut() } else { bins.as_mut_ptr() };
    hip.check(unsafe {
        sys::ab_process_rgb_fits_view(hip.ctx, &r.ab(), &g.ab(), &b.ab(), &cfg, max_dim as i64, pixels.as_mut_ptr(), 0, bins_ptr, 0, &mut info)
    })?;
    Ok(RgbFitsView {
        pixels,
        display_bins: bins,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        stats: [stats_from_sys(&info.stats[0]), stats_from_sys(&info.stats[1]), stats_from_sys(&info.stats[2])],
        stf: [stf_from_sys(&info.stf[0]), stf_from_sys(&info.stf[1]), stf_from_sys(&info.stf[2])],
    })
}

// ---- the compose wizard's blend and colour steps: cmd/compose/blend.rs (blend_channels_cmd), cmd/compose/color.rs ----------------------------------------
/// how a channel's kept statistics were computed (color.rs:21-49, :138-159)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ColorStatsRoute {
    /// compute_image_stats of the final plane
    ExactOrFull,
    /// compute_image_stats_with_known_range of the final plane (a channel SCNR leaves alone, above 4 000 000 px)
    KnownRange,
}
fn route_from_sys(r: i32) -> ColorStatsRoute {
    if r == sys::AB_COLOR_STATS_KNOWN_RANGE as i32 { ColorStatsRoute::KnownRange } else { ColorStatsRoute::ExactOrFull }
}
/// calibrate_and_scnr_cmd's decisions (color.rs:115-117, :138-159)
#[derive(Clone, Debug)]
pub struct ColorPlan {
    pub factors: [f32; 3],
    pub scnr_applied: bool,
    pub route: [ColorStatsRoute; 3],
    pub known_range: [(f64, f64); 3],
}
/// what calibrate_and_scnr_cmd encodes and reports beside the planes it caches as __composite_r / _g / _b: pixels is RgbImage::from_raw's input
pub struct ColorStep {
    pub pixels: Vec<u8>,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
    pub factors: [f32; 3],
    pub scnr_applied: bool,
    pub route: [ColorStatsRoute; 3],
    pub stats: [ImageStats; 3],
    pub stf: StfParams,
}
/// what blend_channels_cmd encodes and reports beside the planes it caches (blend.rs:185-221)
pub struct BlendComposite {
    pub pixels: Vec<u8>,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
    pub resampled: bool,
    pub stats: [ImageStats; 3],
    pub stf: StfParams,
}
/// compute_auto_wb_cmd's JSON (color.rs:214-222)
#[derive(Clone, Debug)]
pub struct AutoWb {
    pub factors: [f64; 3],
    pub stability: [f64; 3],
    pub ref_channel: char,
}
fn scnr_arg(scnr: Option<&ScnrConfig>) -> (i32, sys::ab_scnr_config) {
    match scnr {
        Some(s) => (1, scnr_to_sys(s)),
        None => (0, unsafe { std::mem::zeroed() }),
    }
}
/// the colour step's decisions without its pixels; host-only
pub fn color_step_plan(n_pixels: usize, orig_stats: &[ImageStats; 3], factors: [f64; 3], scnr: Option<&ScnrConfig>) -> Result<ColorPlan> {
    let s = [stats_to_sys(&orig_stats[0]), stats_to_sys(&orig_stats[1]), stats_to_sys(&orig_stats[2])];
    let (has, cfg) = scnr_arg(scnr);
    let mut plan: sys::ab_color_plan = unsafe { std::mem::zeroed() };
    if unsafe { sys::ab_color_step_plan(n_pixels as u64, s.as_ptr(), factors.as_ptr(), has, &cfg, &mut plan) } != 0 {
        bail!("the colour step's plan could not be computed");
    }
    Ok(ColorPlan {
        factors: plan.factors,
        scnr_applied: plan.scnr_applied != 0,
        route: [route_from_sys(plan.route[0]), route_from_sys(plan.route[1]), route_from_sys(plan.route[2])],
        known_range: [(plan.known_min[0], plan.known_max[0]), (plan.known_min[1], plan.known_max[1]), (plan.known_min[2], plan.known_max[2])],
    })
}
/// calibrate_and_scnr_cmd (color.rs:97-184) from its loaded originals to the encoder's input as one device chain with one synchronisation:
/// white balance and SCNR in one kernel, the three statistics the command keeps, the linked STF and the preview
#[allow(clippy::too_many_arguments)]
pub fn calibrate_and_scnr_into(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, orig_stats: &[ImageStats; 3], factors: [f64; 3], scnr: Option<&ScnrConfig>, max_dim: usize,
                               out_r: &mut impl PlaneDst, out_g: &mut impl PlaneDst, out_b: &mut impl PlaneDst) -> Result<ColorStep> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let s = [stats_to_sys(&orig_stats[0]), stats_to_sys(&orig_stats[1]), stats_to_sys(&orig_stats[2])];
    let (has, cfg) = scnr_arg(scnr);
    let mut pp = [out_r.ab_mut(), out_g.ab_mut(), out_b.ab_mut()];
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_color_step_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_calibrate_and_scnr(hip.ctx, &r.ab(), &g.ab(), &b.ab(), s.as_ptr(), factors.as_ptr(), has, &cfg, max_dim as i64, pp.as_mut_ptr(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    Ok(ColorStep {
        pixels,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        factors: info.factors,
        scnr_applied: info.scnr_applied != 0,
        route: [route_from_sys(info.route[0]), route_from_sys(info.route[1]), route_from_sys(info.route[2])],
        stats: [stats_from_sys(&info.stats[0]), stats_from_sys(&info.stats[1]), stats_from_sys(&info.stats[2])],
        stf: stf_from_sys(&info.stf),
    })
}
/// the same into three host planes it allocates
pub fn calibrate_and_scnr(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, orig_stats: &[ImageStats; 3], factors: [f64; 3], scnr: Option<&ScnrConfig>, max_dim: usize) -> Result<([Array2<f32>; 3], ColorStep)> {
    let (rows, cols) = r.dims();
    let [mut pr, mut pg, mut pb] = planes3(rows, cols);
    let out = calibrate_and_scnr_into(hip, r, g, b, orig_stats, factors, scnr, max_dim, &mut pr, &mut pg, &mut pb)?;
    Ok(([pr, pg, pb], out))
}
/// the dims blend_channels_cmd blends at: the largest rows and the largest cols (blend.rs:148-150); Err on no channel (:139-141)
pub fn blend_composite_dims<P: PlaneSrc>(channels: &[P]) -> Result<(usize, usize)> {
    if channels.is_empty() {
        bail!("No channel paths provided");
    }
    Ok((channels.iter().map(|c| c.dims().0).max().unwrap(), channels.iter().map(|c| c.dims().1).max().unwrap()))
}
/// blend_channels_cmd (blend.rs:128-223) from its loaded channels on as one device chain with one synchronisation: the bicubic resample
/// of channels that differ in size, blend_channels, three statistics, the linked STF and the preview
pub fn blend_composite_into<P: PlaneSrc>(hip: &Hip, channels: &[P], weights: &[BlendWeight], max_dim: usize, out_r: &mut impl PlaneDst, out_g: &mut impl PlaneDst,
                                         out_b: &mut impl PlaneDst) -> Result<BlendComposite> {
    let (rows, cols) = blend_composite_dims(channels)?;
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let in_planes: Vec<_> = channels.iter().map(|c| c.ab()).collect();
    let w = blend_weights(weights);
    let mut pp = [out_r.ab_mut(), out_g.ab_mut(), out_b.ab_mut()];
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_blend_composite_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_blend_composite(hip.ctx, in_planes.as_ptr(), in_planes.len(), w.as_ptr(), w.len(), max_dim as i64, pp.as_mut_ptr(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    Ok(BlendComposite {
        pixels,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        resampled: info.resampled != 0,
        stats: [stats_from_sys(&info.stats[0]), stats_from_sys(&info.stats[1]), stats_from_sys(&info.stats[2])],
        stf: stf_from_sys(&info.stf),
    })
}
/// the same into three host planes it allocates
pub fn blend_composite<P: PlaneSrc>(hip: &Hip, channels: &[P], weights: &[BlendWeight], max_dim: usize) -> Result<([Array2<f32>; 3], BlendComposite)> {
    let (rows, cols) = blend_composite_dims(channels)?;
    let [mut r, mut g, mut b] = planes3(rows, cols);
    let out = blend_composite_into(hip, channels, weights, max_dim, &mut r, &mut g, &mut b)?;
    Ok(([r, g, b], out))
}
/// drop-in for the body of compute_auto_wb_cmd (color.rs:192-222); host-only
pub fn compute_auto_wb(sr: &ImageStats, sg: &ImageStats, sb: &ImageStats) -> Result<AutoWb> {
    let mut out: sys::ab_auto_wb = unsafe { std::mem::zeroed() };
    if unsafe { sys::ab_compute_auto_wb(&stats_to_sys(sr), &stats_to_sys(sg), &stats_to_sys(sb), &mut out) } != 0 {
        bail!("compute_auto_wb: null argument");
    }
    Ok(AutoWb { factors: out.factors, stability: out.stability, ref_channel: ['R', 'G', 'B'][out.ref_channel as usize] })
}

// ---- a13  core/imaging/star_mask.rs, masked_stretch.rs -------------------------------------------------------------------------------------------------
/// drop-in for generate_star_mask (star_mask.rs:38-44)
pub fn generate_star_mask(hip: &Hip, image: &impl PlaneSrc, config: &StarMaskConfig) -> Result<StarMaskResult, String> {
    let mut mask = Array2::<f32>::zeros(image.dims());
    let mut info = sys::ab_star_mask_info { stars_masked: 0, coverage_fraction: 0.0 };
    hip.check(unsafe { sys::ab_generate_star_mask(hip.ctx, &image.ab(), &mask_cfg(config), &mut mask.ab_mut(), &mut info) }).map_err(|e| e.to_string())?;
    Ok(StarMaskResult { mask, stars_masked: info.stars_masked, coverage_fraction: info.coverage_fraction })
}
/// drop-in for generate_star_mask_from_detection (star_mask.rs:46-138)
pub fn generate_star_mask_from_detection(hip: &Hip, image: &impl PlaneSrc, detection: &DetectionResult, config: &StarMaskConfig) -> Result<StarMaskResult, String> {
    let stars: Vec<_> = detection.stars.iter().map(star_to_sys).collect();
    let mut mask = Array2::<f32>::zeros(image.dims());
    let mut info = sys::ab_star_mask_info { stars_masked: 0, coverage_fraction: 0.0 };
    hip.check(unsafe { sys::ab_generate_star_mask_from_stars(hip.ctx, &image.ab(), stars.as_ptr(), stars.len(), &mask_cfg(config), &mut mask.ab_mut(), &mut info) })
        .map_err(|e| e.to_string())?;
    Ok(StarMaskResult { mask, stars_masked: info.stars_masked, coverage_fraction: info.coverage_fraction })
}
/// drop-in for masked_stretch (masked_stretch.rs:44-58)
pub fn masked_stretch(hip: &Hip, image: &impl PlaneSrc, config: &MaskedStretchConfig) -> Result<MaskedStretchResult, String> {
    let mut out = Array2::<f32>::zeros(image.dims());
    let mut res: sys::ab_masked_stretch_result = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_masked_stretch(hip.ctx, &image.ab(), &masked_cfg(config), &mut out.ab_mut(), &mut res) }).map_err(|e| e.to_string())?;
    Ok(masked_res(out, &res))
}
/// drop-in for masked_stretch_with_mask (masked_stretch.rs:60-118)
pub fn masked_stretch_with_mask(hip: &Hip, image: &impl PlaneSrc, mask_result: &StarMaskResult, config: &MaskedStretchConfig) -> Result<MaskedStretchResult, String> {
    let mut out = Array2::<f32>::zeros(image.dims());
    let mut res: sys::ab_masked_stretch_result = unsafe { std::mem::zeroed() };
    let info = sys::ab_star_mask_info { stars_masked: mask_result.stars_masked, coverage_fraction: mask_result.coverage_fraction };
    hip.check(unsafe { sys::ab_masked_stretch_with_mask(hip.ctx, &image.ab(), &mask_result.mask.ab(), &info, &masked_cfg(config), &mut out.ab_mut(), &mut res) })
        .map_err(|e| e.to_string())?;
    Ok(masked_res(out, &res))
}
/// drop-in for masked_stretch_rgb_shared (masked_stretch.rs:157-193)
pub fn masked_stretch_rgb_shared(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, config: &MaskedStretchConfig) -> Result<MaskedStretchRgbResult, String> {
    let d = r.dims();
    let (mut or, mut og, mut ob) = (Array2::<f32>::zeros(d), Array2::<f32>::zeros(d), Array2::<f32>::zeros(d));
    let (res3, shared) = masked_stretch_rgb_shared_into(hip, r, g, b, config, &mut or, &mut og, &mut ob).map_err(|e| e.to_string())?;
    Ok(MaskedStretchRgbResult {
        r: masked_res(or, &res3[0]),
        g: masked_res(og, &res3[1]),
        b: masked_res(ob, &res3[2]),
        shared_mask_coverage: shared.coverage_fraction,
        shared_stars_masked: shared.stars_masked,
    })
}
pub fn masked_stretch_rgb_shared_into(
    hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, config: &MaskedStretchConfig,
    out_r: &mut impl PlaneDst, out_g: &mut impl PlaneDst, out_b: &mut impl PlaneDst,
) -> Result<([sys::ab_masked_stretch_result; 3], sys::ab_star_mask_info)> {
    let mut res3: [sys::ab_masked_stretch_result; 3] = unsafe { std::mem::zeroed() };
    let mut shared = sys::ab_star_mask_info { stars_masked: 0, coverage_fraction: 0.0 };
    hip.check(unsafe {
        sys::ab_masked_stretch_rgb_shared(hip.ctx, &r.ab(), &g.ab(), &b.ab(), &masked_cfg(config), &mut out_r.ab_mut(), &mut out_g.ab_mut(), &mut out_b.ab_mut(), res3.as_mut_ptr(), &mut shared)
    })?;
    Ok((res3, shared))
}

// ---- the compose wizard's stretch step: cmd/processing/stretch.rs, core/imaging/stretch.rs:47-90 -----------------------------------------------------------
/// what arcsinh_stretch_composite_cmd encodes and reports (stretch.rs:94-124): pixels is RgbImage::from_raw's input
pub struct ArcsinhComposite {
    pub pixels: Vec<u8>,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
    pub factor: f32,
    pub global_range: (f32, f32),
    pub degenerate: bool,
}
/// what apply_arcsinh_stretch_cmd saves and reports (stretch.rs:15-43 with render_and_save, cmd/common.rs:209-240)
pub struct ArcsinhView {
    pub stretched: Array2<f32>,
    pub pixels: Vec<u8>,
    pub dims: (usize, usize),
    pub factor: f32,
    pub data_range: (f32, f32),
    pub degenerate: bool,
    pub stats: ImageStats,
    pub stf: StfParams,
}
/// one channel of masked_stretch_composite_cmd's "channels" (stretch.rs:126-132)
#[derive(Clone, Copy, Debug)]
pub struct MaskedChannelStats {
    pub iterations_run: usize,
    pub final_background: f64,
    pub converged: bool,
}
/// what masked_stretch_composite_cmd encodes and reports (stretch.rs:135-221)
pub struct MaskedStretchComposite {
    pub pixels: Vec<u8>,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
    pub channels: [MaskedChannelStats; 3],
    pub stars_masked: usize,
    pub mask_coverage: f64,
    pub mask_mode: &'static str,
}
fn opt_ptr(v: &Option<f32>) -> *const f32 {
    match v {
        Some(x) => x as *const f32,
        None => std::ptr::null(),
    }
}
/// the fold of stretch.rs:72-78 over three channels' cached statistics: (global_min, global_max); host-only
pub fn arcsinh_rgb_range(sr: &ImageStats, sg: &ImageStats, sb: &ImageStats) -> (f32, f32) {
    let s = [stats_to_sys(sr), stats_to_sys(sg), stats_to_sys(sb)];
    let mut mm = [0f32; 2];
    unsafe { sys::ab_arcsinh_rgb_range(s.as_ptr(), mm.as_mut_ptr()) };
    (mm[0], mm[1])
}
/// drop-in for arcsinh_stretch_rgb_with_stats (core/imaging/stretch.rs:56-90): one range pass unless both values are given, one kernel
pub fn arcsinh_stretch_rgb_with_stats(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, global_min: Option<f32>, global_max: Option<f32>, factor: f32,
                                      gamma: f32) -> Result<(Array2<f32>, Array2<f32>, Array2<f32>)> {
    let (rows, cols) = r.dims();
    let [mut or, mut og, mut ob] = planes3(rows, cols);
    // (Some, None) and (None, Some) compute the range like (None, None): stretch.rs:69-71
    let (mn, mx) = if global_min.is_some() && global_max.is_some() { (global_min, global_max) } else { (None, None) };
    let mut pp = [or.ab_mut(), og.ab_mut(), ob.ab_mut()];
    hip.check(unsafe { sys::ab_arcsinh_stretch_rgb(hip.ctx, &r.ab(), &g.ab(), &b.ab(), opt_ptr(&mn), opt_ptr(&mx), factor, gamma, pp.as_mut_ptr(), std::ptr::null_mut()) })?;
    Ok((or, og, ob))
}
/// drop-in for arcsinh_stretch_rgb (core/imaging/stretch.rs:47-54)
pub fn arcsinh_stretch_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, factor: f32) -> Result<(Array2<f32>, Array2<f32>, Array2<f32>)> {
    arcsinh_stretch_rgb_with_stats(hip, r, g, b, None, None, factor, 1.0)
}
/// arcsinh_stretch_composite_cmd (stretch.rs:94-124) from the loaded composite to the encoder's input; the command discards the planes, so none are written.
/// global_range: the cached statistics' fold (arcsinh_rgb_range), which skips the range pass
pub fn arcsinh_stretch_composite(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, factor: f64, global_range: Option<(f32, f32)>, max_dim: usize) -> Result<ArcsinhComposite> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let (mn, mx) = (global_range.map(|v| v.0), global_range.map(|v| v.1));
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_arcsinh_composite_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_arcsinh_stretch_composite(hip.ctx, &r.ab(), &g.ab(), &b.ab(), factor, opt_ptr(&mn), opt_ptr(&mx), max_dim as i64, std::ptr::null_mut(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    Ok(ArcsinhComposite {
        pixels,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        factor: info.factor,
        global_range: (info.global_min, info.global_max),
        degenerate: info.degenerate != 0,
    })
}
/// apply_arcsinh_stretch_cmd (stretch.rs:15-43) with render_and_save's preview as one device chain with one synchronisation
pub fn arcsinh_stretch_view(hip: &Hip, image: &impl PlaneSrc, factor: f64) -> Result<ArcsinhView> {
    let (rows, cols) = image.dims();
    let mut stretched = Array2::<f32>::zeros((rows, cols));
    let mut pixels = vec![0u8; rows * cols];
    let mut info: sys::ab_arcsinh_view_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_arcsinh_stretch_view(hip.ctx, &image.ab(), factor, &mut stretched.ab_mut(), pixels.as_mut_ptr(), 0, &mut info) })?;
    Ok(ArcsinhView {
        stretched,
        pixels,
        dims: (info.rows as usize, info.cols as usize),
        factor: info.factor,
        data_range: (info.data_min, info.data_max),
        degenerate: info.degenerate != 0,
        stats: stats_from_sys(&info.stats),
        stf: stf_from_sys(&info.stf),
    })
}
/// masked_stretch_composite_cmd (stretch.rs:135-221): masked_stretch_rgb_shared (shared_mask) or masked_stretch x 3, then the preview; the stretched
/// channels stay in a workspace of the context
pub fn masked_stretch_composite(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, config: &MaskedStretchConfig, shared_mask: bool, max_dim: usize) -> Result<MaskedStretchComposite> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_masked_stretch_composite_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_masked_stretch_composite(hip.ctx, &r.ab(), &g.ab(), &b.ab(), &masked_cfg(config), shared_mask as i32, max_dim as i64, std::ptr::null_mut(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    let ch = |c: &sys::ab_masked_stretch_result| MaskedChannelStats { iterations_run: c.iterations_run, final_background: c.final_background, converged: c.converged != 0 };
    Ok(MaskedStretchComposite {
        pixels,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        channels: [ch(&info.channels[0]), ch(&info.channels[1]), ch(&info.channels[2])],
        stars_masked: info.stars_masked as usize,
        mask_coverage: info.mask_coverage,
        mask_mode: if info.mask_mode == sys::AB_MASK_SHARED_LUMINANCE as i32 { "shared_luminance" } else { "per_channel" },
    })
}

// ---- the compose wizard's background step: cmd/processing/background.rs:17-94, cmd/common.rs:18-22, :152-193 ------------------------------------------------
/// what auto_stretch_preview + save_preview_png hand to save_stf_png (cmd/common.rs:190-193), with the statistics behind the stretch
pub struct MonoPreview {
    pub pixels: Vec<u8>,
    pub preview_dims: (usize, usize),
    pub stats: ImageStats,
    pub stf: StfParams,
}
/// what extract_background_cmd encodes, caches and reports (background.rs:51-92)
pub struct BackgroundStep {
    pub corrected_pixels: Vec<u8>,
    pub model_pixels: Vec<u8>,
    pub dims: (usize, usize),
    pub preview_dims: (usize, usize),
    pub sample_count: usize,
    pub rms_residual: f64,
    pub corrected_stats: ImageStats,
    pub model_stats: ImageStats,
    pub elapsed_ms: u64,
}
/// auto_stretch_preview (cmd/common.rs:18-22) followed by save_preview_png's pick (:190-193): only the picked pixels are stretched
pub fn auto_stretch_preview_sampled(hip: &Hip, image: &impl PlaneSrc, max_dim: usize) -> Result<MonoPreview> {
    let (rows, cols) = image.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let mut pixels = vec![0u8; ph * pw];
    let mut stats: sys::ab_image_stats = unsafe { std::mem::zeroed() };
    let mut stf: sys::ab_stf_params = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_auto_stretch_preview_sampled(hip.ctx, &image.ab(), std::ptr::null(), max_dim as i64, pixels.as_mut_ptr(), 0, &mut stats, &mut stf) })?;
    Ok(MonoPreview { pixels, preview_dims: (ph, pw), stats: stats_from_sys(&stats), stf: stf_from_sys(&stf) })
}
/// the clamps extract_background_cmd applies before it builds its BackgroundConfig (background.rs:44-47, types/constants.rs:11-16)
pub fn background_step_clamp_config(grid_size: usize, poly_degree: usize, iterations: usize) -> (usize, usize, usize) {
    (grid_size.clamp(3, 32), poly_degree.clamp(1, 5), iterations.clamp(1, 10))
}
/// extract_background_cmd (background.rs:17-94) from the loaded plane to the two encoders' inputs: extract_background, each plane's statistics once, both
/// previews in one launch; the model stays in a workspace of the context.  `corrected` (host array or DevicePlane of the image's dims) receives the plane the
/// command caches with corrected_stats.  config is taken as extract_background takes it (background_step_clamp_config)
pub fn background_step_into(hip: &Hip, image: &impl PlaneSrc, config: &BackgroundConfig, max_dim: usize, corrected: &mut impl PlaneDst,
                            progress: Option<&ProgressHandle>) -> Result<BackgroundStep> {
    let start = std::time::Instant::now();
    let (rows, cols) = image.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let (mut corrected_pixels, mut model_pixels) = (vec![0u8; ph * pw], vec![0u8; ph * pw]);
    let cfg = sys::ab_background_config { grid_size: config.grid_size, poly_degree: config.poly_degree, sigma_clip: config.sigma_clip, iterations: config.iterations, mode: config.mode as i32 };
    let mut info: sys::ab_background_step_info = unsafe { std::mem::zeroed() };
    let mut pc = corrected.ab_mut();
    hip.with_progress(progress, || {
        hip.check(unsafe {
            sys::ab_background_step(hip.ctx, &image.ab(), &cfg, max_dim as i64, &mut pc, std::ptr::null_mut(), corrected_pixels.as_mut_ptr(), model_pixels.as_mut_ptr(), 0, &mut info)
        })
    })?;
    if let Some(p) = progress {
        p.emit_complete(); // background.rs:105-107
    }
    Ok(BackgroundStep {
        corrected_pixels,
        model_pixels,
        dims: (info.rows as usize, info.cols as usize),
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        sample_count: info.bg.sample_count,
        rms_residual: info.bg.rms_residual,
        corrected_stats: stats_from_sys(&info.corrected_stats),
        model_stats: stats_from_sys(&info.model_stats),
        elapsed_ms: start.elapsed().as_millis() as u64,
    })
}
/// the same with the corrected plane on the host
pub fn background_step(hip: &Hip, image: &impl PlaneSrc, config: &BackgroundConfig, max_dim: usize, progress: Option<&ProgressHandle>) -> Result<(Array2<f32>, BackgroundStep)> {
    let (rows, cols) = image.dims();
    let mut corrected = Array2::<f32>::zeros((rows, cols));
    let step = background_step_into(hip, image, config, max_dim, &mut corrected, progress)?;
    Ok((corrected, step))
}

// ---- a17  core/compose/rgb.rs, white_balance.rs, lrgb.rs, core/imaging/resample.rs ---------------------------------------------------------------------
/// drop-in for resample_image (resample.rs:25-61)
pub fn resample_image(hip: &Hip, image: &impl PlaneSrc, target_rows: usize, target_cols: usize) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros((target_rows, target_cols));
    hip.check(unsafe { sys::ab_resample_image(hip.ctx, &image.ab(), &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for select_wb_reference (white_balance.rs:3-20)
pub fn select_wb_reference(sr: &ImageStats, sg: &ImageStats, sb: &ImageStats) -> (f64, f64, f64) {
    let mut m = [1.0f64; 3];
    unsafe { sys::ab_select_wb_reference(&stats_to_sys(sr), &stats_to_sys(sg), &stats_to_sys(sb), m.as_mut_ptr()) };
    (m[0], m[1], m[2])
}
fn rgb_compose_cfg(config: &RgbComposeConfig) -> sys::ab_rgb_compose_config {
    let mut cfg: sys::ab_rgb_compose_config = unsafe { std::mem::zeroed() };
    match config.white_balance {
        WhiteBalance::Auto => cfg.white_balance = 0,
        WhiteBalance::Manual(x, y, z) => {
            cfg.white_balance = 1;
            cfg.wb_manual = [x, y, z];
        }
        WhiteBalance::None => cfg.white_balance = 2,
    }
    cfg.auto_stretch = config.auto_stretch as i32;
    cfg.linked_stf = config.linked_stf as i32;
    for (i, s) in [&config.stf_r, &config.stf_g, &config.stf_b].iter().enumerate() {
        if let Some(p) = s {
            cfg.has_stf[i] = 1;
            cfg.stf[i] = stf_to_sys(p);
        }
    }
    cfg.align = config.align as i32;
    cfg.align_method = matches!(config.align_method, AlignMethod::Affine) as i32;
    if let Some(s) = config.scnr.as_ref() {
        cfg.has_scnr = 1;
        cfg.scnr = scnr_to_sys(s);
    }
    cfg.num_threads = num_threads();
    cfg
}
/// drop-in for process_rgb (rgb.rs:209-323)
pub fn process_rgb(hip: &Hip, r: Option<&Array2<f32>>, g: Option<&Array2<f32>>, b: Option<&Array2<f32>>, config: &RgbComposeConfig) -> Result<ProcessedRgb> {
    let count = [r, g, b].iter().filter(|c| c.is_some()).count();
    if count < 2 {
        bail!("Need at least 2 channels for RGB compose (got {})", count); // rgb.rs:217
    }
    let rows = [r, g, b].iter().flatten().map(|a| a.nrows()).max().unwrap();
    let cols = [r, g, b].iter().flatten().map(|a| a.ncols()).max().unwrap();
    let (pr, pg, pb) = (opt_plane(r), opt_plane(g), opt_plane(b));
    let cfg = rgb_compose_cfg(config);
    let z = || Array2::<f32>::zeros((rows, cols));
    let (mut or, mut og, mut ob, mut qr, mut qg, mut qb) = (z(), z(), z(), z(), z(), z());
    let mut info: sys::ab_processed_rgb_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_process_rgb(hip.ctx, opt_ptr(&pr), opt_ptr(&pg), opt_ptr(&pb), &cfg, &mut or.ab_mut(), &mut og.ab_mut(), &mut ob.ab_mut(), &mut qr.ab_mut(), &mut qg.ab_mut(), &mut qb.ab_mut(), &mut info)
    })?;
    let cs = |i: usize| ChannelStats { min: info.chan_stats[i][0], max: info.chan_stats[i][1], median: info.chan_stats[i][2], mean: info.chan_stats[i][3] };
    let dims = |a: Option<&Array2<f32>>| a.map(|x| [x.nrows(), x.ncols()]);
    Ok(ProcessedRgb {
        r: or,
        g: og,
        b: ob,
        rows: info.rows as usize,
        cols: info.cols as usize,
        stf_r: stf_from_sys(&info.stf[0]),
        stf_g: stf_from_sys(&info.stf[1]),
        stf_b: stf_from_sys(&info.stf[2]),
        stats_r: cs(0),
        stats_g: cs(1),
        stats_b: cs(2),
        offset_g: (info.offset_g[0], info.offset_g[1]),
        offset_b: (info.offset_b[0], info.offset_b[1]),
        scnr_applied: info.scnr_applied != 0,
        dimension_info: (info.resampled != 0).then(|| DimensionHarmonize { original_r: dims(r), original_g: dims(g), original_b: dims(b), target: [rows, cols], resampled: true }),
        pre_stretch_r: Some(qr),
        pre_stretch_g: Some(qg),
        pre_stretch_b: Some(qb),
        stats_wb_r: Some(stats_from_sys(&info.stats_wb[0])),
        stats_wb_g: Some(stats_from_sys(&info.stats_wb[1])),
        stats_wb_b: Some(stats_from_sys(&info.stats_wb[2])),
    })
}
/// what compose_rgb_cmd encodes, caches and reports (cmd/compose/rgb.rs:106-116, :153-203)
pub struct ComposedRgb {
    pub pixels: Vec<u8>,
    pub preview_dims: (usize, usize),
    /// the white-balanced, aligned, pre-stretch planes: __composite_* / __composite_orig_*, with stats_wb
    pub pre_stretch: [Array2<f32>; 3],
    pub stats_wb: [ImageStats; 3],
    pub rows: usize,
    pub cols: usize,
    pub stf: [StfParams; 3],
    pub stats: [ChannelStats; 3],
    pub offset_g: (f64, f64),
    pub offset_b: (f64, f64),
    pub scnr_applied: bool,
    pub resampled: bool,
    pub lrgb_applied: bool,
    pub elapsed_ms: u64,
}
/// compose_rgb_cmd (cmd/compose/rgb.rs:43-205) from its loaded entries to the encoder's input as one chain: process_rgb, the L branch (resample_image,
/// stf::analyze, auto_stf, apply_stf_f32, apply_lrgb) and render_rgb_preview; above max_dim only the picked pixels are finished
pub fn compose_rgb(hip: &Hip, l: Option<&Array2<f32>>, r: Option<&Array2<f32>>, g: Option<&Array2<f32>>, b: Option<&Array2<f32>>, config: &RgbComposeConfig,
                   lrgb_lightness: f32, lrgb_chrominance: f32, max_dim: usize) -> Result<ComposedRgb> {
    let start = std::time::Instant::now();
    let count = [r, g, b].iter().filter(|c| c.is_some()).count();
    if count < 2 {
        bail!("Need at least 2 channels for RGB compose (got {})", count); // rgb.rs:217
    }
    let rows = [r, g, b].iter().flatten().map(|a| a.nrows()).max().unwrap();
    let cols = [r, g, b].iter().flatten().map(|a| a.ncols()).max().unwrap();
    let (pl, pr, pg, pb) = (opt_plane(l), opt_plane(r), opt_plane(g), opt_plane(b));
    let cfg = rgb_compose_cfg(config);
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let mut pre = planes3(rows, cols);
    let mut pp = [pre[0].ab_mut(), pre[1].ab_mut(), pre[2].ab_mut()];
    let mut pixels = vec![0u8; ph * pw * 3];
    let mut info: sys::ab_compose_rgb_info = unsafe { std::mem::zeroed() };
    hip.check(unsafe {
        sys::ab_compose_rgb(hip.ctx, opt_ptr(&pl), opt_ptr(&pr), opt_ptr(&pg), opt_ptr(&pb), &cfg, lrgb_lightness, lrgb_chrominance, max_dim as i64, pp.as_mut_ptr(),
                            std::ptr::null_mut(), pixels.as_mut_ptr(), 0, &mut info)
    })?;
    let cs = |i: usize| ChannelStats { min: info.rgb.chan_stats[i][0], max: info.rgb.chan_stats[i][1], median: info.rgb.chan_stats[i][2], mean: info.rgb.chan_stats[i][3] };
    Ok(ComposedRgb {
        pixels,
        preview_dims: (info.preview_rows as usize, info.preview_cols as usize),
        pre_stretch: pre,
        stats_wb: [stats_from_sys(&info.rgb.stats_wb[0]), stats_from_sys(&info.rgb.stats_wb[1]), stats_from_sys(&info.rgb.stats_wb[2])],
        rows: info.rgb.rows as usize,
        cols: info.rgb.cols as usize,
        stf: [stf_from_sys(&info.rgb.stf[0]), stf_from_sys(&info.rgb.stf[1]), stf_from_sys(&info.rgb.stf[2])],
        stats: [cs(0), cs(1), cs(2)],
        offset_g: (info.rgb.offset_g[0], info.rgb.offset_g[1]),
        offset_b: (info.rgb.offset_b[0], info.rgb.offset_b[1]),
        scnr_applied: info.rgb.scnr_applied != 0,
        resampled: info.rgb.resampled != 0,
        lrgb_applied: info.lrgb_applied != 0,
        elapsed_ms: start.elapsed().as_millis() as u64,
    })
}
/// restretch_composite_cmd (cmd/compose/rgb.rs:208-241) on the tone editor's kernel: three explicit STFs normalised with the cached statistics, SCNR whenever a
/// config is present (apply_scnr_inplace's own threshold decides), the preview's pick and pack -> preview_dims.0 x preview_dims.1 x 3 bytes.
/// update_composite_channel_cmd (:255-293) beside it is resample_image + compute_image_stats
pub fn restretch_composite(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, stats: &[ImageStats; 3], stf: &[StfParams; 3], scnr: Option<&ScnrConfig>,
                           max_dim: usize) -> Result<Vec<u8>> {
    let (rows, cols) = r.dims();
    let (ph, pw) = preview_dims(rows, cols, max_dim);
    let s = [stats_to_sys(&stats[0]), stats_to_sys(&stats[1]), stats_to_sys(&stats[2])];
    let p = [stf_to_sys(&stf[0]), stf_to_sys(&stf[1]), stf_to_sys(&stf[2])];
    let sc = scnr.map(scnr_to_sys);
    let mut pixels = vec![0u8; ph * pw * 3];
    hip.check(unsafe {
        sys::ab_restretch_composite(hip.ctx, &r.ab(), &g.ab(), &b.ab(), s.as_ptr(), p.as_ptr(), sc.is_some() as i32, sc.as_ref().map_or(std::ptr::null(), |c| c as *const _),
                                    max_dim as i64, std::ptr::null_mut(), pixels.as_mut_ptr(), 0)
    })?;
    Ok(pixels)
}
/// drop-in for apply_lrgb (lrgb.rs:4-45)
pub fn apply_lrgb(hip: &Hip, l: &impl PlaneSrc, r: &mut impl PlaneDst, g: &mut impl PlaneDst, b: &mut impl PlaneDst, lightness_weight: f32, chrominance_weight: f32) -> Result<()> {
    hip.check(unsafe { sys::ab_apply_lrgb(hip.ctx, &l.ab(), &mut r.ab_mut(), &mut g.ab_mut(), &mut b.ab_mut(), lightness_weight, chrominance_weight) })
}
/// drop-in for synthesize_luminance (lrgb.rs:47-64)
pub fn synthesize_luminance(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc) -> Result<Array2<f32>> {
    let mut out = Array2::<f32>::zeros(r.dims());
    hip.check(unsafe { sys::ab_synthesize_luminance(hip.ctx, &r.ab(), &g.ab(), &b.ab(), &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for helpers::compute_linked_stf_with_stats (cmd/helpers.rs:185-202)
pub fn compute_linked_stf_with_stats(sr: &ImageStats, sg: &ImageStats, sb: &ImageStats, config: &AutoStfConfig) -> (StfParams, ImageStats) {
    let cfg = sys::ab_auto_stf_config { target_bg: config.target_bg, shadow_k: config.shadow_k };
    let mut p = sys::ab_stf_params { shadow: 0.0, midtone: 0.5, highlight: 1.0 };
    let mut c: sys::ab_image_stats = unsafe { std::mem::zeroed() };
    unsafe { sys::ab_compute_linked_stf(&stats_to_sys(sr), &stats_to_sys(sg), &stats_to_sys(sb), &cfg, &mut p, &mut c) };
    (stf_from_sys(&p), stats_from_sys(&c))
}
/// drop-in for calibrate_channel (cmd/compose/color.rs:21-49): the scaled plane and its statistics
pub fn calibrate_channel(hip: &Hip, orig: &impl PlaneSrc, factor: f32, orig_stats: &ImageStats) -> Result<(Array2<f32>, ImageStats)> {
    let mut out = Array2::<f32>::zeros(orig.dims());
    let st = calibrate_channel_into(hip, orig, factor, orig_stats, &mut out)?;
    Ok((out, st))
}
pub fn calibrate_channel_into(hip: &Hip, orig: &impl PlaneSrc, factor: f32, orig_stats: &ImageStats, out: &mut impl PlaneDst) -> Result<ImageStats> {
    let mut st: sys::ab_image_stats = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_calibrate_channel(hip.ctx, &orig.ab(), factor, &stats_to_sys(orig_stats), &mut out.ab_mut(), &mut st) })?;
    Ok(stats_from_sys(&st))
}

// ---- the compose wizard's crop step, cmd/compose/crop.rs -----------------------------------------------------------------------------------------------------
fn box_to_sys(b: (usize, usize, usize, usize)) -> sys::ab_crop_box {
    sys::ab_crop_box { top: b.0 as u64, bottom: b.1 as u64, left: b.2 as u64, right: b.3 as u64 }
}
fn box_from_sys(b: &sys::ab_crop_box) -> (usize, usize, usize, usize) {
    (b.top as usize, b.bottom as usize, b.left as usize, b.right as usize)
}
/// crop_array's clamp (crop.rs:65-69): the dims of the plane it returns
fn cropped_dims(b: &sys::ab_crop_box, (rows, cols): (usize, usize)) -> (usize, usize) {
    let (t, l) = ((b.top as usize).min(rows), (b.left as usize).min(cols));
    ((b.bottom as usize).min(rows).max(t) - t, (b.right as usize).min(cols).max(l) - l)
}
/// drop-in for detect_valid_region (crop.rs:14-62): (top, bottom, left, right); only the four bounds cross to the host
pub fn detect_valid_region(hip: &Hip, arr: &impl PlaneSrc, threshold: f32) -> Result<(usize, usize, usize, usize)> {
    let mut b = box_to_sys((0, 0, 0, 0));
    hip.check(unsafe { sys::ab_detect_valid_region(hip.ctx, &arr.ab(), threshold, &mut b) })?;
    Ok(box_from_sys(&b))
}
/// the loop crop.rs:109-116 over planes of any dims in one launch chain: every plane's box and the running
/// (max top, min bottom, max left, min right)
pub fn detect_valid_regions<P: PlaneSrc>(hip: &Hip, arrs: &[P], threshold: f32) -> Result<(Vec<(usize, usize, usize, usize)>, (usize, usize, usize, usize))> {
    let planes: Vec<_> = arrs.iter().map(|a| a.ab()).collect();
    let mut each = vec![box_to_sys((0, 0, 0, 0)); planes.len()];
    let mut common = box_to_sys((0, 0, 0, 0));
    hip.check(unsafe { sys::ab_detect_valid_regions(hip.ctx, planes.as_ptr(), planes.len(), threshold, each.as_mut_ptr(), &mut common) })?;
    Ok((each.iter().map(box_from_sys).collect(), box_from_sys(&common)))
}
/// drop-in for crop_array (crop.rs:64-71) on a host array
pub fn crop_array(hip: &Hip, arr: &impl PlaneSrc, top: usize, bottom: usize, left: usize, right: usize) -> Result<Array2<f32>> {
    let b = box_to_sys((top, bottom, left, right));
    let mut out = Array2::<f32>::zeros(cropped_dims(&b, arr.dims()));
    hip.check(unsafe { sys::ab_crop_array(hip.ctx, &arr.ab(), &b, &mut out.ab_mut()) })?;
    Ok(out)
}
/// the same from HBM to HBM (asynchronous on the context's stream)
pub fn crop_array_device(hip: &Hip, arr: &DevicePlane, top: usize, bottom: usize, left: usize, right: usize) -> Result<DevicePlane> {
    let b = box_to_sys((top, bottom, left, right));
    let (rows, cols) = cropped_dims(&b, arr.dims());
    let mut out = DevicePlane::alloc(rows, cols)?;
    hip.check(unsafe { sys::ab_crop_array(hip.ctx, &arr.ab(), &b, &mut out.ab_mut()) })?;
    Ok(out)
}
/// What crop_channels_cmd's JSON needs besides its paths and keys (crop.rs:185-195): `dimensions` = [out_cols, out_rows].
pub struct CropChannels<P> {
    pub cropped: Vec<P>,
    pub stats: Vec<ImageStats>,
    pub dimensions: [usize; 2],
    pub crop_top: usize,
    pub crop_bottom: usize,
    pub crop_left: usize,
    pub crop_right: usize,
    pub auto_detected: bool,
}
fn crop_plan(hip: &Hip, planes: &[sys::ab_plane], top: usize, bottom: usize, left: usize, right: usize, auto_detect: Option<bool>) -> Result<(sys::ab_crop_plan, Vec<u64>)> {
    let mut cfg: sys::ab_crop_config = unsafe { std::mem::zeroed() };
    unsafe { sys::ab_crop_config_default(&mut cfg) }; // AUTO_THRESHOLD (:12)
    cfg.auto_detect = auto_detect.unwrap_or(true) as i32; // :101
    (cfg.top, cfg.bottom, cfg.left, cfg.right) = (top as u64, bottom as u64, left as u64, right as u64);
    let mut plan: sys::ab_crop_plan = unsafe { std::mem::zeroed() };
    let mut dims = vec![0u64; 2 * planes.len()];
    hip.check(unsafe { sys::ab_crop_channels_plan(hip.ctx, planes.as_ptr(), planes.len(), &cfg, &mut plan, dims.as_mut_ptr()) })?;
    Ok((plan, dims))
}
fn crop_result<P>(plan: &sys::ab_crop_plan, cropped: Vec<P>, stats: &[sys::ab_image_stats]) -> CropChannels<P> {
    CropChannels {
        cropped,
        stats: stats.iter().map(stats_from_sys).collect(),
        dimensions: [plan.out_cols as usize, plan.out_rows as usize],
        crop_top: plan.actual_top as usize,
        crop_bottom: plan.actual_bottom as usize,
        crop_left: plan.actual_left as usize,
        crop_right: plan.actual_right as usize,
        auto_detected: plan.auto_detected != 0,
    }
}
/// drop-in for the pixel work of crop_channels_cmd (crop.rs:92-183) on host arrays: the box (auto or manual margins), every plane
/// cropped, compute_image_stats of each; Err "No paths provided for cropping" / "Auto-crop found no valid overlapping region"
pub fn crop_channels<P: PlaneSrc>(hip: &Hip, arrs: &[P], top: usize, bottom: usize, left: usize, right: usize, auto_detect: Option<bool>) -> Result<CropChannels<Array2<f32>>> {
    let planes: Vec<_> = arrs.iter().map(|a| a.ab()).collect();
    let (plan, dims) = crop_plan(hip, &planes, top, bottom, left, right, auto_detect)?;
    let mut cropped: Vec<_> = dims.chunks(2).map(|d| Array2::<f32>::zeros((d[0] as usize, d[1] as usize))).collect();
    let mut outs: Vec<_> = cropped.iter_mut().map(|c| c.ab_mut()).collect();
    let mut stats: Vec<sys::ab_image_stats> = vec![unsafe { std::mem::zeroed() }; planes.len()];
    hip.check(unsafe { sys::ab_crop_channels(hip.ctx, planes.as_ptr(), planes.len(), &plan, outs.as_mut_ptr(), stats.as_mut_ptr()) })?;
    Ok(crop_result(&plan, cropped, &stats))
}
/// the same between planes that stay in HBM (align_channels_cmd's outputs in, blend_channels_cmd's inputs out): one detection
/// chain, one crop launch, the statistics; nothing but the boxes and the statistics crosses to the host
pub fn crop_channels_device(hip: &Hip, arrs: &[&DevicePlane], top: usize, bottom: usize, left: usize, right: usize, auto_detect: Option<bool>) -> Result<CropChannels<DevicePlane>> {
    let planes: Vec<_> = arrs.iter().map(|a| a.ab()).collect();
    let (plan, dims) = crop_plan(hip, &planes, top, bottom, left, right, auto_detect)?;
    let mut cropped = dims.chunks(2).map(|d| DevicePlane::alloc(d[0] as usize, d[1] as usize)).collect::<Result<Vec<_>>>()?;
    let mut outs: Vec<_> = cropped.iter_mut().map(|c| c.ab_mut()).collect();
    let mut stats: Vec<sys::ab_image_stats> = vec![unsafe { std::mem::zeroed() }; planes.len()];
    hip.check(unsafe { sys::ab_crop_channels(hip.ctx, planes.as_ptr(), planes.len(), &plan, outs.as_mut_ptr(), stats.as_mut_ptr()) })?;
    Ok(crop_result(&plan, cropped, &stats))
}

// ---- a18  core/astrometry/spcc.rs ---------------------------------------------------------------------------------------------------------------------------
fn spcc_cfg(config: &SpccConfig) -> sys::ab_spcc_config {
    let (kind, custom) = match config.white_reference {
        WhiteReference::AverageSpiral => (0, [0.0; 3]),
        WhiteReference::G2V => (1, [0.0; 3]),
        WhiteReference::Photopic => (2, [0.0; 3]),
        WhiteReference::Custom(r, g, b) => (3, [r, g, b]),
    };
    sys::ab_spcc_config { min_snr: config.min_snr, max_stars: config.max_stars as u64, saturation_limit: config.saturation_limit, white_reference: kind, custom }
}
fn white_ref_name(w: &WhiteReference) -> String {
    // spcc.rs:157-162
    match w {
        WhiteReference::AverageSpiral => "Average Spiral Galaxy".into(),
        WhiteReference::G2V => "G2V (Sun-like)".into(),
        WhiteReference::Photopic => "Photopic".into(),
        WhiteReference::Custom(..) => "Custom".into(),
    }
}
/// drop-in for spcc_calibrate_rgb with the built-in Bp-Rp catalogue (spcc.rs:73-183).  The header enters that path only
/// through its WCS's pixel scale (include/astroburst_hip.h, a18).
pub fn spcc_calibrate_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, header: &crate::types::header::HduHeader, config: &SpccConfig) -> Result<SpccResult, String> {
    let wcs = crate::core::astrometry::wcs::WcsTransform::from_header(header).map_err(|e| format!("WCS not available: {}. Run Plate Solve first.", e))?; // spcc.rs:80-81
    let mut res: sys::ab_spcc_result = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_spcc_calibrate_rgb(hip.ctx, &r.ab(), &g.ab(), &b.ab(), wcs.pixel_scale_arcsec(), &spcc_cfg(config), &mut res) }).map_err(|e| e.to_string())?;
    Ok(spcc_result(&res, config))
}
/// the part of spcc_calibrate_rgb after detection (spcc.rs:90-183) on a detection the caller already has
pub fn spcc_from_detection(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, detection: &DetectionResult, lum_max: f64, pixel_scale_arcsec: f64, config: &SpccConfig) -> Result<SpccResult, String> {
    let stars: Vec<_> = detection.stars.iter().map(star_to_sys).collect();
    let mut res: sys::ab_spcc_result = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_spcc_from_detection(hip.ctx, &r.ab(), &g.ab(), &b.ab(), stars.as_ptr(), stars.len(), lum_max, pixel_scale_arcsec, &spcc_cfg(config), &mut res) })
        .map_err(|e| e.to_string())?;
    Ok(spcc_result(&res, config))
}
fn spcc_result(res: &sys::ab_spcc_result, config: &SpccConfig) -> SpccResult {
    SpccResult {
        r_factor: res.r_factor,
        g_factor: res.g_factor,
        b_factor: res.b_factor,
        stars_matched: res.stars_matched as usize,
        stars_total: res.stars_total as usize,
        avg_color_index: res.avg_color_index,
        white_ref_name: white_ref_name(&config.white_reference),
        catalog_name: "Built-in Bp-Rp (synthetic)".into(), // spcc.rs:164-166
        is_synthetic_catalog: true,
    }
}
/// white_reference_rgb (spcc.rs:245-255)
pub fn white_reference_rgb(w: &WhiteReference) -> (f64, f64, f64) {
    let c = spcc_cfg(&SpccConfig { white_reference: w.clone(), ..SpccConfig::default() });
    let mut out = [1.0f64; 3];
    unsafe { sys::ab_spcc_white_reference_rgb(c.white_reference, c.custom.as_ptr(), out.as_mut_ptr()) };
    (out[0], out[1], out[2])
}

// ---- f1  infra/fits/reader.rs, writer.rs ---------------------------------------------------------------------------------------------------------------------------
/// decode_pixels (reader.rs:41-110): a FITS data unit (big-endian, any BITPIX) -> f32 plane, host or device bytes
pub fn fits_decode_pixels(hip: &Hip, data: &[u8], bitpix: i64, bscale: f64, bzero: f64, out: &mut impl PlaneDst) -> Result<()> {
    hip.check(unsafe { sys::ab_fits_decode_pixels(hip.ctx, data.as_ptr() as *const c_void, data.len(), 0, bitpix, bscale, bzero, &mut out.ab_mut()) })
}
/// compute_bzero_bscale (writer.rs:150-186)
pub fn fits_compute_bzero_bscale(hip: &Hip, image: &impl PlaneSrc) -> Result<(f64, f64)> {
    let (mut bzero, mut bscale) = (0.0, 1.0);
    hip.check(unsafe { sys::ab_fits_compute_bzero_bscale(hip.ctx, &image.ab(), &mut bzero, &mut bscale) })?;
    Ok((bzero, bscale))
}
/// the pixel encoder of write_fits_mono (writer.rs:188-240): f32 plane -> big-endian data unit bytes
pub fn fits_encode_pixels(hip: &Hip, image: &impl PlaneSrc, bitpix: i32, bzero: f64, bscale: f64) -> Result<Vec<u8>> {
    let (r, c) = image.dims();
    let mut out = vec![0u8; r * c * (bitpix.unsigned_abs() as usize / 8)];
    hip.check(unsafe { sys::ab_fits_encode_pixels(hip.ctx, &image.ab(), bitpix, bzero, bscale, out.as_mut_ptr() as *mut c_void, 0) })?;
    Ok(out)
}

// ---- f2  core/imaging/calibration_pipeline.rs ----------------------------------------------------------------------------------------------------------------------------
fn batch_cfg(c: &BatchStackConfig) -> sys::ab_batch_stack_config {
    sys::ab_batch_stack_config { sigma_low: c.sigma_low, sigma_high: c.sigma_high, max_iterations: c.max_iterations as u64, normalize_before_stack: c.normalize_before_stack as i32 }
}
struct Masters {
    planes: [Option<sys::ab_plane>; 3],
}
impl Masters {
    fn new(m: &CalibrationMasters) -> Self {
        Self { planes: [opt_plane(m.bias.as_ref()), opt_plane(m.dark.as_ref()), opt_plane(m.flat.as_ref())] }
    }
    fn sys(&self) -> sys::ab_calibration_masters {
        sys::ab_calibration_masters { bias: opt_ptr(&self.planes[0]), dark: opt_ptr(&self.planes[1]), flat: opt_ptr(&self.planes[2]) }
    }
}
/// drop-in for calibrate_light (calibration_pipeline.rs:74-118)
pub fn calibrate_light(hip: &Hip, light: &impl PlaneSrc, masters: &CalibrationMasters) -> Result<Array2<f32>> {
    let m = Masters::new(masters);
    let mut out = Array2::<f32>::zeros(light.dims());
    hip.check(unsafe { sys::ab_calibrate_light(hip.ctx, &light.ab(), &m.sys(), &mut out.ab_mut()) })?;
    Ok(out)
}
/// drop-in for normalize_frames (calibration_pipeline.rs:309-319)
pub fn normalize_frames(hip: &Hip, frames: &[Array2<f32>]) -> Result<Vec<Array2<f32>>> {
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let mut outs: Vec<Array2<f32>> = frames.iter().map(|f| Array2::zeros(f.dim())).collect();
    let mut po: Vec<_> = outs.iter_mut().map(|o| o.ab_mut()).collect();
    hip.check(unsafe { sys::ab_normalize_frames(hip.ctx, planes.as_ptr(), planes.len(), po.as_mut_ptr()) })?;
    Ok(outs)
}
/// drop-in for sigma_clipped_mean_stack (calibration_pipeline.rs:321-378): (master, per-frame rejection counts)
pub fn sigma_clipped_mean_stack(hip: &Hip, frames: &[Array2<f32>], config: &BatchStackConfig) -> Result<(Array2<f32>, Vec<usize>)> {
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let mut out = Array2::<f32>::zeros(frames.first().map_or((0, 0), |f| f.dim()));
    let mut rej = vec![0u64; frames.len()];
    hip.check(unsafe { sys::ab_sigma_clipped_mean_stack(hip.ctx, planes.as_ptr(), planes.len(), &batch_cfg(config), &mut out.ab_mut(), rej.as_mut_ptr()) })?;
    Ok((out, rej.into_iter().map(|x| x as usize).collect()))
}
/// one channel of run_batch_pipeline (calibration_pipeline.rs:157-190), fused: no calibrated or normalised frame is written
pub fn run_batch_channel(hip: &Hip, lights: &[Array2<f32>], masters: &CalibrationMasters, config: &BatchStackConfig, label: &str) -> Result<(Array2<f32>, BatchChannelStats)> {
    let planes: Vec<_> = lights.iter().map(|f| f.ab()).collect();
    let m = Masters::new(masters);
    let mut out = Array2::<f32>::zeros(lights.first().map_or((0, 0), |f| f.dim()));
    let mut rej = vec![0u64; lights.len()];
    let mut st: sys::ab_batch_channel_stats = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_run_batch_channel(hip.ctx, planes.as_ptr(), planes.len(), &m.sys(), &batch_cfg(config), &mut out.ab_mut(), rej.as_mut_ptr(), &mut st) })?;
    Ok((out, BatchChannelStats { label: label.to_string(), lights_input: st.lights_input as usize, lights_after_rejection: rej.into_iter().map(|x| x as usize).collect(), mean: st.mean, stddev: st.stddev }))
}
/// compose_rgb_from_masters (calibration_pipeline.rs:201-267)
pub fn compose_rgb_from_masters(hip: &Hip, r: &Array2<f32>, g: &Array2<f32>, b: &Array2<f32>, l: Option<&Array2<f32>>) -> Result<Array3<f32>> {
    let lp = opt_plane(l);
    let (mut rows, mut cols) = (0i64, 0i64);
    hip.check(unsafe { sys::ab_compose_rgb_from_masters(hip.ctx, &r.ab(), &g.ab(), &b.ab(), opt_ptr(&lp), std::ptr::null_mut(), 0, &mut rows, &mut cols) })?;
    let mut out = Array3::<f32>::zeros((rows as usize, cols as usize, 3));
    hip.check(unsafe { sys::ab_compose_rgb_from_masters(hip.ctx, &r.ab(), &g.ab(), &b.ab(), opt_ptr(&lp), out.as_mut_ptr(), 0, &mut rows, &mut cols) })?;
    Ok(out)
}
/// drop-in for run_batch_pipeline (calibration_pipeline.rs:120-199)
pub fn run_batch_pipeline(hip: &Hip, channels: Vec<ChannelInput>, masters: &CalibrationMasters, config: &BatchPipelineConfig) -> Result<BatchPipelineResult, String> {
    if channels.is_empty() {
        return Err("No channels provided".into()); // :125-127
    }
    let labels: Vec<CString> = channels.iter().map(|c| CString::new(c.label.as_str()).unwrap_or_default()).collect();
    let planes: Vec<Vec<sys::ab_plane>> = channels.iter().map(|c| c.lights.iter().map(|l| l.ab()).collect()).collect();
    let mut rej: Vec<Vec<u64>> = channels.iter().map(|c| vec![0u64; c.lights.len()]).collect();
    let inputs: Vec<sys::ab_batch_channel_input> = (0..channels.len())
        .map(|i| sys::ab_batch_channel_input { label: labels[i].as_ptr(), lights: planes[i].as_ptr(), n_lights: planes[i].len(), rejection_counts: rej[i].as_mut_ptr() })
        .collect();
    let m = Masters::new(masters);
    let mut outs: Vec<Array2<f32>> = channels.iter().map(|c| Array2::zeros(c.lights.first().map_or((0, 0), |l| l.dim()))).collect();
    let mut po: Vec<_> = outs.iter_mut().map(|o| o.ab_mut()).collect();
    let mut stats: Vec<sys::ab_batch_channel_stats> = vec![unsafe { std::mem::zeroed() }; channels.len()];
    let rmin = outs.iter().map(|o| o.nrows()).min().unwrap();
    let cmin = outs.iter().map(|o| o.ncols()).min().unwrap();
    let mut rgb = vec![0f32; rmin * cmin * 3];
    let (mut rr, mut rc) = (0i64, 0i64);
    hip.check(unsafe { sys::ab_run_batch_pipeline(hip.ctx, inputs.as_ptr(), inputs.len(), &m.sys(), &batch_cfg(&config.stack), po.as_mut_ptr(), stats.as_mut_ptr(), rgb.as_mut_ptr(), 0, &mut rr, &mut rc) })
        .map_err(|e| e.to_string())?;
    let rgb = (rr > 0).then(|| {
        rgb.truncate(rr as usize * rc as usize * 3);
        Array3::from_shape_vec((rr as usize, rc as usize, 3), rgb).unwrap()
    });
    let chan_stats = (0..channels.len())
        .map(|i| BatchChannelStats {
            label: channels[i].label.clone(),
            lights_input: stats[i].lights_input as usize,
            lights_after_rejection: rej[i].iter().map(|&x| x as usize).collect(),
            mean: stats[i].mean,
            stddev: stats[i].stddev,
        })
        .collect();
    Ok(BatchPipelineResult {
        master_channels: channels.iter().map(|c| c.label.clone()).zip(outs).collect(),
        rgb,
        stats: BatchPipelineStats {
            darks_combined: masters.dark.is_some() as usize, // :192-194
            flats_combined: masters.flat.is_some() as usize,
            bias_combined: masters.bias.is_some() as usize,
            channels: chan_stats,
        },
    })
}

// ---- f3  core/analysis/subframe.rs ----------------------------------------------------------------------------------------------------------------------------------------
fn subframe_cfg(c: &SubframeWeightConfig) -> sys::ab_subframe_weight_config {
    sys::ab_subframe_weight_config {
        fwhm_weight: c.fwhm_weight,
        eccentricity_weight: c.eccentricity_weight,
        snr_weight: c.snr_weight,
        noise_weight: c.noise_weight,
        max_fwhm: c.max_fwhm,
        max_eccentricity: c.max_eccentricity,
        min_snr: c.min_snr,
        min_stars: c.min_stars as u64,
    }
}
fn subframe_metrics(m: &sys::ab_subframe_metrics, file_path: &str) -> SubframeMetrics {
    SubframeMetrics {
        file_path: file_path.to_string(),
        file_name: file_path.split(&['/', '\\'][..]).last().unwrap_or(file_path).to_string(), // subframe.rs:56-60
        star_count: m.star_count as usize,
        median_fwhm: m.median_fwhm,
        median_eccentricity: m.median_eccentricity,
        median_snr: m.median_snr,
        background_median: m.background_median,
        background_sigma: m.background_sigma,
        noise_ratio: m.noise_ratio,
        weight: m.weight,
        accepted: m.accepted != 0,
    }
}
/// drop-in for analyze_subframe (subframe.rs:51-136)
pub fn analyze_subframe(hip: &Hip, image: &impl PlaneSrc, file_path: &str, config: &SubframeWeightConfig) -> Result<SubframeMetrics> {
    let mut m: sys::ab_subframe_metrics = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_analyze_subframe(hip.ctx, &image.ab(), &subframe_cfg(config), &mut m) })?;
    Ok(subframe_metrics(&m, file_path))
}
/// analyze_subframe over a batch + normalize_weights (subframe.rs:138-159), the body of analyze_subframes_cmd
pub fn analyze_subframes<P: PlaneSrc>(hip: &Hip, images: &[P], file_paths: &[String], config: &SubframeWeightConfig) -> Result<Vec<SubframeMetrics>> {
    let planes: Vec<_> = images.iter().map(|i| i.ab()).collect();
    let mut ms: Vec<sys::ab_subframe_metrics> = vec![unsafe { std::mem::zeroed() }; images.len()];
    hip.check(unsafe { sys::ab_analyze_subframes(hip.ctx, planes.as_ptr(), planes.len(), &subframe_cfg(config), ms.as_mut_ptr()) })?;
    unsafe { sys::ab_normalize_subframe_weights(ms.as_mut_ptr(), ms.len()) };
    Ok(ms.iter().zip(file_paths).map(|(m, p)| subframe_metrics(m, p)).collect())
}

// ---- the weighted, normalised stack: the consumer of the subframe scores (no counterpart in the reference: combine.rs:14-92 ends in an unweighted mean) ----
/// one frame of `stack_weighted_into`: ab_stack_frame_param, field for field
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct StackFrameParam {
    /// >= 0; a frame of weight 0 takes part in nothing
    pub weight: f64,
    pub scale: f32,
    pub offset: f32,
}
// (the wrappers hand a `*const StackFrameParam` to the library as a `*const sys::ab_stack_frame_param`: same size, alignment and offsets)
const _: () = {
    assert!(std::mem::size_of::<StackFrameParam>() == std::mem::size_of::<sys::ab_stack_frame_param>());
    assert!(std::mem::align_of::<StackFrameParam>() == std::mem::align_of::<sys::ab_stack_frame_param>());
    assert!(std::mem::offset_of!(StackFrameParam, weight) == std::mem::offset_of!(sys::ab_stack_frame_param, weight));
    assert!(std::mem::offset_of!(StackFrameParam, scale) == std::mem::offset_of!(sys::ab_stack_frame_param, scale));
    assert!(std::mem::offset_of!(StackFrameParam, offset) == std::mem::offset_of!(sys::ab_stack_frame_param, offset));
};
/// how `stack_params_from_metrics` brings the frames' backgrounds to the best frame's (ab_stack_norm)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum StackNormalize {
    None = 0,
    Additive = 1,
    Multiplicative = 2,
}
/// the weights of the accepted subframes and the offsets / scales that normalise them; -> (one parameter per frame, index of the reference
/// frame).  Host arithmetic only.
pub fn stack_params_from_metrics(metrics: &[SubframeMetrics], normalize: StackNormalize) -> Result<(Vec<StackFrameParam>, usize)> {
    let ms: Vec<sys::ab_subframe_metrics> = metrics
        .iter()
        .map(|m| sys::ab_subframe_metrics {
            star_count: m.star_count as u64,
            median_fwhm: m.median_fwhm,
            median_eccentricity: m.median_eccentricity,
            median_snr: m.median_snr,
            background_median: m.background_median,
            background_sigma: m.background_sigma,
            noise_ratio: m.noise_ratio,
            weight: m.weight,
            accepted: m.accepted as i32,
        })
        .collect();
    let mut out = vec![StackFrameParam { weight: 0.0, scale: 1.0, offset: 0.0 }; metrics.len()];
    let mut reference = 0usize;
    let rc = unsafe { sys::ab_stack_params_from_metrics(ms.as_ptr(), ms.len(), normalize as i32, out.as_mut_ptr() as *mut sys::ab_stack_frame_param, &mut reference) };
    if rc != 0 {
        bail!("No accepted subframe of positive weight to stack, or the best frame's background cannot be normalised to");
    }
    Ok((out, reference))
}
/// every frame normalised (p * scale + offset), sigma_clip_combine's rejection on the normalised samples, the survivors' mean weighted
/// per frame; at most 64 frames of weight > 0.  `out_weight`: the per-pixel sum of the surviving weights.  Returns the rejected count.
pub fn stack_weighted_into<P: PlaneSrc, D: PlaneDst>(hip: &Hip, frames: &[P], params: &[StackFrameParam], config: &StackConfig, out: &mut D, out_weight: Option<&mut D>) -> Result<u64> {
    if frames.len() != params.len() {
        bail!("{} parameters for {} frames", params.len(), frames.len());
    }
    let planes: Vec<_> = frames.iter().map(|f| f.ab()).collect();
    let mut rejected = 0u64;
    let mut pw = out_weight.map(|w| w.ab_mut());
    let pw_ptr = pw.as_mut().map_or(std::ptr::null_mut(), |p| p as *mut sys::ab_plane_mut);
    hip.check(unsafe {
        sys::ab_stack_weighted(hip.ctx, planes.as_ptr(), params.as_ptr() as *const sys::ab_stack_frame_param, planes.len(), &stack_cfg(config), &mut out.ab_mut(), pw_ptr, &mut rejected)
    })?;
    Ok(rejected)
}

// ---- f4  cmd/helpers.rs render_rgb_preview, infra/ipc.rs, infra/tiles.rs -----------------------------------------------------------------------------------------------------
/// preview dims of render_rgb_preview (cmd/helpers.rs:204-230)
pub fn preview_dims(rows: usize, cols: usize, max_dim: usize) -> (usize, usize) {
    let (mut r, mut c) = (0i64, 0i64);
    unsafe { sys::ab_preview_dims(rows as i64, cols as i64, max_dim as i64, &mut r, &mut c) };
    (r as usize, c as usize)
}
/// the pixel half of render_rgb_preview(_with_stf): box-downsampled interleaved RGB u8, `stf`/`stats` = None for planes already in [0, 1]
pub fn render_rgb_preview(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, max_dim: usize, stf: Option<(&[StfParams; 3], &[ImageStats; 3])>) -> Result<(Vec<u8>, usize, usize)> {
    let (rows, cols) = r.dims();
    let (pr, pc) = preview_dims(rows, cols, max_dim);
    let mut out = vec![0u8; pr * pc * 3];
    let (p, s): (Vec<_>, Vec<_>) = stf.map_or((vec![], vec![]), |(p, s)| (p.iter().map(stf_to_sys).collect(), s.iter().map(stats_to_sys).collect()));
    let (pp, sp) = if p.is_empty() { (std::ptr::null(), std::ptr::null()) } else { (p.as_ptr(), s.as_ptr()) };
    hip.check(unsafe { sys::ab_render_rgb_preview(hip.ctx, &r.ab(), &g.ab(), &b.ab(), max_dim as i64, pp, sp, out.as_mut_ptr(), 0) })?;
    Ok((out, pr, pc))
}
/// infra/ipc.rs encode_with_header: the f32 preview payload the frontend reads
pub fn ipc_encode_with_header(hip: &Hip, image: &impl PlaneSrc, max_dim: usize) -> Result<Vec<u8>> {
    let (rows, cols) = image.dims();
    let (pr, pc) = preview_dims(rows, cols, max_dim);
    let mut out = vec![0u8; 64 + pr * pc * 4];
    let mut len = 0usize;
    hip.check(unsafe { sys::ab_ipc_encode_with_header(hip.ctx, &image.ab(), max_dim as i64, out.as_mut_ptr() as *mut c_void, 0, &mut len) })?;
    out.truncate(len);
    Ok(out)
}
/// compute_num_levels (tiles.rs:137-147)
pub fn tile_compute_num_levels(width: usize, height: usize, tile_size: usize) -> usize {
    unsafe { sys::ab_tile_compute_num_levels(width as i64, height as i64, tile_size as i64) as usize }
}
/// downsample_2x (tiles.rs:41-70)
pub fn tile_downsample_2x(hip: &Hip, image: &impl PlaneSrc) -> Result<Array2<f32>> {
    let (r, c) = image.dims();
    let mut out = Array2::<f32>::zeros(((r + 1) / 2, (c + 1) / 2));
    hip.check(unsafe { sys::ab_tile_downsample_2x(hip.ctx, &image.ab(), &mut out.ab_mut()) })?;
    Ok(out)
}
/// percentile bounds of the tile normalisation (tiles.rs:72-100)
pub fn tile_percentile_bounds(hip: &Hip, image: &impl PlaneSrc, low_pct: f64, high_pct: f64) -> Result<(f32, f32)> {
    let (mut lo, mut hi) = (0f32, 1f32);
    hip.check(unsafe { sys::ab_tile_percentile_bounds(hip.ctx, &image.ab(), low_pct, high_pct, &mut lo, &mut hi) })?;
    Ok((lo, hi))
}
pub struct TilePyramid {
    pub levels: Vec<sys::ab_tile_level>,
    pub tiles: Vec<u8>,
    pub global_min: f32,
    pub global_max: f32,
}
fn pyramid_layout(rows: usize, cols: usize, tile_size: usize, channels: i32) -> (Vec<sys::ab_tile_level>, i32, usize) {
    let mut levels: Vec<sys::ab_tile_level> = vec![unsafe { std::mem::zeroed() }; 32];
    let (mut n, mut bytes) = (0i32, 0usize);
    unsafe { sys::ab_tile_pyramid_layout(rows as i64, cols as i64, tile_size as i64, channels, levels.as_mut_ptr(), &mut n, &mut bytes) };
    (levels, n, bytes)
}
/// generate_tile_pyramid (tiles.rs:149-230): every level's u8 tiles in one buffer + the level table
pub fn generate_tile_pyramid(hip: &Hip, normalized: &impl PlaneSrc, tile_size: usize) -> Result<TilePyramid> {
    let (rows, cols) = normalized.dims();
    let (mut levels, mut n, bytes) = pyramid_layout(rows, cols, tile_size, 1);
    let mut tiles = vec![0u8; bytes];
    let (mut gmin, mut gmax) = (0f32, 1f32);
    hip.check(unsafe { sys::ab_generate_tile_pyramid(hip.ctx, &normalized.ab(), tile_size as i64, tiles.as_mut_ptr(), 0, levels.as_mut_ptr(), &mut n, &mut gmin, &mut gmax) })?;
    levels.truncate(n as usize);
    Ok(TilePyramid { levels, tiles, global_min: gmin, global_max: gmax })
}
/// the RGB pyramid of the composite viewer (tiles.rs:232-300)
pub fn generate_tile_pyramid_rgb(hip: &Hip, r: &impl PlaneSrc, g: &impl PlaneSrc, b: &impl PlaneSrc, tile_size: usize, stf: &[StfParams; 3], stats: &[ImageStats; 3]) -> Result<TilePyramid> {
    let (rows, cols) = r.dims();
    let (mut levels, mut n, bytes) = pyramid_layout(rows, cols, tile_size, 3);
    let mut tiles = vec![0u8; bytes];
    let p: Vec<_> = stf.iter().map(stf_to_sys).collect();
    let s: Vec<_> = stats.iter().map(stats_to_sys).collect();
    hip.check(unsafe { sys::ab_generate_tile_pyramid_rgb(hip.ctx, &r.ab(), &g.ab(), &b.ab(), tile_size as i64, p.as_ptr(), s.as_ptr(), tiles.as_mut_ptr(), 0, levels.as_mut_ptr(), &mut n) })?;
    levels.truncate(n as usize);
    Ok(TilePyramid { levels, tiles, global_min: 0.0, global_max: 1.0 })
}

// ---- several GPUs of one node (include/astroburst_hip.h section (e)) -----------------------------------------------------------
pub struct Comm(pub *mut sys::ab_comm);
unsafe impl Send for Comm {}
impl Comm {
    pub fn rank(&self) -> i32 {
        unsafe { sys::ab_comm_rank(self.0) }
    }
    pub fn size(&self) -> i32 {
        unsafe { sys::ab_comm_size(self.0) }
    }
    pub fn is_host_transport(&self) -> bool {
        unsafe { sys::ab_comm_is_host(self.0) != 0 }
    }
    pub fn collectives_issued(&self) -> u64 {
        unsafe { sys::ab_comm_collectives_issued(self.0) }
    }
    /// every later collective on this communicator fails with AB_ERR_COMM instead of waiting for a rank that is gone
    pub fn abort(&self) {
        unsafe { sys::ab_comm_abort(self.0) };
    }
    pub fn set_timeout_ms(&self, ms: i64) {
        unsafe { sys::ab_comm_set_timeout_ms(self.0, ms) };
    }
    /// one process per GPU (the RCCL transport): rank 0 makes the id and hands it to the others out of band
    pub fn unique_id() -> Result<[u8; sys::AB_COMM_ID_BYTES]> {
        let mut id = [0u8; sys::AB_COMM_ID_BYTES];
        match unsafe { sys::ab_comm_get_unique_id(id.as_mut_ptr()) } {
            sys::AB_OK => Ok(id),
            rc => bail!("ab_comm_get_unique_id failed ({rc})"),
        }
    }
    pub fn init_rank(hip: &Hip, id: &[u8; sys::AB_COMM_ID_BYTES], nranks: i32, rank: i32) -> Result<Self> {
        let mut c = std::ptr::null_mut();
        hip.check(unsafe { sys::ab_comm_init_rank(hip.ctx, id.as_ptr(), nranks, rank, &mut c) })?;
        Ok(Self(c))
    }
    /// host-staged transport (a POSIX shared-memory segment `name`): several ranks on ONE GPU, or a node without xGMI
    pub fn init_rank_host(hip: &Hip, name: &str, nranks: i32, rank: i32) -> Result<Self> {
        let n = CString::new(name)?;
        let mut c = std::ptr::null_mut();
        hip.check(unsafe { sys::ab_comm_init_rank_host(hip.ctx, n.as_ptr(), nranks, rank, &mut c) })?;
        Ok(Self(c))
    }
    /// agree on a status before a data collective: every rank returns the same Ok / Err (a failed rank fails all, none hangs)
    pub fn agree(&self, hip: &Hip, local_ok: bool) -> Result<()> {
        hip.check(unsafe { sys::ab_comm_agree(hip.ctx, self.0, if local_ok { sys::AB_OK } else { sys::AB_ERR_INVALID }) })
    }
    pub fn allreduce_f64_sum(&self, hip: &Hip, buf_dev: *mut f64, count: usize) -> Result<()> {
        hip.check(unsafe { sys::ab_comm_allreduce(hip.ctx, self.0, buf_dev as *mut c_void, count, sys::AB_DT_F64, sys::AB_RED_SUM) })
    }
    pub fn allgather(&self, hip: &Hip, send_dev: *const c_void, recv_dev: *mut c_void, bytes_per_rank: usize) -> Result<()> {
        hip.check(unsafe { sys::ab_comm_allgather(hip.ctx, self.0, send_dev, recv_dev, bytes_per_rank) })
    }
    pub fn broadcast(&self, hip: &Hip, buf_dev: *mut c_void, bytes: usize, root: i32) -> Result<()> {
        hip.check(unsafe { sys::ab_comm_broadcast(hip.ctx, self.0, buf_dev, bytes, root) })
    }
    /// several collectives as one RCCL group (no-ops on the host transport)
    pub fn group<T>(f: impl FnOnce() -> Result<T>) -> Result<T> {
        unsafe { sys::ab_comm_group_start() };
        let r = f();
        unsafe { sys::ab_comm_group_end() };
        r
    }
}
impl Drop for Comm {
    fn drop(&mut self) {
        unsafe { sys::ab_comm_destroy(self.0) }
    }
}
/// rows [row0, row0 + nrows) of a `rows`-row image that belong to `rank`
pub fn shard_rows(rows: usize, nranks: i32, rank: i32) -> Result<(usize, usize)> {
    let (mut r0, mut n) = (0i64, 0i64);
    let rc = unsafe { sys::ab_shard_rows(rows as i64, nranks, rank, &mut r0, &mut n) };
    if rc != 0 {
        bail!("shard_rows: invalid arguments (status {rc}: {rows} rows, rank {rank} of {nranks})");
    }
    Ok((r0 as usize, n as usize))
}
/// what `rank` must hold of every target frame to warp its band with `transforms`: its rows + the halo (first row, count)
pub fn shard_source_rows(transforms: &[AffineTransform], src_rows: usize, src_cols: usize, out_rows: usize, out_cols: usize, nranks: i32, rank: i32) -> Result<(usize, usize)> {
    let flat: Vec<f64> = transforms.iter().flat_map(|t| [t.a, t.b, t.tx, t.c, t.d, t.ty]).collect();
    let (mut s0, mut sn) = (0i64, 0i64);
    let rc = unsafe {
        sys::ab_shard_source_rows(flat.as_ptr(), transforms.len(), src_rows as i64, src_cols as i64, out_rows as i64, out_cols as i64, nranks, rank, &mut s0, &mut sn)
    };
    if rc != 0 {
        // (AB_ERR_INVALID from ab_shard_rows or the dimension checks: an empty band would only fail later, in ab_warp_image_rows_from_band)
        bail!("shard_source_rows: invalid arguments (status {rc}: src {src_rows}x{src_cols}, out {out_rows}x{out_cols}, rank {rank} of {nranks})");
    }
    Ok((s0 as usize, sn as usize))
}
/// frames [f0, f0 + nf) of an n-frame stack that belong to `rank`
pub fn shard_frames(n_frames: usize, nranks: i32, rank: i32) -> Result<(usize, usize)> {
    let (mut f0, mut nf) = (0usize, 0usize);
    let rc = unsafe { sys::ab_shard_frames(n_frames, nranks, rank, &mut f0, &mut nf) };
    if rc != 0 {
        bail!("shard_frames: invalid arguments (status {rc}: {n_frames} frames, rank {rank} of {nranks})");
    }
    Ok((f0, nf))
}

/// One context + one RCCL rank per GPU, each driven by its own thread (what `handleStackAll`'s concurrent commands already
/// are on the host side).  `f(rank, hip, comm)` runs on every rank; the sharded entry points inside enqueue their collectives
/// on the rank's stream.
pub fn on_all_gpus<T: Send>(devices: &[i32], f: impl Fn(usize, &Hip, &Comm) -> Result<T> + Sync) -> Result<Vec<T>> {
    let hips: Vec<Hip> = devices.iter().map(|&d| Hip::new(d)).collect::<Result<_>>()?;
    let ctxs: Vec<*mut sys::ab_ctx> = hips.iter().map(|h| h.ctx).collect();
    let mut raw = vec![std::ptr::null_mut(); devices.len()];
    hips[0].check(unsafe { sys::ab_comm_init_all(ctxs.as_ptr(), ctxs.len() as i32, raw.as_mut_ptr()) })?;
    let comms: Vec<Comm> = raw.into_iter().map(Comm).collect(); // destroyed on drop, after the scope below has joined every rank
    let results = std::thread::scope(|s| {
        let handles: Vec<_> = hips
            .iter()
            .zip(comms.iter())
            .enumerate()
            .map(|(rank, (hip, comm))| {
                let f = &f;
                let comm = SendRef(comm);
                s.spawn(move || {
                    let c = comm; // the whole wrapper moves into the thread (edition-2021 closures capture fields otherwise)
                    f(rank, hip, c.0)
                })
            })
            .collect();
        handles.into_iter().map(|h| h.join().expect("rank thread")).collect::<Vec<_>>()
    });
    results.into_iter().collect()
}
struct SendRef<'a>(&'a Comm);
unsafe impl<'a> Send for SendRef<'a> {}

/// rows [row0, ..) of the per-pixel loop on this GPU alone (no communicator)
pub fn stack_sigma_clip_rows(hip: &Hip, planes_dev: &[DevicePlane], config: &StackConfig, row0: usize, out_band: &mut DevicePlane) -> Result<u64> {
    let planes: Vec<_> = planes_dev.iter().map(|p| p.ab()).collect();
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_sigma_clip_rows(hip.ctx, planes.as_ptr(), planes.len(), &stack_cfg(config), row0 as i64, &mut out_band.ab_mut(), &mut rejected) })?;
    Ok(rejected)
}
/// stack_images over frames already resident on the GPUs, the per-pixel loop split by ROWS (exact: equals the single-GPU
/// and the reference result bit for bit).  `planes_dev` = this rank's device copies of all n frames.
pub fn stack_rowband(hip: &Hip, comm: &Comm, planes_dev: &[DevicePlane], config: &StackConfig, out_band: &mut DevicePlane) -> Result<u64> {
    let planes: Vec<_> = planes_dev.iter().map(|p| p.ab()).collect();
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_sigma_clip_rowband(hip.ctx, comm.0, planes.as_ptr(), planes.len(), &stack_cfg(config), &mut out_band.ab_mut(), &mut rejected) })?;
    Ok(rejected)
}
/// the frames sharded over the ranks: per-GPU partial + all-reduce(sum f64, count u32) + divide (the two-level estimator)
pub fn stack_sharded(hip: &Hip, comm: &Comm, local_planes: &[DevicePlane], config: &StackConfig, out: &mut DevicePlane) -> Result<u64> {
    let planes: Vec<_> = local_planes.iter().map(|p| p.ab()).collect();
    let mut rejected = 0u64;
    hip.check(unsafe { sys::ab_stack_sigma_clip_sharded(hip.ctx, comm.0, planes.as_ptr(), planes.len(), &stack_cfg(config), &mut out.ab_mut(), &mut rejected) })?;
    Ok(rejected)
}
/// (partial stacks' span on the context's stream, time inside the all-reduces + divisions on the comm stream) of the last `stack_sharded`, ms
pub fn stack_sharded_last_ms(hip: &Hip) -> Result<(f32, f32)> {
    let (mut stack_ms, mut comm_ms) = (0f32, 0f32);
    hip.check(unsafe { sys::ab_stack_sharded_last_ms(hip.ctx, &mut stack_ms, &mut comm_ms) })?;
    Ok((stack_ms, comm_ms))
}
pub fn allgather_rows(hip: &Hip, comm: &Comm, band: &DevicePlane, full: &mut DevicePlane) -> Result<()> {
    hip.check(unsafe { sys::ab_allgather_rows(hip.ctx, comm.0, &band.ab(), &mut full.ab_mut()) })
}
/// register_frames with the targets spread over the ranks and the 80-byte results exchanged
pub fn register_frames_sharded(hip: &Hip, comm: &Comm, reference: &DevicePlane, targets: &[DevicePlane]) -> Result<Vec<AffineAlignResult>> {
    let planes: Vec<_> = targets.iter().map(|t| t.ab()).collect();
    let mut out: Vec<sys::ab_affine_align_result> = vec![unsafe { std::mem::zeroed() }; targets.len()];
    hip.check(unsafe { sys::ab_register_frames_sharded(hip.ctx, comm.0, &reference.ab(), planes.as_ptr(), planes.len(), num_threads(), out.as_mut_ptr()) })?;
    Ok(out.iter().map(align_from_sys).collect())
}
/// the row-band scheme's registration as one call: this rank's rows `[row0, row0 + bands[i].rows)` of every registered frame.  `targets[i]` holds
/// rows `[target_row0[i], ..)` of target i -- whole for the targets this rank estimates (i mod size == rank); own frames are warped as they are
/// fitted, the estimates are exchanged, the other frames are warped from their bands
pub fn align_pairs_affine_rowband(hip: &Hip, comm: &Comm, reference: &DevicePlane, targets: &[DevicePlane], target_row0: &[usize], row0: usize,
                                  bands: &mut [DevicePlane]) -> Result<Vec<AffineAlignResult>> {
    if targets.len() != target_row0.len() || targets.len() != bands.len() {
        bail!("align_pairs_affine_rowband: {} targets, {} first rows, {} bands", targets.len(), target_row0.len(), bands.len());
    }
    let planes: Vec<_> = targets.iter().map(|t| t.ab()).collect();
    let first: Vec<i64> = target_row0.iter().map(|&r| r as i64).collect();
    let mut outs: Vec<_> = bands.iter_mut().map(|b| b.ab_mut()).collect();
    let mut out: Vec<sys::ab_affine_align_result> = vec![unsafe { std::mem::zeroed() }; targets.len()];
    hip.check(unsafe {
        sys::ab_align_pairs_affine_rowband(hip.ctx, comm.0, &reference.ab(), planes.as_ptr(), first.as_ptr(), planes.len(), num_threads(), row0 as i64,
                                           out.as_mut_ptr(), outs.as_mut_ptr())
    })?;
    Ok(out.iter().map(align_from_sys).collect())
}
/// compute_image_stats of an image of which this rank holds a row band (histograms all-reduced in stream)
pub fn compute_image_stats_sharded(hip: &Hip, comm: &Comm, band: &DevicePlane, total_rows: usize) -> Result<ImageStats> {
    let mut st: sys::ab_image_stats = unsafe { std::mem::zeroed() };
    hip.check(unsafe { sys::ab_compute_image_stats_sharded(hip.ctx, comm.0, &band.ab(), total_rows as i64, &mut st) })?;
    Ok(stats_from_sys(&st))
}
