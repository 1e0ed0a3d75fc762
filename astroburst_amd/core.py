"""Host-side mirror of the reference's `core::*` functions for the hot path, over the C ABI.

Names, argument meaning and error behaviour follow the reference (src-tauri/src/core/...), so the
parity tests read like the reference's own unit tests.  Planes may be numpy arrays (host: staged
through HBM by the library) or torch CUDA tensors (device: used in place on torch's current
stream).  Every function here ends in a HIP kernel of libastroburst_hip.so; nothing is computed
in Python or on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import AstroBurstError, AutoStfConfigC, ImageStatsC, Plane, StackConfig, StfParamsC

try:  # torch is plumbing only (device memory, streams, torch.distributed)
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class ImageStats:  # types/image.rs:2-10
    min: float = 0.0
    max: float = 0.0
    median: float = 0.0
    mad: float = 0.0
    sigma: float = 0.0
    mean: float = 0.0
    valid_count: int = 0


@dataclass
class StfParams:  # types/image.rs:36-50
    shadow: float = 0.0
    midtone: float = 0.5
    highlight: float = 1.0


WHITE_REFERENCES = {"average_spiral": 0, "g2v": 1, "photopic": 2}


@dataclass
class SpccResult:  # spcc.rs:45-56
    r_factor: float
    g_factor: float
    b_factor: float
    stars_matched: int
    stars_total: int
    avg_color_index: float
    white_ref_name: str
    catalog_name: str = "Built-in Bp-Rp"
    is_synthetic_catalog: bool = True


@dataclass
class ProcessedRgb:  # rgb.rs:18-40
    r: object
    g: object
    b: object
    rows: int
    cols: int
    stf: tuple            # (StfParams r, g, b)
    channel_stats: tuple  # 3 x (min, max, median, mean) before white balance
    offset_g: tuple
    offset_b: tuple
    scnr_applied: bool
    resampled: bool
    pre_stretch: tuple    # (r, g, b) white-balanced, pre-STF planes (or Nones)
    stats_wb: tuple       # 3 x ImageStats after white balance


@dataclass
class StarMaskResult:  # star_mask.rs:32-37
    mask: object
    stars_masked: int
    coverage_fraction: float


@dataclass
class MaskedStretchResult:  # masked_stretch.rs:34-42
    image: object
    iterations_run: int
    final_background: float
    stars_masked: int
    mask_coverage: float
    converged: bool


@dataclass
class BackgroundResult:  # background.rs:35-42
    model: object
    corrected: object
    sample_count: int
    rms_residual: float
    coeffs: np.ndarray


@dataclass
class StackResult:  # types/stacking.rs:22-28
    image: object
    frame_count: int
    rejected_pixels: int
    offsets: list


@dataclass
class DrizzleResult:  # types/stacking.rs DrizzleResult (drizzle.rs:335-344)
    image: object
    weight_map: object
    frame_count: int
    output_scale: float
    input_dims: tuple
    output_dims: tuple
    offsets: list  # (dx, dy) per frame
    rejected_pixels: int


@dataclass
class PsfStar:  # StarCandidate (psf_estimation.rs:4-14)
    x: float
    y: float
    peak: float
    flux: float
    fwhm: float
    ellipticity: float
    distance_from_center: float
    snr: float


@dataclass
class PsfResult:  # psf_estimation.rs:41-50 (kernel: the (2 r + 1)^2 f32 plane psf_to_kernel yields) + the two counts
    kernel: object
    kernel_size: int
    average_fwhm: float
    average_ellipticity: float
    stars_used: list
    stars_rejected: int
    spread_pixels: float
    stars_detected: int
    stars_filtered: int


@dataclass
class FftResult:  # core/analysis/fft.rs:11-17
    spectrum: object
    display_rows: int
    display_cols: int
    original_size: int
    windowed: bool


@dataclass
class GlobalCubeStats:  # core/cube/eager.rs:160-166
    median: float
    sigma: float
    low: float
    high: float


CUBE_VALID_NONZERO, CUBE_VALID_ABOVE_PADDING = 0, 1  # ab_cube_valid_rule: the eager path's rule, the lazy path's


@dataclass
class AsinhStats:  # what asinh_normalize_simd takes from the valid pixels (math/simd.rs:163-180)
    median: float
    sigma: float
    low: float
    high: float
    valid_count: int


ASINH_ROUTE_AVX2, ASINH_ROUTE_SCALAR = 0, 1  # ab_asinh_route: the reference's AVX2 route (+ its scalar remainder), its scalar loop


RGB_PACK_8, RGB_PACK_8_ROUND, RGB_PACK_16BE = 0, 1, 2  # ab_rgb_pack: render_rgb's truncation, drizzle_rgb's rounding, render_rgb_16bit's big-endian pairs


def rgb_packed_bytes(rows: int, cols: int, pack: int = RGB_PACK_8) -> int:
    """The size of an interleaved RGB buffer: rows * cols * 3, twice that for RGB_PACK_16BE.  Host-only."""
    n = C.c_size_t(0)
    rc = _lib.lib().ab_rgb_packed_bytes(int(rows), int(cols), int(pack), C.byref(n))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, f"rgb_packed_bytes: bad dims {rows} x {cols} or packer {pack}")
    return int(n.value)


@dataclass
class RgbExportInfo:  # what stretch_and_render derived on its way (cmd/export/mod.rs:357-409)
    rows: int
    cols: int
    resampled: bool
    stats: tuple  # 3 x ImageStats
    stf: tuple    # 3 x StfParams


@dataclass
class ProcessedDrizzleRgb:  # drizzle_rgb.rs:24-39 (+ the bytes of :232-248 and the statistics the stretch used)
    stretched: tuple   # (r, g, b) or None
    wb: tuple          # (r_wb, g_wb, b_wb) or None
    rgb8: object       # uint8 (rows, cols, 3) or None
    rows: int
    cols: int
    wb_factors: tuple
    stf: tuple         # 3 x StfParams
    chan_stats: tuple  # 3 x (min, max, median, mean) before white balance
    stats_wb: tuple    # 3 x ImageStats
    scnr_applied: bool


@dataclass
class DrizzleRgbResult:  # types/compose.rs DrizzleRgbResult without its paths
    processed: ProcessedDrizzleRgb
    channels: tuple    # 3 x (frame_count, output_scale, in_dims, out_dims, rejected_pixels), None for a channel that is not there


@dataclass
class ToneInfo:  # what apply_tone_composite_cmd decided and reports (cmd/processing/curves.rs:163-189)
    stf: tuple             # 3 x StfParams: what was applied (RES_STF)
    norm: tuple            # 3 x ImageStats: what each channel was normalised with (the combined ones x 3 when linked)
    levels_applied: bool
    curves_applied: bool
    scnr_applied: bool
    rows: int              # 0 from tone_plan, which sees no plane
    cols: int
    preview_rows: int
    preview_cols: int


@dataclass
class ToneResult:
    planes: tuple          # (r, g, b) toned f32 planes of full size, or None
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    info: ToneInfo


def _tone_config(stf, linked_stf, levels, curves, scnr, keep):
    """ab_tone_config of apply_tone_composite_cmd's arguments (cmd/processing/curves.rs:58-71).  stf: None or three of (None |
    StfParams | (shadow, midtone, highlight)); levels: None or three of (None | (black, gamma, white)); curves: None or three of
    (None | a list of (x, y), which may be empty: Some(points)); scnr: None or dict(method=, amount=, preserve_luminance=).  The
    point arrays the configuration points at are appended to `keep`."""
    cfg = _lib.ToneConfigC()
    _lib.lib().ab_tone_config_default(C.byref(cfg))
    for c, p in enumerate(stf or ()):
        if p is not None:
            cfg.has_stf[c] = 1
            cfg.stf[c] = StfParamsC(*(p if isinstance(p, (tuple, list)) else (p.shadow, p.midtone, p.highlight)))
    cfg.linked_stf = int(bool(linked_stf))
    for c, p in enumerate(levels or ()):
        if p is not None:
            cfg.levels[c] = _lib.LevelsParamsC(*[float(v) for v in p])
    for c, pts in enumerate(curves or ()):
        if pts is not None:
            n = len(pts)
            xy = (C.c_double * max(2 * n, 2))(*[float(v) for p in pts for v in p])   # (Some([]) is a pointer all the same)
            keep.append(xy)
            cfg.curve_xy[c] = C.cast(xy, C.POINTER(C.c_double))
            cfg.n_curve[c] = n
    if scnr is not None:
        cfg.has_scnr = 1
        m = scnr.get("method", "average")
        cfg.scnr = _lib.ScnrConfigC(0 if m in ("average", "AverageNeutral", 0) else 1, scnr.get("amount", 1.0),
                                    int(bool(scnr.get("preserve_luminance", False))))
    return cfg


def _tone_info(info) -> ToneInfo:
    return ToneInfo(tuple(StfParams(p.shadow, p.midtone, p.highlight) for p in info.stf),
                    tuple(ImageStats(s.min, s.max, s.median, s.mad, s.sigma, s.mean, int(s.valid_count)) for s in info.norm),
                    bool(info.levels_applied), bool(info.curves_applied), bool(info.scnr_applied), int(info.rows), int(info.cols),
                    int(info.preview_rows), int(info.preview_cols))


def tone_plan(stats, stf=None, linked_stf=False, levels=None, curves=None, scnr=None, want_luts=True):
    """The decisions of apply_tone_composite_cmd (cmd/processing/curves.rs:86-154) without its pixels -> (ToneInfo, the three LUTs it
    would apply as float32 (3, 4096), or None when no curve runs).  Host-only."""
    keep = []
    cfg = _tone_config(stf, linked_stf, levels, curves, scnr, keep)
    st = (_lib.ImageStatsC * 3)(*[ImageStatsC(s.min, s.max, s.median, s.mad, s.sigma, s.mean, s.valid_count) for s in stats])
    info = _lib.ToneInfoC()
    luts = np.zeros((3, 4096), np.float32) if want_luts else None
    rc = _lib.lib().ab_tone_plan(st, C.byref(cfg), C.byref(info), luts.ctypes.data_as(C.POINTER(C.c_float)) if want_luts else None)
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_tone_plan: bad arguments")
    return _tone_info(info), (luts if want_luts and info.curves_applied else None)


@dataclass
class FitsView:  # what process_fits / process_fits_full hand to the encoder and the JSON (cmd/io/mod.rs:105-172)
    u8: object             # uint8 (rows, cols): apply_stf's bytes
    bins: object           # uint32 (hist_len,): the display histogram, or None (hist_bins = 0)
    rows: int
    cols: int
    stats: object          # ImageStats, or None (fetch=False)
    stf: object            # StfParams, or None


@dataclass
class RgbFitsView:  # process_rgb_fits' (cmd/io/mod.rs:33-102)
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    bins: object           # uint32 (hist_len,): the display histogram of R, or None
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    stats: object          # 3 x ImageStats, or None (fetch=False)
    stf: object            # 3 x StfParams, or None


COLOR_STATS_EXACT_OR_FULL, COLOR_STATS_KNOWN_RANGE = _lib.AB_COLOR_STATS_EXACT_OR_FULL, _lib.AB_COLOR_STATS_KNOWN_RANGE


@dataclass
class ColorPlan:  # what calibrate_and_scnr_cmd decides (cmd/compose/color.rs:115-117, :138-159 with calibrate_channel, :21-49)
    factors: tuple         # 3 x the f32 factor applied, as Python floats
    scnr_applied: bool
    route: tuple           # 3 x COLOR_STATS_EXACT_OR_FULL | COLOR_STATS_KNOWN_RANGE
    known_min: tuple       # 3 x float (0.0 off the known-range route)
    known_max: tuple


@dataclass
class ColorStepResult:  # calibrate_and_scnr_cmd: what it caches, encodes and reports (color.rs:161-183)
    planes: tuple          # (r, g, b): __composite_r / _g / _b
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    factors: object        # 3 x float, or None (fetch=False)
    scnr_applied: object   # bool, or None
    route: object          # 3 x route, or None
    stats: object          # 3 x ImageStats, or None
    stf: object            # the linked StfParams, or None


@dataclass
class BlendCompositeResult:  # blend_channels_cmd's (cmd/compose/blend.rs:185-221)
    planes: tuple          # (r, g, b)
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    resampled: object      # bool, or None (fetch=False)
    stats: object          # 3 x ImageStats, or None
    stf: object            # the linked StfParams, or None


@dataclass
class AutoWb:  # compute_auto_wb_cmd's JSON (color.rs:214-222)
    factors: tuple         # (r, g, b)
    stability: tuple       # (stab_r, stab_g, stab_b)
    ref_channel: str       # "R" | "G" | "B"


def _stats3(stats):
    return (_lib.ImageStatsC * 3)(*[ImageStatsC(s.min, s.max, s.median, s.mad, s.sigma, s.mean, s.valid_count) for s in stats])


def _scnr_config(scnr):
    """(has_scnr, ab_scnr_config | None) of None or dict(method=, amount=, preserve_luminance=)"""
    if scnr is None:
        return 0, None
    m = scnr.get("method", "average")
    return 1, _lib.ScnrConfigC(0 if m in ("average", "AverageNeutral", 0) else 1, scnr.get("amount", 1.0), int(bool(scnr.get("preserve_luminance", False))))


def color_step_plan(n_pixels: int, orig_stats, factors, scnr=None) -> ColorPlan:
    """The decisions of calibrate_and_scnr_cmd (cmd/compose/color.rs:97-184) without its pixels: the f32 factors, whether SCNR runs and
    the statistics route of each channel's final plane.  Host-only."""
    has, cfg = _scnr_config(scnr)
    plan = _lib.ColorPlanC()
    f = (C.c_double * 3)(*[float(v) for v in factors])
    rc = _lib.lib().ab_color_step_plan(int(n_pixels), _stats3(orig_stats), f, has, C.byref(cfg) if cfg is not None else None, C.byref(plan))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_color_step_plan: bad arguments")
    return ColorPlan(tuple(float(v) for v in plan.factors), bool(plan.scnr_applied), tuple(int(v) for v in plan.route),
                     tuple(float(v) for v in plan.known_min), tuple(float(v) for v in plan.known_max))


def compute_auto_wb(sr, sg, sb) -> AutoWb:
    """compute_auto_wb_cmd (cmd/compose/color.rs:187-224) of the three channels' ImageStats.  Host-only."""
    st = _stats3((sr, sg, sb))
    out = _lib.AutoWbC()
    rc = _lib.lib().ab_compute_auto_wb(C.byref(st[0]), C.byref(st[1]), C.byref(st[2]), C.byref(out))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_compute_auto_wb: bad arguments")
    return AutoWb(tuple(float(v) for v in out.factors), tuple(float(v) for v in out.stability), "RGB"[out.ref_channel])


MASK_PER_CHANNEL, MASK_SHARED_LUMINANCE = _lib.AB_MASK_PER_CHANNEL, _lib.AB_MASK_SHARED_LUMINANCE


@dataclass
class ArcsinhCompositeResult:  # arcsinh_stretch_composite_cmd's (cmd/processing/stretch.rs:94-124)
    planes: object         # (r, g, b) stretched, or None (the command discards them)
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    factor: object         # the clamped f32 factor, or None (fetch=False)
    global_min: object     # float, or None
    global_max: object
    degenerate: object     # bool: the range is below 1e-10, planes and bytes are zeros; or None


@dataclass
class ArcsinhViewResult:  # apply_arcsinh_stretch_cmd's (stretch.rs:15-43) with render_and_save's preview (cmd/common.rs:209-240)
    plane: object          # the stretched plane: write_fits_mono's input
    u8: object             # uint8 (rows, cols), or None
    rows: int
    cols: int
    factor: object         # the clamped f32 factor, or None (fetch=False)
    data_min: object
    data_max: object
    degenerate: object
    stats: object          # ImageStats of the stretched plane, or None
    stf: object            # StfParams, or None


@dataclass
class MaskedStretchCompositeResult:  # masked_stretch_composite_cmd's (stretch.rs:135-221)
    planes: object         # (r, g, b) stretched, or None
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    channels: object       # 3 x MaskedStretchResult (image None), or None (fetch=False)
    stars_masked: object   # the shared mask's, or the sum of the three channels'
    mask_coverage: object  # the shared mask's, or the mean of the three
    mask_mode: object      # "shared_luminance" | "per_channel"


@dataclass
class BackgroundStepResult:  # extract_background_cmd's (cmd/processing/background.rs:17-94) outputs up to the PNG encoders
    corrected: object        # the corrected plane: what the command caches under wizard_bg_key
    model: object            # the model, or None (want_model=False)
    corrected_u8: object     # uint8 (preview_rows, preview_cols), or None
    model_u8: object
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    sample_count: object     # int, or None (fetch=False)
    rms_residual: object
    coeffs: object           # the fitted coefficients (21 f64)
    corrected_stats: object  # ImageStats the command caches with the plane, or None
    model_stats: object
    corrected_stf: object    # StfParams, or None
    model_stf: object


@dataclass
class ComposeRgbResult:  # compose_rgb_cmd's (cmd/compose/rgb.rs:43-205) outputs up to the PNG encoder
    pre_stretch: tuple     # (r, g, b) white-balanced, aligned, pre-stretch planes: what the command caches as __composite_*
    planes: object         # (r, g, b) final planes the command drops, or None (want_planes=False)
    rgb8: object           # uint8 (preview_rows, preview_cols, 3), or None
    rows: int
    cols: int
    preview_rows: int
    preview_cols: int
    stf: object            # (StfParams r, g, b), or None (fetch=False), like everything below
    channel_stats: object  # 3 x (min, max, median, mean) before white balance
    offset_g: object
    offset_b: object
    scnr_applied: object
    resampled: object
    stats_wb: object       # 3 x ImageStats after white balance: what the command caches with the planes
    lrgb_applied: object
    l_resampled: object
    l_stats: object        # ImageStats of the matched L, or None (no L, or auto_stretch off)
    l_stf: object


def arcsinh_rgb_range(sr, sg, sb) -> tuple:
    """(global_min, global_max) of arcsinh_stretch_rgb_with_stats (core/imaging/stretch.rs:72-78): the f32 fold of three channels'
    ImageStats.  Host-only."""
    out = (C.c_float * 2)()
    rc = _lib.lib().ab_arcsinh_rgb_range(_stats3((sr, sg, sb)), out)
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_arcsinh_rgb_range: bad arguments")
    return float(out[0]), float(out[1])


HISTOGRAM_BINS = 65536     # stats.rs:8: what compute_histogram_with_stats builds before the fold


def downsample_histogram(bins, target_bins: int) -> np.ndarray:
    """downsample_histogram (core/imaging/stats.rs:423-444), host only: saturating u32 sums of the source ranges the reference's
    f64 ratio picks -- the dropped last source bin of e.g. 65536 -> 49 included."""
    src = np.ascontiguousarray(bins, dtype=np.uint32)
    out = np.zeros(max(1, min(int(target_bins), src.size)), np.uint32)
    n = C.c_size_t(0)
    u32p = C.POINTER(C.c_uint32)
    rc = _lib.lib().ab_downsample_histogram(src.ctypes.data_as(u32p), src.size, int(target_bins), out.ctypes.data_as(u32p), C.byref(n))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_downsample_histogram: no source bins or target_bins == 0")
    return out[:n.value]


def histogram_bin_edges(dmin: float, dmax: float, bins: int) -> np.ndarray:
    """Histogram.bin_edges of build_histogram (stats.rs:379-387, :412-413), host only: bins + 1 doubles."""
    out = np.zeros(max(int(bins), 0) + 1, np.float64)
    rc = _lib.lib().ab_histogram_bin_edges(float(dmin), float(dmax), int(bins), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_histogram_bin_edges: bins == 0")
    return out


class CropBox(NamedTuple):  # detect_valid_region's tuple (cmd/compose/crop.rs:14-62): rows [top, bottom), columns [left, right)
    top: int
    bottom: int
    left: int
    right: int

    def clamped(self, rows: int, cols: int) -> "CropBox":
        """the window crop_array takes from a rows x cols plane (crop.rs:65-69)"""
        t = min(self.top, rows)
        l = min(self.left, cols)
        return CropBox(t, max(min(self.bottom, rows), t), l, max(min(self.right, cols), l))


CROP_AUTO_THRESHOLD = float(np.float32(1e-6))  # AUTO_THRESHOLD (crop.rs:12)


@dataclass
class CropPlan:  # what crop_channels_cmd decides and reports (crop.rs:103-126, :170-183)
    crop_box: CropBox
    out_rows: int          # plane 0's cropped dims ("dimensions" is [out_cols, out_rows])
    out_cols: int
    actual_top: int
    actual_bottom: int
    actual_left: int
    actual_right: int
    auto_detected: bool
    out_dims: tuple        # (rows, cols) of each plane's cropped output


def cube_streaming_step(depth: int) -> int:
    """The frame stride of compute_global_stats_streaming (core/cube/lazy.rs:334-335).  Host-only."""
    return int(_lib.lib().ab_cube_streaming_step(int(depth)))


DRIZZLE_KERNELS = {"square": 0, "gaussian": 1, "lanczos3": 2}
DRIZZLE_ALIGNMENT = {"phase_correlation": 0, "zncc": 1}


@dataclass
class DetectedStar:  # star_detection.rs:10-20
    x: float
    y: float
    flux: float
    fwhm: float
    eccentricity: float
    peak: float
    npix: int
    snr: float


@dataclass
class AffineAlignResult:  # affine.rs:82-89
    transform: tuple
    matched_stars: int
    inliers: int
    residual_px: float
    method: str


@dataclass
class BatchStackConfig:  # calibration_pipeline.rs:20-37
    sigma_low: float = 2.5
    sigma_high: float = 3.0
    max_iterations: int = 5
    normalize_before_stack: bool = True

    def _c(self):
        return _lib.BatchStackConfigC(self.sigma_low, self.sigma_high, self.max_iterations, int(self.normalize_before_stack))


@dataclass
class BatchChannelStats:  # calibration_pipeline.rs:65-72
    label: str
    lights_input: int
    lights_after_rejection: list
    mean: float
    stddev: float


@dataclass
class BatchPipelineResult:  # calibration_pipeline.rs:51-56
    master_channels: list          # [(label, master)]
    rgb: object                    # (h, w, 3) f32 or None
    channels: list                 # [BatchChannelStats]
    darks_combined: int = 0
    flats_combined: int = 0
    bias_combined: int = 0


@dataclass
class SubframeWeightConfig:  # subframe.rs:24-49
    fwhm_weight: float = 1.0
    eccentricity_weight: float = 0.5
    snr_weight: float = 1.0
    noise_weight: float = 0.3
    max_fwhm: float = 8.0
    max_eccentricity: float = 0.7
    min_snr: float = 5.0
    min_stars: int = 5

    def _c(self):
        return _lib.SubframeWeightConfigC(self.fwhm_weight, self.eccentricity_weight, self.snr_weight, self.noise_weight,
                                          self.max_fwhm, self.max_eccentricity, self.min_snr, self.min_stars)


@dataclass
class SubframeMetrics:  # subframe.rs:9-22 (file_path stays with the caller)
    star_count: int
    median_fwhm: float
    median_eccentricity: float
    median_snr: float
    background_median: float
    background_sigma: float
    noise_ratio: float
    weight: float
    accepted: bool


class StackFrameParams(NamedTuple):
    """ab_stack_frame_param of n frames, column by column: what stack_params_from_metrics returns and Context.stack_weighted takes"""
    weights: np.ndarray    # f64 [n]; 0 = the frame takes no part
    scales: np.ndarray     # f32 [n]
    offsets: np.ndarray    # f32 [n]
    reference: int         # the frame the others were normalised to


def stack_params_from_metrics(metrics, normalize: str = "none") -> StackFrameParams:
    """ab_stack_params_from_metrics: the weights of the accepted subframes and, with normalize = "additive" | "multiplicative", the
    offsets or scales that bring every frame's background to the best frame's.  Host arithmetic in the library: no GPU, no context."""
    if normalize not in _lib.STACK_NORM:
        raise AstroBurstError(_lib.AB_ERR_INVALID, f"normalize must be one of {sorted(_lib.STACK_NORM)} (got {normalize!r})")
    n = len(metrics)
    ms = (_lib.SubframeMetricsC * max(n, 1))(*[
        _lib.SubframeMetricsC(int(m.star_count), m.median_fwhm, m.median_eccentricity, m.median_snr, m.background_median, m.background_sigma,
                              m.noise_ratio, m.weight, 1 if m.accepted else 0) for m in metrics])
    out = (_lib.StackFrameParamC * max(n, 1))()
    ref = C.c_size_t(0)
    rc = _lib.lib().ab_stack_params_from_metrics(ms, n, _lib.STACK_NORM[normalize], out, C.byref(ref))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_stack_params_from_metrics: no accepted frame of positive weight, or the best frame's background cannot "
                                  "be normalised to")
    return StackFrameParams(np.array([p.weight for p in out[:n]], np.float64), np.array([p.scale for p in out[:n]], np.float32),
                            np.array([p.offset for p in out[:n]], np.float32), int(ref.value))


def stack_frame_params(n: int, weights, scales=None, offsets=None):
    """-> the ctypes array of n ab_stack_frame_param (scales default to 1, offsets to 0).  Raises what ab_stack_weighted would return for
    them, before anything touches the device: a count that is not n, a negative or non-finite weight, a non-finite scale or offset."""
    w = np.asarray(weights, np.float64).ravel()
    with np.errstate(over="ignore"):  # (a value beyond f32 becomes inf and is refused below)
        s = np.ones(n, np.float32) if scales is None else np.asarray(scales, np.float32).ravel()
        o = np.zeros(n, np.float32) if offsets is None else np.asarray(offsets, np.float32).ravel()
    for name, a in (("weights", w), ("scales", s), ("offsets", o)):
        if a.size != n:
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"{a.size} {name} for {n} frames")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise AstroBurstError(_lib.AB_ERR_INVALID, "a frame has a negative or non-finite weight")
    if not (np.isfinite(s).all() and np.isfinite(o).all()):
        raise AstroBurstError(_lib.AB_ERR_INVALID, "a frame has a non-finite scale or offset")
    return (_lib.StackFrameParamC * max(n, 1))(*[_lib.StackFrameParamC(float(w[i]), float(s[i]), float(o[i])) for i in range(n)])


AFFINE_METHODS = ("affine", "rigid", "phase_correlation", "identity")


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def generate_gaussian_psf(size: int, sigma: float) -> np.ndarray:
    """generate_gaussian_psf (deconvolution.rs:12-33) -> size x size f32, normalised (host scalar maths in the library: no GPU)."""
    out = np.zeros((int(size), int(size)), np.float32)
    rc = _lib.lib().ab_generate_gaussian_psf(int(size), float(sigma), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_generate_gaussian_psf: bad arguments")
    return out


def _psf_config(num_stars=None, cutout_radius=None, saturation_threshold=None, min_peak_fraction=None, max_ellipticity=None,
                edge_margin=None, max_center_distance_fraction=None):
    """PsfEstimationConfig::default() (psf_estimation.rs:27-39, filled in by the library) with the given fields replaced"""
    cfg = _lib.PsfEstimationConfigC()
    _lib.lib().ab_psf_estimation_config_default(C.byref(cfg))
    for name, val, conv in (("num_stars", num_stars, int), ("cutout_radius", cutout_radius, int), ("saturation_threshold", saturation_threshold, float),
                            ("min_peak_fraction", min_peak_fraction, float), ("max_ellipticity", max_ellipticity, float),
                            ("edge_margin", edge_margin, int), ("max_center_distance_fraction", max_center_distance_fraction, float)):
        if val is not None:
            if conv is int and int(val) < 0:
                raise AstroBurstError(_lib.AB_ERR_INVALID, f"{name} must not be negative")
            setattr(cfg, name, conv(val))
    return cfg


def _psf_star_array(stars):
    arr = (_lib.PsfStarC * max(len(stars), 1))()
    for i, s in enumerate(stars):
        t = (s.x, s.y, s.peak, s.flux, s.fwhm, s.ellipticity, s.distance_from_center, s.snr) if hasattr(s, "fwhm") else tuple(s)
        arr[i] = _lib.PsfStarC(*[float(v) for v in t])
    return arr


def psf_select_stars(stars, max_val: float, rows: int, cols: int, **config):
    """The quality filter, score_star, the stable descending sort and take(num_stars) of estimate_psf (psf_estimation.rs:68-92,
    :509-516) -> (indices of the selected stars in selection order, number of stars that passed the filter).  stars: PsfStar
    objects or 8-tuples (x, y, peak, flux, fwhm, ellipticity, distance_from_center, snr); max_val: the image's maximum; config:
    PsfEstimationConfig's fields.  Host scalar maths in the library: no GPU."""
    cfg = _psf_config(**config)
    n = len(stars)
    arr = _psf_star_array(stars)
    idx = (C.c_size_t * max(n, 1))()
    sel, flt = C.c_size_t(0), C.c_size_t(0)
    rc = _lib.lib().ab_psf_select_stars(arr, n, C.byref(cfg), float(max_val), int(rows), int(cols), idx, n, C.byref(sel), C.byref(flt))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_psf_select_stars: bad arguments")
    return [int(idx[i]) for i in range(sel.value)], int(flt.value)


VOTE_DIM = 64  # a vote matrix is VOTE_DIM x VOTE_DIM uint32: row = reference star index, column = target star index


def _star_xy(xy) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))


def triangle_votes_host(ref_xy, tgt_xy) -> np.ndarray:
    """The vote matrix of the library's HOST matcher (the vote half of match_triangles, affine.rs:320-350) for two star lists of
    (x, y) -> uint32 [64, 64].  Host arithmetic in the library: no GPU."""
    r, t = _star_xy(ref_xy), _star_xy(tgt_xy)
    out = np.zeros((VOTE_DIM, VOTE_DIM), np.uint32)
    dp = C.POINTER(C.c_double)
    rc = _lib.lib().ab_triangle_votes_host(r.ctypes.data_as(dp), r.shape[0], t.ctypes.data_as(dp), t.shape[0],
                                           out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_triangle_votes_host: bad arguments")
    return out


def matches_from_votes(votes, n_ref: int, n_tgt: int):
    """The greedy half of match_triangles (affine.rs:351-384) on a given 64 x 64 vote matrix -> [(ref index, tgt index)] in
    acceptance order (votes descending, ties by (ref, tgt) index).  Host arithmetic in the library: no GPU."""
    v = np.ascontiguousarray(np.asarray(votes, np.uint32).reshape(VOTE_DIM, VOTE_DIM))
    ri, ti = (C.c_size_t * VOTE_DIM)(), (C.c_size_t * VOTE_DIM)()
    n = C.c_size_t(0)
    rc = _lib.lib().ab_matches_from_votes(int(n_ref), int(n_tgt), v.ctypes.data_as(C.POINTER(C.c_uint32)), ri, ti, VOTE_DIM, C.byref(n))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_matches_from_votes: bad arguments")
    return [(int(ri[i]), int(ti[i])) for i in range(min(n.value, VOTE_DIM))]


_SYNTH_FIELDS = {"uniform": _lib.AB_SYNTH_FIELD_UNIFORM, "king_cluster": _lib.AB_SYNTH_FIELD_KING_CLUSTER,
                 "exponential_disk": _lib.AB_SYNTH_FIELD_EXPONENTIAL_DISK}
_SYNTH_PSFS = {"gaussian": _lib.AB_SYNTH_PSF_GAUSSIAN, "moffat": _lib.AB_SYNTH_PSF_MOFFAT, "airy": _lib.AB_SYNTH_PSF_AIRY}


def synth_psf_type(psf) -> "_lib.SynthPsfTypeC":
    """PsfType (core/synth/pipeline.rs:24-28) from ("gaussian", fwhm), ("moffat", fwhm, beta) or ("airy", lambda_over_d)"""
    if isinstance(psf, _lib.SynthPsfTypeC):
        return psf
    kind, *par = psf
    par = [float(v) for v in par] + [0.0, 0.0]
    return _lib.SynthPsfTypeC(_SYNTH_PSFS[kind] if isinstance(kind, str) else int(kind), par[0], par[1])


def synth_noise_params(**fields) -> "_lib.SynthNoiseParamsC":
    """NoiseParams::default() (noise.rs:18-30, filled in by the library) with the given fields replaced"""
    cfg = _lib.SynthConfigC()
    _lib.lib().ab_synth_config_default(C.byref(cfg))
    p = _lib.SynthNoiseParamsC.from_buffer_copy(cfg.noise)
    for name, val in fields.items():
        setattr(p, name, int(val) & (2 ** 64 - 1) if name == "seed" else float(val))
    return p


def synth_config(field_type=("uniform",), psf=None, noise=None, apply_vignette=None, vignette_strength=None, n_frames=None,
                 **field) -> "_lib.SynthConfigC":
    """SynthConfig::default() (pipeline.rs:41-53, filled in by the library) with the given parts replaced.  field_type: ("uniform",),
    ("king_cluster", core_radius, tidal_radius) or ("exponential_disk", scale_length, inclination_deg); psf: see synth_psf_type;
    noise: a dict of NoiseParams fields; the remaining keywords are FieldConfig's (width, height, n_stars, flux_min, flux_max, seed)."""
    cfg = _lib.SynthConfigC()
    _lib.lib().ab_synth_config_default(C.byref(cfg))
    kind, *par = field_type
    par = [float(v) for v in par] + [0.0, 0.0]
    cfg.field_type = _lib.SynthFieldTypeC(_SYNTH_FIELDS[kind] if isinstance(kind, str) else int(kind), par[0], par[1])
    if psf is not None:
        cfg.psf_type = synth_psf_type(psf)
    if noise is not None:
        cfg.noise = synth_noise_params(**noise)
    if apply_vignette is not None:
        cfg.apply_vignette = 1 if apply_vignette else 0
    if vignette_strength is not None:
        cfg.vignette_strength = float(vignette_strength)
    if n_frames is not None:
        cfg.n_frames = int(n_frames)
    for name, val in field.items():
        if name not in ("width", "height", "n_stars", "flux_min", "flux_max", "seed"):
            raise TypeError(f"unknown FieldConfig field {name}")
        setattr(cfg.field, name, float(val) if name.startswith("flux") else int(val) & (2 ** 64 - 1) if name == "seed" else int(val))
    return cfg


def synth_rng_f64(seed: int, skip: int, n: int) -> np.ndarray:
    """draws skip .. skip + n - 1 (gen::<f64>()) of rand 0.8.5's StdRng::seed_from_u64(seed); host-only"""
    out = np.empty(int(n), np.float64)
    rc = _lib.lib().ab_synth_rng_f64(int(seed) & (2 ** 64 - 1), int(skip), int(n), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_synth_rng_f64: bad arguments")
    return out


def synth_chacha_block(key, counter: int, rounds: int = 12) -> np.ndarray:
    """test hook: the 16 output words of one ChaCha block (key: eight u32 words; 64-bit counter; zero stream id); host-only"""
    k = np.ascontiguousarray(key, dtype=np.uint32)
    assert k.shape == (8,)
    out = np.empty(16, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = _lib.lib().ab_synth_chacha_block(k.ctypes.data_as(u32p), int(counter), int(rounds), out.ctypes.data_as(u32p))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_synth_chacha_block: rounds must be 12 or 20")
    return out


def synth_star_field(cfg=None, **config) -> np.ndarray:
    """gen_field (pipeline.rs:126-138) of a SynthConfig (or of synth_config(**config)) -> float64 array (n_stars, 5): x, y, z, flux,
    temperature per star.  Host scalar maths in the library: no GPU."""
    cfg = cfg if cfg is not None else synth_config(**config)
    n = int(cfg.field.n_stars)
    out = np.zeros((max(n, 1), 5), np.float64)
    got = C.c_size_t(0)
    rc = _lib.lib().ab_synth_star_field(C.byref(cfg), out.ctypes.data_as(C.POINTER(_lib.SynthStarC)), n, C.byref(got))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_synth_star_field: the field would not terminate (king_cluster radii) or its kind is unknown")
    return out[:n]


@dataclass
class SynthFrames:  # what generate / generate_stack return (pipeline.rs:63, :84) + the library's route count
    frames: list
    truth: object
    stars: np.ndarray   # (star_count, 5): x, y, z, flux, temperature
    frames_on_host: int


def power_spectrum_dims(rows: int, cols: int):
    """(original_size, display_size) of compute_power_spectrum (core/analysis/fft.rs:24-25, :53-57): the next power of two of the
    longer side, and that capped at 1024.  Host-only; images beyond 16384 a side raise AB_ERR_UNSUPPORTED."""
    size, disp = C.c_int64(0), C.c_int64(0)
    rc = _lib.lib().ab_power_spectrum_dims(int(rows), int(cols), C.byref(size), C.byref(disp))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_power_spectrum_dims: rows and cols must be >= 1 and at most 16384")
    return int(size.value), int(disp.value)


def hann_symmetric_f32(n: int) -> np.ndarray:
    """hann_symmetric::<f32>(n) (math/window.rs:20-35), host-only: the table the GPU path multiplies by"""
    out = np.empty(int(n), np.float32)
    rc = _lib.lib().ab_hann_symmetric_f32(int(n), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_hann_symmetric_f32: bad arguments")
    return out


def _wavelet_config(num_scales, thresholds, linear_denoise, keep):
    """ab_wavelet_config over a float array that `keep` holds alive for the length of the call"""
    th = (C.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    keep.append(th)
    return _lib.WaveletConfigC(max(int(num_scales), 0), th if len(thresholds) else None, len(thresholds), 1 if linear_denoise else 0)


def wavelet_scale_thresholds(noise_sigma: float, thresholds=(3.0, 2.5, 2.0, 1.5, 1.0)) -> np.ndarray:
    """The eight per-scale f32 thresholds wavelet_denoise derives from noise_sigma (wavelet.rs:93-99, :218-225): scale j takes
    thresholds[j], beyond the list its last entry, of an empty list 1.0 (host scalar maths in the library: no GPU)."""
    keep = []
    cfg = _wavelet_config(8, thresholds, True, keep)
    out = np.zeros(8, np.float32)
    rc = _lib.lib().ab_wavelet_scale_thresholds(float(noise_sigma), C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != _lib.AB_OK:
        raise AstroBurstError(rc, "ab_wavelet_scale_thresholds: bad arguments")
    return out


def _drizzle_config(scale, pixfrac, kernel, sigma_low, sigma_high, sigma_iterations, align=False, alignment_method=0, num_threads=8):
    kernel = DRIZZLE_KERNELS[kernel.lower()] if isinstance(kernel, str) else int(kernel)
    alignment_method = DRIZZLE_ALIGNMENT[alignment_method.lower()] if isinstance(alignment_method, str) else int(alignment_method)
    return _lib.DrizzleConfigC(float(scale), float(pixfrac), kernel, float(sigma_low), float(sigma_high), int(sigma_iterations),
                               1 if align else 0, alignment_method, int(num_threads))


def _host_shapes(frames):
    """ab_plane descriptors carrying only the dims (the host-only entry point never reads the data)"""
    return (Plane * max(len(frames), 1))(*[Plane(None, int(f.shape[0]), int(f.shape[1]), 0) for f in frames])


def drizzle_output_dims(frames, scale=2.0, pixfrac=0.7):
    """the checks and dims of drizzle_stack (drizzle.rs:231-279) -> (in_rows, in_cols, out_rows, out_cols); frames: arrays / tensors
    or (rows, cols) shapes.  Host-only: no GPU.  AstroBurstError for no frames, one frame, dims that vary too much, > 32 767 frames."""
    class _S:
        def __init__(self, shape):
            self.shape = shape
    fr = [f if hasattr(f, "shape") else _S(tuple(f)) for f in frames]
    cfg = _drizzle_config(scale, pixfrac, 0, 3.0, 3.0, 5)
    v = [C.c_int64(0) for _ in range(4)]
    rc = _lib.lib().ab_drizzle_output_dims(_host_shapes(fr), len(fr), C.byref(cfg), *[C.byref(x) for x in v])
    if rc != _lib.AB_OK:
        n = len(fr)
        raise AstroBurstError(rc, "No images to drizzle" if n == 0 else "Drizzle requires at least 2 frames for sub-pixel reconstruction" if n < 2
                              else "ab_drizzle_output_dims: frame dimensions vary too much, too many frames or a NaN scale / pixfrac")
    return tuple(int(x.value) for x in v)


class Comm:
    """One RCCL rank bound to a Context's GPU (include/astroburst_hip.h section (e)).  Multi-process: rank 0 calls
    Comm.unique_id(), the host carries the 128 bytes to the other ranks, every rank constructs Comm(ctx, id, nranks, rank)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * _lib.AB_COMM_ID_BYTES)()
        rc = _lib.lib().ab_comm_get_unique_id(buf)
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "ab_comm_get_unique_id failed (librccl.so.1 not loadable?)")
        return bytes(buf)

    def __init__(self, ctx: "Context", uid: bytes, nranks: int, rank: int):
        assert len(uid) == _lib.AB_COMM_ID_BYTES
        self._ctx = ctx
        self._L = ctx._L
        h = C.c_void_p()
        buf = (C.c_uint8 * _lib.AB_COMM_ID_BYTES).from_buffer_copy(uid)
        ctx._check(self._L.ab_comm_init_rank(ctx._h, buf, nranks, rank, C.byref(h)))
        self._h = h

    @classmethod
    def host(cls, ctx: "Context", name: str, nranks: int, rank: int) -> "Comm":
        """ab_comm_init_rank_host: host-staged collectives through the shared segment /abcomm_<name> (ranks may share a GPU)."""
        self = cls.__new__(cls)
        self._ctx = ctx
        self._L = ctx._L
        h = C.c_void_p()
        ctx._check(self._L.ab_comm_init_rank_host(ctx._h, name.encode(), nranks, rank, C.byref(h)))
        self._h = h
        return self

    @property
    def is_host(self) -> bool:
        return bool(self._L.ab_comm_is_host(self._h))

    def agree(self, local_status: int = 0) -> int:
        """ab_comm_agree: AB_OK only if every rank passed AB_OK (raises otherwise)"""
        self._ctx.use_torch_stream()
        rc = self._L.ab_comm_agree(self._ctx._h, self._h, int(local_status))
        self._ctx._check(rc)
        return rc

    def abort(self):
        self._L.ab_comm_abort(self._h)

    def set_timeout_ms(self, ms: int):
        self._ctx._check(self._L.ab_comm_set_timeout_ms(self._h, int(ms)))

    @property
    def rank(self) -> int:
        return self._L.ab_comm_rank(self._h)

    @property
    def size(self) -> int:
        return self._L.ab_comm_size(self._h)

    @property
    def collectives_issued(self) -> int:
        return int(self._L.ab_comm_collectives_issued(self._h))

    _DT = {"torch.int32": _lib.AB_DT_I32, "torch.int64": _lib.AB_DT_I64, "torch.float32": _lib.AB_DT_F32, "torch.float64": _lib.AB_DT_F64,
           "torch.uint32": _lib.AB_DT_U32, "torch.uint64": _lib.AB_DT_U64}

    def allreduce(self, t, op: str = "sum"):
        """in place, on the context's stream"""
        assert t.is_cuda and t.is_contiguous()
        self._ctx.use_torch_stream()
        ops = {"sum": _lib.AB_RED_SUM, "max": _lib.AB_RED_MAX, "min": _lib.AB_RED_MIN}
        self._ctx._check(self._L.ab_comm_allreduce(self._ctx._h, self._h, C.c_void_p(t.data_ptr()), t.numel(), self._DT[str(t.dtype)], ops[op]))
        return t

    def close(self):
        if getattr(self, "_h", None):
            self._L.ab_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlaneList:
    """The ab_plane descriptors of a list of planes, built ONCE (Context.planes).  A host in Rust or C holds its `ab_plane` array ready;
    this module rebuilds one per call -- 2 us of Python per plane, 0.4 ms of an idle GPU for the bench step's 190 planes -- so a caller
    that passes the same frames again and again (bench.py) marshals them once and passes the list."""

    def __init__(self, ctx, frames):
        self.frames = list(frames)
        self.keep = []
        self.n = len(self.frames)
        self.array = (Plane * max(self.n, 1))(*[ctx._plane(f, self.keep) for f in self.frames])
        self.device = any(_is_torch(f) and f.is_cuda for f in self.frames)
        self.rows = min((p.rows for p in self.array[:self.n]), default=0)
        self.cols = min((p.cols for p in self.array[:self.n]), default=0)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.frames[i]


class Context:
    """One ab_ctx: a device, a stream, a scratch arena.  Not thread-safe; one per caller thread."""

    def __init__(self, device: int = 0):
        self._L = _lib.lib()
        h = C.c_void_p()
        rc = self._L.ab_ctx_create(device, C.byref(h))
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "ab_ctx_create failed: no gfx950 (MI355X) device visible"
                                      if rc == _lib.AB_ERR_NO_DEVICE else "ab_ctx_create failed")
        self._h = h
        self.device = device
        self._stream = None   # the torch stream the context currently launches on (None: its own)

    def close(self):
        if getattr(self, "_h", None):
            self._L.ab_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, self._L.ab_last_error(self._h).decode())

    def use_torch_stream(self):
        """Launch on torch's current stream: calls are then ordered with the torch kernels that produce their inputs and
        consume their outputs, and torch.cuda.Event timing brackets them.  Done automatically whenever a torch tensor is
        passed as a plane (a device plane handed over by torch is only meaningful in torch's stream order)."""
        s = torch.cuda.current_stream().cuda_stream
        if s != self._stream:
            self._check(self._L.ab_ctx_set_stream(self._h, C.c_void_p(s)))
            self._stream = s

    def use_own_stream(self):
        """Back to the context's private stream (host planes; C callers that manage ordering themselves)."""
        self._check(self._L.ab_ctx_reset_stream(self._h))
        self._stream = None

    def synchronize(self):
        self._check(self._L.ab_ctx_synchronize(self._h))

    def trim(self):
        """release the device memory the context has grown (workspaces, scratch, host-frame staging); it stays usable"""
        self._check(self._L.ab_ctx_trim(self._h))

    FALLBACK_KINDS = ("frames_redone", "tile_slots", "component_table", "selection_short", "selection_cut", "tiles_declined",
                      "stats_chain", "stack_general_pixels", "label_tiles_dense")   # ab_fallback_kind, include/astroburst_hip.h

    def fallback_counts(self, reset: bool = False) -> dict:
        """How often a fast path handed over to its exact fallback (same results, more time) since the context was created or last
        reset -- frame workers included (ab_ctx_fallback_counts)."""
        out = (C.c_uint64 * len(self.FALLBACK_KINDS))()
        self._check(self._L.ab_ctx_fallback_counts(self._h, out, len(self.FALLBACK_KINDS), 1 if reset else 0))
        return dict(zip(self.FALLBACK_KINDS, (int(v) for v in out)))

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(), C.c_uint64()
        self._check(self._L.ab_device_info(self._h, name, 256, C.byref(cu), C.byref(mem)))
        return name.value.decode(), cu.value, mem.value

    # ---- plane marshalling -----------------------------------------------------------------
    def planes(self, frames) -> "PlaneList":
        """the frames' ab_plane descriptors, marshalled once; every call that takes a list of planes takes the result too"""
        return frames if isinstance(frames, PlaneList) else PlaneList(self, frames)

    def _plane_array(self, frames, keep):
        """(ctypes array of ab_plane, count) of a list of planes or of a PlaneList"""
        if isinstance(frames, PlaneList):
            if frames.device:
                self.use_torch_stream()   # (what _plane does once per call for device planes)
            return frames.array, frames.n
        return (Plane * max(len(frames), 1))(*[self._plane(f, keep) for f in frames]), len(frames)

    def _plane(self, x, keep):
        if _is_torch(x) and not x.is_cuda:  # a host plane held by torch (pinned memory keeps the library's uploads asynchronous)
            assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous(), "host planes are contiguous 2-D float32 tensors"
            keep.append(x)
            return Plane(C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], 0)
        if _is_torch(x):
            assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous(), \
                "device planes are contiguous 2-D float32 CUDA tensors"
            if not keep or not _is_torch(keep[-1]):  # once per call: torch.cuda.current_stream() costs microseconds, a stack has 64 planes
                self.use_torch_stream()
            keep.append(x)
            return Plane(C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], 1)
        a = np.ascontiguousarray(x, dtype=np.float32)
        assert a.ndim == 2, "planes are 2-D (rows, cols)"
        keep.append(a)
        return Plane(C.c_void_p(a.ctypes.data), a.shape[0], a.shape[1], 0)

    def _new_like(self, ref, rows, cols):
        if _is_torch(ref):
            return torch.empty((rows, cols), dtype=torch.float32, device=ref.device)
        return np.empty((rows, cols), np.float32)

    # ---- core/stacking/combine.rs ------------------------------------------------------------
    def stack_sigma_clip(self, frames, sigma_low=3.0, sigma_high=3.0, max_iterations=5, out=None, want_rejected=True):
        """Per-pixel sigma_clip_combine over equal-or-larger frames (combine.rs:14-92,160-182).
        want_rejected=False keeps the call asynchronous (fetch the count with last_rejected())."""
        if len(frames) == 0:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "No images to stack")
        keep = []
        planes, n = self._plane_array(frames, keep)
        if isinstance(frames, PlaneList):
            rows, cols = frames.rows, frames.cols
        else:
            rows = min(p.rows for p in planes)
            cols = min(p.cols for p in planes)
        if out is None:
            out = self._new_like(frames[0], rows, cols)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), rows, cols, 0)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_sigma_clip(self._h, planes, n, C.byref(cfg), C.byref(po),
                                                C.byref(rej) if want_rejected else None))
        return out, (int(rej.value) if want_rejected else None)

    def stack_weighted(self, frames, weights, scales=None, offsets=None, sigma_low=3.0, sigma_high=3.0, max_iterations=5, out=None,
                       want_weight=False, want_rejected=True):
        """ab_stack_weighted: every frame normalised (p * scale + offset), sigma_clip_combine's rejection on the normalised samples,
        then the mean of the survivors weighted per frame.  A frame of weight 0 takes no part; at most 64 frames of weight > 0.
        -> (image, rejected), or (image, weight_plane, rejected) with want_weight; want_rejected=False keeps the call asynchronous
        (fetch the count with last_rejected())."""
        if len(frames) == 0:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "No images to stack")
        params = stack_frame_params(len(frames), weights, scales, offsets)
        keep = []
        planes, n = self._plane_array(frames, keep)
        if isinstance(frames, PlaneList):
            rows, cols = frames.rows, frames.cols
        else:
            rows = min(p.rows for p in planes)
            cols = min(p.cols for p in planes)
        if out is None:
            out = self._new_like(frames[0], rows, cols)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), rows, cols, 0)
        wplane, pw = None, None
        if want_weight:
            wplane = self._new_like(out, rows, cols)
            pw = self._plane(wplane, keep) if _is_torch(wplane) else Plane(C.c_void_p(wplane.ctypes.data), rows, cols, 0)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_weighted(self._h, planes, params, n, C.byref(cfg), C.byref(po), C.byref(pw) if want_weight else None,
                                              C.byref(rej) if want_rejected else None))
        rejected = int(rej.value) if want_rejected else None
        return (out, wplane, rejected) if want_weight else (out, rejected)

    def last_rejected(self) -> int:
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_last_rejected(self._h, C.byref(rej)))
        return int(rej.value)

    def stack_last_kernel_ms(self) -> float:
        """duration of the last stack launch's kernels (HIP events recorded by the library on the launch stream)"""
        ms = C.c_float()
        self._check(self._L.ab_stack_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def stack_images(self, images, sigma_low=3.0, sigma_high=3.0, max_iterations=5, align=True) -> StackResult:
        """stack_images(&[Array2<f32>], &StackConfig) (combine.rs:94-193)."""
        n = len(images)
        if n == 0:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "No images to stack")
        keep = []
        planes = (Plane * n)(*[self._plane(f, keep) for f in images])
        rows = min(p.rows for p in planes)
        cols = min(p.cols for p in planes)
        out = self._new_like(images[0], rows, cols)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), rows, cols, 0)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 1 if align else 0)
        rej = C.c_uint64(0)
        offs = (C.c_int32 * (2 * n))()
        self._check(self._L.ab_stack_images(self._h, planes, n, C.byref(cfg), C.byref(po), offs, C.byref(rej)))
        offsets = [(int(offs[2 * i]), int(offs[2 * i + 1])) for i in range(n)]
        return StackResult(out, n, int(rej.value), offsets)

    def sigma_clip_combine(self, values, sigma_low=3.0, sigma_high=3.0, max_iter=5):
        """sigma_clip_combine(values, lo, hi, max_iter) -> (f32, u32) (combine.rs:14-92), run on
        the GPU as a one-pixel stack of len(values) frames."""
        vals = np.asarray(values, dtype=np.float32).ravel()
        if vals.size == 0:
            return np.float32(0.0), 0  # combine.rs:21-23 (no frames: nothing to launch)
        frames = [np.full((1, 1), v, np.float32) for v in vals]
        out, rej = self.stack_sigma_clip(frames, sigma_low, sigma_high, max_iter)
        return np.float32(out[0, 0]), rej

    def stack_partial(self, frames, sigma_low=3.0, sigma_high=3.0, max_iterations=5):
        """Frame-sharded partial: per-pixel (f64 sum, u32 count) of this shard's survivors."""
        assert all(_is_torch(f) for f in frames), "partial stacking takes device frames"
        keep = []
        planes = (Plane * len(frames))(*[self._plane(f, keep) for f in frames])
        rows = min(p.rows for p in planes)
        cols = min(p.cols for p in planes)
        dev = frames[0].device
        s = torch.empty((rows, cols), dtype=torch.float64, device=dev)
        cnt = torch.empty((rows, cols), dtype=torch.int32, device=dev)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_sigma_clip_partial(self._h, planes, len(frames), C.byref(cfg), rows, cols,
                                                        C.c_void_p(s.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                        C.byref(rej)))
        return s, cnt, int(rej.value)

    def stack_partial_into(self, frames, s, cnt, sigma_low=3.0, sigma_high=3.0, max_iterations=5):
        """stack_partial into caller-owned device buffers, fully asynchronous (no rejected read-back)."""
        keep = []
        planes = (Plane * len(frames))(*[self._plane(f, keep) for f in frames])
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        self._check(self._L.ab_stack_sigma_clip_partial(self._h, planes, len(frames), C.byref(cfg), s.shape[0],
                                                        s.shape[1], C.c_void_p(s.data_ptr()),
                                                        C.c_void_p(cnt.data_ptr()), None))
        return s, cnt, None

    def stack_finalize_partial_into(self, s, cnt, out):
        self._check(self._L.ab_stack_finalize_partial(self._h, C.c_void_p(s.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                      s.numel(), C.c_void_p(out.data_ptr())))
        return out

    def stack_finalize_partial(self, s, cnt):
        out = torch.empty(s.shape, dtype=torch.float32, device=s.device)
        self._check(self._L.ab_stack_finalize_partial(self._h, C.c_void_p(s.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                      s.numel(), C.c_void_p(out.data_ptr())))
        return out

    # ---- progress / cancel (infra/progress.rs:39-74) ------------------------------------------
    def set_progress_cb(self, fn):
        """fn(stage: str, current: int, total: int) at the reference's stage boundaries; None removes it."""
        if fn is None:
            self._progress = None
            self._check(self._L.ab_ctx_set_progress_cb(self._h, _lib.PROGRESS_CB(0), None))
            return
        self._progress = _lib.PROGRESS_CB(lambda stage, cur, tot, _u: fn(stage.decode(), int(cur), int(tot)))
        self._check(self._L.ab_ctx_set_progress_cb(self._h, self._progress, None))

    def request_cancel(self):
        self._check(self._L.ab_ctx_request_cancel(self._h))

    def clear_cancel(self):
        self._check(self._L.ab_ctx_clear_cancel(self._h))

    # ---- (e) multi-GPU: row bands, frame shards (csrc/sharded.hip) ---------------
    def shard_rows(self, rows: int, nranks: int, rank: int):
        r0, nr = C.c_int64(), C.c_int64()
        self._check(self._L.ab_shard_rows(rows, nranks, rank, C.byref(r0), C.byref(nr)))
        return int(r0.value), int(nr.value)

    def shard_frames(self, n_frames: int, nranks: int, rank: int):
        f0, nf = C.c_size_t(), C.c_size_t()
        self._check(self._L.ab_shard_frames(n_frames, nranks, rank, C.byref(f0), C.byref(nf)))
        return int(f0.value), int(nf.value)

    def stack_sigma_clip_rows(self, frames, row0: int, nrows: int, sigma_low=3.0, sigma_high=3.0, max_iterations=5, out=None,
                              want_rejected=True):
        """rows [row0, row0 + nrows) of the stack of ALL frames (the exact single-level estimator on a band)."""
        keep = []
        planes = (Plane * len(frames))(*[self._plane(f, keep) for f in frames])
        cols = min(p.cols for p in planes)
        if out is None:
            out = torch.empty((nrows, cols), dtype=torch.float32, device=frames[0].device)
        po = Plane(C.c_void_p(out.data_ptr()), nrows, cols, 1)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_sigma_clip_rows(self._h, planes, len(frames), C.byref(cfg), row0, C.byref(po),
                                                     C.byref(rej) if want_rejected else None))
        return out, (int(rej.value) if want_rejected else None)

    def stack_sigma_clip_rowband(self, comm, frames, out_band, sigma_low=3.0, sigma_high=3.0, max_iterations=5, want_rejected=True):
        """this rank's band of the exact stack + StackResult.rejected_pixels summed over the ranks"""
        keep = []
        planes = (Plane * len(frames))(*[self._plane(f, keep) for f in frames])
        po = Plane(C.c_void_p(out_band.data_ptr()), out_band.shape[0], out_band.shape[1], 1)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_sigma_clip_rowband(self._h, comm._h if comm else None, planes, len(frames), C.byref(cfg), C.byref(po),
                                                        C.byref(rej) if want_rejected else None))
        return out_band, (int(rej.value) if want_rejected else None)

    def stack_sigma_clip_sharded(self, comm, local_frames, out, sigma_low=3.0, sigma_high=3.0, max_iterations=5, want_rejected=False):
        """frame-sharded two-level stack: partial over this rank's frames -> RCCL all-reduce(sum, count) -> divide"""
        keep = []
        planes = (Plane * len(local_frames))(*[self._plane(f, keep) for f in local_frames])
        po = self._plane(out, keep)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_sigma_clip_sharded(self._h, comm._h if comm else None, planes, len(local_frames), C.byref(cfg),
                                                        C.byref(po), C.byref(rej) if want_rejected else None))
        return out, (int(rej.value) if want_rejected else None)

    def stack_sharded_last_ms(self):
        """(span of the partial stacks on the context's stream, time inside the all-reduces + divisions on the comm stream) of the last
        stack_sigma_clip_sharded; blocks until that call's work is done"""
        a, b = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.ab_stack_sharded_last_ms(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def allgather_rows(self, comm, band, full):
        keep = []
        pb = Plane(C.c_void_p(band.data_ptr() if band.numel() else 0), band.shape[0], band.shape[1], 1)
        pf = self._plane(full, keep)
        self._check(self._L.ab_allgather_rows(self._h, comm._h if comm else None, C.byref(pb), C.byref(pf)))
        return full

    def register_frames_sharded(self, comm, reference, targets, num_threads: int = 8):
        """align_channel_affine(reference, t) for every t, target i estimated on rank i mod size; all results everywhere"""
        keep = []
        pr = self._plane(reference, keep)
        planes = (Plane * max(len(targets), 1))(*[self._plane(t, keep) for t in targets])
        res = (_lib.AffineAlignResultC * max(len(targets), 1))()
        self._check(self._L.ab_register_frames_sharded(self._h, comm._h if comm else None, C.byref(pr), planes, len(targets), num_threads, res))
        return [AffineAlignResult(tuple(r.transform), int(r.matched_stars), int(r.inliers), r.residual_px, AFFINE_METHODS[r.method])
                for r in res[:len(targets)]]

    def align_pairs_affine_rowband(self, comm, reference, targets, out_bands, row0: int, target_row0=None, num_threads: int = 8):
        """the row-band scheme's registration as one call: this rank's rows [row0, row0 + band rows) of every registered frame;
        targets[i] = rows [target_row0[i], ...) of target i (whole for i mod size == rank); own frames are warped as they are fitted"""
        keep = []
        pr = self._plane(reference, keep)
        n = len(targets)
        planes = (Plane * max(n, 1))()
        for i, t in enumerate(targets):
            if t.numel() == 0:
                planes[i] = Plane(C.c_void_p(0), 0, reference.shape[1], 1)
            else:
                planes[i] = self._plane(t, keep)
        outs = (Plane * max(n, 1))()
        for i, o in enumerate(out_bands):
            outs[i] = Plane(C.c_void_p(o.data_ptr() if o.numel() else 0), o.shape[0], o.shape[1], 1)
        t0 = (C.c_int64 * max(n, 1))(*[int(v) for v in (target_row0 if target_row0 is not None else [0] * n)]) if n else None
        res = (_lib.AffineAlignResultC * max(n, 1))()
        self._check(self._L.ab_align_pairs_affine_rowband(self._h, comm._h if comm else None, C.byref(pr), planes, t0, n, num_threads, row0, res, outs))
        return [AffineAlignResult(tuple(r.transform), int(r.matched_stars), int(r.inliers), r.residual_px, AFFINE_METHODS[r.method]) for r in res[:n]]

    def compute_image_stats_sharded(self, comm, band, total_rows: int) -> ImageStats:
        keep = []
        pb = self._plane(band, keep)
        s = ImageStatsC()
        self._check(self._L.ab_compute_image_stats_sharded(self._h, comm._h if comm else None, C.byref(pb), total_rows, C.byref(s)))
        return self._stats_out(s)

    def warp_image_rows(self, image, transform, out_rows: int, row0: int, out_band):
        keep = []
        pi = self._plane(image, keep)
        po = self._plane(out_band, keep)
        t = (C.c_double * 6)(*[float(v) for v in transform])
        self._check(self._L.ab_warp_image_rows(self._h, C.byref(pi), t, out_rows, row0, C.byref(po)))
        return out_band

    def warp_image_rows_from_band(self, src_band, src_row0: int, src_rows: int, transform, out_rows: int, row0: int, out_band):
        """rows [row0, ..) of warp_image with the source given as rows [src_row0, src_row0 + len(src_band)) of a src_rows-row frame"""
        keep = []
        pi = self._plane(src_band, keep)
        po = self._plane(out_band, keep)
        t = (C.c_double * 6)(*[float(v) for v in transform])
        self._check(self._L.ab_warp_image_rows_from_band(self._h, C.byref(pi), src_row0, src_rows, t, out_rows, row0, C.byref(po)))
        return out_band

    def warp_source_rows(self, transform, src_rows: int, src_cols: int, out_cols: int, row0: int, nrows: int):
        """(first source row, count) that output rows [row0, row0 + nrows) of warp_image read"""
        t = (C.c_double * 6)(*[float(v) for v in transform])
        s0, sn = C.c_int64(), C.c_int64()
        self._check(self._L.ab_warp_source_rows(t, src_rows, src_cols, out_cols, row0, nrows, C.byref(s0), C.byref(sn)))
        return s0.value, sn.value

    def shard_source_rows(self, transforms, src_rows: int, src_cols: int, out_rows: int, out_cols: int, nranks: int, rank: int):
        """(first source row, count): this rank's rows of every target + the halo the transforms need"""
        flat = [float(v) for tr in transforms for v in tr]
        t = (C.c_double * max(len(flat), 1))(*flat)
        s0, sn = C.c_int64(), C.c_int64()
        self._check(self._L.ab_shard_source_rows(t, len(transforms), src_rows, src_cols, out_rows, out_cols, nranks, rank, C.byref(s0), C.byref(sn)))
        return s0.value, sn.value

    def auto_stretch_preview(self, image, out=None, comm=None, total_rows: int = 0, target_bg=0.25, shadow_k=-2.8, fetch=True):
        """auto_stretch_preview (cmd/common.rs:18-22): compute_image_stats -> auto_stf -> apply_stf (u8) as one asynchronous device
        chain.  -> (u8 plane, ImageStats | None, StfParams | None); fetch=False leaves the call fully asynchronous."""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = torch.empty((pi.rows, pi.cols), dtype=torch.uint8, device=image.device)
        cfg = AutoStfConfigC(target_bg, shadow_k)
        s, p = ImageStatsC(), StfParamsC()
        self._check(self._L.ab_auto_stretch_preview(self._h, comm._h if comm else None, C.byref(pi), total_rows, C.byref(cfg),
                                                    C.c_void_p(out.data_ptr()), C.byref(s) if fetch else None, C.byref(p) if fetch else None))
        if not fetch:
            return out, None, None
        return out, self._stats_out(s), StfParams(p.shadow, p.midtone, p.highlight)

    # ---- core/stacking/align.rs, core/alignment/affine.rs -------------------------------------
    def shift_image_subpixel(self, image, dy: float, dx: float, out=None):
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), pi.rows, pi.cols, 0)
        self._check(self._L.ab_shift_image_subpixel(self._h, C.byref(pi), dy, dx, C.byref(po)))
        return out

    def warp_image(self, image, transform, out_rows: int, out_cols: int, out=None):
        """transform = (a, b, tx, c, d, ty): output (x, y) -> source (sx, sy) (affine.rs:74-80)."""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, out_rows, out_cols)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), out_rows, out_cols, 0)
        t = (C.c_double * 6)(*[float(v) for v in transform])
        self._check(self._L.ab_warp_image(self._h, C.byref(pi), t, C.byref(po)))
        return out

    # ---- core/imaging/stats.rs ------------------------------------------------------------------
    @staticmethod
    def _stats_out(s: ImageStatsC) -> ImageStats:
        return ImageStats(s.min, s.max, s.median, s.mad, s.sigma, s.mean, int(s.valid_count))

    @staticmethod
    def _stats_in(st: ImageStats) -> ImageStatsC:
        return ImageStatsC(st.min, st.max, st.median, st.mad, st.sigma, st.mean, st.valid_count)

    def compute_image_stats(self, image) -> ImageStats:
        keep = []
        pi = self._plane(image, keep)
        s = ImageStatsC()
        self._check(self._L.ab_compute_image_stats(self._h, C.byref(pi), C.byref(s)))
        return self._stats_out(s)

    def compute_image_stats_with_known_range(self, image, known_min: float, known_max: float) -> ImageStats:
        keep = []
        pi = self._plane(image, keep)
        s = ImageStatsC()
        self._check(self._L.ab_compute_image_stats_with_known_range(self._h, C.byref(pi), known_min, known_max,
                                                                    C.byref(s)))
        return self._stats_out(s)

    def build_histogram(self, image, bins: int, dmin: float, dmax: float) -> np.ndarray:
        keep = []
        pi = self._plane(image, keep)
        out = np.zeros(bins, np.uint32)
        self._check(self._L.ab_build_histogram(self._h, C.byref(pi), bins, dmin, dmax, C.c_void_p(out.ctypes.data)))
        return out

    def stats_value_hist(self, image, gmin: float, gmax: float):
        keep = []
        pi = self._plane(image, keep)
        h = np.zeros(65536, np.uint64)
        s, c = C.c_double(), C.c_uint64()
        self._check(self._L.ab_stats_value_hist(self._h, C.byref(pi), gmin, gmax, C.c_void_p(h.ctypes.data),
                                                C.byref(s), C.byref(c)))
        return h, s.value, int(c.value)

    # ---- core/imaging/stf.rs ---------------------------------------------------------------------
    def auto_stf(self, stats: ImageStats, target_bg=0.25, shadow_k=-2.8) -> StfParams:
        s = self._stats_in(stats)
        cfg = AutoStfConfigC(target_bg, shadow_k)
        p = StfParamsC()
        rc = self._L.ab_auto_stf(C.byref(s), C.byref(cfg), C.byref(p))
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "ab_auto_stf: null argument")
        return StfParams(p.shadow, p.midtone, p.highlight)

    def apply_stf(self, image, params: StfParams, stats: ImageStats, out=None):
        """apply_stf -> u8 (stf.rs:89-102)."""
        keep = []
        pi = self._plane(image, keep)
        p = StfParamsC(params.shadow, params.midtone, params.highlight)
        s = self._stats_in(stats)
        if _is_torch(image):
            if out is None:
                out = torch.empty((pi.rows, pi.cols), dtype=torch.uint8, device=image.device)
            self._check(self._L.ab_apply_stf_u8(self._h, C.byref(pi), C.byref(p), C.byref(s),
                                                C.c_void_p(out.data_ptr()), 1))
        else:
            if out is None:
                out = np.empty((pi.rows, pi.cols), np.uint8)
            self._check(self._L.ab_apply_stf_u8(self._h, C.byref(pi), C.byref(p), C.byref(s),
                                                C.c_void_p(out.ctypes.data), 0))
        return out

    def apply_stf_f32(self, image, params: StfParams, stats: ImageStats, out=None):
        """apply_stf_f32 (stf.rs:104-120); pass out=image for apply_stf_inplace (:147-155)."""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), pi.rows, pi.cols, 0)
        p = StfParamsC(params.shadow, params.midtone, params.highlight)
        s = self._stats_in(stats)
        self._check(self._L.ab_apply_stf_f32(self._h, C.byref(pi), C.byref(p), C.byref(s), C.byref(po)))
        return out

    # ---- core/imaging/calibration_pipeline.rs -------------------------------------------
    def _masters(self, bias, dark, flat, keep):
        m = _lib.CalibrationMastersC()
        for name, x in (("bias", bias), ("dark", dark), ("flat", flat)):
            if x is not None:
                pl = self._plane(x, keep)
                keep.append(pl)
                setattr(m, name, C.pointer(pl))
        return m

    def _planes(self, xs, keep):
        return (Plane * max(len(xs), 1))(*[self._plane(x, keep) for x in xs])

    def calibrate_light(self, light, bias=None, dark=None, flat=None, out=None):
        """calibrate_light (calibration_pipeline.rs:74-118)"""
        keep = []
        pi = self._plane(light, keep)
        if out is None:
            out = self._new_like(light, pi.rows, pi.cols)
        po = self._plane(out, keep)
        m = self._masters(bias, dark, flat, keep)
        self._check(self._L.ab_calibrate_light(self._h, C.byref(pi), C.byref(m), C.byref(po)))
        return out

    def normalize_frames(self, frames):
        """normalize_frames (:309-319) -> new frames"""
        keep = []
        outs = [self._new_like(f, f.shape[0], f.shape[1]) for f in frames]
        self._check(self._L.ab_normalize_frames(self._h, self._planes(frames, keep), len(frames), self._planes(outs, keep)))
        return outs

    def sigma_clipped_mean_stack(self, frames, config: "BatchStackConfig | None" = None):
        """sigma_clipped_mean_stack (:321-378) -> (stacked, rejection_counts)"""
        keep = []
        out = self._new_like(frames[0], frames[0].shape[0], frames[0].shape[1]) if len(frames) else None
        rej = (C.c_uint64 * max(len(frames), 1))()
        cfg = (config or BatchStackConfig())._c()
        po = self._plane(out, keep) if out is not None else Plane()
        self._check(self._L.ab_sigma_clipped_mean_stack(self._h, self._planes(frames, keep), len(frames), C.byref(cfg), C.byref(po), rej))
        return out, list(rej[:len(frames)])

    def run_batch_channel(self, lights, bias=None, dark=None, flat=None, config: "BatchStackConfig | None" = None):
        """one channel of run_batch_pipeline (:157-190), fused -> (master, rejection_counts, mean, stddev)"""
        keep = []
        out = self._new_like(lights[0], lights[0].shape[0], lights[0].shape[1])
        rej = (C.c_uint64 * max(len(lights), 1))()
        st = _lib.BatchChannelStatsC()
        cfg = (config or BatchStackConfig())._c()
        m = self._masters(bias, dark, flat, keep)
        po = self._plane(out, keep)
        self._check(self._L.ab_run_batch_channel(self._h, self._planes(lights, keep), len(lights), C.byref(m), C.byref(cfg), C.byref(po), rej,
                                                 C.byref(st)))
        return out, list(rej[:len(lights)]), st.mean, st.stddev

    def compose_rgb_from_masters(self, r, g, b, l=None):
        """compose_rgb_from_masters (:201-267) -> (h, w, 3) f32"""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        pl = self._plane(l, keep) if l is not None else None
        h, w = min(pr.rows, pg.rows, pb.rows), min(pr.cols, pg.cols, pb.cols)
        if _is_torch(r):
            out = torch.empty((h, w, 3), dtype=torch.float32, device=r.device)
            ptr, dev = C.c_void_p(out.data_ptr()), 1
        else:
            out = np.empty((h, w, 3), np.float32)
            ptr, dev = C.c_void_p(out.ctypes.data), 0
        oh, ow = C.c_int64(), C.c_int64()
        self._check(self._L.ab_compose_rgb_from_masters(self._h, C.byref(pr), C.byref(pg), C.byref(pb), C.byref(pl) if pl is not None else None,
                                                        ptr, dev, C.byref(oh), C.byref(ow)))
        assert (oh.value, ow.value) == (h, w)
        return out

    def run_batch_pipeline(self, channels, bias=None, dark=None, flat=None, config: "BatchStackConfig | None" = None):
        """run_batch_pipeline (:120-199); channels = [(label, [lights])] -> BatchPipelineResult"""
        keep = []
        n = len(channels)
        cin = (_lib.BatchChannelInputC * max(n, 1))()
        masters, rejs = [], []
        for c, (label, lights) in enumerate(channels):
            cin[c].label = label.encode()
            planes = self._planes(lights, keep)
            keep.append(planes)
            cin[c].lights = planes if len(lights) else None
            cin[c].n_lights = len(lights)
            rej = (C.c_uint64 * max(len(lights), 1))()
            rejs.append(rej)
            cin[c].rejection_counts = rej
            masters.append(self._new_like(lights[0], lights[0].shape[0], lights[0].shape[1]) if len(lights) else np.zeros((1, 1), np.float32))
        pout = self._planes(masters, keep)
        st = (_lib.BatchChannelStatsC * max(n, 1))()
        cfg = (config or BatchStackConfig())._c()
        m = self._masters(bias, dark, flat, keep)
        find = {}
        for c, (label, _) in enumerate(channels):
            find.setdefault(label.upper(), c)
        rgb, ptr, dev = None, None, 0
        if n and all(k in find for k in "RGB"):
            h = min(masters[find[k]].shape[0] for k in "RGB")
            w = min(masters[find[k]].shape[1] for k in "RGB")
            if _is_torch(masters[0]):
                rgb = torch.empty((h, w, 3), dtype=torch.float32, device=masters[0].device)
                ptr, dev = C.c_void_p(rgb.data_ptr()), 1
            else:
                rgb = np.empty((h, w, 3), np.float32)
                ptr, dev = C.c_void_p(rgb.ctypes.data), 0
        oh, ow = C.c_int64(), C.c_int64()
        self._check(self._L.ab_run_batch_pipeline(self._h, cin, n, C.byref(m), C.byref(cfg), pout, st, ptr, dev, C.byref(oh), C.byref(ow)))
        stats = [BatchChannelStats(channels[c][0], int(st[c].lights_input), list(rejs[c][:len(channels[c][1])]), st[c].mean, st[c].stddev)
                 for c in range(n)]
        return BatchPipelineResult([(channels[c][0], masters[c]) for c in range(n)], rgb, stats, int(dark is not None), int(flat is not None),
                                   int(bias is not None))

    # ---- preview / tile renderers up to the PNG encoder --------------------------------
    def _stf3(self, stf, stats):
        if stf is None:
            return None, None
        return ((StfParamsC * 3)(*[StfParamsC(p.shadow, p.midtone, p.highlight) for p in stf]),
                (_lib.ImageStatsC * 3)(*[self._stats_in(s) for s in stats]) if stats is not None else None)

    def _bytes_out(self, like, shape, out=None):
        """u8 output next to the input: a CUDA tensor for device planes, a numpy array for host planes -> (array, ptr, on_device);
        or the caller's `out` (contiguous uint8 of that many bytes, CUDA tensor or numpy array)"""
        if out is not None:
            n = int(np.prod(shape))
            if _is_torch(out):
                ok = out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
                ptr, dev = out.data_ptr(), 1
            else:
                ok = isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.size == n
                ptr, dev = (out.ctypes.data, 0) if ok else (0, 0)
            if not ok:
                raise AstroBurstError(_lib.AB_ERR_INVALID, f"the output must be contiguous uint8 of {n} bytes")
            return out, C.c_void_p(ptr), dev
        if _is_torch(like):
            out = torch.empty(shape, dtype=torch.uint8, device=like.device)
            return out, C.c_void_p(out.data_ptr()), 1
        out = np.empty(shape, np.uint8)
        return out, C.c_void_p(out.ctypes.data), 0

    def preview_dims(self, rows: int, cols: int, max_dim: int):
        ph, pw = C.c_int64(), C.c_int64()
        if self._L.ab_preview_dims(rows, cols, max_dim, C.byref(ph), C.byref(pw)) != _lib.AB_OK:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "ab_preview_dims: bad arguments")
        return ph.value, pw.value

    def render_rgb_preview(self, r, g, b, max_dim: int, stf=None, stats=None, out=None):
        """render_rgb_preview / render_rgb (stf None) or render_rgb_preview_with_stf (stf, stats = 3 each)
        (cmd/helpers.rs:204-322) -> (ph, pw, 3) u8 (or `out`, contiguous uint8 of that size)"""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        ph, pw = self.preview_dims(pr.rows, pr.cols, max_dim) if max_dim > 0 else (1, 1)
        out, ptr, dev = self._bytes_out(r, (ph, pw, 3), out)
        p, s = self._stf3(stf, stats)
        self._check(self._L.ab_render_rgb_preview(self._h, C.byref(pr), C.byref(pg), C.byref(pb), max_dim, p, s, ptr, dev))
        return out

    def ipc_encode_with_header(self, image, max_dim: int = 0, out=None):
        """encode_with_header / encode_with_header_downsampled (infra/ipc.rs:93-148) -> u8 buffer (header + f32 LE pixels)"""
        keep = []
        pi = self._plane(image, keep)
        full = max_dim <= 0 or (pi.rows <= max_dim and pi.cols <= max_dim)
        ph, pw = (pi.rows, pi.cols) if full else self.preview_dims(pi.rows, pi.cols, max_dim)
        out, ptr, dev = self._bytes_out(image, (16 + 4 * ph * pw,), out)
        n = C.c_size_t(0)
        self._check(self._L.ab_ipc_encode_with_header(self._h, C.byref(pi), max_dim, ptr, dev, C.byref(n)))
        assert n.value == 16 + 4 * ph * pw
        return out

    def tile_compute_num_levels(self, width: int, height: int, tile_size: int) -> int:
        return self._L.ab_tile_compute_num_levels(width, height, tile_size)

    def tile_pyramid_layout(self, rows: int, cols: int, tile_size: int, channels: int):
        lv, n, total = (_lib.TileLevelC * _lib.MAX_TILE_LEVELS)(), C.c_int32(), C.c_size_t()
        if self._L.ab_tile_pyramid_layout(rows, cols, tile_size, channels, lv, C.byref(n), C.byref(total)) != _lib.AB_OK:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "ab_tile_pyramid_layout: bad arguments")
        return [{k: getattr(l, k) for k, _ in l._fields_} for l in lv[:n.value]], total.value

    def tile_downsample_2x(self, image):
        keep = []
        pi = self._plane(image, keep)
        out = self._new_like(image, (pi.rows + 1) // 2, (pi.cols + 1) // 2)
        po = self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), out.shape[0], out.shape[1], 0)
        self._check(self._L.ab_tile_downsample_2x(self._h, C.byref(pi), C.byref(po)))
        return out

    def tile_percentile_bounds(self, image, low_pct: float = 0.001, high_pct: float = 0.999):
        keep = []
        pi = self._plane(image, keep)
        lo, hi = C.c_float(), C.c_float()
        self._check(self._L.ab_tile_percentile_bounds(self._h, C.byref(pi), low_pct, high_pct, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def generate_tile_pyramid(self, normalized, tile_size: int = 256, out=None):
        """generate_tile_pyramid (infra/render/tiles.rs:180-255) up to the encoder -> (packed tiles u8, levels, (gmin, gmax))"""
        keep = []
        pi = self._plane(normalized, keep)
        levels, total = self.tile_pyramid_layout(pi.rows, pi.cols, tile_size, 1)
        out, ptr, dev = self._bytes_out(normalized, (total,), out)
        lv, n, lo, hi = (_lib.TileLevelC * _lib.MAX_TILE_LEVELS)(), C.c_int32(), C.c_float(), C.c_float()
        self._check(self._L.ab_generate_tile_pyramid(self._h, C.byref(pi), tile_size, ptr, dev, lv, C.byref(n), C.byref(lo), C.byref(hi)))
        return out, levels, (lo.value, hi.value)

    def generate_tile_pyramid_rgb(self, r, g, b, tile_size: int = 256, stf=None, stats=None, out=None):
        """generate_tile_pyramid_rgb / _rgb_stf (tiles.rs:363-481) up to the encoder -> (packed tiles u8, levels)"""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        levels, total = self.tile_pyramid_layout(pr.rows, pr.cols, tile_size, 3)
        out, ptr, dev = self._bytes_out(r, (total,), out)
        lv, n = (_lib.TileLevelC * _lib.MAX_TILE_LEVELS)(), C.c_int32()
        p, s = self._stf3(stf, stats)
        self._check(self._L.ab_generate_tile_pyramid_rgb(self._h, C.byref(pr), C.byref(pg), C.byref(pb), tile_size, p, s, ptr, dev, lv,
                                                         C.byref(n)))
        return out, levels

    # ---- core/analysis/star_detection.rs, core/alignment/affine.rs ------------------------------------
    def estimate_background(self, image, tile_size: int):
        keep = []
        pi = self._plane(image, keep)
        m, s = C.c_double(), C.c_double()
        self._check(self._L.ab_estimate_background(self._h, C.byref(pi), tile_size, C.byref(m), C.byref(s)))
        return m.value, s.value

    def background_tile_stats(self, image, tile_size: int):
        """per-tile sigma_clipped_stats of estimate_background's tiling -> (median[nty, ntx], sigma[nty, ntx], valid[nty, ntx])"""
        keep = []
        pi = self._plane(image, keep)
        step = max(int(tile_size), 16)
        nty, ntx = -(-pi.rows // step), -(-pi.cols // step)
        med, sig = np.zeros(nty * ntx), np.zeros(nty * ntx)
        val = np.zeros(nty * ntx, np.int32)
        n, nx = C.c_size_t(), C.c_size_t()
        self._check(self._L.ab_background_tile_stats(self._h, C.byref(pi), tile_size, med.ctypes.data_as(C.POINTER(C.c_double)),
                                                     sig.ctypes.data_as(C.POINTER(C.c_double)), val.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     nty * ntx, C.byref(n), C.byref(nx)))
        assert (n.value, nx.value) == (nty * ntx, ntx)
        return med.reshape(nty, ntx), sig.reshape(nty, ntx), val.reshape(nty, ntx).astype(bool)

    def detect_stars(self, image, sigma_threshold: float, max_stars: int = 100000):
        """detect_stars(image, sigma) -> (stars, background_median, background_sigma) (star_detection.rs:86-258)"""
        keep = []
        pi = self._plane(image, keep)
        buf = (_lib.DetectedStarC * max_stars)()
        n, tot = C.c_size_t(0), C.c_size_t(0)
        m, s = C.c_double(), C.c_double()
        self._check(self._L.ab_detect_stars(self._h, C.byref(pi), sigma_threshold, buf, max_stars, C.byref(n),
                                            C.byref(tot), C.byref(m), C.byref(s)))
        stars = [DetectedStar(b.x, b.y, b.flux, b.fwhm, b.eccentricity, b.peak, int(b.npix), b.snr)
                 for b in buf[:n.value]]
        return stars, m.value, s.value

    def normalize_for_detection(self, image, out=None):
        return self._unary(self._L.ab_normalize_for_detection, image, out)

    def align_channel_affine(self, reference, target, num_threads: int = 8) -> "AffineAlignResult":
        """align_channel_affine(reference, target) (affine.rs:129-212)"""
        keep = []
        pr, pt = self._plane(reference, keep), self._plane(target, keep)
        res = _lib.AffineAlignResultC()
        self._check(self._L.ab_align_channel_affine(self._h, C.byref(pr), C.byref(pt), num_threads, C.byref(res)))
        return AffineAlignResult(tuple(res.transform), int(res.matched_stars), int(res.inliers), res.residual_px,
                                 AFFINE_METHODS[res.method])

    def register_frames(self, reference, targets, num_threads: int = 8):
        """align_channel_affine(reference, t) for every t in targets, sharing the reference's detection
        (affine.rs:129-212) -> [AffineAlignResult]"""
        keep = []
        pr = self._plane(reference, keep)
        planes = (Plane * max(len(targets), 1))(*[self._plane(t, keep) for t in targets])
        res = (_lib.AffineAlignResultC * max(len(targets), 1))()
        self._check(self._L.ab_register_frames(self._h, C.byref(pr), planes, len(targets), num_threads, res))
        return [AffineAlignResult(tuple(r.transform), int(r.matched_stars), int(r.inliers), r.residual_px, AFFINE_METHODS[r.method])
                for r in res[:len(targets)]]

    def align_pairs_affine(self, reference, targets, outs, num_threads: int = 8):
        """align_pair(reference, t, AlignMethod::Affine) for every t (pair.rs:41-77): estimate + warp_image into outs[i]
        (device planes).  The reference and the targets may be HOST planes (numpy arrays / CPU tensors, pinned for asynchronous
        copies): the library uploads them on its own stream and registers every frame as it lands.  -> [AffineAlignResult]"""
        keep = []
        pr = self._plane(reference, keep)
        planes, n = self._plane_array(targets, keep)
        pouts, n_out = self._plane_array(outs, keep)
        assert n == n_out, "one output plane per target"
        res = (_lib.AffineAlignResultC * max(len(targets), 1))()
        self._check(self._L.ab_align_pairs_affine(self._h, C.byref(pr), planes, n, num_threads, res, pouts))
        return [AffineAlignResult(tuple(r.transform), int(r.matched_stars), int(r.inliers), r.residual_px, AFFINE_METHODS[r.method])
                for r in res[:len(targets)]]

    def analyze_subframes(self, images, config: "SubframeWeightConfig | None" = None, normalize: bool = False):
        """analyze_subframe(image, _, config) for every image (subframe.rs:51-121), frame-parallel -> [SubframeMetrics];
        normalize=True also applies normalize_weights (:148-159)."""
        keep = []
        n = len(images)
        planes = (Plane * max(n, 1))(*[self._plane(im, keep) for im in images])
        res = (_lib.SubframeMetricsC * max(n, 1))()
        cfg = (config or SubframeWeightConfig())._c()
        self._check(self._L.ab_analyze_subframes(self._h, planes, n, C.byref(cfg), res))
        if normalize:
            self._L.ab_normalize_subframe_weights(res, n)
        return [SubframeMetrics(int(r.star_count), r.median_fwhm, r.median_eccentricity, r.median_snr, r.background_median,
                                r.background_sigma, r.noise_ratio, r.weight, bool(r.accepted)) for r in res[:n]]

    def analyze_subframe(self, image, config: "SubframeWeightConfig | None" = None):
        return self.analyze_subframes([image], config)[0]

    def affine_from_stars(self, ref_xy, tgt_xy, rows, cols, num_threads: int = 8):
        r = np.ascontiguousarray(np.asarray(ref_xy, np.float64).reshape(-1, 2))
        t = np.ascontiguousarray(np.asarray(tgt_xy, np.float64).reshape(-1, 2))
        res, found = _lib.AffineAlignResultC(), C.c_int(0)
        rc = self._L.ab_affine_from_stars(r.ctypes.data_as(C.POINTER(C.c_double)), r.shape[0],
                                          t.ctypes.data_as(C.POINTER(C.c_double)), t.shape[0], rows, cols,
                                          num_threads, C.byref(res), C.byref(found))
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "ab_affine_from_stars: bad arguments")
        if not found.value:
            return None
        return AffineAlignResult(tuple(res.transform), int(res.matched_stars), int(res.inliers), res.residual_px,
                                 AFFINE_METHODS[res.method])

    def triangle_votes(self, ref_xy, targets, grouped: bool = False) -> np.ndarray:
        """The vote matrices of the GPU matcher (the one register_frames / align_pairs_affine run after detection) for GIVEN star
        lists: one reference list against every list of `targets` -> uint32 [len(targets), 64, 64].  grouped=False takes the targets
        one after another, grouped=True in groups of up to eight in the given order, as a batch's two forms do."""
        r = _star_xy(ref_xy)
        ts = [_star_xy(t) for t in targets]
        cat = np.ascontiguousarray(np.concatenate(ts + [np.zeros((0, 2))]) if ts else np.zeros((0, 2)))
        counts = (C.c_size_t * max(len(ts), 1))(*[t.shape[0] for t in ts])
        out = np.zeros((len(ts), VOTE_DIM, VOTE_DIM), np.uint32)
        dp = C.POINTER(C.c_double)
        self._check(self._L.ab_triangle_votes_device(self._h, r.ctypes.data_as(dp), r.shape[0], cat.ctypes.data_as(dp), counts, len(ts),
                                                     1 if grouped else 0, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    # ---- core/alignment/phase_correlation.rs ----------------------------------------------------------
    def phase_correlate(self, reference, target):
        """phase_correlate(reference, target) -> (dx, dy, confidence) (phase_correlation.rs:22-89)."""
        keep = []
        pr, pt = self._plane(reference, keep), self._plane(target, keep)
        res = _lib.PhaseCorrelationResultC()
        self._check(self._L.ab_phase_correlate(self._h, C.byref(pr), C.byref(pt), C.byref(res)))
        return res.dx, res.dy, res.confidence

    def correlate_single(self, a, b, want_surface=False):
        """correlate_single (phase_correlation.rs:105-141), dims <= 512; optionally the correlation surface."""
        keep = []
        pa, pb = self._plane(a, keep), self._plane(b, keep)
        res = _lib.PhaseCorrelationResultC()
        surf = None
        if want_surface:
            fr = 1 << max(0, (pa.rows - 1).bit_length())
            fc = 1 << max(0, (pa.cols - 1).bit_length())
            surf = np.zeros((fr, fc), np.float64)
        self._check(self._L.ab_correlate_single(self._h, C.byref(pa), C.byref(pb), C.byref(res),
                                                C.c_void_p(surf.ctypes.data) if surf is not None else None))
        return (res.dx, res.dy, res.confidence, surf) if want_surface else (res.dx, res.dy, res.confidence)

    # ---- colour / tone / calibration maps -----------------------------------------------------------
    def _out_plane(self, out, keep, rows, cols):
        return self._plane(out, keep) if _is_torch(out) else Plane(C.c_void_p(out.ctypes.data), rows, cols, 0)

    def _unary(self, fn, image, out, *mid):
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        po = self._out_plane(out, keep, pi.rows, pi.cols)
        self._check(fn(self._h, C.byref(pi), *mid, C.byref(po)))
        return out

    def apply_scnr_inplace(self, r, g, b, method="average", amount=1.0, preserve_luminance=False):
        """apply_scnr_inplace(&mut r, &mut g, &mut b, &ScnrConfig) (scnr.rs:18-53); mutates r, g, b."""
        keep = []
        planes = []
        for x in (r, g, b):
            if _is_torch(x):
                planes.append(self._plane(x, keep))
            else:
                assert isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags.c_contiguous, \
                    "in-place SCNR needs contiguous float32 arrays"
                planes.append(Plane(C.c_void_p(x.ctypes.data), x.shape[0], x.shape[1], 0))
        cfg = _lib.ScnrConfigC(0 if method in ("average", "AverageNeutral", 0) else 1, amount,
                               1 if preserve_luminance else 0)
        self._check(self._L.ab_apply_scnr_inplace(self._h, C.byref(planes[0]), C.byref(planes[1]),
                                                  C.byref(planes[2]), C.byref(cfg)))

    def blend_channels(self, channels, weights, rows, cols):
        """blend_channels(&[&Array2], &[BlendWeight], rows, cols) -> (R, G, B) (channel_blend.rs:13-70).
        weights: iterable of (channel_idx, r_weight, g_weight, b_weight)."""
        keep = []
        chans = (Plane * len(channels))(*[self._plane(c, keep) for c in channels])
        ws = (_lib.BlendWeightC * max(1, len(weights)))(*[_lib.BlendWeightC(int(w[0]), w[1], w[2], w[3])
                                                           for w in weights])
        outs = [self._new_like(channels[0], rows, cols) for _ in range(3)]
        pos = [self._out_plane(o, keep, rows, cols) for o in outs]
        self._check(self._L.ab_blend_channels(self._h, chans, len(channels), ws, len(weights), C.byref(pos[0]),
                                              C.byref(pos[1]), C.byref(pos[2])))
        return tuple(outs)

    def spline_lut_from_points(self, points) -> np.ndarray:
        """SplineLut::from_points (curves.rs:69-95) -> 4096 f32 (host scalar maths in the library)."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
        lut = np.zeros(4096, np.float32)
        rc = self._L.ab_spline_lut_from_points(pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0],
                                               lut.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "ab_spline_lut_from_points: bad arguments")
        return lut

    def apply_curve(self, image, lut, out=None):
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        assert lut.size == 4096
        return self._unary(self._L.ab_apply_curve, image, out, lut.ctypes.data_as(C.POINTER(C.c_float)))

    def apply_levels(self, image, black=0.0, gamma=1.0, white=1.0, out=None):
        p = _lib.LevelsParamsC(black, gamma, white)
        return self._unary(self._L.ab_apply_levels, image, out, C.byref(p))

    def arcsinh_stretch_with_stats(self, image, dmin, dmax, factor, gamma=1.0, out=None):
        return self._unary(self._L.ab_arcsinh_stretch_with_stats, image, out, C.c_float(dmin), C.c_float(dmax),
                           C.c_float(factor), C.c_float(gamma))

    def scale(self, image, factor, out=None):
        return self._unary(self._L.ab_scale, image, out, C.c_float(factor))

    def luminance(self, r, g, b, out=None):
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        if out is None:
            out = self._new_like(r, pr.rows, pr.cols)
        po = self._out_plane(out, keep, pr.rows, pr.cols)
        self._check(self._L.ab_luminance(self._h, C.byref(pr), C.byref(pg), C.byref(pb), C.byref(po)))
        return out

    def calibrate_image(self, raw, master_bias=None, master_dark=None, master_flat=None, dark_exposure_ratio=1.0,
                        out=None):
        """calibrate_image(raw, &CalibrationConfig) (calibration.rs:47-82)."""
        keep = []
        praw = self._plane(raw, keep)
        opt = [C.byref(self._plane(x, keep)) if x is not None else None for x in (master_bias, master_dark, master_flat)]
        if out is None:
            out = self._new_like(raw, praw.rows, praw.cols)
        po = self._out_plane(out, keep, praw.rows, praw.cols)
        self._check(self._L.ab_calibrate_image(self._h, C.byref(praw), opt[0], opt[1], opt[2],
                                               C.c_float(dark_exposure_ratio), C.byref(po)))
        return out

    def median_combine(self, frames, out=None):
        """median_combine_row_major (calibration.rs:84-125): per-pixel upper median of the finite samples."""
        keep = []
        planes = (Plane * len(frames))(*[self._plane(f, keep) for f in frames])
        rows, cols = planes[0].rows, planes[0].cols
        if out is None:
            out = self._new_like(frames[0], rows, cols)
        po = self._out_plane(out, keep, rows, cols)
        self._check(self._L.ab_median_combine(self._h, planes, len(frames), C.byref(po)))
        return out

    # ---- a12 background extraction ------------------------------------------------------------------
    def extract_background(self, image, grid_size=8, poly_degree=3, sigma_clip=2.5, iterations=3, mode="subtract",
                           want_model=True):
        """extract_background (background.rs:55-116) -> BackgroundResult(model, corrected, sample_count, rms_residual).

        mode: "subtract" | "divide" (BackgroundMode).  Raises AstroBurstError with the reference's message when the
        image is too small for the grid, too few samples survive, or the fit is singular."""
        keep = []
        pi = self._plane(image, keep)
        rows, cols = pi.rows, pi.cols
        corrected = self._new_like(image, rows, cols)
        pc = self._out_plane(corrected, keep, rows, cols)
        model, pm = None, None
        if want_model:
            model = self._new_like(image, rows, cols)
            pm = C.byref(self._out_plane(model, keep, rows, cols))
        cfg = _lib.BackgroundConfigC(grid_size, poly_degree, sigma_clip, iterations,
                                     {"subtract": 0, "divide": 1}[mode] if isinstance(mode, str) else int(mode))
        info = _lib.BackgroundInfoC()
        self._check(self._L.ab_extract_background(self._h, C.byref(pi), C.byref(cfg), pm, C.byref(pc), C.byref(info)))
        return BackgroundResult(model, corrected, int(info.sample_count), float(info.rms_residual),
                                np.array(info.coeffs[:], dtype=np.float64))

    # ---- the compose wizard's background step: cmd/processing/background.rs, cmd/common.rs:18-22, :152-193 ----------
    def auto_stretch_preview_sampled(self, image, max_dim=4096, target_bg=0.25, shadow_k=-2.8, fetch=True, out=None):
        """auto_stretch_preview (cmd/common.rs:18-22) followed by save_preview_png's pick (:152-193) as one chain: only the picked
        pixels are stretched.  -> (uint8 (preview_rows, preview_cols), ImageStats | None, StfParams | None); numpy in, numpy out,
        CUDA tensor in, CUDA tensor out (or `out`, contiguous uint8 of that size).  fetch=False with a device output leaves the
        call asynchronous."""
        keep = []
        pi = self._plane(image, keep)
        ph, pw = self.preview_dims(int(pi.rows), int(pi.cols), int(max_dim)) if max_dim >= 1 else (1, 1)
        u8, ptr, dev = self._bytes_out(image, (ph, pw), out)
        cfg = AutoStfConfigC(target_bg, shadow_k)
        s, p = ImageStatsC(), StfParamsC()
        self._check(self._L.ab_auto_stretch_preview_sampled(self._h, C.byref(pi), C.byref(cfg), int(max_dim), ptr, dev, C.byref(s) if fetch else None,
                                                            C.byref(p) if fetch else None))
        if not fetch:
            return u8, None, None
        return u8, self._stats_out(s), StfParams(p.shadow, p.midtone, p.highlight)

    @staticmethod
    def background_step_clamp_config(grid_size: int, poly_degree: int, iterations: int):
        """the clamps extract_background_cmd applies before it builds its BackgroundConfig (background.rs:44-47, types/constants.rs:11-16):
        grid_size 3 ..= 32, poly_degree 1 ..= 5, iterations 1 ..= 10.  background_step takes its arguments as extract_background does."""
        return min(max(int(grid_size), 3), 32), min(max(int(poly_degree), 1), 5), min(max(int(iterations), 1), 10)

    def background_step(self, image, grid_size=8, poly_degree=3, sigma_clip=2.5, iterations=3, mode="subtract", max_dim=4096, want_model=True,
                        want_corrected_u8=True, want_model_u8=True, fetch=True, out_corrected=None, out_model=None, out_corrected_u8=None,
                        out_model_u8=None) -> BackgroundStepResult:
        """extract_background_cmd (cmd/processing/background.rs:17-94) from its loaded plane to the two PNG encoders' inputs and the
        JSON, as one chain: extract_background, each plane's statistics once (the model's with the range its own kernel reduced),
        both previews' picked pixels in one launch, one final synchronisation.  Numpy means host planes and host bytes, CUDA tensors
        device planes and device bytes.  Raises AstroBurstError with the reference's message like extract_background."""
        keep = []
        pi = self._plane(image, keep)
        rows, cols = int(pi.rows), int(pi.cols)
        if out_corrected is None:
            out_corrected = self._new_like(image, rows, cols)
        pc = self._out_plane(out_corrected, keep, out_corrected.shape[0], out_corrected.shape[1])   # (its own dims: the library refuses a mismatch)
        pm = None
        if want_model or out_model is not None:
            if out_model is None:
                out_model = self._new_like(image, rows, cols)
            pm = C.byref(self._out_plane(out_model, keep, out_model.shape[0], out_model.shape[1]))
        ph, pw = self.preview_dims(rows, cols, int(max_dim)) if max_dim >= 1 else (1, 1)
        cu8, cptr, dev = self._bytes_out(image, (ph, pw), out_corrected_u8) if (want_corrected_u8 or out_corrected_u8 is not None) else (None, None, None)
        mu8, mptr, mdev = self._bytes_out(image, (ph, pw), out_model_u8) if (want_model_u8 or out_model_u8 is not None) else (None, None, None)
        if dev is not None and mdev is not None and dev != mdev:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "the two previews' outputs are both host or both device")
        dev = dev if dev is not None else (mdev if mdev is not None else int(_is_torch(image) and image.is_cuda))
        cfg = _lib.BackgroundConfigC(grid_size, poly_degree, sigma_clip, iterations,
                                     {"subtract": 0, "divide": 1}[mode] if isinstance(mode, str) else int(mode))
        info = _lib.BackgroundStepInfoC()
        self._check(self._L.ab_background_step(self._h, C.byref(pi), C.byref(cfg), int(max_dim), C.byref(pc), pm, cptr, mptr, dev,
                                               C.byref(info) if fetch else None))
        if not fetch:
            return BackgroundStepResult(out_corrected, out_model, cu8, mu8, rows, cols, ph, pw, None, None, None, None, None, None, None)
        stf = lambda p: StfParams(p.shadow, p.midtone, p.highlight)  # noqa: E731
        return BackgroundStepResult(out_corrected, out_model, cu8, mu8, int(info.rows), int(info.cols), int(info.preview_rows), int(info.preview_cols),
                                    int(info.bg.sample_count), float(info.bg.rms_residual), np.array(info.bg.coeffs[:], dtype=np.float64),
                                    self._stats_out(info.corrected_stats), self._stats_out(info.model_stats), stf(info.corrected_stf), stf(info.model_stf))

    # ---- a17 RGB composition -------------------------------------------------------------------------
    def resample_image(self, image, target_rows: int, target_cols: int, out=None):
        """resample_image(image, target_rows, target_cols) (resample.rs:25-61)"""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, target_rows, target_cols)
        po = self._out_plane(out, keep, target_rows, target_cols)
        self._check(self._L.ab_resample_image(self._h, C.byref(pi), C.byref(po)))
        return out

    def select_wb_reference(self, sr: ImageStats, sg: ImageStats, sb: ImageStats):
        """select_wb_reference (white_balance.rs:3-20) -> (wb_r, wb_g, wb_b)"""
        out = (C.c_double * 3)()
        rc = self._L.ab_select_wb_reference(*[C.byref(self._stats_in(s)) for s in (sr, sg, sb)], out)
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "select_wb_reference: null argument")
        return tuple(out)

    @staticmethod
    def _rgb_compose_config(white_balance, auto_stretch, stf, linked_stf, align, align_method, scnr, num_threads):
        """ab_rgb_compose_config of process_rgb's keyword arguments"""
        cfg = _lib.RgbComposeConfigC()
        if isinstance(white_balance, str):
            cfg.white_balance = {"auto": 0, "none": 2}[white_balance]
        else:
            cfg.white_balance = 1
            cfg.wb_manual[:] = [float(v) for v in white_balance]
        cfg.auto_stretch, cfg.linked_stf = int(bool(auto_stretch)), int(bool(linked_stf))
        for c, p in enumerate(stf):
            if p is not None:
                cfg.has_stf[c] = 1
                cfg.stf[c] = StfParamsC(p.shadow, p.midtone, p.highlight)
        cfg.align = int(bool(align))
        cfg.align_method = {"phase_correlation": 0, "affine": 1}[align_method]
        if scnr is not None:
            cfg.has_scnr = 1
            m = scnr.get("method", "average")
            cfg.scnr = _lib.ScnrConfigC(0 if m in ("average", "AverageNeutral", 0) else 1, scnr.get("amount", 1.0),
                                        int(bool(scnr.get("preserve_luminance", False))))
        cfg.num_threads = num_threads
        return cfg

    def process_rgb(self, r, g, b, white_balance="auto", auto_stretch=True, stf=(None, None, None), linked_stf=False,
                    align=True, align_method="phase_correlation", scnr=None, num_threads=8, want_pre_stretch=True
                    ) -> ProcessedRgb:
        """process_rgb(r?, g?, b?, &RgbComposeConfig) (rgb.rs:209-323).  Absent channels are None.
        white_balance: "auto" | "none" | (r, g, b) manual multipliers; stf: per-channel StfParams or None (used when
        auto_stretch is False); scnr: None or dict(method=, amount=, preserve_luminance=)."""
        keep = []
        chans = [None if x is None else self._plane(x, keep) for x in (r, g, b)]
        present = [p for p in chans if p is not None]
        first = next((x for x in (r, g, b) if x is not None), None)
        rows = max((p.rows for p in present), default=0)
        cols = max((p.cols for p in present), default=0)
        cfg = self._rgb_compose_config(white_balance, auto_stretch, stf, linked_stf, align, align_method, scnr, num_threads)
        if first is None:
            first = np.empty((0, 0), np.float32)
        outs = [self._new_like(first, rows, cols) for _ in range(3)]
        pos = [self._out_plane(o, keep, rows, cols) for o in outs]
        pres = [self._new_like(first, rows, cols) if want_pre_stretch else None for _ in range(3)]
        pps = [None if p is None else C.byref(self._out_plane(p, keep, rows, cols)) for p in pres]
        info = _lib.ProcessedRgbInfoC()
        self._check(self._L.ab_process_rgb(self._h, *[None if p is None else C.byref(p) for p in chans], C.byref(cfg),
                                           *[C.byref(p) for p in pos], *pps, C.byref(info)))
        return ProcessedRgb(outs[0], outs[1], outs[2], int(info.rows), int(info.cols),
                            tuple(StfParams(p.shadow, p.midtone, p.highlight) for p in info.stf),
                            tuple(tuple(row) for row in info.chan_stats), tuple(info.offset_g), tuple(info.offset_b),
                            bool(info.scnr_applied), bool(info.resampled), tuple(pres),
                            tuple(self._stats_out(s) for s in info.stats_wb))

    # ---- FITS pixel codecs ----------------------------------------------------------
    _BPP = {8: 1, 16: 2, 32: 4, -32: 4, -64: 8}

    def fits_decode_pixels(self, data, rows: int, cols: int, bitpix: int, bscale=1.0, bzero=0.0, out=None):
        """decode_pixels (reader.rs:42-101): data = the big-endian data unit (bytes / numpy uint8 on the host, or a torch
        uint8 CUDA tensor) -> f32 plane."""
        if bitpix not in self._BPP:
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"unsupported BITPIX {bitpix}")
        keep = []
        if _is_torch(data):
            assert data.is_cuda and data.dtype == torch.uint8 and data.is_contiguous()
            self.use_torch_stream()
            ptr, nbytes, on_dev = C.c_void_p(data.data_ptr()), data.numel(), 1
            keep.append(data)
            if out is None:
                out = torch.empty((rows, cols), dtype=torch.float32, device=data.device)
        else:
            buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
            keep.append(buf)
            ptr, nbytes, on_dev = C.c_void_p(buf.ctypes.data), buf.size, 0
            if out is None:
                out = np.empty((rows, cols), np.float32)
        po = self._out_plane(out, keep, rows, cols)
        self._check(self._L.ab_fits_decode_pixels(self._h, ptr, nbytes, on_dev, bitpix, bscale, bzero, C.byref(po)))
        return out

    def fits_compute_bzero_bscale(self, image):
        """compute_bzero_bscale (writer.rs:143-159) -> (bzero, bscale)"""
        keep = []
        pi = self._plane(image, keep)
        bz, bs = C.c_double(), C.c_double()
        self._check(self._L.ab_fits_compute_bzero_bscale(self._h, C.byref(pi), C.byref(bz), C.byref(bs)))
        return bz.value, bs.value

    def fits_encode_pixels(self, image, bitpix: int, bzero=0.0, bscale=1.0) -> np.ndarray:
        """write_*_slice_as_be (writer.rs:82-135) -> the big-endian data unit as a host uint8 array"""
        keep = []
        pi = self._plane(image, keep)
        if bitpix not in (-32, 16, -64):
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"the writer supports BITPIX -32, 16 and -64 (got {bitpix})")
        out = np.empty(pi.rows * pi.cols * self._BPP[bitpix], np.uint8)
        self._check(self._L.ab_fits_encode_pixels(self._h, C.byref(pi), bitpix, bzero, bscale, C.c_void_p(out.ctypes.data), 0))
        return out

    def stack_sigma_clip_raw(self, raw_planes, rows: int, cols: int, bitpix: int, bscale=1.0, bzero=0.0, sigma_low=3.0, sigma_high=3.0,
                             max_iterations=5, out=None, want_rejected=True):
        """ab_stack_sigma_clip over raw big-endian data units (torch uint8 CUDA tensors): decode fused into the stack."""
        need = rows * cols * (abs(int(bitpix)) // 8)
        for t in raw_planes:
            assert _is_torch(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
            if bitpix in (-32, 16) and t.numel() < need:   # a truncated data unit would make the kernel read past the tensor
                raise AstroBurstError(_lib.AB_ERR_INVALID, f"raw plane holds {t.numel()} bytes, {rows}x{cols} BITPIX {bitpix} needs {need}")
        self.use_torch_stream()
        ptrs = (C.c_void_p * len(raw_planes))(*[t.data_ptr() for t in raw_planes])
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float32, device=raw_planes[0].device)
        keep = []
        po = self._out_plane(out, keep, rows, cols)
        cfg = StackConfig(sigma_low, sigma_high, max_iterations, 0)
        rej = C.c_uint64(0)
        self._check(self._L.ab_stack_sigma_clip_raw(self._h, ptrs, len(raw_planes), bitpix, bscale, bzero, C.byref(cfg), C.byref(po),
                                                    C.byref(rej) if want_rejected else None))
        return (out, int(rej.value)) if want_rejected else out

    # ---- caller-side helpers of a17 / a20 ----------------------------------------------------------------
    def apply_lrgb(self, l, r, g, b, lightness_weight=1.0, chrominance_weight=1.0):
        """apply_lrgb(l, &mut r, &mut g, &mut b, lw, cw) (lrgb.rs:4-45); mutates r, g, b."""
        keep = []
        pl = self._plane(l, keep)
        pr, pg, pb = (self._out_plane(x, keep, x.shape[0], x.shape[1]) for x in (r, g, b))
        self._check(self._L.ab_apply_lrgb(self._h, C.byref(pl), C.byref(pr), C.byref(pg), C.byref(pb), lightness_weight,
                                          chrominance_weight))

    def synthesize_luminance(self, r, g, b, out=None):
        """synthesize_luminance (lrgb.rs:47-64 / spcc.rs:185-196): no finite guard."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        if out is None:
            out = self._new_like(r, pr.rows, pr.cols)
        po = self._out_plane(out, keep, pr.rows, pr.cols)
        self._check(self._L.ab_synthesize_luminance(self._h, C.byref(pr), C.byref(pg), C.byref(pb), C.byref(po)))
        return out

    def compute_linked_stf(self, sr: ImageStats, sg: ImageStats, sb: ImageStats, target_bg=0.25, shadow_k=-2.8):
        """compute_linked_stf_with_stats (cmd/helpers.rs:185-202) -> (StfParams, combined ImageStats)"""
        cfg = AutoStfConfigC(target_bg, shadow_k)
        stf, comb = StfParamsC(), ImageStatsC()
        rc = self._L.ab_compute_linked_stf(*[C.byref(self._stats_in(s)) for s in (sr, sg, sb)], C.byref(cfg), C.byref(stf),
                                           C.byref(comb))
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "compute_linked_stf: null argument")
        return StfParams(stf.shadow, stf.midtone, stf.highlight), self._stats_out(comb)

    def calibrate_channel(self, orig, factor: float, orig_stats: ImageStats):
        """calibrate_channel (cmd/compose/color.rs:21-49) -> (scaled plane, ImageStats)"""
        keep = []
        pi = self._plane(orig, keep)
        out = self._new_like(orig, pi.rows, pi.cols)
        po = self._out_plane(out, keep, pi.rows, pi.cols)
        st = ImageStatsC()
        self._check(self._L.ab_calibrate_channel(self._h, C.byref(pi), factor, C.byref(self._stats_in(orig_stats)),
                                                 C.byref(po), C.byref(st)))
        return out, self._stats_out(st)

    def create_master(self, kind: str, frames, master_bias=None, master_dark=None):
        """create_master_bias / _dark / _flat on in-memory frames (calibration.rs:127-255); kind in bias|dark|flat."""
        keep = []
        k = {"bias": 0, "dark": 1, "flat": 2}[kind]
        if len(frames) == 0:
            self._check(self._L.ab_create_master(self._h, k, None, 0, None, None, C.byref(Plane(None, 0, 0, 0))))
        planes = (Plane * len(frames))(*[self._plane(f, keep) for f in frames])
        rows, cols = planes[0].rows, planes[0].cols
        out = self._new_like(frames[0], rows, cols)
        po = self._out_plane(out, keep, rows, cols)
        pb = None if master_bias is None else C.byref(self._plane(master_bias, keep))
        pd = None if master_dark is None else C.byref(self._plane(master_dark, keep))
        self._check(self._L.ab_create_master(self._h, k, planes, len(frames), pb, pd, C.byref(po)))
        return out

    # ---- a18 spectrophotometric colour calibration -------------------------------------------------------
    @staticmethod
    def _spcc_cfg(min_snr, max_stars, saturation_limit, white_reference):
        cfg = _lib.SpccConfigC(min_snr, max_stars, saturation_limit, 0, (C.c_double * 3)(0, 0, 0))
        if isinstance(white_reference, str):
            cfg.white_reference = WHITE_REFERENCES[white_reference]
            name = {"average_spiral": "Average Spiral Galaxy", "g2v": "G2V (Solar)", "photopic": "Photopic (Human Eye)"}[white_reference]
        else:
            cfg.white_reference = 3
            cfg.custom[:] = [float(v) for v in white_reference]
            name = "Custom ({:.2f},{:.2f},{:.2f})".format(*cfg.custom)
        return cfg, name

    def spcc_calibrate_rgb(self, r, g, b, pixel_scale_arcsec: float, min_snr=20.0, max_stars=200, saturation_limit=0.90,
                           white_reference="average_spiral", detection=None) -> SpccResult:
        """spcc_calibrate_rgb (spcc.rs:73-183), built-in Bp-Rp catalogue; pixel_scale_arcsec = WCS pixel scale.
        detection=(stars, lum_max) runs the part after detect_stars on a given detection (:90-183)."""
        keep = []
        ps = [self._plane(x, keep) for x in (r, g, b)]
        cfg, name = self._spcc_cfg(min_snr, max_stars, saturation_limit, white_reference)
        res = _lib.SpccResultC()
        if detection is None:
            rc = self._L.ab_spcc_calibrate_rgb(self._h, *[C.byref(p) for p in ps], pixel_scale_arcsec, C.byref(cfg), C.byref(res))
        else:
            stars, lum_max = detection
            buf = (_lib.DetectedStarC * max(len(stars), 1))()
            for d, s in zip(buf, stars):
                d.x, d.y, d.flux, d.fwhm, d.eccentricity, d.peak, d.snr, d.npix = (s.x, s.y, s.flux, s.fwhm, s.eccentricity,
                                                                                   s.peak, s.snr, s.npix)
            rc = self._L.ab_spcc_from_detection(self._h, *[C.byref(p) for p in ps], buf, len(stars), lum_max,
                                                pixel_scale_arcsec, C.byref(cfg), C.byref(res))
        self._check(rc)
        return SpccResult(res.r_factor, res.g_factor, res.b_factor, int(res.stars_matched), int(res.stars_total),
                          res.avg_color_index, name)

    def spcc_white_reference_rgb(self, white_reference="average_spiral"):
        cfg, _ = self._spcc_cfg(20.0, 200, 0.9, white_reference)
        out = (C.c_double * 3)()
        rc = self._L.ab_spcc_white_reference_rgb(cfg.white_reference, cfg.custom, out)
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "spcc_white_reference_rgb: invalid argument")
        return tuple(out)

    # ---- a13 star mask + masked stretch ---------------------------------------------------------------
    @staticmethod
    def _mask_cfg(growth_factor, softness, detection_sigma, min_fwhm, max_fwhm, luminance_protect, luminance_ceiling):
        return _lib.StarMaskConfigC(growth_factor, softness, detection_sigma, min_fwhm, max_fwhm, int(bool(luminance_protect)),
                                    luminance_ceiling)

    def generate_star_mask(self, image, growth_factor=2.5, softness=4.0, detection_sigma=5.0, min_fwhm=1.5, max_fwhm=30.0,
                           luminance_protect=False, luminance_ceiling=0.85, stars=None, out=None) -> StarMaskResult:
        """generate_star_mask (star_mask.rs:38-44); with stars=[DetectedStar | (x, y, fwhm)] it is
        generate_star_mask_from_detection (:46-138) on that detection.  out: the mask's plane (allocated like the image when None)."""
        keep = []
        pi = self._plane(image, keep)
        mask = self._new_like(image, pi.rows, pi.cols) if out is None else out
        pm = self._out_plane(mask, keep, mask.shape[0], mask.shape[1])
        cfg = self._mask_cfg(growth_factor, softness, detection_sigma, min_fwhm, max_fwhm, luminance_protect, luminance_ceiling)
        info = _lib.StarMaskInfoC()
        if stars is None:
            self._check(self._L.ab_generate_star_mask(self._h, C.byref(pi), C.byref(cfg), C.byref(pm), C.byref(info)))
        else:
            buf = (_lib.DetectedStarC * max(len(stars), 1))()
            for b, s in zip(buf, stars):
                b.x, b.y, b.fwhm = (s.x, s.y, s.fwhm) if hasattr(s, "fwhm") else s
            self._check(self._L.ab_generate_star_mask_from_stars(self._h, C.byref(pi), buf, len(stars), C.byref(cfg),
                                                                 C.byref(pm), C.byref(info)))
        return StarMaskResult(mask, int(info.stars_masked), float(info.coverage_fraction))

    @staticmethod
    def _ms_cfg(iterations, target_background, mask_growth, mask_softness, luminance_protect, luminance_ceiling,
                protection_amount, convergence_threshold):
        return _lib.MaskedStretchConfigC(iterations, target_background, mask_growth, mask_softness, int(bool(luminance_protect)),
                                         luminance_ceiling, protection_amount, convergence_threshold)

    @staticmethod
    def _ms_result(image, r):
        return MaskedStretchResult(image, int(r.iterations_run), float(r.final_background), int(r.stars_masked),
                                   float(r.mask_coverage), bool(r.converged))

    def masked_stretch(self, image, iterations=10, target_background=0.25, mask_growth=2.5, mask_softness=4.0,
                       luminance_protect=True, luminance_ceiling=0.85, protection_amount=0.85, convergence_threshold=1e-5,
                       mask: "StarMaskResult | None" = None, out=None) -> MaskedStretchResult:
        """masked_stretch (masked_stretch.rs:44-58); with mask=StarMaskResult it is masked_stretch_with_mask (:60-118).  out: the
        stretched plane (allocated like the image when None)."""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        po = self._out_plane(out, keep, out.shape[0], out.shape[1])
        cfg = self._ms_cfg(iterations, target_background, mask_growth, mask_softness, luminance_protect, luminance_ceiling,
                           protection_amount, convergence_threshold)
        res = _lib.MaskedStretchResultC()
        if mask is None:
            self._check(self._L.ab_masked_stretch(self._h, C.byref(pi), C.byref(cfg), C.byref(po), C.byref(res)))
        else:
            pm = self._plane(mask.mask, keep)
            mi = _lib.StarMaskInfoC(mask.stars_masked, mask.coverage_fraction)
            self._check(self._L.ab_masked_stretch_with_mask(self._h, C.byref(pi), C.byref(pm), C.byref(mi), C.byref(cfg),
                                                            C.byref(po), C.byref(res)))
        return self._ms_result(out, res)

    def masked_stretch_rgb_shared(self, r, g, b, iterations=10, target_background=0.25, mask_growth=2.5, mask_softness=4.0,
                                  luminance_protect=True, luminance_ceiling=0.85, protection_amount=0.85,
                                  convergence_threshold=1e-5, outs=None):
        """masked_stretch_rgb_shared (masked_stretch.rs:155-193) -> (res_r, res_g, res_b, shared StarMask scalars).  outs: the three
        stretched planes (allocated like their channels when None)."""
        keep = []
        ps = [self._plane(x, keep) for x in (r, g, b)]
        if outs is None:
            outs = [self._new_like(x, p.rows, p.cols) for x, p in zip((r, g, b), ps)]
        pos = [self._out_plane(o, keep, o.shape[0], o.shape[1]) for o in outs]
        cfg = self._ms_cfg(iterations, target_background, mask_growth, mask_softness, luminance_protect, luminance_ceiling,
                           protection_amount, convergence_threshold)
        res = (_lib.MaskedStretchResultC * 3)()
        shared = _lib.StarMaskInfoC()
        self._check(self._L.ab_masked_stretch_rgb_shared(self._h, *[C.byref(p) for p in ps], C.byref(cfg),
                                                         *[C.byref(p) for p in pos], res, C.byref(shared)))
        return (*[self._ms_result(o, x) for o, x in zip(outs, res)],
                StarMaskResult(None, int(shared.stars_masked), float(shared.coverage_fraction)))

    # ---- core/analysis/deconvolution.rs ----------------------------------------------------------------
    generate_gaussian_psf = staticmethod(generate_gaussian_psf)

    def richardson_lucy(self, image, psf, iterations=20, regularization=0.001, deringing=True, deringing_threshold=0.1, out=None):
        """richardson_lucy (deconvolution.rs:141-221) -> (image, iterations_run, convergence).  image, psf and out: numpy (host)
        or CUDA tensors (device); the result is of the image's kind unless `out` is given."""
        keep = []
        pi = self._plane(image, keep)
        pk = self._plane(psf, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        po = self._out_plane(out, keep, pi.rows, pi.cols)
        cfg = _lib.RLConfigC(int(iterations), float(regularization), 1 if deringing else 0, float(deringing_threshold))
        res = _lib.RLResultC()
        self._check(self._L.ab_richardson_lucy(self._h, C.byref(pi), C.byref(pk), C.byref(cfg), C.byref(po), C.byref(res)))
        return out, int(res.iterations_run), float(res.convergence)

    # ---- core/imaging/psf_estimation.rs --------------------------------------------------------------------
    psf_select_stars = staticmethod(psf_select_stars)

    def estimate_psf(self, image, out=None, **config) -> PsfResult:
        """estimate_psf + psf_to_kernel (psf_estimation.rs:52-149) -> PsfResult.  image: numpy (host) or a CUDA tensor (device); the
        (2 * cutout_radius + 1)^2 f32 kernel is of the image's kind unless `out` is given -- a device kernel goes straight into
        richardson_lucy.  config: PsfEstimationConfig's fields (num_stars, cutout_radius, saturation_threshold, min_peak_fraction,
        max_ellipticity, edge_margin, max_center_distance_fraction); the rest are its defaults.  The reference's three Err returns
        raise AstroBurstError with the reference's string as .message (code AB_ERR_INVALID)."""
        cfg = _psf_config(**config)
        keep = []
        pi = self._plane(image, keep)
        size = 2 * int(cfg.cutout_radius) + 1
        if cfg.cutout_radius <= _lib.AB_PSF_MAX_CUTOUT_RADIUS:   # (beyond it the library answers AB_ERR_UNSUPPORTED before it looks at the plane)
            if out is None:
                out = self._new_like(image, size, size)
            if not _is_torch(out) and (out.dtype != np.float32 or not out.flags.c_contiguous):
                raise AstroBurstError(_lib.AB_ERR_INVALID, "the kernel output must be a contiguous float32 array")
            orows, ocols = (int(out.shape[0]), int(out.shape[1])) if len(out.shape) == 2 else (0, 0)
            po = self._out_plane(out, keep, orows, ocols)
        else:
            po = Plane(None, size, size, 0)
        cap = int(cfg.num_stars) if 0 < cfg.num_stars < (1 << 20) else (1 << 20 if cfg.num_stars else 0)
        stars = (_lib.PsfStarC * max(cap, 1))()
        res = _lib.PsfResultC()
        self._check(self._L.ab_estimate_psf(self._h, C.byref(pi), C.byref(cfg), C.byref(po), stars, cap, C.byref(res)))
        if res.outcome != _lib.AB_PSF_OK:
            raise AstroBurstError(_lib.AB_ERR_INVALID, _lib.PSF_OUTCOME_MESSAGES[res.outcome])
        used = [PsfStar(s.x, s.y, s.peak, s.flux, s.fwhm, s.ellipticity, s.distance_from_center, s.snr)
                for s in stars[:min(int(res.stars_used), cap)]]
        return PsfResult(out, int(res.kernel_size), float(res.average_fwhm), float(res.average_ellipticity), used, int(res.stars_rejected),
                         float(res.spread_pixels), int(res.stars_detected), int(res.stars_filtered))

    # ---- core/imaging/wavelet.rs ---------------------------------------------------------------------------
    wavelet_scale_thresholds = staticmethod(wavelet_scale_thresholds)

    def wavelet_denoise(self, image, num_scales=5, thresholds=(3.0, 2.5, 2.0, 1.5, 1.0), linear_denoise=True, out=None):
        """wavelet_denoise (wavelet.rs:41-133) -> (image, scales_processed, noise_estimate), bit for bit the reference's.  image and
        out: numpy (host) or CUDA tensors (device), CPU tensors accepted; the result is of the image's kind unless `out` is given.
        num_scales is clamped to [1, 8]; the defaults are WaveletConfig::default()."""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        if not _is_torch(out) and (out.shape != (pi.rows, pi.cols) or out.dtype != np.float32 or not out.flags.c_contiguous):
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"output must be a contiguous float32 array of {pi.rows}x{pi.cols}")
        po = self._out_plane(out, keep, pi.rows, pi.cols)
        cfg = _wavelet_config(num_scales, thresholds, linear_denoise, keep)
        res = _lib.WaveletResultC()
        self._check(self._L.ab_wavelet_denoise(self._h, C.byref(pi), C.byref(cfg), C.byref(po), C.byref(res)))
        return out, int(res.scales_processed), float(res.noise_estimate)

    # ---- core/analysis/fft.rs (compute_fft_spectrum) ----------------------------------------------------------
    power_spectrum_dims = staticmethod(power_spectrum_dims)
    hann_symmetric_f32 = staticmethod(hann_symmetric_f32)

    def fft2_forward(self, image, fft_rows, fft_cols, win_y=None, win_x=None, out=None):
        """prepare_windowed_buffer / prepare_buffer_no_window + FftEngine2D::<f32>::forward_2d (math/fft.rs:137-148, :202-245) ->
        complex64 (fft_rows, fft_cols).  image: numpy (host) or a CUDA tensor (device); win_y / win_x: host f32 tables of the image's
        rows / cols, both or neither; the result is of the image's kind unless `out` (complex64, contiguous) is given."""
        keep = []
        pi = self._plane(image, keep)
        if (win_y is None) != (win_x is None):
            raise AstroBurstError(_lib.AB_ERR_INVALID, "win_y and win_x must both be given or both be None")
        wy = wx = None
        if win_y is not None:
            wy = np.ascontiguousarray(win_y, dtype=np.float32)
            wx = np.ascontiguousarray(win_x, dtype=np.float32)
            if wy.shape != (pi.rows,) or wx.shape != (pi.cols,):
                raise AstroBurstError(_lib.AB_ERR_INVALID, f"the windows must hold {pi.rows} and {pi.cols} floats")
        fft_rows, fft_cols = int(fft_rows), int(fft_cols)
        if fft_rows < 1 or fft_cols < 1:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "fft_rows and fft_cols must be powers of two in 1 .. 16384")
        if out is None:
            out = (torch.empty((fft_rows, fft_cols), dtype=torch.complex64, device=image.device) if _is_torch(image) and image.is_cuda
                   else np.empty((fft_rows, fft_cols), np.complex64))
        f32p = C.POINTER(C.c_float)
        if _is_torch(out):
            assert out.is_cuda and out.dtype == torch.complex64 and out.is_contiguous() and tuple(out.shape) == (fft_rows, fft_cols)
            self.use_torch_stream()
            ptr, on_dev = out.data_ptr(), 1
        else:
            assert out.dtype == np.complex64 and out.flags.c_contiguous and out.shape == (fft_rows, fft_cols)
            ptr, on_dev = out.ctypes.data, 0
        self._check(self._L.ab_fft2_forward_f32(self._h, C.byref(pi), wy.ctypes.data_as(f32p) if wy is not None else None,
                                                wx.ctypes.data_as(f32p) if wx is not None else None, fft_rows, fft_cols,
                                                C.c_void_p(ptr), on_dev))
        return out

    def compute_power_spectrum(self, image, apply_window=True, out=None) -> FftResult:
        """compute_power_spectrum_opts (core/analysis/fft.rs:23-68) -> FftResult: the shifted ln(1 + |F|) map of the (Hann-windowed)
        image zero-padded to a power of two, area-averaged down to 1024^2 beyond that.  image: numpy (host) or a CUDA tensor
        (device); the spectrum is of the image's kind unless `out` is given."""
        keep = []
        pi = self._plane(image, keep)
        _, disp = power_spectrum_dims(pi.rows, pi.cols)
        if out is None:
            out = self._new_like(image, disp, disp)
        orows, ocols = (int(out.shape[0]), int(out.shape[1])) if len(out.shape) == 2 else (0, 0)
        if not _is_torch(out) and (out.dtype != np.float32 or not out.flags.c_contiguous):
            raise AstroBurstError(_lib.AB_ERR_INVALID, "the spectrum must be a contiguous float32 array")
        po = self._out_plane(out, keep, orows, ocols)
        res = _lib.FftResultC()
        self._check(self._L.ab_compute_power_spectrum(self._h, C.byref(pi), 1 if apply_window else 0, C.byref(po), C.byref(res)))
        return FftResult(out, int(res.display_rows), int(res.display_cols), int(res.original_size), bool(res.windowed))

    def spectrum_to_u8(self, spectrum, out=None):
        """The per-pixel part of compute_fft_spectrum (cmd/analysis/mod.rs:66-96) -> (u8 image, min, max, dc): the spectrum
        stretched to bytes over its own range, dc = spectrum[rows / 2, cols / 2].  Bytes are of the spectrum's kind."""
        keep = []
        ps = self._plane(spectrum, keep)
        dev = _is_torch(spectrum) and spectrum.is_cuda
        if out is None:
            out = torch.empty((ps.rows, ps.cols), dtype=torch.uint8, device=spectrum.device) if dev else np.empty((ps.rows, ps.cols), np.uint8)
        ptr = out.data_ptr() if _is_torch(out) else out.ctypes.data
        mn, mx, dc = C.c_float(0), C.c_float(0), C.c_float(0)
        self._check(self._L.ab_spectrum_to_u8(self._h, C.byref(ps), C.c_void_p(ptr), 1 if (_is_torch(out) and out.is_cuda) else 0,
                                              C.byref(mn), C.byref(mx), C.byref(dc)))
        return out, mn.value, mx.value, dc.value

    # ---- core/cube/{eager,lazy}.rs (process_cube_cmd, process_cube_lazy_cmd) ---------------------------------------
    cube_streaming_step = staticmethod(cube_streaming_step)

    def _cube(self, cube, keep):
        """ab_cube of a contiguous 3-D float32 numpy array (host) or CUDA tensor (device), [z][y][x]"""
        if _is_torch(cube):
            if not (cube.is_cuda and cube.dtype == torch.float32 and cube.dim() == 3 and cube.is_contiguous()):
                raise AstroBurstError(_lib.AB_ERR_INVALID, "a device cube is a contiguous 3-D float32 CUDA tensor")
            self.use_torch_stream()
            keep.append(cube)
            return _lib.CubeC(C.c_void_p(cube.data_ptr()), cube.shape[0], cube.shape[1], cube.shape[2], 1)
        a = np.ascontiguousarray(cube, dtype=np.float32)
        if a.ndim != 3:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "a cube is 3-D (depth, rows, cols)")
        keep.append(a)
        return _lib.CubeC(C.c_void_p(a.ctypes.data), a.shape[0], a.shape[1], a.shape[2], 0)

    @staticmethod
    def _cube_stats_c(stats):
        if isinstance(stats, GlobalCubeStats):
            stats = (stats.median, stats.sigma, stats.low, stats.high)
        return _lib.CubeStatsC(*[float(np.float32(v)) for v in stats])

    def _collapse(self, fn, cube, rule, out):
        keep = []
        pc = self._cube(cube, keep)
        if out is None:
            out = self._new_like(cube, int(pc.rows), int(pc.cols))
        po = self._out_plane(out, keep, int(out.shape[0]), int(out.shape[1]))
        self._check(fn(self._h, C.byref(pc), int(rule), C.byref(po)))
        return out

    def collapse_mean(self, cube, rule=CUBE_VALID_NONZERO, out=None):
        """collapse_mean (core/cube/eager.rs:24-26 = math/simd.rs:216-253; rule 1: collapse_mean_lazy, lazy.rs:246-284) -> (rows, cols):
        per pixel the f64 sum of the valid samples in ascending z over their count, as f32; bit for bit.  Of the cube's kind."""
        return self._collapse(self._L.ab_cube_collapse_mean, cube, rule, out)

    def collapse_median(self, cube, rule=CUBE_VALID_NONZERO, out=None):
        """collapse_median (eager.rs:28-55; rule 1: collapse_median_lazy, lazy.rs:286-329) -> (rows, cols): element [len / 2] of every
        column's valid samples; bit for bit.  Of the cube's kind."""
        return self._collapse(self._L.ab_cube_collapse_median, cube, rule, out)

    def compute_global_stats(self, cube, rule=CUBE_VALID_NONZERO, frame_step=1, want_count=False):
        """compute_global_stats (eager.rs:168-208) -> GlobalCubeStats over the frames z = 0, frame_step, ...; with want_count also n"""
        keep = []
        pc = self._cube(cube, keep)
        st, n = _lib.CubeStatsC(), C.c_uint64(0)
        self._check(self._L.ab_cube_global_stats(self._h, C.byref(pc), int(rule), int(frame_step), C.byref(st), C.byref(n)))
        g = GlobalCubeStats(st.median, st.sigma, st.low, st.high)
        return (g, int(n.value)) if want_count else g

    def compute_global_stats_streaming(self, cube, want_count=False):
        """compute_global_stats_streaming (lazy.rs:331-370): the lazy path's rule over every cube_streaming_step(depth)-th frame"""
        depth = int(cube.shape[0]) if len(cube.shape) == 3 else 0
        return self.compute_global_stats(cube, CUBE_VALID_ABOVE_PADDING, cube_streaming_step(depth), want_count)

    def normalize_with_global(self, frame, stats, out=None):
        """normalize_with_global (eager.rs:210-222) = normalize_frame_with_stats (lazy.rs:87-99): asinh((10 / sigma) * (clamp(v, low,
        high) - median)), a non-finite pixel -> 0; the f32 rounding of the f64 asinh of the f32 argument.  Of the frame's kind."""
        st = self._cube_stats_c(stats)
        return self._unary(self._L.ab_cube_normalize_frame, frame, out, C.byref(st))

    def export_cube_frames(self, cube, stats, frame_step=1, out=None):
        """The per-pixel work of export_cube_frames_sampled (eager.rs:224-246) / process_cube_lazy's frame loop (lazy.rs:414-420) up to
        the PNG encoder -> uint8 (frame_count, rows, cols): every frame_step-th frame normalised and stretched over its own range.
        Of the cube's kind unless `out` is given."""
        keep = []
        pc = self._cube(cube, keep)
        st = self._cube_stats_c(stats)
        step = max(1, int(frame_step))
        frames = (int(pc.depth) + step - 1) // step
        shape = (frames, int(pc.rows), int(pc.cols))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=cube.device) if _is_torch(cube) else np.empty(shape, np.uint8)
        if _is_torch(out):
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == shape
            ptr, on_dev = out.data_ptr(), 1
        else:
            assert out.dtype == np.uint8 and out.flags.c_contiguous and out.shape == shape
            ptr, on_dev = out.ctypes.data, 0
        count = C.c_int64(0)
        self._check(self._L.ab_cube_export_frames(self._h, C.byref(pc), C.byref(st), step, C.c_void_p(ptr), on_dev, C.byref(count)))
        assert count.value == frames
        return out

    def extract_spectrum(self, cube, y, x, out=None):
        """extract_spectrum (eager.rs:57-60) / extract_spectrum_at (lazy.rs:222-239) -> the depth values at (y, x), of the cube's kind;
        out of bounds raises with the reference's message"""
        keep = []
        pc = self._cube(cube, keep)
        if out is None:
            out = (torch.empty((int(pc.depth),), dtype=torch.float32, device=cube.device) if _is_torch(cube)
                   else np.empty((int(pc.depth),), np.float32))
        if _is_torch(out):
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == pc.depth
            ptr, on_dev = out.data_ptr(), 1
        else:
            assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == pc.depth
            ptr, on_dev = out.ctypes.data, 0
        self._check(self._L.ab_cube_extract_spectrum(self._h, C.byref(pc), int(y), int(x), C.c_void_p(ptr), on_dev))
        return out

    # ---- render_asinh_and_save (cmd/common.rs:242-261), infra/render/grayscale.rs ------------------------------
    @staticmethod
    def _asinh_stats_c(stats):
        if isinstance(stats, AsinhStats):
            stats = (stats.median, stats.sigma, stats.low, stats.high, stats.valid_count)
        return _lib.AsinhStatsC(*[float(np.float32(v)) for v in stats[:4]], int(stats[4]))

    @staticmethod
    def _asinh_stats(st):
        return AsinhStats(st.median, st.sigma, st.low, st.high, int(st.valid_count))

    def _samples_out(self, image, rows, cols, bits, out):
        """(array or tensor, pointer, on_device) of a renderer's output: uint8 (rows, cols), or (rows, cols, 2) big-endian pairs for
        16 bits; of the image's kind unless `out` is given"""
        per = 2 if bits == 16 else 1   # (any other depth is the library's AB_ERR_INVALID)
        shape = (rows, cols, 2) if per == 2 else (rows, cols)
        if out is None:
            dev = _is_torch(image) and image.is_cuda
            out = torch.empty(shape, dtype=torch.uint8, device=image.device) if dev else np.empty(shape, np.uint8)
        if _is_torch(out):
            ok = out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == rows * cols * per
            ptr, on_dev = out.data_ptr(), 1
        else:
            ok = out.dtype == np.uint8 and out.flags.c_contiguous and out.size == rows * cols * per
            ptr, on_dev = out.ctypes.data, 0
        if not ok:
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"the output must be contiguous uint8 of {rows * cols * per} bytes")
        return out, ptr, on_dev

    def asinh_preview_stats(self, image) -> AsinhStats:
        """The statistics of asinh_normalize_simd (math/simd.rs:163-180) over the pixels with is_finite() && v > 1e-7: the f32 median
        (mean of the two middle values for an even count), sigma = max(MAD * 1.4826f32, 1e-10), the 1 % and 99.9 % order statistics;
        bit for bit.  No valid pixel: all zero."""
        keep = []
        pi = self._plane(image, keep)
        st = _lib.AsinhStatsC()
        self._check(self._L.ab_asinh_preview_stats(self._h, C.byref(pi), C.byref(st)))
        return self._asinh_stats(st)

    def asinh_normalize_with_stats(self, image, stats, route=ASINH_ROUTE_AVX2, out=None):
        """The map of asinh_normalize_simd alone (simd.rs:115-158 / :203-211) with the caller's statistics; `out` may be `image`
        itself.  Of the image's kind."""
        st = self._asinh_stats_c(stats)
        return self._unary(self._L.ab_asinh_normalize_with_stats, image, out, C.byref(st), int(route))

    def robust_asinh_preview(self, image, route=ASINH_ROUTE_AVX2, out=None, want_stats=False):
        """robust_asinh_preview = asinh_normalize_simd (math/simd.rs:160-214): the AVX2 route bit for bit, the scalar route bit for
        bit below |x| = 0.5 and the f32 rounding of the f64 log above.  Of the image's kind; with want_stats also the AsinhStats."""
        keep = []
        pi = self._plane(image, keep)
        if out is None:
            out = self._new_like(image, pi.rows, pi.cols)
        po = self._out_plane(out, keep, pi.rows, pi.cols)
        st = _lib.AsinhStatsC()
        self._check(self._L.ab_robust_asinh_preview(self._h, C.byref(pi), int(route), C.byref(po), C.byref(st)))
        return (out, self._asinh_stats(st)) if want_stats else out

    def render_asinh_preview(self, image, route=ASINH_ROUTE_AVX2, out=None, want_stats=False):
        """render_asinh_and_save (cmd/common.rs:242-261) up to the PNG encoder -> uint8 (rows, cols): render_grayscale of the robust
        asinh preview in two launches after the statistics, the f32 preview never written.  Of the image's kind."""
        keep = []
        pi = self._plane(image, keep)
        out, ptr, on_dev = self._samples_out(image, int(pi.rows), int(pi.cols), 8, out)
        st = _lib.AsinhStatsC()
        self._check(self._L.ab_render_asinh_preview(self._h, C.byref(pi), int(route), C.c_void_p(ptr), on_dev, C.byref(st)))
        return (out, self._asinh_stats(st)) if want_stats else out

    def render_grayscale(self, image, bits=8, out=None, want_range=False):
        """render_grayscale / render_grayscale_16bit (infra/render/grayscale.rs:10-50) up to the PNG encoder -> uint8 (rows, cols), or
        (rows, cols, 2) big-endian pairs for bits = 16 (`.view('>u2')`); with want_range also (min, max) of the finite pixels"""
        keep = []
        pi = self._plane(image, keep)
        out, ptr, on_dev = self._samples_out(image, int(pi.rows), int(pi.cols), int(bits), out)
        mn, mx = C.c_float(0), C.c_float(0)
        self._check(self._L.ab_render_grayscale(self._h, C.byref(pi), int(bits), C.c_void_p(ptr), on_dev,
                                                C.byref(mn) if want_range else None, C.byref(mx) if want_range else None))
        return (out, mn.value, mx.value) if want_range else out

    def render_stretched(self, image, bits=8, out=None):
        """render_stretched_8bit / _16bit (grayscale.rs:52-74): (v.clamp(0, 1) * top) as uN, no validity test; bytes as above"""
        keep = []
        pi = self._plane(image, keep)
        out, ptr, on_dev = self._samples_out(image, int(pi.rows), int(pi.cols), int(bits), out)
        self._check(self._L.ab_render_stretched(self._h, C.byref(pi), int(bits), C.c_void_p(ptr), on_dev))
        return out

    # ---- infra/render/rgb.rs, cmd/export/mod.rs, core/compose/drizzle_rgb.rs ------------------------------------
    rgb_packed_bytes = staticmethod(rgb_packed_bytes)

    def _rgb_bytes_out(self, like, rows, cols, pack, out):
        """(array or tensor, pointer, on_device) of an interleaved RGB output: uint8 (rows, cols, 3), or (rows, cols, 6) for
        RGB_PACK_16BE (`.view('>u2')` gives the samples); of `like`'s kind unless `out` is given"""
        per = 6 if pack == RGB_PACK_16BE else 3   # (a packer outside the enum is the library's AB_ERR_INVALID)
        if out is None:
            dev = _is_torch(like) and like.is_cuda
            out = torch.empty((rows, cols, per), dtype=torch.uint8, device=like.device) if dev else np.empty((rows, cols, per), np.uint8)
        if _is_torch(out):
            ok = out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == rows * cols * per
            ptr, on_dev = out.data_ptr(), 1
        else:
            ok = out.dtype == np.uint8 and out.flags.c_contiguous and out.size == rows * cols * per
            ptr, on_dev = out.ctypes.data, 0
        if not ok:
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"the output must be contiguous uint8 of {rows * cols * per} bytes")
        return out, C.c_void_p(ptr), on_dev

    def render_rgb(self, r, g, b, pack=RGB_PACK_8, out=None):
        """render_rgb (rgb.rs:7-47) at full size, render_rgb_16bit (:49-91) or the drizzle packer (drizzle_rgb.rs:232-248) of three
        stretched planes, up to the encoder -> uint8 (rows, cols, 3) or (rows, cols, 6); of r's kind"""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        out, ptr, dev = self._rgb_bytes_out(r, int(pr.rows), int(pr.cols), pack, out)
        self._check(self._L.ab_render_rgb(self._h, C.byref(pr), C.byref(pg), C.byref(pb), int(pack), ptr, dev))
        return out

    def render_rgb_stf(self, r, g, b, stf, stats, pack=RGB_PACK_8, out=None):
        """apply_stf_f32 x 3 and the packer in one launch (export/mod.rs:189-207, :321-328, :362-382); stf, stats: three each"""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        out, ptr, dev = self._rgb_bytes_out(r, int(pr.rows), int(pr.cols), pack, out)
        p, s = self._stf3(stf, stats)
        self._check(self._L.ab_render_rgb_stf(self._h, C.byref(pr), C.byref(pg), C.byref(pb), p, s, int(pack), ptr, dev))
        return out

    def export_rgb(self, r, g, b, bits=16, stf=None, out=None):
        """stretch_and_render (cmd/export/mod.rs:357-409): resample to the largest dims where they differ, statistics per channel, the
        explicit STF (stf = three StfParams) or compute_linked_stf of the three statistics, render_rgb / render_rgb_16bit
        -> (bytes, RgbExportInfo)"""
        keep = []
        planes = [self._plane(x, keep) for x in (r, g, b)]
        rows, cols = max(int(p.rows) for p in planes), max(int(p.cols) for p in planes)
        cfg = _lib.RgbExportConfigC()
        cfg.bits = int(bits)
        if stf is not None:
            cfg.has_stf = 1
            for c, p in enumerate(stf):
                cfg.stf[c] = StfParamsC(p.shadow, p.midtone, p.highlight)
        out, ptr, dev = self._rgb_bytes_out(r, rows, cols, RGB_PACK_16BE if int(bits) == 16 else RGB_PACK_8, out)
        info = _lib.RgbExportInfoC()
        self._check(self._L.ab_export_rgb(self._h, *[C.byref(p) for p in planes], C.byref(cfg), ptr, dev, C.byref(info)))
        return out, RgbExportInfo(int(info.rows), int(info.cols), bool(info.resampled), tuple(self._stats_out(s) for s in info.stats),
                                  tuple(StfParams(p.shadow, p.midtone, p.highlight) for p in info.stf))

    @staticmethod
    def _drizzle_rgb_config(white_balance, auto_stretch, linked_stf, scnr):
        cfg = _lib.DrizzleRgbConfigC()
        if isinstance(white_balance, str):
            cfg.white_balance = {"auto": 0, "none": 2}[white_balance]
        else:
            cfg.white_balance = 1
            cfg.wb_manual[:] = [float(v) for v in white_balance]
        cfg.auto_stretch, cfg.linked_stf = int(bool(auto_stretch)), int(bool(linked_stf))
        if scnr is not None:
            cfg.has_scnr = 1
            m = scnr.get("method", "average")
            cfg.scnr = _lib.ScnrConfigC(0 if m in ("average", "AverageNeutral", 0) else 1, scnr.get("amount", 1.0),
                                        int(bool(scnr.get("preserve_luminance", False))))
        return cfg

    def _plane3(self, like, rows, cols, keep):
        """three new planes of `like`'s kind and their ab_plane_mut[3]"""
        arrs = tuple(self._new_like(like, rows, cols) for _ in range(3))
        return arrs, (Plane * 3)(*[self._out_plane(a, keep, rows, cols) for a in arrs])

    def _processed_drizzle_rgb(self, stretched, wb, rgb8, info):
        return ProcessedDrizzleRgb(stretched, wb, rgb8, int(info.rows), int(info.cols), tuple(info.wb),
                                   tuple(StfParams(p.shadow, p.midtone, p.highlight) for p in info.stf), tuple(tuple(row) for row in info.chan_stats),
                                   tuple(self._stats_out(s) for s in info.stats_wb), bool(info.scnr_applied))

    def process_drizzle_rgb(self, r, g, b, white_balance="auto", auto_stretch=True, linked_stf=False, scnr=None, want_stretched=True,
                            want_wb=True, want_rgb8=True) -> ProcessedDrizzleRgb:
        """process_drizzle_rgb (drizzle_rgb.rs:41-145) and the packer of drizzle_rgb (:232-248).  Absent channels are None; the output
        has the minimum rows and cols of the present ones.  white_balance: "auto" | "none" | (r, g, b); scnr: None or
        dict(method=, amount=, preserve_luminance=).  Outputs are of the first present channel's kind."""
        keep = []
        chans = [None if x is None else self._plane(x, keep) for x in (r, g, b)]
        present = [p for p in chans if p is not None]
        first = next((x for x in (r, g, b) if x is not None), None)
        if first is None:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "at least one channel must be present")
        rows, cols = min(int(p.rows) for p in present), min(int(p.cols) for p in present)
        cfg = self._drizzle_rgb_config(white_balance, auto_stretch, linked_stf, scnr)
        stretched, ps = self._plane3(first, rows, cols, keep) if want_stretched else (None, None)
        wb, pw = self._plane3(first, rows, cols, keep) if want_wb else (None, None)
        rgb8, ptr, dev = self._rgb_bytes_out(first, rows, cols, RGB_PACK_8_ROUND, None) if want_rgb8 else (None, None, 0)
        info = _lib.ProcessedDrizzleRgbInfoC()
        self._check(self._L.ab_process_drizzle_rgb(self._h, *[None if p is None else C.byref(p) for p in chans], C.byref(cfg), ps, pw, ptr, dev,
                                                   C.byref(info)))
        return self._processed_drizzle_rgb(stretched, wb, rgb8, info)

    def drizzle_rgb(self, r_frames, g_frames, b_frames, scale=2.0, pixfrac=0.7, kernel="square", sigma_low=3.0, sigma_high=3.0,
                    sigma_iterations=5, align=True, alignment_method="phase_correlation", num_threads=8, white_balance="auto", auto_stretch=True,
                    linked_stf=False, scnr=None, want_wb=True, want_rgb8=True) -> DrizzleRgbResult:
        """drizzle_rgb (drizzle_rgb.rs:159-286) up to the PNG / FITS writers: each list of frames (None: no such channel; fewer than two
        frames: treated as absent) is drizzled into an image that stays on the device, then process_drizzle_rgb."""
        lists = [r_frames, g_frames, b_frames]
        given = sum(f is not None for f in lists)
        if given < 2:
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"Need at least 2 channels for RGB drizzle (got {given})")
        dcfg = _drizzle_config(scale, pixfrac, kernel, sigma_low, sigma_high, sigma_iterations, align, alignment_method, num_threads)
        keep, arrays, counts, dims, first = [], [], [], [], None
        for frames in lists:
            if frames is None:
                arrays.append(None), counts.append(0)
                continue
            arrays.append(self._planes(frames, keep)), counts.append(len(frames))
            if len(frames) >= 2:
                first = frames[0] if first is None else first
                d = [C.c_int64(0) for _ in range(4)]
                self._check_noctx(self._L.ab_drizzle_output_dims(arrays[-1], len(frames), C.byref(dcfg), *[C.byref(x) for x in d]), len(frames))
                dims.append((int(d[2].value), int(d[3].value)))
        if first is None:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "All channels failed or have fewer than 2 frames")
        rows, cols = min(d[0] for d in dims), min(d[1] for d in dims)
        cfg = self._drizzle_rgb_config(white_balance, auto_stretch, linked_stf, scnr)
        wb, pw = self._plane3(first, rows, cols, keep) if want_wb else (None, None)
        rgb8, ptr, dev = self._rgb_bytes_out(first, rows, cols, RGB_PACK_8_ROUND, None) if want_rgb8 else (None, None, 0)
        res = (_lib.DrizzleResultC * 3)()
        info = _lib.ProcessedDrizzleRgbInfoC()
        self._check(self._L.ab_drizzle_rgb(self._h, arrays[0], counts[0], arrays[1], counts[1], arrays[2], counts[2], C.byref(dcfg), C.byref(cfg), pw, ptr,
                                           dev, res, C.byref(info)))
        chans = tuple(None if x.frame_count == 0 else (int(x.frame_count), float(x.output_scale), (int(x.in_rows), int(x.in_cols)),
                                                       (int(x.out_rows), int(x.out_cols)), int(x.rejected_pixels)) for x in res)
        return DrizzleRgbResult(self._processed_drizzle_rgb(None, wb, rgb8, info), chans)

    # ---- cmd/processing/curves.rs: the compose wizard's tone editor ---------------------------------------------
    tone_plan = staticmethod(tone_plan)

    def apply_tone_composite(self, r, g, b, stats, stf=None, linked_stf=False, levels=None, curves=None, scnr=None, max_dim=4096,
                             want_planes=False, want_rgb8=True, out=None) -> ToneResult:
        """apply_tone_composite_cmd (cmd/processing/curves.rs:57-191) from its loaded channels to the encoder's input, fused: STF,
        levels, curves, SCNR and the preview's pick and pack in one launch (two with want_planes on an image above max_dim).
        stats: the three channels' ImageStats; stf, levels, curves, scnr: as tone_plan takes them.  want_planes: the three toned
        f32 planes of full size as well.  out: the caller's byte buffer (contiguous uint8 of preview_rows * preview_cols * 3, any
        address).  Outputs are of r's kind: numpy in -> numpy out, CUDA tensors in -> CUDA tensors out."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        cfg = _tone_config(stf, linked_stf, levels, curves, scnr, keep)
        st = (_lib.ImageStatsC * 3)(*[self._stats_in(s) for s in stats])
        planes, pp = self._plane3(r, rows, cols, keep) if want_planes else (None, None)
        rgb8, ptr, dev = None, None, 0
        if want_rgb8 or out is not None:
            ph, pw = self.preview_dims(rows, cols, max_dim) if max_dim > 0 else (1, 1)   # (max_dim < 1 is the library's AB_ERR_INVALID)
            rgb8, ptr, dev = self._bytes_out(r, (ph, pw, 3), out)
        info = _lib.ToneInfoC()
        self._check(self._L.ab_apply_tone_composite(self._h, C.byref(pr), C.byref(pg), C.byref(pb), st, C.byref(cfg), int(max_dim), pp, ptr, dev,
                                                    C.byref(info)))
        return ToneResult(planes, rgb8, _tone_info(info))

    # ---- the RGB Compose panel: cmd/compose/rgb.rs ----------------------------------------------------------------------
    def compose_rgb(self, l, r, g, b, white_balance="auto", auto_stretch=True, stf=(None, None, None), linked_stf=False, align=True,
                    align_method="phase_correlation", scnr=None, num_threads=8, lrgb_lightness=1.0, lrgb_chrominance=1.0, max_dim=4096,
                    want_planes=False, want_rgb8=True, fetch=True, out_pre=None, out_planes=None, out=None) -> ComposeRgbResult:
        """compose_rgb_cmd (cmd/compose/rgb.rs:43-205) from its loaded entries to the PNG encoder's input and the JSON, as one chain:
        process_rgb, L's resample / auto-STF / stretch, apply_lrgb and render_rgb_preview.  l and up to one of r, g, b may be None.
        The keyword arguments up to num_threads are process_rgb's.  Numpy in, numpy out; CUDA tensors in, CUDA tensors out.
        out_pre / out_planes: three planes of the composite's dims each; out: contiguous uint8 of preview_rows * preview_cols * 3,
        any address.  fetch=False (info NULL) leaves only the white-balance synchronisation, and none for "none" / manual."""
        keep = []
        chans = [None if x is None else self._plane(x, keep) for x in (r, g, b)]
        pl = None if l is None else self._plane(l, keep)
        present = [p for p in chans if p is not None]
        first = next((x for x in (r, g, b, l) if x is not None), None)
        if first is None:
            first = np.empty((0, 0), np.float32)
        rows = max((int(p.rows) for p in present), default=0)
        cols = max((int(p.cols) for p in present), default=0)
        cfg = self._rgb_compose_config(white_balance, auto_stretch, stf, linked_stf, align, align_method, scnr, num_threads)
        if out_pre is None:
            out_pre = tuple(self._new_like(first, rows, cols) for _ in range(3))
        ppre = (Plane * 3)(*[self._out_plane(a, keep, a.shape[0], a.shape[1]) for a in out_pre])   # (their own dims: the library refuses a mismatch)
        pout = None
        if want_planes or out_planes is not None:
            if out_planes is None:
                out_planes = tuple(self._new_like(first, rows, cols) for _ in range(3))
            pout = (Plane * 3)(*[self._out_plane(a, keep, a.shape[0], a.shape[1]) for a in out_planes])
        rgb8, ptr, dev = None, None, int(_is_torch(first) and first.is_cuda)
        ph, pw = self.preview_dims(rows, cols, int(max_dim)) if (max_dim >= 1 and rows >= 1 and cols >= 1) else (1, 1)
        if want_rgb8 or out is not None:
            rgb8, ptr, dev = self._bytes_out(first, (ph, pw, 3), out)
        info = _lib.ComposeRgbInfoC()
        self._check(self._L.ab_compose_rgb(self._h, None if pl is None else C.byref(pl), *[None if p is None else C.byref(p) for p in chans],
                                           C.byref(cfg), float(lrgb_lightness), float(lrgb_chrominance), int(max_dim), ppre, pout, ptr, dev,
                                           C.byref(info) if fetch else None))
        if not fetch:
            return ComposeRgbResult(tuple(out_pre), None if pout is None else tuple(out_planes), rgb8, rows, cols, ph, pw, *([None] * 11))
        pi = info.rgb
        has_l_stats = pl is not None and bool(auto_stretch)
        return ComposeRgbResult(tuple(out_pre), None if pout is None else tuple(out_planes), rgb8, int(pi.rows), int(pi.cols),
                                int(info.preview_rows), int(info.preview_cols), tuple(StfParams(p.shadow, p.midtone, p.highlight) for p in pi.stf),
                                tuple(tuple(row) for row in pi.chan_stats), tuple(pi.offset_g), tuple(pi.offset_b), bool(pi.scnr_applied),
                                bool(pi.resampled), tuple(self._stats_out(s) for s in pi.stats_wb), bool(info.lrgb_applied), bool(info.l_resampled),
                                self._stats_out(info.l_stats) if has_l_stats else None,
                                StfParams(info.l_stf.shadow, info.l_stf.midtone, info.l_stf.highlight) if has_l_stats else None)

    def restretch_composite(self, r, g, b, stats, stf, scnr=None, max_dim=4096, want_planes=False, want_rgb8=True, out=None):
        """restretch_composite_cmd (cmd/compose/rgb.rs:208-241), the STF slider loop of the RGB Compose panel, on the tone editor's
        kernel: the three explicit StfParams (or (shadow, midtone, highlight)) normalised with the cached ImageStats, SCNR whenever
        scnr is not None (apply_scnr_inplace's own threshold decides), the preview's pick and pack.  -> (planes | None, rgb8 | None)."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        st = (_lib.ImageStatsC * 3)(*[self._stats_in(s) for s in stats])
        sp = (StfParamsC * 3)(*[StfParamsC(*(p if isinstance(p, (tuple, list)) else (p.shadow, p.midtone, p.highlight))) for p in stf])
        sc = None
        if scnr is not None:
            m = scnr.get("method", "average")
            sc = _lib.ScnrConfigC(0 if m in ("average", "AverageNeutral", 0) else 1, scnr.get("amount", 1.0), int(bool(scnr.get("preserve_luminance", False))))
        planes, pp = self._plane3(r, rows, cols, keep) if want_planes else (None, None)
        rgb8, ptr, dev = None, None, 0
        if want_rgb8 or out is not None:
            ph, pw = self.preview_dims(rows, cols, max_dim) if max_dim > 0 else (1, 1)   # (max_dim < 1 is the library's AB_ERR_INVALID)
            rgb8, ptr, dev = self._bytes_out(r, (ph, pw, 3), out)
        self._check(self._L.ab_restretch_composite(self._h, C.byref(pr), C.byref(pg), C.byref(pb), st, sp, int(sc is not None),
                                                   None if sc is None else C.byref(sc), int(max_dim), pp, ptr, dev))
        return planes, rgb8

    # ---- cmd/io/mod.rs: opening a file (process_fits, process_fits_full, process_rgb_fits) and the histogram panel ------------
    downsample_histogram = staticmethod(downsample_histogram)
    histogram_bin_edges = staticmethod(histogram_bin_edges)

    def _bins_out(self, like, n, out=None):
        """the display bins next to the input: an int32 CUDA tensor for device planes (torch has no arithmetic on uint32; a count is
        below 2^31, so the words are the same), a uint32 numpy array for host planes -> (array, ptr, on_device); or the caller's"""
        if out is not None:
            if _is_torch(out):
                ok = out.is_cuda and out.dtype in (torch.int32, torch.uint32) and out.is_contiguous() and out.numel() >= n
                return self._bins_ok(ok, n), out, C.c_void_p(out.data_ptr()), 1
            ok = isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.flags.c_contiguous and out.size >= n
            return self._bins_ok(ok, n), out, C.c_void_p(out.ctypes.data if ok else 0), 0
        if _is_torch(like) and like.is_cuda:
            out = torch.empty((n,), dtype=torch.int32, device=like.device)
            return None, out, C.c_void_p(out.data_ptr()), 1
        out = np.zeros(n, np.uint32)
        return None, out, C.c_void_p(out.ctypes.data), 0

    @staticmethod
    def _bins_ok(ok, n):
        if not ok:
            raise AstroBurstError(_lib.AB_ERR_INVALID, f"the bin output must be contiguous, 32-bit and hold {n} words")

    def display_histogram(self, image, dmin: float, dmax: float, target_bins: int = 512, out=None):
        """downsample_histogram(compute_histogram_with_stats(image, {min, max}), target_bins) (stats.rs:373-376, :423-444) in one pass
        -> min(target_bins, 65536) bins: uint32 numpy for a host plane, int32 CUDA (asynchronous) for a device plane, or `out`."""
        keep = []
        pi = self._plane(image, keep)
        n = max(1, min(int(target_bins), HISTOGRAM_BINS))
        _, bins, ptr, dev = self._bins_out(image, n, out)
        got = C.c_size_t(0)
        self._check(self._L.ab_display_histogram(self._h, C.byref(pi), float(dmin), float(dmax), int(target_bins), ptr, dev, C.byref(got)))
        return bins[:got.value]

    @staticmethod
    def _view_config(hist_bins, target_bg, shadow_k):
        cfg = _lib.FitsViewConfigC()
        _lib.lib().ab_fits_view_config_default(C.byref(cfg))
        cfg.hist_bins = int(hist_bins)
        if target_bg is not None:
            cfg.stf.target_bg = float(target_bg)
        if shadow_k is not None:
            cfg.stf.shadow_k = float(shadow_k)
        return cfg

    def process_fits_view(self, image, hist_bins: int = 512, target_bg=None, shadow_k=None, fetch=True, out=None, out_bins=None) -> FitsView:
        """The mono branch of process_fits_full (cmd/io/mod.rs:138-144) as one chain: compute_image_stats -> auto_stf -> apply_stf and
        the display histogram in the same pass.  hist_bins=0: process_fits, no histogram.  fetch=False with device outputs keeps the
        call asynchronous (stats and stf are then None).  Outputs are of the image's kind unless `out` / `out_bins` are given."""
        keep = []
        pi = self._plane(image, keep)
        rows, cols = int(pi.rows), int(pi.cols)
        cfg = self._view_config(hist_bins, target_bg, shadow_k)
        u8, ptr, dev = self._bytes_out(image, (rows, cols), out)
        nb = min(int(hist_bins), HISTOGRAM_BINS)
        _, bins, bptr, bdev = self._bins_out(image, nb, out_bins) if nb > 0 else (None, None, None, 0)
        info = _lib.FitsViewInfoC()
        self._check(self._L.ab_process_fits_view(self._h, C.byref(pi), C.byref(cfg), ptr, dev, bptr, bdev, C.byref(info) if fetch else None))
        if bins is not None:
            bins = bins[:nb]
        if not fetch:
            return FitsView(u8, bins, rows, cols, None, None)
        return FitsView(u8, bins, int(info.rows), int(info.cols), self._stats_out(info.stats),
                        StfParams(info.stf.shadow, info.stf.midtone, info.stf.highlight))

    def process_rgb_fits_view(self, r, g, b, hist_bins: int = 512, max_dim: int = 4096, target_bg=None, shadow_k=None, fetch=True, want_rgb8=True,
                              out=None, out_bins=None) -> RgbFitsView:
        """process_rgb_fits from its three planes on (cmd/io/mod.rs:44-62) as one chain: statistics and auto_stf per channel (unlinked),
        apply_stf_f32 and render_rgb_preview(.., max_dim) fused into one packer, the display histogram of R riding in it.  fetch=False
        with device outputs keeps the call asynchronous."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        cfg = self._view_config(hist_bins, target_bg, shadow_k)
        ph, pw = self.preview_dims(rows, cols, max_dim) if max_dim > 0 else (1, 1)   # (max_dim < 1 is the library's AB_ERR_INVALID)
        rgb8, ptr, dev = self._bytes_out(r, (ph, pw, 3), out) if (want_rgb8 or out is not None) else (None, None, 0)
        nb = min(int(hist_bins), HISTOGRAM_BINS)
        _, bins, bptr, bdev = self._bins_out(r, nb, out_bins) if nb > 0 else (None, None, None, 0)
        info = _lib.RgbFitsViewInfoC()
        self._check(self._L.ab_process_rgb_fits_view(self._h, C.byref(pr), C.byref(pg), C.byref(pb), C.byref(cfg), int(max_dim), ptr, dev, bptr, bdev,
                                                     C.byref(info) if fetch else None))
        if bins is not None:
            bins = bins[:nb]
        if not fetch:
            return RgbFitsView(rgb8, bins, rows, cols, ph, pw, None, None)
        return RgbFitsView(rgb8, bins, int(info.rows), int(info.cols), int(info.preview_rows), int(info.preview_cols),
                           tuple(self._stats_out(s) for s in info.stats), tuple(StfParams(p.shadow, p.midtone, p.highlight) for p in info.stf))

    # ---- cmd/compose/blend.rs and cmd/compose/color.rs: the wizard's blend and colour steps ---------------------------------
    color_step_plan = staticmethod(color_step_plan)
    compute_auto_wb = staticmethod(compute_auto_wb)

    def _composite_outputs(self, like, rows, cols, max_dim, want_rgb8, out, out_planes, keep):
        """the three f32 planes and the preview's bytes of a wizard step: the caller's (out_planes: three arrays or CUDA tensors of
        rows x cols; out: contiguous uint8 of preview_rows * preview_cols * 3, any address) or new ones of `like`'s kind"""
        if out_planes is None:
            planes, pp = self._plane3(like, rows, cols, keep)
        else:
            planes = tuple(out_planes)
            ok = len(planes) == 3 and all(tuple(p.shape) == (rows, cols) and (_is_torch(p) or (isinstance(p, np.ndarray) and p.dtype == np.float32
                                                                                              and p.flags.c_contiguous)) for p in planes)
            if not ok:
                raise AstroBurstError(_lib.AB_ERR_INVALID, f"out_planes must be three contiguous float32 planes of {rows} x {cols}")
            pp = (Plane * 3)(*[self._out_plane(a, keep, rows, cols) for a in planes])
        ph, pw = self.preview_dims(rows, cols, max_dim) if max_dim > 0 else (1, 1)   # (max_dim < 1 is the library's AB_ERR_INVALID)
        rgb8, ptr, dev = self._bytes_out(like, (ph, pw, 3), out) if (want_rgb8 or out is not None) else (None, None, 0)
        return planes, pp, rgb8, ptr, dev, ph, pw

    def calibrate_and_scnr(self, r, g, b, orig_stats, factors, scnr=None, max_dim=4096, fetch=True, want_rgb8=True, out=None,
                           out_planes=None) -> ColorStepResult:
        """calibrate_and_scnr_cmd (cmd/compose/color.rs:97-184) from its loaded originals to the encoder's input as one chain: white
        balance and SCNR in one kernel, three statistics chains by color_step_plan's routes, the linked STF on the device and the
        preview, one synchronisation.  orig_stats: the originals' ImageStats; factors: (r, g, b) as the command receives them; scnr:
        None or dict(method=, amount=, preserve_luminance=).  fetch=False with device outputs keeps the call asynchronous (the
        scalars are then None).  Outputs are of r's kind unless out / out_planes are given."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        planes, pp, rgb8, ptr, dev, ph, pw = self._composite_outputs(r, rows, cols, max_dim, want_rgb8, out, out_planes, keep)
        has, cfg = _scnr_config(scnr)
        f = (C.c_double * 3)(*[float(v) for v in factors])
        info = _lib.ColorStepInfoC()
        self._check(self._L.ab_calibrate_and_scnr(self._h, C.byref(pr), C.byref(pg), C.byref(pb), _stats3(orig_stats), f, has,
                                                  C.byref(cfg) if cfg is not None else None, int(max_dim), pp, ptr, dev, C.byref(info) if fetch else None))
        if not fetch:
            return ColorStepResult(planes, rgb8, rows, cols, ph, pw, None, None, None, None, None)
        return ColorStepResult(planes, rgb8, int(info.rows), int(info.cols), int(info.preview_rows), int(info.preview_cols),
                               tuple(float(v) for v in info.factors), bool(info.scnr_applied), tuple(int(v) for v in info.route),
                               tuple(self._stats_out(s) for s in info.stats), StfParams(info.stf.shadow, info.stf.midtone, info.stf.highlight))

    def blend_composite(self, channels, weights, max_dim=4096, fetch=True, want_rgb8=True, out=None, out_planes=None) -> BlendCompositeResult:
        """blend_channels_cmd (cmd/compose/blend.rs:128-223) from its loaded channels on as one chain: channels of differing dims are
        resampled (bicubic) to the largest rows and the largest cols, blend_channels, three statistics chains, the linked STF on the
        device and the preview, one synchronisation.  weights: iterable of (channel_idx, r_weight, g_weight, b_weight).  Outputs are
        of the first channel's kind unless out / out_planes are given."""
        if len(channels) == 0:   # (the library's own error: no plane is there to take the output's kind from)
            self._check(self._L.ab_blend_composite(self._h, None, 0, None, 0, int(max_dim), None, None, 0, None))
        keep = []
        chans = (Plane * len(channels))(*[self._plane(c, keep) for c in channels])
        rows, cols = max(int(p.rows) for p in chans), max(int(p.cols) for p in chans)
        ws = (_lib.BlendWeightC * max(1, len(weights)))(*[_lib.BlendWeightC(int(w[0]), w[1], w[2], w[3]) for w in weights])
        planes, pp, rgb8, ptr, dev, ph, pw = self._composite_outputs(channels[0], rows, cols, max_dim, want_rgb8, out, out_planes, keep)
        info = _lib.BlendCompositeInfoC()
        self._check(self._L.ab_blend_composite(self._h, chans, len(channels), ws, len(weights), int(max_dim), pp, ptr, dev,
                                               C.byref(info) if fetch else None))
        if not fetch:
            return BlendCompositeResult(planes, rgb8, rows, cols, ph, pw, None, None, None)
        return BlendCompositeResult(planes, rgb8, int(info.rows), int(info.cols), int(info.preview_rows), int(info.preview_cols),
                                    bool(info.resampled), tuple(self._stats_out(s) for s in info.stats),
                                    StfParams(info.stf.shadow, info.stf.midtone, info.stf.highlight))

    # ---- cmd/processing/stretch.rs: the wizard's stretch step ------------------------------------------------------------------
    arcsinh_rgb_range = staticmethod(arcsinh_rgb_range)

    def _stretch_outputs(self, like, rows, cols, max_dim, want_planes, want_rgb8, out, out_planes, keep):
        """_composite_outputs with optional planes: (None, None, ...) when neither want_planes nor out_planes asks for them"""
        if want_planes or out_planes is not None:
            return self._composite_outputs(like, rows, cols, max_dim, want_rgb8, out, out_planes, keep)
        ph, pw = self.preview_dims(rows, cols, max_dim) if max_dim > 0 else (1, 1)
        rgb8, ptr, dev = self._bytes_out(like, (ph, pw, 3), out) if (want_rgb8 or out is not None) else (None, None, 0)
        return None, None, rgb8, ptr, dev, ph, pw

    @staticmethod
    def _range_args(global_range):
        if global_range is None:
            return None, None
        return C.byref(C.c_float(global_range[0])), C.byref(C.c_float(global_range[1]))

    def arcsinh_stretch_rgb(self, r, g, b, factor, gamma=1.0, global_range=None, fetch=True, out_planes=None):
        """arcsinh_stretch_rgb_with_stats (core/imaging/stretch.rs:56-90): one streaming pass for the global range (skipped with
        global_range=(min, max)), one kernel for the three planes.  -> ((r, g, b), (global_min, global_max) | None)."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        planes, pp, _, _, _, _, _ = self._composite_outputs(r, rows, cols, 1, False, None, out_planes, keep)
        mn, mx = self._range_args(global_range)
        mm = (C.c_float * 2)()
        self._check(self._L.ab_arcsinh_stretch_rgb(self._h, C.byref(pr), C.byref(pg), C.byref(pb), mn, mx, C.c_float(factor), C.c_float(gamma), pp,
                                                   mm if fetch else None))
        return planes, ((float(mm[0]), float(mm[1])) if fetch else None)

    def arcsinh_stretch_composite(self, r, g, b, factor, max_dim=4096, global_range=None, fetch=True, want_planes=False, want_rgb8=True, out=None,
                                  out_planes=None) -> ArcsinhCompositeResult:
        """arcsinh_stretch_composite_cmd (cmd/processing/stretch.rs:94-124) from the loaded composite to the encoder's input: the range
        pass, then the stretch and the truncating packer in registers; above max_dim without planes only the picked pixels are
        stretched.  fetch=False with device outputs keeps the call asynchronous (the scalars are then None)."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        planes, pp, rgb8, ptr, dev, ph, pw = self._stretch_outputs(r, rows, cols, max_dim, want_planes, want_rgb8, out, out_planes, keep)
        mn, mx = self._range_args(global_range)
        info = _lib.ArcsinhCompositeInfoC()
        self._check(self._L.ab_arcsinh_stretch_composite(self._h, C.byref(pr), C.byref(pg), C.byref(pb), float(factor), mn, mx, int(max_dim), pp, ptr, dev,
                                                         C.byref(info) if fetch else None))
        if not fetch:
            return ArcsinhCompositeResult(planes, rgb8, rows, cols, ph, pw, None, None, None, None)
        return ArcsinhCompositeResult(planes, rgb8, int(info.rows), int(info.cols), int(info.preview_rows), int(info.preview_cols), float(info.factor),
                                      float(info.global_min), float(info.global_max), bool(info.degenerate))

    def arcsinh_stretch_view(self, image, factor, fetch=True, want_u8=True, out=None, out_plane=None) -> ArcsinhViewResult:
        """apply_arcsinh_stretch_cmd (stretch.rs:15-43) with render_and_save's preview as one chain: the range pass, the stretch, the
        statistics and the STF of the stretched plane, one synchronisation."""
        keep = []
        pi = self._plane(image, keep)
        rows, cols = int(pi.rows), int(pi.cols)
        if out_plane is None:
            out_plane = self._new_like(image, rows, cols)
        po = self._out_plane(out_plane, keep, out_plane.shape[0], out_plane.shape[1])   # (its own dims: the library refuses a mismatch)
        u8, ptr, dev = self._bytes_out(image, (rows, cols), out) if (want_u8 or out is not None) else (None, None, 0)
        info = _lib.ArcsinhViewInfoC()
        self._check(self._L.ab_arcsinh_stretch_view(self._h, C.byref(pi), float(factor), C.byref(po), ptr, dev, C.byref(info) if fetch else None))
        if not fetch:
            return ArcsinhViewResult(out_plane, u8, rows, cols, None, None, None, None, None, None)
        return ArcsinhViewResult(out_plane, u8, int(info.rows), int(info.cols), float(info.factor), float(info.data_min), float(info.data_max),
                                 bool(info.degenerate), self._stats_out(info.stats), StfParams(info.stf.shadow, info.stf.midtone, info.stf.highlight))

    def masked_stretch_composite(self, r, g, b, shared_mask=False, max_dim=4096, iterations=10, target_background=0.25, mask_growth=2.5,
                                 mask_softness=4.0, luminance_protect=True, luminance_ceiling=0.85, protection_amount=0.85, convergence_threshold=1e-5,
                                 fetch=True, want_planes=False, want_rgb8=True, out=None, out_planes=None) -> MaskedStretchCompositeResult:
        """masked_stretch_composite_cmd (stretch.rs:135-221): masked_stretch_rgb_shared (shared_mask) or masked_stretch x 3, then the
        truncating packer; without planes the stretched channels stay in a workspace of the context."""
        keep = []
        pr, pg, pb = (self._plane(x, keep) for x in (r, g, b))
        rows, cols = int(pr.rows), int(pr.cols)
        planes, pp, rgb8, ptr, dev, ph, pw = self._stretch_outputs(r, rows, cols, max_dim, want_planes, want_rgb8, out, out_planes, keep)
        cfg = self._ms_cfg(iterations, target_background, mask_growth, mask_softness, luminance_protect, luminance_ceiling, protection_amount,
                           convergence_threshold)
        info = _lib.MaskedStretchCompositeInfoC()
        self._check(self._L.ab_masked_stretch_composite(self._h, C.byref(pr), C.byref(pg), C.byref(pb), C.byref(cfg), int(bool(shared_mask)), int(max_dim),
                                                        pp, ptr, dev, C.byref(info) if fetch else None))
        if not fetch:
            return MaskedStretchCompositeResult(planes, rgb8, rows, cols, ph, pw, None, None, None, None)
        return MaskedStretchCompositeResult(planes, rgb8, int(info.rows), int(info.cols), int(info.preview_rows), int(info.preview_cols),
                                            tuple(self._ms_result(None, x) for x in info.channels), int(info.stars_masked), float(info.mask_coverage),
                                            "shared_luminance" if info.mask_mode == MASK_SHARED_LUMINANCE else "per_channel")

    # ---- cmd/compose/crop.rs ---------------------------------------------------------------------------------
    @staticmethod
    def _box_out(b) -> CropBox:
        return CropBox(int(b.top), int(b.bottom), int(b.left), int(b.right))

    def detect_valid_region(self, image, threshold: float = CROP_AUTO_THRESHOLD) -> CropBox:
        """detect_valid_region(arr, threshold) (crop.rs:14-62): (top, bottom, left, right) of the pixels with |v| > threshold;
        (rows, 0, cols, 0) when there is none."""
        keep = []
        pi = self._plane(image, keep)
        box = _lib.CropBoxC()
        self._check(self._L.ab_detect_valid_region(self._h, C.byref(pi), float(threshold), C.byref(box)))
        return self._box_out(box)

    def detect_valid_regions(self, images, threshold: float = CROP_AUTO_THRESHOLD, want_each=True, want_common=True):
        """The loop crop.rs:109-116 over planes of any dims, one launch chain -> (each plane's CropBox or None, the running
        (max top, min bottom, max left, min right) or None)."""
        keep = []
        arr, n = self._plane_array(images, keep)
        each = (_lib.CropBoxC * max(n, 1))() if want_each else None
        common = _lib.CropBoxC() if want_common else None
        self._check(self._L.ab_detect_valid_regions(self._h, arr, n, float(threshold), each, C.byref(common) if want_common else None))
        return ([self._box_out(each[i]) for i in range(n)] if want_each else None), (self._box_out(common) if want_common else None)

    def crop_array(self, image, box, out=None):
        """crop_array(arr, top, bottom, left, right) (crop.rs:64-71): the dense copy of the box, clamped to the plane as the reference
        clamps it.  out: a plane of the clamped window's dims (allocated like the input when None)."""
        keep = []
        pi = self._plane(image, keep)
        box = CropBox(*(int(v) for v in box))
        w = box.clamped(int(pi.rows), int(pi.cols))
        if out is None:
            out = self._new_like(image, w.bottom - w.top, w.right - w.left)
        po = self._out_plane(out, keep, out.shape[0], out.shape[1])
        self._check(self._L.ab_crop_array(self._h, C.byref(pi), C.byref(_lib.CropBoxC(*box)), C.byref(po)))
        return out

    def crop_channels_plan(self, images, auto_detect=True, top=0, bottom=0, left=0, right=0, threshold=None) -> CropPlan:
        """crop.rs:92-126: the box of crop_channels_cmd.  auto_detect: the intersection of the planes' valid regions (raises "Auto-crop
        found no valid overlapping region"); else top / bottom / left / right are margins taken off plane 0's dims."""
        keep = []
        arr, n = self._plane_array(images, keep)
        cfg = _lib.CropConfigC()
        self._L.ab_crop_config_default(C.byref(cfg))
        cfg.auto_detect = 1 if auto_detect else 0
        cfg.top, cfg.bottom, cfg.left, cfg.right = int(top), int(bottom), int(left), int(right)
        if threshold is not None:
            cfg.threshold = float(threshold)
        plan = _lib.CropPlanC()
        dims = (C.c_uint64 * (2 * max(n, 1)))()
        self._check(self._L.ab_crop_channels_plan(self._h, arr, n, C.byref(cfg), C.byref(plan), dims))
        return CropPlan(self._box_out(plan.crop_box), int(plan.out_rows), int(plan.out_cols), int(plan.actual_top), int(plan.actual_bottom),
                        int(plan.actual_left), int(plan.actual_right), bool(plan.auto_detected),
                        tuple((int(dims[2 * i]), int(dims[2 * i + 1])) for i in range(n)))

    def crop_channels(self, images, plan: CropPlan, want_stats=True, outs=None):
        """crop.rs:133-168 without the files and the cache: every plane cropped to plan.crop_box (one launch) -> (the cropped planes, each
        allocated like its input, and their ImageStats or None).  want_stats=False keeps the call asynchronous for device planes."""
        keep = []
        arr, n = self._plane_array(images, keep)
        if outs is None:
            outs = []
            for i in range(n):
                w = plan.crop_box.clamped(int(arr[i].rows), int(arr[i].cols))
                outs.append(self._new_like(images[i], w.bottom - w.top, w.right - w.left))
        po = (Plane * max(n, 1))(*[self._out_plane(o, keep, o.shape[0], o.shape[1]) for o in outs])
        pc = _lib.CropPlanC(_lib.CropBoxC(*plan.crop_box), plan.out_rows, plan.out_cols, plan.actual_top, plan.actual_bottom, plan.actual_left,
                            plan.actual_right, 1 if plan.auto_detected else 0)
        st = (ImageStatsC * max(n, 1))() if want_stats else None
        self._check(self._L.ab_crop_channels(self._h, arr, n, C.byref(pc), po, st))
        return list(outs), ([self._stats_out(st[i]) for i in range(n)] if want_stats else None)

    # ---- core/stacking/drizzle.rs -------------------------------------------------------------------------
    drizzle_output_dims = staticmethod(drizzle_output_dims)

    def _drizzle(self, frames, offsets, cfg, out, out_weight, want_weight):
        n = len(frames)
        if n == 0:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "No images to drizzle")
        keep = []
        planes = self._planes(frames, keep)
        dims = [C.c_int64(0) for _ in range(4)]
        self._check_noctx(self._L.ab_drizzle_output_dims(planes, n, C.byref(cfg), *[C.byref(x) for x in dims]), n)
        orows, ocols = int(dims[2].value), int(dims[3].value)
        if out is None:
            out = self._new_like(frames[0], orows, ocols)
        if out_weight is None and want_weight:
            out_weight = self._new_like(frames[0], orows, ocols)
        for o in (out, out_weight):
            if o is not None and not _is_torch(o) and (o.shape != (orows, ocols) or o.dtype != np.float32 or not o.flags.c_contiguous):
                raise AstroBurstError(_lib.AB_ERR_INVALID, f"output must be a contiguous float32 array of {orows}x{ocols}")
        po = self._out_plane(out, keep, orows, ocols)
        pw = self._out_plane(out_weight, keep, orows, ocols) if out_weight is not None else None
        res = _lib.DrizzleResultC()
        off = (C.c_double * (2 * n))()
        if offsets is not None:
            flat = [float(v) for pair in offsets for v in pair]
            assert len(flat) == 2 * n, "one (dx, dy) pair per frame"
            off[:] = flat
            self._check(self._L.ab_drizzle_frames(self._h, planes, n, off, C.byref(cfg), C.byref(po), C.byref(pw) if pw is not None else None,
                                                  C.byref(res)))
        else:
            self._check(self._L.ab_drizzle_stack(self._h, planes, n, C.byref(cfg), C.byref(po), C.byref(pw) if pw is not None else None, off,
                                                 C.byref(res)))
        return DrizzleResult(out, out_weight, int(res.frame_count), float(res.output_scale), (int(res.in_rows), int(res.in_cols)),
                             (int(res.out_rows), int(res.out_cols)), [(off[2 * i], off[2 * i + 1]) for i in range(n)], int(res.rejected_pixels))

    def _check_noctx(self, rc, n):
        if rc != _lib.AB_OK:
            raise AstroBurstError(rc, "No images to drizzle" if n == 0 else "Drizzle requires at least 2 frames for sub-pixel reconstruction" if n < 2
                                  else "Frame dimensions vary too much, too many frames or a NaN scale / pixfrac")

    def drizzle_frames(self, frames, offsets, scale=2.0, pixfrac=0.7, kernel="square", sigma_low=3.0, sigma_high=3.0, sigma_iterations=5,
                       out=None, out_weight=None, want_weight=True) -> DrizzleResult:
        """drizzle_frame per frame + finalize (drizzle.rs:46-199) with the caller's offsets: one (dx, dy) per frame as
        DrizzleResult.offsets reports them.  frames: numpy (host) or CUDA tensors (device), dims within the reference's tolerance;
        the image and weight map are of the first frame's kind unless out / out_weight are given."""
        cfg = _drizzle_config(scale, pixfrac, kernel, sigma_low, sigma_high, sigma_iterations)
        return self._drizzle(frames, offsets, cfg, out, out_weight, want_weight)

    def drizzle_stack(self, frames, scale=2.0, pixfrac=0.7, kernel="square", sigma_low=3.0, sigma_high=3.0, sigma_iterations=5, align=True,
                      alignment_method="phase_correlation", num_threads=8, out=None, out_weight=None, want_weight=True) -> DrizzleResult:
        """drizzle_stack (drizzle.rs:227-346): offsets against frame 0 by phase correlation (the affine estimate where its confidence is
        low; always for "zncc"), then drizzle_frames."""
        cfg = _drizzle_config(scale, pixfrac, kernel, sigma_low, sigma_high, sigma_iterations, align, alignment_method, num_threads)
        return self._drizzle(frames, None, cfg, out, out_weight, want_weight)

    # ---- core/synth (generate_synth_cmd, generate_synth_stack_cmd) ----------------------------------------
    synth_config = staticmethod(synth_config)
    synth_star_field = staticmethod(synth_star_field)
    synth_rng_f64 = staticmethod(synth_rng_f64)

    def _synth_out(self, out, rows, cols, device, keep):
        """(array or tensor, ab_plane_mut) of a synth output: `out` if given, else a new CUDA tensor (device) or numpy array"""
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float32, device=f"cuda:{self.device}") if device else np.empty((rows, cols), np.float32)
        if not _is_torch(out) and (out.dtype != np.float32 or not out.flags.c_contiguous or out.ndim != 2):
            raise AstroBurstError(_lib.AB_ERR_INVALID, "outputs are contiguous 2-D float32 arrays")
        return out, self._out_plane(out, keep, int(out.shape[0]), int(out.shape[1]))

    @staticmethod
    def _synth_stars(stars):
        a = np.ascontiguousarray(stars, dtype=np.float64).reshape(-1, 5)
        return a, a.ctypes.data_as(C.POINTER(_lib.SynthStarC)), a.shape[0]

    def synth_render_stars(self, stars, psf, rows, cols, out=None, device=False):
        """render_stars (core/synth/psf.rs:123-158): stars (n, 5) as synth_star_field returns them, psf as synth_psf_type takes it ->
        the rows x cols f32 plane (numpy, or a CUDA tensor with device=True / a tensor `out`)"""
        keep = []
        out, po = self._synth_out(out, int(rows), int(cols), device, keep)
        a, ptr, n = self._synth_stars(stars)
        pt = synth_psf_type(psf)
        self._check(self._L.ab_synth_render_stars(self._h, ptr, n, C.byref(pt), C.byref(po)))
        return out

    def synth_flat_field(self, rows, cols, seed, vignette_strength, out=None, device=False):
        """generate_flat_field (noise.rs:81-99), bit for bit"""
        keep = []
        out, po = self._synth_out(out, int(rows), int(cols), device, keep)
        self._check(self._L.ab_synth_flat_field(self._h, int(seed) & (2 ** 64 - 1), float(vignette_strength), C.byref(po)))
        return out

    def synth_apply_flat_field(self, image, flat):
        """apply_flat_field (noise.rs:101-111): image /= flat where flat > 1e-6, in place (a float32 numpy array or a CUDA tensor)"""
        keep = []
        if not _is_torch(image) and not (isinstance(image, np.ndarray) and image.dtype == np.float32 and image.flags.c_contiguous and image.ndim == 2):
            raise AstroBurstError(_lib.AB_ERR_INVALID, "the in-place image must be a contiguous 2-D float32 array")
        pi = self._out_plane(image, keep, int(image.shape[0]), int(image.shape[1]))
        pf = self._plane(flat, keep)
        self._check(self._L.ab_synth_apply_flat_field(self._h, C.byref(pi), C.byref(pf)))
        return image

    def synth_apply_noise(self, image, out=None, **noise):
        """apply_noise (noise.rs:62-79) -> (noisy plane of the image's kind, frames_on_host: 1 if the general host route ran, else 0).
        noise: NoiseParams' fields (gain, readout_noise, sky_background, dark_current, exposure_time, bias_level, seed)."""
        keep = []
        pi = self._plane(image, keep)
        out, po = self._synth_out(out, pi.rows, pi.cols, _is_torch(image) and image.is_cuda, keep)
        p = synth_noise_params(**noise)
        res = _lib.SynthResultC()
        self._check(self._L.ab_synth_apply_noise(self._h, C.byref(pi), C.byref(p), C.byref(po), C.byref(res)))
        return out, int(res.frames_on_host)

    def _synth_generate(self, cfg, n, stack, device, want_truth):
        keep = []
        rows, cols = int(cfg.field.height), int(cfg.field.width)
        outs = [self._synth_out(None, rows, cols, device, keep) for _ in range(n)]
        frames = (Plane * max(n, 1))(*[po for _, po in outs])
        truth, pt = self._synth_out(None, rows, cols, device, keep) if want_truth else (None, None)
        cap = int(cfg.field.n_stars)
        stars = np.zeros((max(cap, 1), 5), np.float64)
        res = _lib.SynthResultC()
        fn = self._L.ab_synth_generate_stack if stack else self._L.ab_synth_generate
        self._check(fn(self._h, C.byref(cfg), frames, C.byref(pt) if pt is not None else None, stars.ctypes.data_as(C.POINTER(_lib.SynthStarC)),
                       cap, C.byref(res)))
        return SynthFrames([o for o, _ in outs], truth, stars[:min(cap, int(res.star_count))], int(res.frames_on_host))

    def synth_generate(self, cfg=None, device=False, want_truth=True, **config) -> SynthFrames:
        """generate (pipeline.rs:63-82) of a SynthConfig (or synth_config(**config)): one noisy frame, the ground truth, the stars"""
        cfg = cfg if cfg is not None else synth_config(**config)
        return self._synth_generate(cfg, 1, False, device, want_truth)

    def synth_generate_stack(self, cfg=None, device=False, want_truth=True, **config) -> SynthFrames:
        """generate_stack (pipeline.rs:84-108): cfg.n_frames noisy frames of one rendering; device frames go straight into
        stack_sigma_clip"""
        cfg = cfg if cfg is not None else synth_config(**config)
        if int(cfg.n_frames) == 0:
            raise AstroBurstError(_lib.AB_ERR_INVALID, "n_frames must be at least 1")
        return self._synth_generate(cfg, int(cfg.n_frames), True, device, want_truth)

    # ---- bench support -----------------------------------------------------------------------------
    def bench_copy(self, src, dst):
        self._check(self._L.ab_bench_copy(self._h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel()))
