"""Plain Python / numpy restatement of what opening a file computes beside the pixels the oracle already restates: downsample_histogram
(core/imaging/stats.rs:423-444), build_histogram's bin edges (:379-387, :412-413) and the composition of the two commands
(cmd/io/mod.rs:33-172).  Python floats are IEEE doubles and int() truncates towards zero, which for the non-negative values here is
Rust's `as usize`.  Pinned by the hand-computed cases of tests/test_view_cpu.py."""
import numpy as np

U32_MAX = 0xFFFFFFFF
HISTOGRAM_BINS = 65536          # stats.rs:8
HISTOGRAM_BINS_DISPLAY = 512    # types/constants.rs:9
MAX_PREVIEW_DIM = 4096          # cmd/common.rs:16


def ranges(n_bins: int, target: int):
    """[(start, end)] of downsample_histogram's source ranges (stats.rs:431-435); target < n_bins"""
    ratio = float(n_bins) / float(target)
    return [(int(float(i) * ratio), min(int(float(i + 1) * ratio), n_bins)) for i in range(target)]


def downsample(bins, target: int) -> np.ndarray:
    """downsample_histogram(&Histogram { bins, .. }, target) (stats.rs:423-444)"""
    src = np.asarray(bins, dtype=np.uint32)
    n = src.size
    if target >= n:
        return src.copy()                                  # :426-428
    out = np.zeros(target, np.uint32)
    wide = src.astype(np.uint64)
    for i, (start, end) in enumerate(ranges(n, target)):
        # u32::saturating_add in sequence == the exact sum clamped: the partial sums never decrease
        out[i] = min(int(wide[start:end].sum()), U32_MAX)
    return out


def dropped_tail(n_bins: int, target: int) -> int:
    """how many source bins at the top no output bin covers (target < n_bins)"""
    ratio = float(n_bins) / float(target)
    return n_bins - min(int(float(target) * ratio), n_bins)


def bin_edges(dmin: float, dmax: float, bins: int) -> np.ndarray:
    """Histogram.bin_edges of build_histogram (stats.rs:379-387, :412-413)"""
    rng = dmax - dmin
    if rng < 1e-10:
        return np.full(bins + 1, dmin, np.float64)
    step = rng / float(bins)
    return np.array([dmin + float(i) * step for i in range(bins + 1)], np.float64)


def display_histogram(oracle, img, dmin, dmax, target) -> np.ndarray:
    """downsample_histogram(&build_histogram(img, 65536, dmin, dmax), target)"""
    return downsample(oracle.build_histogram(img, HISTOGRAM_BINS, dmin, dmax), target)


def fits_view(oracle, img, hist_bins=HISTOGRAM_BINS_DISPLAY, target_bg=0.25, shadow_k=-2.8):
    """the mono branch of process_fits_full (cmd/io/mod.rs:138-144 with render_to_png, :25-27) -> (bytes, bins | None, stats, stf)"""
    st = oracle.compute_image_stats(img)
    stf = oracle.auto_stf(st, target_bg, shadow_k)
    u8 = oracle.apply_stf(img, stf, st)
    bins = display_histogram(oracle, img, st.min, st.max, hist_bins) if hist_bins > 0 else None
    return u8, bins, st, stf


def rgb_fits_view(oracle, r, g, b, hist_bins=HISTOGRAM_BINS_DISPLAY, max_dim=MAX_PREVIEW_DIM):
    """process_rgb_fits from its three planes on (cmd/io/mod.rs:44-62) -> (rgb8, bins | None, [stats], [stf])"""
    stats = [oracle.compute_image_stats(x) for x in (r, g, b)]
    stf = [oracle.auto_stf(s) for s in stats]
    toned = [oracle.apply_stf_f32(x, p, s) for x, p, s in zip((r, g, b), stf, stats)]
    rgb8 = oracle.render_rgb_preview(*toned, max_dim)
    bins = display_histogram(oracle, r, stats[0].min, stats[0].max, hist_bins) if hist_bins > 0 else None
    return rgb8, bins, stats, stf
