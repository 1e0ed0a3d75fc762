"""Plain Python restatement of the compose wizard's stretch step out of oracle.pyoracle: arcsinh_stretch_rgb_with_stats
(core/imaging/stretch.rs:56-90), the three commands of cmd/processing/stretch.rs that use it or the masked stretch
(apply_arcsinh_stretch_cmd :15-43, arcsinh_stretch_composite_cmd :94-124, masked_stretch_composite_cmd :135-221), and the truncating
preview packer (cmd/helpers.rs:243-245, :282-300) in numpy.  numpy.float32 arithmetic is IEEE binary32, Python floats are IEEE doubles.
Pinned by tests/test_stretch_step_cpu.py."""
import numpy as np

F32 = np.float32
MAX_PREVIEW_DIM = 4096          # cmd/common.rs:16


def f32_min(a, b):
    """f32::min: of a NaN and a number, the number"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def f32_max(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def clamp_factor(factor: float) -> np.float32:
    """(factor as f32).clamp(1.0, 500.0) (stretch.rs:26, :102): f32::clamp keeps a NaN"""
    with np.errstate(over="ignore"):
        f = F32(factor)
    if f != f:
        return f
    return F32(1.0) if f < F32(1.0) else (F32(500.0) if f > F32(500.0) else f)


def fold(sr, sg, sb):
    """(sr.min as f32).min(sg.min as f32).min(sb.min as f32) and likewise the maximum (core/imaging/stretch.rs:76-77)"""
    with np.errstate(over="ignore"):
        mn = f32_min(f32_min(F32(sr.min), F32(sg.min)), F32(sb.min))
        mx = f32_max(f32_max(F32(sr.max), F32(sg.max)), F32(sb.max))
    return F32(mn), F32(mx)


def arcsinh_stretch(oracle, image, factor):
    """arcsinh_stretch (core/imaging/stretch.rs:5-8)"""
    st = oracle.compute_image_stats(image)
    return oracle.arcsinh_stretch_with_stats(image, float(F32(st.min)), float(F32(st.max)), float(F32(factor)), 1.0)


def arcsinh_stretch_rgb(oracle, r, g, b, factor, gamma=1.0, global_min=None, global_max=None):
    """arcsinh_stretch_rgb_with_stats (:56-90) -> ((ro, go, bo), (gmin, gmax) | None for the clones)"""
    factor = F32(factor)
    if abs(factor) < F32(1e-10):
        return tuple(np.array(x, dtype=F32, copy=True) for x in (r, g, b)), None
    if global_min is not None and global_max is not None:
        gmin, gmax = F32(global_min), F32(global_max)
    else:
        gmin, gmax = fold(*[oracle.compute_image_stats(x) for x in (r, g, b)])
    planes = tuple(oracle.arcsinh_stretch_with_stats(x, float(gmin), float(gmax), float(factor), float(F32(gamma))) for x in (r, g, b))
    return planes, (gmin, gmax)


def preview_pick(oracle, rows, cols, max_dim):
    """(ph, pw, source rows, source cols) of render_rgb_preview's nearest-neighbour pick (helpers.rs:282-300)"""
    ph, pw = oracle.preview_dims(rows, cols, max_dim)
    if (ph, pw) == (rows, cols):
        return ph, pw, np.arange(rows), np.arange(cols)
    y_ratio, x_ratio = rows / ph, cols / pw
    sy = np.minimum(np.arange(ph, dtype=np.float64) * y_ratio, float(rows - 1)).astype(np.int64)
    sx = np.minimum(np.arange(pw, dtype=np.float64) * x_ratio, float(cols - 1)).astype(np.int64)
    return ph, pw, sy, sx


def pack_trunc(oracle, planes, max_dim):
    """(v.clamp(0, 1) * 255f32) as u8, NaN -> 0 (helpers.rs:243-245), of the picked pixels, interleaved: numpy f32"""
    rows, cols = planes[0].shape
    ph, pw, sy, sx = preview_pick(oracle, rows, cols, max_dim)
    out = np.zeros((ph, pw, 3), np.uint8)
    for c, p in enumerate(planes):
        v = np.asarray(p, dtype=F32)[np.ix_(sy, sx)]
        x = np.where(v < F32(0.0), F32(0.0), np.where(v > F32(1.0), F32(1.0), v)) * F32(255.0)   # f32::clamp keeps a NaN
        out[..., c] = np.where(np.isnan(x), F32(0.0), x).astype(np.uint8)                          # `as u8` truncates; NaN -> 0
    return out


def arcsinh_stretch_composite(oracle, r, g, b, factor, max_dim=MAX_PREVIEW_DIM, global_min=None, global_max=None):
    """arcsinh_stretch_composite_cmd (stretch.rs:101-115) -> (planes, rgb8, clamped factor, (gmin, gmax), degenerate)"""
    f = clamp_factor(factor)
    planes, (gmin, gmax) = arcsinh_stretch_rgb(oracle, r, g, b, f, 1.0, global_min, global_max)
    rgb8 = oracle.render_rgb_preview(*planes, max_dim)
    return planes, rgb8, f, (gmin, gmax), bool(gmax - gmin < F32(1e-10))


def arcsinh_stretch_view(oracle, image, factor):
    """apply_arcsinh_stretch_cmd (stretch.rs:23-32) with render_and_save's auto_stretch_preview (cmd/common.rs:18-22)
    -> (plane, u8, clamped factor, stats, stf)"""
    f = clamp_factor(factor)
    plane = arcsinh_stretch(oracle, image, f)
    st = oracle.compute_image_stats(plane)
    stf = oracle.auto_stf(st)
    return plane, oracle.apply_stf(plane, stf, st), f, st, stf


def masked_stretch_composite(oracle, r, g, b, shared_mask=False, max_dim=MAX_PREVIEW_DIM, **cfg):
    """masked_stretch_composite_cmd (stretch.rs:160-209) -> (planes, rgb8, [MaskedStretchResult x 3], stars, coverage, mask_mode)"""
    if shared_mask:
        rr, rg, rb, mask = oracle.masked_stretch_rgb_shared(r, g, b, **cfg)
        stars, coverage, mode = mask.stars_masked, mask.coverage_fraction, "shared_luminance"
    else:
        rr, rg, rb = (oracle.masked_stretch(x, **cfg) for x in (r, g, b))
        stars = rr.stars_masked + rg.stars_masked + rb.stars_masked
        coverage = (rr.mask_coverage + rg.mask_coverage + rb.mask_coverage) / 3.0
        mode = "per_channel"
    planes = (rr.image, rg.image, rb.image)
    return planes, oracle.render_rgb_preview(*planes, max_dim), [rr, rg, rb], stars, coverage, mode
