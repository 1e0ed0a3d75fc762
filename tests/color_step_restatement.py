"""Plain Python restatement of what the compose wizard's blend and colour steps decide beside the pixels the oracle already restates:
calibrate_and_scnr_cmd's factor clamp, its scnr_applied and the statistics it keeps (cmd/compose/color.rs:21-49, :97-184),
compute_auto_wb_cmd (:187-224), and the composition of both commands (color.rs and cmd/compose/blend.rs:128-223) out of
oracle.pyoracle.  numpy.float32 arithmetic is IEEE binary32, Python floats are IEEE doubles.  Pinned by the hand-computed cases of
tests/test_color_step_cpu.py."""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
PAR_THRESHOLD = 4_000_000       # color.rs:19
MAX_PREVIEW_DIM = 4096          # cmd/common.rs:16
EXACT_OR_FULL, KNOWN_RANGE = 0, 1
F64_MAX = float(np.finfo(np.float64).max)


def f32_max(a, b):
    """f32::max / f64::max: of a NaN and a number, the number"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def factor_f32(factor: float) -> np.float32:
    """(factor as f32).max(1e-6) (color.rs:115-117)"""
    with np.errstate(over="ignore"):
        return F32(f32_max(F32(factor), F32(1e-6)))


def scnr_applied(scnr) -> bool:
    """matches!(scnr_config, Some(cfg) if cfg.amount > 1e-7) (color.rs:138-139); amount is an f32"""
    return scnr is not None and bool(F32(scnr.get("amount", 1.0)) > F32(1e-7))


@dataclass
class Plan:
    factors: tuple      # 3 x float (the f32 factor's value)
    scnr_applied: bool
    route: tuple        # 3 x EXACT_OR_FULL | KNOWN_RANGE
    known_min: tuple    # 3 x float, 0.0 off the known-range route
    known_max: tuple


def known_range(orig_stats, factor: np.float32):
    """calibrate_channel's (known_min, known_max) (color.rs:41-45)"""
    f = float(factor)
    if factor >= F32(0.0):
        return orig_stats.min * f, orig_stats.max * f
    return orig_stats.max * f, orig_stats.min * f


def plan(n_pixels: int, orig_stats, factors, scnr=None) -> Plan:
    """The statistics the command KEEPS per channel and how it computed them.  calibrate_channel (color.rs:21-49) takes
    compute_image_stats of the scaled plane up to PAR_THRESHOLD pixels and compute_image_stats_with_known_range above.  With SCNR
    applied, G's are replaced by compute_image_stats of the final G (:154), and with preserve_luminance all three are (:142-152).  A
    channel SCNR leaves alone keeps calibrate_channel's, and its final plane is its scaled plane."""
    fs = [factor_f32(f) for f in factors]
    applied = scnr_applied(scnr)
    preserve = bool(scnr.get("preserve_luminance", False)) if scnr is not None else False
    route, kmin, kmax = [], [], []
    for c in range(3):
        replaced = applied and (c == 1 or preserve)
        if n_pixels <= PAR_THRESHOLD or replaced:
            route.append(EXACT_OR_FULL), kmin.append(0.0), kmax.append(0.0)
        else:
            lo, hi = known_range(orig_stats[c], fs[c])
            route.append(KNOWN_RANGE), kmin.append(lo), kmax.append(hi)
    return Plan(tuple(float(f) for f in fs), applied, tuple(route), tuple(kmin), tuple(kmax))


def compute_auto_wb(sr, sg, sb):
    """compute_auto_wb_cmd (color.rs:196-221) -> ((wb_r, wb_g, wb_b), (stab_r, stab_g, stab_b), "R" | "G" | "B")"""
    def stability(med, mad):
        return mad / med if med > 1e-10 else F64_MAX
    stab_r, stab_g, stab_b = stability(sr.median, sr.mad), stability(sg.median, sg.mad), stability(sb.median, sb.mad)
    mr, mg, mb = f32_max(sr.median, 1e-10), f32_max(sg.median, 1e-10), f32_max(sb.median, 1e-10)
    if stab_r <= stab_g and stab_r <= stab_b:
        wb, ref = (1.0, mr / mg, mr / mb), "R"
    elif stab_b <= stab_g:
        wb, ref = (mb / mr, mb / mg, 1.0), "B"
    else:
        wb, ref = (mg / mr, 1.0, mg / mb), "G"
    return wb, (stab_r, stab_g, stab_b), ref


def _tail(oracle, planes, stats, max_dim):
    """compute_linked_stf, make_stf_u8_fn x 3 and render_rgb_preview_with_stf (color.rs:163-168, blend.rs:200-205)"""
    linked, _ = oracle.compute_linked_stf(*stats)
    rgb8 = oracle.render_rgb_preview(*planes, max_dim, stf=[linked] * 3, stats=stats)
    return linked, rgb8


def calibrate_and_scnr(oracle, r, g, b, orig_stats, factors, scnr=None, max_dim=MAX_PREVIEW_DIM):
    """calibrate_and_scnr_cmd from its loaded originals on (color.rs:112-169), statement for statement -- the statistics it overwrites
    included -> (planes, rgb8, [stats], linked stf, scnr_applied)"""
    planes, stats = [], []
    for x, f, s in zip((r, g, b), factors, orig_stats):
        p, st = oracle.calibrate_channel(x, float(factor_f32(f)), s)
        planes.append(p), stats.append(st)
    applied = scnr_applied(scnr)
    if applied:
        planes = list(oracle.apply_scnr(*planes, method=scnr.get("method", "average"), amount=float(F32(scnr.get("amount", 1.0))),
                                        preserve_luminance=bool(scnr.get("preserve_luminance", False))))
        if scnr.get("preserve_luminance", False):
            stats = [oracle.compute_image_stats(p) for p in planes]
        else:
            stats[1] = oracle.compute_image_stats(planes[1])
    linked, rgb8 = _tail(oracle, planes, stats, max_dim)
    return planes, rgb8, stats, linked, applied


def blend_composite(oracle, channels, weights, max_dim=MAX_PREVIEW_DIM):
    """blend_channels_cmd from its loaded channels on (blend.rs:148-205) -> (planes, rgb8, [stats], linked stf, resampled)"""
    rows, cols = max(c.shape[0] for c in channels), max(c.shape[1] for c in channels)
    resampled = any(c.shape != (rows, cols) for c in channels)
    arrays = [oracle.resample_image(c, rows, cols) if c.shape != (rows, cols) else c for c in channels]
    planes = list(oracle.blend_channels(arrays, weights, rows, cols))   # (drops a weight whose channel_idx is out of range itself)
    stats = [oracle.compute_image_stats(p) for p in planes]
    linked, rgb8 = _tail(oracle, planes, stats, max_dim)
    return planes, rgb8, stats, linked, resampled
