"""Plain Python restatement of the RGB Compose panel's commands out of oracle.pyoracle: compose_rgb_cmd (cmd/compose/rgb.rs:43-205) --
process_rgb (:99-104), the L branch (:118-151: resample_image when L's dims differ, stf::analyze = compute_image_stats, auto_stf and
apply_stf_f32 when auto_stretch, apply_lrgb) and render_rgb_preview (:155-161) -- and restretch_composite_cmd (:208-241).  apply_lrgb_np
restates lrgb.rs:25-42 in numpy f32 operations, one rounding per operation as in the Rust closure, so that the oracle's own apply_lrgb
can be pinned against hand-computed pixels.  Pinned by tests/test_compose_step_cpu.py."""
from dataclasses import dataclass

import numpy as np

MAX_PREVIEW_DIM = 4096          # cmd/common.rs:16
F32 = np.float32


def apply_lrgb_np(l, r, g, b, lightness_weight=1.0, chrominance_weight=1.0, clamp=True):
    """lrgb.rs:25-42 -> new (r, g, b).  f32::clamp keeps a NaN; `lum_old < 1e-10` is false for a NaN lum_old.  clamp=False: the values
    the clamp of :39-41 receives (to see whether it binds)."""
    l, r, g, b = (np.asarray(x, F32) for x in (l, r, g, b))
    lw, cw, one = F32(lightness_weight), F32(chrominance_weight), F32(1.0)
    with np.errstate(all="ignore"):
        lum_old = r * F32(0.2126) + g * F32(0.7152) + b * F32(0.0722)
        dark = lum_old < F32(1e-10)
        blended = l * lw
        ratio = (l * lw + lum_old * (one - lw)) / lum_old
        out = []
        for v in (r, g, b):
            x = v * ratio * cw + l * (one - cw)
            if clamp:
                x = np.where(x < F32(0.0), F32(0.0), np.where(x > one, one, x)).astype(F32)
            out.append(np.where(dark, blended, x).astype(F32))
    return tuple(out)


@dataclass
class Composed:
    rgb: object              # oracle.ProcessedRgb: planes BEFORE LRGB in .r/.g/.b, pre_stretch, stf, channel_stats, offsets, stats_wb
    planes: tuple            # the final processed.r / g / b (after LRGB when L is given)
    rgb8: np.ndarray         # render_rgb_preview's bytes
    lrgb_applied: bool
    l_resampled: bool
    l_matched: object        # L at the composite's dims, or None
    l_stretched: object      # what apply_lrgb received, or None
    l_stats: object          # of the matched L (auto_stretch), or None
    l_stf: object


def compose_rgb(oracle, l, r, g, b, lrgb_lightness=1.0, lrgb_chrominance=1.0, max_dim=MAX_PREVIEW_DIM, **cfg) -> Composed:
    """compose_rgb_cmd's body; cfg: process_rgb's keyword arguments.  Raises ValueError with the reference's message."""
    p = oracle.process_rgb(r, g, b, **cfg)
    planes = (p.r, p.g, p.b)
    l_matched = l_stretched = l_stats = l_stf = None
    l_resampled = False
    if l is not None:                                                      # :118-151
        l = np.asarray(l, F32)
        l_resampled = l.shape != (p.rows, p.cols)
        l_matched = oracle.resample_image(l, p.rows, p.cols) if l_resampled else l.copy()
        l_stretched = l_matched
        if cfg.get("auto_stretch", True):
            l_stats = oracle.compute_image_stats(l_matched)
            l_stf = oracle.auto_stf(l_stats)
            l_stretched = oracle.apply_stf_f32(l_matched, l_stf, l_stats)
        planes = oracle.apply_lrgb(l_stretched, p.r, p.g, p.b, F32(lrgb_lightness), F32(lrgb_chrominance))
    rgb8 = oracle.render_rgb_preview(*planes, max_dim)
    return Composed(p, planes, rgb8, l is not None, l_resampled, l_matched, l_stretched, l_stats, l_stf)


def branches(c: Composed, lrgb_lightness=1.0, lrgb_chrominance=1.0):
    """which of apply_lrgb's branches a case takes, from the restatement alone: (pixels with lum_old < 1e-10, pixels, the clamp of
    :39-41 receives a value above 1 at some pixel of the other branch).  lum_old is of the planes before LRGB."""
    r, g, b = (np.asarray(x, F32) for x in (c.rgb.r, c.rgb.g, c.rgb.b))
    with np.errstate(all="ignore"):
        lum_old = r * F32(0.2126) + g * F32(0.7152) + b * F32(0.0722)
    dark = int(np.count_nonzero(lum_old < F32(1e-10)))
    raw = apply_lrgb_np(c.l_stretched, r, g, b, lrgb_lightness, lrgb_chrominance, clamp=False)
    with np.errstate(all="ignore"):
        clamped = any(bool(np.any((x > F32(1.0)) & ~(lum_old < F32(1e-10)))) for x in raw)
    return dark, r.size, clamped


def restretch(oracle, r, g, b, stats, stf, scnr=None, max_dim=MAX_PREVIEW_DIM):
    """restretch_composite_cmd's body (:224-237) -> (planes, bytes): apply_stf_f32 x 3 with the cached statistics, apply_scnr_inplace
    whenever a config is present, render_rgb_preview"""
    planes = tuple(oracle.apply_stf_f32(x, p, s) for x, p, s in zip((r, g, b), stf, stats))
    if scnr is not None:
        planes = oracle.apply_scnr(*planes, method=scnr.get("method", "average"), amount=scnr.get("amount", 1.0),
                                   preserve_luminance=scnr.get("preserve_luminance", False))
    return planes, oracle.render_rgb_preview(*planes, max_dim)
