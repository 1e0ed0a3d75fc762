"""apply_tone_composite_cmd (cmd/processing/curves.rs:57-191) restated in plain Python over the oracle's existing pieces.

The command's decision logic is written out here from the Rust -- the two is_identity rules (core/imaging/curves.rs:18-22, :94-103),
the STF choice (:86-111), the LUT each channel is looked up in (:133-146), the SCNR condition (:148-154) -- and the pixels come from
pyoracle.apply_stf_f32, apply_levels, apply_curve, apply_scnr and render_rgb_preview.  A configuration is the dict of keyword
arguments astroburst_amd's tone_plan / Context.apply_tone_composite take, so one table serves both sides:
    stf         None | three of (None | (shadow, midtone, highlight))      stf_r / stf_g / stf_b: Option<[f64; 3]>
    linked_stf  bool                                                      Option<bool>.unwrap_or(false)
    levels      None | three of (None | (black, gamma, white))            Option<ToneLevelsInput>
    curves      None | three of (None | [(x, y), ...], possibly empty)    Option<ToneCurveInput>
    scnr        None | dict(method=, amount=, preserve_luminance=)        Option<ScnrConfig>
"""
import dataclasses

import numpy as np

F32 = np.float32
IDENTITY_POINTS = [(0.0, 0.0), (1.0, 1.0)]     # identity_lut (cmd/processing/curves.rs:53-55)
S_CURVE = [(0.0, 0.0), (0.25, 0.15), (0.5, 0.5), (0.75, 0.85), (1.0, 1.0)]


def levels_is_identity(p) -> bool:
    """LevelsParams::is_identity (core/imaging/curves.rs:18-22)"""
    black, gamma, white = p
    return abs(black) < 1e-7 and abs(gamma - 1.0) < 1e-7 and abs(white - 1.0) < 1e-7


def curve_is_identity(points) -> bool:
    """SplineLut::is_identity (core/imaging/curves.rs:94-103)"""
    if len(points) > 2:
        return False
    if len(points) == 0:
        return True
    if len(points) == 1:
        return abs(points[0][0] - points[0][1]) < 1e-6
    near_start = abs(points[0][0]) < 1e-6 and abs(points[0][1]) < 1e-6
    near_end = abs(points[1][0] - 1.0) < 1e-6 and abs(points[1][1] - 1.0) < 1e-6
    return near_start and near_end


def _three(x):
    return (None, None, None) if x is None else tuple(x)


def plan(oracle, stats, stf=None, linked_stf=False, levels=None, curves=None, scnr=None) -> dict:
    """cmd/processing/curves.rs:86-154 without the pixels -> dict(stf, norm, levels, levels_applied, curves_applied, luts, scnr_applied)"""
    stf, levels, curves = _three(stf), _three(levels), _three(curves)
    if linked_stf:                                                     # :89-91
        p, combined = oracle.compute_linked_stf(*stats)
        auto, norm = [p] * 3, [combined] * 3
    else:                                                              # :92-100
        auto, norm = [oracle.auto_stf(s) for s in stats], list(stats)
    applied = [auto[c] if stf[c] is None else oracle.StfParams(*stf[c]) for c in range(3)]   # :103-111
    lv = [(0.0, 1.0, 1.0) if p is None else tuple(float(v) for v in p) for p in levels]     # :121-123
    levels_applied = any(not levels_is_identity(p) for p in lv)        # :125
    ident = [pts is None or curve_is_identity(pts) for pts in curves]  # :133-135
    curves_applied = not all(ident)                                    # :136
    luts = None
    if curves_applied:                                                 # :139-141: Some -> build_spline, None -> identity_lut
        luts = [oracle.spline_lut_from_points(IDENTITY_POINTS if pts is None else list(pts)) for pts in curves]
    # :149 `cfg.amount > 1e-7` on an f32 (a NaN compares false)
    scnr_applied = scnr is not None and bool(F32(scnr.get("amount", 1.0)) > F32(1e-7))
    return dict(stf=applied, norm=norm, levels=lv, levels_applied=levels_applied, curves_applied=curves_applied, luts=luts,
                scnr_applied=scnr_applied)


def compose(oracle, r, g, b, stats, max_dim, **cfg):
    """the command from its loaded channels to the encoder's input -> ((r_img, g_img, b_img), preview bytes, plan)"""
    pl = plan(oracle, stats, **cfg)
    ch = [oracle.apply_stf_f32(x, pl["stf"][c], pl["norm"][c]) for c, x in enumerate((r, g, b))]   # :113-119
    if pl["levels_applied"]:                                           # :126-131 (apply_levels clones an identity channel)
        ch = [oracle.apply_levels(x, *pl["levels"][c]) for c, x in enumerate(ch)]
    if pl["curves_applied"]:                                           # :138-146
        ch = [oracle.apply_curve(x, pl["luts"][c]) for c, x in enumerate(ch)]
    if pl["scnr_applied"]:                                             # :148-152
        s = cfg["scnr"]
        ch = list(oracle.apply_scnr(*ch, s.get("method", "average"), s.get("amount", 1.0), s.get("preserve_luminance", False)))
    return tuple(ch), oracle.render_rgb_preview(*ch, max_dim), pl      # :161


def unfused_chain(ctx, r, g, b, stats, max_dim, **cfg):
    """the same command through the library's own entry points, one launch per stage and channel (INTEGRATION.md's earlier form):
    apply_stf_f32 x 3 -> apply_levels x 3 -> apply_curve x 3 -> apply_scnr_inplace -> render_rgb_preview.  The decisions are the
    library's tone_plan -> ((r_img, g_img, b_img), preview bytes)"""
    info, luts = ctx.tone_plan(stats, **cfg)
    levels = [(0.0, 1.0, 1.0) if p is None else p for p in _three(cfg.get("levels"))]
    ch = [ctx.apply_stf_f32(x, info.stf[c], info.norm[c]) for c, x in enumerate((r, g, b))]
    if info.levels_applied:
        ch = [ctx.apply_levels(x, *levels[c]) for c, x in enumerate(ch)]
    if info.curves_applied:
        ch = [ctx.apply_curve(x, luts[c]) for c, x in enumerate(ch)]
    if info.scnr_applied:
        s = cfg["scnr"]
        ctx.apply_scnr_inplace(*ch, s.get("method", "average"), s.get("amount", 1.0), s.get("preserve_luminance", False))
    return tuple(ch), ctx.render_rgb_preview(*ch, max_dim)


def stats_tuple(s):
    """an ImageStats of either side as exact numbers"""
    return dataclasses.astuple(s)


def stf_tuple(p):
    return (p.shadow, p.midtone, p.highlight)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- the configurations ------------------------------------------------------------------------------------------------------------
# statistics of a plausible composite (they need not belong to any plane: the command takes them as given)
def sample_stats(oracle):
    return [oracle.ImageStats(0.001, 0.95, 0.12, 0.02, 0.03, 0.14, 30000), oracle.ImageStats(0.002, 1.10, 0.10, 0.015, 0.022, 0.12, 29000),
            oracle.ImageStats(0.0005, 0.80, 0.15, 0.03, 0.044, 0.17, 31000)]


EXPLICIT = (0.05, 0.3, 0.9)
PLAN_TABLE = {
    "auto_unlinked": dict(),
    "auto_linked": dict(linked_stf=True),
    "one_explicit_linked": dict(stf=(None, EXPLICIT, None), linked_stf=True),
    "three_explicit": dict(stf=((0.0, 0.5, 1.0), EXPLICIT, (0.1, 0.7, 0.8))),
    "levels_identity_within": dict(levels=((5e-8, 1.0 + 5e-8, 1.0 - 5e-8), None, (-9e-8, 1.0, 1.0))),
    "levels_gamma_just_outside": dict(levels=(None, (0.0, 1.0 + 2e-7, 1.0), None)),
    "levels_black_just_outside": dict(levels=((2e-7, 1.0, 1.0), None, None)),
    "levels_white_just_outside": dict(levels=(None, None, (0.0, 1.0, 1.0 - 2e-7))),
    "levels_one_channel": dict(levels=((0.1, 1.8, 0.9), None, None)),
    "levels_three": dict(levels=((0.1, 1.8, 0.9), (0.0, 0.5, 1.0), (0.02, 1.0, 0.7))),
    "levels_nan_gamma": dict(levels=(None, (0.0, float("nan"), 1.0), None)),
    "curves_none": dict(curves=(None, None, None)),
    "curves_some_empty": dict(curves=([], None, None)),
    "curves_one_on_diagonal": dict(curves=(None, [(0.4, 0.4)], None)),
    "curves_one_off_diagonal": dict(curves=(None, [(0.4, 0.6)], None)),
    "curves_one_off_with_empty_and_diagonal": dict(curves=([], [(0.4, 0.6)], [(0.3, 0.3 + 5e-7)])),
    "curves_two_identity_within": dict(curves=([(5e-7, -5e-7), (1.0 - 5e-7, 1.0 + 5e-7)], None, None)),
    "curves_two_just_outside": dict(curves=([(0.0, 2e-6), (1.0, 1.0)], None, None)),
    "curves_three_collinear": dict(curves=(None, None, [(0.0, 0.0), (0.5, 0.5), (1.0, 1.0)])),
    "curves_s_and_none": dict(curves=(S_CURVE, None, None)),
    "curves_unsorted_duplicate_x": dict(curves=([(0.7, 0.9), (0.2, 0.1), (0.2, 0.3)], [(0.5, 0.2)], S_CURVE)),
    "scnr_amount_1e-7": dict(scnr=dict(method="average", amount=1e-7)),
    "scnr_amount_2e-7": dict(scnr=dict(method="average", amount=2e-7)),
    "scnr_amount_nan": dict(scnr=dict(method="maximum", amount=float("nan"))),
    "scnr_full": dict(scnr=dict(method="maximum", amount=1.0, preserve_luminance=True)),
    "everything": dict(stf=(EXPLICIT, None, None), linked_stf=True, levels=((0.1, 1.8, 0.9), None, (0.0, 0.7, 1.0)), curves=(S_CURVE, None, []),
                       scnr=dict(method="average", amount=0.8, preserve_luminance=True)),
}


def flat_stats(oracle):
    """max == min: the range is 1e-30 (stf.rs:70)"""
    return [oracle.ImageStats(0.25, 0.25, 0.25, 0.0, 0.0, 0.25, 1000), oracle.ImageStats(0.5, 0.5, 0.5, 0.0, 0.0, 0.5, 10),
            oracle.ImageStats(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 5)]


def denominator_stats(oracle):
    """min 0, max 1.5: pixel 1.0 normalises to the f64 nearest 2 / 3, where the MTF's denominator (2 m - 1) x - m vanishes for m = 2"""
    return [oracle.ImageStats(0.0, 1.5, 0.6, 0.1, 0.15, 0.6, 1000)] * 3


def empty_stats(oracle):
    """valid_count == 0: auto_stf returns {0, 0.5, 1} (stf.rs:14-16) whatever else the statistics hold"""
    return [oracle.ImageStats(), oracle.ImageStats(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0), oracle.ImageStats(0.2, 0.9, 0.4, 0.1, 0.15, 0.45, 0)]
