"""The tone editor's decisions without a GPU: ab_tone_plan (host-only scalar code in the library) against tests/tone_restatement.py,
which restates apply_tone_composite_cmd (cmd/processing/curves.rs:86-154) in plain Python over the oracle's auto_stf,
compute_linked_stf and spline_lut_from_points.  Everything is compared exactly: flags with ==, STF parameters and statistics as f64
tuples, LUTs with array_equal.
"""
import ctypes as C

import numpy as np
import pytest

import tone_restatement as T
from astroburst_amd import _lib
from astroburst_amd.core import tone_plan


def _check_plan(oracle, stats, cfg, what):
    want = T.plan(oracle, stats, **cfg)
    info, luts = tone_plan(stats, **cfg)
    assert (info.levels_applied, info.curves_applied, info.scnr_applied) == (want["levels_applied"], want["curves_applied"], want["scnr_applied"]), what
    assert [T.stf_tuple(p) for p in info.stf] == [T.stf_tuple(p) for p in want["stf"]], what
    assert [T.stats_tuple(s) for s in info.norm] == [T.stats_tuple(s) for s in want["norm"]], what
    assert (info.rows, info.cols, info.preview_rows, info.preview_cols) == (0, 0, 0, 0), what
    if want["curves_applied"]:
        assert luts is not None and luts.shape == (3, 4096)
        for c in range(3):
            assert np.array_equal(luts[c], want["luts"][c]), f"{what}: LUT {c}"
    else:
        assert luts is None, what
    return info, want


@pytest.mark.parametrize("name", list(T.PLAN_TABLE))
def test_tone_plan_equals_the_restatement(oracle, name):
    _check_plan(oracle, T.sample_stats(oracle), T.PLAN_TABLE[name], name)


@pytest.mark.parametrize("name", ["auto_unlinked", "auto_linked", "one_explicit_linked", "everything"])
def test_tone_plan_on_statistics_without_valid_pixels(oracle, name):
    info, _ = _check_plan(oracle, T.empty_stats(oracle), T.PLAN_TABLE[name], name)
    if name == "auto_unlinked":
        assert [T.stf_tuple(p) for p in info.stf] == [(0.0, 0.5, 1.0)] * 3


@pytest.mark.parametrize("name", ["auto_unlinked", "auto_linked", "everything"])
def test_tone_plan_on_degenerate_statistics(oracle, name):
    _check_plan(oracle, T.flat_stats(oracle), T.PLAN_TABLE[name], f"{name}, max == min")
    _check_plan(oracle, T.denominator_stats(oracle), T.PLAN_TABLE[name], f"{name}, min 0 max 1.5")


def test_the_table_holds_what_it_says(oracle):
    """the restatement's own verdicts on the rows whose names promise one, so that a row cannot drift to the other side of its rule"""
    st = T.sample_stats(oracle)
    verdict = {n: T.plan(oracle, st, **c) for n, c in T.PLAN_TABLE.items()}
    for n in ("levels_identity_within", "auto_unlinked", "curves_s_and_none"):
        assert not verdict[n]["levels_applied"], n
    for n in ("levels_gamma_just_outside", "levels_black_just_outside", "levels_white_just_outside", "levels_one_channel", "levels_nan_gamma"):
        assert verdict[n]["levels_applied"], n
    for n in ("curves_none", "curves_some_empty", "curves_one_on_diagonal", "curves_two_identity_within"):
        assert not verdict[n]["curves_applied"], n
    for n in ("curves_one_off_diagonal", "curves_two_just_outside", "curves_three_collinear", "curves_s_and_none"):
        assert verdict[n]["curves_applied"], n
    assert not verdict["scnr_amount_1e-7"]["scnr_applied"] and verdict["scnr_amount_2e-7"]["scnr_applied"]
    assert not verdict["scnr_amount_nan"]["scnr_applied"] and verdict["scnr_full"]["scnr_applied"]
    # an explicit STF under linked_stf keeps the combined statistics; the identity LUT is no identity map; identity points still get
    # their own LUT once another channel has a curve
    one = verdict["one_explicit_linked"]
    assert T.stf_tuple(one["stf"][1]) == T.EXPLICIT and T.stf_tuple(one["stf"][0]) == T.stf_tuple(verdict["auto_linked"]["stf"][0])
    assert T.stats_tuple(one["norm"][1]) == T.stats_tuple(verdict["auto_linked"]["norm"][1])
    ident = verdict["curves_s_and_none"]["luts"][1]
    assert ident[0] == 0.0 and ident[4095] == 1.0 and np.all(np.diff(ident) > 0)
    mixed = verdict["curves_one_off_with_empty_and_diagonal"]["luts"]
    assert np.array_equal(mixed[0], ident) and not np.array_equal(mixed[2], ident)


def test_tone_config_default():
    cfg = _lib.ToneConfigC()
    C.memset(C.byref(cfg), 0xAB, C.sizeof(cfg))
    _lib.lib().ab_tone_config_default(C.byref(cfg))
    assert list(cfg.has_stf) == [0, 0, 0] and cfg.linked_stf == 0 and cfg.has_scnr == 0
    assert [(p.black, p.gamma, p.white) for p in cfg.levels] == [(0.0, 1.0, 1.0)] * 3
    assert not any(bool(p) for p in cfg.curve_xy) and list(cfg.n_curve) == [0, 0, 0]
    _lib.lib().ab_tone_config_default(None)   # tolerated


def test_null_arguments_are_invalid_and_touch_nothing(oracle):
    """every argument a caller may get wrong before a context exists: AB_ERR_INVALID with a message, and no device is needed to
    say so (the same paths with a live context are in tests/test_gpu_tone.py)"""
    L = _lib.lib()
    st = (_lib.ImageStatsC * 3)()
    cfg, info = _lib.ToneConfigC(), _lib.ToneInfoC()
    L.ab_tone_config_default(C.byref(cfg))
    assert L.ab_tone_plan(None, C.byref(cfg), C.byref(info), None) == _lib.AB_ERR_INVALID
    assert L.ab_tone_plan(st, None, C.byref(info), None) == _lib.AB_ERR_INVALID
    assert L.ab_tone_plan(st, C.byref(cfg), None, None) == _lib.AB_ERR_INVALID
    assert L.ab_tone_plan(st, C.byref(cfg), C.byref(info), None) == _lib.AB_OK   # the LUTs are optional
    a = np.zeros((4, 4), np.float32)
    p = _lib.Plane(C.c_void_p(a.ctypes.data), 4, 4, 0)
    out = np.zeros(48, np.uint8)
    rc = L.ab_apply_tone_composite(None, C.byref(p), C.byref(p), C.byref(p), st, C.byref(cfg), 4096, None, C.c_void_p(out.ctypes.data), 0, C.byref(info))
    assert rc == _lib.AB_ERR_INVALID and L.ab_last_error(None)
    assert not out.any()
