"""The compose wizard's blend and colour steps without a GPU (csrc/wizard_color.hip): the host-only entry points ab_color_step_plan and
ab_compute_auto_wb against tests/color_step_restatement.py, which is itself pinned by hand-computed cases here; the argument errors
that exist without a context; and the kernels' code for gfx950 (no scratch, no spills, no fused multiply-add in the white balance).
Every comparison is ==: integers, or the same IEEE operations.  The argument errors that carry a message (mismatched dims,
max_dim < 1, "No channel paths provided") need a live context, which needs the device: they are in tests/test_gpu_color_step.py."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import astroburst_amd as ab
import color_step_restatement as R
from astroburst_amd import ImageStats, _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "astroburst_amd", "csrc")
F32 = np.float32
E, K = R.EXACT_OR_FULL, R.KNOWN_RANGE
NO_SCNR, TINY, SCNR, PRESERVE = None, dict(amount=1e-8), dict(method="average", amount=0.8), dict(method="maximum", amount=1.0, preserve_luminance=True)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _st(mn=0.0, mx=1.0, median=0.5, mad=0.1):
    return ImageStats(mn, mx, median, mad, mad * 1.4826, median, 1000)


STATS = (_st(2.0, 10.0), _st(-4.0, 8.0), _st(0.25, 0.75))


# ---- the restatement, by hand ---------------------------------------------------------------------------------------------------
def test_restatement_factor_clamp():
    tiny = float(F32(1e-6))
    assert tiny == 9.999999974752427e-07
    for bad in (0.0, -3.0, float("nan"), -float("inf"), 1e-7):
        assert float(R.factor_f32(bad)) == tiny, bad
    assert float(R.factor_f32(1.5)) == 1.5 and float(R.factor_f32(1.7)) == 1.7000000476837158      # (1.7 as f32)
    assert float(R.factor_f32(1e40)) == math.inf                                                      # f64 as f32 overflows to inf
    assert float(R.factor_f32(2e-6)) == float(F32(2e-6))


def test_restatement_scnr_applied():
    assert not R.scnr_applied(None)
    assert not R.scnr_applied(dict(amount=1e-8)) and not R.scnr_applied(dict(amount=0.0)) and not R.scnr_applied(dict(amount=-1.0))
    assert not R.scnr_applied(dict(amount=float("nan")))
    assert not R.scnr_applied(dict(amount=1e-7))          # (1e-7 as f32) > 1e-7f32 is false
    assert R.scnr_applied(dict(amount=1.1e-7)) and R.scnr_applied(dict(amount=1.0)) and R.scnr_applied(dict(amount=7.0))


@pytest.mark.parametrize("n,scnr,want", [
    (4_000_000, NO_SCNR, (E, E, E)), (4_000_000, TINY, (E, E, E)), (4_000_000, SCNR, (E, E, E)), (4_000_000, PRESERVE, (E, E, E)),
    (4_000_001, NO_SCNR, (K, K, K)), (4_000_001, TINY, (K, K, K)), (4_000_001, SCNR, (K, E, K)), (4_000_001, PRESERVE, (E, E, E)),
], ids=lambda v: v if isinstance(v, int) else None)
def test_restatement_routes(n, scnr, want):
    p = R.plan(n, STATS, (1.5, 0.5, 2.0), scnr)
    assert p.route == want
    assert p.scnr_applied == (scnr is SCNR or scnr is PRESERVE)
    hand = ((3.0, 15.0), (-2.0, 4.0), (0.5, 1.5))        # orig.min * f, orig.max * f with f = 1.5, 0.5, 2.0
    for c in range(3):
        assert (p.known_min[c], p.known_max[c]) == (hand[c] if want[c] == K else (0.0, 0.0))


def test_restatement_known_range():
    assert R.known_range(STATS[0], F32(1.5)) == (3.0, 15.0)
    assert R.known_range(STATS[0], F32(-2.0)) == (-20.0, -4.0)      # swapped for a negative factor (color.rs:43-44)
    assert R.known_range(STATS[1], F32(0.0)) == (-0.0, 0.0)         # factor >= 0.0 holds for 0
    f = R.factor_f32(1.7)                                           # the f32 factor widened, not the f64 the command received
    assert R.known_range(STATS[0], f) == (2.0 * 1.7000000476837158, 10.0 * 1.7000000476837158)
    p = R.plan(5_000_000, STATS, (0.0, float("nan"), -3.0))         # the clamp comes first: 1e-6 for all three
    tiny = float(F32(1e-6))
    assert p.factors == (tiny, tiny, tiny) and p.route == (K, K, K)
    assert (p.known_min[1], p.known_max[1]) == (-4.0 * tiny, 8.0 * tiny)


def _wb(medians, mads):
    return R.compute_auto_wb(*[_st(median=m, mad=d) for m, d in zip(medians, mads)])


def test_restatement_auto_wb():
    M = R.F64_MAX
    assert M == 1.7976931348623157e308
    assert _wb((100.0, 200.0, 50.0), (1.0, 4.0, 2.0)) == ((1.0, 0.5, 2.0), (0.01, 0.02, 0.04), "R")          # R the most stable
    assert _wb((100.0, 200.0, 50.0), (5.0, 4.0, 0.5)) == ((0.5, 0.25, 1.0), (0.05, 0.02, 0.01), "B")         # B
    assert _wb((100.0, 200.0, 50.0), (5.0, 2.0, 5.0)) == ((2.0, 1.0, 4.0), (0.05, 0.01, 0.1), "G")           # G
    assert _wb((100.0, 200.0, 50.0), (1.0, 2.0, 2.0))[2] == "R"        # stab_r == stab_g: `<=` keeps R
    assert _wb((100.0, 200.0, 50.0), (1.0, 4.0, 0.5))[2] == "R"        # stab_r == stab_b: R
    assert _wb((100.0, 200.0, 50.0), (5.0, 2.0, 0.5))[2] == "B"        # stab_b == stab_g below stab_r: `<=` gives B, not G
    # a median <= 1e-10 is the least stable channel and counts as 1e-10 in the quotients
    assert _wb((1e-10, 200.0, 50.0), (0.0, 2.0, 2.0)) == ((200.0 / 1e-10, 1.0, 4.0), (M, 0.01, 0.04), "G")
    assert _wb((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) == ((1.0, 1.0, 1.0), (M, M, M), "R")
    assert _wb((-5.0, 200.0, 50.0), (1.0, 2.0, 2.0))[0] == (200.0 / 1e-10, 1.0, 4.0)
    nan = float("nan")                                                  # a NaN median is not > 1e-10 either: f64::MAX, and 1e-10 in the quotients
    assert _wb((nan, 200.0, 50.0), (1.0, 2.0, 4.0)) == ((200.0 / 1e-10, 1.0, 4.0), (M, 0.01, 0.08), "G")


# ---- ab_color_step_plan ---------------------------------------------------------------------------------------------------------------
def _plan_eq(got, want):
    assert got.factors == want.factors or all(a == b or (a != a and b != b) for a, b in zip(got.factors, want.factors))
    assert got.scnr_applied == want.scnr_applied and got.route == want.route
    assert got.known_min == want.known_min and got.known_max == want.known_max


@pytest.mark.parametrize("scnr", [NO_SCNR, TINY, SCNR, PRESERVE, dict(amount=float("nan")), dict(amount=1e-7), dict(amount=1.1e-7, preserve_luminance=True)],
                         ids=["none", "1e-8", "average", "max+preserve", "nan", "1e-7", "1.1e-7+preserve"])
@pytest.mark.parametrize("factors", [(1.0, 1.0, 1.0), (1.7, 0.6, 1.25), (0.0, float("nan"), 2.0), (-3.0, 1e-7, 1e40)],
                         ids=["ones", "mixed", "0-nan-2", "neg-tiny-huge"])
@pytest.mark.parametrize("n", [1, 3_999_999, 4_000_000, 4_000_001, 171_313_309])
def test_plan_equals_restatement(n, factors, scnr):
    _plan_eq(ab.color_step_plan(n, STATS, factors, scnr), R.plan(n, STATS, factors, scnr))


def test_plan_extreme_statistics():
    big = (_st(-1e300, 1e300), _st(float("-inf"), float("inf")), _st(0.0, 0.0))
    _plan_eq(ab.color_step_plan(10_000_000, big, (1e30, 2.0, 3.0)), R.plan(10_000_000, big, (1e30, 2.0, 3.0)))


def test_plan_argument_errors(L):
    st = (_lib.ImageStatsC * 3)()
    f = (C.c_double * 3)(1.0, 1.0, 1.0)
    cfg = _lib.ScnrConfigC(0, 1.0, 0)
    plan = _lib.ColorPlanC()
    INV = _lib.AB_ERR_INVALID
    assert L.ab_color_step_plan(10, None, f, 0, None, C.byref(plan)) == INV
    assert L.ab_color_step_plan(10, st, None, 0, None, C.byref(plan)) == INV
    assert L.ab_color_step_plan(10, st, f, 0, None, None) == INV
    assert L.ab_color_step_plan(10, st, f, 1, None, C.byref(plan)) == INV           # has_scnr without a configuration
    assert L.ab_color_step_plan(10, st, f, 0, None, C.byref(plan)) == _lib.AB_OK    # scnr may be NULL when has_scnr == 0
    assert L.ab_color_step_plan(10, st, f, 0, C.byref(cfg), C.byref(plan)) == _lib.AB_OK and plan.scnr_applied == 0
    assert L.ab_color_step_plan(10, st, f, 1, C.byref(cfg), C.byref(plan)) == _lib.AB_OK and plan.scnr_applied == 1


# ---- ab_compute_auto_wb --------------------------------------------------------------------------------------------------------------
def _wb_cases():
    rng = np.random.default_rng(187)
    vals = [0.0, 1e-10, 1.0000001e-10, 0.5, 100.0, 200.0, -5.0]
    cases = [(m, d) for m in itertools.product(vals[:6], repeat=3) for d in ((1.0, 1.0, 1.0), (0.5, 2.0, 1.0))]
    cases += [(tuple(rng.uniform(0.01, 1000.0, 3)), tuple(rng.uniform(0.0, 10.0, 3))) for _ in range(200)]
    cases += [((-5.0, 200.0, 50.0), (1.0, 2.0, 2.0)), ((float("nan"), 200.0, 50.0), (1.0, 2.0, 4.0)), ((100.0, 200.0, 50.0), (1.0, 2.0, 0.5))]
    return cases


def test_auto_wb_equals_restatement():
    for med, mad in _wb_cases():
        s = [_st(median=m, mad=d) for m, d in zip(med, mad)]
        got = ab.compute_auto_wb(*s)
        wb, stab, ref = R.compute_auto_wb(*s)
        assert (got.factors, got.stability, got.ref_channel) == (wb, stab, ref), (med, mad)


def test_auto_wb_factors_equal_select_wb_reference(L):
    """today's rgb.rs rule gives the same factors on every branch and tie -- the claim of the header's comment"""
    out = (C.c_double * 3)()
    for med, mad in _wb_cases():
        s = [_lib.ImageStatsC(0.0, 1.0, m, d, d, m, 10) for m, d in zip(med, mad)]
        assert L.ab_select_wb_reference(C.byref(s[0]), C.byref(s[1]), C.byref(s[2]), out) == _lib.AB_OK
        got = ab.compute_auto_wb(*[_st(median=m, mad=d) for m, d in zip(med, mad)])
        assert all(a == b or (a != a and b != b) for a, b in zip(got.factors, tuple(out))), (med, mad)


def test_auto_wb_argument_errors(L):
    s = _lib.ImageStatsC()
    out = _lib.AutoWbC()
    for args in ((None, s, s, out), (s, None, s, out), (s, s, None, out), (s, s, s, None)):
        assert L.ab_compute_auto_wb(*[None if a is None else C.byref(a) for a in args]) == _lib.AB_ERR_INVALID


# ---- the device entry points without a context --------------------------------------------------------------------------------------
def test_null_context(L):
    img = np.ones((2, 2), F32)
    pl = _lib.Plane(C.c_void_p(img.ctypes.data), 2, 2, 0)
    outs = [np.zeros((2, 2), F32) for _ in range(3)]
    po = (_lib.Plane * 3)(*[_lib.Plane(C.c_void_p(o.ctypes.data), 2, 2, 0) for o in outs])
    st = (_lib.ImageStatsC * 3)()
    f = (C.c_double * 3)(1.0, 1.0, 1.0)
    u8 = np.zeros(12, np.uint8)
    w = (_lib.BlendWeightC * 1)(_lib.BlendWeightC(0, 1.0, 1.0, 1.0))
    INV = _lib.AB_ERR_INVALID
    assert L.ab_calibrate_and_scnr(None, C.byref(pl), C.byref(pl), C.byref(pl), st, f, 0, None, 4096, po, C.c_void_p(u8.ctypes.data), 0, None) == INV
    assert L.ab_blend_composite(None, C.byref(pl), 1, w, 1, 4096, po, C.c_void_p(u8.ctypes.data), 0, None) == INV
    assert L.ab_blend_composite(None, None, 0, None, 0, 4096, None, None, 0, None) == INV
    assert not u8.any() and not any(o.any() for o in outs)


def test_symbols_and_wrappers():
    for name in ("ab_color_step_plan", "ab_calibrate_and_scnr", "ab_blend_composite", "ab_compute_auto_wb"):
        assert name in _lib.declared_symbols(), name
    assert callable(ab.Context.calibrate_and_scnr) and callable(ab.Context.blend_composite)
    assert ab.Context.color_step_plan is ab.color_step_plan and ab.Context.compute_auto_wb is ab.compute_auto_wb
    assert (ab.COLOR_STATS_EXACT_OR_FULL, ab.COLOR_STATS_KNOWN_RANGE) == (E, K)


# ---- the kernels, compiled for gfx950 with the Makefile's flags ---------------------------------------------------------------------
def test_kernels_have_no_scratch_no_spills_and_no_fused_multiply_add(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in base
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *base, "-w", "--save-temps", "-c", os.path.join(CSRC, "wizard_color.hip"), "-o",
                    os.path.join(tmp_path, "wizard_color.o")], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lst = open(os.path.join(tmp_path, "wizard_color-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_spill_count:\s+\d+", lst, re.S)}
    for family, count in (("wb_scnr_kernel", 4), ("linked_stf_kernel", 1), ("preview_stf_kernel", 2), ("save_stats_kernel", 1)):
        names = [n for n in meta if family in n]
        assert len(names) == count, (family, sorted(meta))
        for name in names:
            body = re.split(r"^%s:" % re.escape(name), lst, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[name]).group(1)) == 0, name
            assert "scratch_" not in body, name
            if family == "wb_scnr_kernel":      # v * factor and SCNR's gv + amount * (..) stay separate roundings
                for fused in ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_mad_f32", "v_mac_f32", "v_fma_mix"):
                    assert fused not in body, (name, fused)
                assert "v_mul_f32" in body or "v_pk_mul_f32" in body, name
                if name.endswith("Lb1EEEvNS_6WbArgsE"):        # <SCNR, VEC = true>: a group is one 16-byte access
                    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, name
    spills = re.findall(r"\.name:\s+(\S+)\n.*?\.vgpr_spill_count:\s+(\d+)", lst, re.S)
    assert len(spills) == 8 and all(int(n) == 0 for _, n in spills), spills
