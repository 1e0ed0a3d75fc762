"""The RGB Compose panel's commands without a GPU (csrc/compose_step.hip, tone.hip's ab_restretch_composite): tests/
compose_step_restatement.py pinned with the reference's own apply_lrgb cases (core/compose/lrgb.rs:69-136) and hand-computed pixels,
the reference's two error strings out of the restatement, the NULL-context answer of both entry points whatever else is wrong (only
that answer), and the agreement of the header, bindings/sys.rs and _lib.py on the prototypes and the info struct's layout.  The
library's own worded refusals need a live context, which needs the device: they are in tests/test_gpu_compose_step.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compose_step_restatement as R
from astroburst_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
WEIGHTS = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.35, 0.6)]


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def both(oracle, l, r, g, b, lw=1.0, cw=1.0):
    """oracle.apply_lrgb, after holding apply_lrgb_np to it bit for bit"""
    want = oracle.apply_lrgb(l, r, g, b, F32(lw), F32(cw))
    got = R.apply_lrgb_np(l, r, g, b, lw, cw)
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    return want


def full(shape, v):
    return np.full(shape, v, F32)


# ---- lrgb.rs:69-136 --------------------------------------------------------------------------------------------------------------------
def test_lrgb_preserves_gray(oracle):
    """test_lrgb_preserves_gray (:69-85)"""
    out = both(oracle, full((10, 10), 0.5), full((10, 10), 0.5), full((10, 10), 0.5), full((10, 10), 0.5))
    assert all(np.all(np.abs(p - F32(0.5)) < 0.01) for p in out)


def test_lrgb_boosts_luminance(oracle):
    """test_lrgb_boosts_luminance (:87-98)"""
    r, g, b = both(oracle, full((10, 10), 0.8), full((10, 10), 0.3), full((10, 10), 0.1), full((10, 10), 0.05))
    assert r[5, 5] > F32(0.3) and g[5, 5] > F32(0.1)


def test_lrgb_dimension_mismatch(oracle):
    """test_lrgb_dimension_mismatch (:100-108); the command resamples L first, so compose_rgb never raises it"""
    with pytest.raises(ValueError, match="do not match RGB"):
        oracle.apply_lrgb(full((10, 10), 0.5), full((10, 20), 0.5), full((10, 20), 0.5), full((10, 20), 0.5))


def test_lrgb_output_clamped(oracle):
    """test_output_clamped (:120-136): lum_old = 0.27008, ratio = 1 / 0.27008 = 3.7026, r = 0.9 * 3.7026 = 3.33 -> 1"""
    r, g, b = both(oracle, full((10, 10), 1.0), full((10, 10), 0.9), full((10, 10), 0.1), full((10, 10), 0.1))
    assert np.all(r == F32(1.0)) and np.all((g > F32(0.37)) & (g < F32(0.371))) and np.array_equal(g, b)


# ---- hand-computed pixels ----------------------------------------------------------------------------------------------------------------
def test_lrgb_dark_branch_and_its_threshold(oracle):
    """lum_old < 1e-10 (:28-33): the three channels become lum_new * lightness_weight, whatever the chrominance weight.  A gray pixel
    of 1e-10 has lum_old = 1e-10 * (0.2126 + 0.7152 + 0.0722) rounded per operation: just below, at or above the f32 1e-10, so its
    neighbours decide the branch on either side."""
    z = np.zeros((1, 4), F32)
    l = np.array([[0.7, 0.0, -0.5, np.inf]], F32)
    for lw, cw in WEIGHTS:
        out = both(oracle, l, z, z, z, lw, cw)
        with np.errstate(invalid="ignore"):
            want = l * F32(lw)                      # 0.7 * lw, 0, -0.5 * lw (NOT clamped in this branch), inf * lw (NaN for lw = 0)
        assert all(np.array_equal(p, want, equal_nan=True) for p in out)
    tiny = np.array([[5e-11, 2e-10, 0.0, -1.0]], F32)        # lum_old 5e-11 < 1e-10 <= 2e-10; a negative pixel is "dark" too
    out = both(oracle, full((1, 4), 0.25), tiny, tiny, tiny)
    assert out[0][0, 0] == F32(0.25) and out[0][0, 2] == F32(0.25) and out[0][0, 3] == F32(0.25)
    assert abs(float(out[0][0, 1]) - 0.25) < 1e-6    # (2e-10 takes the ratio branch: ratio = 0.25 / lum_old, the product comes back to ~0.25)


def test_lrgb_weights(oracle):
    """(0, 1): ratio = lum_old / lum_old = 1, out = v (clamped).  (1, 0): out = v * ratio * 0 + lum_new = lum_new (clamped).
    (0.35, 0.6) at r, g, b = 0.4, 0.2, 0.1 and lum_new = 0.5: lum_old = 0.2353, ratio = (0.175 + 0.152945) / 0.2353 = 1.39373,
    r = 0.4 * 1.39373 * 0.6 + 0.5 * 0.4 = 0.534495, g = 0.367247, b = 0.283624."""
    r, g, b, l = full((1, 1), 0.4), full((1, 1), 0.2), full((1, 1), 0.1), full((1, 1), 0.5)
    out = both(oracle, l, r, g, b, 0.0, 1.0)
    assert out[0][0, 0] == F32(0.4) and out[1][0, 0] == F32(0.2) and out[2][0, 0] == F32(0.1)
    out = both(oracle, l, r, g, b, 1.0, 0.0)
    assert all(p[0, 0] == F32(0.5) for p in out)
    out = both(oracle, l, r, g, b, 0.35, 0.6)
    assert np.allclose([p[0, 0] for p in out], [0.534495, 0.367247, 0.283624], rtol=0, atol=2e-6)
    out = both(oracle, l, r, g, b, 1.0, 1.0)      # ratio = 0.5 / 0.2353 = 2.12495
    assert np.allclose([p[0, 0] for p in out], [0.849979, 0.424989, 0.212495], rtol=0, atol=2e-6)


def test_lrgb_clamps_at_both_ends(oracle):
    """(1, 0) hands lum_new to the clamp: 1.5 -> 1, -0.25 -> 0, 1 stays; (1, 1) with lum_new = -1: ratio < 0, every product < 0 -> 0"""
    r, g, b = full((1, 3), 0.4), full((1, 3), 0.2), full((1, 3), 0.1)
    out = both(oracle, np.array([[1.5, -0.25, 1.0]], F32), r, g, b, 1.0, 0.0)
    assert all(p.tolist() == [[1.0, 0.0, 1.0]] for p in out)
    out = both(oracle, full((1, 3), -1.0), r, g, b, 1.0, 1.0)
    assert all(not p.any() for p in out)


def test_lrgb_nan_in_l(oracle):
    """a NaN lum_new: the dark branch writes NaN * lw; the ratio branch's NaN passes f32::clamp.  A NaN CHANNEL makes lum_old NaN,
    which is not < 1e-10: the ratio branch, all three NaN.  The preview's byte of a NaN is 0 (helpers.rs:243-245)."""
    l = np.array([[np.nan, np.nan, 0.5]], F32)
    r = np.array([[0.0, 0.4, np.nan]], F32)
    g = np.array([[0.0, 0.2, 0.2]], F32)
    b = np.array([[0.0, 0.1, 0.1]], F32)
    for lw, cw in WEIGHTS:
        out = both(oracle, l, r, g, b, lw, cw)
        assert all(np.isnan(p[0, 0]) and np.isnan(p[0, 2]) for p in out)
        if (lw, cw) == (0.0, 1.0):      # ratio = (NaN * 0 + ...) is NaN all the same
            assert all(np.isnan(p[0, 1]) for p in out)
    out = both(oracle, l, r, g, b)
    assert not oracle.render_rgb_preview(*out, 4096).any()


# ---- the command's restatement -------------------------------------------------------------------------------------------------------------
def planes(seed, rows, cols):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.01, 0.9, (rows, cols)).astype(F32) for _ in range(4)]


def test_restatement_is_the_commands_sequence(oracle):
    """compose_rgb is process_rgb, then L's stages in the command's order; without L the planes are process_rgb's own"""
    l, r, g, b = planes(3, 24, 40)
    kw = dict(align=False, scnr=dict(method="average", amount=0.7))
    c = R.compose_rgb(oracle, None, r, g, b, **kw)
    p = oracle.process_rgb(r, g, b, **kw)
    assert not c.lrgb_applied and c.l_stats is None and all(np.array_equal(x, y) for x, y in zip(c.planes, (p.r, p.g, p.b)))
    assert np.array_equal(c.rgb8, oracle.render_rgb_preview(p.r, p.g, p.b, 4096))
    c = R.compose_rgb(oracle, l, r, g, b, 0.35, 0.6, **kw)
    st = oracle.compute_image_stats(l)
    ls = oracle.apply_stf_f32(l, oracle.auto_stf(st), st)
    want = R.apply_lrgb_np(ls, p.r, p.g, p.b, 0.35, 0.6)
    assert c.lrgb_applied and not c.l_resampled and c.l_stats == st
    assert all(np.array_equal(x, y) for x, y in zip(c.planes, want))
    c = R.compose_rgb(oracle, l[:12, :20], r, g, b, auto_stretch=False, **kw)    # L as it is, after the resample
    p = oracle.process_rgb(r, g, b, auto_stretch=False, **kw)
    lm = oracle.resample_image(l[:12, :20], 24, 40)
    assert c.l_resampled and c.l_stats is None and np.array_equal(c.l_stretched, lm)
    assert all(np.array_equal(x, y) for x, y in zip(c.planes, R.apply_lrgb_np(lm, p.r, p.g, p.b)))
    c16 = R.compose_rgb(oracle, l, r, g, b, max_dim=16, **kw)
    assert c16.rgb8.shape == (10, 16, 3)


def test_restatement_keeps_the_references_error_strings(oracle):
    """rgb.rs:217 and harmonize_dimensions' ratio message, before L is looked at"""
    l, r, g, b = planes(4, 64, 96)
    with pytest.raises(ValueError, match=r"Need at least 2 channels for RGB compose \(got 1\)"):
        R.compose_rgb(oracle, l, r, None, None)
    with pytest.raises(ValueError, match=r"Need at least 2 channels for RGB compose \(got 0\)"):
        R.compose_rgb(oracle, l, None, None, None)
    with pytest.raises(ValueError, match=r"Channel dimension ratio 24\.0x exceeds 8x limit\. R=96x64 G=4x4\. Check channel assignments\."):
        R.compose_rgb(oracle, None, r, np.ones((4, 4), F32), None)


def test_restretch_restatement(oracle):
    """apply_stf_f32 x 3 with the cached statistics; apply_scnr_inplace's own threshold (scnr.rs:28-31) leaves the planes alone for an
    amount of 0, 1e-8 or below zero, and changes them at 0.5"""
    _, r, g, b = planes(5, 16, 24)
    g = (g + F32(0.5)).astype(F32)                # green above the others: SCNR has something to take
    stats = [oracle.compute_image_stats(x) for x in (r, g, b)]
    stf = [oracle.StfParams(0.02, 0.3, 0.9), oracle.StfParams(0.0, 0.5, 1.0), oracle.StfParams(0.1, 0.2, 0.8)]
    plain, by = R.restretch(oracle, r, g, b, stats, stf)
    assert all(np.array_equal(p, oracle.apply_stf_f32(x, s, t)) for p, x, s, t in zip(plain, (r, g, b), stf, stats))
    assert np.array_equal(by, oracle.render_rgb_preview(*plain, 4096))
    for amount in (0.0, 1e-8, -0.25):
        got, by2 = R.restretch(oracle, r, g, b, stats, stf, scnr=dict(method="average", amount=amount, preserve_luminance=True))
        assert all(np.array_equal(x, y) for x, y in zip(got, plain)) and np.array_equal(by, by2)
    got, _ = R.restretch(oracle, r, g, b, stats, stf, scnr=dict(method="average", amount=0.5))
    assert np.array_equal(got[0], plain[0]) and not np.array_equal(got[1], plain[1])


# ---- errors that need no device --------------------------------------------------------------------------------------------------------
def test_a_null_context_is_invalid_whatever_else_is_wrong(L):
    """Every call here passes a NULL context and proves only that answer: the entry points return AB_ERR_INVALID on their first line,
    whatever else is wrong with the arguments (noted per call), and write nothing.  The refusals themselves -- fewer than two channels,
    the ratio, a NULL out_pre, max_dim < 1 -- need a live context for their messages, which needs the device:
    tests/test_gpu_compose_step.py::test_refusals_leave_the_outputs_untouched exercises them."""
    a = [np.zeros((8, 8), F32) for _ in range(4)]
    o = [np.zeros((8, 8), F32) for _ in range(3)]
    p = [_lib.Plane(C.c_void_p(x.ctypes.data), 8, 8, 0) for x in a]
    small = _lib.Plane(C.c_void_p(a[3].ctypes.data), 1, 1, 0)
    po = (_lib.Plane * 3)(*[_lib.Plane(C.c_void_p(x.ctypes.data), 8, 8, 0) for x in o])
    by = np.zeros(8 * 8 * 3, np.uint8)
    bp = C.c_void_p(by.ctypes.data)
    cfg, info = _lib.RgbComposeConfigC(), _lib.ComposeRgbInfoC()
    f = L.ab_compose_rgb
    bad = _lib.AB_ERR_INVALID
    assert f(None, C.byref(p[3]), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(cfg), 1.0, 1.0, 4096, po, None, bp, 0, C.byref(info)) == bad
    assert f(None, None, C.byref(p[0]), None, None, C.byref(cfg), 1.0, 1.0, 4096, po, None, bp, 0, C.byref(info)) == bad          # (also: fewer than two channels)
    assert f(None, None, C.byref(p[0]), C.byref(small), None, C.byref(cfg), 1.0, 1.0, 4096, po, None, bp, 0, C.byref(info)) == bad  # (also: the ratio)
    assert f(None, None, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(cfg), 1.0, 1.0, 4096, None, None, bp, 0, C.byref(info)) == bad  # (also: NULL out_pre)
    assert f(None, None, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(cfg), 1.0, 1.0, 0, po, None, bp, 0, C.byref(info)) == bad      # (also: max_dim < 1)
    assert f(None, None, None, None, None, None, 1.0, 1.0, 0, None, None, None, 0, None) == bad
    st = (_lib.ImageStatsC * 3)()
    sp = (_lib.StfParamsC * 3)()
    g = L.ab_restretch_composite
    assert g(None, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), st, sp, 0, None, 4096, None, bp, 0) == bad
    assert g(None, None, None, None, None, None, 1, None, 0, None, None, 0) == bad
    assert not by.any() and not any(x.any() for x in o)
    assert bytes(info) == bytes(C.sizeof(info))


# ---- the three descriptions of the ABI ---------------------------------------------------------------------------------------------------
PROTOS = {
    "ab_compose_rgb": ["ctx", "l", "r", "g", "b", "cfg", "lrgb_lightness", "lrgb_chrominance", "max_dim", "out_pre", "out_planes", "out_rgb8",
                       "out_on_device", "info"],
    "ab_restretch_composite": ["ctx", "r", "g", "b", "stats", "stf", "has_scnr", "scnr", "max_dim", "out_planes", "out_rgb8", "out_on_device"],
}
C_TO_RUST = {"ab_ctx *": "*mut ab_ctx", "const ab_plane *": "*const ab_plane", "const ab_rgb_compose_config *": "*const ab_rgb_compose_config",
             "const ab_scnr_config *": "*const ab_scnr_config", "const ab_image_stats": "*const ab_image_stats", "const ab_stf_params": "*const ab_stf_params",
             "int64_t": "i64", "int32_t": "i32", "float": "f32", "uint8_t *": "*mut u8", "ab_plane_mut *": "*mut ab_plane_mut",
             "ab_compose_rgb_info *": "*mut ab_compose_rgb_info"}
C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "ab_ctx *": C.c_void_p, "uint8_t *": C.c_void_p}
MIRRORS = {"const ab_plane *": "Plane", "ab_plane_mut *": "Plane", "const ab_rgb_compose_config *": "RgbComposeConfigC", "const ab_scnr_config *": "ScnrConfigC",
           "const ab_image_stats": "ImageStatsC", "const ab_stf_params": "StfParamsC", "ab_compose_rgb_info *": "ComposeRgbInfoC"}


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "astroburst_hip.h")).read()
    args = re.search(r"AB_API int %s\(([^;]*?)\);" % name, text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(.*?)(\w+)(\[3\])?\s*$", " ".join(a.split()))      # (`stats[3]` decays to a pointer)
        out.append((m.group(1).strip(), m.group(2)))
    return out


@pytest.mark.parametrize("name", list(PROTOS))
def test_header_sys_rs_and_lib_py_agree_on_the_prototype(L, name):
    params = _header_params(name)
    assert [n for _, n in params] == PROTOS[name]
    sys_rs = open(os.path.join(ROOT, "bindings", "sys.rs")).read()
    rust = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, sys_rs).group(1)
    assert rust == ", ".join(f"{n}: {C_TO_RUST[t]}" for t, n in params)
    argtypes = getattr(L, name).argtypes
    assert len(argtypes) == len(params) and getattr(L, name).restype is C.c_int
    for (t, n), at in zip(params, argtypes):
        if t in C_TO_CTYPES:
            assert at is C_TO_CTYPES[t], (n, at)
        else:                                                   # a pointer to a struct: POINTER(its mirror)
            assert issubclass(at, C._Pointer) and at._type_ is getattr(_lib, MIRRORS[t]), (n, at)


def test_info_layout_is_the_same_in_the_header_sys_rs_and_lib_py(tmp_path):
    cls, n = _lib.ComposeRgbInfoC, "ab_compose_rgb_info"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "astroburst_hip.h"', 'int main(void) {', f'    printf("%zu", sizeof({n}));']
    lines += [f'    printf(" %zu", offsetof({n}, {f}));' for f, _ in cls._fields_]
    lines.append('    printf(" %zu\\n", sizeof(ab_processed_rgb_info));\n    return 0;\n}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    want = [int(t) for t in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert want.pop() == C.sizeof(_lib.ProcessedRgbInfoC)
    assert want == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    sys_rs = open(os.path.join(ROOT, "bindings", "sys.rs")).read()
    m = re.search(r"/// size (\d+), align 8\n#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct %s \{\n(.*?)\n\}" % n, sys_rs, re.S)
    fields = re.findall(r"pub (\w+): [^,]+, // offset (\d+)", m.group(2))
    assert [int(m.group(1))] + [int(o) for _, o in fields] == want
    assert [f for f, _ in fields] == [f for f, _ in cls._fields_]
