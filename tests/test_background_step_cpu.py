"""The compose wizard's background step without a GPU (csrc/wizard_background.hip): tests/background_step_restatement.py's pick against
hand-computed cases of downsample_nn (cmd/common.rs:152-184), its dims against ab_preview_dims, the NULL-context error of both entry
points, and the agreement of the header, bindings/sys.rs and _lib.py on the two prototypes and the info struct's layout.  The argument
errors that carry a message need a live context, which needs the device: they are in tests/test_gpu_background_step.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import astroburst_amd as ab
import background_step_restatement as R
from astroburst_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


# ---- the pick ------------------------------------------------------------------------------------------------------------------------
def test_pick_both_dims_fit():
    """cmd/common.rs:158-160: the bytes as they are"""
    assert R.pick_dims(5, 3, 5) == (5, 3) and R.pick_dims(5, 3, 4096) == (5, 3)
    px = np.arange(15, dtype=np.uint8).reshape(3, 5)
    got = R.downsample_nn(px, 5)
    assert got is not px and np.array_equal(got, px)


def test_pick_one_dim_over():
    """width 10, height 4, max_dim 5: scale 0.5 -> 5 x 2, both ratios 2.0"""
    assert R.pick_dims(10, 4, 5) == (5, 2)
    assert R.pick_indices(10, 5) == [0, 2, 4, 6, 8] and R.pick_indices(4, 2) == [0, 2]
    px = np.arange(40, dtype=np.uint8).reshape(4, 10)
    assert R.downsample_nn(px, 5).tolist() == [[0, 2, 4, 6, 8], [20, 22, 24, 26, 28]]
    # width 7, height 3, max_dim 4: scale 4 / 7 -> round(4.0) = 4 x round(1.714) = 2; ratios 1.75 and 1.5
    assert R.pick_dims(7, 3, 4) == (4, 2)
    assert R.pick_indices(7, 4) == [0, 1, 3, 5] and R.pick_indices(3, 2) == [0, 1]        # 0, 1.75, 3.5, 5.25 and 0, 1.5


def test_pick_rounds_half_away_from_zero():
    """f64::round, not Python's round-half-even: 10 * 0.25 = 2.5 -> 3, 6 * 0.25 = 1.5 -> 2, 2 * 0.25 = 0.5 -> 1"""
    assert R.round_half_away(2.5) == 3.0 and R.round_half_away(1.5) == 2.0 and R.round_half_away(0.5) == 1.0 and R.round_half_away(2.4999) == 2.0
    assert R.pick_dims(20, 10, 5) == (5, 3) and R.pick_dims(8, 6, 2) == (2, 2) and R.pick_dims(4, 2, 1) == (1, 1)


def test_pick_dst_rounds_to_one():
    """width 100, height 1, max_dim 10: 1 * 0.1 rounds to 0, .max(1.0) keeps one row; 517 x 301 at max_dim 1: one pixel, the first"""
    assert R.pick_dims(100, 1, 10) == (10, 1)
    assert R.pick_indices(1, 1) == [0] and R.pick_indices(100, 10) == list(range(0, 100, 10))
    assert R.pick_dims(517, 301, 1) == (1, 1)
    px = np.arange(301 * 517, dtype=np.uint32).astype(np.uint8).reshape(301, 517)
    assert R.downsample_nn(px, 1).tolist() == [[px[0, 0]]]
    assert R.pick_dims(3, 4000, 100) == (1, 100)      # 3 * 0.025 = 0.075 -> 0 -> 1 column: column 0 of every 40th row
    assert R.pick_indices(3, 1) == [0] and R.pick_indices(4000, 100) == list(range(0, 4000, 40))


def test_pick_clamp_binds():
    """.min((n - 1) as f64): along an axis that is NOT shrunk the product passes n - 1 and the clamp, not the cast, yields the last
    index -- 3 source pixels on 5 destinations: 0, 0.6, 1.2, 1.8, 2.4 -> min(2.4, 2.0)"""
    assert R.pick_indices(3, 5) == [0, 0, 1, 1, 2]
    assert min(4.0 * (3.0 / 5.0), 2.0) == 2.0 and 4.0 * (3.0 / 5.0) > 2.0
    assert R.pick_indices(2, 5) == [0, 0, 0, 1, 1]                                     # 0, 0.4, 0.8, 1.2, 1.6 -> min(1.6, 1.0)
    # inside downsample_nn dst <= n, so the largest product is (dst - 1) * n / dst <= n - 1: the clamp binds as an equality at dst == n
    assert R.pick_dims(100, 2, 99) == (99, 2) and R.pick_indices(2, 2) == [0, 1]
    for n, dst in ((13759, 4096), (12451, 3707), (517, 128), (301, 75), (2003, 512)):
        idx = R.pick_indices(n, dst)
        assert idx[0] == 0 and idx[-1] <= n - 1 and all(b > a for a, b in zip(idx, idx[1:]))


DIMS = [(64, 64, 4096), (301, 517, 4096), (301, 517, 128), (301, 517, 1), (257, 130, 100), (2001, 2003, 512), (2001, 2003, 4096),
        (13759, 12451, 4096), (12451, 13759, 4096), (10, 20, 5), (6, 8, 2), (2, 4, 1), (1, 100, 10), (4000, 3, 100), (4097, 4096, 4096),
        (1, 1, 1), (5, 5, 5), (5, 5, 4), (65535, 9, 4096)]


@pytest.mark.parametrize("rows,cols,max_dim", DIMS)
def test_pick_dims_are_ab_preview_dims(L, rows, cols, max_dim):
    """downsample_nn's round().max(1.0) (cmd/common.rs:162-164) is cmd/helpers.rs:285-287's rule, which ab_preview_dims restates"""
    ph, pw = C.c_int64(), C.c_int64()
    assert L.ab_preview_dims(rows, cols, max_dim, C.byref(ph), C.byref(pw)) == _lib.AB_OK
    dst_w, dst_h = R.pick_dims(cols, rows, max_dim)
    assert (ph.value, pw.value) == (dst_h, dst_w)


def test_restatement_preview_is_the_pick_of_every_pixels_bytes(oracle):
    rng = np.random.default_rng(2)
    plane = rng.uniform(0.0, 1.0, (37, 53)).astype(F32)
    plane[3, 4], plane[5, 6], plane[0, 0] = np.nan, 0.0, -1.0
    full, st, stf = R.auto_stretch_preview(oracle, plane)
    for max_dim in (4096, 16, 1):
        u8, st2, stf2 = R.preview_sampled(oracle, plane, max_dim)
        dst_w, dst_h = R.pick_dims(53, 37, max_dim)
        assert u8.shape == (dst_h, dst_w) and st2 == st and stf2 == stf
        for dy, sy in enumerate(R.pick_indices(37, dst_h)) if max_dim != 4096 else ():
            for dx, sx in enumerate(R.pick_indices(53, dst_w)):
                assert u8[dy, dx] == full[sy, sx]
    assert np.array_equal(R.preview_sampled(oracle, plane, 4096)[0], full)


def test_clamp_config_is_the_commands():
    """background.rs:44-47 with types/constants.rs:11-16"""
    f = ab.Context.background_step_clamp_config
    assert f(8, 3, 3) == (8, 3, 3) and f(0, 0, 0) == (3, 1, 1) and f(100, 9, 50) == (32, 5, 10) and f(3, 1, 1) == (3, 1, 1) and f(32, 5, 10) == (32, 5, 10)


# ---- errors that need no device ------------------------------------------------------------------------------------------------------
def test_a_null_context_is_invalid(L):
    a = np.zeros((8, 8), F32)
    o = np.zeros((8, 8), F32)
    p = _lib.Plane(C.c_void_p(a.ctypes.data), 8, 8, 0)
    po = _lib.Plane(C.c_void_p(o.ctypes.data), 8, 8, 0)
    by = np.zeros(64, np.uint8)
    cfg = _lib.BackgroundConfigC(2, 1, 2.5, 3, 0)
    st, stf, info = _lib.ImageStatsC(), _lib.StfParamsC(), _lib.BackgroundStepInfoC()
    assert L.ab_auto_stretch_preview_sampled(None, C.byref(p), None, 4096, C.c_void_p(by.ctypes.data), 0, C.byref(st), C.byref(stf)) == _lib.AB_ERR_INVALID
    assert L.ab_background_step(None, C.byref(p), C.byref(cfg), 4096, C.byref(po), None, C.c_void_p(by.ctypes.data), None, 0, C.byref(info)) == _lib.AB_ERR_INVALID
    # a NULL context comes first, whatever else is wrong
    assert L.ab_auto_stretch_preview_sampled(None, None, None, 0, None, 0, None, None) == _lib.AB_ERR_INVALID
    assert L.ab_background_step(None, None, None, 0, None, None, None, None, 0, None) == _lib.AB_ERR_INVALID
    assert not by.any() and not o.any()


# ---- the three descriptions of the ABI -----------------------------------------------------------------------------------------------
PROTOS = {
    "ab_auto_stretch_preview_sampled": ["ctx", "img", "cfg", "max_dim", "out_u8", "out_on_device", "out_stats", "out_stf"],
    "ab_background_step": ["ctx", "img", "cfg", "max_dim", "out_corrected", "out_model", "out_corrected_u8", "out_model_u8", "out_on_device", "info"],
}
C_TO_RUST = {"ab_ctx *": "*mut ab_ctx", "const ab_plane *": "*const ab_plane", "const ab_auto_stf_config *": "*const ab_auto_stf_config",
             "const ab_background_config *": "*const ab_background_config", "int64_t": "i64", "int32_t": "i32", "uint8_t *": "*mut u8",
             "ab_plane_mut *": "*mut ab_plane_mut", "ab_image_stats *": "*mut ab_image_stats", "ab_stf_params *": "*mut ab_stf_params",
             "ab_background_step_info *": "*mut ab_background_step_info"}
C_TO_CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "ab_ctx *": C.c_void_p, "uint8_t *": C.c_void_p}


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "astroburst_hip.h")).read()
    args = re.search(r"AB_API int %s\(([^;]*?)\);" % name, text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(.*?)(\w+)\s*$", " ".join(a.split()))
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
        else:                                                   # a pointer to a struct: POINTER(mirror) of the right size
            assert issubclass(at, C._Pointer), (n, at)
    assert argtypes[1]._type_ is _lib.Plane
    if name == "ab_background_step":
        assert argtypes[2]._type_ is _lib.BackgroundConfigC and argtypes[4]._type_ is _lib.Plane and argtypes[9]._type_ is _lib.BackgroundStepInfoC
    else:
        assert argtypes[2]._type_ is _lib.AutoStfConfigC and argtypes[6]._type_ is _lib.ImageStatsC and argtypes[7]._type_ is _lib.StfParamsC


def test_info_layout_is_the_same_in_the_header_sys_rs_and_lib_py(tmp_path):
    cls, n = _lib.BackgroundStepInfoC, "ab_background_step_info"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "astroburst_hip.h"', 'int main(void) {', f'    printf("%zu", sizeof({n}));']
    lines += [f'    printf(" %zu", offsetof({n}, {f}));' for f, _ in cls._fields_]
    lines.append('    printf("\\n");\n    return 0;\n}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    want = [int(t) for t in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert want == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    sys_rs = open(os.path.join(ROOT, "bindings", "sys.rs")).read()
    m = re.search(r"/// size (\d+), align 8\n#\[repr\(C\)\]\n#\[derive\([^)]*\)\]\npub struct %s \{\n(.*?)\n\}" % n, sys_rs, re.S)
    fields = re.findall(r"pub (\w+): [^,]+, // offset (\d+)", m.group(2))
    assert [int(m.group(1))] + [int(o) for _, o in fields] == want
    assert [f for f, _ in fields] == [f for f, _ in cls._fields_]
