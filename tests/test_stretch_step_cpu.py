"""The compose wizard's stretch step without a GPU (csrc/wizard_stretch.hip): tests/stretch_step_restatement.py against the reference's
own unit cases for the RGB form and against the oracle's packer; the host-only fold ab_arcsinh_rgb_range against the restatement; the
argument errors that exist without a context; the ctypes mirrors of the new structs; and the kernels' code for gfx950 (no scratch, no
spills, 16-byte loads and one vector atomic per word in the range pass).  Every comparison is ==.  The argument errors that carry a
message (mismatched dims, max_dim < 1, both outputs NULL, one of global_min / global_max, overlaps) need a live context, which needs
the device: they are in tests/test_gpu_stretch_step.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import astroburst_amd as ab
import stretch_step_restatement as R
from astroburst_amd import ImageStats, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astroburst_amd", "csrc")
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _st(mn, mx):
    return ImageStats(mn, mx, 0.5 * (mn + mx), 0.1, 0.14826, 0.5 * (mn + mx), 1000)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_restatement_factor_clamp():
    assert float(R.clamp_factor(0.3)) == 1.0 and float(R.clamp_factor(-7.0)) == 1.0 and float(R.clamp_factor(-math.inf)) == 1.0
    assert float(R.clamp_factor(20.0)) == 20.0 and float(R.clamp_factor(1.7)) == 1.7000000476837158      # (1.7 as f32)
    assert float(R.clamp_factor(1e9)) == 500.0 and float(R.clamp_factor(1e300)) == 500.0 and float(R.clamp_factor(math.inf)) == 500.0
    assert math.isnan(float(R.clamp_factor(math.nan)))                                                    # f32::clamp keeps a NaN


def test_restatement_reproduces_the_reference_rgb_consistency_case(oracle):
    """test_arcsinh_stretch_rgb_consistency (core/imaging/stretch.rs:146-154)"""
    ch = np.fromfunction(lambda r, c: (r + c) / 20.0, (10, 10)).astype(F32)
    single = R.arcsinh_stretch(oracle, ch, 20.0)
    (ro, go, bo), (gmin, gmax) = R.arcsinh_stretch_rgb(oracle, ch, ch, ch, 20.0)
    assert float(gmin) == float(F32(0.05)) and float(gmax) == float(F32(0.9))     # (the zero pixel is padding, not the minimum)
    for x in (ro, go, bo):
        assert np.array_equal(single.view(np.uint32), x.view(np.uint32))


def test_restatement_reproduces_the_reference_rgb_global_norm_case(oracle):
    """test_arcsinh_stretch_rgb_global_norm (core/imaging/stretch.rs:166-179)"""
    r, g, b = (np.array([v], dtype=F32) for v in ([0.5, 2.0], [0.3, 1.0], [0.1, 0.5]))
    (ro, go, bo), (gmin, gmax) = R.arcsinh_stretch_rgb(oracle, r, g, b, 20.0)
    assert (float(gmin), float(gmax)) == (float(F32(0.1)), 2.0)
    assert ro[0, 1] > go[0, 1] > bo[0, 1]
    for ch in (ro, go, bo):
        assert ((ch >= 0.0) & (ch <= 1.0)).all()
    assert abs(float(ro[0, 1]) - 1.0) < 1e-6 and bo[0, 0] == 0.0


def test_restatement_zero_factor_clones_and_given_range(oracle):
    r, g, b = (np.array([v], dtype=F32) for v in ([0.5, 2.0], [0.3, np.nan], [0.1, 0.5]))
    planes, rng = R.arcsinh_stretch_rgb(oracle, r, g, b, 0.0)
    assert rng is None and all(np.array_equal(p.view(np.uint32), x.view(np.uint32)) for p, x in zip(planes, (r, g, b)))
    a, ra = R.arcsinh_stretch_rgb(oracle, r, g, b, 20.0)
    c, rc = R.arcsinh_stretch_rgb(oracle, r, g, b, 20.0, global_min=ra[0], global_max=ra[1])
    assert ra == rc and all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, c))
    d, rd = R.arcsinh_stretch_rgb(oracle, r, g, b, 20.0, global_min=0.0)    # (Some, None): the range is computed (stretch.rs:69-71)
    assert rd == ra


def test_restatement_nan_factor_and_degenerate_range(oracle):
    """a NaN factor: every finite pixel becomes NaN, a non-finite one 0, the bytes 0; a flat composite: zeros"""
    r, g, b = (np.array([v], dtype=F32) for v in ([0.5, 2.0, np.inf], [0.3, np.nan, 1.0], [0.1, 0.5, -1.0]))
    planes, rgb8, f, _, degenerate = R.arcsinh_stretch_composite(oracle, r, g, b, math.nan, 4096)
    assert math.isnan(float(f)) and not degenerate
    for p, x in zip(planes, (r, g, b)):
        assert np.isnan(p[np.isfinite(x)]).all() and (p[~np.isfinite(x)] == 0.0).all()
    assert not rgb8.any()
    flat = np.full((2, 3), 0.25, F32)
    planes, rgb8, _, (gmin, gmax), degenerate = R.arcsinh_stretch_composite(oracle, flat, flat, flat, 20.0, 4096)
    assert degenerate and gmin == gmax == F32(0.25) and not rgb8.any() and not any(p.any() for p in planes)


@pytest.mark.parametrize("max_dim", [4096, 7, 1])
def test_restatement_numpy_packer_is_the_oracles(oracle, max_dim):
    rng = np.random.default_rng(5)
    planes = [rng.uniform(-0.2, 1.2, (13, 29)).astype(F32) for _ in range(3)]
    planes[0][3, 4], planes[1][5, 6], planes[2][7, 8] = np.nan, np.inf, -np.inf
    planes[0][0, 0], planes[1][0, 0] = F32(1.0), F32(np.nextafter(F32(1.0), F32(0.0)))   # 255 and 254.99998 -> 254
    got = R.pack_trunc(oracle, planes, max_dim)
    assert got.shape[:2] == oracle.preview_dims(13, 29, max_dim)
    assert np.array_equal(got, oracle.render_rgb_preview(*planes, max_dim))
    if max_dim == 4096:
        assert tuple(got[0, 0, :2]) == (255, 254) and got[3, 4, 0] == 0 and got[5, 6, 1] == 255 and got[7, 8, 2] == 0


# ---- ab_arcsinh_rgb_range ------------------------------------------------------------------------------------------------------------
RANGE_CASES = {
    "ordinary": (_st(2.0, 10.0), _st(0.125, 8.0), _st(0.25, 0.75)),
    "default-channel": (_st(2.0, 10.0), ImageStats(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0), _st(0.25, 0.75)),   # contributes 0 to both
    "equal": (_st(0.3, 0.9),) * 3,
    "not-f32": (_st(0.1, 0.7), _st(1e-7 * 1.5, 1e39), _st(0.2, 16777217.0)),    # roundings of `as f32`, an overflow to inf
}


@pytest.mark.parametrize("case", list(RANGE_CASES), ids=list(RANGE_CASES))
def test_rgb_range_is_the_restatements_fold(case):
    st = RANGE_CASES[case]
    want = R.fold(*st)
    got = ab.arcsinh_rgb_range(*st)
    assert got == (float(want[0]), float(want[1]))
    if case == "default-channel":
        assert got == (0.0, 10.0)
    if case == "not-f32":
        assert got == (float(F32(1.5e-7)), math.inf)


def test_rgb_range_null_arguments(L):
    out = (C.c_float * 2)()
    st = (_lib.ImageStatsC * 3)()
    assert L.ab_arcsinh_rgb_range(None, out) == _lib.AB_ERR_INVALID
    assert L.ab_arcsinh_rgb_range(st, None) == _lib.AB_ERR_INVALID
    assert L.ab_arcsinh_rgb_range(st, out) == _lib.AB_OK and tuple(out) == (0.0, 0.0)


# ---- errors that need no device ------------------------------------------------------------------------------------------------------
def test_a_null_context_is_invalid(L):
    a = np.zeros((2, 2), F32)
    p = _lib.Plane(C.c_void_p(a.ctypes.data), 2, 2, 0)
    pp = (_lib.Plane * 3)(p, p, p)
    by = C.c_void_p(np.zeros(12, np.uint8).ctypes.data)
    cfg = _lib.MaskedStretchConfigC(10, 0.25, 2.5, 4.0, 1, 0.85, 0.85, 1e-5)
    assert L.ab_arcsinh_stretch_rgb(None, C.byref(p), C.byref(p), C.byref(p), None, None, C.c_float(20.0), C.c_float(1.0), pp, None) == _lib.AB_ERR_INVALID
    assert L.ab_arcsinh_stretch_composite(None, C.byref(p), C.byref(p), C.byref(p), 20.0, None, None, 4096, pp, by, 0, None) == _lib.AB_ERR_INVALID
    assert L.ab_arcsinh_stretch_view(None, C.byref(p), 20.0, pp, by, 0, None) == _lib.AB_ERR_INVALID
    assert L.ab_masked_stretch_composite(None, C.byref(p), C.byref(p), C.byref(p), C.byref(cfg), 0, 4096, pp, by, 0, None) == _lib.AB_ERR_INVALID


def test_ctypes_mirrors_have_the_headers_layout(tmp_path):
    names = {"ab_arcsinh_composite_info": _lib.ArcsinhCompositeInfoC, "ab_arcsinh_view_info": _lib.ArcsinhViewInfoC,
             "ab_masked_stretch_composite_info": _lib.MaskedStretchCompositeInfoC}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "astroburst_hip.h"', 'int main(void) {']
    for n, cls in names.items():
        lines.append(f'    printf("{n} %zu", sizeof({n}));')
        for f, _ in cls._fields_:
            lines.append(f'    printf(" %zu", offsetof({n}, {f}));')
        lines.append('    printf("\\n");')
    lines.append("    return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for line in out:
        toks = line.split()
        cls = names[toks[0]]
        assert [int(t) for t in toks[1:]] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], toks[0]


# ---- the kernels' code ---------------------------------------------------------------------------------------------------------------
def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in base
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *base, "-w", "--save-temps", "-c", os.path.join(CSRC, "wizard_stretch.hip"), "-o",
                    os.path.join(tmp_path, "wizard_stretch.o")], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lst = open(os.path.join(tmp_path, "wizard_stretch-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_spill_count:\s+\d+", lst, re.S)}
    for family, count in (("range_kernel", 1), ("stretch_kernel", 11)):
        names = [n for n in meta if family in n]
        assert len(names) == count, (family, sorted(meta))
        for name in names:
            body = re.split(r"^%s:" % re.escape(name), lst, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[name]).group(1)) == 0, name
            assert "scratch_" not in body, name
            if family == "range_kernel":        # 16-byte loads; the wave's shuffles; one vector atomic per workgroup and word
                assert "global_load_dwordx4" in body and "global_atomic_umax" in body, name
                assert body.count("global_atomic_umax") == 1, name
    spills = re.findall(r"\.name:\s+(\S+)\n.*?\.vgpr_spill_count:\s+(\d+)", lst, re.S)
    assert len(spills) == 12 and all(int(n) == 0 for _, n in spills), spills
