"""The shared path of warp_kernel_shared (csrc/resample.hip) forms no address outside the taps the per-pixel sampler would load --
checked where it can be checked without a GPU.

The kernel's wave-wide sharing predicate is restated in numpy (tests/warp_shared_cases.py).  For every wave and every group height
K in {2, 3, 4} where it holds, the rectangle the shared path walks -- source rows iy_0 - 1 .. iy_0 + K + 1, columns ix_0 - 1 ..
ix_0 + 2 of every lane -- must lie inside the source AND inside ab_warp_source_rows of the group's own band of K output rows: the
row-band entry point hands the kernel a base pointer moved back by the band's first source row with only that hull behind it, so a
row outside it is a memory fault.  Over the GPU test's transforms at its shapes, and over transforms of the benchmark at 4096^2
(every pixel; the transforms are subsampled)."""
import ctypes as C

import numpy as np
import pytest

import warp_shared_cases as wc


def source_rows(t, src_rows, src_cols, out_cols, row0, nrows):
    """ab_warp_source_rows of the library itself (host code: no GPU is needed)"""
    from astroburst_amd import _lib
    s0, sn = C.c_int64(), C.c_int64()
    tt = (C.c_double * 6)(*[float(v) for v in t])
    assert _lib.lib().ab_warp_source_rows(tt, src_rows, src_cols, out_cols, row0, nrows, C.byref(s0), C.byref(sn)) == 0
    return s0.value, sn.value


def check_launch(t, src_dims, out_cols, row0, nrows, classes=None):
    """every sharing wave of the launch for rows [row0, row0 + nrows), K = 2, 3, 4 -> the number of sharing waves per K"""
    src_rows, src_cols = src_dims
    classes = classes or wc.pixel_classes(t, src_rows, src_cols, out_cols, row0, nrows)
    shared = {}
    for K in wc.KS:
        share, _, ix0, iy0 = wc.share_map(classes, K)
        shared[K] = int(share.sum())
        lanes = np.repeat(share, wc.WAVE, axis=1)[:, :out_cols]               # [groups, cols]: the lane's wave shares
        assert lanes.sum() == shared[K] * wc.WAVE                              # (a sharing wave has no dead lane)
        if not shared[K]:
            continue
        big = np.iinfo(np.int64).max
        first_row = np.where(lanes, iy0 - 1, big).min(axis=1)                  # per group, over its sharing lanes
        last_row = np.where(lanes, iy0 + K + 1, -big).max(axis=1)
        first_col = np.where(lanes, ix0 - 1, big).min()
        last_col = np.where(lanes, ix0 + 2, -big).max()
        assert 0 <= first_col and last_col < src_cols, (t, K, first_col, last_col)
        for g in np.nonzero(lanes.any(axis=1))[0]:
            lo, hi = int(first_row[g]), int(last_row[g])
            assert 0 <= lo and hi < src_rows, (t, K, g, lo, hi)
            s0, sn = source_rows(t, src_rows, src_cols, out_cols, row0 + K * int(g), K)
            assert s0 <= lo and hi < s0 + sn, (t, K, int(g), (lo, hi), (s0, sn))
    return shared


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_shared_rectangle_inside_source_and_hull_at_the_test_shapes(case):
    name, make, _, _, is_routed = case
    for cols in wc.OUT_COLS:
        for rows in wc.OUT_ROWS:
            t = make((rows, cols))
            assert wc.routed(t) == is_routed, (name, t)
            for row0 in sorted({0, 1, 2, 3, rows - 1}):
                for n in range(1, 6):
                    if row0 < rows and row0 + n <= rows:
                        check_launch(t, wc.SRC_DIMS, cols, row0, n)
            check_launch(t, wc.SRC_DIMS, cols, 0, rows)


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_cases_populate_the_class_they_are_named_for(case):
    """at 67 rows, both widths, every K: some wave shares in (a), (b), (c); some sampling wave does not in (b), (d), (e), (f); none
    can in (g)"""
    name, make, must_share, must_not_share, is_routed = case
    for cols in wc.OUT_COLS:
        out = (wc.POPULATED_AT[0], cols)
        t = make(out)
        for K in wc.KS:
            sharing, not_sharing = wc.counts(t, wc.SRC_DIMS, out, K)
            if must_share is True:
                assert sharing > 0, (name, cols, K)
            if must_share is False and name.startswith("g"):
                assert sharing == 0 and not wc.routed(t), (name, cols, K, sharing)
            if must_not_share:
                assert not_sharing > 0, (name, cols, K)


def test_shared_rectangle_inside_source_and_hull_at_the_benchmark_size():
    """four of the benchmark's transforms (the identity among them) at 4096^2, every pixel, one launch for the whole image; the
    shared path must also be the usual one there, or the kernel is of no use"""
    import bench
    R = C_ = 4096
    ts = bench.rigid_transforms(64, R, C_)
    for t in ts[::21]:
        assert wc.routed(t), t
        shared = check_launch(t, (R, C_), C_, 0, R)
        for K in wc.KS:
            waves = -(-R // K) * (C_ // wc.WAVE)
            assert shared[K] >= 0.95 * waves, (t, K, shared[K], waves)
