"""warp_kernel_shared decides sharing first, on truncated coordinates (csrc/resample.hip, LABNOTES 37).  Its predicate, restated in
numpy (tests/warp_share_first_cases.py: truncating, saturating conversion; unsigned compares against bounds clamped at 0; scalar row
liveness), must mark exactly the waves the former predicate (warp_shared_cases.share_map: live, inside, interior, equal floor(sx),
consecutive floor(sy)) marks, for K = 2, 3, 4 -- then the address invariant of test_warp_shared_taps_predicate.py carries over
unchanged.  On every sharing lane truncation must equal the floor and s - floor(s) must be exact and below 1, because the shared path
takes its fractions from v_fract_f64."""
import numpy as np
import pytest

import warp_share_first_cases as sf
import warp_shared_cases as wc


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_same_waves_at_every_shape_and_band_of_the_shared_taps_test(case):
    _, make, _, _, _ = case
    for cols in wc.OUT_COLS:
        for rows in wc.OUT_ROWS:
            t = make((rows, cols))
            for row0 in sorted({0, 1, 2, 3, rows - 1}):
                for n in range(1, 6):
                    if row0 < rows and row0 + n <= rows:
                        sf.check_launch(t, wc.SRC_DIMS, cols, row0, n)
            sf.check_launch(t, wc.SRC_DIMS, cols, 0, rows)


def test_same_waves_for_random_routed_transforms_on_small_sources():
    """420 routed transforms: sources down to K + 2 rows and 3 columns (the clamped bounds are 0 there), offsets below 0, on 0 and 1,
    and beyond the int range; whole warps and row bands"""
    cases = sf.random_routed()
    assert len(cases) == 420
    shared = {K: 0 for K in wc.KS}
    for src, t, (rows, cols) in cases:
        for row0, n in [(0, rows)] + sf.bands_of(rows):
            for K, count in sf.check_launch(t, src, cols, row0, n).items():
                shared[K] += count
                assert count == 0 or (src[1] >= 4 and src[0] >= K + 3), (src, t, K)   # what the host's guard relies on
    assert all(shared[K] > 0 for K in wc.KS), shared   # (the sweep is not vacuous)


def test_gpu_cases_are_routed_and_some_share():
    """the inputs of test_gpu_warp_share_first.py: all routed to the kernel, same waves, and the shared path is reached on the sources
    that allow it"""
    shared = {K: 0 for K in wc.KS}
    for src in sf.GPU_SOURCES:
        for t in sf.gpu_transforms(src):
            assert wc.routed(t), t
            for rows, cols in sf.GPU_OUT_DIMS:
                for row0, n in [(0, rows)] + sf.bands_of(rows):
                    for K, count in sf.check_launch(t, src, cols, row0, n).items():
                        shared[K] += count
    assert all(shared[K] > 0 for K in wc.KS), shared


def test_same_waves_at_the_benchmark_size():
    """four of the benchmark's transforms at 4096^2, every pixel: the same waves, and still >= 95 % of them (the reference predicate
    alone leaves 2.0 - 3.3 % out)"""
    import bench
    R = C = 4096
    for t in bench.rigid_transforms(64, R, C)[::21]:
        assert wc.routed(t), t
        shared = sf.check_launch(t, (R, C), C, 0, R)
        for K in wc.KS:
            waves = -(-R // K) * (C // wc.WAVE)
            assert shared[K] >= 0.95 * waves, (t, K, shared[K], waves)
