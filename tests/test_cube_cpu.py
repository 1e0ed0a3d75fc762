"""The spectral-cube entry points, as far as they can be held without a GPU: the numpy restatement of core/cube/{eager,lazy}.rs
(tests/cube_restatement.py) on hand-worked columns, its rank arithmetic, the host-only ab_cube_streaming_step through ctypes, the
fixtures the GPU tests share, and the distance between the two forms of the normalisation on the GPU tests' inputs."""
import ctypes

import numpy as np
import pytest

import cube_restatement as R

F32 = np.float32
NAN = np.nan


def _col(values):
    return np.array(values, F32).reshape(-1, 1, 1)


def test_hand_worked_columns():
    col = _col([3, 0, NAN, -1, 2])
    # rule 0 (finite && != 0): the samples are 3, -1, 2 -> sorted -1, 2, 3 -> [3 / 2] = 2; mean 4 / 3 in f64, rounded to f32
    assert R.collapse_median(col, R.NONZERO)[0, 0] == F32(2)
    assert R.bits(R.collapse_mean(col, R.NONZERO))[0, 0] == R.bits(F32(np.float64(4.0) / np.float64(3.0)))[0]
    # rule 1 (finite && > 1e-7): the samples are 3, 2 -> sorted 2, 3 -> [2 / 2] = 3; mean 2.5
    assert R.collapse_median(col, R.ABOVE_PADDING)[0, 0] == F32(3)
    assert R.collapse_mean(col, R.ABOVE_PADDING)[0, 0] == F32(2.5)
    for rule in (R.NONZERO, R.ABOVE_PADDING):
        dead = _col([0.0, -0.0, NAN, np.inf, -np.inf])
        assert R.bits(R.collapse_median(dead, rule))[0, 0] == 0 and R.bits(R.collapse_mean(dead, rule))[0, 0] == 0
    # the two rules part on the values around the padding threshold
    edge = _col([1e-8, 1e-7, np.nextafter(F32(1e-7), F32(1))])
    assert R.valid(edge, R.NONZERO).sum() == 3 and R.valid(edge, R.ABOVE_PADDING).sum() == 1
    # the mean's additions happen in z order in f64: 1e8 + 1 - 1e8 is 1 in f64 and would be 0 in f32
    assert R.collapse_mean(_col([1e8, 1.0, -1e8]), R.NONZERO)[0, 0] == F32(1.0 / 3.0)


@pytest.mark.parametrize("depth,want", [(1, 1), (32, 1), (33, 1), (63, 1), (64, 2), (100, 3), (3000, 93)])
def test_streaming_step_through_the_library(depth, want):
    """ab_cube_streaming_step is host-only scalar maths (lazy.rs:334-335): no context, no GPU"""
    from astroburst_amd import _lib
    L = _lib.lib()
    L.ab_cube_streaming_step.argtypes = [ctypes.c_int64]
    L.ab_cube_streaming_step.restype = ctypes.c_uint64
    assert L.ab_cube_streaming_step(depth) == want
    assert R.streaming_step(depth) == want


def test_streaming_step_python_wrapper():
    from astroburst_amd.core import Context, cube_streaming_step
    assert [cube_streaming_step(d) for d in (1, 64, 3000)] == [1, 2, 93]
    assert Context.cube_streaming_step(100) == 3


@pytest.mark.parametrize("n,want", [(1, (0, 0, 0)), (3, (1, 0, 2)), (100, (50, 1, 99)), (1000, (500, 10, 999))])
def test_rank_arithmetic(n, want):
    """n / 2, (n as f64 * 0.01) as usize, min((n as f64 * 0.999) as usize, n - 1): 100 * 0.999 = 99.9 -> 99, 1000 * 0.999 = 999"""
    assert R.stat_ranks(n) == want
    v = np.arange(n, dtype=F32) - F32(n // 3) + F32(0.5)              # distinct signed values, none zero
    (median, sigma, low, high), count = R.global_stats(v.reshape(n, 1, 1), R.NONZERO)
    s = np.sort(v)
    assert count == n and (median, low, high) == (s[want[0]], s[want[1]], s[want[2]])
    d = np.sort(np.abs(v - median))
    assert sigma == max(F32(d[n // 2] * F32(1.4826)), F32(1e-10))


def test_global_stats_defaults_and_stepping():
    assert R.global_stats(np.zeros((3, 2, 2), F32), R.NONZERO) == ((0, 1, 0, 1), 0)
    c = R.poisoned_frames_cube((7, 5, 6), 3)
    assert R.global_stats(c, R.NONZERO, 3) == R.global_stats(c[::3], R.NONZERO, 1)
    assert R.global_stats(c, R.NONZERO, 3)[0][3] < F32(1e30) < R.global_stats(c, R.NONZERO, 1)[0][3]


def test_pairs_are_the_select_tests_pairs_with_the_sign_bit():
    import select_adversarial as SA
    for name, (lo, hi) in R.PAIRS.items():
        assert (R.from_bits(lo), R.from_bits(hi)) == SA.PAIRS[name][:2]
    for shape in R.STATS_SHAPES:
        for name, cube in R.stats_populations(shape):
            if "-neg-" in name:
                v = cube[R.valid(cube, R.NONZERO)]
                assert v.size and (v < 0).all() and np.unique(v).size <= 2, name
    big, lower, upper = R.big_two_valued_cube()
    assert R.global_stats(big, R.NONZERO)[0][0] == lower and big[0, 0, 0] == lower and big[0, 0, -1] == lower
    assert R.global_stats(big[:, :, 1:], R.NONZERO)[0][0] == upper == R.global_stats(big[:, :, :-1], R.NONZERO)[0][0]


def test_adversarial_columns_hold_what_they_claim():
    for depth in R.ADVERSARIAL_DEPTHS:
        cube, names = R.adversarial_cube(depth)
        assert cube.shape == (depth, 1, len(names)) and names[-1] == "one_valid"
        for rule in (R.NONZERO, R.ABOVE_PADDING):
            med, mean = R.collapse_median(cube, rule), R.collapse_mean(cube, rule)
            lost = cube.copy()
            lost[-1, 0, -1] = NAN                                        # the cube's last voxel
            if rule == R.NONZERO:
                assert med[0, -1] == F32(-2.5) == mean[0, -1] and R.collapse_median(lost, rule)[0, -1] == 0
            j = names.index("subnormals")
            assert rule == R.NONZERO or med[0, j] == 0                   # no subnormal passes the padding threshold
        if depth >= 4:
            assert all(not np.isfinite(cube[:, 0, j]).all() for j in range(len(names)))
        if depth >= 255:
            assert all(np.isnan(cube[:, 0, j]).any() and np.isinf(cube[:, 0, j]).any() for j in range(len(names)))
            j = names.index("thresholds")
            assert R.collapse_median(cube, R.NONZERO)[0, j] != R.collapse_median(cube, R.ABOVE_PADDING)[0, j]
            j = names.index("middle_in_two_bins")
            v = np.sort(cube[:, 0, j][R.valid(cube[:, 0, j], R.NONZERO)])
            if v.size % 2 == 0:
                assert R.bits(v[v.size // 2 - 1]) >> 24 != R.bits(v[v.size // 2]) >> 24


def test_the_f32_formula_stays_within_2_ulp_of_the_definition():
    """Rust's f32::asinh evaluated in numpy f32 against the definition (f64 asinh rounded once), on the inputs the GPU test uses.
    Its bits depend on the libm, which is why it is not the target; 2 ulp is the distance the C header promises."""
    worst, differ, total = 0, 0, 0
    for shape in R.NORMALIZE_SHAPES:
        for name, frame, stats in R.normalize_cases(shape):
            want = R.normalize_definition(frame, stats)
            d = R.ulp_distance(R.normalize_f32_formula(frame, stats), want)
            worst, differ, total = max(worst, int(d.max())), differ + int((d > 0).sum()), total + d.size
    print(f"f32 formula vs definition: max {worst} ulp, {differ} of {total} values differ ({100.0 * differ / total:.2f} %)")
    assert worst <= 2


def test_the_two_f64_forms_of_the_definition_agree():
    """numpy's arcsinh and the log1p form, both in f64 and rounded once: at most 2 values per 2^21 may differ (double rounding)"""
    for shape in R.NORMALIZE_SHAPES:
        for name, frame, stats in R.normalize_cases(shape):
            a, b = R.normalize_definition(frame, stats), R.normalize_definition_log1p(frame, stats)
            assert R.ulp_distance(a, b).max() <= 1
            assert int((R.bits(a) != R.bits(b)).sum()) <= 2 * max(1, -(-a.size // (1 << 21))), name


def test_frame_bytes_by_hand():
    # min -1, max 3 -> inv = 63.75; 1e-7 and everything below it renders 0 whatever its scaled value
    v = np.array([[-1.0, 0.0, 1e-7, 1.0, 3.0, NAN]], F32)
    assert R.frame_bytes(v).tolist() == [[0, 0, 0, 127, 255, 0]]
    assert R.frame_bytes(np.zeros((2, 3), F32)).tolist() == [[0, 0, 0], [0, 0, 0]]
    cube = R.export_cube((7, 33, 65))
    stats, _ = R.global_stats(cube, R.NONZERO)
    out = R.export_frames(cube, stats, 3)
    assert out.shape == (3, 33, 65) and not out[0].max() == 0
    assert R.export_frames(cube, stats, 1)[1].max() == 0                # the all-non-finite frame


def test_rust_cube_struct_takes_the_const_pointer_the_wrappers_give_it():
    """the header declares `const float *data`; bindings/mod.rs fills it from `as_ptr()` (a `*const f32`), which Rust does not coerce
    to `*mut`: the generated struct must say `*const f32` (tools/gen_rust_sys.py's const rule), or the wrappers do not compile"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys_rs = open(os.path.join(root, "bindings", "sys.rs")).read()
    body = re.search(r"pub struct ab_cube \{(.*?)\n\}", sys_rs, re.S).group(1)
    assert re.search(r"pub data: \*const f32,", body), body
