"""tests/crop_restatement.py (the checker of tests/test_gpu_crop.py) against hand-computed cases of cmd/compose/crop.rs, and its
vectorised detection against its literal loops.  No GPU."""
import numpy as np
import pytest

import crop_restatement as R

F32 = np.float32
BOTH = (R.detect_valid_region_loops, R.detect_valid_region)


@pytest.mark.parametrize("detect", BOTH, ids=["loops", "vectorised"])
def test_an_empty_plane_gives_rows_0_cols_0(detect):
    for shape in ((1, 1), (3, 5), (7, 1), (1, 7)):
        assert detect(np.zeros(shape, F32), 1e-6) == (shape[0], 0, shape[1], 0)


@pytest.mark.parametrize("detect", BOTH, ids=["loops", "vectorised"])
def test_a_single_valid_pixel(detect):
    shape = (5, 9)
    for r, c in ((0, 0), (0, 8), (4, 0), (4, 8), (2, 3)):
        assert detect(R.single(shape, r, c), 1e-6) == (r, r + 1, c, c + 1)
    assert detect(R.single((1, 1), 0, 0), 1e-6) == (0, 1, 0, 1)


@pytest.mark.parametrize("detect", BOTH, ids=["loops", "vectorised"])
def test_two_pixels_span_the_box(detect):
    a = R.single((6, 8), 1, 5)
    a[4, 2] = -3.0
    assert detect(a, 1e-6) == (1, 5, 2, 6)


@pytest.mark.parametrize("detect", BOTH, ids=["loops", "vectorised"])
def test_the_test_is_strict_and_in_f32(detect):
    thr = F32(0.25)
    assert detect(R.single((3, 3), 1, 1, thr), thr) == (3, 0, 3, 0)            # |v| == threshold is not valid
    assert detect(R.single((3, 3), 1, 1, -thr), thr) == (3, 0, 3, 0)
    assert detect(R.single((3, 3), 1, 1, np.nextafter(thr, F32(1))), thr) == (1, 2, 1, 2)
    # f32(0.1) lies above the f64 0.1: the pixel equals the f32 threshold and is not valid (it would be in an f64 comparison)
    assert detect(R.single((3, 3), 1, 1, F32(0.1)), 0.1) == (3, 0, 3, 0)
    assert detect(R.single((3, 3), 1, 1, F32(1e-6)), 1e-6) == (3, 0, 3, 0)


@pytest.mark.parametrize("detect", BOTH, ids=["loops", "vectorised"])
def test_special_pixels(detect):
    shape = (4, 4)
    assert detect(R.single(shape, 2, 1, np.nan), 1e-6) == (4, 0, 4, 0)         # NaN is never valid
    assert detect(R.single(shape, 2, 1, np.inf), 1e-6) == (2, 3, 1, 2)
    assert detect(R.single(shape, 2, 1, -np.inf), 1e-6) == (2, 3, 1, 2)
    assert detect(np.full(shape, -0.0, F32), 0.0) == (4, 0, 4, 0)              # |-0.0| > 0.0 is false
    assert detect(np.full(shape, -0.0, F32), -1.0) == (0, 4, 0, 4)             # valid only for a negative threshold


@pytest.mark.parametrize("detect", BOTH, ids=["loops", "vectorised"])
def test_special_thresholds(detect):
    a = R.noise((4, 6), 1)
    a[0, 0], a[3, 5] = np.inf, -np.inf
    assert detect(a, np.nan) == (4, 0, 6, 0)                                    # a NaN threshold: nothing
    assert detect(a, np.inf) == (4, 0, 6, 0)                                    # inf > inf is false
    z = np.zeros((4, 6), F32)
    z[:, 0] = np.nan
    assert detect(z, -1.0) == (0, 4, 1, 6)                                      # negative: every non-NaN pixel
    assert detect(np.full((2, 2), np.nan, F32), -1.0) == (2, 0, 2, 0)


def test_crop_array_clamps_as_the_reference():
    a = R.noise((6, 7), 2)
    assert np.array_equal(R.crop_array(a, 1, 5, 2, 6), a[1:5, 2:6])
    assert np.array_equal(R.crop_array(a, 0, 99, 0, 99), a)                    # larger than the plane
    assert R.crop_array(a, 9, 12, 0, 7).shape == (0, 7)                        # top past the plane
    assert R.crop_array(a, 4, 2, 5, 1).shape == (0, 0)                         # bottom < top, right < left
    assert R.crop_array(a, 2, 2, 0, 7).shape == (0, 7)
    assert R.clamp_box((6, 7), 4, 2, 5, 1) == (4, 4, 5, 5)


def test_auto_mode_intersects_and_reports():
    a = R.bordered((10, 12), (2, 1, 3, 0), 3)
    b = R.bordered((10, 12), (0, 3, 1, 2), 4)
    plan = R.crop_channels_plan([a, b])
    assert plan.crop_box == (2, 7, 3, 10) and (plan.out_rows, plan.out_cols) == (5, 7)
    assert (plan.actual_top, plan.actual_bottom, plan.actual_left, plan.actual_right) == (2, 3, 3, 2)
    assert plan.auto_detected and plan.out_dims == ((5, 7), (5, 7))
    cropped, _ = R.crop_channels([a, b], plan)
    assert np.array_equal(cropped[0], a[2:7, 3:10]) and np.array_equal(cropped[1], b[2:7, 3:10])


def test_auto_mode_with_disjoint_boxes_raises_the_references_message():
    a, b = R.single((8, 8), 1, 1), R.single((8, 8), 6, 6)
    with pytest.raises(ValueError, match=R.NO_OVERLAP):
        R.crop_channels_plan([a, b])
    with pytest.raises(ValueError, match=R.NO_OVERLAP):
        R.crop_channels_plan([np.zeros((4, 4), F32)])                          # (4, 0, 4, 0)
    c = R.single((8, 8), 1, 6)                                                  # rows overlap, columns touch: right <= left
    with pytest.raises(ValueError, match=R.NO_OVERLAP):
        R.crop_channels_plan([R.single((8, 8), 1, 5), c])
    with pytest.raises(ValueError, match=R.NO_PATHS):
        R.crop_channels_plan([])


def test_manual_margins_saturate_and_have_no_emptiness_check():
    a = R.noise((6, 8), 5)
    plan = R.crop_channels_plan([a], auto_detect=False, top=1, bottom=2, left=3, right=1)
    assert plan.crop_box == (1, 4, 3, 7) and plan.out_dims == ((3, 4),) and not plan.auto_detected
    assert (plan.actual_top, plan.actual_bottom, plan.actual_left, plan.actual_right) == (1, 2, 3, 1)
    plan = R.crop_channels_plan([a], auto_detect=False, top=9, bottom=50, left=2, right=50)      # margins larger than the plane
    assert plan.crop_box == (9, 0, 2, 0) and plan.out_dims == ((0, 0),)
    assert (plan.actual_top, plan.actual_bottom, plan.actual_left, plan.actual_right) == (9, 6, 2, 8)
    cropped, _ = R.crop_channels([a], plan)
    assert cropped[0].shape == (0, 0)


def test_planes_of_different_dims_give_per_plane_outputs(oracle):
    a, b, c = R.noise((8, 10), 6), R.noise((5, 12), 7), R.noise((9, 4), 8)
    plan = R.crop_channels_plan([a, b, c], auto_detect=False, top=1, bottom=1, left=2, right=3)
    assert plan.crop_box == (1, 7, 2, 7) and plan.out_dims == ((6, 5), (4, 5), (6, 2))
    cropped, stats = R.crop_channels([a, b, c], plan, oracle)
    assert np.array_equal(cropped[1], b[1:5, 2:7]) and np.array_equal(cropped[2], c[1:7, 2:4])
    assert stats[2] == R.stats_row(oracle.compute_image_stats(c[1:7, 2:4]))
    auto = R.crop_channels_plan([a, b, c])                                      # each measured with its own dims
    assert auto.crop_box == (0, 5, 0, 4) and auto.out_dims == ((5, 4), (5, 4), (5, 4))
    empty = R.crop_channels_plan([a], auto_detect=False, top=20)
    assert R.crop_channels([a], empty, oracle)[1] == [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0)]


def test_the_literal_loops_and_the_vectorised_form_agree():
    rng = np.random.default_rng(11)
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-6, -1e-6, 2e-6, 0.5, -0.5], F32)
    for k in range(300):
        rows, cols = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        a = specials[rng.integers(0, specials.size, (rows, cols))]
        a[rng.random((rows, cols)) < rng.random()] = 0.0                        # from almost empty to almost full
        thr = [1e-6, 0.0, -1.0, np.nan, np.inf, 0.5][k % 6]
        assert R.detect_valid_region_loops(a, thr) == R.detect_valid_region(a, thr), (a, thr)
