"""CPU-side checks of the PSF estimation (no GPU): hand-worked cases of tests/psf_restatement.py (the checker of ab_estimate_psf),
ab_psf_select_stars and ab_psf_estimation_config_default through ctypes against it, and the conditions the fixtures of
tests/test_gpu_psf.py have to meet."""
import ctypes as C
import math

import numpy as np
import pytest

import psf_restatement as P


# ---- hand-worked cases of the restatement -------------------------------------------------------------------------------------------
def test_single_symmetric_star_centroid_and_subpixel_peak_by_hand():
    img = np.zeros((15, 17), np.float32)
    img[7, 8] = 10.0
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        img[7 + dy, 8 + dx] = 4.0
    for dy, dx in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        img[7 + dy, 8 + dx] = 1.0
    # symmetric about (8, 7): sum_w = 10 + 16 + 4 = 30, sum_x = 8 * 30, sum_y = 7 * 30 (all products are small integers: exact)
    assert P.centroid_subpixel(img, 8, 7, 3) == (8.0, 7.0)
    # dx = dy = 0, dxx = dyy = 4 + 4 - 20 = -12, dxy = 0, det = 144: sx = sy = -0.0, the peak is c itself
    assert P.subpixel_peak(img, 8, 7) == 10.0
    # an asymmetric neighbour: v(0, 1) = 6 -> dx_val = 1, dxx = -10, det = 120, sx = -(-12 * 1) / 120 = 0.1, peak = 10 + 0.5 * 0.1
    img[7, 9] = 6.0
    assert P.subpixel_peak(img, 8, 7) == 10.0 + 0.5 * (1.0 * (-(-12.0 * 1.0 - 0.0) / 120.0))
    assert abs(P.subpixel_peak(img, 8, 7) - 10.05) < 1e-15
    # on the border the pixel itself (:379-381)
    assert P.subpixel_peak(img, 0, 7) == float(img[7, 0])
    # a centroid window with no positive weight falls back to the pixel (:301-305)
    assert P.centroid_subpixel(np.zeros((9, 9), np.float32), 4, 4, 3) == (4.0, 4.0)


def test_bilinear_shift_of_a_delta_by_half_a_pixel():
    d = np.zeros((5, 5))
    d[2, 2] = 1.0
    out = P.bilinear_shift(d, 0.5, 0.0)   # result(x) samples the source at x - 0.5: the delta spreads over x = 2 and x = 3
    want = np.zeros((5, 5))
    want[2, 2] = want[2, 3] = 0.5
    assert np.array_equal(out, want)
    out = P.bilinear_shift(d, 0.0, -0.25)  # upwards by a quarter: 0.75 stays, 0.25 moves to row 1
    want = np.zeros((5, 5))
    want[2, 2], want[1, 2] = 0.75, 0.25
    assert np.array_equal(out, want)
    edge = np.zeros((3, 3))
    edge[0, 0] = 1.0
    assert P.bilinear_shift(edge, -0.5, -0.5)[0, 0] == 0.25   # zero outside the cutout


def test_middle_half_mean_on_a_known_annulus():
    # radius 10 around (12, 12) of a 25 x 25 plane whose value is the row index: the annulus 36 <= d2 <= 100 is symmetric about row 12
    img = np.repeat(np.arange(25, dtype=np.float32)[:, None], 25, axis=1)
    n = sum(1 for dy in range(-10, 11) for dx in range(-10, 11) if 36 <= dx * dx + dy * dy <= 100)
    vals = sorted(float(12 + dy) for dy in range(-10, 11) for dx in range(-10, 11) if 36 <= dx * dx + dy * dy <= 100)
    lo, hi = n // 4, max(3 * n // 4, n // 4 + 1)
    assert P.estimate_local_bg(img, 12, 12, 10) == sum(vals[lo:hi]) / (hi - lo)   # (small integers: any summation order is exact)
    # the slice rule on short lists (:435-436), lo = n / 4, hi = max(3 n / 4, lo + 1): 1 value -> itself; 2 -> the LOWER one
    # (lo = 0, hi = 1); 3 -> the lower two (hi = 2); 4 -> the middle two
    assert P.middle_half_mean([5.0]) == 5.0
    assert P.middle_half_mean([9.0, 1.0]) == 1.0
    assert P.middle_half_mean([3.0, 9.0, 1.0]) == 2.0
    assert P.middle_half_mean([4.0, 2.0, 8.0, 6.0]) == 5.0
    assert P.middle_half_mean([]) == 0.0


def test_score_star_on_given_numbers():
    s = P.Star(0.0, 0.0, 1.0, 1.0, fwhm=4.0, ellipticity=0.0, distance_from_center=0.0, snr=100.0)
    assert P.score_star(s) == 1.0 * 0.35 + 1.0 * 0.30 + 1.0 * 0.15 + 1.0 * 0.20
    s = P.Star(0.0, 0.0, 1.0, 1.0, fwhm=8.0, ellipticity=0.2, distance_from_center=500.0, snr=50.0)
    assert P.score_star(s) == 0.8 * 0.35 + 0.5 * 0.30 + 0.5 * 0.15 + 0.5 * 0.20
    s = P.Star(0.0, 0.0, 1.0, 1.0, fwhm=2.0, ellipticity=0.0, distance_from_center=0.0, snr=1e6)   # snr saturates at 1
    assert P.score_star(s) == 0.35 + 0.30 + 0.15 + (1.0 / 1.5) * 0.20


def test_stars_rejected_is_filtered_minus_cutouts_not_detected_minus_used():
    """the reference's quirk (:131): candidates.len() - count, where candidates is the FILTERED list and count the extracted cutouts"""
    img = P.field_a()
    r = P.estimate_psf(img, num_stars=8)
    assert r.error is None and len(r.stars_used) == 8 and r.cutouts_used == 8
    assert r.stars_rejected == r.stars_filtered - 8 and r.stars_filtered > 8 and r.stars_detected >= r.stars_filtered


# ---- the library's host-only entry points ----------------------------------------------------------------------------------------------
def _select(stars, max_val, rows, cols, **config):
    import astroburst_amd as ab
    return ab.psf_select_stars([s.astuple() for s in stars], max_val, rows, cols, **config)


def _cfg(**kw):
    return dict(P.DEFAULTS, **kw)


def test_config_defaults():
    from astroburst_amd import _lib
    cfg = _lib.PsfEstimationConfigC()
    _lib.lib().ab_psf_estimation_config_default(C.byref(cfg))
    got = {k: getattr(cfg, k) for k in P.DEFAULTS}
    assert got == P.DEFAULTS
    assert C.sizeof(_lib.PsfStarC) == 64 and C.sizeof(_lib.PsfEstimationConfigC) == 56


def test_select_stars_matches_the_restatement_on_measured_stars():
    img = P.field_a()
    st = P.image_stats(img)
    stars = []
    for (y, x) in P.detect_peaks(img, st["median"] + 5.0 * st["stddev"], 30):
        s, ok = P.measure_star(img, x, y)
        if ok:
            stars.append(s)
    assert len(stars) > 20
    for num in (1, 8, 30, 1000):   # (1000: num_stars larger than the list)
        want = P.select_stars(stars, st["max_val"], 192, 256, _cfg(num_stars=num))
        got = _select(stars, st["max_val"], 192, 256, num_stars=num)
        assert got == (want[0], want[1])
    assert len(_select(stars, st["max_val"], 192, 256, num_stars=1000)[0]) == P.select_stars(stars, st["max_val"], 192, 256, _cfg())[1]


def test_select_stars_keeps_equal_scores_in_input_order():
    base = dict(peak=50.0, flux=1.0, fwhm=4.0, ellipticity=0.1, distance_from_center=10.0, snr=80.0)
    stars = [P.Star(100.0 + i, 100.0, **base) for i in range(6)]
    stars[3] = P.Star(103.0, 100.0, **dict(base, ellipticity=0.05))   # the one better star goes first, the rest keep their order
    got, nf = _select(stars, 100.0, 300, 300)
    assert (got, nf) == ([3, 0, 1, 2, 4, 5], 6)
    assert (got, nf) == P.select_stars(stars, 100.0, 300, 300, _cfg())
    assert _select(stars, 100.0, 300, 300, num_stars=2)[0] == [3, 0]


@pytest.mark.parametrize("field,on,off", [
    # norm_peak = peak / 100: `< saturation_threshold` and `> min_peak_fraction` are strict
    ("peak", 94.0, 95.0), ("peak", 11.0, 10.0),
    # `ellipticity < max_ellipticity` and `distance < max_dist` are strict
    ("ellipticity", 0.29, 0.3), ("distance_from_center", 148.0, 0.7 * math.sqrt(150.0 * 150.0 + 150.0 * 150.0)),
    # x >= margin is inclusive, x < w - margin strict; the same for y
    ("x", 30.0, 29.999), ("x", 269.999, 270.0), ("y", 30.0, 29.999), ("y", 269.999, 270.0),
])
def test_select_stars_filter_boundaries(field, on, off):
    base = dict(x=150.0, y=150.0, peak=50.0, flux=1.0, fwhm=4.0, ellipticity=0.1, distance_from_center=10.0, snr=80.0)
    inside, outside = P.Star(**dict(base, **{field: on})), P.Star(**dict(base, **{field: off}))
    assert P.select_stars([inside, outside], 100.0, 300, 300, _cfg()) == ([0], 1)
    assert _select([inside, outside], 100.0, 300, 300) == ([0], 1)
    assert _select([outside, inside], 100.0, 300, 300) == ([1], 1)
    if field == "peak":   # the boundary value itself is computed as the reference computes it: peak / max_val against the f64 constant
        assert (off / 100.0 < 0.95) is False or (off / 100.0 > 0.10) is False


def test_select_stars_bad_arguments():
    from astroburst_amd import _lib
    L = _lib.lib()
    sel, flt = C.c_size_t(7), C.c_size_t(7)
    assert L.ab_psf_select_stars(None, 3, None, 1.0, 10, 10, None, 0, C.byref(sel), C.byref(flt)) == _lib.AB_ERR_INVALID
    cfg = _lib.PsfEstimationConfigC()
    L.ab_psf_estimation_config_default(C.byref(cfg))
    assert L.ab_psf_select_stars(None, 0, C.byref(cfg), 1.0, 10, 10, None, 0, C.byref(sel), C.byref(flt)) == _lib.AB_OK
    assert (sel.value, flt.value) == (0, 0)


# ---- the fixtures of tests/test_gpu_psf.py meet their conditions --------------------------------------------------------------------------
def test_fixture_a_integer_field_selects_eight_and_its_sums_are_exact():
    img = P.field_a()
    assert img.shape == (192, 256) and np.array_equal(img, np.rint(img))
    st = P.image_stats(img)
    assert st["sum_sq"] < 2.0 ** 53   # both sums exact in any order
    r = P.estimate_psf(img, num_stars=8)
    assert r.error is None and len(r.stars_used) == 8 and r.stars_detected >= 30


def test_fixture_b_inexact_sums_has_an_empty_guard_band():
    img = P.field_a() * np.float32(0.0137)
    assert img.dtype == np.float32 and not np.array_equal(img, np.rint(img))
    r = P.estimate_psf(img, num_stars=8)
    assert r.error is None and len(r.stars_used) == 8
    assert P.guard_band_empty(img, r.threshold)
    assert not P.guard_band_empty(np.array([[r.threshold * (1 + 5e-10)]]), r.threshold)   # (the helper does see a pixel inside the band)


def test_fixture_c_ties_follow_raster_order():
    img, planted = P.field_c()
    st = P.image_stats(img)
    thr = st["median"] + 5.0 * st["stddev"]
    wm = P.window_max(img, 5)
    for (y, x) in [planted["core_first"]] + planted["core_rest"] + planted["kept"] + planted["suppressed"]:
        assert img[y, x] >= thr and img[y, x] == wm[y, x], (y, x)   # every planted pixel is a candidate: an exact tie
    peaks = P.detect_peaks(img, thr, 20)
    assert planted["core_first"] in peaks and not any(p in peaks for p in planted["core_rest"])
    assert all(p in peaks for p in planted["kept"]) and not any(p in peaks for p in planted["suppressed"])
    assert img[92, 123] == img[90, 126]   # the survivor of this pair is the one first in raster order, not a brighter one
    r = P.estimate_psf(img, edge_margin=20, num_stars=6)
    assert r.error is None and r.stars_detected >= 8


@pytest.mark.parametrize("variant", [1, 2])
def test_fixture_d_odd_shape_reaches_the_margins_and_the_border(variant):
    img, cfg = P.field_d(variant)
    assert img.shape == (131, 197) and cfg["cutout_radius"] == 7
    m = cfg["edge_margin"]
    r = P.estimate_psf(img, **cfg)
    assert r.error is None
    ys, xs = [p[0] for p in r.peaks], [p[1] for p in r.peaks]
    assert min(ys) == m and max(ys) == 131 - 1 - m and min(xs) == m and max(xs) == 197 - 1 - m
    clipped_annulus = False
    for (y, x) in r.peaks:
        s, _ = P.measure_star(img, x, y)
        clipped_annulus |= s.y - 3.0 * s.fwhm < 0.0
    assert clipped_annulus
    if variant == 1:
        assert r.cutouts_used == len(r.stars_used)
    else:
        assert m < cfg["cutout_radius"] and min(ys) < 12            # the 25 x 25 window leaves the image
        assert 0 < r.cutouts_used < len(r.stars_used)               # extract_cutout returned None for a selected star


def test_fixture_e_large_annuli():
    img = P.field_e()
    r = P.estimate_psf(img, num_stars=8)
    assert r.error is None
    assert (215, 215) in r.peaks and (60, 70) in r.peaks
    a, ok_a = P.measure_star(img, 215, 215)
    b, ok_b = P.measure_star(img, 70, 60)
    assert 17.0 < a.fwhm < 19.0 and ok_a and a.x + 3.0 * a.fwhm > 255.0          # kept; its annulus leaves the image
    assert 23.0 < b.fwhm < 25.0 and not ok_b and b.snr > 10.0                     # rejected by `fwhm < 20` alone
    assert b.y - 3.0 * b.fwhm < 0.0 and P.annulus_count(img, b.x, b.y, 2.0 * b.fwhm, 3.0 * b.fwhm) > 8000


def test_fixture_f_negative_pixels_still_select_stars():
    a = P.field_a()
    img = a - np.float32(np.median(a))
    assert (img < 0).mean() > 0.4
    r = P.estimate_psf(img, num_stars=8)
    assert r.error is None and len(r.stars_used) == 8


def test_fixture_g_outcomes():
    assert P.estimate_psf(P.field_noise(), edge_margin=16).error == P.ERR_NO_STARS
    r = P.estimate_psf(P.field_saturated(), edge_margin=20)
    assert r.error == P.ERR_NO_PASS and r.stars_detected == 4
    flat = np.full((96, 128), 7.0, np.float32)
    st = P.image_stats(flat)
    assert st["stddev"] == 0.0 and st["median"] == 7.0   # threshold = the constant: every pixel inside the margins is a candidate
    assert P.estimate_psf(flat, edge_margin=16).error is not None
