"""The fixtures of tests/masked_adversarial.py held to what they claim, without a GPU.

  parity       on every fixture oracle/orc_masked.c equals tests/masked_restatement.py exactly (masks, planes, counts, backgrounds)
  conditions   every family contains what it exists for (lattice points on both radii, coverage strictly inside (0, 1), loops that
               stop beyond the first chunk of 32 iterations, planes that leave [0, 1] before the clamp, subnormal medians, ...)
  sensitivity  the restatement under each mutation differs from itself on the family that exists to catch that mutation

No tolerance anywhere: planes through their uint32 views (a NaN equal to a NaN), scalars with ==."""
import numpy as np
import pytest

import masked_adversarial as MA
import masked_restatement as mr

F = np.float32
MASK_CASES = MA.mask_cases()
STRETCH_CASES = MA.stretch_cases()
RGB_CASES = MA.rgb_cases()
_mask, _stretch = {}, {}


def mask_of(case, mutation=""):
    k = (case.name, mutation)
    if k not in _mask:
        _mask[k] = mr.star_mask_from_stars(case.image, list(case.stars), mutation=mutation, **case.cfg)
    return _mask[k]


def stretch_of(case, mutation=""):
    k = (case.name, mutation)
    if k not in _stretch:
        _stretch[k] = mr.masked_stretch_with_mask(case.image, case.mask, mutation=mutation, return_unclamped=True, **case.cfg)
    return _stretch[k]


def by_name(cases, prefix):
    found = [c for c in cases if c.name.startswith(prefix)]
    assert found, prefix
    return found


def ids(cases):
    return [c.name for c in cases]


def test_fixtures_are_small_named_once_and_read_only():
    names = [c.name for c in MASK_CASES + STRETCH_CASES + RGB_CASES]
    assert len(set(names)) == len(names)
    for c in MASK_CASES + STRETCH_CASES:
        assert not c.image.flags.writeable
        assert c.image.shape == MA.BIG_SHAPE if c.name.endswith("-big") or "-big-" in c.name else c.image.size <= 65 * 257, c.name
    for fam in ("S-shapes", "M-long", "M-clamp", "RGB-"):
        cases = [c for c in MASK_CASES + STRETCH_CASES + RGB_CASES if c.name.startswith(fam)]
        assert sum(getattr(c, "image", getattr(c, "r", None)).shape == MA.BIG_SHAPE for c in cases) == 1, fam


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MASK_CASES, ids=ids(MASK_CASES))
def test_oracle_mask_equals_the_restatement(oracle, case):
    want_mask, want_n, want_cov = mask_of(case)
    got = oracle.generate_star_mask(case.image, stars=list(case.stars), **case.cfg)
    assert got.stars_masked == want_n
    assert got.coverage_fraction == want_cov
    assert MA.same_planes(got.mask, want_mask)
    assert not np.isnan(want_mask).any() and (want_mask >= 0).all() and (want_mask <= 1).all()


@pytest.mark.parametrize("case", STRETCH_CASES, ids=ids(STRETCH_CASES))
def test_oracle_stretch_equals_the_restatement(oracle, case):
    want, iters, final_bg, conv, _ = stretch_of(case)
    got = oracle.masked_stretch(case.image, mask=oracle.StarMaskResult(case.mask, case.stars_masked, case.coverage), **case.cfg)
    assert (got.iterations_run, got.final_background, got.converged) == (iters, final_bg, conv)
    assert MA.same_planes(got.image, want)


@pytest.mark.parametrize("case", RGB_CASES, ids=ids(RGB_CASES))
def test_oracle_shared_mask_equals_the_restatement_and_finds_no_star(oracle, case):
    *chans, shared = oracle.masked_stretch_rgb_shared(case.r, case.g, case.b, **case.cfg)
    assert shared.stars_masked == 0                                                 # the condition that makes the family exact
    assert 0.0 < shared.coverage_fraction < 1.0                                     # ... and the luminance protection fills the mask
    lum = mr.luminance(case.r, case.g, case.b)
    mask, n, cov = mr.star_mask_from_stars(lum, [], luminance_protect=True, luminance_ceiling=case.cfg.get("luminance_ceiling", 0.85))
    assert n == 0 and cov == shared.coverage_fraction and MA.same_planes(mask, shared.mask)
    for got, plane in zip(chans, (case.r, case.g, case.b)):
        cfg = {k: v for k, v in case.cfg.items() if k != "luminance_ceiling"}
        want, iters, final_bg, conv = mr.masked_stretch_with_mask(plane, mask, **cfg)
        assert (got.iterations_run, got.final_background, got.converged) == (iters, final_bg, conv)
        assert MA.same_planes(got.image, want)
        assert (got.stars_masked, got.mask_coverage) == (0, cov)


def test_shared_mask_families_are_what_they_are_for(oracle):
    counts = {}
    for case in RGB_CASES:
        *chans, _ = oracle.masked_stretch_rgb_shared(case.r, case.g, case.b, **case.cfg)
        counts[case.name] = [c.iterations_run for c in chans]
        if case.name == "RGB-mixed":                                                # G has no valid pixel, B's are all equal
            for c in chans[1:]:
                assert not c.image.any() and c.final_background == 0.0 and not c.converged
            assert chans[0].image.any()
    assert counts["RGB-starless-t0"] == [40, 40, 40]
    assert any(len(set(v)) > 1 for v in counts.values()), counts                    # the three chains do not always stop together


# ---- conditions: star mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", by_name(MASK_CASES, "S-shapes"), ids=ids(by_name(MASK_CASES, "S-shapes")))
def test_shapes_hold_what_they_claim(case):
    h, w = case.image.shape
    mask, n, cov = mask_of(case)
    kept = [s for s in case.stars if case.cfg["min_fwhm"] <= s[2] <= case.cfg["max_fwhm"]]
    assert n == len(kept)
    if case.group in ("border", "all"):
        lo, hi = case.cfg["min_fwhm"], case.cfg["max_fwhm"]
        fw = [s[2] for s in case.stars]
        assert lo in fw and hi in fw and any(f != f for f in fw)                    # exactly on the bounds: kept; NaN: dropped
        assert any(f < lo and np.nextafter(f, np.inf) == lo for f in fw) and any(f > hi and np.nextafter(f, -np.inf) == hi for f in fw)
        assert len(case.stars) - n == 3
        assert mask[0, 0] == 1 and mask[0, w - 1] == 1 and mask[h - 1, 0] == 1 and mask[h - 1, w - 1] == 1
    if case.group in ("cluster", "all"):
        x0, y0 = max(0, w - 32), max(0, h - 30)
        assert sum(1 for s in case.stars if s[2] <= 3.0 and x0 <= s[0] <= x0 + 24 and y0 <= s[1] <= y0 + 24) >= 200
    if case.lattice and min(h, w) >= 16:
        lx, ly, r2_inner, r2_outer = case.lattice
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        d2 = (xx - lx) ** 2 + (yy - ly) ** 2                                         # f64, exact on integers
        assert (d2 == r2_inner).sum() >= 6 and (d2 == r2_outer).sum() >= 2
        assert (r2_inner, r2_outer) == ((25.0, 81.0) if case.cfg["softness"] == 4.0 else (25.0, 25.0))
    if min(h, w) >= 16 and not (case.group in ("cluster", "all") and (h, w) == (16, 16)):
        # (a 24 x 24 cluster covers a 16 x 16 plane whole: the one combination that cannot stay below 1)
        assert 0.0 < cov < 1.0, cov
        assert (mask == 1).any() and (mask == 0).any()
        if case.cfg["softness"] > 0:
            assert ((mask > 0) & (mask < 1)).any()
    if (h, w) == (40, 60) and case.group == "discs":
        whole = case.stars[-1]
        sr = whole[2] * 2.5 + case.cfg["softness"]
        if case.cfg["softness"] > 0:
            assert np.floor(whole[0] - sr) <= 0 and np.ceil(whole[0] + sr) >= w - 1 and np.floor(whole[1] - sr) <= 0 and np.ceil(whole[1] + sr) >= h - 1


@pytest.mark.parametrize("case", by_name(MASK_CASES, "S-nonfinite"), ids=ids(by_name(MASK_CASES, "S-nonfinite")))
def test_nonfinite_stars_hold_what_they_claim(case):
    mask, n, cov = mask_of(case)
    xs, ys = [s[0] for s in case.stars], [s[1] for s in case.stars]
    for v in MA.NONFINITE:
        assert any(x == v or (x != x and v != v) for x in xs) and any(y == v or (y != y and v != v) for y in ys)
    if case.strict_coverage:
        assert 0.0 < cov < 1.0, cov
    else:
        assert cov in (0.0, 1.0)
    # without the wild stars the mask is the same: each of them either paints nothing or indexes inside the plane
    tame = [s for s in case.stars if np.isfinite(s[0]) and np.isfinite(s[1]) and abs(s[0]) < 1e17 and abs(s[1]) < 1e17]
    tame_mask, tame_n, _ = mr.star_mask_from_stars(case.image, tame, **case.cfg)
    assert MA.same_planes(mask, tame_mask) and n - tame_n == len(case.stars) - len(tame)


@pytest.mark.parametrize("case", by_name(MASK_CASES, "S-protect"), ids=ids(by_name(MASK_CASES, "S-protect")))
def test_protection_holds_what_it_claims(case):
    mask, _, cov = mask_of(case)
    bare, _, _ = mr.star_mask_from_stars(case.image, list(case.stars), **dict(case.cfg, luminance_protect=False))
    img = case.image
    assert np.isnan(img).any() and (img == np.inf).any() and (img == -np.inf).any()
    c = F(case.cfg["luminance_ceiling"])
    if c != c:
        assert MA.same_planes(mask, bare)                                            # nothing is above a NaN ceiling
        return
    assert (img == c).any() and (img == np.nextafter(c, F(np.inf))).any()
    assert not mask[img == c].any() or (bare[img == c] == mask[img == c]).all()      # at the ceiling: untouched
    assert ((mask > 0) & (mask <= F(0.01))).any() and ((mask > F(0.01)) & (mask < F(0.012))).any()   # both sides of the coverage threshold
    painted = bare > 0
    assert (painted & (mask > bare)).any(), "no painted pixel raised by the protection"
    assert (painted & (bare < 1) & (mask == bare)).any(), "no painted skirt pixel left alone"
    assert 0.0 < cov < 1.0


def test_orders_are_permutations_of_one_list():
    base, orders = MA.order_cases()
    for o in orders:
        assert o.stars != base.stars and sorted(map(repr, o.stars)) == sorted(map(repr, base.stars))
        assert MA.same_planes(mask_of(o)[0], mask_of(base)[0]) and mask_of(o)[1:] == mask_of(base)[1:]


# ---- conditions: stretch -----------------------------------------------------------------------------------------------------------
def test_tiny_planes():
    one = next(c for c in STRETCH_CASES if c.name == "M-tiny-1x1-default")
    out, iters, final_bg, conv, _ = stretch_of(one)
    assert not out.any() and (iters, final_bg, conv) == (2, 0.0, False)             # a zero-range plane
    assert sorted({c.image.shape for c in by_name(STRETCH_CASES, "M-tiny")}) == sorted(MA.SMALL_SHAPES)


@pytest.mark.parametrize("case", by_name(STRETCH_CASES, "M-long"), ids=ids(by_name(STRETCH_CASES, "M-long")))
def test_long_loops_stop_where_they_claim(case):
    _, iters, _, conv, _ = stretch_of(case)
    if case.stops_in:
        lo, hi = case.stops_in
        assert conv and lo <= iters <= hi < case.cfg["iterations"], (iters, case.stops_in)
    else:
        assert iters == case.cfg["iterations"] and not conv


def test_long_family_covers_every_chunk_position():
    cases = by_name(STRETCH_CASES, "M-long")
    assert sorted(c.cfg["iterations"] for c in cases if not c.stops_in) == [31, 32, 33, 64, 65, 65]
    assert [c.stops_in for c in cases if c.stops_in] == [(32, 32), (33, 64), (65, 96)]


@pytest.mark.parametrize("case", by_name(STRETCH_CASES, "M-clamp"), ids=ids(by_name(STRETCH_CASES, "M-clamp")))
def test_clamp_planes_leave_the_unit_interval(case):
    out, iters, _, _, before = stretch_of(case)
    first = mr.masked_stretch_with_mask(case.image, case.mask, return_unclamped=True, **dict(case.cfg, iterations=1))[4]
    with np.errstate(invalid="ignore"):
        if case.cfg["protection_amount"] > 0:
            assert (before < 0).any() and (before > 1).any()
        else:   # (see tests/masked_adversarial.py: a weight <= 0.5 cannot keep a pixel outside; the flag goes up and comes down again)
            assert ((first < 0) | (first > 1)).any() and not ((before < 0) | (before > 1)).any()
        assert np.isnan(out).any() and not (out < 0).any() and not (out > 1).any()
    assert iters == case.cfg["iterations"] or case.cfg.get("convergence_threshold", 1e-5) > 0
    with np.errstate(invalid="ignore"):
        for v in MA.CLAMP_MASK_VALUES:
            assert (np.isnan(case.mask) if v != v else case.mask == F(v)).any()


def test_subnormal_plane_is_subnormal():
    case = next(c for c in STRETCH_CASES if c.name == "M-subnormal")
    work = mr.normalize_to_01(case.image)
    tiny = np.finfo(F).tiny
    assert int(((work > 0) & (work < tiny)).sum()) >= 100
    assert 0.0 < mr.masked_median(work, case.mask) < tiny
    _, iters, final_bg, conv, _ = stretch_of(case)
    assert 0.0 < final_bg < tiny and not conv and iters == 2                       # stagnates


def test_range_planes_hold_what_they_claim():
    mixed = next(c for c in STRETCH_CASES if c.name == "M-range-mixed")
    img = mixed.image
    with np.errstate(invalid="ignore"):
        assert ((img > 0) & (img < F(1e-7))).sum() >= 50 and (img == F(1e-7)).any() and (img < 0).any()
        assert (np.signbit(img) & (img == 0)).any() and np.isnan(img).any() and (img == np.inf).any() and (img == -np.inf).any()
    for name in ("M-range-equal", "M-range-none"):
        out, iters, final_bg, conv, _ = stretch_of(next(c for c in STRETCH_CASES if c.name == name))
        assert not out.any() and (iters, final_bg, conv) == (2, 0.0, False)
    assert not np.isfinite(next(c for c in STRETCH_CASES if c.name == "M-range-none").image).all()


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------
def masks_differ(case, mutation):
    return not MA.same_planes(mask_of(case)[0], mask_of(case, mutation)[0])


def stretches_differ(case, mutation):
    a, b = stretch_of(case), stretch_of(case, mutation)
    return not MA.same_planes(a[0], b[0]) or a[1:4] != b[1:4]


def test_a_strict_disc_edge_is_told_apart():
    hard = [c for c in by_name(MASK_CASES, "S-shapes") if c.lattice and c.cfg["softness"] == 0.0 and min(c.image.shape) >= 16
            and not (c.group == "all" and c.image.shape == (16, 16))]        # (there the cluster paints the whole plane 1)
    assert hard and all(masks_differ(c, "edge") for c in hard)
    # with a skirt the strict comparison is invisible by construction (see tests/masked_adversarial.py): not a gap of these fixtures
    soft = next(c for c in MASK_CASES if c.name == "S-shapes-40x60-discs-soft")
    assert not masks_differ(soft, "edge")
    assert masks_differ(next(c for c in MASK_CASES if c.name == "S-nonfinite-g0-s0"), "edge")


def test_a_last_writer_is_told_apart():
    base, orders = MA.order_cases()
    got = {mask_of(c, "lastwriter")[0].tobytes() for c in [base] + orders}
    assert len(got) > 1                                                              # the orders disagree with one another
    for c in [base] + orders:
        assert masks_differ(c, "lastwriter")
    for c in by_name(MASK_CASES, "S-shapes"):
        if c.group == "cluster" and c.cfg["softness"] > 0 and min(c.image.shape) >= 16:     # (a hard disc is 1 in any order)
            assert masks_differ(c, "lastwriter"), c.name


def test_a_loop_cut_at_the_first_chunk_is_told_apart():
    for c in by_name(STRETCH_CASES, "M-long"):
        beyond = c.cfg["iterations"] > 32 and (not c.stops_in or c.stops_in[0] > 32)
        assert stretches_differ(c, "cut32") == beyond, c.name
    assert sum(stretches_differ(c, "cut32") for c in by_name(STRETCH_CASES, "M-clamp")) >= 3


def test_a_missing_clamp_is_told_apart():
    for c in by_name(STRETCH_CASES, "M-clamp"):
        assert stretches_differ(c, "noclamp") == (c.cfg["protection_amount"] > 0), c.name
    assert not any(stretches_differ(c, "noclamp") for c in by_name(STRETCH_CASES, "M-tiny"))   # (a mask in [0, 1] never needs it)


def test_flushed_subnormals_are_told_apart():
    assert all(stretches_differ(c, "ftz") for c in by_name(STRETCH_CASES, "M-subnormal"))


def test_a_range_over_every_positive_pixel_is_told_apart():
    assert all(stretches_differ(c, "range0") for c in by_name(STRETCH_CASES, "M-range-mixed"))
    assert stretches_differ(next(c for c in STRETCH_CASES if c.name == "M-range-none"), "range0")
