"""The fixtures of tests/select_adversarial.py held to what they claim (no GPU): the pairs differ where they say, the populations
have the stated candidates and middle ranks, the numpy statement of percentile_bounds agrees with the CPU oracle on every one of
them, the background images do to the oracle what their docstrings say (and the oracle agrees with the independent restatement
there), the wavelet planes' noise estimate is a tied value.  A fixture that has drifted fails here, so the GPU test
(tests/test_gpu_select_adversarial.py) cannot pass by testing nothing."""
import numpy as np
import pytest

import background_restatement as BR
import masked_restatement as MR
import select_adversarial as SA
import wavelet_restatement as WR

F32 = np.float32
POPULATIONS = SA.populations()
BACKGROUNDS = SA.background_cases()


def same_bits(a, b):
    return np.array_equal(SA.bits_of(a), SA.bits_of(b))


# ---- pairs and populations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SA.PAIRS))
def test_pairs_are_adjacent_and_differ_exactly_at_their_level(name):
    lower, upper, level = SA.PAIRS[name]
    assert SA.key(upper) == SA.key(lower) + 1 and upper == np.nextafter(lower, SA.INF)
    lo_bins, up_bins = SA.level_bins(lower), SA.level_bins(upper)
    assert lo_bins[:level] == up_bins[:level] and lo_bins[level] != up_bins[level]
    if level < 2:   # the upper value opens its bin: everything below the level is zero, and all ones in the lower value
        assert all(b == 0 for b in up_bins[level + 1:]) and lo_bins[2] == 0x3FF


def test_the_named_values():
    assert SA.PAIRS["L0"][1] == F32(1.25) and SA.PAIRS["BINADE"][1] == F32(1.0)
    assert SA.PAIRS["TOP"][1] == np.finfo(F32).max
    assert SA.FLOOR == F32(1e-7) and not SA.is_candidate(SA.FLOOR) and SA.is_candidate(SA.FLOOR_UP)
    assert len({SA.level_bins(v)[0] for v in SA.FOUR_VALUES}) == 4
    assert not SA.is_candidate(SA.CONTAMINATION).any()
    for t in SA.MS_TARGETS[:3]:      # level-0 bin edges
        assert SA.level_bins(F32(t))[1:] == (0, 0) and F32(t) == t
    assert SA.level_bins(F32(SA.MS_TARGETS[3]))[1:] != (0, 0)


def test_population_list_covers_what_the_issue_names():
    names = {p.name for p in POPULATIONS}
    assert len(names) == len(POPULATIONS)
    for pair in SA.PAIRS:
        for m in SA.M_LIST:
            assert f"{pair}-{m}" in names
    big = next(p for p in POPULATIONS if p.name == "L0-big")
    assert big.count == SA.BIG == 600_001 and SA.BIG > 256 * 8 * 256 and SA.BIG % 256 and big.values.size % 256
    lower, upper, _ = SA.PAIRS["L0"]
    assert same_bits(big.values[0], lower) and same_bits(big.values[-1], lower)      # the deciding copies: first and last pixel
    c = big.values[SA.is_candidate(big.values)]
    assert np.sort(c)[c.size // 2] == lower and np.sort(c[1:])[(c.size - 1) // 2] == upper == np.sort(c[:-1])[(c.size - 1) // 2]


@pytest.mark.parametrize("pop", POPULATIONS, ids=lambda p: p.name)
def test_population_has_the_stated_candidates(pop):
    ok = SA.is_candidate(pop.values)
    assert int(ok.sum()) == pop.count
    if pop.name != "L0-big":      # contamination is interleaved: every kind of it is there, 1e-7f in front
        assert not ok[0]
    for c in SA.CONTAMINATION:
        assert (SA.bits_of(pop.values) == SA.bits_of(c)).any(), c
    s = np.sort(pop.values[ok])
    if pop.middle is not None:
        assert pop.count % 2 == 0 and same_bits(s[pop.count // 2 - 1], pop.middle[0]) and same_bits(s[pop.count // 2], pop.middle[1])
    pair = pop.meta.get("pair")
    if pair and pair != "FLOOR":
        lower, upper, _ = SA.PAIRS[pair]
        m = pop.meta["m"]
        assert int((s == lower).sum()) == m - m // 2 and int((s == upper).sum()) == m // 2
    for plane in pop.planes():
        assert int(SA.is_candidate(plane).sum()) == pop.count and same_bits(plane.ravel()[:pop.values.size], pop.values)
    one, square = pop.planes()
    assert one.shape == (1, pop.values.size) and abs(square.shape[0] - square.shape[1]) <= 2 + square.shape[0] // 8


def test_four_valued_quartiles_fall_on_the_first_and_last_element_of_a_bin():
    for pop in (p for p in POPULATIONS if p.name.startswith("four-") and p.count >= 8):
        m = pop.count
        assert int(m * 0.25) == m // 4 and int(m * 0.75) == 3 * m // 4                 # the first candidate of bins 2 and 4
        assert int(m * 0.2499) == m // 4 - 1 and int(m * 0.7499) == 3 * m // 4 - 1     # the last candidate of bins 1 and 3
        assert SA.percentile_statement(pop.values, 0.25, 0.75) == (SA.FOUR_VALUES[1], SA.FOUR_VALUES[3])
        assert SA.percentile_statement(pop.values, 0.2499, 0.7499) == (SA.FOUR_VALUES[0], SA.FOUR_VALUES[2])


@pytest.mark.parametrize("pop", POPULATIONS, ids=lambda p: p.name)
def test_oracle_percentile_bounds_equal_the_numpy_statement(oracle, pop):
    for lo_pct, hi_pct in SA.PCT_PAIRS:
        want = SA.percentile_statement(pop.values, lo_pct, hi_pct)
        for plane in pop.planes():
            got = oracle.tile_percentile_bounds(plane, lo_pct, hi_pct)
            assert same_bits(np.array(got, F32), np.array(want, F32)), (pop.name, lo_pct, hi_pct, got, want)
    if pop.middle is not None:      # the middle pair straddles the edge it is named for
        assert SA.percentile_statement(pop.values, 0.499, 0.5)[1] == pop.middle[1]
        assert SA.percentile_statement(pop.values, (pop.count // 2 - 0.5) / pop.count, 0.5)[0] == pop.middle[0]


def test_oracle_min_max_branch_equals_the_numpy_statement(oracle):
    big = np.finfo(F32).max
    for name, plane in SA.no_candidate_planes().items():
        assert not SA.is_candidate(plane).any()
        want = SA.percentile_statement(plane, 0.001, 0.999)
        assert same_bits(np.array(oracle.tile_percentile_bounds(plane), F32), np.array(want, F32)), name
    assert SA.percentile_statement(SA.no_candidate_planes()["all_nan"], 0.0, 1.0) == (big, -big)
    assert SA.percentile_statement(SA.no_candidate_planes()["all_floor"], 0.0, 1.0) == (SA.FLOOR, SA.FLOOR)
    assert SA.percentile_statement(SA.no_candidate_planes()["contamination_only"], 0.0, 1.0) == (F32(-3.0e38), SA.FLOOR)


def test_pyramid_plane_bounds_sit_inside_ties(oracle):
    plane = SA.pyramid_plane()
    assert plane.shape == (300, 260)
    lo, hi = SA.percentile_statement(plane, 0.001, 0.999)
    assert lo == SA.FOUR_VALUES[0] and hi == SA.FOUR_VALUES[3]
    assert same_bits(np.array(oracle.generate_tile_pyramid(plane, 256)[2], F32), np.array([lo, hi], F32))
    assert (~SA.is_candidate(plane)).sum() > 700


# ---- background ------------------------------------------------------------------------------------------------------------------
def global_median_mad(img):
    with np.errstate(invalid="ignore"):
        px = img[np.isfinite(img) & (img > F32(0.0))]
    med = BR.median_f32(px)
    return med, BR.median_f32(np.abs(px - med)), px.size


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("case", BACKGROUNDS, ids=lambda c: c.name)
def test_oracle_background_equals_the_restatement(oracle, case, iterations, mode):
    kw = dict(grid_size=case.grid, poly_degree=case.degree, sigma_clip=case.sigma_clip, iterations=iterations, mode=mode)
    try:
        model, corrected, count, rms, coeffs = BR.extract_background(case.image, **kw)
    except BR.BackgroundError as e:
        with pytest.raises(ValueError) as got:
            oracle.extract_background(case.image, **kw)
        assert str(got.value) == str(e)
        assert case.name == "B6-scattered" and str(e) == f"Not enough background samples (0) for polynomial degree {case.degree}"
        return
    assert case.name != "B6-scattered"
    want = oracle.extract_background(case.image, **kw)
    assert want.sample_count == count
    n_terms = (case.degree + 1) * (case.degree + 2) // 2
    assert np.array_equal(want.coeffs[:n_terms], np.array(coeffs))
    assert np.array_equal(want.model, model, equal_nan=True) and np.array_equal(want.corrected, corrected, equal_nan=True)
    assert want.rms_residual == pytest.approx(rms, rel=1e-12, abs=1e-300)


def case_named(name):
    return next(c for c in BACKGROUNDS if c.name == name)


def test_b1_reads_the_median_and_the_mad_to_the_ulp(oracle):
    c = case_named("B1")
    med, mad, n = global_median_mad(c.image)
    assert med == F32(1000.0) and mad == F32(3.0) and n == c.image.size
    sigma = F32(3.0) * F32(1.4826)
    assert c.meta["hi"] == F32(1000.0) + F32(2.5) * sigma and c.meta["lo"] == F32(1000.0) - F32(2.5) * sigma
    got = oracle.extract_background(c.image, c.grid, c.degree, c.sigma_clip, 1, 0)
    assert got.sample_count == c.grid ** 2 - 2
    # one ulp of the tied median moves both thresholds by one ulp: another pair of the flat cells becomes the samples
    flats = [c.meta["hi"], np.nextafter(c.meta["hi"], SA.INF), c.meta["lo"], np.nextafter(c.meta["lo"], -SA.INF)]
    assert [c.meta["lo"] <= v <= c.meta["hi"] for v in flats] == [True, False, True, False]
    up, down = np.nextafter(med, SA.INF), np.nextafter(med, -SA.INF)
    assert [up - F32(2.5) * sigma <= v <= up + F32(2.5) * sigma for v in flats] == [True, True, False, False]
    assert [down - F32(2.5) * sigma <= v <= down + F32(2.5) * sigma for v in flats] == [False, False, True, True]


def test_b2_middle_ranks_straddle_a_level0_edge():
    c = case_named("B2")
    with np.errstate(invalid="ignore"):
        s = np.sort(c.image[c.image > 0])
    assert s.size % 2 == 0 and same_bits(s[s.size // 2 - 1], c.meta["lower"]) and same_bits(s[s.size // 2], c.meta["upper"])
    assert SA.level_bins(c.meta["lower"])[0] + 1 == SA.level_bins(c.meta["upper"])[0]
    med, _, _ = global_median_mad(c.image)
    d = np.sort(np.abs(s - med))
    assert SA.level_bins(d[d.size // 2 - 1])[0] != SA.level_bins(d[d.size // 2])[0]     # and so do the deviations'


def test_b3_model_is_one_value(oracle):
    c = case_named("B3")
    got = oracle.extract_background(c.image, c.grid, c.degree, c.sigma_clip, 3, 0)
    assert np.unique(got.model).size == 1 and got.model.size % 2 == 0 and got.model[0, 0] > 0


def test_b4_remainder_counts_in_the_global_median_only():
    for c in (x for x in BACKGROUNDS if x.name.startswith("B4")):
        rows, cols = c.image.shape
        rr, rc = c.meta["remainder"]
        assert (rr, rc) == (rows % c.grid, cols % c.grid)
        med, _, _ = global_median_mad(c.image)
        inner = c.image[:rows - rr, :cols - rc]
        assert (rr, rc) == (0, 0) or global_median_mad(inner)[2] < global_median_mad(c.image)[2]
        assert ((c.image == med).sum()) > 1000       # a long tie
    big = case_named("B4-263x517")
    assert big.meta["remainder"] == (7, 5) and (big.image[-7:, :-5] == F32(3e38)).all() and (big.image[:, -5:] == F32(1e-30)).all()
    assert (case_named("B4-256x256").image.shape[1] & 255) == 0


def test_b5_model_is_positive_on_a_strict_subset(oracle):
    c = case_named("B5")
    for mode in (0, 1):
        got = oracle.extract_background(c.image, c.grid, c.degree, c.sigma_clip, 3, mode)
        assert 0 < int((got.model > 0).sum()) < got.model.size


def test_b6_tiny_pixels_count_in_the_global_median(oracle):
    c = case_named("B6")
    assert abs(float(c.meta["tiny"].mean()) - 0.40) < 0.005 and (c.image[c.meta["tiny"]] == F32(1e-8)).all()
    without = c.image.copy()
    without[c.meta["tiny"]] = 0.0
    assert global_median_mad(c.image)[0] != global_median_mad(without)[0]
    assert global_median_mad(c.image)[2] == c.image.size
    got = oracle.extract_background(c.image, c.grid, c.degree, c.sigma_clip, 1, 0)
    assert 0 < got.sample_count <= 5 * c.grid
    s = case_named("B6-scattered")
    assert abs(float(s.meta["tiny"].mean()) - 0.40) < 0.005


# ---- wavelet ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,plane,parity", SA.wavelet_planes(), ids=lambda v: v if isinstance(v, str) else "")
def test_wavelet_noise_estimate_is_a_tied_value(name, plane, parity):
    with np.errstate(invalid="ignore"):
        d0 = (plane - WR.atrous_smooth(plane, 1)).astype(F32).ravel()
    a = np.sort(np.abs(d0[np.isfinite(d0)]))
    assert a.size % 2 == parity and a.size in (plane.size, plane.size - 25)
    mids = (a[a.size // 2],) if a.size % 2 else (a[a.size // 2 - 1], a[a.size // 2])
    for v in mids:
        assert int((a == v).sum()) >= 2, (name, v)
    sigma = WR.wavelet_denoise(plane, 3)[2]
    assert sigma == float(np.float64(WR.median_f32(a)) * np.float64(WR.MAD_TO_SIGMA)) and sigma > 0


# ---- masked stretch --------------------------------------------------------------------------------------------------------------
def test_masked_planes_are_what_they_say():
    planes = SA.masked_planes()
    assert len(planes) == 6 and {p[1].shape for p in planes} == set(SA.MASKED_SHAPES)
    for name, img, mask in planes:
        assert img.dtype == F32 and mask.dtype == F32 and img.shape == mask.shape
        if name.startswith("two-valued"):
            v, n = np.unique(img, return_counts=True)
            assert v.tolist() == [F32(0.2), F32(0.6)] and abs(int(n[0]) - int(n[1])) <= 1
        else:
            fin = img[np.isfinite(img) & (img > 0)]
            assert np.array_equal(fin, (np.rint(fin.astype(np.float64) * 65535.0) / 65535.0).astype(F32))    # 16-bit levels
            assert np.sort(np.unique(fin, return_counts=True)[1])[-8:].sum() > 0.8 * fin.size                # the sky: a few levels
        if name.startswith("soft-mask"):
            soft = (mask > 0) & (mask < 0.5)
            assert abs(float(soft.mean()) - 0.45) < 0.01 and ((mask == 0) | soft).all()


@pytest.mark.parametrize("shape", SA.MASKED_SHAPES)
def test_soft_mask_moves_the_median_out_of_the_predicted_level0_bin(shape):
    """the blend pass of csrc/masked_stretch.hip predicts the next median's level-0 bin as that of mtf(median): on the soft-mask
    plane the blended candidates pull the real median out of it for some (target, protection), and leave it in for others -- both
    forms of level 1 run on these fixtures"""
    name, img, mask = next(p for p in SA.masked_planes() if p[0] == f"soft-mask-{shape[0]}x{shape[1]}")
    hits = misses = 0
    for target in SA.MS_TARGETS:
        for protection in SA.MS_PROTECTIONS:
            working = MR.normalize_to_01(img)
            bg = MR.masked_median(working, mask)
            m = F32(MR.mtf_balance(bg, target))
            predicted = MR.apply_mtf(np.array([bg], F32), m)[0]
            blend = mask * F32(protection)
            working = (working * blend + MR.apply_mtf(working, m) * (F32(1.0) - blend)).astype(F32)
            real = F32(MR.masked_median(working, mask))
            same = SA.level_bins(predicted)[0] == SA.level_bins(real)[0]
            hits, misses = hits + same, misses + (not same)
    assert hits >= 2 and misses >= 2, (hits, misses)


@pytest.mark.parametrize("name,img,mask", SA.masked_planes(), ids=lambda v: v if isinstance(v, str) else "")
def test_oracle_masked_stretch_equals_the_restatement(oracle, name, img, mask):
    for target in SA.MS_TARGETS:
        for protection in (SA.MS_PROTECTIONS[1],) if target != SA.MS_TARGETS[0] else SA.MS_PROTECTIONS:
            want = oracle.masked_stretch(img, mask=oracle.StarMaskResult(mask, 0, 0.0), target_background=target, protection_amount=protection)
            image, iterations_run, final_bg, converged = MR.masked_stretch_with_mask(img, mask, target_background=target,
                                                                                     protection_amount=protection)
            assert (want.iterations_run, want.final_background, want.converged) == (iterations_run, final_bg, converged)
            assert same_bits(want.image, image)
            assert iterations_run >= 2 or name.startswith("two-valued")      # the loop runs: there is a median after a blend


# ---- the fixtures tell a wrong select from a right one (tests/select_model.py) ---------------------------------------------------
def model_mismatches(mutation):
    """(percentile cases, background images, wavelet planes) on which the model of plane_select.hip's host logic, with one mistake
    switched on, differs from the plain statements"""
    import select_model as SM
    pct = []
    for pop in (p for p in POPULATIONS if p.count <= 60_000):
        for lo_pct, hi_pct in SA.PCT_PAIRS:
            got = SM.percentile_bounds(pop.values, lo_pct, hi_pct, mutation)
            if got is not None and not same_bits(np.array(got, F32), np.array(SA.percentile_statement(pop.values, lo_pct, hi_pct), F32)):
                pct.append((pop.name, lo_pct, hi_pct))
    bg = []
    for c in BACKGROUNDS:
        med, mad, _ = global_median_mad(c.image)
        got = (SM.median_f32(c.image, 0.0, False, 0.0, mutation), SM.median_f32(c.image, 0.0, True, med, mutation))
        if not same_bits(np.array(got, F32), np.array([med, mad], F32)):
            bg.append(c.name)
    wv = []
    for name, plane, _ in SA.wavelet_planes():
        with np.errstate(invalid="ignore"):
            d0 = (plane - WR.atrous_smooth(plane, 1)).astype(F32)
        want = WR.median_f32(np.abs(d0[np.isfinite(d0)]))
        if not same_bits(SM.median_f32(d0, -np.inf, True, 0.0, mutation), want):
            wv.append(name)
    return pct, bg, wv


def test_model_of_the_select_agrees_with_the_statements():
    assert model_mismatches("") == ([], [], [])


@pytest.mark.parametrize("mutation", ["a", "b", "d", "e"])
def test_fixtures_catch_a_wrong_select(mutation):
    pct, bg, wv = model_mismatches(mutation)
    if mutation == "a":      # `>=` in locate: rank 0 lands in the empty bin 0, a rank on the first element of a bin in the bin before
        assert any(k[1:] == (0.0, 1.0) for k in pct) and any(k[0].startswith("four-") and k[1:] == (0.25, 0.75) for k in pct)
    if mutation == "b":      # only the reversed pair asks for rank == count
        assert pct and all(k[1:] == (1.0, 0.0) for k in pct) and not bg and not wv
    if mutation == "d":      # B2: the two middle deviations are far apart (its middle VALUES average back to the upper one in f32)
        assert "B2" in bg and not pct
    if mutation == "e":      # signed deviations: half of the keys leave the order
        assert len(bg) >= 5 and len(wv) == len(SA.wavelet_planes()) and not pct


def test_reusing_h1_for_the_level2_pass_changes_nothing():
    """descend locates every item of a level before the level's first child pass: the issue's `h2 overwritten while level 1 still
    needs it` cannot happen, and no fixture can tell the two buffer assignments apart"""
    assert model_mismatches("c") == ([], [], [])


@pytest.mark.parametrize("name,img,mask", SA.masked_planes(), ids=lambda v: v if isinstance(v, str) else "")
def test_model_of_the_speculative_level1_and_its_mutation(name, img, mask):
    """the model of masked_stretch.hip's select chain equals the restatement in both forms of level 1; with mutation f (level 1 reads
    the predicted histogram whether or not the prediction held) the stretched image changes exactly where some median left its
    predicted level-0 bin -- on the soft-mask planes that happens for several (target, protection)"""
    import select_model as SM
    caught = 0
    for target in SA.MS_TARGETS:
        for protection in SA.MS_PROTECTIONS:
            kw = dict(target_background=target, protection_amount=protection)
            want = MR.masked_stretch_with_mask(img, mask, **kw)
            for predict in (True, False):
                got = SM.masked_stretch_chain(img, mask, predict=predict, **kw)
                assert same_bits(got[0], want[0]) and got[1:4] == want[1:4], (name, target, protection, predict)
                assert predict or not got[4]
            trace = SM.masked_stretch_chain(img, mask, **kw)[4]
            wrong = SM.masked_stretch_chain(img, mask, mutation="f", **kw)
            differs = not same_bits(wrong[0], want[0]) or wrong[1:4] != want[1:4]
            missed = any(pred != real for pred, real in trace)
            assert differs == missed, (name, target, protection, trace)
            caught += differs
    if name.startswith("soft-mask"):
        assert caught >= 2, caught
