"""The cases of tests/drizzle_adversarial.py held to what they claim, without a GPU.

  placement    every designed pixel's list, as tests/drizzle_restatement.py builds it, is the designed list bit for bit and in order,
               and the round-by-round walk the census uses rejects what the restatement rejects
  hand         the small lists of every family against answers worked out by hand
  census       conditions (not measurements) per case: a threshold tie in every A1 call, MAD == 0 rounds, merge ties, pixels where
               nothing survives, every count up to the cap, the cap reached, >= 6 acting rounds, odd and even survivor counts
  sensitivity  the walk with one decision restated wrongly (`>` for `>=`, no 1e-10 floor, flushed subnormals, an f64 median or MAD average)
               rejects differently on every call of the family that exists to catch it
  geometry     drizzle_loop == drizzle element for element on every geometry case, and gather_pixel's lists and weight sums equal to
               theirs on every pixel of an output of up to 200 pixels, else on 28 border and 24 seeded pixels; threshold-pixel share 0;
               footprint edges exactly on and on either side of integers; far frames change nothing; the 7.44-sigma frames fall on
               either side of the cut"""
import numpy as np
import pytest

import drizzle_adversarial as DA
import drizzle_restatement as R

F = np.float32
DESIGNED = DA.designed_cases()
GEOMETRY = DA.geometry_cases()
INF = F(np.inf)


def ids(cases):
    return [c.name for c in cases]


def family(name, cases=DESIGNED):
    found = [c for c in cases if c.family == name]
    assert found, name
    return found


def fin(vals, sl=3.0, sh=3.0, iters=5):
    v, _, rej, _ = R.finalize_pixel([F(x) for x in vals], 1.0, sl, sh, iters)
    return v, rej


def test_cases_are_small_named_once_and_read_only():
    names = [c.name for c in DESIGNED + GEOMETRY]
    assert len(set(names)) == len(names)
    for c in DESIGNED + GEOMETRY:
        assert 2 <= len(c.frames) <= 40 and len(c.offsets) == len(c.frames), c.name
        for f in c.frames:
            assert not f.flags.writeable and f.dtype == F and f.size <= 8 * 40, c.name
    for fam in ("A1d", "A1g", "A2", "A3", "A4z", "A4d", "A5z", "A5d", "A5o", "A7", "A8"):
        assert [len(c.frames) for c in family(fam)] == DA.FRAME_COUNTS, fam
    assert sorted((len(c.frames), c.iters) for c in family("A6")) == sorted((n, it) for n in (32, 33) for it in DA.A6_ITERS)
    assert len(family("cap")) == 1


# ---- placement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DESIGNED, ids=ids(DESIGNED))
def test_designed_pixels_receive_their_lists(case):
    want = DA.wanted(case)
    ocols = want.dims[3]
    cap = max(2 * len(case.frames), 4)
    assert int(want.counts.max()) <= cap and np.isfinite(want.image).all() and np.isfinite(want.weight).all()
    assert not want.threshold.any()
    for oy, ox, vals, tag in case.designed:
        got = want.lists[oy * ocols + ox]
        assert DA.bits(got).tobytes() == DA.bits(list(vals)).tobytes(), (tag, oy, ox)
        if len(vals) >= 2:      # the census walks the same rounds as the restatement
            assert DA.rejected_after(vals, case.sl, case.sh, case.iters) == want.rejected_map[oy, ox], tag
            v, _, rej, _ = R.finalize_pixel(list(vals), 1.0, case.sl, case.sh, min(case.iters, cap))
            assert rej == want.rejected_map[oy, ox] and DA.bits(v) == DA.bits(want.image[oy, ox]), tag


# ---- hand-computed ---------------------------------------------------------------------------------------------------------------
def test_threshold_tie_by_hand():
    """[-1, -0.5, 0, 0.5, X]: median 0, deviations 0, .5, .5, 1, X: MAD 0.5, sigma f32(0.7413), 2 sigma = X exactly"""
    x = DA.X_TIE
    assert x == F(F(2.0) * F(0.7413)) and float(x) > 1.0
    assert fin([-1, -0.5, 0, 0.5, x], 2, 2) == (F((float(x) - 1.0) / 5.0), 0)
    assert fin([-1, -0.5, 0, 0.5, np.nextafter(x, INF)], 2, 2) == (F(-0.25), 1)     # then [-1 .. 0.5]: median -0.25, MAD 0.5: all stay
    assert fin([-1, -0.5, 0, 0.5, np.nextafter(x, F(0))], 2, 2)[1] == 0
    assert fin([1, 0.5, 0, -0.5, -x], 2, 2) == (F((1.0 - float(x)) / 5.0), 0)
    assert fin([1, 0.5, 0, -0.5, -np.nextafter(x, INF)], 2, 2) == (F(0.25), 1)
    assert fin([1, 0.5, 0, -0.5, -np.nextafter(x, F(0))], 2, 2)[1] == 0
    for k in DA.A1D_SCALES:     # a power of two moves everything together (2^-20 * 0.74 is still far above the 1e-10 floor)
        s = 2.0 ** k
        assert fin([-s, -0.5 * s, 0, 0.5 * s, float(x) * s], 2, 2)[1] == 0
        assert fin([-s, -0.5 * s, 0, 0.5 * s, float(np.nextafter(x, INF)) * s], 2, 2)[1] == 1


def test_general_tie_by_hand():
    """MAD 0.75, sigma f32(0.75 * 1.4826); the searched factors put f32(sh sigma) and f32(sl sigma) exactly on the 2^-12 grid"""
    sl, sh, d_lo, d_hi = DA.A1G_SETTINGS
    sigma = F(0.75 * R.MAD_TO_SIGMA)
    assert F(F(sh) * sigma) == F(d_hi) and F(F(sl) * sigma) == F(d_lo) and sl != sh
    for f in (sl, sh):
        mant, _ = np.frexp(f)
        assert mant != 0.5 and float(F(f)) == f and f * 2 ** 12 != round(f * 2 ** 12)        # an f32, and nothing dyadic about it
    g = DA.A1G_GRID
    for med in DA.A1G_MEDIANS:
        base = [med - 0.9375, med - 0.75, med, med + 0.75]
        assert fin(base + [med + d_hi], sl, sh)[1] == 0 and fin(base + [med + d_hi + g], sl, sh)[1] == 1 and fin(base + [med + d_hi - g], sl, sh)[1] == 0
        base = [med + 0.9375, med + 0.75, med, med - 0.75]
        assert fin(base + [med - d_lo], sl, sh)[1] == 0 and fin(base + [med - d_lo - g], sl, sh)[1] == 1 and fin(base + [med - d_lo + g], sl, sh)[1] == 0


def test_zero_mad_by_hand():
    """sigma = f32(1e-10): 3 sigma = 3e-10 lies far below an ulp of 900 (6.1e-5) and between 2e-10 and 4e-10"""
    c = F(900.0)
    up, down = np.nextafter(c, INF), np.nextafter(c, -INF)
    assert fin([c, c, c, up]) == (c, 1) and fin([c, c, c, down, up]) == (c, 2) and fin([c] * 7) == (c, 0)
    assert fin([0, 0, 0, 2e-10])[1] == 0 and fin([0, 0, 0, 4e-10]) == (F(0.0), 1)
    assert fin([0, 0, 0, -2e-10])[1] == 0 and fin([0, 0, 0, -4e-10]) == (F(0.0), 1)
    t = DA.T_FLOOR
    assert t == F(F(3.0) * F(1e-10))
    assert fin([0, 0, 0, t])[1] == 0 and fin([0, 0, 0, np.nextafter(t, INF)])[1] == 1
    assert fin([0, 0, 0, -t])[1] == 0 and fin([0, 0, 0, -np.nextafter(t, INF)])[1] == 1


def test_subnormals_by_hand():
    u = float(DA.U)
    vals = [1 * u, 2 * u, 3 * u, 4 * u, 50 * u]
    v, rej = fin(vals, 0.0, 0.0)
    assert rej == 4 and v == F(3 * u) and str(v) == "4e-45"                     # only dev == 0: the median itself
    v, rej = fin(vals)                                                           # MAD 2^-149: the floor holds, everything stays
    assert rej == 0 and v == F(12 * u)
    assert DA.rejected_after(vals, 0.0, 0.0, 5, "ftz") == 0                      # flushed: five zeros, nothing to reject


def test_near_flt_max_by_hand():
    vals = [F(-3e38), F(2e38), F(2.5e38), F(3e38)]                              # 2e38 + 2.5e38 > FLT_MAX: median +inf
    with np.errstate(over="ignore"):
        assert R.median_f32(vals) == INF
    mean = F(sum(float(v) for v in sorted(vals)) / 4.0)
    assert np.isfinite(mean)
    assert fin(vals, 0.0, 0.0) == (mean, 4)                                      # -0 * inf = NaN: nothing survives, the mean of all
    assert fin(vals, 3.0, 3.0) == (mean, 0)                                      # -inf >= -inf and -inf <= inf: everything stays
    pairs = [F(-3e38), F(3e38), F(-3.2e38), F(3.2e38)]                          # median (-3e38 + 3e38) / 2 = 0, MAD (3e38 + 3e38) / 2 = inf
    assert fin(pairs, 0.0, 0.0) == (F(0.0), 4) and fin(pairs, 3.0, 3.0) == (F(0.0), 0)
    assert DA.rejected_after(vals, 3.0, 3.0, 5, "f64median") == 1    # a finite median (2.25e38) would put -3e38 beyond 3 sigma


def test_single_negative_zero_by_hand():
    v, _, rej, _ = R.finalize_pixel([F(-0.0)], 0.25, 3.0, 3.0, 5)
    assert DA.bits(v) == 0x80000000 and rej == 0
    assert DA.bits(fin([F(-0.0), F(-0.0)])[0]) == 0                              # the f64 sum starts at +0.0


# ---- census ----------------------------------------------------------------------------------------------------------------------
def first_round(case, vals):
    return DA.trace(vals, case.sl, case.sh)[0]


@pytest.mark.parametrize("case", family("A1d") + family("A1g"), ids=ids(family("A1d") + family("A1g")))
def test_a1_every_call_has_ties_and_both_neighbours(case):
    c = DA.census(case)
    assert c["tie_pixels"] >= 1 and c["odd_survivors"] > 0 and c["even_survivors"] > 0
    seen = set()
    for _, _, vals, tag in case.designed:
        r = first_round(case, vals)
        if case.family == "A1d":
            kind = tag.split("-")[0]
            assert (r["tie"], r["removed"]) == {"tie": (True, 0), "over": (False, 1), "under": (False, 0)}[kind], tag
            seen.add((kind, tag.split("-")[1]))
        else:
            hi, lo = tag.split("-")[0][2:], tag.split("-")[1][2:]
            assert r["tie"] == ("0" in (hi, lo)) and r["removed"] == (hi == "1") + (lo == "1"), tag
            seen.add((hi, lo))
    assert len(seen) == (6 if case.family == "A1d" else 7)
    assert sorted({len(v) for _, _, v, _ in case.designed}) == DA.lengths(2 * len(case.frames), 5)
    assert c["tie_pixels"] == sum(1 for _, _, _, t in case.designed if t.startswith("tie") or "hi0" in t or "lo0" in t)


@pytest.mark.parametrize("case", family("A2"), ids=ids(family("A2")))
def test_a2_every_list_has_a_zero_mad(case):
    c = DA.census(case)
    assert c["mad0_rounds"] >= len(case.designed) and c["odd_survivors"] > 0 and c["even_survivors"] > 0
    for _, _, vals, tag in case.designed:
        r = first_round(case, vals)
        assert r["mad0"], tag
        major = len(vals) // 2 + 1
        if tag.startswith("ulp"):
            assert r["removed"] == len(vals) - major, tag
        elif tag.startswith("equal"):
            assert r["removed"] == 0, tag
        else:
            assert r["removed"] == sum(1 for v in vals if abs(v) > DA.T_FLOOR), tag
    tags = {t.split("-")[0] for _, _, _, t in case.designed}
    assert tags == {"ulp", "floor0", "floor3", "equal"}
    if len(case.frames) >= 8:      # (16 slots and more: every value around the floor is in some list, the threshold itself included)
        assert c["tie_pixels"] >= 1


@pytest.mark.parametrize("case", family("A3"), ids=ids(family("A3")))
def test_a3_the_merge_ties_in_every_list(case):
    for _, _, vals, tag in case.designed:
        if not (tag.startswith("two-valued") and len(vals) % 2) and "-run-out-" not in tag:     # ([a, a, b, b, b]: the median is b, the right run starts at 0)
            assert first_round(case, vals)["merge_ties"] >= 1, tag
        assert len(set(vals)) < len(vals), tag
    c = DA.census(case)
    assert c["odd_survivors"] > 0 and c["even_survivors"] > 0
    assert {len(v) % 2 for _, _, v, _ in case.designed} == {0, 1}
    assert DA.rejected_after(next(v for _, _, v, t in case.designed if t.startswith("steps-outlier")), 3.0, 3.0, 5) >= 1
    out = [(v, t) for _, _, v, t in case.designed if "-run-out-" in t]
    assert {t.split("-")[0] for _, t in out} == {"left", "right"}
    for vals, tag in out:          # the median is one of the two middle samples, and one run is used up before the merge ends
        r = first_round(case, vals)
        s = sorted(vals)
        assert R.median_f32(list(vals)) in (s[len(s) // 2 - 1], s[len(s) // 2]) and s[len(s) // 2 - 1] != s[len(s) // 2], tag
        assert r["exhausted"] == 1 and not r["mad0"], tag


@pytest.mark.parametrize("case", family("A4z") + family("A4d"), ids=ids(family("A4z") + family("A4d")))
def test_a4_lists_are_subnormal(case):
    tiny = np.finfo(F).tiny
    assert sum(1 for _, _, vals, _ in case.designed if all(abs(v) < tiny for v in vals)) >= len(case.designed) // 2
    assert any(any(abs(v) < tiny for v in vals) and any(abs(v) >= tiny for v in vals) for _, _, vals, _ in case.designed)
    want = DA.wanted(case)
    sub = (np.abs(want.image) > 0) & (np.abs(want.image) < tiny)
    assert sub.sum() >= len(case.designed) // 2            # subnormal results too
    if case.family == "A4z":
        ramp = [(oy, ox, v) for oy, ox, v, t in case.designed if t.startswith("ramp") and len(v) % 2 == 1]
        for oy, ox, v in ramp:                              # only the median itself survives
            assert want.rejected_map[oy, ox] == len(v) - 1 and want.image[oy, ox] == sorted(v)[len(v) // 2]
        assert ramp and DA.census(case)["none_survive"] >= 1
    else:
        assert want.rejected_map[[d[0] for d in case.designed], [d[1] for d in case.designed]].sum() == 0   # the floor holds


A5 = family("A5z") + family("A5d") + family("A5o")


@pytest.mark.parametrize("case", A5, ids=ids(A5))
def test_a5_medians_overflow_and_the_output_stays_finite(case):
    want = DA.wanted(case)
    assert np.isfinite(want.image).all()
    c = DA.census(case)
    n_inf = 0
    for oy, ox, vals, tag in case.designed:
        s = sorted(vals)
        with np.errstate(over="ignore"):
            med = R.median_f32(list(vals))
        if tag.startswith("median-inf"):
            assert med == INF and np.isfinite(s[len(s) // 2 - 1]) and len(s) % 2 == 0, tag
            assert want.rejected_map[oy, ox] == (len(vals) if case.family == "A5z" else 0), tag     # (1 * inf and 3 * inf alike)
            n_inf += 1
        elif tag.startswith("pairs-L") or tag.startswith("pairs-mid"):
            assert med == 0 and max(abs(v) for v in vals) > 4e37, tag
    assert n_inf >= 2
    if case.family == "A5z":
        assert c["none_survive"] >= n_inf
    else:
        assert c["none_survive"] == 0
    over = [(oy, ox, v) for oy, ox, v, t in case.designed if t.startswith("mad-overflow")]
    assert over
    for oy, ox, vals in over:      # the MAD is +inf: under 1 / 1 and 3 / 3 everything stays
        devs = sorted(abs(v) for v in vals)
        mid = len(devs) // 2
        assert float(devs[mid - 1]) + float(devs[mid]) > float(DA.FMAX) > (float(devs[mid - 1]) + float(devs[mid])) / 2.0 * R.MAD_TO_SIGMA
        if case.family != "A5z":
            assert want.rejected_map[oy, ox] == 0


def test_a6_rounds():
    """the acting-round maximum over the designed lists is at least 6 (here 16), and each call's sigma_iterations cuts it there"""
    unlimited = [c for c in family("A6") if c.iters == 2 ** 40]
    assert len(unlimited) == 2
    most = DA.census(unlimited[0])["acting_max"]
    assert most >= 6, most
    for case in family("A6"):
        c = DA.census(case)
        assert c["acting_max"] == min(case.iters, most), (case.name, c["acting_max"])
        assert c["counts"] == {64} and len(case.designed) == 156
        assert c["odd_survivors"] > 0 and c["even_survivors"] > 0
    for case in unlimited:      # all of a 64-sample list is in the network at n = 32; at n = 33 it is heap-sorted with room to spare
        assert (DA.wanted(case).counts == 64).sum() >= 156
    a, b = (DA.wanted(c) for c in family("A6") if c.iters in (5, 1000) and len(c.frames) == 32)
    assert a.rejected != b.rejected     # (the later rounds do reject)


@pytest.mark.parametrize("case", family("A7"), ids=ids(family("A7")))
def test_a7_every_count_up_to_the_cap(case):
    n = len(case.frames)
    cap = 2 * n
    c = DA.census(case)
    assert c["counts"] == set(range(cap + 1))
    want = DA.wanted(case)
    at = {(oy, ox): len(v) for oy, ox, v, _ in case.designed}
    assert all(want.counts[oy, ox] == k for (oy, ox), k in at.items())
    assert sum(1 for k in at.values() if k == cap) >= 5 and (want.counts == cap).any()
    assert {2, 3, cap - 1, cap} <= set(at.values())
    if n in (4, 8, 16, 32):      # the whole network holds samples: no +inf pad
        assert cap in (8, 16, 32, 64)
    assert c["odd_survivors"] > 0 and c["even_survivors"] > 0 and want.rejected > 0


@pytest.mark.parametrize("case", family("A8"), ids=ids(family("A8")))
def test_a8_single_zeros_keep_their_sign(case):
    want = DA.wanted(case)
    singles = {t: (oy, ox) for oy, ox, v, t in case.designed if len(v) == 1}
    assert len(singles) == 4
    for tag, (oy, ox) in singles.items():
        assert want.counts[oy, ox] == 1 and want.weight[oy, ox] == F(0.25)
        expect = 0x80000000 if "negative" in tag else (0 if "positive" in tag else DA.bits(F(900.0)))
        assert DA.bits(want.image[oy, ox]) == expect, tag
    assert (want.counts == 1).sum() >= 4


def test_the_cap_drops_the_later_frames():
    case = family("cap")[0]
    want = DA.wanted(case)
    assert (want.counts == 10).sum() >= 7 * 39
    inner = [want.lists[oy * DA.COLS + ox] for oy in range(DA.ROWS - 1) for ox in range(DA.COLS - 1)]
    assert all(len(l) == 10 and max(l) < 3000.0 and sum(1 for v in l if v >= 2000.0) == 2 for l in inner)
    assert any(max(l) >= 4000.0 for l in want.lists)     # (the border lists, two pushes per frame, do reach the last frame)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
def told_apart(case, mutation):
    return any(DA.rejected_after(v, case.sl, case.sh, case.iters) != DA.rejected_after(v, case.sl, case.sh, case.iters, mutation)
               for _, _, v, _ in case.designed if len(v) >= 3)


def test_strict_thresholds_are_told_apart():
    for case in family("A1d") + family("A1g"):
        assert told_apart(case, "strict"), case.name
    for case in family("A7"):      # (nothing in random data sits on a threshold: the gap these cases close)
        assert not told_apart(case, "strict"), case.name


def test_a_missing_floor_is_told_apart():
    for case in family("A2"):
        assert told_apart(case, "nofloor"), case.name


def test_flushed_subnormals_are_told_apart():
    for case in family("A4z"):
        assert told_apart(case, "ftz"), case.name


def test_an_f64_mad_average_is_told_apart():
    for case in family("A5o"):
        assert told_apart(case, "f64mad"), case.name


def test_an_f64_median_average_is_told_apart():
    for case in family("A5d"):     # (under sl = sh = 0 nothing survives either way: a finite median is no sample)
        assert told_apart(case, "f64median"), case.name


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def sample_pixels(orows, ocols):
    if orows * ocols <= 200:
        return [(oy, ox) for oy in range(orows) for ox in range(ocols)]
    rng = np.random.default_rng(orows * 1000 + ocols)
    border = [(0, 0), (0, ocols - 1), (orows - 1, 0), (orows - 1, ocols - 1)]
    border += [(0, int(v)) for v in rng.integers(0, ocols, 6)] + [(orows - 1, int(v)) for v in rng.integers(0, ocols, 6)]
    border += [(int(v), 0) for v in rng.integers(0, orows, 6)] + [(int(v), ocols - 1) for v in rng.integers(0, orows, 6)]
    return border + [(int(a), int(b)) for a, b in zip(rng.integers(0, orows, 24), rng.integers(0, ocols, 24))]


@pytest.mark.parametrize("case", GEOMETRY, ids=ids(GEOMETRY))
def test_loops_vectorised_and_gather_agree(case):
    x = R.drizzle_loop(*case.args())
    y = DA.wanted(case)
    assert x.image.tobytes() == y.image.tobytes() and x.weight.tobytes() == y.weight.tobytes()
    assert x.rejected == y.rejected and np.array_equal(x.rejected_map, y.rejected_map)
    assert np.array_equal(x.threshold, y.threshold) and np.array_equal(x.exact, y.exact) and np.array_equal(x.counts, y.counts)
    assert [[float(v) for v in l] for l in x.lists] == [[float(v) for v in l] for l in y.lists]
    assert x.wsum.tobytes() == y.wsum.tobytes()
    orows, ocols = y.dims[2:]
    for oy, ox in sample_pixels(orows, ocols):
        s, w = R.gather_pixel(list(case.frames), list(case.offsets), oy, ox, case.scale, case.pixfrac, case.kernel)
        assert [float(v) for v in s] == [float(v) for v in x.lists[oy * ocols + ox]], (oy, ox)
        assert w == x.wsum[oy, ox], (oy, ox)
    assert float(y.threshold.mean()) == 0.0                 # no candidate weight within 1e-6 relative of the cut
    assert y.exact.all() and np.isfinite(y.image).all()     # multiples of 2^-8: the image is held bit for bit
    assert y.counts.max() >= 2


def footprint_edges(case):
    """every c - half and c + half of the case, both axes"""
    half = case.pixfrac * case.scale * 0.5
    rows, cols = case.frames[0].shape
    out = []
    for dx, dy in case.offsets:
        for n, d in ((cols, -dx), (rows, -dy)):
            for i in range(n):
                c = (i + d) * case.scale
                out += [c - half, c + half]
    return np.array(out)


@pytest.mark.parametrize("case", family("B1a", GEOMETRY), ids=ids(family("B1a", GEOMETRY)))
def test_b1a_footprint_edges_lie_on_integers(case):
    e = footprint_edges(case)
    assert (e == np.round(e)).sum() >= 20 and (e != np.round(e)).any()
    assert any(dx < 0 for dx, _ in case.offsets) and any(dx > 0 for dx, _ in case.offsets)
    assert all(v * 8 == round(v * 8) for o in case.offsets for v in o)


@pytest.mark.parametrize("case", family("B1b", GEOMETRY), ids=ids(family("B1b", GEOMETRY)))
def test_b1b_centres_and_edges_fall_on_either_side_of_integers(case):
    e = footprint_edges(case)
    half = case.pixfrac * case.scale * 0.5
    centres = e[0::2] + half
    for v in (centres, e):
        off = v - np.round(v)
        near = np.abs(off) < 1e-9
        assert (off[near] < 0).any() and (off[near] > 0).any() and (off[near] == 0).any()


@pytest.mark.parametrize("case", family("B2", GEOMETRY), ids=ids(family("B2", GEOMETRY)))
def test_b2_an_output_axis_has_length_one_or_two(case):
    want = DA.wanted(case)
    assert want.dims[2:] == case.frames[0].shape and min(want.dims[2:]) <= 2
    rows, cols = case.frames[0].shape
    assert any(abs(dx) >= 1e5 for dx, _ in case.offsets) and any(cols <= dx < cols + 4 for dx, _ in case.offsets)
    if len(case.frames) == 33:
        assert want.image.size < 256     # lists of up to 66: the long-list grid, with one partly filled workgroup


@pytest.mark.parametrize("case", family("B3", GEOMETRY), ids=ids(family("B3", GEOMETRY)))
def test_b3_far_frames_change_nothing(case):
    want = DA.wanted(case)
    frames = list(case.frames)
    for k in case.far:
        assert max(abs(v) for v in case.offsets[k]) >= 1e3
        frames[k] = np.full(frames[k].shape, np.nan, F)     # same frame_count, same cap, no sample
    args = case.args()
    without = R.drizzle(frames, *args[1:])
    assert without.image.tobytes() == want.image.tobytes() and without.weight.tobytes() == want.weight.tobytes()
    assert without.rejected == want.rejected and np.array_equal(without.counts, want.counts)
    xs = [case.offsets[k][0] for k in case.far]
    ys = [case.offsets[k][1] for k in case.far]
    assert min(xs) <= -1e3 and max(xs) >= 1e3 and min(ys) <= -1e3 and max(ys) >= 1e3


def test_b3_covers_every_magnitude():
    mags = sorted({max(abs(v) for o in c.offsets for v in o) for c in family("B3", GEOMETRY)})
    assert mags == sorted([1e3, 1e6, 2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5, 1e9, 1e12, 1e18, 1e300])


@pytest.mark.parametrize("case", family("B4", GEOMETRY), ids=ids(family("B4", GEOMETRY)))
def test_b4_frames_fall_on_either_side_of_the_cut(case):
    want = DA.wanted(case)
    sigma = max(case.pixfrac * case.scale * 0.5, 0.5)
    args = case.args()
    for sign, start, stop in case.note:
        for k in range(start, stop):
            frames = list(case.frames)
            frames[k] = np.full(frames[k].shape, np.nan, F)
            without = R.drizzle(frames, *args[1:])
            pushes = int((want.counts - without.counts).sum())
            inside = 7.44 * sigma + sign * 0.01 < np.sqrt(2.0 * np.log(1e12)) * sigma
            assert (pushes > 0) == inside, (k, sign, pushes)
            if pushes:          # only border pixels receive anything from a frame that lies wholly off the field
                changed = want.counts != without.counts
                assert not changed[1:-1, 1:-1].any()
    assert {s for s, _, _ in case.note} == {-1.0, 1.0}
    if sigma < 1.0:
        assert 7.44 * sigma - 0.01 < np.sqrt(2.0 * np.log(1e12)) * sigma < 7.44 * sigma     # the cut lies between the two


def test_b5_outputs_are_whole_workgroups():
    dims = sorted({DA.wanted(c).dims[2:] for c in family("B5", GEOMETRY)})
    assert dims == [(4, 64), (8, 128)]
    assert {len(c.frames) for c in family("B5", GEOMETRY)} == {5, 33}
    assert {c.kernel for c in family("B5", GEOMETRY)} == set(DA.KERNELS)
