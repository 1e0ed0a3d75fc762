"""The crafted star lists of tests/triangle_cases.py on the CPU: (i) every family still does the job its docstring states, checked
with the restatement (tests/affine_restatement.py); (ii) the families bite -- a restatement with one deliberate mistake differs
from the true one on the family built for that mistake and on no other family's requirement; (iii) the library's HOST matcher
(ab_triangle_votes_host, ab_matches_from_votes, ab_affine_from_stars: host code, no device needed) equals the restatement on every
list pair, every cell.  Votes and indices are integers: everything is compared exactly.  tests/test_gpu_triangle_votes.py holds
the device matcher to the same matrices."""
import ctypes
import itertools

import numpy as np
import pytest

import affine_restatement as ar
import triangle_cases as tc

NAMES = list(tc.CASES)


def stars(xy):
    return [tuple(map(float, p)) for p in xy]


def triangles(xy):
    return ar.build_triangles(stars(xy))


def bucket_counts(xy):
    return np.bincount(tc.tri_bin(np.array([t[1] for t in triangles(xy)])), minlength=tc.TRI_BINS)


def sorted_pairs(votes):
    """the voted pairs in the pinned order: votes descending, then (ref, tgt)"""
    return sorted((-int(votes[r, t]), r, t) for r in range(64) for t in range(64) if votes[r, t] > 0)


def tie_positions(xy):
    """which neighbours of the stable three-element sorts tie, over all triangles of a list: {(0, 1), (1, 2), (0, 1, 2)} ..."""
    s, seen = stars(xy), set()
    for i, j, k in itertools.combinations(range(min(len(s), 60)), 3):
        d = sorted([ar.dist(s[i], s[j]), ar.dist(s[j], s[k]), ar.dist(s[i], s[k])])
        if d[0] == d[1] == d[2]:
            seen.add((0, 1, 2))
        elif d[0] == d[1]:
            seen.add((0, 1))
        elif d[1] == d[2]:
            seen.add((1, 2))
    return seen


# ---- (i) the conditions ---------------------------------------------------------------------------------------------------------
def test_n_counts_groups_and_the_voting_limit():
    # 4 and 56 reference triangles fit one group of 64 lanes, 84 give a second group with 20 live lanes
    assert [len(triangles(tc.n_list(k))) for k in (4, 8, 9)] == [4, 56, 84]
    assert (84 + 63) // 64 == 2 and 84 - 64 == 20
    # the builder's threads clear the vote matrices from 26 stars on, a memset below (4 copies of 64 x 64 words, 256-thread blocks)
    assert -(-25 ** 3 // 256) * 256 < 4 * 4096 <= 26 ** 3
    assert len(triangles(tc.CLUSTER)) == 0 and len(tc.CLUSTER) == 12


@pytest.mark.parametrize("k", tc.N_COUNTS)
@pytest.mark.parametrize("side", ["ref", "tgt"])
def test_n_only_the_first_60_stars_of_a_list_vote(side, k):
    v = tc.want_case(f"N {side} {k} stars")
    assert v.sum() > 0                                           # the moved field matches the field
    assert not v[60:, :].any() and not v[:, 60:].any()           # stars 60 and above receive no vote
    if k < 60:
        assert not (v[k:, :] if side == "ref" else v[:, k:]).any()


@pytest.mark.parametrize("name", ["no", "one", "three", "cluster"])
def test_n_lists_without_a_triangle_have_no_votes(name):
    assert not tc.want_case(f"N ref {name}").any() and not tc.want_case(f"N tgt {name}").any()


def test_s_the_15_px_side_decides_exactly_the_triangles_of_that_pair():
    s = stars(tc.S_EXACT)
    assert ar.dist(s[0], s[1]) == 15.0 and ar.dist(*stars(tc.S_SHORT)[:2]) < 15.0
    # the triangles that have the pair as their shortest side: one per other star, all of them far away
    with_pair = [c for c in s[2:] if min(ar.dist(s[0], c), ar.dist(s[1], c)) >= 15.0]
    assert len(with_pair) == 10
    kept, dropped = triangles(tc.S_EXACT), triangles(tc.S_SHORT)
    assert len(kept) - len(dropped) == len(with_pair)
    assert {t[0] for t in kept} - {t[0] for t in dropped} == {(0, 1, c) for c in range(2, 12)}
    assert tc.want_case("S exactly 15 px").sum() > tc.want_case("S exact against short").sum() > 0


@pytest.mark.parametrize("name,ties,fullest", [("LATTICE_8", {(0, 1), (1, 2)}, 2697), ("LATTICE_10X6", {(0, 1), (1, 2)}, 2444),
                                               ("LATTICE_3X3", {(0, 1), (1, 2)}, 36), ("SUBLATTICE_9X5", {(0, 1), (1, 2)}, 1196),
                                               ("LINE_60", {(0, 1)}, 1140), ("EQUILATERAL", {(0, 1, 2)}, None)])
def test_e_equal_sides_and_full_buckets(name, ties, fullest):
    """(0, 1): the two shortest sides are equal, (1, 2): the two longest, (0, 1, 2): all three -- no square lattice holds an
    equilateral triangle, hence the list built around two.  A collinear triple has sides a, a, 2a at best.  Buckets of more than
    1024 triangles stay unordered in the reference table (tri_bucket_sort_kernel); the 3 x 3 lattice's stay below."""
    xy = getattr(tc, name)
    assert ties <= tie_positions(xy) and (name != "LINE_60" or tie_positions(xy) == ties)
    if fullest is not None:
        assert int(bucket_counts(xy).max()) == fullest
    if name == "LATTICE_3X3":
        assert len(triangles(xy)) == 84


def test_e_tied_maxima_and_lists_of_different_lengths():
    v = tc.want_case("E lattice 10x6")
    assert int((v == v.max()).sum()) == 8              # cells that tie for the maximum
    assert len(tc.LATTICE_8) == 60 and len(tc.SUBLATTICE_9X5) == 45 and tc.want_case("E lattice 8x8 against 9x5").sum() > 0


def test_b_the_last_bucket_is_full_and_matches_straddle_it():
    tr = triangles(tc.B_LIST)
    mid = np.array([t[1] for t in tr])
    lng = np.array([t[2] for t in tr])
    bins = tc.tri_bin(mid)
    assert len(tr) == 58 and 82.6 < mid.min() < 82.7 and 83.6 < mid.max() < 83.7
    cnt = np.bincount(bins, minlength=tc.TRI_BINS)
    assert (cnt[4090:] > 0).all() and cnt[4095] == 43 and cnt[4094] > 0
    assert (mid[bins == 4095] - 1.0).max() / (0.02 * 1.0001) > 4096   # the clamp is at work: these would be buckets past the last
    hit = ~(np.abs(mid[:, None] - mid[None, :]) > 0.02) & ~(np.abs(lng[:, None] - lng[None, :]) > 0.02)
    assert int(hit.sum()) == 172 == int(tc.want_case("B last bucket").sum()) // 3
    assert (hit & (bins[:, None] == 4094) & (bins[None, :] == 4095)).any()   # an accepted pair straddles the two buckets


def test_t_one_step_either_side_of_the_tolerance():
    r0 = tc._ratios(*stars(tc.T_REF[:3]))
    for which, kind in ((0, "mid"), (1, "long")):
        r_in, r_out = (tc._ratios(*stars(tc.T_TARGETS[f"{kind} {side}"][:3])) for side in ("in", "out"))
        d_in, d_out = abs(r0[which] - r_in[which]), abs(r0[which] - r_out[which])
        assert not d_in > 0.02 and d_out > 0.02
        assert abs(d_in - 0.02) <= 1e-14 and abs(d_out - 0.02) <= 1e-14
        other = 1 - which
        assert abs(r0[other] - r_in[other]) < 0.017 and abs(r0[other] - r_out[other]) < 0.017   # the other ratio is inside
        assert int(tc.want_case(f"T {kind} in").sum()) == 3 and int(tc.want_case(f"T {kind} out").sum()) == 0
    for side in ("in", "out"):   # across a bucket boundary
        assert (int(tc.tri_bin(r0[0])), int(tc.tri_bin(tc._ratios(*stars(tc.T_TARGETS[f"mid {side}"][:3]))[0]))) == (24, 25)


@pytest.mark.parametrize("name,last", [("U unrelated", None), ("U lattice 8x8", 2921)])
def test_u_the_greedy_pass_goes_deep(name, last):
    v = tc.want_case(name)
    ref, tgt = tc.CASES[name]
    pairs = sorted_pairs(v)
    assert len(pairs) > 1024                        # the host sorts only the best 512 up front
    m = ar.matches_from_votes(v, len(ref), len(tgt))
    pos = pairs.index((-int(v[m[-1]]), m[-1][0], m[-1][1]))
    assert pos > 512 and (last is None or pos == last)


def test_g_is_two_groups_of_every_kind():
    assert len(tc.GROUP_TARGETS) == 11 and [len(t) for t in tc.GROUP_TARGETS] == [60, 0, 3, 12, 60, 61, 60, 25, 26, 4, 130]


# ---- (ii) the families bite -----------------------------------------------------------------------------------------------------
def requirements():
    """One cheap requirement per family, computed with the restatement AS IT STANDS (a test may have planted a mistake in it)."""
    req = {}
    req["S"] = (len(triangles(tc.S_EXACT)), len(triangles(tc.S_SHORT)))
    req["E"] = tuple(tuple(ar.sort_triangle_vertices(stars(xy), idx)) for xy in (tc.LATTICE_3X3, tc.EQUILATERAL)
                     for idx in itertools.combinations(range(len(xy)), 3))
    v_ref, v_tgt = ar.triangle_votes(tc.n_list(61), tc.n_list(25)), ar.triangle_votes(tc.n_list(25), tc.n_list(61))
    req["N"] = (tuple(len(triangles(tc.n_list(k))) for k in (4, 8, 9)), bool(v_ref[60:].any()), bool(v_tgt[:, 60:].any()), bool(v_ref.any()))
    req["T"] = tuple(int(ar.triangle_votes(tc.T_REF, tc.T_TARGETS[k]).sum()) for k in ("mid in", "mid out", "long in", "long out"))
    req["U"] = tuple(tuple(ar.matches_from_votes(tc.want_case(n), 60, 60)) for n in ("U unrelated", "U lattice 8x8"))   # (the true votes)
    tr = triangles(tc.B_LIST)
    req["B"] = (len(tr), tuple(np.bincount(tc.tri_bin(np.array([t[1] for t in tr])), minlength=tc.TRI_BINS)[4090:]))
    return req


TRUE = {}


def true_requirements():
    if not TRUE:
        TRUE.update(requirements())
        assert TRUE["S"] == (220, 210) and TRUE["T"] == (3, 0, 3, 0) and TRUE["N"] == ((4, 56, 84), False, False, True)
    return TRUE


def _le_at_15(stars_):
    out = []
    for i, j, k in itertools.combinations(range(min(len(stars_), ar.VOTING_STARS)), 3):
        sides = sorted([ar.dist(stars_[i], stars_[j]), ar.dist(stars_[j], stars_[k]), ar.dist(stars_[i], stars_[k])])
        if sides[0] <= ar.MIN_TRIANGLE_SIDE:
            continue
        out.append(((i, j, k), sides[1] / sides[0], sides[2] / sides[0]))
    return out


def _ties_reversed(stars_, idx):
    i, j, k = idx
    verts = [(i, ar.dist(stars_[j], stars_[k])), (j, ar.dist(stars_[i], stars_[k])), (k, ar.dist(stars_[i], stars_[j]))]
    verts.reverse()
    verts.sort(key=lambda v: v[1])
    return [v[0] for v in verts]


def _mid_only(rt, t_mid, t_long):
    return np.flatnonzero(~(np.abs(rt[1] - t_mid) > ar.TRIANGLE_TOLERANCE))


_true_greedy = ar.matches_from_votes


def _ties_by_tgt(votes, n_ref, n_tgt, tie_break=None):
    return _true_greedy(votes, n_ref, n_tgt, tie_break=lambda pair: (pair[1], pair[0]))


MUTATIONS = [("S", "<= for < at the 15 px side", "build_triangles", _le_at_15),
             ("E", "vertex ties broken in reverse", "sort_triangle_vertices", _ties_reversed),
             ("N", "61 voting stars", "VOTING_STARS", 61),
             ("T", "tolerance applied to ratio_mid only", "hit_indices", _mid_only),
             ("U", "greedy ties by (tgt, ref)", "matches_from_votes", _ties_by_tgt)]


@pytest.mark.parametrize("family,what,attr,mutant", MUTATIONS, ids=[m[1] for m in MUTATIONS])
def test_a_planted_mistake_changes_its_family_and_no_other(monkeypatch, family, what, attr, mutant):
    true = true_requirements()
    monkeypatch.setattr(ar, attr, mutant)
    got = requirements()
    assert got[family] != true[family], what
    for other in true:
        if other != family:
            assert got[other] == true[other], (what, other)


# ---- (iii) the library's host matcher -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_votes_and_matches_equal_the_restatement(name):
    import astroburst_amd as ab
    ref, tgt = tc.CASES[name]
    want = tc.want_case(name)
    got = ab.triangle_votes_host(ref, tgt)
    assert got.dtype == np.uint32 and got.shape == (64, 64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, bad[:8].tolist())
    assert ab.matches_from_votes(want, len(ref), len(tgt)) == ar.matches_from_votes(want, len(ref), len(tgt))


def same(res, want):   # as in tests/test_affine_restatement.py: exact
    if want is None:
        assert res is None
        return
    assert res is not None
    assert res.method == want["method"] and res.inliers == want["inliers"] and res.matched_stars == want["matched_stars"]
    assert tuple(res.transform) == tuple(want["transform"]), (res.transform, want["transform"])
    assert res.residual_px == want["residual_px"]


EU = [n for n in NAMES if n[0] in "EU" and n != "U lattice 8x8"]


@pytest.mark.parametrize("name", EU)
@pytest.mark.parametrize("threads", [1, 8])
def test_host_affine_from_stars_equals_the_restatement(name, threads):
    """the whole host chain on the lists with tied votes and a deep greedy pass: triangles -> votes -> matches -> RANSAC -> sanity.
    (The restatement's chain from its cached vote matrix on: ar.affine_from_votes is the tail of ar.affine_from_stars.)"""
    from astroburst_amd import _lib
    from astroburst_amd.core import AFFINE_METHODS, AffineAlignResult
    ref, tgt = tc.CASES[name]
    r, t = np.ascontiguousarray(ref, np.float64), np.ascontiguousarray(tgt, np.float64)
    res, found = _lib.AffineAlignResultC(), ctypes.c_int(0)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = _lib.lib().ab_affine_from_stars(r.ctypes.data_as(dp), r.shape[0], t.ctypes.data_as(dp), t.shape[0], 4096, 4096, threads,
                                         ctypes.byref(res), ctypes.byref(found))
    assert rc == _lib.AB_OK
    got = AffineAlignResult(tuple(res.transform), int(res.matched_stars), int(res.inliers), res.residual_px, AFFINE_METHODS[res.method]) if found.value else None
    same(got, ar.affine_from_votes(ref, tgt, tc.want_case(name), 4096, 4096, num_threads=threads))


def test_argument_errors():
    import astroburst_amd as ab
    from astroburst_amd import _lib
    L = _lib.lib()
    dp, up, sp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_size_t)
    xy = np.ascontiguousarray(tc.n_list(8))
    votes = np.zeros((64, 64), np.uint32)
    n = ctypes.c_size_t(0)
    idx = (ctypes.c_size_t * 64)()
    p, v = xy.ctypes.data_as(dp), votes.ctypes.data_as(up)
    assert L.ab_triangle_votes_host(None, 8, p, 8, v) == _lib.AB_ERR_INVALID
    assert L.ab_triangle_votes_host(p, 8, None, 8, v) == _lib.AB_ERR_INVALID
    assert L.ab_triangle_votes_host(p, 8, p, 8, None) == _lib.AB_ERR_INVALID
    assert L.ab_matches_from_votes(8, 8, None, idx, idx, 64, ctypes.byref(n)) == _lib.AB_ERR_INVALID
    assert L.ab_matches_from_votes(8, 8, v, None, idx, 64, ctypes.byref(n)) == _lib.AB_ERR_INVALID
    assert L.ab_matches_from_votes(8, 8, v, idx, None, 64, ctypes.byref(n)) == _lib.AB_ERR_INVALID
    assert L.ab_matches_from_votes(8, 8, v, idx, idx, 64, None) == _lib.AB_ERR_INVALID
    assert L.ab_triangle_votes_device(None, p, 8, p, ctypes.cast(idx, sp), 1, 0, v) == _lib.AB_ERR_INVALID   # no context
    for bad in (np.nan, np.inf, -np.inf):
        for where in (0, 15):   # (x of the first star, y of the last)
            broken = xy.copy()
            broken.reshape(-1)[where] = bad
            votes[:] = 7
            with pytest.raises(ab.AstroBurstError) as e:
                ab.triangle_votes_host(broken, xy)
            assert e.value.code == _lib.AB_ERR_INVALID
            with pytest.raises(ab.AstroBurstError):
                ab.triangle_votes_host(xy, broken)
    # a non-finite coordinate beyond the voting stars is refused as well: the list is what is judged, not the part that is used
    long_list = np.vstack([tc.n_list(130), [[np.nan, 1.0]]])
    with pytest.raises(ab.AstroBurstError):
        ab.triangle_votes_host(long_list, xy)
    # capacity: the first `cap` pairs are written, the count is the whole number
    want = tc.want_case("N ref 8 stars")
    full = ab.matches_from_votes(want, 8, 60)
    assert len(full) == 8
    ri, ti = (ctypes.c_size_t * 3)(), (ctypes.c_size_t * 3)()
    assert L.ab_matches_from_votes(8, 60, want.ctypes.data_as(up), ri, ti, 3, ctypes.byref(n)) == _lib.AB_OK
    assert n.value == 8 and [(ri[i], ti[i]) for i in range(3)] == full[:3]
    assert L.ab_matches_from_votes(8, 60, want.ctypes.data_as(up), None, None, 0, ctypes.byref(n)) == _lib.AB_OK and n.value == 8
    # empty lists and an all-zero matrix are answers, not errors
    assert not ab.triangle_votes_host(np.zeros((0, 2)), xy).any() and ab.matches_from_votes(votes * 0, 60, 60) == []
