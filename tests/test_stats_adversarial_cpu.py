"""The fixtures of tests/stats_adversarial.py held to what they claim (no GPU): on every one the CPU oracle equals the numpy
statement (min, max, median, mad, sigma and valid_count `==`, the mean within the project's 1e-12 relative), the trace of the
histogram statement shows the edge the fixture is named after, the deviations of exact/deviation carry the intended bit patterns,
and over the whole list every branch the GPU test is meant to exercise is taken by at least one fixture.  A fixture that has drifted
fails here, so the GPU test (tests/test_gpu_stats_adversarial.py) cannot pass by testing nothing."""
import numpy as np
import pytest

import select_adversarial as SA
import stats_adversarial as A
import stats_protocol as SP

F32 = np.float32
_seen = {}         # fixture name -> (result, trace): filled by test_oracle_equals_the_statement, read by the coverage test


def expected(fx):
    if fx.name not in _seen:
        _seen[fx.name] = A.statement(fx.plane(), fx.known)
    return _seen[fx.name]


def assert_same(st: dict, o, what):
    for k in A.FIELDS_EXACT:
        assert st[k] == getattr(o, k), (what, k, st[k], getattr(o, k))
    assert abs(st["mean"] - o.mean) <= 1e-12 * abs(o.mean), (what, st["mean"], o.mean)


def test_fixture_list_covers_what_the_issue_names():
    names = set(A.BY_NAME)
    pops = SA.populations()
    assert len(pops) == 67
    for p in pops:
        assert {f"select/{p.name}/row", f"select/{p.name}/square"} <= names
    for pair in A.DEV_PAIRS:
        assert {m for m, _ in A.DEV_COUNTS} == {1, 2, 3, 255, 256, 257, 600_001, 600_002}
        for m, side in A.DEV_COUNTS:
            assert f"deviation/{pair}-{m}-{side}/row" in names
    assert {SA.PAIRS[p][2] for p in A.DEV_PAIRS} == {0, 1, 2}
    assert {"limit/4000000", "limit/4000001"} <= names
    for b in (64, 256, 32768, 65535):
        for which in ("last", "first"):
            for total in (3_999_998, 3_999_999):
                assert f"edge/{b}-{which}-{total}" in names
    for k in (64, 256, 4096):
        for c in (1_000_000, 1_000_001):
            assert f"dev-edge/{k}-{c}" in names
    assert {"known/100-900", "known/1-2", "known/2000-3000", "known/nan-bound", "known/min-ge-max", "known/exact-path"} <= names
    assert {f"quantised/{k}" for k in ("60000", "1e6", "integers", "two-random", "two-half", "two-half-plus-1", "wide")} <= names
    assert {f"shapes/{k}" for k in ("1x4000001", "2001x2000", "62x65536", "last-65536")} <= names


@pytest.mark.parametrize("fx", A.FIXTURES, ids=lambda f: f.name)
def test_oracle_equals_the_statement_and_the_trace_shows_the_edge(oracle, fx):
    plane = fx.plane()
    assert plane.dtype == F32 and plane.ndim == 2
    assert (plane.size <= A.EXACT_LIMIT) == (fx.path == "exact")
    if fx.family != "exact/select" or fx.meta["pop"] != "L0-big":     # (L0-big keeps its deciding copies at both ends)
        for c in SA.CONTAMINATION:       # every kind of contamination is in every plane
            assert (SA.bits_of(plane) == SA.bits_of(c)).any(), c
    st, trace = expected(fx)
    got = oracle.compute_image_stats_with_known_range(plane, *fx.known) if fx.known else oracle.compute_image_stats(plane)
    assert_same(st, got, fx.name)
    assert st["valid_count"] == int(SA.is_candidate(plane).sum())          # the two validity filters are one
    assert st["valid_count"] > 0 or fx.name.startswith("select/FLOOR-1/")  # (FLOOR-1 holds 1e-7f alone: no valid pixel, all zeros)
    assert (trace is None) == (fx.path == "exact")
    for path, want in fx.claims.items():
        if fx.path == "hist":
            assert A.lookup(trace, path) == want, (fx.name, path, A.lookup(trace, path), want)
        elif path == "median_f32":
            assert float(F32(st["median"])) == want, (fx.name, st["median"])
        else:
            assert st[path] == want, (fx.name, path, st[path], want)


def test_the_statement_agrees_with_the_sharded_protocol_and_the_forced_paths(oracle):
    """on one histogram plane: the traced statement is stats_protocol's own composition with a single band, and the oracle's forced
    histogram path; on one exact plane: the oracle's forced exact path"""
    fx = A.BY_NAME["edge/256-last-3999998"]
    st, _ = expected(fx)
    one = SP.stats_hist_sharded(fx.plane().ravel(), lambda a: a, lambda a: a)
    assert {k: one[k] for k in A.FIELDS_EXACT} == {k: st[k] for k in A.FIELDS_EXACT}
    assert_same(st, oracle.compute_image_stats(fx.plane(), path="hist"), fx.name)
    fx = A.BY_NAME["deviation/L0-256-even/square"]
    assert_same(expected(fx)[0], oracle.compute_image_stats(fx.plane(), path="exact"), fx.name)


# ---- exact/deviation: the bit patterns ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", A.DEV_PAIRS)
@pytest.mark.parametrize("m,side", A.DEV_COUNTS)
def test_deviations_carry_the_pair_bit_for_bit(pair, m, side):
    pop = A.deviation_population(pair, m, side)
    lower, upper, level = SA.PAIRS[pair]
    c = pop.values[SA.is_candidate(pop.values)]
    assert c.size == m == pop.count
    s = np.sort(c)
    median = (float(s[m // 2 - 1]) + float(s[m // 2])) / 2.0 if m % 2 == 0 else float(s[m // 2])
    assert F32(median) == A.DEV_M and (m == 2 or median == float(A.DEV_M))
    d32 = np.abs(c - F32(median))                                         # what the kernel forms, in f32
    assert np.array_equal(d32.astype(np.float64), np.abs(c.astype(np.float64) - float(A.DEV_M)))   # ... and it is exact
    d = np.sort(d32)
    allowed = {int(SA.key(F32(0.0))), int(SA.key(lower)), int(SA.key(upper)), int(SA.key(F32(2.0)))}
    assert set(int(b) for b in np.unique(SA.bits_of(d))) <= allowed
    want = pop.meta["want"]
    if m == 1:
        assert d[0] == 0.0
    elif m % 2 == 0:      # the two middle ranks straddle the pair's edge: they differ at `level` of the select and at no level above
        assert SA.key(d[m // 2 - 1]) == SA.key(lower) and SA.key(d[m // 2]) == SA.key(upper) and want == (lower, upper)
        lo_bins, up_bins = SA.level_bins(d[m // 2 - 1]), SA.level_bins(d[m // 2])
        assert lo_bins[:level] == up_bins[:level] and lo_bins[level] != up_bins[level]
    else:
        assert SA.key(d[m // 2]) == SA.key(want[0])
        if m > 3 and side == "lower":      # the last element of the lower bin: the next rank is across the edge
            assert SA.key(d[m // 2 + 1]) == SA.key(upper)
        if m > 3 and side == "upper":      # the first element of the upper bin
            assert SA.key(d[m // 2 - 1]) == SA.key(lower)


def test_half_of_the_select_populations_have_mad_zero():
    """why exact/deviation exists: on most of select_adversarial's populations the second select never meets an edge"""
    st = [A.exact_statement(p.values) for p in SA.populations()]
    assert sum(1 for x in st if x["valid_count"] > 0 and x["mad"] == 0.0) == 40 and sum(1 for x in st if x["valid_count"] == 0) == 1


# ---- hist: the values sit where the docstrings say ---------------------------------------------------------------------------------
def test_edge_values_sit_in_their_bin_and_sub_bin_exactly():
    for b in A.EDGE_BINS + tuple(x - 1 for x in A.EDGE_BINS):
        v = A.edge_values(b, 6)
        f = v.astype(np.float64)
        assert np.array_equal(f, 1.0 + b / 65536.0 + A.EDGE_SUB[np.arange(6) % 3] * 2.0 ** -23)
        assert np.array_equal(SP._bin((f - 1.0) * 65536.0, 65535), np.full(6, b))
        lo = 1.0 + b * (1.0 / 65536.0)
        assert np.array_equal(SP._bin((f - lo) * (65536.0 / 2.0 ** -16), 65535), 512 * A.EDGE_SUB[np.arange(6) % 3])


def test_every_named_branch_is_taken_by_some_fixture(oracle):
    """over the whole list (no fixture skipped): ranks on the last element of a bin that ends a 64-group and a 256-group, ranks on
    the first element of a bin that opens one, the deviation rank in the last bin of a group, not-found for the median alone and
    for median and MAD together, the known-range fall-backs, both paths at the 4 000 000 px limit"""
    traces = {fx.name: expected(fx)[1] for fx in A.HIST}
    assert len(traces) == len(A.HIST) == 39 and all(t is not None for t in traces.values())
    t = traces.values()
    last = [x for x in t if x["median"]["cum_is_half"] and x["median"]["rank"] == x["median"]["count"]]
    first = [x for x in t if x["median"]["rank"] == 1]
    assert any(x["median"]["mod64"] == 63 and x["median"]["mod256"] != 255 for x in last)
    assert any(x["median"]["mod256"] == 255 for x in last)
    assert any(x["median"]["mod64"] == 0 and x["median"]["mod256"] != 0 for x in first)
    assert any(x["median"]["mod256"] == 0 for x in first)
    assert any(x["median"]["bin"] == 65535 for x in first) and any(x["median"]["bin"] == 65534 for x in last)
    assert any(x["median"]["sub"] and x["median"]["sub"].get("cum_is_rank") and x["median"]["sub"]["bin"] == 65024 for x in last)
    assert any(x["median"]["sub"]["bin"] == 0 and x["median"]["sub"]["rank_in_bin"] == 1 for x in first)
    assert any(x["dev"]["mod64"] == 63 and x["dev"]["mod256"] != 255 for x in t) and any(x["dev"]["mod256"] == 255 for x in t)
    assert any(x["dev"]["cum_is_half"] for x in t)
    assert any(x["median"]["not_found"] and not x["mad"]["not_found"] for x in t)
    assert any(x["median"]["not_found"] and x["mad"]["not_found"] and x["median"]["bin"] == 65535 for x in t)
    assert any(x["median"]["not_found"] and x["mad"]["not_found"] and x["median"]["bin"] == 0 for x in t)
    assert any(x["mad"]["not_found"] and x["mad"]["region_total"] > 0 for x in t) and any(x["mad"]["region_total"] == 0 for x in t)
    assert all(x["mad"]["rank"] > 0 and x["median"]["rank"] > 0 for x in t)       # the two rank-0 branches: unreachable (module docstring)
    assert sum(1 for x in t if not x["known"]) >= 2 and not traces["known/nan-bound"]["known"] and not traces["known/min-ge-max"]["known"]
    assert A.BY_NAME["known/exact-path"].path == "exact" and A.BY_NAME["limit/4000000"].plane().size == A.EXACT_LIMIT
    assert A.BY_NAME["limit/4000001"].plane().size == A.EXACT_LIMIT + 1
    assert np.array_equal(SA.bits_of(A.BY_NAME["limit/4000001"].plane().ravel()[:-1]), SA.bits_of(A.BY_NAME["limit/4000000"].plane().ravel()))
    # exact path: the values' and the deviations' middle ranks straddle an edge at every level of the select
    for fam, key in (("exact/select", "values"), ("exact/deviation", "deviations")):
        levels = set()
        for fx in A.EXACT:
            if fx.family != fam or not fx.name.endswith("/row"):
                continue
            v = fx.plane().ravel()
            s = np.sort(v[SA.is_candidate(v)])
            m = s.size
            if m % 2 or m < 2:
                continue
            if key == "deviations":
                s = np.sort(np.abs(s - F32((float(s[m // 2 - 1]) + float(s[m // 2])) / 2.0)))
            a, b = SA.level_bins(s[m // 2 - 1]), SA.level_bins(s[m // 2])
            levels |= {lv for lv in range(3) if a[:lv] == b[:lv] and a[lv] != b[lv]}
        assert levels == {0, 1, 2}, (fam, levels)
    # the plane whose valid pixels all lie in the last 65 536
    p = A.BY_NAME["shapes/last-65536"].plane().ravel()
    assert not SA.is_candidate(p[:-65536]).any() and SA.is_candidate(p[-65536:]).sum() > 60000
