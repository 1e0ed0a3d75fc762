"""The adversarial stack fixtures (tests/stack_adversarial.py) against the CPU oracle: every fixture does what it claims.

A fixture that stops being adversarial -- a tie that no longer sits on its threshold, a sum that became exact -- fails here rather
than passing silently on the GPU (tests/test_gpu_stack_adversarial.py).
"""
import numpy as np
import pytest

import stack_adversarial as sa

F32 = np.float32


def sum_is_exact(values):
    """True when an f64 sum of these f32 samples is exact in every order: all are multiples of the smallest quantum q among them and
    the sum of their magnitudes is below 2^53 q"""
    v = np.asarray(values, F32)
    v = v[np.isfinite(v) & (v != 0)].astype(np.float64)
    if v.size == 0:
        return True
    m, e = np.frexp(v)
    mant = np.abs(m * 2.0 ** 24).astype(np.int64)
    tz = [(int(mi) & -int(mi)).bit_length() - 1 for mi in mant]
    low = [int(ei) - 24 + t for ei, t in zip(e, tz)]                 # exponent of each sample's lowest set bit
    q = min(low)
    total = sum((int(mi) >> t) << (lo - q) for mi, t, lo in zip(mant, tz, low))
    return total < 2 ** 53


def survivors(values, sl, sh, it):
    """the samples the restatement keeps (every subset of an exactly-summable set is exactly summable, but not the reverse)"""
    _, _, trace = sa.clip_reference(values, sl, sh, it)
    v = np.asarray(values, F32)
    if not trace:
        return v[np.isfinite(v)]
    center, _, lo, hi, before = trace[-1]
    dev = before - center
    return before[(dev >= lo) & (dev <= hi)]


@pytest.mark.parametrize("n", sa.N_LIST)
def test_threshold_ties_flip_on_the_oracle(oracle, n):
    """each T pixel: the oracle equals the restatement, and its twin (boundary sample one ulp outside) changes both the rejected
    count and the value; every sample set sums exactly (so bit equality is owed by every engine)"""
    sets = sa.fixture_sets("T", n)
    count = 0
    for fs in sets:
        for px in fs.pixels:
            val, rej = oracle.sigma_clip_combine(px.values, fs.sl, fs.sh, fs.it)
            tval, trej = oracle.sigma_clip_combine(px.twin.values, fs.sl, fs.sh, fs.it)
            rv, rr, _ = sa.clip_reference(px.values, fs.sl, fs.sh, fs.it)
            assert (val, rej) == (rv, rr), px.name
            assert rej != trej, (px.name, rej, trej)
            assert val != tval, (px.name, val, tval)
            assert sum_is_exact(px.values) and sum_is_exact(px.twin.values[px.twin.values != px.twin.values[px.meta["idx"]]]), px.name
            count += 1
    if n >= 8:
        assert count > 0
    # coverage: ranks past the fast passes' eight samples per end, at iteration 0 and at iteration 1, on both ends
    got = {(p.meta["iteration"], p.meta["rank"], p.meta["side"]) for fs in sets for p in fs.pixels}
    want_it0 = [r for r in sa.RANKS if 2 * r + 1 <= n // 2]
    want_it1 = [r for r in sa.RANKS if n >= 16 * r] if n >= 16 else []
    for side in (1, -1):
        assert all((0, r, side) in got for r in want_it0), (n, sorted(got))
        assert all((1, r, side) in got for r in want_it1), (n, sorted(got))
    if n >= 256:
        assert {r for (i, r, s) in got if i == 1} == set(sa.RANKS)


def test_threshold_tie_of_the_issue(oracle):
    """64 samples: 7 at mu, 27 pairs at mu +- 4, mu +- 8, an outlier at mu + 1000; kappa 2 / 2, 5 iterations.  Iteration 1 has mean mu
    and sigma 4 exactly: the +-8 samples are on the threshold and kept; either one moved one ulp outwards is rejected."""
    mu = F32(300.0)
    v = np.array([mu] * 7 + [mu + 4] * 27 + [mu - 4] * 27 + [mu + 8, mu - 8, mu + 1000], F32)
    assert oracle.sigma_clip_combine(v, 2.0, 2.0, 5)[1] == 1
    for k in (61, 62):
        t = v.copy()
        t[k] = np.nextafter(t[k], F32(np.inf) if t[k] > mu else F32(-np.inf))
        assert oracle.sigma_clip_combine(t, 2.0, 2.0, 5)[1] == 3


@pytest.mark.parametrize("n", sa.N_LIST)
def test_wide_sums_depend_on_the_order(oracle, n):
    """each W pixel: magnitudes spanning more than 2^30, and an ascending f64 sum that differs from the descending or pairwise one"""
    for fs in sa.fixture_sets("W", n):
        for px in fs.pixels:
            a, d, p = sa.order_sums(px.values)
            assert a != d or a != p, px.name
            assert px.meta["span"] > 2.0 ** 30, px.name
            assert not sum_is_exact(px.values), px.name
    # and the oracle's plain mean (max_iter 0) is the ascending sum's
    fs = next(f for f in sa.fixture_sets("W", n) if f.it == 0)
    for px in fs.pixels:
        val, rej = oracle.sigma_clip_combine(px.values, fs.sl, fs.sh, 0)
        assert rej == 0 and val == F32(sa.ascending_sum(px.values) / px.values.size), px.name


@pytest.mark.parametrize("n", sa.N_LIST)
def test_moment_switch_sides(oracle, n):
    """M pixels: the iteration-0 median (oracle selection) lies at c * sigma0 on the intended side of the raw / centred switch
    |median| <= 1024 sigma0, and both sides are present"""
    sides = set()
    for px in [p for fs in sa.fixture_sets("M", n) if fs.sl == 2.0 for p in fs.pixels]:
        v = px.values[np.isfinite(px.values)]
        med = F32(oracle.select_nth(v, v.size // 2)[v.size // 2])
        dev = np.abs(v - med).astype(F32)
        mad = F32(oracle.select_nth(dev, dev.size // 2)[dev.size // 2])
        sig0 = F32(max(float(mad) * sa.MAD_TO_SIGMA, 1e-10))
        raw = bool(abs(med) <= F32(1024.0) * sig0)
        assert raw == px.meta["raw"] and med == F32(px.meta["median"]), px.name
        c = px.meta["c"]
        if c in (1023.0, 1024.0, "c1023", "c1024"):
            assert raw, px.name
        else:
            assert not raw, px.name
        if c in (1024.0, "c1024"):
            assert med == F32(1024.0) * sig0, px.name       # exactly on the switch
        sides.add(raw)
    if n >= 3:
        assert sides == {True, False}


@pytest.mark.parametrize("n", sa.N_LIST)
def test_edge_pixels_sum_exactly(oracle, n):
    """E pixels: the survivors' f64 sums are exact (the engines owe bit equality), except the one tagged `inexact`, which the GPU test
    holds to the W assertions; the restatement equals the oracle"""
    for fs in sa.fixture_sets("E", n):
        for px in fs.pixels:
            fin = px.values[np.isfinite(px.values)]                 # (the stack hands sigma_clip_combine the finite samples)
            val, rej = oracle.sigma_clip_combine(fin, fs.sl, fs.sh, fs.it)
            rv, rr, _ = sa.clip_reference(px.values, fs.sl, fs.sh, fs.it)
            assert rej == rr and (val == rv or (np.isnan(val) and np.isnan(rv))), (px.name, val, rv)
            exact = sum_is_exact(survivors(px.values, fs.sl, fs.sh, fs.it))
            assert exact != px.meta.get("inexact", False), (px.name, fs.sl, fs.sh, fs.it)


@pytest.mark.parametrize("n", sa.N_LIST)
def test_batch_ties_flip_on_the_oracle(oracle, n):
    """each B pixel: z == kappa exactly (rejected under the strict comparisons), the twin one ulp inside is kept (per-frame counts and
    value differ), the twin one ulp outside is rejected like the tie"""
    sets = sa.fixture_sets("B", n)
    for fs in sets:
        for px in fs.pixels:
            res = {}
            for key, p in (("tie", px), ("in", px.twin), ("out", px.twin_out)):
                fr = [np.array([[x]], F32) for x in p.values]
                out, rej = oracle.sigma_clipped_mean_stack(fr, fs.sl, fs.sh, fs.it)
                res[key] = (out[0, 0], rej)
            assert res["tie"][1][px.meta["idx"]] == 1 and res["out"][1][px.meta["idx"]] == 1, px.name
            assert res["in"][1][px.meta["idx"]] == 0, px.name
            assert res["tie"][1] != res["in"][1] and res["tie"][0] != res["in"][0], px.name
    if n >= 8:
        assert sum(len(fs.pixels) for fs in sets) > 0


@pytest.mark.parametrize("layout", ["mult16", "odd", "rows"])
def test_pack_layouts(layout):
    px = [p for fs in sa.fixture_sets("E", 9) for p in fs.pixels][:20]
    frames, P = sa.pack(px, layout, rows=3)
    total = frames[0].size
    assert len(frames) == 9 and P == 20
    assert (total % 16 == 0) == (layout == "mult16")
    flat = np.stack([f.ravel() for f in frames])
    for k in range(total):
        assert np.array_equal(flat[:, k], px[k % P].values, equal_nan=True)


def _oracle_side(oracle, values):
    """the moment switch from the oracle's own selection: |median| <= 1024 sigma0 (None with fewer than two finite samples)"""
    v = np.asarray(values, F32)
    v = v[np.isfinite(v)]
    if v.size < 2:
        return None
    med = F32(oracle.select_nth(v, v.size // 2)[v.size // 2])
    dev = np.abs(v - med).astype(F32)
    mad = F32(oracle.select_nth(dev, dev.size // 2)[dev.size // 2])
    return bool(abs(med) <= F32(1024.0) * F32(max(float(mad) * sa.MAD_TO_SIGMA, 1e-10)))


@pytest.mark.parametrize("n", sa.N_LIST)
def test_every_wave_runs_the_intended_moment_form(oracle, n):
    """the kernels choose raw or centred moments per wave (every lane must be within 1024 sigma0 for the raw form), so each T, W and
    M set is of one side: every 64-pixel wave of every packed layout is uniformly on the set's side, and both forms are exercised"""
    sides = {}
    for family in "TWM":
        for fs in sa.fixture_sets(family, n):
            assert fs.raw in (True, False), (family, fs.sl, fs.sh, fs.it)
            for layout in ("mult16", "odd", "rows"):
                frames, _ = sa.pack(fs.all_pixels(), layout, rows=3)
                flat = np.stack([f.ravel() for f in frames])
                for w0 in range(0, flat.shape[1], 64):
                    got = {_oracle_side(oracle, flat[:, k]) for k in range(w0, min(w0 + 64, flat.shape[1]))}
                    assert got == {fs.raw}, (family, layout, fs.sl, fs.sh, fs.it, w0, got)
            sides.setdefault(family, set()).add(fs.raw)
    assert sides["M"] == {True, False}
    assert sides["T"] == {True, False}
    # the raw tail gets iteration-1 ties and the medians at 1023 / 1024 sigma0 (the raw form at its worst cancellation)
    raw_t = [p for fs in sa.fixture_sets("T", n) if fs.raw for p in fs.pixels]
    cen_t = [p for fs in sa.fixture_sets("T", n) if not fs.raw for p in fs.pixels]
    if n >= 16:
        assert any(p.meta["iteration"] == 1 for p in raw_t) and any(p.meta["iteration"] == 1 for p in cen_t)
    raw_m = {p.meta["c"] for fs in sa.fixture_sets("M", n) if fs.raw for p in fs.pixels}
    assert {1023.0, 1024.0} <= raw_m
    if n >= 64:
        assert {"c1023", "c1024"} <= raw_m                  # (the exact-arithmetic ties on the switch)


@pytest.mark.parametrize("n", sa.N_LIST)
def test_every_listed_centre_is_built(n):
    """each centre of IT0_MU is built at every n (iteration-0 ties), each of IT1_MU from 16 frames on (iteration-1 ties), on both
    ends"""
    sets = sa.fixture_sets("T", n)
    for iteration, kinds, n_min in ((0, [k for k, _ in sa.IT0_MU], 3), (1, list(sa.IT1_MU), 16)):
        if n < n_min:
            continue
        for side in (1, -1):
            built = {p.meta["mu_kind"] for fs in sets for p in fs.pixels if p.meta["iteration"] == iteration and p.meta["side"] == side}
            assert built == set(kinds), (iteration, side, sorted(built))


@pytest.mark.parametrize("n", sa.N_LIST)
def test_cancelling_overflow_pixel(oracle, n):
    """the E pixel whose MAD overflows: sigma0 is inf (nothing is clipped), and its samples do not sum exactly"""
    px = next(p for p in sa.fixture_sets("E", n)[0].pixels if p.name == "cancelling overflow")
    _, _, trace = sa.clip_reference(px.values, 3.0, 3.0, 5)
    assert np.isinf(trace[0][1]) and oracle.sigma_clip_combine(px.values, 3.0, 3.0, 5)[1] == 0
    assert not sum_is_exact(px.values)
