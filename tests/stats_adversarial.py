"""Adversarial planes for compute_image_stats (pure numpy, fixed seeds: no GPU, no library, no oracle import), and a traced numpy
statement of what the reference computes on them.

csrc/stats.hip, csrc/stats_resident.hpp and csrc/stf.hip find a rank in three separate ways:

  exact path (<= 4 000 000 px)   an 11/11/10-bit radix select of its own (select_hist_kernel / select_pick_kernel); the two middle
                                 ranks of an even count descend together, and the select runs a second time on |v - (float)median|
  histogram path, chain engine   block_find_rank: the 65 536 bins as 1024 groups of 64
  histogram path, resident       the same bin by a two-level 256 x 256 descent

Smooth random sky data never puts a rank on the first or last element of a bin, on a 64-bin group edge or a 256-bin coarse edge,
and never takes the "rank not found" fall-through of resolve_rank_in_hist (stats.rs:352).  The families here do, on purpose:

  exact/select      select_adversarial.populations() as they stand (their candidate filter IS the statistics' validity filter)
  exact/deviation   populations whose median is (or rounds to) DEV_M and whose deviations |v - DEV_M| at the middle ranks are
                    exactly a PAIRS pair: the SECOND select sees the rank pair straddle a bin edge at level 0, 1 and 2
  exact/limit       4 000 000 px (the last exact plane) and the same plane plus one pixel (the first histogram plane)
  hist/edge         range [1, 2]: the value 1 + b / 65536 + s * 2^-23 sits in bin b, sub-bin 512 s, exactly; the median's rank is
                    the last element below / the first element above a bin boundary at 64, 256, 32768 and 65535
  hist/dev-edge     the MAD's coarse rank lands in deviation bin k - 1 for k = 64, 256, 4096: the last bin of a group
  hist/known-range  ranges that miss the data: the median's and the MAD's refine histograms are (nearly) empty -> not found;
                    and the reference's fall-backs (a NaN bound, min >= max, a plane of <= 4 000 000 px)
  hist/quantised    bin width below the f32 spacing of the values, integers, two-valued planes split exactly, 2e-7 against 3e38
  hist/shapes       1 x 4 000 001, 2001 x 2000, 62 x 65 536 (62 whole workgroups of the resident engine), valid pixels in the last
                    65 536 only

Every plane is interleaved with select_adversarial.CONTAMINATION (NaN, +-inf, 0, -0, negatives, 1e-8, 1e-7) and shuffled.

Which deviation pairs exist: the candidates are DEV_M - d (or DEV_M + d), which must be valid pixels (finite, > 1e-7f) and exact in
f32 together with their difference from DEV_M.  That holds for L0, BINADE, L1 and L2 with DEV_M = 1.5.  TOP cannot be a deviation
(DEV_M + d overflows, DEV_M - d is negative), and FLOOR cannot either (d = 1e-7f has its last bit at 2^-47; DEV_M +- d would have
to lie below 2^-23 and above 1e-7 at once).  A single pixel deviates from itself by 0, so count 1 has MAD 0 by construction.

Two branches of the reference cannot be reached, and nothing here chases them:
  * rank 0 of the MAD (`below >= half`) with an automatic range: the exact and the coarse median lie in one bin, so the deviations
    about them differ by less than a bin width, and the MAD's region is widened by one bin on either side of the coarse bin;
  * rank 0 of the median: `before`, the count below the median's bin, is < half by the definition of that bin.

tests/test_stats_adversarial_cpu.py holds every fixture to what it claims here (against the CPU oracle and the trace), so that a
fixture that has drifted fails there and the GPU test (tests/test_gpu_stats_adversarial.py) cannot pass by testing nothing.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

import select_adversarial as SA
import stats_protocol as SP

F32 = np.float32
EXACT_LIMIT = 4_000_000          # stats.rs:18
BINS = SP.HIST_BINS
ZERO = dict(min=0.0, max=0.0, median=0.0, mad=0.0, sigma=0.0, mean=0.0, valid_count=0)   # ImageStats::default()
FIELDS_EXACT = ("min", "max", "median", "mad", "sigma", "valid_count")


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def exact_statement(plane) -> dict:
    """stats.rs:43-73 with math/median.rs:27-73: the median is the f64 mean of the two middle values of an even count; the MAD is
    taken of |v - f32(median)| in f32, with an F32 average for an even count"""
    v = np.asarray(plane, F32).ravel()
    with np.errstate(invalid="ignore"):
        s = np.sort(v[SP.valid(v)])
    m = s.size
    if m == 0:
        return dict(ZERO)
    if m % 2 == 0:
        median = (float(s[m // 2 - 1]) + float(s[m // 2])) / 2.0
    else:
        median = float(s[m // 2])
    d = np.sort(np.abs(s - F32(median)))
    mad = float((d[m // 2 - 1] + d[m // 2]) / F32(2.0)) if m % 2 == 0 else float(d[m // 2])
    return dict(min=float(s[0]), max=float(s[-1]), median=median, mad=mad, sigma=max(mad * SP.MAD_TO_SIGMA, 1e-30),
                mean=float(s.astype(np.float64).sum()) / m, valid_count=m)


def _rank_trace(hist, rank):
    """where `rank` (>= 1) lands in a 65 536-bin histogram: the bin, its count, the rank inside the bin"""
    cum = np.cumsum(hist)
    total = int(cum[-1])
    if total < rank:
        return dict(not_found=True, total=total, rank=rank)
    b = int(np.searchsorted(cum, rank, side="left"))
    before = int(cum[b] - hist[b])
    return dict(not_found=False, total=total, rank=rank, bin=b, count=int(hist[b]), rank_in_bin=rank - before,
                cum_is_rank=int(cum[b]) == rank, mod64=b % 64, mod256=b % 256)


def hist_statement(plane, known=None):
    """compute_stats_hist_core(gmin, gmax) (stats.rs:85-210) on the passes of stats_protocol with a single band -> (result, trace).
    `known` = (min, max) or None; a bound that is not finite or min >= max falls back to the scanned range (stats.rs:36-38)."""
    v = np.ascontiguousarray(plane, dtype=F32).ravel()
    with np.errstate(invalid="ignore"):
        use_known = known is not None and math.isfinite(known[0]) and math.isfinite(known[1]) and known[0] < known[1]
        if use_known:
            gmin, gmax = float(known[0]), float(known[1])
        else:
            nm = SP.scan_pass(v)
            gmin, gmax = -nm[0], nm[1]
            if gmin == np.finfo(np.float64).max:
                return dict(ZERO), None
        rng = max(gmax - gmin, 1e-30)
        bin_width, inv = rng / BINS, BINS / rng
        hist, s, total = SP.value_pass(v, gmin, inv)
        if total == 0:
            return dict(ZERO), None
        half = int(math.ceil(total * 0.5))
        median_bin = SP.find_percentile_bin(hist, total, 0.5)
        before = int(hist[:median_bin].sum())
        lo = gmin + median_bin * bin_width
        hi = lo + bin_width
        coarse = SP.interpolate_percentile(hist, total, 0.5, gmin, bin_width)
        dev_bw, dev_inv = rng / BINS, BINS / rng
        refine_range = max(hi - lo, 1e-30)
        refine, dev = SP.dev_pass(v, F32(coarse), dev_inv, lo, hi, BINS / refine_range)
        rank_in_bin = max(half - before, 0)
        median = SP.resolve_rank_in_hist(refine, rank_in_bin, lo, refine_range / BINS)
        mad_bin = SP.find_percentile_bin(dev, total, 0.5)
        e_lo, e_hi = max(mad_bin - 1, 0), min(mad_bin + 2, BINS)
        r_lo, r_hi = e_lo * dev_bw, e_hi * dev_bw
        mad_range = max(r_hi - r_lo, 1e-30)
        below, h = SP.mad_pass(v, F32(median), F32(r_lo), F32(r_hi), r_lo, BINS / mad_range)
        mad_rank = max(half - below, 0)
        mad = SP.resolve_rank_in_hist(h, mad_rank, r_lo, mad_range / BINS)
    cum_med = int(hist[:median_bin + 1].sum())
    cum_dev = int(dev[:mad_bin + 1].sum())
    trace = dict(
        total=total, half=half, known=bool(use_known),
        # the median's coarse bin, and where its rank lands among that bin's 65 536 sub-bins
        median=dict(bin=median_bin, count=int(hist[median_bin]), cum_is_half=cum_med == half, mod64=median_bin % 64,
                    mod256=median_bin % 256, rank=rank_in_bin, refine_total=int(refine.sum()),
                    not_found=int(refine.sum()) < rank_in_bin, sub=_rank_trace(refine, rank_in_bin) if rank_in_bin else None),
        # the deviation histogram's bin at `half`
        dev=dict(bin=mad_bin, count=int(dev[mad_bin]), cum_is_half=cum_dev == half, mod64=mad_bin % 64, mod256=mad_bin % 256,
                 rank=half - (cum_dev - int(dev[mad_bin]))),
        # the MAD's region and where its rank lands among the region's 65 536 sub-bins
        mad=dict(region=(e_lo, e_hi), below=below, rank=mad_rank, region_total=int(h.sum()), not_found=int(h.sum()) < mad_rank,
                 sub=_rank_trace(h, mad_rank) if mad_rank else None),
        below=below)
    res = dict(min=gmin, max=gmax, median=median, mad=mad, sigma=max(mad * SP.MAD_TO_SIGMA, 1e-30), mean=s / total, valid_count=total)
    return res, trace


def statement(plane, known=None):
    """compute_image_stats (known is None) / compute_image_stats_with_known_range (stats.rs:15-41) -> (result, trace | None)"""
    if np.asarray(plane).size <= EXACT_LIMIT:
        return exact_statement(plane), None
    return hist_statement(plane, known)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
@dataclass
class Fixture:
    name: str
    family: str
    build: "callable"            # () -> 2-D f32 plane (built on demand: a histogram plane is 16 MB)
    path: str                    # "exact" | "hist": the path the plane's pixel count selects
    known: "tuple | None" = None
    claims: dict = field(default_factory=dict)     # what the trace / the statement must show (tests/test_stats_adversarial_cpu.py)
    meta: dict = field(default_factory=dict)

    def plane(self) -> np.ndarray:
        return _plane_of(self.name)


@functools.lru_cache(maxsize=3)
def _plane_of(name):
    p = np.ascontiguousarray(BY_NAME[name].build(), dtype=F32)
    p.setflags(write=False)
    return p


def fill(cands, rows, cols, seed):
    """the candidates and CONTAMINATION (in turn) up to rows x cols pixels, shuffled"""
    n = rows * cols
    assert n - cands.size >= SA.CONTAMINATION.size, (n, cands.size)
    out = np.concatenate([np.asarray(cands, F32), np.resize(SA.CONTAMINATION, n - cands.size)])
    np.random.default_rng(seed).shuffle(out)
    return out.reshape(rows, cols)


def sprinkle(vals, every=97):
    """one element of CONTAMINATION (in turn) over every `every`-th pixel of a flat array, in place"""
    k = vals[::every].size
    vals[::every] = SA.CONTAMINATION[np.arange(k) % SA.CONTAMINATION.size]
    return vals


BIG_SHAPE = (2001, 2000)         # 4 002 000 px: the histogram path, no multiple of 65 536, rows of 8000 bytes


# exact/select -------------------------------------------------------------------------------------------------------------------
def _select_fixtures():
    out = []
    for pop in SA.populations():
        for k, form in enumerate(("row", "square")):
            claims = {}
            if pop.middle is not None:
                claims["median"] = (float(pop.middle[0]) + float(pop.middle[1])) / 2.0
            out.append(Fixture(f"select/{pop.name}/{form}", "exact/select", functools.partial(lambda p, i: p.planes()[i], pop, k), "exact",
                               claims=claims, meta=dict(pop=pop.name, count=pop.count)))
    return out


# exact/deviation ----------------------------------------------------------------------------------------------------------------
DEV_M = F32(1.5)
DEV_FAR = F32(3.5)               # |DEV_FAR - DEV_M| = 2: above every pair
DEV_PAIRS = ("L0", "BINADE", "L1", "L2")
DEV_COUNTS = ((1, "single"), (2, "even"), (3, "lower"), (3, "upper"), (255, "lower"), (255, "upper"), (256, "even"), (257, "lower"),
              (257, "upper"), (600_001, "lower"), (600_001, "upper"), (600_002, "even"))


def _exact_f32(x: float) -> bool:
    return float(F32(x)) == x


def deviation_candidates(pair: str, m: int, side: str):
    """-> (candidates, the deviations wanted at the middle rank(s)).  a copies of M - upper, b of M - lower, c of M, the rest at
    M + 2: the values' middle rank(s) sit inside the copies of M, and the deviations in rising order are c zeros, b times `lower`,
    a times `upper`, then 2s -- with c + b placed so that the middle rank(s) meet the pair's edge:
      even   ranks m/2 - 1 | m/2 are the last `lower` | the first `upper`
      lower  the middle rank of an odd count is the last `lower`;  upper: it is the first `upper`"""
    lower, upper, _ = SA.PAIRS[pair]
    M = DEV_M
    if m == 1:
        return np.array([M], F32), (F32(0.0),)
    if m == 2:   # one value on either side of M: the f64 mean of the two is M +- 2^-24 or closer, and rounds to M (ties to even)
        for lo_v, hi_v, want in ((float(M) - float(lower), float(M) + float(upper), (lower, upper)),
                                 (float(M) - float(upper), float(M) + float(lower), (lower, upper))):
            if _exact_f32(lo_v) and _exact_f32(hi_v) and F32((lo_v + hi_v) / 2.0) == M:
                return np.array([lo_v, hi_v], F32), want
        raise AssertionError(pair)
    v_low, v_up = M - lower, M - upper
    if m == 3:
        return np.array([v_low if side == "lower" else v_up, M, DEV_FAR], F32), ((lower,) if side == "lower" else (upper,))
    h = m // 2
    a = b = max(1, m // 8)
    c = h - b if (m % 2 == 0 or side == "upper") else h + 1 - b
    cands = np.concatenate([np.full(a, v_up, F32), np.full(b, v_low, F32), np.full(c, M, F32), np.full(m - a - b - c, DEV_FAR, F32)])
    return cands, ((lower, upper) if m % 2 == 0 else ((lower,) if side == "lower" else (upper,)))


def deviation_population(pair: str, m: int, side: str) -> SA.Population:
    cands, want = deviation_candidates(pair, m, side)
    np.random.default_rng(m + 7 * len(pair)).shuffle(cands)
    pop = SA.Population(f"{pair}-{m}-{side}", SA.interleave(cands, every=max(2, m // 500)), m, None,
                        dict(pair=pair, m=m, side=side, want=want, level=SA.PAIRS[pair][2]))
    return pop


def _deviation_fixtures():
    out = []
    for pair in DEV_PAIRS:
        for m, side in DEV_COUNTS:
            pop = deviation_population(pair, m, side)
            want = pop.meta["want"]
            mad = float((want[0] + want[1]) / F32(2.0)) if len(want) == 2 else float(want[0])
            claims = dict(mad=mad, median_f32=float(DEV_M))
            if m != 2:
                claims["median"] = float(DEV_M)
            for k, form in enumerate(("row", "square")):
                out.append(Fixture(f"deviation/{pop.name}/{form}", "exact/deviation", functools.partial(lambda p, i: p.planes()[i], pop, k),
                                   "exact", claims=claims, meta=dict(pop=pop, **pop.meta)))
    return out


# exact/limit --------------------------------------------------------------------------------------------------------------------
def _limit_plane(extra: int):
    rng = np.random.default_rng(4_000_000)
    vals = sprinkle(np.rint(rng.normal(1000.0, 30.0, EXACT_LIMIT)).astype(F32))
    if extra:
        vals = np.concatenate([vals, np.full(extra, 1000.0, F32)])
        return vals.reshape(1, -1)
    return vals.reshape(2000, 2000)


def _limit_fixtures():
    return [Fixture("limit/4000000", "exact/limit", functools.partial(_limit_plane, 0), "exact"),
            Fixture("limit/4000001", "exact/limit", functools.partial(_limit_plane, 1), "hist")]


# hist/edge ----------------------------------------------------------------------------------------------------------------------
EDGE_BINS = (64, 256, 32768, 65535)
EDGE_COUNTS = (3_999_998, 3_999_999)
EDGE_SUB = np.array([0, 1, 127])


def edge_values(b: int, count: int):
    """`count` values of bin b of the range [1, 2], spread over the sub-bins 0, 512 and 65 024 (s = 0, 1, 127)"""
    s = EDGE_SUB[np.arange(count) % 3]
    v = 1.0 + b / 65536.0 + s * 2.0 ** -23       # exact in f64, and a multiple of 2^-23 below 2: exact in f32
    return v.astype(F32)


def _edge_plane(bstar: int, which: str, total: int):
    half = (total + 1) // 2
    L = half if which == "last" else half - 1       # the cumulative count through bin b* - 1, the pixel at 1.0 included
    cands = np.concatenate([np.array([1.0], F32), edge_values(bstar - 1, L - 1), edge_values(bstar, total - L - 1), np.array([2.0], F32)])
    assert cands.size == total
    return fill(cands, *BIG_SHAPE, seed=bstar + total)


def _edge_fixtures():
    out = []
    for bstar in EDGE_BINS:
        for which in ("last", "first"):
            for total in EDGE_COUNTS:
                half = (total + 1) // 2
                if which == "last":     # the rank is the last element of bin b* - 1 (and of its last occupied sub-bin)
                    claims = {"median.bin": bstar - 1, "median.cum_is_half": True, "median.rank": half - 1, "median.count": half - 1,
                              "median.sub.cum_is_rank": True, "median.sub.bin": 127 * 512}
                else:                   # the rank is the first element of bin b* (and of its first sub-bin)
                    claims = {"median.bin": bstar, "median.cum_is_half": False, "median.rank": 1, "median.sub.bin": 0,
                              "median.sub.rank_in_bin": 1}
                out.append(Fixture(f"edge/{bstar}-{which}-{total}", "hist/edge", functools.partial(_edge_plane, bstar, which, total), "hist",
                                   claims=dict(claims, total=total, **{"median.not_found": False, "mad.not_found": False}),
                                   meta=dict(bstar=bstar, which=which)))
    return out


# hist/dev-edge ------------------------------------------------------------------------------------------------------------------
DEV_EDGE_K = (64, 256, 4096)
DEV_EDGE_CENTRE = (1_000_000, 1_000_001)
DEV_EDGE_OUTER = 1_200_000


def _dev_edge_plane(k: int, centre: int):
    """range [1, 2] (one pixel at either end); `centre` pixels alternate between M = 1.5 and M + 2^-23 (the even count starts with M,
    the odd one with M + 2^-23), DEV_EDGE_OUTER pixels each sit at M - D and M + D with D = k / 65536.  The coarse median is
    M + 2^-17 (half way into its bin), so the cluster at M - D deviates by D + 2^-17 (bin k) and the one at M + D by D - 2^-17
    (bin k - 1, where the MAD's rank lands)."""
    M, D = 1.5, k / 65536.0
    mid = np.where((np.arange(centre) + centre) % 2 == 0, M, M + 2.0 ** -23)
    cands = np.concatenate([[1.0, 2.0], mid, np.full(DEV_EDGE_OUTER, M - D), np.full(DEV_EDGE_OUTER, M + D)]).astype(F32)
    return fill(cands, *BIG_SHAPE, seed=k + centre)


def _dev_edge_fixtures():
    out = []
    for k in DEV_EDGE_K:
        for centre in DEV_EDGE_CENTRE:
            claims = {"median.bin": 32768, "dev.bin": k - 1, "dev.mod64": 63, "dev.count": DEV_EDGE_OUTER, "median.not_found": False,
                      "mad.not_found": False, "mad.region": (k - 2, k + 1), "below": centre, "total": centre + 2 * DEV_EDGE_OUTER + 2,
                      # the median's rank: the last element of sub-bin 0 (even) / the first element of sub-bin 512 (odd)
                      "median.sub.bin": 0 if centre % 2 == 0 else 512, "median.sub.cum_is_rank": centre % 2 == 0,
                      "median.sub.rank_in_bin": centre // 2 if centre % 2 == 0 else 1}
            out.append(Fixture(f"dev-edge/{k}-{centre}", "hist/dev-edge", functools.partial(_dev_edge_plane, k, centre), "hist", claims=claims,
                               meta=dict(k=k)))
    return out


# hist/known-range ---------------------------------------------------------------------------------------------------------------
def _sky_plane(rows, cols, seed=1000):
    rng = np.random.default_rng(seed)
    return sprinkle((1000.0 + 30.0 * rng.standard_normal(rows * cols)).astype(F32)).reshape(rows, cols)


def _known_fixtures():
    big = functools.partial(_sky_plane, *BIG_SHAPE)
    nf = {"median.not_found": True}
    return [
        # the median's bin is the saturated last one, [900 - width, 900): next to no pixel of it lies inside -> not found
        Fixture("known/100-900", "hist/known-range", big, "hist", (100.0, 900.0), dict(nf, **{"median.bin": 65535, "known": True})),
        Fixture("known/1-2", "hist/known-range", big, "hist", (1.0, 2.0), dict(nf, **{"median.bin": 65535, "mad.not_found": True, "known": True})),
        Fixture("known/2000-3000", "hist/known-range", big, "hist", (2000.0, 3000.0),
                dict(nf, **{"median.bin": 0, "mad.not_found": True, "known": True, "median.refine_total": 0})),
        # the reference's fall-backs (stats.rs:32-38)
        Fixture("known/nan-bound", "hist/known-range", big, "hist", (float("nan"), 1.0), {"known": False, "median.not_found": False}),
        Fixture("known/min-ge-max", "hist/known-range", big, "hist", (1500.0, 1500.0), {"known": False, "median.not_found": False}),
        Fixture("known/exact-path", "hist/known-range", functools.partial(_sky_plane, 300, 401), "exact", (1.0, 2.0)),
    ]


# hist/quantised -----------------------------------------------------------------------------------------------------------------
def _quantised_plane(kind: str):
    rows, cols = BIG_SHAPE
    n = rows * cols
    rng = np.random.default_rng(len(kind) + 60000)
    if kind == "60000":           # f32 spacing 2^-8 against a bin width of 1.5e-5
        vals = rng.uniform(59999.5, 60000.5, n).astype(F32)
    elif kind == "1e6":           # f32 spacing 2^-4 against a bin width of 9e-6
        vals = rng.uniform(1e6 - 0.3, 1e6 + 0.3, n).astype(F32)
    elif kind == "integers":
        vals = np.rint(rng.normal(1000.0, 30.0, n)).astype(F32)
    elif kind == "two-random":    # the two-valued plane of test_gpu_stats_stf.py
        vals = np.where(rng.random(n) < 0.5, F32(3.0), F32(5.0)).astype(F32)
    elif kind == "wide":          # 2e-7 against 3e38: every pixel in the first or the last bin
        vals = np.where(rng.random(n) < 0.5, F32(2e-7), F32(3e38)).astype(F32)
    else:
        raise KeyError(kind)
    return sprinkle(vals).reshape(rows, cols)


TWO_VALID = 3_999_000            # an even count of valid pixels in the two exact splits


def _two_split_plane(low: int):
    cands = np.concatenate([np.full(low, 3.0, F32), np.full(TWO_VALID - low, 5.0, F32)])
    return fill(cands, *BIG_SHAPE, seed=low)


def _quantised_fixtures():
    out = [Fixture(f"quantised/{k}", "hist/quantised", functools.partial(_quantised_plane, k), "hist")
           for k in ("60000", "1e6", "integers", "two-random", "wide")]
    half = TWO_VALID // 2
    # N // 2 low: cum(bin 0) == half, the median is the last `3.0`; N // 2 + 1 low: one to spare
    out.append(Fixture("quantised/two-half", "hist/quantised", functools.partial(_two_split_plane, half), "hist",
                       claims={"median.bin": 0, "median.cum_is_half": True, "median.rank": half, "total": TWO_VALID}))
    out.append(Fixture("quantised/two-half-plus-1", "hist/quantised", functools.partial(_two_split_plane, half + 1), "hist",
                       claims={"median.bin": 0, "median.cum_is_half": False, "median.rank": half, "total": TWO_VALID}))
    return out


# hist/shapes --------------------------------------------------------------------------------------------------------------------
def _last_tile_plane():
    rows, cols = 62, 65536
    out = np.resize(SA.CONTAMINATION, rows * cols).astype(F32)
    out[-65536:] = _sky_plane(1, 65536, seed=62).ravel()
    return out.reshape(rows, cols)


def _shape_fixtures():
    return [Fixture("shapes/1x4000001", "hist/shapes", functools.partial(_sky_plane, 1, 4_000_001, 11), "hist"),
            Fixture("shapes/2001x2000", "hist/shapes", functools.partial(_sky_plane, 2001, 2000, 12), "hist"),
            Fixture("shapes/62x65536", "hist/shapes", functools.partial(_sky_plane, 62, 65536, 13), "hist"),
            Fixture("shapes/last-65536", "hist/shapes", _last_tile_plane, "hist")]


FIXTURES = (_select_fixtures() + _deviation_fixtures() + _limit_fixtures() + _edge_fixtures() + _dev_edge_fixtures() + _known_fixtures()
            + _quantised_fixtures() + _shape_fixtures())
BY_NAME = {f.name: f for f in FIXTURES}
assert len(BY_NAME) == len(FIXTURES)
EXACT = [f for f in FIXTURES if f.path == "exact"]
HIST = [f for f in FIXTURES if f.path == "hist"]


def lookup(trace: dict, path: str):
    """trace["a"]["b"] for path "a.b" """
    cur = trace
    for k in path.split("."):
        cur = cur[k]
    return cur
