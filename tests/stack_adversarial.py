"""Adversarial per-pixel sample sets for the kappa-sigma stacks (pure numpy: no GPU, no oracle import).

The generated stack data of the other tests cannot tell one summation order from another (every f64 sum of those samples is exact)
and never puts a sample exactly on a clip threshold.  The families built here do both, on purpose:

  T  threshold ties with exact arithmetic: a one-sided sample exactly on `hi` (or `lo`) at iteration 0 (median / MAD sigma) or at
     iteration 1 (mean / sigma of an integer design with an exact mean and a perfect-square variance), at rank 1, 4, 5, 8, 9, 16
     and 17 from its end, for several centres and kappas; each with a twin whose boundary sample sits one f32 ulp outside.
  W  inexact sums: mixed-sign samples whose magnitudes span more than 2^30 (the f64 sum depends on the order), means near 0 by
     cancellation included.
  M  the fast engine's moment switch: median at 1023, 1024, 1025 and 2^20 times the iteration-0 sigma.
  E  the n = 8 edge pixels of tests/test_gpu_stack.py at any n: overflowing deviations, subnormals, -0.0, zero majorities, MAD = 0.
  B  ties of the batch stack (orc_batch.c: z = (v - median) / sigma, kept when -sl < z < sh): z == kappa exactly, with twins one
     ulp inside and one ulp outside.

Every tie is checked here against `clip_reference` (a restatement of the oracle's sigma_clip_combine) and `batch_reference`
(of its sigma_clipped_mean_stack pixel) before it is emitted; tests/test_stack_adversarial_cpu.py proves against the oracle itself
that each fixture still does what it claims.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
MAD_TO_SIGMA = 1.4826

# both sides of every frame-count class edge of the stack kernels
N_LIST = (3, 8, 9, 16, 32, 33, 64, 65, 128, 129, 192, 256, 257, 384, 512, 513, 1024, 1025, 2048, 4096, 4100)
RANKS = (1, 4, 5, 8, 9, 16, 17)


@dataclass
class Pixel:
    family: str            # "T", "W", "M", "E" or "B"
    name: str
    values: np.ndarray     # float32, n samples in frame order
    twin: "Pixel | None" = None      # T: the boundary sample one ulp outside; B: one ulp inside
    twin_out: "Pixel | None" = None  # B only: one ulp outside
    meta: dict = field(default_factory=dict)


@dataclass
class FixtureSet:
    """pixels that share one (sigma_low, sigma_high, max_iter)"""
    family: str
    sl: float
    sh: float
    it: int
    pixels: list
    raw: "bool | None" = None   # T, W, M: every pixel's iteration-0 median is within 1024 sigma0 (True) or beyond it (False)

    def all_pixels(self):
        out = []
        for p in self.pixels:
            out.append(p)
            for t in (p.twin, p.twin_out):
                if t is not None:
                    out.append(t)
        return out


# ---- restatements (f32 / f64 exactly as oracle/orc_combine.c and oracle/orc_batch.c) -------------------------------------------
def clip_reference(values, sl, sh, max_iter):
    """sigma_clip_combine_impl in ascending order: (value, rejected, [(center, sigma, lo, hi, survivors before the clip)])."""
    v = np.sort(np.asarray(values, F32)[np.isfinite(values)])
    sl, sh = F32(sl), F32(sh)
    trace = []
    if v.size == 0:
        return F32(0.0), 0, trace
    if v.size == 1:
        return v[0], 0, trace
    rejected = 0
    last_center = F32(np.nan)
    for it in range(max_iter):
        if v.size < 2:
            break
        if it == 0:
            med = v[v.size // 2]
            mad = np.sort(np.abs(v - med))[v.size // 2]
            center, sigma = med, F32(max(float(mad) * MAD_TO_SIGMA, 1e-10))
        else:
            s = 0.0
            for x in v:
                s += float(x)
            mean = s / v.size
            q = 0.0
            for x in v:
                d = float(x) - mean
                q += d * d
            center = F32(mean)
            sigma = F32(max(math.sqrt(q / max(v.size - 1.0, 1.0)), 1e-10))
        last_center = center
        lo, hi = -sl * sigma, sh * sigma
        dev = v - center
        keep = (dev >= lo) & (dev <= hi)
        trace.append((center, sigma, lo, hi, v.copy()))
        removed = int(v.size - keep.sum())
        rejected += removed
        v = v[keep]
        if removed == 0:
            break
    if v.size == 0:
        return (last_center if np.isfinite(last_center) else F32(0.0)), rejected, trace
    s = 0.0
    for x in v:
        s += float(x)
    return F32(s / v.size), rejected, trace


def raw_side(values):
    """the fast engine's moment switch for one pixel: |median| <= 1024 sigma0 (iteration 0's median and MAD sigma, f32 as the
    kernels compute them); None with fewer than two finite samples.  The kernels decide per wave (every lane must agree for the raw
    moments), so a FixtureSet holds pixels of one side only: every wave of a call then runs the tail the set is built for."""
    v = np.sort(np.asarray(values, F32)[np.isfinite(values)])
    if v.size < 2:
        return None
    med = v[v.size // 2]
    mad = np.sort(np.abs(v - med))[v.size // 2]
    sig0 = F32(max(float(mad) * MAD_TO_SIGMA, 1e-10))
    return bool(abs(med) <= F32(1024.0) * sig0)


def _split_sides(sets):
    """one FixtureSet per (settings, moment side)"""
    out = []
    for fs in sets:
        for side in (True, False):
            px = [p for p in fs.pixels if raw_side(p.values) == side]
            if px:
                out.append(FixtureSet(fs.family, fs.sl, fs.sh, fs.it, px, side))
    return out


def batch_reference(values, sl, sh, max_iter):
    """scms_pixel: (value, rejected frame indices, [(median, sigma)])"""
    vals = np.asarray(values, F32).copy()
    owner = np.arange(vals.size)
    sl, sh = F32(sl), F32(sh)
    rej, trace = [], []
    for _ in range(max_iter):
        if vals.size < 3:
            break
        med = np.sort(vals)[vals.size // 2]
        sigma = F32(float(np.sort(np.abs(vals - med))[vals.size // 2]) * MAD_TO_SIGMA)
        if sigma < F32(1e-10):
            break
        trace.append((med, sigma))
        with np.errstate(invalid="ignore", over="ignore"):
            z = (vals - med) / sigma
        keep = (z > -sl) & (z < sh)
        rej += owner[~keep].tolist()
        if keep.all():
            break
        vals, owner = vals[keep], owner[keep]
    s = F32(0.0)
    for x in vals:
        s = F32(s + x)
    return (F32(s / F32(vals.size)) if vals.size else F32(0.0)), rej, trace


def _ulp_out(x, outward_positive):
    return np.nextafter(F32(x), F32(np.inf) if outward_positive else F32(-np.inf)).astype(F32)


def _twin(values, idx, outward_positive):
    t = np.array(values, F32)
    t[idx] = _ulp_out(t[idx], outward_positive)
    return t


def _shuffle(vals, seed):
    """frame order: a fixed permutation (the kernels sort; the oracle's selection must not depend on arrival order)"""
    vals = np.asarray(vals, F32)
    perm = np.random.default_rng(seed).permutation(vals.size)
    return vals[perm], int(np.argsort(perm)[0])  # (permuted, new position of the old index 0)


# ---- T: ties at iteration >= 1 (integer designs: exact mean, variance sigma^2) ---------------------------------------------------
def _tune_zero_pairs(zeros, need, cap):
    """turn pairs of zeros into (-d, +d) so that the sum of squares grows by exactly `need` (2 d^2 per pair); None if impossible"""
    if need < 0 or need % 2:
        return None
    half = need // 2
    out = []
    while half > 0:
        d = min(int(math.isqrt(half)), cap)
        out += [-d, d]
        half -= d * d
        if len(out) > zeros:
            return None
    return out + [0] * (zeros - len(out))


def iter1_deviations(m, sigma, kh, kl, rank):
    """m integer deviations with sum 0 and sum of squares sigma^2 (m - 1): one sample at kh*sigma (the tie), rank - 1 beyond it at
    kh*sigma + sigma/4, the rest strictly inside (-kl*sigma, kh*sigma) and mostly at +-sigma (so that the iteration-0 MAD is
    sigma and its wider window keeps every one of them).  Returns (deviations, index of the tie) or None."""
    t = kh * sigma
    beyond = t + sigma // 4
    if t != int(t) or beyond >= 1.45 * kh * sigma:
        return None
    t, beyond = int(t), int(beyond)
    A = t + (rank - 1) * beyond
    B = t * t + (rank - 1) * beyond * beyond
    c = m - rank
    for Z in range(1, c + 1):
        nz = c - Z                        # bulk at +-sigma
        # P - N = round(-A / sigma), P + N = nz
        diff = -int(round(A / sigma))
        if (nz + diff) % 2:
            diff += 1 if diff < 0 else -1
        P, N = (nz + diff) // 2, (nz - diff) // 2
        if P < 0 or N < 0:
            continue
        R = -A - sigma * (P - N)          # residual, carried by one of the zeros
        if abs(R) >= min(kl, kh) * sigma or Z < 1:
            continue
        S = B + sigma * sigma * nz + R * R
        tuned = _tune_zero_pairs(Z - 1, sigma * sigma * (m - 1) - S, sigma - 1)
        if tuned is None:
            continue
        devs = [t] + [beyond] * (rank - 1) + [sigma] * P + [-sigma] * N + [R] + tuned
        if 2 * (P + N) <= m + 2:          # MAD must be sigma: most samples at +-sigma
            continue
        d = np.array(devs, np.int64)
        assert d.sum() == 0 and (d * d).sum() == sigma * sigma * (m - 1)
        return d, 0
    return None


def _ties_iter1(n, mu_kind, kh, kl, rank, side, sigma=64):
    """a T pixel whose boundary sample lies exactly on hi (side +1) or lo (side -1) at iteration 1 (kh: the kappa of the tie's
    side, kl: of the other one)"""
    outl = 1 if n < 40 else 2
    m = n - outl
    if m < 10 or rank > m // 6 + 1:
        return None
    got = iter1_deviations(m, sigma, kh, kl, rank)
    if got is None:
        return None
    d, ti = got
    d = d * side
    sig0 = F32(sigma * MAD_TO_SIGMA)       # (the MAD is sigma: checked below through the restatement)
    mu = {"neg": -777.0 * sigma, "zero": 0.0, "pos": 300.0 * sigma, "c1023": float(F32(1023) * sig0),
          "c1024": float(F32(1024) * sig0), "c1025": float(F32(1025) * sig0), "far": float(F32(5000) * sig0),
          "c2p20": float(F32(2.0 ** 20) * sig0)}[mu_kind]
    vals = (F32(mu) + d.astype(F32)).astype(F32)
    if not np.array_equal(vals.astype(np.float64) - np.float64(F32(mu)), d):
        return None                         # the grid of mu is coarser than the design
    big = F32(abs(mu) + 4096.0 * sigma)
    outs = [big if k % 2 == 0 else -big for k in range(outl)]
    allv = np.concatenate([vals, np.array(outs, F32)])
    return allv, ti, F32(mu)


def _check_tie(vals, idx, sl, sh, it, iteration, side):
    """the restatement puts vals[idx] exactly on the threshold of `iteration`, and the twin one ulp outside changes the count and the
    value"""
    _, rej, trace = clip_reference(vals, sl, sh, it)
    if len(trace) <= iteration:
        return False
    center, sigma, lo, hi, before = trace[iteration]
    x = vals[idx]
    if x not in before or F32(x - center) != (hi if side > 0 else lo):
        return False
    others = np.delete(before, np.where(before == x)[0][:1]) - center
    if side > 0 and np.any(others == hi) or side < 0 and np.any(others == lo):
        return False                        # one-sided: the tie is the only sample on its threshold
    val2, rej2, _ = clip_reference(_twin(vals, idx, side > 0), sl, sh, it)
    return rej2 != rej and val2 != clip_reference(vals, sl, sh, it)[0]


# ---- T: ties at iteration 0 (median / MAD sigma on a grid where kappa * sigma is exact) -------------------------------------------
def _mad_grid(kappas, g):
    """MAD values m0 = k 2^-g in [4, 8) whose sigma0 = f32(m0 * 1.4826) and kappa * sigma0 are multiples of 2^-(g - 1)"""
    m0 = (np.arange(4 << g, 8 << g, dtype=np.float64) / (1 << g)).astype(F32)
    s0 = np.maximum(m0.astype(np.float64) * MAD_TO_SIGMA, 1e-10).astype(F32)
    ok = np.ones(m0.size, bool)
    for k in kappas:
        h = (F32(k) * s0).astype(np.float64) * (1 << (g - 1))
        ok &= h == np.round(h)
    return m0[ok], s0[ok]


_GRID = {}


def _grid_for(kappas, g=12):
    key = (tuple(sorted(set(kappas))), g)
    if key not in _GRID:
        _GRID[key] = _mad_grid(key[0], g)
    return _GRID[key]


def _ties_iter0(n, mu, kh, kl, rank, side, g=12):
    """a T (or B) pixel whose boundary sample lies exactly on the iteration-0 threshold about the median (kh: the kappa of the tie's
    side, kl: of the other one).  g: the MAD grid 2^-g; a centre beyond 1024 sigma0 (f32 ulp 2^-9 at 2^14) needs g = 10."""
    m0s, s0s = _grid_for((kh, kl), g)
    if m0s.size == 0:
        return None
    m0, s0 = F32(m0s[0]), F32(s0s[0])
    t = F32(F32(kh) * s0)                        # |tie deviation|
    r = rank - 1
    # n = 1 (tie) + r (beyond) + rank (compensators at -m0) + Z (zeros) + 2P (+-m0): the median is 0 and the MAD m0 when
    # Z <= n // 2 = P + rank + Z // 2
    rest = n - 1 - r - rank
    Z = max(1, rest // 5)
    if (rest - Z) % 2:
        Z += 1
    P = (rest - Z) // 2
    if P < 0 or P + rank < Z - Z // 2:
        return None
    d = [t] + [F32(2) * t + m0] * r + [-m0] * rank + [F32(0)] * Z + [m0] * P + [-m0] * P
    d = np.array(d, F32) * F32(side)
    vals = (F32(mu) + d).astype(F32)
    if not np.array_equal(vals - F32(mu), d):
        return None
    return vals, 0


# ---- the families ----------------------------------------------------------------------------------------------------------------
T_KAPPAS = ((2.0, 2.0), (2.5, 1.5), (1.5, 3.0))      # (sigma_high, sigma_low) of the tie's side first
# centres of the ties: "far" lies beyond 1024 sigma0 (the centred moments), the others within it (the raw moments); c1024 exactly on it
IT0_MU = (("neg", -1500.0), ("zero", 0.0), ("pos", 1000.0), ("far", 2.0 ** 14))
IT1_MU = ("neg", "zero", "pos", "c1024", "far")


def family_T(n):
    """-> FixtureSets (max_iter 1: the iteration-0 ties; 2: the iteration-1 ties, decided at the last iteration; 5: rank-1 ties)"""
    sets = {}
    for kh, kl in T_KAPPAS:
        for side in (+1, -1):
            sl, sh = (kl, kh) if side > 0 else (kh, kl)
            # iteration 0
            for mu_kind, mu in IT0_MU:
                for rank in RANKS:
                    got = _ties_iter0(n, mu, kh, kl, rank, side, g=(10 if mu_kind == "far" else 12))
                    if got is None:
                        continue
                    vals, idx = got
                    for it in ((1, 5) if rank == 1 else (1,)):
                        if not _check_tie(vals, idx, sl, sh, it, 0, side):
                            continue
                        p, j = _shuffle(vals, 1000 * n + rank)
                        px = Pixel("T", f"it0 {mu_kind} r{rank} {'hi' if side > 0 else 'lo'} k{kh}/{kl} i{it}", p,
                                   meta=dict(iteration=0, rank=rank, side=side, idx=j, mu_kind=mu_kind))
                        px.twin = Pixel("T", px.name + " +ulp", _twin(p, j, side > 0), meta=dict(twin_of=px.name))
                        sets.setdefault((sl, sh, it), []).append(px)
            # iteration 1
            for mu_kind in IT1_MU:
                for rank in RANKS:
                    got = _ties_iter1(n, mu_kind, kh, kl, rank, side)
                    if got is None:
                        continue
                    vals, idx, _ = got
                    for it in ((2, 5) if rank == 1 else (2,)):
                        if not _check_tie(vals, idx, sl, sh, it, 1, side):
                            continue
                        p, j = _shuffle(vals, 2000 * n + rank)
                        px = Pixel("T", f"it1 {mu_kind} r{rank} {'hi' if side > 0 else 'lo'} k{kh}/{kl} i{it}", p,
                                   meta=dict(iteration=1, rank=rank, side=side, idx=j, mu_kind=mu_kind))
                        px.twin = Pixel("T", px.name + " +ulp", _twin(p, j, side > 0), meta=dict(twin_of=px.name))
                        sets.setdefault((sl, sh, it), []).append(px)
    return _split_sides([FixtureSet("T", sl, sh, it, pxs) for (sl, sh, it), pxs in sorted(sets.items())])


def _wide_values(rng, n, centre, spread, cancel):
    """mixed-sign samples with full mantissas whose magnitudes span more than 2^30; `cancel`: the large ones come in pairs of opposite
    sign a few f32 ulp apart, so that the mean stays near the bulk's (near 0 for bias-subtracted frames)"""
    v = centre + spread * rng.standard_normal(n)
    k = max(2, n // 8) // 2 * 2
    k = min(k, (n - 1) // 2 * 2) if n >= 3 else 0
    pick = rng.choice(n, size=min(n, 2 * k if n > 2 else n), replace=False)
    big = rng.uniform(1, 2, k) * 2.0 ** rng.integers(18, 26, k)
    if cancel:
        big[1::2] = -(big[0::2] + rng.integers(1, 9, k // 2) * 2.0 ** (np.floor(np.log2(big[0::2])) - 23))
    else:
        big *= np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    tiny = rng.uniform(1, 2, max(k, 1)) * 2.0 ** rng.integers(-16, -8, max(k, 1)) * rng.choice([-1, 1], max(k, 1))
    v[pick[:k]] = big
    v[pick[k:k + tiny.size][: max(0, pick.size - k)]] = tiny[: max(0, pick.size - k)]
    return v.astype(F32)


def ascending_sum(v):
    s = 0.0
    for x in np.sort(np.asarray(v, F32)).astype(np.float64):
        s += x
    return s


def order_sums(v):
    """(ascending, descending, pairwise) f64 sums of the finite samples"""
    f = np.sort(np.asarray(v, F32)[np.isfinite(v)]).astype(np.float64)
    desc = 0.0
    for x in f[::-1]:
        desc += x
    while f.size > 1:                       # pairwise tree (the >512-frame engines add their survivors as a tree)
        if f.size % 2:
            f = np.append(f, 0.0)
        f = f[0::2] + f[1::2]
    return ascending_sum(v), desc, float(f[0]) if f.size else 0.0


def family_W(n):
    rng = np.random.default_rng(700 + n)
    pixels = []
    specs = [("near0", 0.0, 20.0), ("bias", 0.03125, 6.0), ("neg", -300.0, 40.0), ("pos", 1000.0, 50.0)]
    for name, centre, spread in specs:
        for rep in range(3):
            for attempt in range(500):
                v = _wide_values(rng, n, centre, spread, name in ("near0", "bias") and n > 3)
                a, d, p = order_sums(v)
                if a != d or a != p:
                    break
            mag = np.abs(v[(v != 0) & np.isfinite(v)])
            pixels.append(Pixel("W", f"{name}#{rep}", v, meta=dict(span=float(mag.max() / mag.min()))))
    return _split_sides([FixtureSet("W", sl, sh, it, pixels)
                         for sl, sh, it in ((3.0, 3.0, 0), (1e9, 1e9, 5), (3.0, 3.0, 5), (2.0, 2.5, 5))])


def _moment_pixel(rng, n, c, m0):
    """median exactly mu = f32(c * sigma0) with sigma0 = f32(m0 * 1.4826), MAD m0, the other samples with full mantissas"""
    s0 = F32(max(float(m0) * MAD_TO_SIGMA, 1e-10))
    mu = F32(F32(c) * s0)
    half = n // 2
    mag = np.empty(n)
    mag[0] = 0.0                                          # the median sample
    mag[1:half] = rng.uniform(0.05, 0.9, max(half - 1, 0)) * float(m0)
    mag[half] = float(m0)                                 # the MAD sample (positive)
    mag[half + 1:] = rng.uniform(1.1, 2.5, n - half - 1) * float(m0)
    sign = np.ones(n)
    others = np.array([i for i in range(1, n) if i != half])
    sign[rng.choice(others, size=half, replace=False)] = -1.0   # exactly n // 2 samples below the median
    v = (np.float64(mu) + sign * mag).astype(F32)
    v[0], v[half] = mu, F32(mu + m0)
    return v, mu, s0


def family_M(n):
    rng = np.random.default_rng(900 + n)
    pixels = []
    for c in (1023.0, 1024.0, 1025.0, 2.0 ** 20):
        for m0 in (F32(1.0), F32(0.75)):
            if n < 3:
                continue
            v, mu, s0 = _moment_pixel(rng, n, c, m0)
            _, _, tr = clip_reference(v, 3.0, 3.0, 1)
            if not tr:
                continue
            med, sig = tr[0][0], tr[0][1]
            pixels.append(Pixel("M", f"med {c:g} sigma m0={m0:g}", v,
                                meta=dict(raw=bool(abs(med) <= F32(1024.0) * sig), c=c, median=float(med), sigma0=float(sig))))
    # an exact-arithmetic tie on top of the switch
    for kind in ("c1023", "c1024", "c1025", "c2p20"):
        got = _ties_iter1(n, kind, 2.0, 2.0, 1, +1, sigma=8 if kind == "c2p20" else 64)
        if got is not None and _check_tie(got[0], got[1], 2.0, 2.0, 5, 1, +1):
            _, _, tr = clip_reference(got[0], 2.0, 2.0, 1)
            med, sig = tr[0][0], tr[0][1]
            pixels.append(Pixel("M", f"tie {kind}", got[0],
                                meta=dict(raw=bool(abs(med) <= F32(1024.0) * sig), c=kind, median=float(med), sigma0=float(sig))))
    return _split_sides([FixtureSet("M", sl, sh, it, pixels)
                         for sl, sh, it in ((2.0, 2.0, 5), (3.0, 3.0, 5), (1e9, 1e9, 5), (3.0, 3.0, 0))])


def _tile(pattern, n, fill):
    """the 8-sample edge pattern spread over n frames (copies of it, the remainder filled with `fill`)"""
    pattern = np.asarray(pattern, F32)
    reps = max(1, n // pattern.size)
    v = np.full(n, fill, F32)
    t = np.tile(pattern, reps)[:n]
    v[:t.size] = t
    return v


def family_E(n):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    px = []

    def add(name, v):
        px.append(Pixel("E", name, np.asarray(v, F32)))

    add("all nan", np.full(n, nan))
    v = np.full(n, nan); v[n // 2] = 42.5; add("one finite", v)
    v = np.full(n, inf); v[0] = -7.0; v[-1] = 9.0; add("two finite", v)
    add("constant", np.full(n, 5.0))
    v = np.full(n, 5.0, F32); v[n // 3] = np.nextafter(F32(5.0), F32(10)); add("constant + 1 ulp", v)
    v = np.full(n, 0.0, F32); v[n - 1] = np.nextafter(F32(0.0), F32(1)); add("zeros + 1 subnormal ulp", v)
    add("ties about the median", np.where(np.arange(n) % 2 == 0, 1.0, 2.0))
    v = (np.arange(n) % 6 + 1).astype(F32)
    if n >= 3:
        v[0], v[1] = -3e38, 3e38
    add("deviation overflows", v)
    if n < 8:
        # (three samples: the MAD is an overflowing deviation, sigma is inf and nothing is clipped: -3e38 + 3e38 + 3 is not exact in
        # f64.  The oracle's ascending chain gives 0, the default engine's moments about the median 3 (the exact mean is 1): outside
        # any relative contract, so on the default engine only the rejected count is held -- see DESIGN 4.1)
        px[-1].meta["inexact"] = True
        px[-1].meta["sigma_inf"] = True
    v = -(np.arange(n) % 7 + 1).astype(F32)
    v[-1] = -800.0; add("negatives + outlier", v)
    add("subnormals", _tile([1e-40, 2e-40, 3e-40, 1e-39, 0, -0.0, 1e-45, 5e-41], n, 0.0))
    add("-0.0 majority", _tile([-0.0, -0.0, -0.0, -0.0, -0.0, 1e-45, -1e-45, -0.0], n, -0.0))
    v = np.zeros(n, F32); v[-2:] = [1000.0, 1001.0]; add("zero majority", v)
    add("many outliers", _tile([100, 101, 99, 100, 5000, 6000, 7000, 100.5], n, 100.0))
    v = (np.arange(n) % 4 + 1).astype(F32); v[: n // 2] = 3e38; add("huge majority", v)
    if n % 2 == 0:
        # (half of the samples at 3e38: the MAD is 3e38, sigma inf, nothing is clipped, and 3e38 + small integers is not exact in
        # f64 -- held to the W assertions.  Odd n: the 3e38 samples are the minority and are clipped.)
        px[-1].meta["inexact"] = True
    v = np.full(n, -3.0, F32); v[::2] = inf; v[1] = -inf; add("mixed infinities", v)
    add("ramp", np.arange(n, dtype=F32))
    sets = [FixtureSet("E", sl, sh, it, px) for sl, sh, it in ((3.0, 3.0, 5), (1.0, 1.0, 5), (3.0, 3.0, 1))]
    # max_iter 0: the plain mean of every finite sample, without the iteration-0 walk (the pixels whose finite samples sum exactly)
    sets.append(FixtureSet("E", 3.0, 3.0, 0, [p for p in px if p.name not in ("deviation overflows", "huge majority")]))
    # ceil(n / 2) samples at -3e38, +3e38 alternately, small ones below them: the MAD overflows (sigma inf), nothing is clipped, and
    # the kept samples cancel.  Not exact in f64: only AB_STACK_EXACT=1 reproduces the oracle's ascending chain (the moment forms and
    # the workgroup-per-pixel kernel give other values), every route is held to the rejected count.
    v = (np.arange(n) % 5 + 1).astype(F32)
    h = n - n // 2
    v[:h] = np.where(np.arange(h) % 2 == 0, F32(-3e38), F32(3e38))
    over = Pixel("E", "cancelling overflow", v, meta=dict(inexact=True, sigma_inf=True))
    for fs in sets:
        fs.pixels.append(over)
    return sets


B_KAPPAS = ((3.0, 2.5), (2.0, 2.0), (1.5, 3.0))       # (sigma_high, sigma_low)


def family_B(n):
    """batch-stack ties: v - median == kappa * sigma exactly (rejected: strict comparisons), twins one ulp inside and outside"""
    sets = {}
    for kh, kl in B_KAPPAS:
        for side in (+1, -1):
            sl, sh = (kl, kh) if side > 0 else (kh, kl)
            for mu in (-1500.0, 0.0, 1000.0):
                for rank in (1, 5, 9, 17):
                    got = _ties_iter0(n, mu, kh, kl, rank, side)
                    if got is None:
                        continue
                    vals, idx = got
                    p, j = _shuffle(vals, 3000 * n + rank)
                    it = 1 if rank > 1 else 3
                    _, rej, tr = batch_reference(p, sl, sh, it)
                    if not tr:
                        continue
                    med, sigma = tr[0]
                    z = F32(p[j] - med) / sigma
                    if z != F32(kh) * side:
                        continue
                    inside = _twin(p, j, side < 0)
                    _, rej_in, _ = batch_reference(inside, sl, sh, it)
                    if sorted(rej_in) == sorted(rej):
                        continue
                    px = Pixel("B", f"{mu:g} r{rank} {'hi' if side > 0 else 'lo'} k{kh}/{kl}", p,
                               meta=dict(rank=rank, side=side, idx=j))
                    px.twin = Pixel("B", px.name + " -ulp", inside, meta=dict(twin_of=px.name, inside=True))
                    px.twin_out = Pixel("B", px.name + " +ulp", _twin(p, j, side > 0), meta=dict(twin_of=px.name))
                    sets.setdefault((sl, sh, it), []).append(px)
    return [FixtureSet("B", sl, sh, it, pxs) for (sl, sh, it), pxs in sorted(sets.items())]


FAMILIES = {"T": family_T, "W": family_W, "M": family_M, "E": family_E, "B": family_B}
_CACHE = {}


def fixture_sets(family, n):
    key = (family, n)
    if key not in _CACHE:
        _CACHE[key] = FAMILIES[family](n)
    return _CACHE[key]


# ---- packing: one fixture pixel per plane position -------------------------------------------------------------------------------
def pack(pixels, layout="mult16", rows=None):
    """-> (frames: n float32 planes, npix): pixel k of `pixels` at flat position k.  layout "mult16": a pixel count that is a
    multiple of 16 (16 columns per row, the tail padded with copies of the first pixels); "odd": one row of an odd pixel count
    that is not a multiple of 16; "rows": `rows` rows (for row bands), the pixels repeated to fill them."""
    vals = [p.values for p in pixels]
    n = vals[0].size
    assert all(v.size == n for v in vals)
    P = len(vals)
    if layout == "mult16":
        total = max(16, -(-P // 16) * 16)
        shape = (total // 16, 16)
    elif layout == "odd":
        total = P + (1 if P % 2 == 0 else 0)
        if total % 16 == 0:
            total += 1
        shape = (1, total)
    elif layout == "rows":
        cols = max(P, 3) if P % 16 else P + 1
        total = rows * cols
        shape = (rows, cols)
    else:
        raise ValueError(layout)
    stack = np.empty((n, total), F32)
    for k in range(total):
        stack[:, k] = vals[k % P]
    return [stack[i].reshape(shape).copy() for i in range(n)], P
