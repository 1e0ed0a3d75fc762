"""Named, seeded, read-only cases for drizzle (csrc/drizzle.hip): sample lists designed value by value for the finalize, and frame
geometries designed offset by offset for the gather.  Pure numpy; nothing here knows the library.  The judge is
tests/drizzle_restatement.py; tests/test_drizzle_adversarial_cpu.py holds every case to what it claims (the census below) and
tests/test_gpu_drizzle_adversarial.py runs them on the device.

How a pixel's list is designed.  Two geometries give the builder every sample of a pixel, in push order:
  "one"   scale 2, pixfrac 0.5, every offset zero, Square: output (oy, ox) receives input ((oy + 1) // 2, (ox + 1) // 2) of every
          frame, in frame order (weight 0.25).  A list is written down the frame axis of one input pixel; NaN = no sample.
  "two"   scale 1, pixfrac 1, every frame reported at dx = 0.5, dy = 0, Square: output (oy, ox) receives input rows oy, oy + 1 of
          column ox + 1 of every frame (weight 0.5 each): two pushes per frame, lists of up to the cap of 2 n.  The designed pixels
          are the even output rows; the odd rows between them mix two designed lists and are compared all the same.
A list shorter than the geometry's capacity sits in a seeded choice of the slots, the others NaN.

Families (A: finalize; every family at n = 3, 4, 5, 8, 9, 16, 17, 32 -- the first and the last cap of each network width -- and at
33 and 40 frames, where the column lies in global memory and a heap sort orders it):
  A1d  exact threshold ties, deterministic: median 0, sl = sh = 2, [-1, -a.., 0, a.., X] with X = f32(2 * f32(0.5 * 1.4826)), its two
       f32 neighbours, the mirror images, all of them times 2^k, padded with +-0.5 to every length
  A1g  the same with a non-zero dyadic median and non-dyadic sl / sh found by an ulp search: f32(sh * sigma) == f32(v - med)
  A2   MAD == 0: more than half the samples equal; the others 1 ulp away (rejected), or, around 0, inside / on / outside the 1e-10
       floor times 3 (f32(3 * f32(1e-10)) itself is kept, its successor rejected); all equal
  A3   duplicates on both sides of the median: the two runs of the MAD merge tie again and again.  (A tie's two candidates are
       EQUAL, so the side taken cannot change the MAD; what these lists pin is the merge's handling of an exhausted run, the f32
       average of two samples as median and as MAD, and every sort on long runs of equal keys.  Two list kinds use up one run
       before the merge is done -- reachable only through a median that the f32 average rounds onto one of its two samples.)
  A4z / A4d  subnormal samples (multiples of 2^-149, and around 2^-126) under sl = sh = 0 (only dev == 0 survives) and under 3 / 3
  A5z / A5d / A5o  samples near FLT_MAX under sl = sh = 0, 3, 1: the two middle samples sum past it (median +inf, MAD inf,
       -0 * inf = NaN: nothing survives under sl = 0, everything under 3 / 3), and +-x pairs whose median is 0 and whose MAD
       overflows as an f32 average (inf: everything stays) where an f64 average would not (under 1 / 1 the outer pair would go)
  A6   (n = 32, 33 only) 64-sample lists under (1.0, 1.0) with sigma_iterations 1 .. 12, 20, 1000, 2^40: up to 16 acting rounds
  A7   every count 0 .. cap in one call, the full network with no +inf pad included
  A8   ("one") single samples of -0.0 and +0.0, and short lists of zeros of either sign
  cap  one case with four pushes per frame (scale 1, zero offsets): the cap drops the later frames

Families (B: gather; Square, Gaussian and Lanczos3; every value a multiple of 2^-8, so every mean is exact):
  B1a  scales 1, 2, 4 x pixfrac 0.5, 1 with offsets that are multiples of 1/8: c -+ half are integers, floor / ceil tie
  B1b  scales 1.5, 2.5, 3 with offsets k / scale and (k +- half) / scale, each also 1 and 2 ulp to either side
  B2   frames of 1 x 1, 1 x 5, 5 x 1, 2 x 2 at scale 1 (an output pixel that is both borders), 4 and 33 frames, offsets inside the
       field, just off it and far off it
  B3   three ordinary frames and three at |offset| = 1e3, 1e6, 2^31 -+ 0.5, 1e9, 1e12, 1e18, 1e300, both signs, both axes
  B4   (Gaussian) frames whose nearest pixel centre lies 7.44 sigma -+ 0.01 px beyond each border pixel's centre, and one corner
       (the weight crosses 1e-12 at 7.4338 sigma; the kernel rounds its candidate range outward to whole input pixels, so these
       frames tell a reach that is short by an input pixel or more, not 7.40 from 7.44)
  B5   outputs of exactly 4 x 64 and 8 x 128 pixels: no partly filled workgroup
Every offset of B is dyadic, k / scale or a few ulp from it, or 0.004 px and more from where a Gaussian weight crosses 1e-12: no
candidate weight of any case lies within 1e-6 relative of the cut (threshold-pixel share exactly 0.0; the CPU test asserts it)."""
from dataclasses import dataclass

import numpy as np

import drizzle_restatement as R

F = np.float32
LDS_COUNTS = [3, 4, 5, 8, 9, 16, 17, 32]
LONG_COUNTS = [33, 40]
FRAME_COUNTS = LDS_COUNTS + LONG_COUNTS
ROWS, COLS = 8, 40
KERNELS = [R.SQUARE, R.GAUSSIAN, R.LANCZOS3]
KNAME = {R.SQUARE: "square", R.GAUSSIAN: "gaussian", R.LANCZOS3: "lanczos3"}
U = F(2.0 ** -149)
FMAX = np.finfo(F).max
A6_ITERS = list(range(1, 13)) + [20, 1000, 2 ** 40]


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    frames: tuple
    offsets: tuple
    scale: float
    pixfrac: float
    kernel: int = R.SQUARE
    sl: float = 3.0
    sh: float = 3.0
    iters: int = 5
    designed: tuple = ()    # (oy, ox, the list in push order as a tuple of np.float32, tag)
    far: tuple = ()         # B3: indices of the far frames
    note: tuple = ()        # family-specific facts for the CPU test

    def args(self):
        return list(self.frames), list(self.offsets), self.scale, self.pixfrac, self.kernel, self.sl, self.sh, self.iters


_wanted = {}


def wanted(case):
    """the restatement's result for the case (with the lists), computed once and never modified"""
    if case.name not in _wanted:
        _wanted[case.name] = R.drizzle(*case.args(), keep_lists=True)
    return _wanted[case.name]


def _ro(a):
    a = np.ascontiguousarray(a, dtype=F)
    a.flags.writeable = False
    return a


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


# ---- the clip, round by round --------------------------------------------------------------------------------------------------------
def _merge_ties(s, med):
    """the outward merge of mad_of_sorted: (how often its two runs offer equal deviations while both still have elements, how often
    it takes from one run after the other has run out)"""
    m = len(s)
    mid = m // 2
    l, r, ties, exhausted = mid - 1, mid, 0, 0
    for _ in range(mid + 1):
        if l >= 0 and r < m:
            dl, dr = F(abs(F(s[l] - med))), F(abs(F(s[r] - med)))
            ties += bool(dl == dr)
            take_l = bool(dl <= dr)
        else:
            take_l = l >= 0
            exhausted += 1
        if take_l:
            l -= 1
        else:
            r += 1
    return ties, exhausted


_traces = {}


def trace(values, sl, sh, mutation=""):
    """finalize's rounds (drizzle.rs:134-179 as tests/drizzle_restatement.py states them) until one removes nothing: a list of
    dict(m, mad0, tie, merge_ties, removed), and the survivors.  `mutation` restates one decision wrongly, for the sensitivity
    tests: "strict" (> and < at the thresholds), "nofloor" (no 1e-10 under sigma), "ftz" (subnormals read and computed as zero),
    "f64median" (the average of the two middle samples taken in f64), "f64mad" (the same for the two middle deviations)."""
    key = (tuple(float(v) for v in values), tuple(bool(np.signbit(v)) for v in values), float(sl), float(sh), mutation)
    if key in _traces:
        return _traces[key]
    tiny = np.finfo(F).tiny

    def z(x):
        return F(0.0) if mutation == "ftz" and abs(x) < tiny else x

    def median(vals):
        s = sorted(vals)
        n = len(s)
        if mutation == "f64median" and n % 2 == 0:
            return F((float(s[n // 2 - 1]) + float(s[n // 2])) / 2.0)
        return z(R.median_f32(s))

    sl, sh = F(sl), F(sh)
    active = sorted(z(F(v)) for v in values)
    rounds = []
    with np.errstate(all="ignore"):
        while len(active) >= 3:
            med = median(active)
            dev = [z(F(v - med)) for v in active]
            devs = sorted(F(abs(d)) for d in dev)
            if mutation == "f64mad" and len(devs) % 2 == 0:
                mad = F((float(devs[len(devs) // 2 - 1]) + float(devs[len(devs) // 2])) / 2.0)
            else:
                mad = median(devs)
            sigma = F(float(mad) * R.MAD_TO_SIGMA) if mutation == "nofloor" else F(max(float(mad) * R.MAD_TO_SIGMA, 1e-10))
            lo, hi = z(F(-sl * sigma)), z(F(sh * sigma))
            if mutation == "strict":
                kept = [v for v, d in zip(active, dev) if bool(d > lo) and bool(d < hi)]
            else:
                kept = [v for v, d in zip(active, dev) if bool(d >= lo) and bool(d <= hi)]
            ties, exhausted = _merge_ties(active, med)
            rounds.append(dict(m=len(active), mad0=bool(mad == 0), tie=any(bool(d == lo) or bool(d == hi) for d in dev),
                               merge_ties=ties, exhausted=exhausted, removed=len(active) - len(kept)))
            if len(kept) == len(active):
                break
            active = kept
    _traces[key] = rounds
    return rounds


def rejected_after(values, sl, sh, iters, mutation=""):
    return sum(r["removed"] for r in trace(values, sl, sh, mutation)[:iters])


def census(case):
    """what the designed pixels of a case contain, from the rounds that its sigma_iterations lets run"""
    out = dict(tie_pixels=0, mad0_rounds=0, merge_ties=0, exhausted=0, none_survive=0, counts=set(), acting_max=0, odd_survivors=0, even_survivors=0)
    for _, _, vals, _ in case.designed:
        out["counts"].add(len(vals))
        if len(vals) < 2:
            continue
        rounds = trace(vals, case.sl, case.sh)[:case.iters]
        out["tie_pixels"] += any(r["tie"] for r in rounds)
        out["mad0_rounds"] += sum(r["mad0"] for r in rounds)
        out["merge_ties"] += sum(r["merge_ties"] for r in rounds)
        out["exhausted"] += sum(r["exhausted"] for r in rounds)
        left = len(vals) - sum(r["removed"] for r in rounds)
        out["none_survive"] += left == 0
        out["odd_survivors"] += left % 2 == 1
        out["even_survivors"] += left > 0 and left % 2 == 0
        out["acting_max"] = max(out["acting_max"], sum(r["removed"] > 0 for r in rounds))
    return out


# ---- placing lists -------------------------------------------------------------------------------------------------------------------
def place_two(lists, n, seed):
    """`lists`: [(tag, values)], each of at most 2 n finite values -> (frames, offsets, scale, pixfrac, designed)"""
    per_row = COLS - 1
    assert len(lists) <= (ROWS // 2) * per_row, len(lists)
    cols = min(COLS, max(3, -(-len(lists) // (ROWS // 2)) + 1))
    per_row = cols - 1
    stack = np.full((n, ROWS, cols), np.nan, F)
    rng = np.random.default_rng(seed)
    designed = []
    for j, (tag, vals) in enumerate(lists):
        vals = [F(v) for v in vals]
        assert len(vals) <= 2 * n and all(np.isfinite(v) for v in vals), tag
        oy, ox = 2 * (j // per_row), j % per_row
        slots = np.sort(rng.choice(2 * n, len(vals), replace=False))
        for s, v in zip(slots, vals):
            stack[s // 2, oy + s % 2, ox + 1] = v
        designed.append((oy, ox, tuple(vals), tag))
    return tuple(_ro(f) for f in stack), ((0.5, 0.0),) * n, 1.0, 1.0, tuple(designed)


def place_one(lists, n, seed):
    """`lists`: [(tag, values)], each of at most n finite values -> (frames, offsets, scale, pixfrac, designed)"""
    assert len(lists) <= ROWS * COLS
    cols = min(COLS, max(2, -(-len(lists) // ROWS)))
    stack = np.full((n, ROWS, cols), np.nan, F)
    rng = np.random.default_rng(seed)
    designed = []
    for j, (tag, vals) in enumerate(lists):
        vals = [F(v) for v in vals]
        assert len(vals) <= n and all(np.isfinite(v) for v in vals), tag
        iy, ix = j // cols, j % cols
        slots = np.sort(rng.choice(n, len(vals), replace=False))
        for s, v in zip(slots, vals):
            stack[s, iy, ix] = v
        designed.append((2 * iy, 2 * ix, tuple(vals), tag))
    return tuple(_ro(f) for f in stack), ((0.0, 0.0),) * n, 2.0, 0.5, tuple(designed)


def lengths(m, lo):
    """odd and even lengths from `lo`, and the last two that fit"""
    return sorted({v for v in (lo, lo + 1, lo + 2, lo + 3, m - 1, m) if lo <= v <= m})


def _shuffled(vals, rng):
    vals = list(vals)
    rng.shuffle(vals)
    return vals


# ---- A1: threshold ties --------------------------------------------------------------------------------------------------------------
X_TIE = F(F(2.0) * F(0.5 * R.MAD_TO_SIGMA))   # f32(sh * sigma) for MAD 0.5 and sh = 2


def tie_list(length, outer_lo, outer_hi, a=0.5):
    """[outer_lo, -a x p, 0 x z, a x p, outer_hi] of `length` >= 5: median 0 and MAD a whatever the length"""
    z = 1 if length % 2 else 2
    p = (length - 2 - z) // 2
    assert p >= 1
    return [outer_lo] + [-a] * p + [0.0] * z + [a] * p + [outer_hi]


A1D_SCALES = (0, -20, 7, 100)
A1D_VARIANTS = (("tie", X_TIE), ("over", np.nextafter(X_TIE, F(np.inf))), ("under", np.nextafter(X_TIE, F(0.0))))


def a1d_lists(m, rng):
    out = []
    for li, length in enumerate(lengths(m, 5)):
        scales = A1D_SCALES if length == 5 else (A1D_SCALES[li % 4], A1D_SCALES[(li + 1) % 4])
        for side in (1.0, -1.0):
            for vname, x in A1D_VARIANTS:
                for k in scales:
                    vals = [F(side * float(v) * 2.0 ** k) for v in tie_list(length, -1.0, float(x))]
                    out.append((f"{vname}-{'hi' if side > 0 else 'lo'}-L{length}-k{k}", _shuffled(vals, rng)))
    return out


A1G_A, A1G_GRID = 0.75, 2.0 ** -12
A1G_MEDIANS = (1.0, -2.0, 24.0, 640.0, -1536.0, 2048.0)
A1G_VARIANTS = ((0, None), (1, None), (-1, None), (None, 0), (None, 1), (None, -1), (0, 0))


def _search_factor(target, sigma, start):
    """the f32 factor nearest `start` with f32(factor * sigma) == target, by single-ulp steps to either side"""
    up = down = F(start)
    for _ in range(64):
        for cand in (up, down):
            if F(cand * sigma) == F(target):
                return cand
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
    return None   # (sigma > 1: the products of neighbouring factors step over about one f32 in ten)


def _tie_factor(start, sigma):
    """(deviation on the grid, factor) nearest `start` * sigma for which such a factor exists"""
    base = round(start * float(sigma) / A1G_GRID)
    for j in range(64):
        for d in ((base + j) * A1G_GRID, (base - j) * A1G_GRID):
            f = _search_factor(d, sigma, d / float(sigma))
            if f is not None:
                return d, float(f)
    raise AssertionError("no factor found")


def a1g_settings(seed):
    """(sl, sh, d_lo, d_hi): deviations on the 2^-12 grid and the sigma factors that put the thresholds exactly on them"""
    rng = np.random.default_rng(seed)
    sigma = F(A1G_A * R.MAD_TO_SIGMA)
    sh0, sl0 = 2.7 + 0.05 * rng.random(), 3.3 + 0.05 * rng.random()
    d_hi, sh = _tie_factor(sh0, sigma)
    d_lo, sl = _tie_factor(sl0, sigma)
    return sl, sh, d_lo, d_hi


def a1g_lists(m, rng, d_lo, d_hi):
    out = []
    inlier = 1.25 * A1G_A
    for li, length in enumerate(lengths(m, 5)):
        medians = A1G_MEDIANS if length == 5 else (A1G_MEDIANS[li % 6], A1G_MEDIANS[(li + 3) % 6])
        for hi_step, lo_step in A1G_VARIANTS:
            hi = inlier if hi_step is None else d_hi + hi_step * A1G_GRID
            lo = inlier if lo_step is None else d_lo + lo_step * A1G_GRID
            for med in medians:
                vals = [F(med + v) for v in tie_list(length, -lo, hi, A1G_A)]
                assert all(float(v) == med + d for v, d in zip(vals, tie_list(length, -lo, hi, A1G_A)))   # (on the grid: exact)
                out.append((f"hi{hi_step}-lo{lo_step}-L{length}-med{med}", _shuffled(vals, rng)))
    return out


# ---- A2: MAD == 0 --------------------------------------------------------------------------------------------------------------------
T_FLOOR = F(F(3.0) * F(1e-10))   # the high threshold at sigma 3 when the floor holds


def a2_lists(m, rng):
    c = F(900.0)
    near = [np.nextafter(c, F(np.inf)), np.nextafter(c, F(-np.inf))]
    around0 = [F(2e-10), F(4e-10), F(-2e-10), F(-4e-10), T_FLOOR, np.nextafter(T_FLOOR, F(np.inf)), -T_FLOOR, -np.nextafter(T_FLOOR, F(np.inf))]
    out = []
    for length in lengths(m, 3):
        major = length // 2 + 1
        rest = length - major
        out.append((f"ulp-L{length}", _shuffled([c] * major + [near[i % 2] for i in range(rest)], rng)))
        for rot in (0, 3):
            out.append((f"floor{rot}-L{length}", _shuffled([F(0.0)] * major + [around0[(i + rot) % 8] for i in range(rest)], rng)))
        out.append((f"equal-L{length}", [c] * length))
    return out


# ---- A3: duplicates on both sides of the median --------------------------------------------------------------------------------------
def a3_lists(m, rng):
    c, d = 900.0, 0.25
    out = []
    for length in sorted(set(lengths(m, 4)) | set(range(4, min(m, 12) + 1))):
        half = length // 2
        lows = [c - d * (1 + j // 2) for j in range(half)]
        highs = [c + d * (1 + j // 2) for j in range(half)]
        centre = [c] * (length % 2)
        out.append((f"steps-L{length}", _shuffled(lows + centre + highs, rng)))
        out.append((f"two-valued-L{length}", _shuffled([c - d] * half + [c + d] * (length - half), rng)))
        out.append((f"steps-outlier-L{length}", _shuffled(lows + centre + highs[:-1] + [c + 1000.0], rng)))
    # an even list whose upper half is all b = 1 + 2u and whose lower half ends in a = 1 + u (u = 2^-23): a + b = 2 + 3u is a tie of the
    # f32 addition and rounds to 2 + 4u, so the median IS b; the right run (deviations 0) is used up after L / 2 steps and the last
    # step must come from the left run alone: MAD = (0 + u) / 2.  The mirror image uses up the left run.
    u = 2.0 ** -23
    for length in sorted({v for v in lengths(m, 4) if v % 2 == 0}):
        half = length // 2
        base = [1.0 + 2.0 * u] * half + [1.0 + u] + [1.0 - j * u for j in range(half - 1)]
        for k in (0, 10):
            out.append((f"right-run-out-L{length}-k{k}", _shuffled([F(v * 2.0 ** k) for v in base], rng)))
            out.append((f"left-run-out-L{length}-k{k}", _shuffled([F(-v * 2.0 ** k) for v in base], rng)))
    return out


# ---- A4: subnormals ------------------------------------------------------------------------------------------------------------------
def a4_lists(m, rng):
    out = []
    tiny = float(np.finfo(F).tiny)
    for length in lengths(m, 5):
        out.append((f"ramp-L{length}", _shuffled([F(k * float(U)) for k in range(1, length)] + [F(50 * float(U))], rng)))
        out.append((f"random-L{length}", [F(int(k) * float(U)) for k in rng.integers(0, 21, length)]))
        out.append((f"edge-of-normal-L{length}", _shuffled([F(tiny + (j - length // 2) * float(U)) for j in range(length)], rng)))
        out.append((f"both-signs-L{length}", [F(int(k) * float(U)) for k in rng.integers(-9, 10, length)]))
    return out


# ---- A5: near FLT_MAX ----------------------------------------------------------------------------------------------------------------
def a5_lists(m, rng):
    out = []
    evens = sorted({v for v in lengths(m, 4) if v % 2 == 0} | {4})
    for length in evens:
        half = length // 2
        lows = [F(-rng.uniform(2.5e38, 3.3e38)) for _ in range(half - 1)]
        highs = [F(rng.uniform(1.8e38, 3.3e38)) for _ in range(half + 1)]
        out.append((f"median-inf-L{length}", _shuffled(lows + highs, rng)))
        xs = [F(rng.uniform(2.0e38, 3.3e38)) for _ in range(half)]
        out.append((f"pairs-L{length}", _shuffled(xs + [-x for x in xs], rng)))
        xs = [F(rng.uniform(0.5e38, 1.6e38)) for _ in range(half)]
        out.append((f"pairs-mid-L{length}", _shuffled(xs + [-x for x in xs], rng)))
    for length in (v for v in evens if v >= 6):     # the two middle deviations sum past FLT_MAX; half their f64 sum times 1.4826 would not
        half = length // 2
        xs = [F(rng.uniform(1.75e38, 1.95e38)) for _ in range(half - 1)] + [F(rng.uniform(3.0e38, 3.3e38))]
        out.append((f"mad-overflow-L{length}", _shuffled(xs + [-x for x in xs], rng)))
    for length in sorted({v for v in lengths(m, 5) if v % 2 == 1} | {5}):
        if length > m:
            continue
        xs = [F(rng.uniform(2.0e38, 3.3e38)) for _ in range(length // 2)]
        out.append((f"pairs-and-zero-L{length}", _shuffled(xs + [-x for x in xs] + [F(0.0)], rng)))
    return out


# ---- A6: many rounds -----------------------------------------------------------------------------------------------------------------
_a6 = []


def a6_lists():
    """64-sample N(900, 40) lists rounded to 2^-8: of 400 seeded draws the 140 with the most acting rounds under (1, 1), and 16 as drawn"""
    if not _a6:
        rng = np.random.default_rng(606)
        draws = [[F(v) for v in np.round(rng.normal(900.0, 40.0, 64) * 256.0) / 256.0] for _ in range(400)]
        acting = [sum(r["removed"] > 0 for r in trace(d, 1.0, 1.0)) for d in draws]
        order = np.argsort(-np.array(acting), kind="stable")
        chosen = list(order[:140]) + list(order[-16:])
        _a6.extend((f"rounds{acting[i]}-draw{i}", draws[i]) for i in chosen)
    return list(_a6)


# ---- A7: every count -----------------------------------------------------------------------------------------------------------------
def a7_lists(m, rng):
    def draw(length):
        v = np.round(rng.normal(900.0, 40.0, length) * 256.0) / 256.0
        if length >= 4 and rng.random() < 0.5:
            v[rng.integers(0, length)] += 6000.0
        return [F(x) for x in v]

    out = [(f"count{length}", draw(length)) for length in range(m + 1)]
    out += [(f"count{m}-again{k}", draw(m)) for k in range(4)]
    while len(out) < min(2 * (m + 1) + 4, (ROWS // 2) * (COLS - 1)):
        length = int(rng.integers(2, m + 1))
        out.append((f"count{length}-more{len(out)}", draw(length)))
    return out


# ---- A8: zeros of either sign --------------------------------------------------------------------------------------------------------
def a8_lists(n, rng):
    nz, pz = F(-0.0), F(0.0)
    out = [("single-negative-zero", [nz]), ("single-positive-zero", [pz]), ("single-negative-zero-again", [nz]), ("single-900", [F(900.0)]),
           ("two-negative-zeros", [nz, nz]), ("mixed-zeros", [nz, pz, nz])]
    if n >= 4:
        out.append(("mixed-zeros-4", [pz, nz, nz, pz]))
    out += [(f"a2-{t}", v) for t, v in a2_lists(n, rng)] + [(f"a3-{t}", v) for t, v in a3_lists(n, rng) if len(v) <= n]
    return out


# ---- the designed cases --------------------------------------------------------------------------------------------------------------
A1G_SETTINGS = a1g_settings(11)


def _two(name, family, lists, n, seed, **kw):
    frames, offsets, scale, pixfrac, designed = place_two(lists, n, seed)
    return Case(name, family, frames, offsets, scale, pixfrac, R.SQUARE, designed=designed, **kw)


def cap_case():
    """scale 1, pixfrac 1, zero offsets: four pushes per frame, so frames 0 and 1 fill the interior lists of 5 frames to the cap of
    10 (frame 2 gets two in), and frames 3 and 4 are dropped whole; frame k's values lie in [1000 k, 1000 k + 64)"""
    rng = np.random.default_rng(99)
    frames = tuple(_ro(1000.0 * k + rng.integers(0, 64 * 256, (ROWS, COLS)) / 256.0) for k in range(5))
    return Case("cap-four-pushes-n5", "cap", frames, ((0.0, 0.0),) * 5, 1.0, 1.0)


_designed = []


def designed_cases():
    if _designed:
        return list(_designed)
    out = []
    sl_g, sh_g, d_lo, d_hi = A1G_SETTINGS
    for n in FRAME_COUNTS:
        m = 2 * n
        rng = np.random.default_rng(1000 + n)
        out.append(_two(f"A1d-n{n}", "A1d", a1d_lists(m, rng), n, n, sl=2.0, sh=2.0))
        out.append(_two(f"A1g-n{n}", "A1g", a1g_lists(m, rng, d_lo, d_hi), n, n, sl=sl_g, sh=sh_g))
        out.append(_two(f"A2-n{n}", "A2", a2_lists(m, rng), n, n))
        out.append(_two(f"A3-n{n}", "A3", a3_lists(m, rng), n, n))
        a4 = a4_lists(m, rng)
        out.append(_two(f"A4z-n{n}", "A4z", a4, n, n, sl=0.0, sh=0.0))
        out.append(_two(f"A4d-n{n}", "A4d", a4, n, n))
        a5 = a5_lists(m, rng)
        out.append(_two(f"A5z-n{n}", "A5z", a5, n, n, sl=0.0, sh=0.0))
        out.append(_two(f"A5d-n{n}", "A5d", a5, n, n))
        out.append(_two(f"A5o-n{n}", "A5o", a5, n, n, sl=1.0, sh=1.0))
        out.append(_two(f"A7-n{n}", "A7", a7_lists(m, rng), n, n))
        frames, offsets, scale, pixfrac, designed = place_one(a8_lists(n, rng), n, n)
        out.append(Case(f"A8-n{n}", "A8", frames, offsets, scale, pixfrac, designed=designed))
    for n in (32, 33):
        frames, offsets, scale, pixfrac, designed = place_two(a6_lists(), n, 6000 + n)
        for it in A6_ITERS:
            out.append(Case(f"A6-n{n}-it{it}", "A6", frames, offsets, scale, pixfrac, sl=1.0, sh=1.0, iters=it, designed=designed))
    out.append(cap_case())
    _designed.extend(out)
    return list(out)


# ---- B: geometry ---------------------------------------------------------------------------------------------------------------------
def dyadic_frames(n, rows, cols, seed, bad=True):
    """multiples of 2^-8 below 2^14 around 900, a few hot pixels, and (bad) NaN / +-inf pixels"""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n):
        f = 900.0 + rng.normal(0.0, 2.0, (rows, cols))
        hot = rng.random((rows, cols)) < 0.04
        f[hot] += rng.uniform(2000.0, 15000.0, int(hot.sum()))
        f = (np.round(f * 256.0) / 256.0).astype(F)
        if bad:
            u = rng.random((rows, cols))
            f[u < 0.02] = np.nan
            f[(u >= 0.02) & (u < 0.03)] = np.inf
            f[(u >= 0.03) & (u < 0.04)] = -np.inf
        frames.append(_ro(f))
    return tuple(frames)


def step(x, k):
    """x moved by k f64 ulps"""
    for _ in range(abs(k)):
        x = float(np.nextafter(x, np.inf if k > 0 else -np.inf))
    return x


EIGHTHS = ((0, 0), (2, -2), (-2, 4), (1, -1), (4, 2), (-4, -6), (8, -8), (-12, 3), (6, 20))


def b1_cases():
    out = []
    for scale in (1.0, 2.0, 4.0):
        for pixfrac in (0.5, 1.0):
            offsets = tuple((kx / 8.0, ky / 8.0) for kx, ky in EIGHTHS)
            frames = dyadic_frames(len(offsets), 5, 7, seed=int(scale * 10 + pixfrac * 2))
            for kernel in KERNELS:
                out.append(Case(f"B1a-s{scale}-p{pixfrac}-{KNAME[kernel]}", "B1a", frames, offsets, scale, pixfrac, kernel))
    for scale in (1.5, 2.5, 3.0):
        for pixfrac in (0.5, 1.0):
            half = pixfrac * scale * 0.5
            bases = (1.0 / scale, -2.0 / scale, (1.0 + half) / scale, -(2.0 - half) / scale, (3.0 - half) / scale, -half / scale)
            offsets = [(0.0, 0.0)]
            for bi, b in enumerate(bases[:3]):
                other = bases[3 + bi]
                for k in (0, 1, -1, 2, -2):
                    offsets.append((step(b, k), step(other, -k)) if bi % 2 == 0 else (step(other, k), step(b, -k)))
            frames = dyadic_frames(len(offsets), 5, 7, seed=int(scale * 10 + pixfrac * 2) + 100)
            for kernel in KERNELS:
                out.append(Case(f"B1b-s{scale}-p{pixfrac}-{KNAME[kernel]}", "B1b", frames, tuple(offsets), scale, pixfrac, kernel))
    return out


def b2_cases():
    out = []
    for rows, cols in ((1, 1), (1, 5), (5, 1), (2, 2)):
        for n in (4, 33):
            rng = np.random.default_rng(rows * 100 + cols * 10 + n)
            kinds = [(0.0, 0.0), (0.375, -0.25), (cols + 0.125, 0.0), (1e6, -1e3)]            # on it, inside, just off, far off
            while len(kinds) < n:
                k = len(kinds) % 6
                e = [float(v) / 8.0 for v in rng.integers(-12, 13, 2)]
                kinds.append([(e[0], e[1]), (cols + abs(e[0]), e[1]), (e[0], -(rows + abs(e[1]))), (-(cols - 0.5) + e[0] / 8.0, e[1]),
                              (e[0] * 1e5, e[1]), (e[0], rows + 2.0 + abs(e[1]))][k])
            frames = dyadic_frames(n, rows, cols, seed=rows * 7 + cols + n, bad=False)
            for kernel in KERNELS:
                out.append(Case(f"B2-{rows}x{cols}-n{n}-{KNAME[kernel]}", "B2", frames, tuple(kinds), 1.0, 1.0, kernel))
    return out


FAR = (("1e3", 1e3), ("1e6", 1e6), ("2p31-half", 2.0 ** 31 - 0.5), ("2p31+half", 2.0 ** 31 + 0.5), ("1e9", 1e9), ("1e12", 1e12),
       ("1e18", 1e18), ("1e300", 1e300))


def b3_cases():
    out = []
    for i, (tag, mag) in enumerate(FAR):
        scale, pixfrac = ((2.0, 0.7), (1.0, 1.0))[i % 2]
        offsets = ((0.0, 0.0), (mag, 0.25), (0.375, -1.25), (-0.5, -mag), (-2.5, 0.625), (-mag, mag))
        frames = dyadic_frames(6, 6, 8, seed=300 + i)
        for kernel in KERNELS:
            out.append(Case(f"B3-{tag}-{KNAME[kernel]}", "B3", frames, offsets, scale, pixfrac, kernel, far=(1, 3, 5)))
    return out


def b4_cases():
    """reported offsets (the reference negates them) that put frame k's nearest pixel centre `dist` beyond a border pixel's centre"""
    out = []
    rows, cols = 5, 6
    for scale, pixfrac in ((2.0, 0.7), (1.0, 1.0), (4.0, 1.0)):
        sigma = max(pixfrac * scale * 0.5, 0.5)
        orows, ocols = int(np.ceil(rows * scale)), int(np.ceil(cols * scale))
        offsets, note = [(0.0, 0.0)], []
        for sign in (-1.0, 1.0):
            dist = 7.44 * sigma + sign * 0.01
            left = -((0.5 - dist) / scale - (cols - 1))                 # the frame's last column, left of output column 0
            right = -((ocols - 0.5 + dist) / scale)                     # its first column, right of the last output column
            top = -((0.5 - dist) / scale - (rows - 1))
            bottom = -((orows - 0.5 + dist) / scale)
            on_row = -0.5 / scale                                       # an input centre exactly on output-pixel centres across
            offsets += [(left, on_row), (right, on_row), (on_row, top), (on_row, bottom)]
            d = dist / np.sqrt(2.0)                                      # the corner: `dist` along the diagonal
            offsets.append((-((0.5 - d) / scale - (cols - 1)), -((0.5 - d) / scale - (rows - 1))))
            note.append((sign, len(offsets) - 5, len(offsets)))
        frames = dyadic_frames(len(offsets), rows, cols, seed=int(400 + scale * 10), bad=False)
        out.append(Case(f"B4-s{scale}-p{pixfrac}", "B4", frames, tuple(offsets), scale, pixfrac, R.GAUSSIAN, note=tuple(note)))
    return out


def b5_cases():
    out = []
    for rows, cols in ((2, 32), (4, 64)):
        for n in (5, 33):
            rng = np.random.default_rng(500 + rows + n)
            offsets = ((0.0, 0.0),) + tuple((float(a) / 8.0, float(b) / 8.0) for a, b in rng.integers(-16, 17, (n - 1, 2)))
            frames = dyadic_frames(n, rows, cols, seed=500 + rows * 3 + n)
            for kernel in KERNELS:
                out.append(Case(f"B5-{int(rows * 2)}x{int(cols * 2)}-n{n}-{KNAME[kernel]}", "B5", frames, offsets, 2.0, 0.7, kernel))
    return out


_geometry = []


def geometry_cases():
    if not _geometry:
        _geometry.extend(b1_cases() + b2_cases() + b3_cases() + b4_cases() + b5_cases())
    return list(_geometry)
