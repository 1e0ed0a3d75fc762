"""Adversarial planes for the whole-plane radix selects (pure numpy, fixed seeds: no GPU, no library, no oracle import).

csrc/plane_select.hip (and the device-resident copy of it in csrc/masked_stretch.hip) is an 11/11/10-bit radix select on f32 bit
patterns: level-0 bin = bits >> 21, level-1 bin = (bits >> 10) & 0x7ff, level-2 bin = bits & 0x3ff.  Continuous random data never
puts a rank on the first or last element of a bin, never splits the two middle ranks of an even count between two bins, and ties
only briefly.  The families built here do all of that, on purpose:

  pairs        adjacent f32 values that differ at exactly one level of the select (PAIRS)
  populations  candidates for ab_tile_percentile_bounds (finite and > 1e-7f): two-valued (a rank pair that straddles the pair's
               edge), four-valued (a quartile rank on the first / last element of a level-0 bin), long ties -- every one interleaved
               with values that must not be counted (CONTAMINATION)
  background   B1 .. B6: images whose sample count, model median and corrected plane read the global median / MAD to the ulp
  wavelet      planes whose finest detail plane |d_0| is tied at its median
  masked       planes for the masked stretch whose median sits on few levels, with a soft mask that pulls the real median away from
               the one the blend pass predicts

tests/test_select_adversarial_cpu.py holds every fixture to what it claims here (against numpy, the restatements and the CPU oracle)
so that a fixture that has drifted fails there and the GPU test cannot pass by testing nothing.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
INF = F32(np.inf)


def from_bits(b: int) -> np.float32:
    return np.array([b], np.uint32).view(F32)[0]


def bits_of(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def key(v) -> int:
    """the select's key of one value: its f32 bit pattern"""
    return int(bits_of(np.array([v], F32))[0])


def level_bins(v):
    """(level-0, level-1, level-2) bins of the key of v"""
    b = key(v)
    return b >> 21, (b >> 10) & 0x7FF, b & 0x3FF


FLOOR = F32(1e-7)                                   # the validity threshold of percentile_bounds / the cells: a strict `>`
FLOOR_UP = np.nextafter(FLOOR, INF)

# name -> (lower, upper, the one level of the select at which the two differ)
PAIRS = {
    "L0": (from_bits(0x3F9FFFFF), from_bits(0x3FA00000), 0),      # at 1.25
    "BINADE": (from_bits(0x3F7FFFFF), from_bits(0x3F800000), 0),  # at the exponent edge
    "L1": (from_bits(0x3F8003FF), from_bits(0x3F800400), 1),
    "L2": (from_bits(0x3F800400), from_bits(0x3F800401), 2),
    "TOP": (from_bits(0x7F7FFFFE), from_bits(0x7F7FFFFF), 2),     # the largest finite values
    "FLOOR": (FLOOR, FLOOR_UP, 2),                                # (lower is NOT a candidate of percentile_bounds)
}

# four values in four different level-0 bins (0x1fb .. 0x1fe)
FOUR_VALUES = (from_bits(0x3F7FFFFF), from_bits(0x3F800000), from_bits(0x3FA00000), from_bits(0x3FC00000))

# never a candidate of percentile_bounds (the last one only there: 1e-7f fails the strict `>`)
CONTAMINATION = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, -3.0e38, 1e-8, 1e-7], F32)

PCT_PAIRS = ((0.5, 0.5), (0.499, 0.501), (0.0, 1.0), (0.001, 0.999), (0.25, 0.75), (0.2499, 0.7499), (1.0, 0.0))
M_LIST = (1, 2, 3, 4, 255, 256, 257, 1000, 1001)
BIG = 600_001      # past the 256 x 8 x 256 pixels one grid stride of the histogram kernel covers, and no multiple of 256


def is_candidate(a):
    """percentile_bounds' filter (tiles.rs:150-154)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (a > FLOOR)


@dataclass
class Population:
    name: str
    values: np.ndarray           # f32, 1-D: the candidates interleaved with CONTAMINATION
    count: int                   # how many of `values` are candidates
    middle: "tuple | None"       # (lower, upper): the [count / 2 - 1] and [count / 2] candidates of an even count
    meta: dict = field(default_factory=dict)

    def planes(self):
        """the population as a 1 x n plane and as a near-square one (padded with NaN, which is no candidate)"""
        n = self.values.size
        rows = max(int(np.sqrt(n)), 1)
        cols = -(-n // rows)
        sq = np.full(rows * cols, np.nan, F32)
        sq[:n] = self.values
        return self.values.reshape(1, n), sq.reshape(rows, cols)


def interleave(cands: np.ndarray, every: int = 2) -> np.ndarray:
    """one element of CONTAMINATION in front, one (in turn) after every `every` candidates, and whatever kinds have not had their
    turn by then at the end: every population holds every kind"""
    out, k = [CONTAMINATION[-1]], 0
    for i in range(0, cands.size, every):
        out.extend(cands[i:i + every])
        out.append(CONTAMINATION[k % CONTAMINATION.size])
        k += 1
    out.extend(CONTAMINATION[k:])
    return np.array(out, F32)


def two_valued(pair: str, m: int, seed: int = 0) -> Population:
    lower, upper, _ = PAIRS[pair]
    rng = np.random.default_rng(1000 * seed + m)
    cands = np.array([lower] * (m - m // 2) + [upper] * (m // 2), F32)
    rng.shuffle(cands)
    if pair == "FLOOR":        # only the copies of `upper` pass the strict `>`
        return Population(f"{pair}-{m}", interleave(cands), m // 2, None, dict(pair=pair, m=m))
    return Population(f"{pair}-{m}", interleave(cands), m, (lower, upper) if m % 2 == 0 else None, dict(pair=pair, m=m))


def big_two_valued() -> Population:
    """BIG candidates, one more `lower` than `upper`, so that the median is `lower` and losing ANY one copy of `lower` makes it
    `upper`: a copy of `lower` sits at index 0 and at the last index of the plane (the pixels a wrong grid stride or tail loses)."""
    lower, upper, _ = PAIRS["L0"]
    rng = np.random.default_rng(7)
    inner = np.array([lower] * (BIG - BIG // 2 - 2) + [upper] * (BIG // 2), F32)
    rng.shuffle(inner)
    step = inner.size // CONTAMINATION.size
    parts = [np.array([lower], F32)]
    for k in range(CONTAMINATION.size):       # the nine contaminants spread over the plane
        parts += [inner[k * step:(k + 1) * step], CONTAMINATION[k:k + 1]]
    parts += [inner[CONTAMINATION.size * step:], np.array([lower], F32)]
    return Population("L0-big", np.concatenate(parts), BIG, None, dict(pair="L0", m=BIG))


def four_valued(m: int) -> Population:
    assert m % 4 == 0
    rng = np.random.default_rng(m)
    cands = np.repeat(np.array(FOUR_VALUES, F32), m // 4)
    rng.shuffle(cands)
    return Population(f"four-{m}", interleave(cands), m, (FOUR_VALUES[1], FOUR_VALUES[2]), dict(m=m))


def one_value(v, m: int) -> Population:
    cands = np.full(m, v, F32)
    return Population(f"tie-{bits_of(cands[:1])[0]:08x}-{m}", interleave(cands), m, (F32(v), F32(v)) if m % 2 == 0 else None, dict(m=m))


def quantised_gaussian(m: int = 50_000) -> Population:
    """a 16-bit camera's sky: a Gaussian of 12 steps' width in steps of 1 / 65535 -- ties of thousands at every rank"""
    rng = np.random.default_rng(16)
    steps = np.rint(rng.normal(0.3, 12.0 / 65535.0, m) * 65535.0)
    cands = (steps / 65535.0).astype(F32)
    s = np.sort(cands)
    return Population(f"q16-{m}", interleave(cands, every=5), m, (s[m // 2 - 1], s[m // 2]), dict(m=m))


def populations() -> list:
    out = [two_valued(p, m, seed=i) for i, p in enumerate(PAIRS) for m in M_LIST]
    out.append(big_two_valued())
    out += [four_valued(m) for m in (4, 8, 256, 1000, 2052)]
    out += [one_value(PAIRS["L0"][1], m) for m in (1, 2, 257, 1000)] + [one_value(PAIRS["TOP"][1], 256), one_value(FLOOR_UP, 255)]
    out.append(quantised_gaussian())
    return out


def no_candidate_planes() -> dict:
    """planes on which percentile_bounds takes its min / max branch (tiles.rs:156-159)"""
    return {"all_nan": np.full((7, 33), np.nan, F32), "all_floor": np.full((9, 31), FLOOR, F32),
            "contamination_only": np.tile(CONTAMINATION, 29).reshape(29, CONTAMINATION.size)}


def percentile_statement(values, low_pct: float, high_pct: float):
    """percentile_bounds (tiles.rs:149-178) in plain numpy -> (lo, hi) as f32: the candidates sorted, indexed at
    min(int(m * pct), m - 1) with the product in f64; without a candidate, the minimum and maximum of the finite values folded from
    +-f32::MAX (math/simd.rs:263-271)"""
    v = np.asarray(values, F32).ravel()
    s = np.sort(v[is_candidate(v)])
    m = s.size
    if m == 0:
        fin = v[np.isfinite(v)]
        big = np.finfo(F32).max
        return (F32(min(big, fin.min())), F32(max(-big, fin.max()))) if fin.size else (big, -big)
    return s[min(int(float(m) * low_pct), m - 1)], s[min(int(float(m) * high_pct), m - 1)]


def pyramid_plane(rows: int = 300, cols: int = 260) -> np.ndarray:
    """the four values (an eighth of the plane each) and the L0 pair (a quarter each), shuffled and contaminated: the 0.1 % and
    99.9 % bounds sit inside long ties, and every tile byte is scaled by them"""
    rng = np.random.default_rng(300)
    n = rows * cols
    lower, upper, _ = PAIRS["L0"]
    vals = np.concatenate([np.repeat(np.array(FOUR_VALUES, F32), n // 8), np.full(n // 4, lower, F32),
                           np.full(n - 4 * (n // 8) - n // 4, upper, F32)])
    rng.shuffle(vals)
    vals[::97] = CONTAMINATION[np.arange(vals[::97].size) % CONTAMINATION.size]
    return vals.reshape(rows, cols)


# ---- background extraction ------------------------------------------------------------------------------------------------------
MAD_TO_SIGMA = F32(1.4826)


@dataclass
class BackgroundCase:
    name: str
    image: np.ndarray
    grid: int
    degree: int
    sigma_clip: float = 2.5
    meta: dict = field(default_factory=dict)


def _q16_sky(rng, rows, cols, level=1000.0, sigma=3.0):
    """an integer-quantised sky: the global median, the MAD and every cell median are long ties"""
    return np.rint(rng.normal(level, sigma, (rows, cols))).astype(F32)


def _cell_box(rows, cols, grid, gy, gx):
    ch, cw = rows // grid, cols // grid
    return slice(gy * ch, (gy + 1) * ch), slice(gx * cw, (gx + 1) * cw)


def b1_three_valued(rows=256, cols=256, grid=8) -> BackgroundCase:
    """30 % M, 35 % M - D, 35 % M + D: the global median is M and the MAD is D, both deep inside ties.  Four whole cells are flat at
    hi, nextafter(hi, +inf), lo and nextafter(lo, -inf), with hi / lo formed in f32 as background.rs:147-179 forms them: the cells
    at hi and lo are samples and the other two are not (grid^2 - 2 samples).  A median one ulp off moves both thresholds by one ulp and
    makes another pair of them the samples -- the same count, other coefficients; a wrong MAD changes the count."""
    rng = np.random.default_rng(1)
    M, D, kappa = F32(1000.0), F32(3.0), F32(2.5)
    sigma = D * MAD_TO_SIGMA
    hi, lo = M + kappa * sigma, M - kappa * sigma
    flat = {(1, 2): hi, (2, 5): np.nextafter(hi, INF), (5, 1): lo, (6, 6): np.nextafter(lo, -INF)}
    n = rows * cols - len(flat) * (rows // grid) * (cols // grid)
    n_mid = int(round(0.30 * n))
    n_low = (n - n_mid) // 2
    sky = np.concatenate([np.full(n_mid, M, F32), np.full(n_low, M - D, F32), np.full(n - n_mid - n_low, M + D, F32)])
    rng.shuffle(sky)
    img = np.empty((rows, cols), F32)
    free = np.ones((rows, cols), bool)
    for (gy, gx), v in flat.items():
        box = _cell_box(rows, cols, grid, gy, gx)
        img[box] = v
        free[box] = False
    img[free] = sky
    return BackgroundCase("B1", img, grid, 1, 2.5, dict(M=M, D=D, hi=hi, lo=lo, outside=2))


def b2_straddling_middle(rows=256, cols=256) -> BackgroundCase:
    """an even candidate count whose two middle values are an L0 pair in the sky's range (0x447FFFFF | 0x44800000: level-0 bins 0x223
    and 0x224); the absolute deviations' two middle values are far apart as well (6.1e-5 and 3)"""
    rng = np.random.default_rng(2)
    lower, upper = from_bits(0x447FFFFF), from_bits(0x44800000)
    q = rows * cols // 4
    img = np.concatenate([np.full(q, lower, F32), np.full(q, F32(1021.0), F32), np.full(q, upper, F32), np.full(q, F32(1027.0), F32)])
    rng.shuffle(img)
    return BackgroundCase("B2", img.reshape(rows, cols), 8, 2, 2.5, dict(lower=lower, upper=upper))


def b3_degree0(rows=130, cols=258) -> BackgroundCase:
    """degree 0: the model is ONE value rows * cols times (an even count), and its median is added to every pixel of `corrected`"""
    img = _q16_sky(np.random.default_rng(3), rows, cols)
    img[7, 9] = np.nan
    return BackgroundCase("B3", img, 4, 0)


def b4_degree1(rows, cols) -> BackgroundCase:
    """degree 1 on a quantised sky with a gradient; the remainder rows and columns (rows % grid, cols % grid) belong to no cell but
    count in the global median: they hold extreme values (3e38 below, 1e-30 to the right)"""
    rng = np.random.default_rng(rows + cols)
    grid = 8
    y, x = np.mgrid[0:rows, 0:cols]
    img = np.rint(rng.normal(1000.0, 3.0, (rows, cols)) + 6.0 * y / rows - 4.0 * x / cols).astype(F32)
    ch, cw = rows // grid, cols // grid
    img[grid * ch:, :] = F32(3e38)
    img[:, grid * cw:] = F32(1e-30)
    img[3, 4], img[5, 6], img[rows // 2, cols // 2] = np.nan, np.inf, -np.inf
    return BackgroundCase(f"B4-{rows}x{cols}", img, grid, 1, 2.5, dict(remainder=(rows - grid * ch, cols - grid * cw)))


def b5_ramp(rows=256, cols=320) -> BackgroundCase:
    """a steep quantised ramp from -500 to 1500 along x: the left quarter is not positive (no candidate, its cells are skipped), the
    fitted plane is <= 0 there, and the model median is taken over a strict subset of the model"""
    x = np.arange(cols, dtype=np.float64)
    img = np.broadcast_to(np.floor(-500.0 + 2000.0 * x / cols), (rows, cols)).astype(F32)
    return BackgroundCase("B5", np.ascontiguousarray(img), 8, 1)


def b6_tiny_pixels(rows=256, cols=256, scattered=False) -> BackgroundCase:
    """40 % of the plane at 1e-8: candidates for the global median (> 0), invalid for the cells (<= 1e-7).  Gathered: the left three
    grid columns and 4 % of the rest -- the global median is the sky's 1/6 quantile, 40 cells are samples.  Scattered: every cell is
    more than 30 % invalid -> "Not enough background samples (0)"."""
    rng = np.random.default_rng(6 + int(scattered))
    img = _q16_sky(rng, rows, cols)
    if scattered:
        tiny = rng.random((rows, cols)) < 0.40
    else:
        tiny = rng.random((rows, cols)) < 0.04
        tiny[:, :3 * (cols // 8)] = True
    img[tiny] = F32(1e-8)
    return BackgroundCase("B6-scattered" if scattered else "B6", img, 8, 1, 2.5, dict(tiny=tiny))


def background_cases() -> list:
    return [b1_three_valued(), b2_straddling_middle(), b3_degree0(), b4_degree1(256, 256), b4_degree1(263, 517), b5_ramp(),
            b6_tiny_pixels(), b6_tiny_pixels(scattered=True)]


# ---- wavelet planes: |d_0| tied at its median ------------------------------------------------------------------------------------
WAVELET_SHAPES = ((64, 64), (65, 67))


def wavelet_planes() -> list:
    """[(name, plane, parity of the finite count of d_0)]: each kind at both shapes, with and without one interior NaN pixel (which
    poisons its 5 x 5 footprint of d_0: 25 details, so the parity flips)"""
    out = []
    for rows, cols in WAVELET_SHAPES:
        y, x = np.mgrid[0:rows, 0:cols]
        kinds = {"checker": np.where((y + x) % 2 == 0, F32(100.0), F32(164.0)).astype(F32),
                 "stripes": np.where(x % 2 == 0, F32(10.0), F32(10.5)).astype(F32) + np.zeros((rows, cols), F32),
                 "integers": np.random.default_rng(rows).integers(0, 2, (rows, cols)).astype(F32)}
        for kind, img in kinds.items():
            for nan in (False, True):
                p = img.copy()
                if nan:
                    p[rows // 2, cols // 2 + 1] = np.nan
                out.append((f"{kind}-{rows}x{cols}" + ("-nan" if nan else ""), p, (rows * cols - (25 if nan else 0)) % 2))
    return out


# ---- masked-stretch planes -------------------------------------------------------------------------------------------------------
MASKED_SHAPES = ((160, 240), (333, 517))
MS_TARGETS = (0.25, 0.5, 0.3125, 0.2)      # the first three are level-0 bin edges, the last is mid-bin
MS_PROTECTIONS = (0.0, 0.5, 1.0)


def _q16_star_field(rng, rows, cols, n_stars=40):
    """a star field in steps of 1 / 65535 whose sky sits on a few levels only"""
    img = rng.normal(0.02, 1.5 / 65535.0, (rows, cols))
    for _ in range(n_stars):
        cy, cx, amp = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(0.05, 0.9)
        y0, y1, x0, x1 = max(int(cy) - 10, 0), min(int(cy) + 11, rows), max(int(cx) - 10, 0), min(int(cx) + 11, cols)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.5 * 1.5))
    img = (np.rint(np.clip(img, 0.0, 1.0) * 65535.0) / 65535.0).astype(F32)
    img[0, 0], img[1, 1], img[2, 2] = np.nan, -1.0, np.inf
    return img


def masked_planes() -> list:
    """[(name, image, mask)] at both shapes"""
    out = []
    for rows, cols in MASKED_SHAPES:
        rng = np.random.default_rng(rows)
        stars = _q16_star_field(rng, rows, cols)
        with np.errstate(invalid="ignore"):
            hard = np.where(stars > F32(0.05), F32(1.0), F32(0.0)).astype(F32)          # the cores masked out, the sky untouched
        two = rng.permutation(np.tile(np.array([0.2, 0.6], F32), rows * cols // 2 + 1)[:rows * cols]).reshape(rows, cols)
        block = np.zeros((rows, cols), F32)
        block[rows // 4:rows // 2, cols // 4:cols // 2] = F32(0.75)
        soft = np.where(rng.random((rows, cols)) < 0.45, rng.uniform(0.01, 0.49, (rows, cols)), 0.0).astype(F32)
        out += [(f"q16-stars-{rows}x{cols}", stars, hard), (f"two-valued-{rows}x{cols}", two, block),
                (f"soft-mask-{rows}x{cols}", stars, soft)]
    return out
