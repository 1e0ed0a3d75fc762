"""The spectral-cube functions of core/cube/{eager,lazy}.rs restated in plain numpy (no library, no GPU), and the fixtures the
cube tests share.

Independent of the library's method on purpose: sorts where the kernels select, a z-sequential f64 accumulation for the mean, the
rank arithmetic written as the reference writes it.  The normalisation is held in two forms: the DEFINITION the C header gives
(the f32 rounding of the f64 asinh of the f32 argument) and the reference's own f32 formula (Rust's f32::asinh:
ln_1p(ax + ax / (hypot(1, 1 / ax) + 1 / ax)) through f32 functions), whose bits depend on the libm and which the library is held
to within 2 ulp of, not to.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
NONZERO, ABOVE_PADDING = 0, 1          # ab_cube_valid_rule
PADDING = F32(1e-7)
MAD_TO_SIGMA = F32(1.4826)


def from_bits(b: int) -> np.float32:
    return np.array([b], np.uint32).view(F32)[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def valid(a, rule: int):
    """eager.rs:39 / :171 / simd.rs:227 (rule 0: finite && != 0.0); stats::is_valid_pixel (rule 1: finite && > 1e-7f)"""
    a = np.asarray(a, F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & ((a != 0) if rule == NONZERO else (a > PADDING))


def collapse_mean(cube, rule: int):
    """collapse_mean_simd (simd.rs:216-253) / collapse_mean_lazy (lazy.rs:246-284): one f64 addition per valid sample, ascending z"""
    cube = np.asarray(cube, F32)
    s = np.zeros(cube.shape[1:], np.float64)
    c = np.zeros(cube.shape[1:], np.uint32)
    for z in range(cube.shape[0]):
        m = valid(cube[z], rule)
        s[m] += cube[z][m].astype(np.float64)
        c[m] += 1
    out = np.zeros(cube.shape[1:], F32)
    out[c > 0] = (s[c > 0] / c[c > 0].astype(np.float64)).astype(F32)
    return out


def collapse_median(cube, rule: int):
    """collapse_median (eager.rs:28-55) / collapse_median_lazy (lazy.rs:286-329): element [len / 2] of the sorted valid samples"""
    cube = np.asarray(cube, F32)
    m = valid(cube, rule)
    n = m.sum(axis=0)
    s = np.sort(np.where(m, cube, F32(np.inf)), axis=0)            # (valid samples are finite: the placeholders sort last)
    pick = np.take_along_axis(s, np.minimum(n // 2, cube.shape[0] - 1)[None], axis=0)[0]
    return np.where(n > 0, pick, F32(0)).astype(F32)


def streaming_step(depth: int) -> int:
    """lazy.rs:334-335"""
    s = min(32, depth)
    return depth // s if depth > s else 1


def stat_ranks(n: int):
    """(median, low, high) ranks of n valid values (eager.rs:185, :199-200): the products in f64, truncated"""
    return n // 2, int(float(n) * 0.01), min(int(float(n) * 0.999), n - 1)


def global_stats(cube, rule: int, frame_step: int = 1):
    """compute_global_stats (eager.rs:168-208) / compute_global_stats_streaming (lazy.rs:331-370) -> ((median, sigma, low, high), n)"""
    cube = np.asarray(cube, F32)
    frames = cube[::max(1, int(frame_step))]
    v = frames[valid(frames, rule)]
    n = v.size
    if n == 0:
        return (F32(0), F32(1), F32(0), F32(1)), 0
    s = np.sort(v)
    mid, lo, hi = stat_ranks(n)
    median = s[mid]
    with np.errstate(over="ignore"):
        d = np.sort(np.abs(v - median))                            # f32 subtraction, as `(v - median).abs()`
        sigma = max(F32(d[n // 2] * MAD_TO_SIGMA), F32(1e-10))
    return (median, F32(sigma), s[lo], s[hi]), n


def normalize_argument(frame, stats):
    """the f32 argument of the asinh (eager.rs:211-219) and the mask of the finite pixels"""
    median, sigma, low, high = (F32(x) for x in stats)
    v = np.asarray(frame, F32)
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        scale = F32(10.0) / sigma
        clamped = np.where(v < low, low, np.where(v > high, high, v)).astype(F32)
        arg = (scale * (clamped - median).astype(F32)).astype(F32)
    return np.where(fin, arg, F32(0)), fin


def normalize_definition(frame, stats):
    """THE DEFINITION: the f32 rounding of the f64 asinh of the f32 argument; a non-finite pixel gives 0"""
    arg, fin = normalize_argument(frame, stats)
    return np.where(fin, np.arcsinh(arg.astype(np.float64)).astype(F32), F32(0)).astype(F32)


def normalize_definition_log1p(frame, stats):
    """the same through an independent f64 form: sign(x) * log1p(ax + ax^2 / (1 + sqrt(ax^2 + 1)))"""
    arg, fin = normalize_argument(frame, stats)
    x = arg.astype(np.float64)
    ax = np.abs(x)
    r = np.copysign(np.log1p(ax + ax * ax / (1.0 + np.sqrt(ax * ax + 1.0))), x)
    return np.where(fin, r.astype(F32), F32(0)).astype(F32)


def normalize_f32_formula(frame, stats):
    """the reference's own arithmetic: Rust's f32::asinh, ln_1p(ax + ax / (hypot(1, 1 / ax) + 1 / ax)).copysign(x), in numpy f32"""
    arg, fin = normalize_argument(frame, stats)
    ax = np.abs(arg)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ix = (F32(1.0) / ax).astype(F32)
        t = (ax / (np.hypot(F32(1.0), ix).astype(F32) + ix).astype(F32)).astype(F32)
        r = np.copysign(np.log1p((ax + t).astype(F32)).astype(F32), arg)
    return np.where(fin, r, F32(0)).astype(F32)


def frame_bytes(normalized):
    """render_grayscale's pixels (grayscale.rs:10-29) of one normalised frame, with find_minmax_simd's scalar fold (simd.rs:263-271)"""
    v = np.asarray(normalized, F32)
    fin = v[np.isfinite(v)]
    big = np.finfo(F32).max
    mn = F32(min(big, fin.min())) if fin.size else big
    mx = F32(max(-big, fin.max())) if fin.size else -big
    with np.errstate(over="ignore", invalid="ignore"):
        rng = max(F32(mx - mn), F32(1e-10))
        inv = F32(255.0) / F32(rng)
        scaled = np.clip(((v - mn).astype(F32) * inv).astype(F32), F32(0), F32(255))
        return np.where(np.isfinite(v) & (v > PADDING), scaled.astype(np.uint8), np.uint8(0)).astype(np.uint8)


def export_frames(cube, stats, frame_step: int = 1, normalize=normalize_definition):
    """export_cube_frames_sampled (eager.rs:224-246) up to the PNG encoder -> uint8 (frame_count, rows, cols)"""
    cube = np.asarray(cube, F32)
    return np.stack([frame_bytes(normalize(cube[z], stats)) for z in range(0, cube.shape[0], max(1, int(frame_step)))])


def ulp_distance(a, b):
    """distance in f32 steps between two finite arrays (the ordered-integer map of the bit patterns; +0 and -0 are 0 apart)"""
    def ordered(x):
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return np.abs(ordered(a) - ordered(b))


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
COLLAPSE_SHAPES = ((1, 1, 1), (2, 1, 77), (3, 65, 1), (5, 33, 65), (64, 7, 9), (65, 50, 50), (9, 129, 131), (257, 17, 63), (1000, 9, 70),
                   (4099, 3, 67))


def random_cube(shape, seed: int = 0):
    """signed fluxes around zero with every kind of invalid sample mixed in: exact zeros of both signs, values at and around the
    padding threshold, NaN, +-inf, and whole columns without a valid sample"""
    rng = np.random.default_rng(1000 + seed + 7 * shape[0] + shape[1] * shape[2])
    c = rng.normal(0.0, 1.0, shape).astype(F32)
    u = rng.random(shape)
    c[u < 0.05] = F32(0.0)
    c[(u >= 0.05) & (u < 0.07)] = F32(-0.0)
    c[(u >= 0.07) & (u < 0.09)] = np.nan
    c[(u >= 0.09) & (u < 0.10)] = np.inf
    c[(u >= 0.10) & (u < 0.11)] = -np.inf
    c[(u >= 0.11) & (u < 0.12)] = F32(1e-8)
    c[(u >= 0.12) & (u < 0.13)] = PADDING
    c[(u >= 0.13) & (u < 0.14)] = np.nextafter(PADDING, F32(1))
    c[:, 0, 0] = np.nan                                           # a column with no valid sample
    c[:, -1, -1] = np.where(np.arange(shape[0]) % 2 == 0, F32(0.0), F32(-np.inf))
    if shape[0] > 2:
        c[-1, -1, -1] = F32(-3.5)                                  # ... and one whose only valid sample is the cube's last voxel
    return c


ADVERSARIAL_DEPTHS = (1, 2, 3, 4, 255, 256, 257, 1000, 1001)
_POISON = np.array([np.nan, np.inf, -np.inf], F32)


def _halves(a, b):
    return lambda m: np.array([a] * (m - m // 2) + [b] * (m // 2), F32)


def _cycle(vals):
    return lambda m: np.array([vals[i % len(vals)] for i in range(m)], F32)


ADVERSARIAL_CASES = {
    "all_negative": lambda m: (-(1.0 + 0.37 * np.arange(m))).astype(F32),
    "median_below_zero": lambda m: np.concatenate([-(1.0 + np.arange(m - 2 * m // 5)), 1.0 + np.arange(2 * m // 5)]).astype(F32),
    "median_above_zero": lambda m: np.concatenate([-(1.0 + np.arange(2 * m // 5)), 1.0 + np.arange(m - 2 * m // 5)]).astype(F32),
    "low_8_bits": _halves(from_bits(0x3F800401), from_bits(0x3F8004FE)),
    "top_8_bits": _halves(from_bits(0x3F800400), from_bits(0x40800400)),
    "negative_digit_edges": _cycle([from_bits(0xBF800100), from_bits(0xBF8000FF), from_bits(0xBF810000), from_bits(0xBF80FFFF)]),
    "middle_in_two_bins": _halves(from_bits(0x3EFFFFFF), from_bits(0x3F000000)),
    "middle_across_zero": _halves(from_bits(0x80800000), from_bits(0x00800000)),
    "all_equal": lambda m: np.full(m, -7.25, F32),
    "subnormals": _cycle([from_bits(0x00000001), from_bits(0x80000001), from_bits(0x007FFFFF), from_bits(0x80000123), from_bits(0x00000100)]),
    "thresholds": _cycle([F32(0.0), F32(-0.0), F32(1e-8), PADDING, np.nextafter(PADDING, F32(1))]),
    "one_valid": None,                                            # (the LAST column: see adversarial_cube)
}


def adversarial_cube(depth: int):
    """(depth, 1, N) cube, one case of ADVERSARIAL_CASES per column, NaN / +-inf sprinkled through every column that has room for
    them (depth >= 4: every z with z % 5 == 3), the population shuffled along z.  The column at the last pixel index holds one valid
    sample, at the cube's last voxel: losing it turns that pixel's median and mean into 0."""
    names = list(ADVERSARIAL_CASES)
    cube = np.empty((depth, 1, len(names)), F32)
    rng = np.random.default_rng(depth)
    poison_at = np.arange(depth) % 5 == 3 if depth >= 4 else np.zeros(depth, bool)
    for j, name in enumerate(names):
        col = np.empty(depth, F32)
        col[poison_at] = _POISON[np.arange(int(poison_at.sum())) % 3]
        m = int((~poison_at).sum())
        if name == "one_valid":
            pop = np.array([F32(0.0), np.nan, -np.inf, F32(-0.0)], F32)[np.arange(m) % 4]
            col[~poison_at] = pop
            col[-1] = F32(-2.5)
        else:
            pop = ADVERSARIAL_CASES[name](m)
            assert pop.size == m and pop.dtype == F32
            rng.shuffle(pop)
            col[~poison_at] = pop
        cube[:, 0, j] = col
    return cube, names


# the pairs of tests/select_adversarial.py (adjacent values that differ at exactly one level of the 11/11/10 select), restated here
# so that this module stays importable on its own; test_cube_cpu.py checks them against the original
PAIRS = {"L0": (0x3F9FFFFF, 0x3FA00000), "BINADE": (0x3F7FFFFF, 0x3F800000), "L1": (0x3F8003FF, 0x3F800400), "L2": (0x3F800400, 0x3F800401),
         "TOP": (0x7F7FFFFE, 0x7F7FFFFF)}
STATS_SHAPES = ((4, 33, 65), (40, 17, 19))
BIG = 600_001


def _fill(shape, pop, seed):
    """a cube of `shape` whose voxels are `pop` shuffled, padded with invalid values of every kind"""
    n = int(np.prod(shape))
    assert pop.size <= n
    junk = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], F32)
    flat = junk[np.arange(n) % junk.size].copy()
    flat[:pop.size] = pop
    np.random.default_rng(seed).shuffle(flat)
    return flat.reshape(shape)


def stats_populations(shape):
    """[(name, cube)]: signed two- and four-valued populations whose three ranks sit on level-0, level-1 and level-2 bin edges, on
    both sides of zero; valid under both rules except where the name says otherwise"""
    n = int(np.prod(shape))
    out = []
    for i, (name, (lo, hi)) in enumerate(PAIRS.items()):
        pos = (from_bits(lo), from_bits(hi))
        neg = (from_bits(hi | 0x80000000), from_bits(lo | 0x80000000))   # (ascending: the larger magnitude first)
        m = n - n // 7
        for sign, (a, b) in (("pos", pos), ("neg", neg)):
            # the median rank on the pair's edge (half / half), then the 1 % and the 99.9 % ranks on it
            for tag, k in (("mid", m // 2), ("low", int(m * 0.01)), ("low+1", int(m * 0.01) + 1), ("high", int(m * 0.999)),
                           ("high+1", min(int(m * 0.999) + 1, m))):
                out.append((f"{name}-{sign}-{tag}", _fill(shape, np.array([a] * k + [b] * (m - k), F32), 31 * i + k)))
        q = m // 4
        four = np.array([neg[0]] * q + [neg[1]] * q + [pos[0]] * q + [pos[1]] * (m - 3 * q), F32)
        out.append((f"{name}-four", _fill(shape, four, 77 + i)))
    out.append(("one", _fill(shape, np.array([-1.5], F32), 5)))
    out.append(("none", _fill(shape, np.zeros(0, F32), 6)))
    out.append(("random", random_cube(shape, 3)))
    return out


def big_two_valued_cube():
    """a (1, 1, BIG) cube of negative values: one more `lower` than `upper`, a copy of `lower` at the first and at the last index --
    losing any one voxel moves the median to `upper`"""
    lower, upper = from_bits(PAIRS["L0"][1] | 0x80000000), from_bits(PAIRS["L0"][0] | 0x80000000)
    inner = np.array([lower] * (BIG - BIG // 2 - 2) + [upper] * (BIG // 2), F32)
    np.random.default_rng(7).shuffle(inner)
    return np.concatenate([[lower], inner, [lower]]).astype(F32).reshape(1, 1, BIG), lower, upper


def poisoned_frames_cube(shape, step):
    """a cube whose frames z % step != 0 hold only huge values that would move every statistic if a stepped pass read them"""
    c = random_cube(shape, 11)
    for z in range(shape[0]):
        if z % step:
            c[z] = F32(3e38) if z % 2 else F32(-3e38)
    return c


NORMALIZE_SHAPES = ((1, 1), (33, 65), (300, 517), (1024, 2048))


def normalize_cases(shape):
    """[(name, frame, stats)]: ordinary fluxes with NaN / inf and values outside [low, high]; a plane within a few hundred ulp of
    the median (tiny arguments, where log(x + sqrt(x^2 + 1)) loses everything); sigma = 1e-10 (huge arguments)"""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    n = shape[0] * shape[1]
    base = rng.normal(0.3, 2.0, shape).astype(F32)
    flat = base.reshape(-1)
    flat[::11] = np.nan
    flat[5::97] = np.inf
    flat[7::101] = -np.inf
    stats = (F32(0.25), F32(0.8), F32(-3.0), F32(4.5))
    median = F32(1.75)
    k = rng.integers(-300, 301, n)
    near = (bits(np.full(n, median, F32)).astype(np.int64) + k).astype(np.uint32).view(F32).reshape(shape)
    tiny_stats = (median, F32(3.0), F32(-10.0), F32(10.0))
    huge = rng.normal(0.0, 1.0, shape).astype(F32)
    huge_stats = (F32(0.0), F32(1e-10), F32(-5.0), F32(5.0))
    return [("ordinary", base, stats), ("near_median", near, tiny_stats), ("huge", huge, huge_stats)]


EXPORT_CASES = (((7, 33, 65), (1, 2, 3, 10)), ((3, 300, 517), (1,)))


def export_cube(shape):
    """fluxes with a gradient along z, invalid samples, and frame 1 entirely non-finite"""
    rng = np.random.default_rng(shape[1])
    c = (rng.normal(0.0, 1.0, shape) + 0.3 * np.arange(shape[0])[:, None, None]).astype(F32)
    c.reshape(-1)[::13] = np.nan
    c.reshape(-1)[3::211] = np.inf
    if shape[0] > 1:
        c[1] = np.where(rng.random(shape[1:]) < 0.5, np.nan, np.inf)
    return c
