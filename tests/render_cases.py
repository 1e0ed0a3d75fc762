"""The renderers' edge cases, shared by test_render_restatement_cpu.py (oracle against the numpy restatement, CPU) and
test_gpu_render_adversarial.py (library against the restatement, GPU).  Every fixture names the edge it is there for and carries a
predicate, computed from the RESTATEMENT (render_restatement.py), that must hold -- so that a case cannot silently test nothing.
The predicates are asserted by test_render_restatement_cpu.py::test_every_fixture_populates_its_edge."""
import functools
import struct
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import render_restatement as R

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
CUT = R.CUT
CUT_NEXT = np.nextafter(CUT, F32(1.0))

# the STF of test_gpu_render.py: three different transforms, so that a swapped channel shows
STF = [(0.10, 0.30, 1.0), (0.0, 0.5, 1.0), (0.2, 0.2, 0.9)]
STATS = [dict(min=-0.2, max=1.2, median=0.4 + 0.05 * c, mad=0.1, sigma=0.15, mean=0.5, valid_count=1000) for c in range(3)]
STATS_NS = [SimpleNamespace(**s) for s in STATS]


def _ro(a):
    a.setflags(write=False)
    return a


# ---- quantisation ties ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_values():
    """for every k in 0..254 an f32 v with f32(v * 255f) == k + 0.5 EXACTLY -> (255,) f32"""
    out = []
    for k in range(255):
        v = F32((k + 0.5) / 255.0)
        cands = [v]
        lo = hi = v
        for _ in range(4):
            lo, hi = np.nextafter(lo, F32(-1.0)), np.nextafter(hi, F32(2.0))
            cands += [lo, hi]
        hit = [c for c in cands if F32(c * F32(255.0)) == F32(k + 0.5)]
        assert hit, k
        out.append(hit[0])
    return _ro(np.array(out, F32))


SPECIALS = np.array([-0.0, 0.0, 1.0, np.nextafter(F32(1.0), F32(0.0)), np.nextafter(F32(1.0), F32(2.0)), F32(1.0) / F32(255.0),
                     F32(254.5) / F32(255.0), np.nan, np.inf, -np.inf, 1e-45, -1e-30, 3e38, 0.5], F32)


@functools.lru_cache(maxsize=None)
def quantisation_values():
    """each tie with its two f32 neighbours, then the specials -> (779,) f32"""
    t = tie_values()
    return _ro(np.concatenate([np.stack([np.nextafter(t, F32(-1.0)), t, np.nextafter(t, F32(2.0))], axis=1).ravel(), SPECIALS]).astype(F32))


QUANT_SHAPE = (19, 41)   # 779 = 19 x 41: odd in both directions, ph * pw % 4 == 3


@functools.lru_cache(maxsize=None)
def quantisation_planes():
    """r: the values in order; g: reversed; b: rotated by 257 -- a channel mix-up cannot cancel"""
    v = quantisation_values()
    assert v.size == QUANT_SHAPE[0] * QUANT_SHAPE[1]
    return tuple(_ro(np.ascontiguousarray(x.reshape(QUANT_SHAPE))) for x in (v, v[::-1], np.roll(v, 257)))


def quantisation_populates():
    """at least one byte differs between truncation and rounding for EVERY k (truncation gives k, rounding k + 1)"""
    t = tie_values()
    tr, ro = R.u8_truncated(t), R.u8_rounded(t)
    exact = bool((t * F32(255.0) == np.arange(255, dtype=F32) + F32(0.5)).all())
    return exact and bool((tr == np.arange(255)).all() and (ro == np.arange(255) + 1).all())


# ---- mono tile ties ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mono_tie_plane():
    """64 x 64 with restated bounds exactly (1.0, 256.0), so inv_range == 1.0f and (v - gmin) * inv_range puts every k + 0.5 on a tie"""
    rng = np.random.default_rng(11)
    invalid = [NAN, INF, -INF, 0.0, -5.0, CUT]                                     # not counted: non-finite or <= 1e-7
    n_valid = 64 * 64 - len(invalid)                                               # 4090: ranks floor(4.09) = 4, floor(4085.91) = 4085
    below, above = [0.25, 0.5], [300.0, 1000.0]                                    # sorted ranks 0..1 and 4088..4089
    ties = [k + 0.5 for k in range(1, 256)]
    filler = rng.integers(5, 1023, n_valid - len(below) - len(above) - 10 - len(ties)) * 0.25   # in (1, 256), multiples of 0.25
    vals = np.array(invalid + below + [1.0] * 5 + ties + list(filler) + [256.0] * 5 + above, F32)
    assert vals.size == 64 * 64
    return _ro(rng.permutation(vals).reshape(64, 64))


def mono_tie_populates():
    a = mono_tie_plane()
    lo, hi = R.percentile_bounds(a)
    valid = np.sort(R.valid_pixels(a))
    lo_idx, hi_idx = R.percentile_ranks(valid.size, 0.001, 0.999)
    around = bool((valid[lo_idx - 2:lo_idx + 3] == 1.0).all() and (valid[hi_idx - 2:hi_idx + 3] == 256.0).all())
    ties = all((a == F32(k + 0.5)).any() for k in range(1, 256))
    outside = bool((valid < 1.0).any() and (valid > 256.0).any() and np.isnan(a).any() and np.isinf(a).any())
    inv_range = F32(255.0) / max(F32(hi - lo), F32(1e-10))
    return (lo, hi) == (1.0, 256.0) and inv_range == F32(1.0) and around and ties and outside


@functools.lru_cache(maxsize=None)
def mono_inexact_plane():
    """a range that is no power of two: inv_range is rounded"""
    rng = np.random.default_rng(12)
    a = rng.gamma(2.0, 0.1, (64, 64)).astype(F32)
    a[rng.random(a.shape) < 0.02] = NAN
    a[:, :2] = 0.0
    return _ro(a)


@functools.lru_cache(maxsize=None)
def mono_flat_plane():
    """gmax == gmin: range = 1e-10"""
    a = np.full((64, 64), 0.5, F32)
    a[3, 5], a[60, 1] = NAN, -INF
    return _ro(a)


MONO_PLANES = [("ties: bounds (1, 256), inv_range 1", mono_tie_plane, mono_tie_populates),
               ("inexact range", mono_inexact_plane,
                lambda: (lambda lo, hi: 255.0 / float(F32(hi - lo)) != float(F32(255.0) / F32(hi - lo)))(*R.percentile_bounds(mono_inexact_plane()))),
               ("flat: range below 1e-10", mono_flat_plane,
                lambda: (lambda lo, hi: lo == hi == 0.5)(*R.percentile_bounds(mono_flat_plane())))]
MONO_TS = 16   # 64 x 64 at ts = 16: three levels


# ---- preview geometry -------------------------------------------------------------------------------------------------------------
# (rows, cols, max_dim, (ph, pw) worked out by hand, what it is there for, d * ratio on exact integers: True / None = not asked)
GEOMETRY = [
    (5, 10, 5, (3, 5), "2.5 rounds up (half away from zero)", None),
    (3, 8, 4, (2, 4), "1.5 rounds up", None),
    (7, 2, 1, (1, 1), "0.2857 rounds to 0, then max(1)", None),
    (1000, 10, 100, (100, 1), "a preview one column wide", True),
    (40, 3, 39, (39, 3), "fewer than four columns: a lane spans two rows", None),
    (41, 2, 40, (40, 2), "two columns: a lane spans two or three rows", None),
    (37, 53, 53, (37, 53), "fits: ratio 1", None),
    (37, 53, 52, (36, 52), "scale just below 1", None),
    (300, 100, 100, (100, 33), "d * ratio lands on integers (y ratio 3)", True),
    (999, 333, 111, (111, 37), "d * ratio lands on integers (both ratios 9)", True),
    (1000, 7, 300, (300, 2), "an inexact ratio", None),
    (1, 301, 50, (1, 50), "one row", None),
    (301, 1, 50, (50, 1), "one column", None),
]
GEOMETRY_IDS = [f"{r}x{c}@{m}" for r, c, m, *_ in GEOMETRY]
# ph * pw % 4 per case, by hand (15, 8, 1, 100, 117, 80, 1961, 1872, 3300, 4107, 600, 50, 50 pixels): the last lane of
# preview_rgb_kernel (4 pixels per lane) holds 3, 4, 1, 4, 1, 4, 1, 4, 4, 3, 4, 2, 2 pixels
GEOMETRY_MOD4 = [3, 0, 1, 0, 1, 0, 1, 0, 0, 3, 0, 2, 2]


def geometry_populates(case):
    rows, cols, max_dim, dims, _, integers = case
    ph, pw, yr, xr = R.preview_dims(rows, cols, max_dim)
    ok = (ph, pw) == dims and (ph * pw) % 4 == GEOMETRY_MOD4[GEOMETRY.index(case)]
    if integers:
        ok = ok and R.lands_on_integers(rows, cols, max_dim)
    if (rows, cols, max_dim) == (1000, 7, 300):
        ok = ok and Fraction(yr) != Fraction(rows, ph) and Fraction(xr) == Fraction(cols, pw)
    if (rows, cols, max_dim) == (37, 53, 52):
        ok = ok and 1.0 < yr < 1.03 and 1.0 < xr < 1.03
    return ok


def last_lane_pixels():
    """pixels in the last lane of preview_rgb_kernel (4 per lane) over the geometry list: all of 1, 2, 3, 4 must occur"""
    return {((ph * pw - 1) % 4) + 1 for _, _, _, (ph, pw), _, _ in GEOMETRY} | {((QUANT_SHAPE[0] * QUANT_SHAPE[1] - 1) % 4) + 1}


@functools.lru_cache(maxsize=None)
def index_planes(rows, cols):
    """three planes whose truncated bytes spell the source index (r: low byte, g: next, b: high), so a wrong source pixel shows"""
    i = np.arange(rows * cols).reshape(rows, cols)
    return tuple(_ro(((((i >> s) & 255) + 0.5) / 255.0).astype(F32)) for s in (0, 8, 16))


@functools.lru_cache(maxsize=None)
def index_plane(rows, cols):
    """one f32 plane for the IPC buffer: the source index plus a fraction, with a NaN, an inf and a -0.0"""
    a = (np.arange(rows * cols, dtype=np.float64) * 1.25 - 17.0).astype(F32).reshape(rows, cols).copy()
    flat = a.reshape(-1)
    flat[flat.size // 2] = NAN
    flat[flat.size // 3] = INF
    flat[-1] = F32(-0.0)
    return _ro(a)


# ---- downsample -------------------------------------------------------------------------------------------------------------------
def _from_cells(cells, per_row):
    """2 x 2 cells [a, b, c, d] -> a plane of them, per_row cells to a row"""
    rows = []
    for s in range(0, len(cells), per_row):
        row = cells[s:s + per_row]
        rows.append(np.concatenate([np.array(c, F32).reshape(2, 2) for c in row], axis=1))
    return _ro(np.concatenate(rows, axis=0))


SUB = F32(1e-45)   # the smallest subnormal
DOWNSAMPLE_CELLS = [
    [1e30, 1.0, -1e30, 1.0],            # sequential: ((1e30 + 1) - 1e30) + 1 = 1 -> 0.25; pairwise: (1e30 + 1) + (-1e30 + 1) = 0
    [3.4e38, 3.4e38, 3.4e38, 3.4e38],   # the f64 sum passes f32::MAX; the mean comes back
    [NAN, 2.0, 3.0, 5.0], [NAN, INF, 3.0, 5.0], [NAN, INF, -INF, 5.0], [NAN, INF, -INF, NAN],   # 1..4 non-finite members; all four: 0.0
    [SUB, SUB, SUB, 0.0], [SUB, -SUB, 3 * SUB, 2 * SUB], [-0.0, -0.0, -0.0, -0.0], [1.0, 1e30, 1.0, -1e30],
    [16777216.0, 1.0, 1.0, 1.0], [0.1, 0.2, 0.3, NAN],
]


@functools.lru_cache(maxsize=None)
def downsample_planes():
    rng = np.random.default_rng(21)
    out = [("the named cells", _from_cells(DOWNSAMPLE_CELLS, 4))]
    for shape in [(1, 1), (1, 9), (9, 1), (2, 2), (5, 5), (257, 3)]:
        a = (rng.normal(0, 1, shape) * 10.0 ** rng.integers(-3, 30, shape)).astype(F32)
        a[rng.random(shape) < 0.1] = NAN
        a[rng.random(shape) < 0.05] = INF
        out.append((f"{shape[0]}x{shape[1]}", _ro(a)))
    return out


def downsample_populates():
    cells = downsample_planes()[0][1]
    seq, pair = R.downsample_2x(cells), R.downsample_2x_pairwise(cells)
    return bool(seq[0, 0] == F32(0.25) and pair[0, 0] == 0.0 and seq[0, 1] == F32(3.4e38) and seq[1, 1] == 0.0 and (seq != pair).any())


# ---- percentile bounds ------------------------------------------------------------------------------------------------------------
PCT_PAIRS = [(0.0, 1.0), (1.0, 0.0), (0.5, 0.5), (-0.25, 0.999), (float("nan"), float("nan")), (0.001, 1e30), (1.5, 2.0), (0.001, 0.999)]
PCT_IDS = ["0,1", "1,0", "0.5,0.5", "-0.25,0.999", "nan,nan", "0.001,1e30", "1.5,2", "0.001,0.999"]
# "-0.25,0.999", "nan,nan" and "0.001,1e30": n * pct is outside usize and a plain C cast of it is undefined.  Measured on x86-64 with
# gcc, -0.25 and NaN gave rank n - 1 (the reference: 0) and 1e30 gave rank 0 (the reference: n - 1): the cases that fail without the
# saturating conversion


def _counted(n, seed):
    """n distinct valid values in shuffled order among five invalid pixels"""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([(np.arange(1, n + 1) * 0.001).astype(F32), np.array([0.0, -1.0, np.nan, np.inf, CUT], F32)])
    return _ro(rng.permutation(vals).reshape(1, -1))


# the plane on which find_minmax_simd's two branches differ: the infinities sit in the one whole chunk of eight, the remainder is finite
AVX2_PLANE = _ro(np.array([[0.0, -2.0, np.inf, np.nan, -np.inf, 1e-8, 0.0, 0.0, -3.0, np.inf]], F32))

# (id, plane, predicate over the plane)
PERCENTILE_PLANES = [
    ("f32(1e-7) excluded, its successor included", _ro(np.array([[CUT, CUT_NEXT, CUT, 0.0, -1.0]], F32)),
     lambda a: list(R.valid_pixels(a)) == [CUT_NEXT] and CUT_NEXT > CUT),
    ("every pixel invalid but finite", _ro(np.array([[0.0, -2.0, -0.5, 1e-8, CUT], [0.0, -1e-30, 0.0, 0.0, 0.0]], F32)),
     lambda a: R.valid_pixels(a).size == 0 and R.percentile_bounds(a) == (-2.0, CUT)),
    ("every pixel non-finite", _ro(np.array([[np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]], F32)),
     lambda a: R.percentile_bounds(a) == (R.F32_MAX, -R.F32_MAX)),
    ("the two fallback branches differ", AVX2_PLANE,
     lambda a: R.valid_pixels(a).size == 0 and R.find_minmax_portable(a) == (-3.0, F32(1e-8)) and R.find_minmax_avx2(a) == (-np.inf, np.inf)),
    ("n = 1", _counted(1, 1), lambda a: R.valid_pixels(a).size == 1),
    ("n = 2", _counted(2, 2), lambda a: R.valid_pixels(a).size == 2),
    ("n = 999: 999 * 0.001 == 0.999", _counted(999, 3), lambda a: R.valid_pixels(a).size == 999 and 999 * 0.001 == 0.999),
    ("n = 1000: 1000 * 0.999 == 999.0", _counted(1000, 4),
     lambda a: R.valid_pixels(a).size == 1000 and 1000 * 0.999 == 999.0 and R.percentile_ranks(1000, 0.001, 0.999) == (1, 999)),
    ("n = 1001", _counted(1001, 5), lambda a: R.valid_pixels(a).size == 1001 and R.percentile_ranks(1001, 0.001, 0.999) == (1, 999)),
    ("four distinct values repeated: ranks land on ties",
     _ro(np.random.default_rng(6).permutation(np.tile(np.array([0.25, 0.5, 0.75, 1.0], F32), 250)).reshape(25, 40)),
     lambda a: np.unique(a).size == 4 and R.percentile_bounds(a, 0.25, 0.5) == (0.5, 0.75) and R.percentile_bounds(a, 0.5, 0.5) == (0.75, 0.75)),
]


def saturating_ranks_populate():
    """the ranks the reference's saturating conversion gives at m = 1000"""
    return (R.percentile_ranks(1000, -0.25, 0.999) == (0, 999) and R.percentile_ranks(1000, float("nan"), float("nan")) == (0, 0)
            and R.percentile_ranks(1000, 0.001, 1e30) == (1, 999) and R.percentile_ranks(1000, 1.5, 2.0) == (999, 999))


# ---- IPC --------------------------------------------------------------------------------------------------------------------------
def _hdr(buf):
    return struct.unpack("<IIff", buf[:16])


def _px(buf):
    return np.frombuffer(buf[16:], "<f4")


def _a(rows):
    return _ro(np.array(rows, F32))


_unsampled = np.arange(1, 33, dtype=F32).reshape(4, 8).copy()
_unsampled[1, 1] = -5.0
_nan_sampled = np.arange(1, 33, dtype=F32).reshape(4, 8).copy()
_nan_sampled[2, 4] = NAN

# (id, plane, max_dim, predicate over the restated buffer, header compared by value only)
IPC_CASES = [
    ("all non-finite, full: header (w, h, 0, 1)", _ro(np.full((5, 7), np.nan, F32)), 0,
     lambda b: _hdr(b) == (7, 5, 0.0, 1.0) and not _px(b).any(), False),
    ("all non-finite, downsampled: the cleaned zeros are the range", _a([[NAN, INF] * 4] * 4), 4,
     lambda b: _hdr(b) == (4, 2, 0.0, 0.0), False),
    ("-0.0 pixels keep their bytes, full", _a([[-0.0, 1.0, -2.0], [0.0, -0.0, 3.0]]), 0,
     lambda b: _hdr(b) == (3, 2, -2.0, 3.0) and list(np.signbit(_px(b))) == [True, False, True, False, True, False], False),
    ("-0.0 pixels keep their bytes, downsampled", _a([[-0.0, 9.0, -2.0, 9.0], [9.0] * 4, [0.0, 9.0, 4.0, 9.0], [9.0] * 4]), 2,
     lambda b: _hdr(b) == (2, 2, -2.0, 4.0) and list(np.signbit(_px(b))) == [True, True, False, False], False),
    ("both zeros and the minimum is zero: header by value", _a([[0.0, -0.0, 2.0, 0.0, -0.0, 1.0, -0.0]]), 0,
     lambda b: _hdr(b)[2:] == (0.0, 2.0) and np.signbit(_px(b)).sum() == 3, True),
    ("both zeros and the maximum is zero: header by value", _a([[-0.0, 0.0, -2.0], [0.0, -0.0, -1.0]]), 0,
     lambda b: _hdr(b)[2:] == (-2.0, 0.0) and np.signbit(_px(b)).sum() == 4, True),
    ("downsampled: the only negative value is not sampled", _ro(_unsampled), 4,
     lambda b: _hdr(b) == (4, 2, 1.0, 23.0) and not (_px(b) < 0).any(), False),
    ("downsampled: a sampled NaN's cleaned 0.0 is the minimum", _ro(_nan_sampled), 4,
     lambda b: _hdr(b) == (4, 2, 0.0, 23.0) and (_px(b) == 0).sum() == 1, False),
    ("full: a NaN is not the minimum", _ro(_nan_sampled), 0, lambda b: _hdr(b) == (8, 4, 1.0, 32.0) and (_px(b) == 0).sum() == 1, False),
    ("more than one 65536-pixel chunk", lambda: index_plane(300, 290), 0, lambda b: _hdr(b)[:2] == (290, 300) and _hdr(b)[2] == -17.0, False),
]
IPC_CASES += [(f"geometry {i}", functools.partial(index_plane, c[0], c[1]), c[2],
               (lambda dims: lambda b: _hdr(b)[:2] == (dims[1], dims[0]))(c[3]), False) for i, c in zip(GEOMETRY_IDS, GEOMETRY)]
IPC_IDS = [c[0] for c in IPC_CASES]


def ipc_plane(case):
    return case[1]() if callable(case[1]) else case[1]


# ---- pyramids ---------------------------------------------------------------------------------------------------------------------
# (rows, cols, ts, levels and padded tiles worked out by hand, what it is there for)
PYRAMIDS = [
    (64, 64, 64, 1, 0, "an exact multiple of ts: one full tile"),
    (128, 64, 64, 2, 1, "an exact multiple of ts, two levels"),
    (65, 65, 64, 2, 4, "one pixel over: 1-pixel sliver tiles in both directions"),
    (63, 32, 31, 3, 7, "odd ts (byte stores only), one pixel over in both directions"),
    (20, 30, 256, 1, 1, "smaller than ts"),
    (257, 300, 256, 2, 4, "ts = 256, one row over"),
    (1, 300, 16, 6, 40, "one row"),
    (300, 1, 16, 6, 40, "one column"),
    (257, 129, 2, 9, 390, "nine levels, odd sizes at most of them, many workspace ping-pongs"),
    (5, 7, 1024, 1, 1, "one tile, many slices per tile"),
    (5, 7, 1, 4, 0, "ts = 1: every pixel its own tile"),
    (10, 10, 3, 3, 10, "ts = 3: tile buffers that start on odd addresses"),
]
PYRAMID_IDS = [f"{r}x{c}/ts{t}" for r, c, t, *_ in PYRAMIDS]


def pyramid_populates(case):
    rows, cols, ts, nl, padded, _ = case
    levels, _ = R.pyramid_layout(rows, cols, ts, 1)
    return len(levels) == nl and R.pyramid_padded_tiles(rows, cols, ts) == padded


@functools.lru_cache(maxsize=None)
def rgb_planes(rows, cols):
    """noise over [-0.2, 1.2] with the quantisation values (ties, specials) written over the start of every channel"""
    rng = np.random.default_rng(rows * 1000 + cols)
    q = quantisation_values()
    out = []
    for c in range(3):
        a = rng.uniform(-0.2, 1.2, rows * cols).astype(F32)
        k = min(a.size, q.size)
        a[:k] = np.roll(q, 101 * c)[:k]
        out.append(_ro(rng.permutation(a).reshape(rows, cols)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mono_plane(rows, cols):
    """the tie plane's population (bounds (1, 256) when the plane is large enough to hold it), any shape"""
    rng = np.random.default_rng(rows * 1000 + cols + 7)
    src = mono_tie_plane().ravel()
    a = src[rng.integers(0, src.size, rows * cols)].copy()
    if a.size >= 16:
        a[:6] = [NAN, INF, 0.0, 1.0, 256.0, 1.5]
    return _ro(a.reshape(rows, cols))


# ---- level arithmetic (host only) -------------------------------------------------------------------------------------------------
LEVEL_ARGS = [(m, ts) for ts in (1, 3, 256) for k in range(0, 32) for m in (2 ** k - 1, 2 ** k, 2 ** k + 1) if m >= 1]
