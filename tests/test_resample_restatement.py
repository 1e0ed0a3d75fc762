"""The oracle's three sampler entry points (oracle/orc_sampling.c, orc_compose.c) held to an independent numpy restatement of the Rust
(tests/resample_restatement.py), BIT FOR BIT: the kernels under 46 % of the bench step are compared with the oracle everywhere else,
and oracle and kernels are by the same hand.  numpy does not fuse and the oracle is built with contraction off, so every
intermediate is the same correctly rounded f64 on both sides; the comparison includes the sign of zeros.

Also here, on the CPU: every edge case of tests/resample_cases.py populates the class it is named for (from the restatement's
coordinates), which test_gpu_resample_shapes.py asserts again next to the kernels."""
import math

import numpy as np
import pytest

import resample_cases as rc
import resample_restatement as rs


def same_bits(got, want):
    """equal values, NaN where NaN, and the same sign on zeros"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(got) & np.isnan(want)
    return bool(((got == want) | nan).all() and (np.signbit(got) == np.signbit(want))[~nan].all())


def first_difference(got, want):
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want))) | ((np.signbit(got) != np.signbit(want)) & ~np.isnan(got))
    y, x = np.argwhere(bad)[0]
    return f"{int(bad.sum())} pixels differ, first at (y={y}, x={x}): oracle {got[y, x]!r}, restatement {want[y, x]!r}"


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def test_catmull_rom_branches_and_known_values(oracle):
    ts = np.concatenate([np.linspace(-3.0, 3.0, 2401), [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, math.nextafter(1.0, 2.0), math.nextafter(1.0, 0.0),
                                                         math.nextafter(2.0, 3.0), math.nextafter(2.0, 0.0), 2.0 ** -52, 1.0 - 2.0 ** -53, 1e300,
                                                         float("inf"), float("nan")]])
    mine = rs.catmull_rom(ts)
    theirs = np.array([oracle.catmull_rom(float(t)) for t in ts])
    assert same_bits(theirs, mine)
    assert rs.catmull_rom(0.0) == 1.0 and rs.catmull_rom(1.0) == 0.0 and rs.catmull_rom(2.0) == 0.0      # sampling.rs:88-101
    assert rs.catmull_rom(0.5) == rs.catmull_rom(-0.5) == 0.5625
    assert rs.catmull_rom(float("nan")) == 0.0 and rs.catmull_rom(float("inf")) == 0.0                    # both compares fail
    # where the two branches touch both polynomials give exactly 0.0 (what lets resample.hip split the branch statically)
    assert 1.0 * 1.0 * (1.5 * 1.0 - 2.5) + 1.0 == 0.0 and 1.0 * (1.0 * (2.5 - 0.5 * 1.0) - 4.0) + 2.0 == 0.0


def test_clamp_index_and_the_saturating_convert(oracle):
    idx = np.array([-(1 << 62), -5, -1, 0, 1, 8, 9, 10, 15, 1 << 62], np.int64)
    for n in (1, 2, 10):
        assert list(rs.clamp_index(idx, n)) == [oracle.clamp_index(int(i), n) for i in idx]
    assert list(rs.clamp_index(idx, 0)) == [0] * len(idx)                                                  # boundary.rs:10-12
    v = np.array([float("nan"), 1e300, -1e300, float("inf"), -float("inf"), 2.0 ** 63, -2.0 ** 63, 2.5, -2.5, -0.0])
    assert list(rs.to_i64(v)) == [0, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, -2 ** 63, 2, -2, 0]


def test_bicubic_sample_reference_cases_and_points(oracle):
    data = np.arange(100, dtype=np.float32).reshape(10, 10)
    assert abs(float(rs.bicubic_sample(data, 3.0, 4.0)) - 34.0) < 1e-3                                      # sampling.rs:133-137
    assert abs(float(rs.bicubic_sample(np.full((8, 8), 42.0, np.float32), 3.5, 4.7)) - 42.0) < 1e-3        # :145-149
    assert float(rs.bicubic_sample(np.zeros((0, 0), np.float32), 1.0, 1.0)) == 0.0                         # :140-142
    img = rc.pattern(23, 31, nan_patch=False)
    rng = np.random.default_rng(0)
    ys = np.concatenate([rng.uniform(-4, 27, 400), [0.0, -0.0, 22.0, 21.999999999999996, -0.5, 22.5, 1e18, -1e18, float("nan")]])
    xs = np.concatenate([rng.uniform(-4, 35, 400), [0.0, -0.0, 30.0, 29.999999999999996, -0.5, 30.5, -1e18, 1e18, 3.25]])
    mine = rs.bicubic_sample(img, ys, xs)
    theirs = np.array([oracle.bicubic_sample(img, 23, 31, float(y), float(x)) for y, x in zip(ys, xs)], np.float32)
    assert same_bits(theirs, mine)


# ---- the three entry points on the edge list -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.WARP_CASES, ids=[c[0] for c in rc.WARP_CASES])
def test_oracle_warp_equals_the_restatement(oracle, case):
    name, src, t, out, _ = case
    ok, classes = rc.warp_populates(case)
    assert ok, (name, classes)
    img = rc.pattern(*src)
    theirs, mine = oracle.warp_image(img, t, *out), rs.warp_image(img, t, *out)
    assert same_bits(theirs, mine), first_difference(theirs, mine)
    band = rs.warp_image(img, t, out[0], out[1], row0=out[0] // 3, nrows=max(out[0] // 4, 1))              # the restatement's own band form
    assert same_bits(band, mine[out[0] // 3: out[0] // 3 + max(out[0] // 4, 1)])


@pytest.mark.parametrize("case", rc.SHIFT_CASES, ids=[c[0] for c in rc.SHIFT_CASES])
def test_oracle_shift_equals_the_restatement(oracle, case):
    name, src, (dy, dx), _ = case
    ok, classes = rc.shift_populates(case)
    assert ok, (name, classes)
    img = rc.pattern(*src)
    theirs, mine = oracle.shift_image_subpixel(img, dy, dx), rs.shift_image_subpixel(img, dy, dx)
    assert same_bits(theirs, mine), first_difference(theirs, mine)


@pytest.mark.parametrize("case", rc.RESAMPLE_CASES, ids=[c[0] for c in rc.RESAMPLE_CASES])
def test_oracle_resample_equals_the_restatement(oracle, case):
    name, src, dst, _ = case
    ok, classes = rc.resample_populates(case)
    assert ok, (name, classes)
    img = rc.pattern(*src)
    img[src[0] // 2, src[1] // 3] = np.nan
    theirs, mine = oracle.resample_image(img, *dst), rs.resample_image(img, *dst)
    assert same_bits(theirs, mine), first_difference(theirs, mine)


# ---- the small cases of test_gpu_resample.py and test_gpu_compose.py -------------------------------------------------------------
@pytest.mark.parametrize("dy,dx", [(0.0, 0.0), (2.0, 3.0), (0.25, -0.75), (-7.3, 5.9), (1e-13, 0.0), (0.5, 0.5), (63.6, -70.2), (200.0, 0.3)])
def test_shift_cases_of_the_gpu_suite(oracle, dy, dx):
    from test_gpu_resample import make_pattern
    img = make_pattern(97, 133)
    theirs, mine = oracle.shift_image_subpixel(img, dy, dx), rs.shift_image_subpixel(img, dy, dx)
    assert same_bits(theirs, mine), first_difference(theirs, mine)


@pytest.mark.parametrize("deg,scale,tx,ty", [(0.0, 1.0, 0.0, 0.0), (0.0, 1.0, 5.0, 3.0), (0.4, 1.0, -6.2, 4.7), (-2.0, 1.03, 3.3, -1.1),
                                              (10.0, 0.9, 20.0, -15.0), (0.0, 1.0, 1000.0, 1000.0)])
def test_warp_cases_of_the_gpu_suite(oracle, deg, scale, tx, ty):
    from test_gpu_resample import make_pattern
    img = make_pattern(120, 150) + np.random.default_rng(3).standard_normal((120, 150)).astype(np.float32)
    img[10:12, 20:40] = np.nan
    c, s = math.cos(math.radians(deg)) * scale, math.sin(math.radians(deg)) * scale
    t = (c, -s, tx, s, c, ty)
    for out_dims in [(120, 150), (100, 170)]:
        theirs, mine = oracle.warp_image(img, t, *out_dims), rs.warp_image(img, t, *out_dims)
        assert same_bits(theirs, mine), first_difference(theirs, mine)


@pytest.mark.parametrize("t", [(1.0, 0.0, float("nan"), 0.0, 1.0, 2.0), (float("inf"), 0.0, 1.0, 0.0, 1.0, 2.0), (1e200, -1e200, 3.0, 0.0, 1.0, 0.5),
                               (1.0, 0.0, 0.25, 1e-300, 1.0, 1e160), (-0.0, -0.0, -0.0, 0.0, 1.0, 0.0)],
                         ids=["nan tx", "inf a", "huge a and b cancel to nan", "ty beyond 1e150", "negative zeros"])
def test_untame_coefficients_of_the_gpu_suite(oracle, t):
    img = np.random.default_rng(4).normal(100, 10, (96, 130)).astype(np.float32)
    theirs, mine = oracle.warp_image(img, t, 96, 130), rs.warp_image(img, t, 96, 130)
    assert same_bits(theirs, mine), first_difference(theirs, mine)


@pytest.mark.parametrize("src,dst", [((100, 100), (100, 100)), ((200, 200), (100, 100)), ((50, 50), (100, 100)), ((37, 53), (80, 31)),
                                     ((301, 517), (1024, 777)), ((1024, 1024), (130, 4096))])
def test_resample_cases_of_the_gpu_suite(oracle, src, dst):
    img = np.random.default_rng(src[0] + dst[1]).uniform(-1, 2, src).astype(np.float32)
    img[src[0] // 2, src[1] // 3] = np.nan
    theirs, mine = oracle.resample_image(img, *dst), rs.resample_image(img, *dst)
    assert same_bits(theirs, mine), first_difference(theirs, mine)


def test_chunking_changes_nothing(monkeypatch):
    """the row chunks are an implementation detail of the restatement: one chunk and many give the same plane"""
    img = rc.pattern(97, 141)
    t = rc.about_centre(10.0, 0.9, (97, 141), (160, 230))
    whole = (rs.warp_image(img, t, 160, 230), rs.shift_image_subpixel(img, 0.25, -0.75), rs.resample_image(img, 83, 311))
    monkeypatch.setattr(rs, "CHUNK_PIXELS", 1000)
    parts = (rs.warp_image(img, t, 160, 230), rs.shift_image_subpixel(img, 0.25, -0.75), rs.resample_image(img, 83, 311))
    for a, b in zip(whole, parts):
        assert same_bits(a, b)


def test_resample_rejects_empty_targets():
    with pytest.raises(ValueError, match="Target dimensions must be > 0"):
        rs.resample_image(np.zeros((4, 4), np.float32), 0, 5)
