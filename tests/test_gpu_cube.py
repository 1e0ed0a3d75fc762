"""HIP parity of the spectral-cube entry points (csrc/cube.hip, and plane_select.hip's cube form) on one MI355X against the numpy
restatement of core/cube/{eager,lazy}.rs (tests/cube_restatement.py).

Collapse and global statistics: bit for bit, through uint32 views.  Normalisation: within 1 f32 ulp of the definition (the f32
rounding of the f64 asinh) and bit-identical except for at most 2 values per 2^21 -- double rounding is expected at about 2e-9 per
value, an f32-libm asinh differs on several per cent, the naive log form fails on the near-median plane.  Export: frame count and
layout exact, every byte within one level, at most 1e-5 of the bytes unequal.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cube_restatement as R
from astroburst_amd import AstroBurstError

pytestmark = pytest.mark.gpu

F32 = np.float32
RULES = (R.NONZERO, R.ABOVE_PADDING)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_bits(got, want, what):
    got, want = _host(got), np.asarray(want, F32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: got {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def _collapse_reference(shape):
    cube = R.random_cube(shape)
    return cube, {rule: (R.collapse_mean(cube, rule), R.collapse_median(cube, rule)) for rule in RULES}


# ---- collapse ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.COLLAPSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_collapse_matches_bit_for_bit(ctx, shape):
    cube, want = _collapse_reference(shape)
    dcube = _dev(cube)
    for rule in RULES:
        mean, median = want[rule]
        assert_bits(ctx.collapse_mean(cube, rule), mean, f"mean host rule {rule}")
        assert_bits(ctx.collapse_median(cube, rule), median, f"median host rule {rule}")
        assert_bits(ctx.collapse_mean(dcube, rule), mean, f"mean device rule {rule}")
        assert_bits(ctx.collapse_median(dcube, rule), median, f"median device rule {rule}")


# The median workgroup takes 16, 8 or 4 waves by the number of 64-pixel groups (under 2, under 4, from 4 per CU of a 256-CU part) and
# halves them while 4 x waves exceeds the depth: 20 and 40 planes of a small plane give 4 and 8 waves, as do the two large planes.
WAVE_FORM_SHAPES = ((20, 5, 7), (40, 5, 7), (33, 129, 256), (17, 257, 256))


@pytest.mark.parametrize("shape", WAVE_FORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_collapse_median_four_and_eight_wave_forms(ctx, shape):
    cube = R.random_cube(shape, 3)
    dcube = _dev(cube)
    for rule in RULES:
        assert_bits(ctx.collapse_median(dcube, rule), R.collapse_median(cube, rule), f"median rule {rule}")
        assert_bits(ctx.collapse_mean(dcube, rule), R.collapse_mean(cube, rule), f"mean rule {rule}")


@pytest.mark.parametrize("depth", R.ADVERSARIAL_DEPTHS)
def test_collapse_adversarial_columns(ctx, depth):
    cube, names = R.adversarial_cube(depth)
    dcube = _dev(cube)
    for rule in RULES:
        median, mean = _host(ctx.collapse_median(dcube, rule)), _host(ctx.collapse_mean(dcube, rule))
        want_median, want_mean = R.collapse_median(cube, rule), R.collapse_mean(cube, rule)
        for j, name in enumerate(names):
            assert R.bits(median)[0, j] == R.bits(want_median)[0, j], f"median of {name} at depth {depth} rule {rule}: {median[0, j]!r} != {want_median[0, j]!r}"
            assert R.bits(mean)[0, j] == R.bits(want_mean)[0, j], f"mean of {name} at depth {depth} rule {rule}"
    assert_bits(ctx.collapse_median(cube, R.NONZERO), R.collapse_median(cube, R.NONZERO), "host cube")


# ---- global statistics ------------------------------------------------------------------------------------------------------------
def _check_stats(ctx, cube, rule, step, what):
    (median, sigma, low, high), n = R.global_stats(_host(cube), rule, step)
    g, count = ctx.compute_global_stats(cube, rule, step, want_count=True)
    got = np.array([g.median, g.sigma, g.low, g.high], F32)
    want = np.array([median, sigma, low, high], F32)
    assert count == n, f"{what}: count {count} != {n}"
    assert (R.bits(got) == R.bits(want)).all(), f"{what}: got {got!r} want {want!r}"


@pytest.mark.parametrize("shape", R.STATS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_global_stats_on_bin_edges(ctx, shape):
    steps = (1, 3, R.streaming_step(shape[0]))
    for name, cube in R.stats_populations(shape):
        dcube = _dev(cube)
        for step in steps:
            for rule in RULES:
                _check_stats(ctx, dcube if step == 1 else cube, rule, step, f"{name} step {step} rule {rule}")
                if step == 1:
                    _check_stats(ctx, cube, rule, step, f"{name} host rule {rule}")


# The histogram kernel puts the frames along grid.y, at most 8 x CU count (2048) rows of blocks, and strides the rest: only a cube
# deeper than that -- the JWST-like eager case -- runs the stride.  4099 frames take it twice and leave a ragged third round.
@pytest.mark.parametrize("shape", ((2100, 1, 3), (4099, 3, 67)), ids=lambda s: "x".join(map(str, s)))
def test_global_stats_deeper_than_the_grid(ctx, shape):
    cube = R.random_cube(shape, 11)
    cube[-1] = F32(-7.5)                                                  # a last frame whose loss changes the count, the median and `low`
    dcube = _dev(cube)
    for rule in RULES:
        for step in (1, 2, R.streaming_step(shape[0])):
            _check_stats(ctx, dcube, rule, step, f"deep {shape} step {step} rule {rule}")
    _check_stats(ctx, cube, R.NONZERO, 1, f"deep {shape} host")


def test_global_stats_streaming_wrapper_and_defaults(ctx):
    cube = R.random_cube((40, 17, 19), 5)
    (median, sigma, low, high), n = R.global_stats(cube, R.ABOVE_PADDING, R.streaming_step(40))
    g, count = ctx.compute_global_stats_streaming(_dev(cube), want_count=True)
    assert count == n and (R.bits(np.array([g.median, g.sigma, g.low, g.high], F32)) == R.bits(np.array([median, sigma, low, high], F32))).all()
    g, count = ctx.compute_global_stats(np.zeros((3, 5, 7), F32), want_count=True)
    assert count == 0 and (g.median, g.sigma, g.low, g.high) == (0.0, 1.0, 0.0, 1.0)
    _check_stats(ctx, np.array([np.nan, 0.0, -1.5, np.inf], F32).reshape(4, 1, 1), R.NONZERO, 1, "n = 1")


def test_global_stats_big_cube_loses_no_voxel(ctx):
    big, lower, upper = R.big_two_valued_cube()
    _check_stats(ctx, _dev(big), R.NONZERO, 1, "big")
    assert ctx.compute_global_stats(big).median == lower


def test_global_stats_stepping_skips_poisoned_frames(ctx):
    for shape, step in (((40, 17, 19), 3), ((40, 17, 19), R.streaming_step(40) + 1), ((4, 33, 65), 3)):
        cube = R.poisoned_frames_cube(shape, step)
        for rule in RULES:
            _check_stats(ctx, _dev(cube), rule, step, f"poisoned {shape} step {step} rule {rule}")
            assert ctx.compute_global_stats(cube, rule, step).high < 1e30


# ---- normalisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.NORMALIZE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_normalize_against_the_definition(ctx, shape):
    for name, frame, stats in R.normalize_cases(shape):
        want = R.normalize_definition(frame, stats)
        other = R.normalize_definition_log1p(frame, stats)
        cap = 2 * max(1, -(-want.size // (1 << 21)))
        assert int((R.bits(want) != R.bits(other)).sum()) <= cap, f"{name}: the two f64 forms of the definition disagree"
        outs = {"device": _host(ctx.normalize_with_global(_dev(frame), stats))}
        if shape[0] <= 300:
            outs["host"] = ctx.normalize_with_global(frame, stats)
        for kind, got in outs.items():
            assert np.isfinite(got).all()
            assert (got[~np.isfinite(frame)] == 0).all(), f"{name} {kind}: a non-finite pixel must give 0"
            d = R.ulp_distance(got, want)
            differ = int((R.bits(got) != R.bits(want)).sum())
            print(f"{name} {shape} {kind}: max {int(d.max())} ulp, {differ} of {want.size} not bit-identical")
            assert d.max() <= 1, f"{name} {kind}: {int(d.max())} ulp from the definition"
            assert differ <= cap, f"{name} {kind}: {differ} values of {want.size} are not bit-identical (cap {cap})"


# ---- export -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,steps", R.EXPORT_CASES, ids=lambda v: "x".join(map(str, v)))
def test_export_frames(ctx, shape, steps):
    cube = R.export_cube(shape)
    stats, _ = R.global_stats(cube, R.NONZERO)
    dcube = _dev(cube)
    for step in steps:
        want = R.export_frames(cube, stats, step)
        for kind, got in (("host", ctx.export_cube_frames(cube, stats, step)), ("device", _host(ctx.export_cube_frames(dcube, stats, step)))):
            assert got.dtype == np.uint8 and got.shape == want.shape == (-(-shape[0] // step),) + shape[1:], f"{kind} step {step}"
            diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
            print(f"export {shape} step {step} {kind}: {int((diff > 0).sum())} of {diff.size} bytes unequal, max {int(diff.max())}")
            assert diff.max() <= 1
            assert (diff > 0).sum() <= 1e-5 * diff.size
            if step == 1 and shape[0] > 1:
                assert got[1].max() == 0, "an entirely non-finite frame renders black"
            assert got[0].max() >= 254 and want[0].max() >= 254


# ---- spectrum ---------------------------------------------------------------------------------------------------------------------
def test_extract_spectrum(ctx):
    cube = R.random_cube((65, 50, 50), 9)
    dcube = _dev(cube)
    for y, x in ((0, 0), (0, 49), (49, 0), (49, 49), (25, 25)):
        assert_bits(ctx.extract_spectrum(cube, y, x), cube[:, y, x], f"host ({y}, {x})")
        assert_bits(ctx.extract_spectrum(dcube, y, x), cube[:, y, x], f"device ({y}, {x})")
    for src in (cube, dcube):
        for y, x in ((50, 0), (0, 50), (-1, 3)):
            with pytest.raises(AstroBurstError, match=rf"Pixel \({y}, {x}\) out of bounds"):
                ctx.extract_spectrum(src, y, x)


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    from astroburst_amd import _lib
    L, h = ctx._L, ctx._h
    cube = np.ones((3, 4, 5), F32)
    out = np.zeros((4, 5), F32)
    pc = _lib.CubeC(C.c_void_p(cube.ctypes.data), 3, 4, 5, 0)
    po = _lib.Plane(C.c_void_p(out.ctypes.data), 4, 5, 0)
    st, n64, i64 = _lib.CubeStatsC(0.0, 1.0, 0.0, 1.0), C.c_uint64(0), C.c_int64(0)
    invalid = _lib.AB_ERR_INVALID
    for fn in (L.ab_cube_collapse_mean, L.ab_cube_collapse_median):
        assert fn(h, None, 0, C.byref(po)) == invalid and fn(h, C.byref(pc), 0, None) == invalid and fn(None, C.byref(pc), 0, C.byref(po)) == invalid
        assert fn(h, C.byref(pc), 2, C.byref(po)) == invalid                                  # unknown rule
        for dims in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
            assert fn(h, C.byref(_lib.CubeC(C.c_void_p(cube.ctypes.data), *dims, 0)), 0, C.byref(po)) == invalid
        assert fn(h, C.byref(_lib.CubeC(None, 3, 4, 5, 0)), 0, C.byref(po)) == invalid
        assert fn(h, C.byref(pc), 0, C.byref(_lib.Plane(C.c_void_p(out.ctypes.data), 5, 4, 0))) == invalid   # wrong out dims
    assert L.ab_cube_global_stats(h, None, 0, 1, C.byref(st), C.byref(n64)) == invalid
    assert L.ab_cube_global_stats(h, C.byref(pc), 0, 1, None, C.byref(n64)) == invalid
    assert L.ab_cube_global_stats(h, C.byref(pc), 0, 1, C.byref(st), None) == _lib.AB_OK       # count is nullable
    pin = _lib.Plane(C.c_void_p(cube.ctypes.data), 4, 5, 0)
    assert L.ab_cube_normalize_frame(h, None, C.byref(st), C.byref(po)) == invalid
    assert L.ab_cube_normalize_frame(h, C.byref(pin), None, C.byref(po)) == invalid
    assert L.ab_cube_normalize_frame(h, C.byref(pin), C.byref(st), None) == invalid
    assert L.ab_cube_normalize_frame(h, C.byref(pin), C.byref(st), C.byref(_lib.Plane(C.c_void_p(out.ctypes.data), 4, 4, 0))) == invalid
    bytes_out = np.zeros((3, 4, 5), np.uint8)
    bp = C.c_void_p(bytes_out.ctypes.data)
    assert L.ab_cube_export_frames(h, None, C.byref(st), 1, bp, 0, C.byref(i64)) == invalid
    assert L.ab_cube_export_frames(h, C.byref(pc), None, 1, bp, 0, C.byref(i64)) == invalid
    assert L.ab_cube_export_frames(h, C.byref(pc), C.byref(st), 1, None, 0, C.byref(i64)) == invalid
    assert L.ab_cube_extract_spectrum(h, C.byref(pc), 0, 0, None, 0) == invalid
    for bad in ((0.0, 1.0, 2.0, 1.0), (np.nan, 1.0, 0.0, 1.0), (0.0, np.nan, 0.0, 1.0), (0.0, 1.0, np.nan, 1.0), (0.0, 1.0, 0.0, np.nan)):
        with pytest.raises(AstroBurstError):
            ctx.normalize_with_global(out, bad)
        with pytest.raises(AstroBurstError):
            ctx.export_cube_frames(cube, bad)
    with pytest.raises(AstroBurstError):
        ctx.collapse_mean(cube, out=np.zeros((5, 4), F32))
    # frame_step < 1 is taken as 1; the library is still in working order after all of the above
    assert ctx.export_cube_frames(cube, (0.0, 1.0, 0.0, 1.0), 0).shape == (3, 4, 5)
    assert_bits(ctx.collapse_mean(cube), np.ones((4, 5), F32), "after the errors")


def test_cancel_and_trim(ctx):
    from astroburst_amd import _lib
    cube = R.random_cube((9, 129, 131))
    want = R.collapse_median(cube, R.NONZERO)
    assert_bits(ctx.collapse_median(cube), want, "before trim")
    ctx.trim()                                                            # releases the cube workspace; the next call takes it again
    ctx.request_cancel()
    try:
        for call in (lambda: ctx.collapse_mean(cube), lambda: ctx.collapse_median(cube), lambda: ctx.compute_global_stats(cube),
                     lambda: ctx.export_cube_frames(cube, (0.0, 1.0, 0.0, 1.0)), lambda: ctx.normalize_with_global(cube[0], (0.0, 1.0, 0.0, 1.0))):
            with pytest.raises(AstroBurstError) as e:
                call()
            assert e.value.code == _lib.AB_ERR_CANCELLED
    finally:
        ctx.clear_cancel()
    assert_bits(ctx.collapse_median(cube), want, "after trim and cancel")
