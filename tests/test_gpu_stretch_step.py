"""HIP parity of the compose wizard's stretch step (csrc/wizard_stretch.hip) on one MI355X: ab_arcsinh_stretch_rgb,
ab_arcsinh_stretch_composite, ab_arcsinh_stretch_view and ab_masked_stretch_composite.

Two references per case:
  1 the library's own unfused chain, compared with == (planes as f32 bit patterns, bytes, the range, the masked results; the mono view's
    statistics and STF too, its mean alone to 1e-12 relative, the bar of tests/test_gpu_stats_stf.py): ab_compute_image_stats x 3 ->
    ab_arcsinh_rgb_range -> ab_arcsinh_stretch_with_stats x 3 -> ab_render_rgb_preview(stf NULL); for the view ab_compute_image_stats
    -> ab_arcsinh_stretch_with_stats -> ab_auto_stretch_preview; for the masked command ab_masked_stretch_rgb_shared or
    ab_masked_stretch x 3 -> ab_render_rgb_preview(stf NULL);
  2 the oracle composition of tests/stretch_step_restatement.py.  The device asinhf is not the host's: planes are held to 1e-6 relative
    (the bar tests/test_gpu_color.py states for ab_arcsinh_stretch_with_stats); the range is ==; bytes must equal the truncating packer
    applied in numpy f32 to the planes the LIBRARY returned, at the pixels ab_preview_dims picks; the mono view's statistics, STF and
    bytes must equal the oracle's of the library's own stretched plane.  The masked command's star detection is held to the bar of
    tests/test_gpu_masked.py (counts ==, images within 1e-5 on at most 1e-5 of the pixels).
The masked composite is tests/test_gpu_masked.py's star_field at 256 x 320, the size of its test_rgb_shared: sky_image's stars are single
pixels, below the detector's min_fwhm, so no smaller sky_image finds any.
The argument errors that carry a message need a live context and are here too (tests/test_stretch_step_cpu.py has the rest)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import astroburst_amd as ab
import stretch_step_restatement as R
from astroburst_amd import AstroBurstError, _lib
from test_gpu_color_step import _bits, _dev, _dev_bytes, _dev_planes, _host, check_stats, check_stf
from test_gpu_masked import close_images, star_field
from test_gpu_stats_stf import sky_image

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
FACTORS = {"0.3": 0.3, "20": 20.0, "1e9": 1e9, "nan": NAN}      # 0.3 clamps to 1, 1e9 to 500, NaN stays
CRAFTED = ("max-first-R", "min-last-B", "zero-channel", "flat")


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=F32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _composite(name, crafted=None):
    """(r, g, b) of one composite around 0.25 with stars above 1; 67x93 carries a zero border, a NaN, both infinities, a negative pixel and
    a pixel at exactly 1e-7 (not valid: the test is v > 1e-7)"""
    rows, cols = (int(v) for v in name.split("x"))
    rng = np.random.default_rng(rows * 131 + cols)
    out = []
    for gain in (1.0, 1.6, 0.7):
        if rows < 10:
            a = rng.uniform(0.05, 1.2, (rows, cols)).astype(F32) * F32(gain)
        else:
            a = sky_image(rng, rows, cols, pad=False) * F32(gain / 4000.0)
        if name == "67x93":
            a[:2, :] = 0.0
            a[-2:, :] = 0.0
            a[:, :3] = 0.0
            a[:, -3:] = 0.0
            a[10, 11] = np.nan
            a[20, 21] = np.inf
            a[30, 31] = -np.inf
            a[40, 41] = -0.5
            a[50, 51] = F32(1e-7)
        out.append(np.ascontiguousarray(a, dtype=F32))
    if crafted == "max-first-R":           # the global maximum only in the first element of R
        out[0][0, 0] = F32(1e4)
    elif crafted == "min-last-B":          # the global minimum only in the last element of B; its index is no multiple of 4
        assert (rows * cols - 1) % 4 != 0
        out[2][-1, -1] = F32(1e-3)
    elif crafted == "zero-channel":        # no valid pixel in G: it contributes 0 to both, the global minimum is 0
        out[1][:] = 0.0
    elif crafted == "flat":                # the range is degenerate
        for a in out:
            a[:] = F32(0.25)
    return tuple(_frozen(a) for a in out)


@functools.lru_cache(maxsize=None)
def _device_composite(name, crafted, offset):
    return tuple(_dev(p, offset) for p in _composite(name, crafted))


@functools.lru_cache(maxsize=None)
def _oracle_composite(name, crafted, fkey):
    """the oracle's planes, clamped factor, range and degenerate flag (the bytes are taken from the library's planes)"""
    from oracle import pyoracle
    planes, _, f, rng, degenerate = R.arcsinh_stretch_composite(pyoracle, *_composite(name, crafted), FACTORS[fkey], 4096)
    return tuple(_frozen(p) for p in planes), f, rng, degenerate


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _close_planes(got, want, what):
    got, want = _host(got), _host(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok]) / np.maximum(np.abs(want[ok].astype(np.float64)), 1e-300)
    err[got[ok] == want[ok]] = 0.0
    print(f"{what}: max relative error {err.max() if err.size else 0.0:.3e}")
    assert (err <= 1e-6).all(), (what, float(err.max()))


def _unfused_composite(ctx, dplanes, factor, max_dim):
    """today's chain of older entry points (core/imaging/stretch.rs:72-88, cmd/processing/stretch.rs:102-115)"""
    gmin, gmax = ab.arcsinh_rgb_range(*[ctx.compute_image_stats(d) for d in dplanes])
    f = float(R.clamp_factor(factor))
    planes = [ctx.arcsinh_stretch_with_stats(d, gmin, gmax, f, 1.0) for d in dplanes]
    return planes, ctx.render_rgb_preview(*planes, max_dim), (gmin, gmax)


def _check_composite(ctx, oracle, name, fkey, max_dim, crafted=None, in_offset=1, out_offset=1, given=False):
    factor = FACTORS[fkey]
    planes = _composite(name, crafted)
    shape = planes[0].shape
    dplanes = _device_composite(name, crafted, in_offset)
    ph, pw = ctx.preview_dims(*shape, max_dim)
    u_planes, u_rgb8, u_range = _unfused_composite(ctx, dplanes, factor, max_dim)
    outs, planes_guarded = _dev_planes(shape, out_offset)
    rgb8, bytes_guarded = _dev_bytes((ph, pw, 3))
    res = ctx.arcsinh_stretch_composite(*dplanes, factor, max_dim=max_dim, global_range=u_range if given else None, out=rgb8, out_planes=outs)
    assert planes_guarded() and bytes_guarded()
    assert (res.rows, res.cols) == shape and (res.preview_rows, res.preview_cols) == (ph, pw)
    # 1: the library's own unfused chain
    assert _same_float(res.factor, float(R.clamp_factor(factor)))
    assert (res.global_min, res.global_max) == u_range
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(u_planes[c])), c
    got = _host(res.rgb8).reshape(ph, pw, 3).copy()
    assert np.array_equal(got, _host(u_rgb8))
    # with out_planes == NULL the bytes are those of the run that returned planes
    rgb8, bytes_guarded = _dev_bytes((ph, pw, 3))
    lone = ctx.arcsinh_stretch_composite(*dplanes, factor, max_dim=max_dim, global_range=u_range if given else None, out=rgb8)
    assert bytes_guarded() and lone.planes is None
    assert np.array_equal(_host(lone.rgb8).reshape(ph, pw, 3), got)
    assert (lone.global_min, lone.global_max, lone.degenerate) == (res.global_min, res.global_max, res.degenerate)
    # 2: the oracle composition
    o_planes, o_f, o_range, o_degenerate = _oracle_composite(name, crafted, fkey)
    assert _same_float(res.factor, float(o_f)) and (res.global_min, res.global_max) == (float(o_range[0]), float(o_range[1]))
    assert res.degenerate == o_degenerate
    for c in range(3):
        _close_planes(res.planes[c], o_planes[c], f"{name} {crafted} factor {fkey} channel {c}")
    assert np.array_equal(got, R.pack_trunc(oracle, [_host(p) for p in res.planes], max_dim))
    return res, got


# ---- ab_arcsinh_stretch_composite ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fkey", list(FACTORS))
def test_composite_3x5_host(ctx, oracle, fkey):
    """3 x 5 host planes: less than one wave, host outputs through the one synchronisation"""
    planes = _composite("3x5")
    res = ctx.arcsinh_stretch_composite(*planes, FACTORS[fkey], want_planes=True)
    assert all(isinstance(p, np.ndarray) for p in res.planes) and isinstance(res.rgb8, np.ndarray) and res.rgb8.shape == (3, 5, 3)
    u_planes, u_rgb8, u_range = _unfused_composite(ctx, planes, FACTORS[fkey], 4096)
    assert (res.global_min, res.global_max) == u_range
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(u_planes[c]))
    assert np.array_equal(res.rgb8, u_rgb8) and np.array_equal(res.rgb8, R.pack_trunc(oracle, res.planes, 4096))
    o_planes, _, o_range, _ = _oracle_composite("3x5", None, fkey)
    assert (res.global_min, res.global_max) == (float(o_range[0]), float(o_range[1]))
    for c in range(3):
        _close_planes(res.planes[c], o_planes[c], f"3x5 host factor {fkey} channel {c}")
    lone = ctx.arcsinh_stretch_composite(*planes, FACTORS[fkey])
    assert lone.planes is None and np.array_equal(lone.rgb8, res.rgb8)


@pytest.mark.parametrize("max_dim", [4096, 37])
@pytest.mark.parametrize("fkey", list(FACTORS))
def test_composite_67x93_device(ctx, oracle, fkey, max_dim):
    """device planes one float past a 16-byte boundary, bytes at an odd address; a zero border, a NaN, both infinities, a negative pixel
    and a pixel at exactly 1e-7"""
    res, got = _check_composite(ctx, oracle, "67x93", fkey, max_dim)
    r = _composite("67x93")[0]
    assert res.global_min > 1e-3 and not res.degenerate                   # neither 0, the negative pixel nor 1e-7 is the minimum
    for y, x in ((10, 11), (20, 21), (30, 31)):                            # a non-finite pixel becomes 0
        assert _host(res.planes[0])[y, x] == 0.0
    if fkey == "nan":
        assert np.isnan(_host(res.planes[0])[np.isfinite(r)]).all() and not got.any()


@pytest.mark.parametrize("max_dim", [4096, 128])
@pytest.mark.parametrize("fkey", ["20", "1e9"])
def test_composite_257x300_device(ctx, oracle, fkey, max_dim):
    """at max_dim 128 the preview is a pick (the sampled route), at 4096 every pixel (the full route); aligned planes: 16-byte accesses"""
    _check_composite(ctx, oracle, "257x300", fkey, max_dim, in_offset=0, out_offset=0)


def test_composite_mixed_alignment(ctx, oracle):
    """inputs one float past a 16-byte boundary, outputs two past: no 16-byte access fits all six planes"""
    _check_composite(ctx, oracle, "67x93", "20", 4096, in_offset=1, out_offset=2)
    _check_composite(ctx, oracle, "67x93", "20", 37, in_offset=3, out_offset=0)


def test_composite_1031x2053(ctx, oracle):
    """more than one iteration of the range pass's persistent grid, unaligned heads and tails"""
    _check_composite(ctx, oracle, "1031x2053", "20", 4096)


@pytest.mark.parametrize("name,max_dim", [("67x93", 4096), ("67x93", 37), ("1031x2053", 1024)])
@pytest.mark.parametrize("crafted", CRAFTED)
def test_composite_crafted_range(ctx, oracle, name, max_dim, crafted):
    res, got = _check_composite(ctx, oracle, name, "20", max_dim, crafted=crafted)
    if crafted == "max-first-R":
        assert res.global_max == 1e4
    elif crafted == "min-last-B":
        assert res.global_min == float(F32(1e-3))
    elif crafted == "zero-channel":
        assert res.global_min == 0.0 and not _host(res.planes[1]).any()
    else:
        assert res.degenerate and res.global_min == res.global_max == 0.25
        assert not got.any() and not any(_host(p).any() for p in res.planes)


@pytest.mark.parametrize("name,crafted", [("67x93", None), ("67x93", "flat"), ("1031x2053", "min-last-B")])
def test_composite_given_range_equals_the_computed_route(ctx, oracle, name, crafted):
    a, bytes_a = _check_composite(ctx, oracle, name, "20", 4096, crafted=crafted)
    b, bytes_b = _check_composite(ctx, oracle, name, "20", 4096, crafted=crafted, given=True)
    assert (a.global_min, a.global_max, a.degenerate) == (b.global_min, b.global_max, b.degenerate)
    assert np.array_equal(bytes_a, bytes_b) and all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a.planes, b.planes))


def test_composite_asynchronous_form(ctx):
    import torch
    dplanes = _device_composite("67x93", None, 1)
    want = ctx.arcsinh_stretch_composite(*dplanes, 20.0, max_dim=37, want_planes=True)
    outs, planes_guarded = _dev_planes((67, 93), 1)
    rgb8, bytes_guarded = _dev_bytes((want.preview_rows, want.preview_cols, 3))
    res = ctx.arcsinh_stretch_composite(*dplanes, 20.0, max_dim=37, fetch=False, out=rgb8, out_planes=outs)
    assert res.factor is None and res.global_min is None and res.degenerate is None
    ctx.synchronize()
    torch.cuda.synchronize()
    assert planes_guarded() and bytes_guarded()
    for c in range(3):
        assert np.array_equal(_bits(outs[c]), _bits(want.planes[c]))
    assert np.array_equal(_host(rgb8).reshape(_host(want.rgb8).shape), _host(want.rgb8))


def _raw_composite(ctx, planes, gmin, gmax, max_dim=4096, out_bytes=True):
    keep = []
    pr, pg, pb = (ctx._plane(x, keep) if not isinstance(x, _lib.Plane) else x for x in planes)
    by = np.zeros(16, np.uint8)
    return ctx._L.ab_arcsinh_stretch_composite(ctx._h, C.byref(pr), C.byref(pg), C.byref(pb), 20.0, gmin, gmax, max_dim, None,
                                               C.c_void_p(by.ctypes.data) if out_bytes else None, 0, None)


def test_composite_errors(ctx):
    r, g, b = _composite("67x93")
    d = _device_composite("67x93", None, 1)
    cases = [((r, g, b[:, :90]), dict()), ((r, g[:60], b), dict()), ((r, g, b), dict(max_dim=0)), ((r, g, b), dict(max_dim=-4)),
             ((r, g, b), dict(want_rgb8=False)),                                                 # both outputs NULL
             ((r, g, b), dict(out_planes=[np.zeros((67, 92), F32)] * 3)),
             (d, dict(out_planes=[d[0], d[1], d[2]])),                                           # an output overlaps an input
             (d, dict(out_planes=[_dev(r, 1)] * 3))]                                             # two outputs overlap
    for planes, kw in cases:
        with pytest.raises(AstroBurstError) as e:
            ctx.arcsinh_stretch_composite(*planes, 20.0, **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
    one = C.byref(C.c_float(0.5))
    assert _raw_composite(ctx, (r, g, b), one, None) == _lib.AB_ERR_INVALID                      # exactly one of global_min / global_max
    assert _raw_composite(ctx, (r, g, b), None, one) == _lib.AB_ERR_INVALID
    huge = _lib.Plane(C.c_void_p(r.ctypes.data), 65536, 32768, 0)                                # rows * cols == 2^31: never read
    assert _raw_composite(ctx, (huge, huge, huge), None, None) == _lib.AB_ERR_INVALID
    assert ctx.arcsinh_stretch_composite(r, g, b, 20.0).rgb8.shape == (67, 93, 3)                # and the context still works


# ---- ab_arcsinh_stretch_rgb ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,gamma", [(20.0, 1.0), (0.0, 1.0), (20.0, 0.5), (NAN, 1.0), (-3.0, 1.0)])
@pytest.mark.parametrize("name", ["3x5", "67x93", "257x300"])
def test_stretch_rgb(ctx, oracle, name, factor, gamma):
    planes = _composite(name)
    dplanes = _device_composite(name, None, 1)
    outs, planes_guarded = _dev_planes(planes[0].shape, 1)
    got, rng = ctx.arcsinh_stretch_rgb(*dplanes, factor, gamma, out_planes=outs)
    assert planes_guarded()
    o_planes, o_range = R.arcsinh_stretch_rgb(oracle, *planes, factor, gamma)
    if factor == 0.0:                                                                            # the clones (stretch.rs:65-67)
        assert rng == (0.0, 0.0) and o_range is None
        for c in range(3):
            assert np.array_equal(_bits(got[c]), _bits(planes[c])) and np.array_equal(_bits(got[c]), _bits(o_planes[c]))
        return
    gmin, gmax = ab.arcsinh_rgb_range(*[ctx.compute_image_stats(d) for d in dplanes])
    assert rng == (gmin, gmax) == (float(o_range[0]), float(o_range[1]))
    for c in range(3):
        assert np.array_equal(_bits(got[c]), _bits(ctx.arcsinh_stretch_with_stats(dplanes[c], gmin, gmax, factor, gamma))), c
        _close_planes(got[c], o_planes[c], f"rgb {name} factor {factor} gamma {gamma} channel {c}")
    again, rng2 = ctx.arcsinh_stretch_rgb(*dplanes, factor, gamma, global_range=(gmin, gmax))    # the given range: the same planes
    assert rng2 == rng and all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(again, got))
    host, rng3 = ctx.arcsinh_stretch_rgb(*planes, factor, gamma)                                  # host planes in and out
    assert rng3 == rng and all(isinstance(p, np.ndarray) and np.array_equal(_bits(p), _bits(q)) for p, q in zip(host, got))


def test_stretch_rgb_errors(ctx):
    r, g, b = _composite("67x93")
    d = _device_composite("67x93", None, 1)
    for planes, kw in [((r, g, b[:, :90]), dict()), ((r, g, b), dict(out_planes=[np.zeros((67, 92), F32)] * 3)), (d, dict(out_planes=list(d)))]:
        with pytest.raises(AstroBurstError) as e:
            ctx.arcsinh_stretch_rgb(*planes, 20.0, **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
    keep = []
    pr, pg, pb = (ctx._plane(x, keep) for x in (r, g, b))
    assert ctx._L.ab_arcsinh_stretch_rgb(ctx._h, C.byref(pr), C.byref(pg), C.byref(pb), None, None, C.c_float(20.0), C.c_float(1.0), None,
                                         None) == _lib.AB_ERR_INVALID                            # out_planes is required


# ---- ab_arcsinh_stretch_view --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fkey", list(FACTORS))
@pytest.mark.parametrize("name", ["3x5", "67x93", "257x300"])
def test_view(ctx, oracle, name, fkey):
    factor, img = FACTORS[fkey], _composite(name)[0]
    dimg = _device_composite(name, None, 1)[0]
    outs, planes_guarded = _dev_planes(img.shape, 1)
    u8, bytes_guarded = _dev_bytes(img.shape)
    res = ctx.arcsinh_stretch_view(dimg, factor, out=u8, out_plane=outs[0])
    assert planes_guarded() and bytes_guarded() and (res.rows, res.cols) == img.shape
    got_u8 = _host(res.u8).reshape(img.shape)
    # 1: the library's own unfused chain
    st = ctx.compute_image_stats(dimg)
    f = float(R.clamp_factor(factor))
    assert _same_float(res.factor, f) and (res.data_min, res.data_max) == (float(F32(st.min)), float(F32(st.max)))
    u_plane = ctx.arcsinh_stretch_with_stats(dimg, res.data_min, res.data_max, f, 1.0)
    u_u8, u_st, u_stf = ctx.auto_stretch_preview(u_plane)
    assert np.array_equal(_bits(res.plane), _bits(u_plane)) and np.array_equal(got_u8, _host(u_u8))
    check_stats(res.stats, u_st)
    check_stf(res.stf, u_stf)
    # 2: the oracle: its plane within the asinh bar; statistics, STF and bytes of the library's own stretched plane
    o_plane, _, o_f, _, _ = R.arcsinh_stretch_view(oracle, img, factor)
    assert _same_float(res.factor, float(o_f))
    _close_planes(res.plane, o_plane, f"view {name} factor {fkey}")
    mine = _host(res.plane)
    o_st = oracle.compute_image_stats(mine)
    check_stats(res.stats, o_st)
    o_stf = oracle.auto_stf(o_st)
    check_stf(res.stf, o_stf)
    assert np.array_equal(got_u8, oracle.apply_stf(mine, o_stf, o_st))
    if fkey == "nan":
        assert res.stats.valid_count == 0 and not got_u8.any()
    # the forms: no bytes; host planes
    bare = ctx.arcsinh_stretch_view(dimg, factor, want_u8=False)
    assert bare.u8 is None and np.array_equal(_bits(bare.plane), _bits(res.plane))
    host = ctx.arcsinh_stretch_view(img, factor)
    assert isinstance(host.plane, np.ndarray) and np.array_equal(_bits(host.plane), _bits(res.plane)) and np.array_equal(host.u8, got_u8)


def test_view_errors(ctx):
    img = _composite("67x93")[0]
    d = _device_composite("67x93", None, 1)[0]
    for image, kw in [(img, dict(out_plane=np.zeros((67, 92), F32))), (d, dict(out_plane=d))]:
        with pytest.raises(AstroBurstError) as e:
            ctx.arcsinh_stretch_view(image, 20.0, **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
    keep = []
    pi = ctx._plane(img, keep)
    assert ctx._L.ab_arcsinh_stretch_view(ctx._h, C.byref(pi), 20.0, None, None, 0, None) == _lib.AB_ERR_INVALID    # out_plane is required


# ---- ab_masked_stretch_composite ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _star_composite():
    base = star_field(np.random.default_rng(6), 256, 320, 50)
    return _frozen(base), _frozen(base * F32(0.8)), _frozen(base * F32(1.15))


@functools.lru_cache(maxsize=None)
def _oracle_masked(shared):
    from oracle import pyoracle
    planes, _, results, stars, coverage, mode = R.masked_stretch_composite(pyoracle, *_star_composite(), shared_mask=shared)
    return tuple(_frozen(p) for p in planes), results, stars, coverage, mode


_unfused_masked_cache = {}


def _unfused_masked(ctx, shared):
    """ab_masked_stretch_rgb_shared or ab_masked_stretch x 3 on device planes; computed once, read-only"""
    if shared not in _unfused_masked_cache:
        d = [_dev(p, 1) for p in _star_composite()]
        if shared:
            rr, rg, rb, mask = ctx.masked_stretch_rgb_shared(*d)
            stars, coverage = mask.stars_masked, mask.coverage_fraction
        else:
            rr, rg, rb = (ctx.masked_stretch(x) for x in d)
            stars, coverage = rr.stars_masked + rg.stars_masked + rb.stars_masked, (rr.mask_coverage + rg.mask_coverage + rb.mask_coverage) / 3.0
        _unfused_masked_cache[shared] = (d, (rr, rg, rb), stars, coverage)
    return _unfused_masked_cache[shared]


@pytest.mark.parametrize("max_dim", [100, 4096])
@pytest.mark.parametrize("with_planes", [True, False])
@pytest.mark.parametrize("shared", [True, False])
def test_masked_composite(ctx, oracle, shared, with_planes, max_dim):
    d, u_res, u_stars, u_coverage = _unfused_masked(ctx, shared)
    shape = (256, 320)
    ph, pw = ctx.preview_dims(*shape, max_dim)
    rgb8, bytes_guarded = _dev_bytes((ph, pw, 3))
    outs, planes_guarded = _dev_planes(shape, 1) if with_planes else (None, lambda: True)
    res = ctx.masked_stretch_composite(*d, shared_mask=shared, max_dim=max_dim, out=rgb8, out_planes=outs)
    assert planes_guarded() and bytes_guarded()
    assert (res.rows, res.cols, res.preview_rows, res.preview_cols) == (*shape, ph, pw)
    got = _host(res.rgb8).reshape(ph, pw, 3)
    # 1: the library's own calls followed by ab_render_rgb_preview(stf NULL)
    assert res.mask_mode == ("shared_luminance" if shared else "per_channel")
    assert res.stars_masked == u_stars > 20 and res.mask_coverage == u_coverage
    for c in range(3):
        assert (res.channels[c].iterations_run, res.channels[c].final_background, res.channels[c].converged, res.channels[c].stars_masked,
                res.channels[c].mask_coverage) == (u_res[c].iterations_run, u_res[c].final_background, u_res[c].converged, u_res[c].stars_masked,
                                                   u_res[c].mask_coverage), c
        if with_planes:
            assert np.array_equal(_bits(res.planes[c]), _bits(u_res[c].image)), c
    assert (res.planes is None) == (not with_planes)
    assert np.array_equal(got, _host(ctx.render_rgb_preview(*[r.image for r in u_res], max_dim)))
    # 2: the oracle composition, at the bar of tests/test_gpu_masked.py; the bytes from the library's planes
    o_planes, o_res, o_stars, o_coverage, o_mode = _oracle_masked(shared)
    assert res.mask_mode == o_mode and res.stars_masked == o_stars and abs(res.mask_coverage - o_coverage) <= 1e-5
    for c in range(3):
        assert res.channels[c].iterations_run == o_res[c].iterations_run and res.channels[c].converged == o_res[c].converged
        close_images(_host(u_res[c].image), o_planes[c])
    assert np.array_equal(got, R.pack_trunc(oracle, [_host(r.image) for r in u_res], max_dim))


def test_masked_composite_host(ctx):
    """host planes in, host planes and bytes out"""
    planes = _star_composite()
    d, u_res, _, _ = _unfused_masked(ctx, True)
    res = ctx.masked_stretch_composite(*planes, shared_mask=True, max_dim=100, want_planes=True)
    assert all(isinstance(p, np.ndarray) for p in res.planes) and isinstance(res.rgb8, np.ndarray)
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(u_res[c].image))
    assert np.array_equal(res.rgb8, _host(ctx.render_rgb_preview(*[r.image for r in u_res], 100)))


def test_masked_composite_errors(ctx):
    r, g, b = _star_composite()
    for planes, kw in [((r, g, b[:, :90]), dict()), ((r, g, b), dict(max_dim=0)), ((r, g, b), dict(want_rgb8=False)),
                       ((r, g, b), dict(out_planes=[np.zeros((256, 319), F32)] * 3))]:
        with pytest.raises(AstroBurstError) as e:
            ctx.masked_stretch_composite(*planes, **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
