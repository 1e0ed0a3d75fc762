"""The synthetic generator (csrc/synth.hip) on the GPU against tests/synth_restatement.py.  Flat field, apply_flat_field and the
general noise route: bit for bit.  The fast noise route: within one f32 ulp wherever the restatement's Gaussian-branch sample is
further than 1e-6 from a half-integer (every fixture: tests/test_synth_cpu.py).  render_stars: within 2 k ulp of a pixel covered
by k stars, exactly 0 where k = 0.  Every reference result is computed once and shared."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import synth_restatement as R

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float32).view(np.uint32)


# ---- flat field ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flat(rows, cols, seed, vs):
    f = R.generate_flat_field(cols, rows, seed, vs)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (37, 53), (64, 96)])
def test_flat_field_bitwise(ctx, shape):
    want = _flat(*shape, 1122, 0.3)
    host = ctx.synth_flat_field(*shape, 1122, 0.3)
    dev = ctx.synth_flat_field(*shape, 1122, 0.3, device=True)
    assert np.array_equal(_bits(host), want.view(np.uint32)) and np.array_equal(_bits(dev), want.view(np.uint32))


def test_apply_flat_field_bitwise(ctx):
    rng = np.random.default_rng(3)
    img = rng.uniform(-5.0, 5e4, (37, 53)).astype(np.float32)
    flat = _flat(37, 53, 1122, 0.3).copy()
    flat[0, :4] = np.float32([1e-6, 0.0, np.nextafter(np.float32(1e-6), np.float32(1.0)), -1.0])   # at, below and just above the threshold
    want = R.apply_flat_field(img, flat)
    assert np.array_equal(want[0, :2], img[0, :2]) and want[0, 2] != img[0, 2] and want[0, 3] == img[0, 3]
    host = ctx.synth_apply_flat_field(img.copy(), flat)
    dev = ctx.synth_apply_flat_field(torch.from_numpy(img).cuda(), torch.from_numpy(flat).cuda())
    assert np.array_equal(_bits(host), want.view(np.uint32)) and np.array_equal(_bits(dev), want.view(np.uint32))


# ---- noise ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noise_want(name):
    img, params = R.noise_fixtures()[name]
    info = {}
    want = R.apply_noise(img, **params, info=info)
    return img, params, want, info


def _assert_noise_close(got, want, margin, gain):
    """within one f32 ulp where the restatement's sample is clear of a half-integer; elsewhere the count may differ by one"""
    got, clear = _np(got).astype(np.float64), margin > 1e-6
    diff = np.abs(got - want.astype(np.float64))
    ulp = R.ulp_f32(want)
    assert (diff[clear] <= ulp[clear]).all(), float((diff[clear] / ulp[clear]).max())
    assert (diff[~clear] <= 1.0 / gain + 2 * ulp[~clear]).all()


@pytest.mark.parametrize("name", sorted(R.noise_fixtures()))
def test_noise_fast_route(ctx, name):
    img, params, want, info = _noise_want(name)
    assert info["min_margin"] > 1e-6
    host, n_host = ctx.synth_apply_noise(img, **params)
    dev, n_dev = ctx.synth_apply_noise(torch.from_numpy(img).cuda(), **params)
    assert n_host == 0 and n_dev == 0
    assert torch.is_tensor(dev) and dev.is_cuda and host.shape == img.shape
    _assert_noise_close(host, want, info["margin"], params["gain"])
    assert np.array_equal(_bits(host), _bits(dev))


def test_noise_general_route_bitwise(ctx):
    img = R.general_route_plane()
    want = R.apply_noise(img, **R.GENERAL_PARAMS)
    host, n_host = ctx.synth_apply_noise(img, **R.GENERAL_PARAMS)
    dev, n_dev = ctx.synth_apply_noise(torch.from_numpy(img).cuda(), **R.GENERAL_PARAMS)
    assert n_host == 1 and n_dev == 1
    assert np.array_equal(_bits(host), want.view(np.uint32)) and np.array_equal(_bits(dev), want.view(np.uint32))


def test_noise_moments(ctx):
    """a zero 256 x 256 plane, default parameters: mean (lambda + bias) / gain, variance (lambda + readout^2) / gain^2"""
    p = R.DEFAULT_NOISE
    out, n_host = ctx.synth_apply_noise(torch.zeros((256, 256), device="cuda"), **p)
    v = out.cpu().numpy().astype(np.float64)
    lam = p["sky_background"] * p["gain"] * p["exposure_time"] + p["dark_current"] * p["exposure_time"]
    var = (lam + p["readout_noise"] ** 2) / p["gain"] ** 2
    assert n_host == 0
    assert abs(v.mean() - (lam + p["bias_level"]) / p["gain"]) < 6.0 * math.sqrt(var / v.size)
    assert abs(v.var() / var - 1.0) < 6.0 * math.sqrt(2.0 / v.size)


# ---- render ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _render_want(case, psf):
    rows, cols = (64, 96) if case == "fixture" else (96, 128)
    stars = R.fixture_stars(rows, cols) if case == "fixture" else R.crowded_stars(rows, cols)
    img, k = R.render_stars(stars, R.PSFS[psf], cols, rows)
    return rows, cols, stars, img, k


def _assert_render_close(got, want, k):
    got = _np(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert not got[k == 0].any()
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (diff <= 2 * k * R.ulp_f32(want)).all(), float((diff / np.maximum(2 * k * R.ulp_f32(want), 1e-300)).max())


@pytest.mark.parametrize("psf", sorted(R.PSFS))
@pytest.mark.parametrize("case", ["fixture", "crowded"])
def test_render_stars(ctx, case, psf):
    rows, cols, stars, want, k = _render_want(case, psf)
    assert k.max() >= 2 and (k == 0).any()
    if case == "crowded":   # windows cross the 16-px tile edges in both axes
        assert (k[:, 15::16] > 0).any() and (k[15::16, :] > 0).any() and k.max() >= 4
    host = ctx.synth_render_stars(stars, R.PSFS[psf], rows, cols)
    dev = ctx.synth_render_stars(stars, R.PSFS[psf], rows, cols, device=True)
    _assert_render_close(host, want, k)
    assert np.array_equal(_bits(host), _bits(dev))


# ---- the chain -------------------------------------------------------------------------------------------------------------------
CHAIN = dict(width=80, height=48, n_stars=12, seed=42)


def _check_frame(ctx, frame, truth, noise_seed, flat_seed, vignette, strength=0.3):
    """one noisy frame against the restatement applied to the library's own truth: flat stage bit for bit, then the noise bound"""
    src = _np(truth)
    if vignette:
        flat = _flat(48, 80, flat_seed, strength)
        assert np.array_equal(_bits(ctx.synth_flat_field(48, 80, flat_seed, strength)), flat.view(np.uint32))
        src = R.apply_flat_field(src, flat)
        assert np.array_equal(_bits(ctx.synth_apply_flat_field(_np(truth).copy(), flat)), src.view(np.uint32))
    info = {}
    want = R.apply_noise(src, **dict(R.DEFAULT_NOISE, seed=noise_seed), info=info)
    _assert_noise_close(frame, want, info["margin"], R.DEFAULT_NOISE["gain"])


@pytest.mark.parametrize("vignette", [False, True])
def test_generate_chain(ctx, vignette):
    got = ctx.synth_generate(apply_vignette=vignette, **CHAIN)
    stars = R.uniform_field(80, 48, 12, 100.0, 50000.0, 42)
    assert got.stars.tobytes() == stars.tobytes() and got.frames_on_host == 0 and len(got.frames) == 1
    want, k = R.render_stars(stars, ("gaussian", 3.0), 80, 48)
    _assert_render_close(got.truth, want, k)
    _check_frame(ctx, got.frames[0], got.truth, 123, R.flat_seed(123), vignette)
    dev = ctx.synth_generate(apply_vignette=vignette, device=True, **CHAIN)
    assert np.array_equal(_bits(dev.truth), _bits(got.truth)) and np.array_equal(_bits(dev.frames[0]), _bits(got.frames[0]))


def test_generate_stack_chain_and_seeds(ctx):
    got = ctx.synth_generate_stack(apply_vignette=True, n_frames=3, **CHAIN)
    assert len(got.frames) == 3 and got.frames_on_host == 0
    one = ctx.synth_generate(apply_vignette=True, **CHAIN)
    assert np.array_equal(_bits(got.truth), _bits(one.truth)) and np.array_equal(_bits(got.frames[0]), _bits(one.frames[0]))
    for i, frame in enumerate(got.frames):   # frame i: flat seed + 999 + i, noise seed + 7919 i
        _check_frame(ctx, frame, got.truth, R.frame_noise_seed(123, i), R.flat_seed(123, i), True)
    assert not np.array_equal(_bits(got.frames[1]), _bits(got.frames[2]))


def test_generate_general_route_is_counted(ctx):
    """no sky, no dark current, a short exposure: lambda is below 30 off the stars -> every frame takes the host route, bit for bit"""
    noise = dict(sky_background=0.0, dark_current=0.0, exposure_time=0.01)
    got = ctx.synth_generate_stack(noise=noise, n_frames=2, device=True, **CHAIN)
    assert got.frames_on_host == 2
    for i, frame in enumerate(got.frames):
        want = R.apply_noise(_np(got.truth), **dict(R.DEFAULT_NOISE, seed=R.frame_noise_seed(123, i), **noise))
        assert np.array_equal(_bits(frame), want.view(np.uint32))


def test_every_device_entry_point_is_deterministic(ctx):
    stars = R.crowded_stars(96, 128)
    img = R.noise_fixtures()["values_37x53"][0]
    calls = [lambda: ctx.synth_render_stars(stars, R.PSFS["moffat"], 96, 128, device=True),
             lambda: ctx.synth_flat_field(37, 53, 5, 0.3, device=True),
             lambda: ctx.synth_apply_flat_field(torch.from_numpy(img).cuda(), torch.from_numpy(_flat(37, 53, 1122, 0.3).copy()).cuda()),
             lambda: ctx.synth_apply_noise(torch.from_numpy(img).cuda(), seed=5)[0],
             lambda: ctx.synth_generate(device=True, **CHAIN).frames[0],
             lambda: ctx.synth_generate_stack(device=True, n_frames=2, apply_vignette=True, **CHAIN).frames[1]]
    for call in calls:
        assert np.array_equal(_bits(call()), _bits(call()))


def test_stack_frames_feed_the_sigma_clip(ctx):
    """8 device frames of one rendering straight into ab_stack_sigma_clip: the stack is the noiseless expectation within the
    standard error of an 8-frame mean"""
    p = R.DEFAULT_NOISE
    got = ctx.synth_generate_stack(width=128, height=96, n_stars=20, n_frames=8, device=True)
    assert all(torch.is_tensor(f) and f.is_cuda for f in got.frames) and got.frames_on_host == 0
    out, _ = ctx.stack_sigma_clip(got.frames, 3.0, 3.0, 5)
    truth = got.truth.cpu().numpy().astype(np.float64)
    expect = (truth + p["sky_background"]) * p["exposure_time"] + p["dark_current"] * p["exposure_time"] / p["gain"] + p["bias_level"] / p["gain"]
    lam = (truth + p["sky_background"]) * p["gain"] * p["exposure_time"] + p["dark_current"] * p["exposure_time"]
    var_px = (lam + p["readout_noise"] ** 2) / p["gain"] ** 2 / 8.0
    resid = out.cpu().numpy().astype(np.float64) - expect
    assert abs(resid.mean()) < 6.0 * math.sqrt(var_px.mean() / resid.size)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    import astroburst_amd as ab
    L, h, lib = ctx._L, ctx._h, ab._lib
    stars = R.fixture_stars(64, 96)
    out = np.zeros((64, 96), np.float32)
    po = lib.Plane(C.c_void_p(out.ctypes.data), 64, 96, 0)
    psf = ab.synth_psf_type(("gaussian", 3.0))
    sp = stars.ctypes.data_as(C.POINTER(lib.SynthStarC))
    cfg = ab.synth_config(width=96, height=64, n_stars=3)
    noise = ab.synth_noise_params()
    # NULL arguments
    assert L.ab_synth_render_stars(h, sp, 10, None, C.byref(po)) == lib.AB_ERR_INVALID
    assert L.ab_synth_render_stars(h, None, 10, C.byref(psf), C.byref(po)) == lib.AB_ERR_INVALID
    assert L.ab_synth_render_stars(None, sp, 10, C.byref(psf), C.byref(po)) == lib.AB_ERR_INVALID
    assert L.ab_synth_flat_field(h, 1, 0.3, None) == lib.AB_ERR_INVALID
    assert L.ab_synth_apply_flat_field(h, None, C.byref(po)) == lib.AB_ERR_INVALID
    assert L.ab_synth_apply_noise(h, C.byref(po), None, C.byref(po), None) == lib.AB_ERR_INVALID
    assert L.ab_synth_generate(h, None, C.byref(po), None, None, 0, None) == lib.AB_ERR_INVALID
    assert L.ab_synth_generate(h, C.byref(cfg), None, None, None, 0, None) == lib.AB_ERR_INVALID
    assert L.ab_synth_generate(h, C.byref(cfg), C.byref(po), None, None, 3, None) == lib.AB_ERR_INVALID
    assert L.ab_synth_generate_stack(h, C.byref(cfg), None, None, None, 0, None) == lib.AB_ERR_INVALID
    # plane dims that do not match the config / each other
    bad = lib.Plane(C.c_void_p(out.ctypes.data), 96, 64, 0)
    assert L.ab_synth_generate(h, C.byref(cfg), C.byref(bad), None, None, 0, None) == lib.AB_ERR_INVALID
    assert L.ab_synth_generate(h, C.byref(cfg), C.byref(po), C.byref(bad), None, 0, None) == lib.AB_ERR_INVALID
    assert L.ab_synth_apply_noise(h, C.byref(po), C.byref(noise), C.byref(bad), None) == lib.AB_ERR_INVALID
    assert L.ab_synth_apply_flat_field(h, C.byref(po), C.byref(bad)) == lib.AB_ERR_INVALID
    # a non-finite star, bad PSF parameters, a radius over the cap
    for col, val in ((0, np.nan), (1, np.inf), (3, -np.inf)):
        s = stars.copy()
        s[4, col] = val
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.synth_render_stars(s, ("gaussian", 3.0), 64, 96)
        assert e.value.code == lib.AB_ERR_INVALID
    for psf_bad in (("gaussian", 0.0), ("gaussian", np.nan), ("moffat", 4.0, -1.0), ("moffat", np.inf, 2.5), ("airy", -2.0), (9, 1.0)):
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.synth_render_stars(stars, psf_bad, 64, 96)
        assert e.value.code == lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.synth_render_stars(stars, ("gaussian", 400.0), 64, 96)   # psf_r = ceil(4 * 400 / 2.3548) = 680 > 512
    assert e.value.code == lib.AB_ERR_UNSUPPORTED
    # n_frames = 0
    cfg.n_frames = 0
    assert L.ab_synth_generate_stack(h, C.byref(cfg), C.byref(po), None, None, 0, None) == lib.AB_ERR_INVALID
    # a field that would not terminate
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.synth_generate(field_type=("king_cluster", 0.0, 10.0), **CHAIN)
    assert e.value.code == lib.AB_ERR_INVALID


def test_cancellation_between_frames(ctx):
    import astroburst_amd as ab
    ticks = []

    def tick(stage, cur, tot):
        ticks.append((stage, cur, tot))
        ctx.request_cancel()

    ctx.set_progress_cb(tick)
    try:
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.synth_generate_stack(n_frames=3, **CHAIN)
        assert e.value.code == ab._lib.AB_ERR_CANCELLED and ticks == [("synth", 1, 3)]
    finally:
        ctx.set_progress_cb(None)
        ctx.clear_cancel()
    ticks.clear()
    ctx.set_progress_cb(lambda *a: ticks.append(a))
    try:
        ctx.synth_generate_stack(n_frames=3, **CHAIN)
    finally:
        ctx.set_progress_cb(None)
    assert ticks == [("synth", 1, 3), ("synth", 2, 3), ("synth", 3, 3)]
