"""ab_estimate_psf (csrc/psf.hip) on the GPU against tests/psf_restatement.py, bit for bit: the f32 kernel through a uint32 view,
every f64 field of every star of stars_used, the averages and the spread through uint64 views, the counts as integers.  The
fixtures' own conditions (what each has to contain to exercise its case) are asserted on the CPU in tests/test_psf_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import psf_restatement as P

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _want(name):
    """(image, config, the restatement's result), computed once per fixture"""
    if name == "A":
        img, cfg = P.field_a(), dict(num_stars=8)
    elif name == "B":
        img, cfg = P.field_a() * np.float32(0.0137), dict(num_stars=8)
    elif name == "C":
        img, cfg = P.field_c()[0], dict(edge_margin=20, num_stars=6)
    elif name in ("D1", "D2"):
        img, cfg = P.field_d(int(name[1]))
    elif name == "E":
        img, cfg = P.field_e(), dict(num_stars=8)
    elif name == "F":
        a = P.field_a()
        img, cfg = a - np.float32(np.median(a)), dict(num_stars=8)
    else:
        raise KeyError(name)
    img = np.ascontiguousarray(img, dtype=np.float32)
    img.setflags(write=False)
    return img, cfg, P.estimate_psf(img, **cfg)


def _bits64(vals):
    return np.asarray(vals, dtype=np.float64).view(np.uint64)


def _assert_same(got, want):
    assert want.error is None
    kernel = got.kernel.cpu().numpy() if torch.is_tensor(got.kernel) else got.kernel
    assert kernel.shape == want.kernel.shape and kernel.dtype == np.float32
    assert (got.stars_detected, got.stars_filtered, got.stars_rejected, got.kernel_size) == \
        (want.stars_detected, want.stars_filtered, want.stars_rejected, want.kernel_size)
    assert len(got.stars_used) == len(want.stars_used)
    for i, (g, w) in enumerate(zip(got.stars_used, want.stars_used)):
        gb = _bits64([g.x, g.y, g.peak, g.flux, g.fwhm, g.ellipticity, g.distance_from_center, g.snr])
        assert np.array_equal(gb, _bits64(w.astuple())), (i, g, w)
    assert np.array_equal(_bits64([got.average_fwhm, got.average_ellipticity, got.spread_pixels]),
                          _bits64([want.average_fwhm, want.average_ellipticity, want.spread_pixels]))
    assert np.array_equal(kernel.view(np.uint32), want.kernel.view(np.uint32))


@pytest.mark.parametrize("img_on_device,out_on_device", [(False, False), (True, True), (True, False), (False, True)])
def test_a_integer_field_bitwise_host_and_device(ctx, img_on_device, out_on_device):
    img, cfg, want = _want("A")
    assert len(want.stars_used) == 8
    src = torch.from_numpy(img.copy()).cuda() if img_on_device else img
    out = torch.full((31, 31), -1.0, device="cuda") if out_on_device else np.full((31, 31), -1.0, np.float32)
    got = ctx.estimate_psf(src, out=out, **cfg)
    assert got.kernel is out
    _assert_same(got, want)
    if not (img_on_device or out_on_device):   # and without `out`: a kernel of the image's kind
        assert isinstance(ctx.estimate_psf(img, **cfg).kernel, np.ndarray)
        assert torch.is_tensor(ctx.estimate_psf(torch.from_numpy(img.copy()).cuda(), **cfg).kernel)


def test_b_inexact_sums_outside_the_guard_band(ctx):
    img, cfg, want = _want("B")
    assert P.guard_band_empty(img, want.threshold)
    _assert_same(ctx.estimate_psf(torch.from_numpy(img.copy()).cuda(), **cfg), want)


def test_c_ties_are_suppressed_in_raster_order(ctx):
    img, cfg, want = _want("C")
    _assert_same(ctx.estimate_psf(torch.from_numpy(img.copy()).cuda(), **cfg), want)
    # every measured peak, not only the selected ones: with no filter and no limit stars_used is the whole detected list, sorted
    wide = dict(edge_margin=20, num_stars=1000, saturation_threshold=10.0, min_peak_fraction=-1.0, max_ellipticity=2.0,
                max_center_distance_fraction=10.0)
    want_all = P.estimate_psf(img, **wide)
    assert len(want_all.stars_used) == want_all.stars_detected >= 8
    _assert_same(ctx.estimate_psf(img, **wide), want_all)


@pytest.mark.parametrize("variant", ["D1", "D2"])
def test_d_odd_shape_margins_border_and_refused_cutouts(ctx, variant):
    img, cfg, want = _want(variant)
    got = ctx.estimate_psf(torch.from_numpy(img.copy()).cuda(), **cfg)
    assert got.kernel.shape == (15, 15)
    _assert_same(got, want)
    if variant == "D2":
        assert want.cutouts_used < len(want.stars_used) and got.stars_rejected == want.stars_filtered - want.cutouts_used


def test_e_large_annuli_and_the_fwhm_gate(ctx):
    img, cfg, want = _want("E")
    _assert_same(ctx.estimate_psf(torch.from_numpy(img.copy()).cuda(), **cfg), want)
    wide = dict(num_stars=1000, saturation_threshold=10.0, min_peak_fraction=-1.0, max_ellipticity=2.0, max_center_distance_fraction=10.0)
    want_all = P.estimate_psf(img, **wide)   # the defocused stars themselves (their peak is the image's maximum) among stars_used
    assert any(s.fwhm > 17.0 for s in want_all.stars_used)
    _assert_same(ctx.estimate_psf(img, **wide), want_all)


def test_f_negative_pixels(ctx):
    img, cfg, want = _want("F")
    assert (img < 0).mean() > 0.4 and len(want.stars_used) == 8
    _assert_same(ctx.estimate_psf(torch.from_numpy(img.copy()).cuda(), **cfg), want)


def test_g_outcomes_and_errors(ctx):
    import astroburst_amd as ab
    from astroburst_amd import _lib

    def outcome(img, **cfg):
        out = np.full((2 * cfg.get("cutout_radius", 15) + 1,) * 2, -7.0, np.float32)
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.estimate_psf(img, out=out, **cfg)
        assert np.all(out == -7.0)   # the kernel is untouched
        return e.value
    e = outcome(P.field_noise(), edge_margin=16)
    assert e.message == P.ERR_NO_STARS == P.estimate_psf(P.field_noise(), edge_margin=16).error
    e = outcome(P.field_saturated(), edge_margin=20)
    assert e.message == P.ERR_NO_PASS == P.estimate_psf(P.field_saturated(), edge_margin=20).error
    flat = np.full((96, 128), 7.0, np.float32)   # every pixel inside the margins is a candidate: more than the first list holds
    e = outcome(flat, edge_margin=16)
    assert e.message == P.estimate_psf(flat, edge_margin=16).error
    e = outcome(torch.from_numpy(flat).cuda(), edge_margin=16)
    assert e.message == P.estimate_psf(flat, edge_margin=16).error
    # bad arguments
    a = P.field_a().copy()
    a[100, 100] = np.nan
    e = outcome(a, num_stars=8)
    assert e.code == _lib.AB_ERR_INVALID and "non-finite" in e.message
    a[100, 100] = np.inf
    assert outcome(a, num_stars=8).code == _lib.AB_ERR_INVALID
    e = outcome(np.zeros((60, 200), np.float32))    # rows <= 2 * 30
    assert e.code == _lib.AB_ERR_INVALID and "edge_margin" in e.message
    assert outcome(np.zeros((200, 60), np.float32)).code == _lib.AB_ERR_INVALID
    assert outcome(P.field_a(), num_stars=0).code == _lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError) as ei:
        ctx.estimate_psf(P.field_a(), out=np.zeros((31, 29), np.float32))
    assert ei.value.code == _lib.AB_ERR_INVALID and "kernel plane" in ei.value.message
    with pytest.raises(ab.AstroBurstError) as ei:
        ctx.estimate_psf(P.field_a(), cutout_radius=_lib.AB_PSF_MAX_CUTOUT_RADIUS + 1)
    assert ei.value.code == _lib.AB_ERR_UNSUPPORTED
    # the largest radius served
    img, _, _ = _want("A")
    _assert_same(ctx.estimate_psf(img, num_stars=8, edge_margin=40, cutout_radius=31),
                 P.estimate_psf(img, num_stars=8, edge_margin=40, cutout_radius=31))


def test_h_device_kernel_goes_straight_into_deconvolution(ctx):
    img, cfg, _ = _want("A")
    dev = torch.from_numpy(img.copy()).cuda()
    res = ctx.estimate_psf(dev, **cfg)
    assert torch.is_tensor(res.kernel) and res.kernel.is_cuda
    a, it_a, conv_a = ctx.richardson_lucy(dev, res.kernel, iterations=3)
    b, it_b, conv_b = ctx.richardson_lucy(dev, res.kernel.cpu().numpy(), iterations=3)
    assert it_a == it_b == 3 and conv_a == conv_b
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
