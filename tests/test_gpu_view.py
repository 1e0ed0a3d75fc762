"""HIP parity of the open-file view (csrc/view.hip) on one MI355X: ab_display_histogram, ab_process_fits_view, ab_process_rgb_fits_view.

Two references, both compared with == (bins, bytes, valid_count, min, max, median, MAD, sigma and the STF parameters are integers or the
same f64 scalar code); the mean alone is held to 1e-12 relative, tests/test_gpu_stats_stf.py's bar, because the reference leaves its
summation order open:
  1 the library's own unfused calls: ab_auto_stretch_preview, ab_compute_image_stats, ab_apply_tone_composite with the default
    configuration, ab_display_histogram;
  2 the oracle composition of tests/view_restatement.py: oracle.compute_image_stats, auto_stf, apply_stf / apply_stf_f32 +
    render_rgb_preview, and oracle.build_histogram(65536) folded by the restatement of downsample_histogram.
"""
import functools

import numpy as np
import pytest

import view_restatement as V
from astroburst_amd import AstroBurstError, _lib
from test_gpu_stats_stf import sky_image

pytestmark = pytest.mark.gpu

F32 = np.float32
TARGETS = [1, 49, 512, 1000, 16384, 16385, 65535, 65536, 100000]
POISON = -1   # 0xFFFFFFFF in the int32 tensors that carry device bins


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _u32(t):
    """bins as uint32 words (device bins travel in int32 tensors)"""
    return np.ascontiguousarray(_host(t)).view(np.uint32)


def _dev(a, offset=1):
    """the array on the device, `offset` floats past a 256-byte boundary (1: one float past a 16-byte boundary)"""
    import torch
    a = np.array(a, copy=True, order="C")
    buf = torch.empty(a.size + offset + 64, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def _dev_bins(n):
    """a poisoned int32 device buffer of n words with a guard band behind it"""
    import torch
    buf = torch.full((n + 16,), POISON, dtype=torch.int32, device="cuda")
    return buf[:n], buf


def check_stats(got, ref):
    assert got.valid_count == ref.valid_count
    assert got.min == ref.min and got.max == ref.max
    assert got.median == ref.median, (got.median, ref.median)
    assert got.mad == ref.mad and got.sigma == ref.sigma
    assert abs(got.mean - ref.mean) <= 1e-12 * abs(ref.mean)


def check_stf(got, ref):
    assert (got.shadow, got.midtone, got.highlight) == (ref.shadow, ref.midtone, ref.highlight)


# ---- ab_display_histogram ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hist_case(name):
    """(plane, dmin, dmax) -- the plane read-only, shared by every target"""
    rng = np.random.default_rng(len(name) + 77)
    if name == "3x5":              # less than one wave
        img = rng.uniform(10.0, 20.0, (3, 5)).astype(F32)
    elif name == "67x93":
        img = rng.uniform(0.0, 1.0, (67, 93)).astype(F32)
        img[3, 4] = np.nan
    else:                          # 300 x 400 sky with padding, NaN, inf and a negative pixel
        img = sky_image(rng, 300, 400)
    valid = img[np.isfinite(img) & (img > 1e-7)]
    img.setflags(write=False)
    return img, float(valid.min()), float(valid.max())


@functools.lru_cache(maxsize=None)
def _src_bins(name):
    from oracle import pyoracle
    img, dmin, dmax = _hist_case(name)
    h = pyoracle.build_histogram(img, V.HISTOGRAM_BINS, dmin, dmax)
    h.setflags(write=False)
    return h


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", ["3x5", "67x93", "300x400"])
def test_display_histogram(ctx, name, target):
    img, dmin, dmax = _hist_case(name)
    want = V.downsample(_src_bins(name), target)
    assert want.size == min(target, 65536)
    if name == "3x5":                        # a host plane, a host output
        got = ctx.display_histogram(img, dmin, dmax, target)
        assert got.dtype == np.uint32
    else:                                    # a device plane one float past a 16-byte boundary, a poisoned device output
        out, whole = _dev_bins(want.size)
        got = ctx.display_histogram(_dev(img, 1), dmin, dmax, target, out=out)
        assert (_host(whole)[want.size:] == POISON).all()
    assert np.array_equal(_u32(got), want)
    if target in (49, 512):                  # and against the library's own two steps
        two = ctx.downsample_histogram(ctx.build_histogram(img, 65536, dmin, dmax), target)
        assert np.array_equal(_u32(got), two)


def _adversarial(kind, shape):
    """(plane, dmin, dmax)"""
    rng = np.random.default_rng(shape[0] + len(kind))
    n = shape[0] * shape[1]
    if kind == "no_valid":
        img = np.zeros(shape, F32)
        img.reshape(-1)[::3] = np.nan
        img.reshape(-1)[1::3] = -4.0
        return img, 0.0, 1.0
    if kind == "one_valid":
        img = np.zeros(shape, F32)
        img.reshape(-1)[n // 2] = 7.5
        return img, 0.0, 10.0
    if kind == "constant":                   # range < 1e-10: zero bins
        return np.full(shape, 1234.5, F32), 1234.5, 1234.5
    if kind == "two_values":                 # everything in the first and the last bin
        img = np.where(rng.random(shape) < 0.3, F32(5.0), F32(900.0)).astype(F32)
        return img, 5.0, 900.0
    if kind == "equal_dmax":                 # pixels exactly at dmax: t = 65536 -> .min(65535)
        img = rng.uniform(1.0, 2.0, shape).astype(F32)
        img.reshape(-1)[::17] = 2.0
        return img, 1.0, 2.0
    if kind == "narrow_range":               # pixels below dmin -> bin 0, above dmax -> the last bin
        img = rng.uniform(1.0, 100.0, shape).astype(F32)
        return img, 30.0, 60.0
    assert kind == "brightest"               # one pixel alone at the top: at 49 bins it vanishes
    img = rng.uniform(1.0, 50.0, shape).astype(F32)
    img.reshape(-1)[n // 3] = 100.0
    return img, float(img.min()), 100.0


@pytest.mark.parametrize("shape", [(64, 64), (257, 311)], ids=["64x64", "257x311"])
@pytest.mark.parametrize("kind", ["no_valid", "one_valid", "constant", "two_values", "equal_dmax", "narrow_range", "brightest"])
def test_display_histogram_adversarial(ctx, oracle, kind, shape):
    img, dmin, dmax = _adversarial(kind, shape)
    src = oracle.build_histogram(img, V.HISTOGRAM_BINS, dmin, dmax)
    dimg = _dev(img, 1)
    valid = int((np.isfinite(img) & (img > 1e-7)).sum())
    for target in (49, 512, 1000):
        want = V.downsample(src, target)
        host = ctx.display_histogram(img, dmin, dmax, target)
        assert np.array_equal(host, want), (kind, target)
        out, whole = _dev_bins(target)
        first = _u32(ctx.display_histogram(dimg, dmin, dmax, target, out=out)).copy()
        again = _u32(ctx.display_histogram(dimg, dmin, dmax, target, out=out))   # nothing of the first call is left in the workspace
        assert np.array_equal(first, want) and np.array_equal(again, want), (kind, target)
        assert (_host(whole)[target:] == POISON).all()
        total = int(want.astype(np.uint64).sum())
        if kind in ("no_valid", "constant"):
            assert total == 0
        elif kind == "two_values" and target == 49:     # the last source bin, with every pixel at dmax, belongs to no display bin
            assert total == int((img == 5.0).sum()) and np.count_nonzero(want) == 1 and want[0] == total
        elif kind == "two_values":
            assert total == valid and np.count_nonzero(want) == 2 and want[0] > 0 and want[-1] > 0
        elif kind == "brightest":
            assert total == (valid - 1 if target == 49 else valid)
        elif kind == "equal_dmax" and target != 49:
            assert total == valid and want[-1] >= int((img == 2.0).sum())
        elif target != 49:
            assert total == valid


# ---- ab_process_fits_view ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mono(shape):
    img = sky_image(np.random.default_rng(shape[0] * 31 + shape[1]), *shape, pad=shape[0] > 50)
    img.setflags(write=False)
    return img


def _check_mono(ctx, oracle, img, dimg, hist_bins, on_device, **cfg):
    ref_u8, ref_stats, ref_stf = ctx.auto_stretch_preview(dimg, **cfg)
    v = ctx.process_fits_view(dimg if on_device else img, hist_bins=hist_bins, **cfg)
    assert (v.rows, v.cols) == img.shape
    assert np.array_equal(_host(v.u8), _host(ref_u8))
    check_stats(v.stats, ref_stats)
    check_stf(v.stf, ref_stf)
    o_u8, o_bins, o_stats, o_stf = V.fits_view(oracle, img, hist_bins, **cfg)
    assert np.array_equal(_host(v.u8), o_u8)
    check_stats(v.stats, o_stats)
    check_stf(v.stf, o_stf)
    if hist_bins == 0:
        assert v.bins is None
    else:
        assert np.array_equal(_u32(v.bins), _u32(ctx.display_histogram(dimg, v.stats.min, v.stats.max, hist_bins)))
        assert np.array_equal(_u32(v.bins), o_bins)
    return v


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("hist_bins", [0, 512, 49])
@pytest.mark.parametrize("shape", [(301, 403), (4, 4)], ids=["301x403", "4x4"])
def test_process_fits_view_exact_path(ctx, oracle, shape, hist_bins, on_device):
    img = _mono(shape)
    _check_mono(ctx, oracle, img, _dev(img, 1), hist_bins, on_device)


def test_process_fits_view_histogram_path(ctx, oracle):
    img = _mono((2048, 2051))                # 4 200 448 px: above the exact select's 4 000 000
    v = _check_mono(ctx, oracle, img, _dev(img, 1), 512, True)
    assert int(_u32(v.bins).astype(np.uint64).sum()) == v.stats.valid_count


def test_process_fits_view_config(ctx, oracle):
    img = _mono((301, 403))
    _check_mono(ctx, oracle, img, _dev(img, 0), 512, True, target_bg=0.1, shadow_k=-1.5)


def test_process_fits_view_asynchronous_form(ctx):
    import torch
    img = _mono((301, 403))
    dimg = _dev(img, 1)
    want = ctx.process_fits_view(dimg, hist_bins=512)
    u8 = torch.full(img.shape, 0xAB, dtype=torch.uint8, device="cuda")
    bins, _ = _dev_bins(512)
    v = ctx.process_fits_view(dimg, hist_bins=512, fetch=False, out=u8, out_bins=bins)   # info == NULL, device outputs
    assert v.stats is None and v.stf is None
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(_host(u8), _host(want.u8)) and np.array_equal(_u32(bins), _u32(want.bins))


def test_process_fits_view_all_invalid(ctx, oracle):
    img = np.zeros((37, 41), F32)
    img[::2] = np.nan
    img[1, 1] = -3.0
    for plane in (img, _dev(img, 1)):
        v = ctx.process_fits_view(plane, hist_bins=512)
        assert not _host(v.u8).any() and not _u32(v.bins).any()
        assert v.stats.valid_count == 0 and (v.stats.min, v.stats.max, v.stats.median, v.stats.mean) == (0.0, 0.0, 0.0, 0.0)
        check_stf(v.stf, oracle.auto_stf(oracle.compute_image_stats(img)))


# ---- ab_process_rgb_fits_view -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rgb(shape, dead=None):
    """three channels of different levels (dead: that channel holds no valid pixel)"""
    rng = np.random.default_rng(shape[0] * 13 + shape[1])
    out = []
    for c, (gain, offset) in enumerate(((1.0, 0.0), (0.4, 150.0), (2.5, -800.0))):
        a = sky_image(rng, *shape, pad=shape[0] > 50) * F32(gain) + F32(offset)
        if c == dead:
            a = np.where(rng.random(shape) < 0.5, F32(np.nan), F32(0.0)).astype(F32)
        a = np.ascontiguousarray(a, dtype=F32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _check_rgb(ctx, oracle, planes, max_dim, hist_bins, on_device, offset=1):
    dplanes = [_dev(p, offset) for p in planes]
    use = dplanes if on_device else planes
    v = ctx.process_rgb_fits_view(*use, hist_bins=hist_bins, max_dim=max_dim)
    stats = [ctx.compute_image_stats(p) for p in dplanes]
    for c in range(3):
        check_stats(v.stats[c], stats[c])
        check_stf(v.stf[c], ctx.auto_stf(stats[c]))
    tone = ctx.apply_tone_composite(*dplanes, stats, max_dim=max_dim)     # ab_tone_config_default
    assert (v.preview_rows, v.preview_cols) == (tone.info.preview_rows, tone.info.preview_cols) and (v.rows, v.cols) == planes[0].shape
    assert np.array_equal(_host(v.rgb8), _host(tone.rgb8))
    o_rgb8, o_bins, o_stats, o_stf = V.rgb_fits_view(oracle, *planes, hist_bins, max_dim)
    assert np.array_equal(_host(v.rgb8), o_rgb8)
    for c in range(3):
        check_stats(v.stats[c], o_stats[c])
        check_stf(v.stf[c], o_stf[c])
    if hist_bins == 0:
        assert v.bins is None
    else:
        assert np.array_equal(_u32(v.bins), _u32(ctx.display_histogram(dplanes[0], v.stats[0].min, v.stats[0].max, hist_bins)))
        assert np.array_equal(_u32(v.bins), o_bins)
    return v


@pytest.mark.parametrize("on_device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("hist_bins", [512, 49, 0])
@pytest.mark.parametrize("shape,max_dim", [((67, 93), 4096), ((130, 70), 32)], ids=["67x93@4096", "130x70@32"])
def test_process_rgb_fits_view(ctx, oracle, shape, max_dim, hist_bins, on_device):
    _check_rgb(ctx, oracle, _rgb(shape), max_dim, hist_bins, on_device)


def test_process_rgb_fits_view_histogram_path(ctx, oracle):
    v = _check_rgb(ctx, oracle, _rgb((2048, 2051)), 4096, 512, True, offset=0)
    assert int(_u32(v.bins).astype(np.uint64).sum()) == v.stats[0].valid_count


@pytest.mark.parametrize("dead", [0, 2])
def test_process_rgb_fits_view_dead_channel(ctx, oracle, dead):
    v = _check_rgb(ctx, oracle, _rgb((67, 93), dead), 4096, 512, True)
    assert v.stats[dead].valid_count == 0 and not _host(v.rgb8)[..., dead].any()
    if dead == 0:
        assert not _u32(v.bins).any()


def test_process_rgb_fits_view_histogram_only_and_asynchronous(ctx):
    import torch
    planes = [_dev(p, 1) for p in _rgb((67, 93))]
    want = ctx.process_rgb_fits_view(*planes, hist_bins=512)
    only = ctx.process_rgb_fits_view(*planes, hist_bins=512, want_rgb8=False)      # out_rgb8 == NULL: one pass over R
    assert only.rgb8 is None and np.array_equal(_u32(only.bins), _u32(want.bins))
    rgb8 = torch.full((67, 93, 3), 0xAB, dtype=torch.uint8, device="cuda")
    bins, _ = _dev_bins(512)
    v = ctx.process_rgb_fits_view(*planes, hist_bins=512, fetch=False, out=rgb8, out_bins=bins)
    assert v.stats is None
    ctx.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(_host(rgb8), _host(want.rgb8)) and np.array_equal(_u32(bins), _u32(want.bins))


def test_process_rgb_fits_view_errors(ctx):
    r, g, b = _rgb((67, 93))
    cases = [((r, g, b[:, :90]), dict()), ((r, g[:60], b), dict()), ((r, g, b), dict(max_dim=0)),
             ((r, g, b), dict(hist_bins=0, want_rgb8=False))]
    for planes, kw in cases:
        with pytest.raises(AstroBurstError) as e:
            ctx.process_rgb_fits_view(*planes, **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
    # a device output over a device input plane (5 x 7: a head, whole four-pixel groups and loose pixels)
    import torch
    dev = [_dev(p) for p in _rgb((5, 7))]
    before = [d.clone() for d in dev]
    over = dev[1].view(-1).view(torch.uint8)[:5 * 7 * 3]
    with pytest.raises(AstroBurstError) as e:
        ctx.process_rgb_fits_view(*dev, hist_bins=0, out=over)
    assert e.value.code == _lib.AB_ERR_INVALID and "an output overlaps an input plane" in e.value.message
    assert all(torch.equal(d, x) for d, x in zip(dev, before))
    assert ctx.process_rgb_fits_view(r, g, b).rgb8.shape == (67, 93, 3)     # and the context still works
