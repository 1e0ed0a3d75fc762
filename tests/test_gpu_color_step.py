"""HIP parity of the compose wizard's blend and colour steps (csrc/wizard_color.hip) on one MI355X: ab_calibrate_and_scnr and
ab_blend_composite.

Two references per case, both compared with == (planes, bytes, valid_count, min, max, median, MAD, sigma, the STF parameters and the
routes are integers, f32 bit patterns or the same f64 scalar code); the mean alone is held to 1e-12 relative, the bar of
tests/test_gpu_stats_stf.py, because the reference leaves its summation order open:
  1 the library's own unfused chain: ab_calibrate_channel x 3 -> ab_apply_scnr_inplace -> ab_compute_image_stats as the command
    repeats it -> ab_compute_linked_stf -> ab_render_rgb_preview(stf x 3, stats); for the blend ab_resample_image ->
    ab_blend_channels -> ab_compute_image_stats x 3 -> the same tail;
  2 the oracle composition of tests/color_step_restatement.py.
The argument errors that carry a message need a live context and are here too (tests/test_color_step_cpu.py has the rest)."""
import functools

import numpy as np
import pytest

import color_step_restatement as R
from astroburst_amd import AstroBurstError, _lib
from test_gpu_stats_stf import sky_image

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
FACTORS = {"ones": (1.0, 1.0, 1.0), "mixed": (1.7, 0.6, 1.25), "0-nan-2": (0.0, NAN, 2.0)}
SCNRS = {"none": None, "1e-8": dict(method="average", amount=1e-8), "average": dict(method="average", amount=0.8),
         "max+preserve": dict(method="maximum", amount=1.0, preserve_luminance=True)}
POISON_F, POISON_B = -12345.5, 0xAB


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_host(a), dtype=F32).view(np.uint32)


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


def _dev_planes(shape, offset):
    """three poisoned device planes `offset` floats past a 16-byte boundary, with 16 floats of guard band on either side of each"""
    import torch
    n = shape[0] * shape[1]
    pitch = (n + 32 + 63) // 64 * 64
    buf = torch.full((3 * pitch + 64,), POISON_F, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    planes = [buf[c * pitch + 16 + offset:c * pitch + 16 + offset + n].view(shape) for c in range(3)]

    def guards_intact():
        h = _host(buf).copy()
        for c in range(3):
            h[c * pitch + 16 + offset:c * pitch + 16 + offset + n] = POISON_F
        return bool((h == F32(POISON_F)).all())
    return planes, guards_intact


def _dev_bytes(shape):
    """a poisoned device byte buffer that starts at an ODD address, with a guard band on either side"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), POISON_B, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    out = buf[17:17 + n]
    assert out.data_ptr() % 2 == 1
    return out, lambda: bool((_host(buf)[:17] == POISON_B).all() and (_host(buf)[17 + n:] == POISON_B).all())


def check_stats(got, ref):
    assert got.valid_count == ref.valid_count
    assert got.min == ref.min and got.max == ref.max
    assert got.median == ref.median, (got.median, ref.median)
    assert got.mad == ref.mad and got.sigma == ref.sigma
    assert abs(got.mean - ref.mean) <= 1e-12 * abs(ref.mean)


def check_stf(got, ref):
    assert (got.shadow, got.midtone, got.highlight) == (ref.shadow, ref.midtone, ref.highlight)


# ---- the cases: built once per module, read-only -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _composite(name):
    """(r, g, b) of one composite in the wizard's range -- around 0.25, stars above 1 -- so that every branch of SCNR is taken"""
    rows, cols = (int(v) for v in name.split("x"))
    rng = np.random.default_rng(rows * 97 + cols)
    out = []
    for gain in (1.0, 1.6, 0.7):         # G above the others: SCNR has green to remove
        if rows < 10:
            a = rng.uniform(0.05, 1.2, (rows, cols)).astype(F32) * F32(gain)
        else:
            a = sky_image(rng, rows, cols, pad=False) * F32(gain / 4000.0)
        if name == "67x93":              # a zero border, a NaN, both infinities and a negative pixel
            a[:2, :] = 0.0
            a[-2:, :] = 0.0
            a[:, :3] = 0.0
            a[:, -3:] = 0.0
            a[10, 11] = np.nan
            a[20, 21] = np.inf
            a[30, 31] = -np.inf
            a[40, 41] = -0.5
        a = np.ascontiguousarray(a, dtype=F32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _orig_stats(name):
    from oracle import pyoracle
    return tuple(pyoracle.compute_image_stats(p) for p in _composite(name))


@functools.lru_cache(maxsize=None)
def _device_composite(name, offset):
    return tuple(_dev(p, offset) for p in _composite(name))


@functools.lru_cache(maxsize=None)
def _oracle_color(name, fkey, skey, max_dim):
    from oracle import pyoracle
    planes, rgb8, stats, linked, applied = R.calibrate_and_scnr(pyoracle, *_composite(name), _orig_stats(name), FACTORS[fkey], SCNRS[skey], max_dim)
    for a in (*planes, rgb8):
        a.setflags(write=False)
    return tuple(planes), rgb8, tuple(stats), linked, applied


def _unfused_color(ctx, dplanes, orig_stats, factors, scnr, max_dim):
    """today's chain of older entry points, statement for statement the command (color.rs:115-168)"""
    planes, stats = [], []
    for x, f, s in zip(dplanes, factors, orig_stats):
        p, st = ctx.calibrate_channel(x, float(R.factor_f32(f)), s)
        planes.append(p), stats.append(st)
    if R.scnr_applied(scnr):
        ctx.apply_scnr_inplace(*planes, method=scnr["method"], amount=scnr["amount"], preserve_luminance=scnr.get("preserve_luminance", False))
        if scnr.get("preserve_luminance", False):
            stats = [ctx.compute_image_stats(p) for p in planes]
        else:
            stats[1] = ctx.compute_image_stats(planes[1])
    linked, _ = ctx.compute_linked_stf(*stats)
    rgb8 = ctx.render_rgb_preview(*planes, max_dim, stf=[linked] * 3, stats=stats)
    return planes, rgb8, stats, linked


def _check_color(ctx, name, fkey, skey, max_dim, on_device=True, in_offset=1, out_offset=1):
    factors, scnr = FACTORS[fkey], SCNRS[skey]
    planes, orig_stats = _composite(name), _orig_stats(name)
    shape = planes[0].shape
    dplanes = _device_composite(name, in_offset)
    want_plan = R.plan(planes[0].size, orig_stats, factors, scnr)
    ph, pw = ctx.preview_dims(*shape, max_dim)
    if on_device:
        outs, planes_guarded = _dev_planes(shape, out_offset)
        rgb8, bytes_guarded = _dev_bytes((ph, pw, 3))
        res = ctx.calibrate_and_scnr(*dplanes, orig_stats, factors, scnr, max_dim=max_dim, out=rgb8, out_planes=outs)
        assert planes_guarded() and bytes_guarded()
    else:
        res = ctx.calibrate_and_scnr(*planes, orig_stats, factors, scnr, max_dim=max_dim)
        assert all(isinstance(p, np.ndarray) for p in res.planes) and isinstance(res.rgb8, np.ndarray)
    assert (res.rows, res.cols) == shape and (res.preview_rows, res.preview_cols) == (ph, pw)
    assert res.factors == want_plan.factors and res.scnr_applied == want_plan.scnr_applied and res.route == want_plan.route
    # 1: the library's own unfused chain
    u_planes, u_rgb8, u_stats, u_linked = _unfused_color(ctx, dplanes, orig_stats, factors, scnr, max_dim)
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(u_planes[c])), c
        check_stats(res.stats[c], u_stats[c])
    check_stf(res.stf, u_linked)
    assert np.array_equal(_host(res.rgb8).reshape(ph, pw, 3), _host(u_rgb8))
    # 2: the oracle composition
    o_planes, o_rgb8, o_stats, o_linked, o_applied = _oracle_color(name, fkey, skey, max_dim)
    assert res.scnr_applied == o_applied
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(o_planes[c])), c
        check_stats(res.stats[c], o_stats[c])
    check_stf(res.stf, o_linked)
    assert np.array_equal(_host(res.rgb8).reshape(ph, pw, 3), o_rgb8)
    return res


# ---- ab_calibrate_and_scnr: small shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skey", list(SCNRS))
@pytest.mark.parametrize("fkey", list(FACTORS))
def test_color_step_3x5_host(ctx, fkey, skey):
    """3 x 5 host planes: less than one wave, host outputs through the one synchronisation"""
    _check_color(ctx, "3x5", fkey, skey, 4096, on_device=False)


@pytest.mark.parametrize("max_dim", [4096, 37])
@pytest.mark.parametrize("skey", list(SCNRS))
@pytest.mark.parametrize("fkey", list(FACTORS))
def test_color_step_67x93_device(ctx, fkey, skey, max_dim):
    """device planes one float past a 16-byte boundary, with a NaN, both infinities, a negative pixel and a zero border"""
    res = _check_color(ctx, "67x93", fkey, skey, max_dim)
    if fkey == "ones" and skey == "none":          # nothing changes a pixel: NaN and the infinities reach the planes as they are
        assert np.array_equal(_bits(res.planes[0]), _bits(_composite("67x93")[0]))


@pytest.mark.parametrize("max_dim", [4096, 128])
@pytest.mark.parametrize("skey", list(SCNRS))
@pytest.mark.parametrize("fkey", list(FACTORS))
def test_color_step_300x400_device(ctx, fkey, skey, max_dim):
    res = _check_color(ctx, "300x400", fkey, skey, max_dim, in_offset=0, out_offset=0)
    if skey == "max+preserve" and fkey != "0-nan-2":   # the luminance branch ran (G's loss exceeds 1e-10 unless G is scaled by 1e-6): R differs from the scaled R
        scaled = _composite("300x400")[0] * R.factor_f32(FACTORS[fkey][0])
        assert not np.array_equal(_bits(res.planes[0]), _bits(scaled))


def test_color_step_mixed_alignment(ctx):
    """inputs one float past a 16-byte boundary, outputs two past: no 16-byte access fits all six planes"""
    _check_color(ctx, "67x93", "mixed", "average", 4096, in_offset=1, out_offset=2)
    _check_color(ctx, "67x93", "mixed", "max+preserve", 37, in_offset=3, out_offset=0)


# ---- ab_calibrate_and_scnr: the 4 000 000 px threshold ---------------------------------------------------------------------------------
THRESHOLD_CASES = [("mixed", "none"), ("mixed", "1e-8"), ("mixed", "average"), ("mixed", "max+preserve"), ("0-nan-2", "none"), ("ones", "average")]


def test_known_range_precondition(oracle):
    """only if the known-range statistics of the scaled R plane differ from its full statistics does a wrong route fail the tests below
    (CPU, the oracle alone)"""
    r = _composite("2000x2001")[0]
    assert r.size == 4_002_000
    scaled, known = oracle.calibrate_channel(r, float(R.factor_f32(1.7)), _orig_stats("2000x2001")[0])
    full = oracle.compute_image_stats(scaled)
    assert known.median != full.median or known.mad != full.mad, (known, full)


@pytest.mark.parametrize("fkey,skey", THRESHOLD_CASES)
def test_color_step_exactly_4000000_px(ctx, fkey, skey):
    res = _check_color(ctx, "2000x2000", fkey, skey, 4096, in_offset=0, out_offset=0)
    assert res.route == (R.EXACT_OR_FULL,) * 3


@pytest.mark.parametrize("fkey,skey", THRESHOLD_CASES)
def test_color_step_smallest_known_range_shape(ctx, fkey, skey):
    res = _check_color(ctx, "2000x2001", fkey, skey, 4096, in_offset=0, out_offset=0)
    want = {"none": (1, 1, 1), "1e-8": (1, 1, 1), "average": (1, 0, 1), "max+preserve": (0, 0, 0)}[skey]
    assert res.route == want


# ---- ab_calibrate_and_scnr: forms and errors -----------------------------------------------------------------------------------------------
def test_color_step_asynchronous_form(ctx):
    import torch
    name, shape = "67x93", (67, 93)
    dplanes, orig_stats = _device_composite(name, 1), _orig_stats(name)
    want = ctx.calibrate_and_scnr(*dplanes, orig_stats, FACTORS["mixed"], SCNRS["average"], max_dim=37)
    outs, planes_guarded = _dev_planes(shape, 1)
    rgb8, bytes_guarded = _dev_bytes((want.preview_rows, want.preview_cols, 3))
    res = ctx.calibrate_and_scnr(*dplanes, orig_stats, FACTORS["mixed"], SCNRS["average"], max_dim=37, fetch=False, out=rgb8, out_planes=outs)
    assert res.stats is None and res.stf is None and res.route is None
    ctx.synchronize()
    torch.cuda.synchronize()
    assert planes_guarded() and bytes_guarded()
    for c in range(3):
        assert np.array_equal(_bits(outs[c]), _bits(want.planes[c]))
    assert np.array_equal(_host(rgb8).reshape(_host(want.rgb8).shape), _host(want.rgb8))


def test_color_step_planes_only(ctx):
    dplanes, orig_stats = _device_composite("67x93", 1), _orig_stats("67x93")
    want = ctx.calibrate_and_scnr(*dplanes, orig_stats, FACTORS["mixed"], SCNRS["average"])
    res = ctx.calibrate_and_scnr(*dplanes, orig_stats, FACTORS["mixed"], SCNRS["average"], want_rgb8=False)      # out_rgb8 == NULL
    assert res.rgb8 is None
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(want.planes[c]))
        check_stats(res.stats[c], want.stats[c])
    check_stf(res.stf, want.stf)


def test_color_step_errors(ctx):
    r, g, b = _composite("67x93")
    st = _orig_stats("67x93")
    d = _device_composite("67x93", 1)
    cases = [((r, g, b[:, :90]), dict()), ((r, g[:60], b), dict()), ((r, g, b), dict(max_dim=0)), ((r, g, b), dict(max_dim=-4)),
             ((r, g, b), dict(out_planes=[np.zeros((67, 92), F32)] * 3)),
             (d, dict(out_planes=[d[0], d[1], d[2]])),                                           # an output overlaps an input
             (d, dict(out_planes=[_dev(r, 1)] * 3))]                                              # two outputs overlap
    for planes, kw in cases:
        with pytest.raises(AstroBurstError) as e:
            ctx.calibrate_and_scnr(*planes, st, (1.0, 1.0, 1.0), **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
    assert ctx.calibrate_and_scnr(r, g, b, st, (1.0, 1.0, 1.0)).rgb8.shape == (67, 93, 3)         # and the context still works


# ---- ab_blend_composite --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _channels(k, mixed_dims=False, with_nan=False):
    rng = np.random.default_rng(1000 + k + 10 * mixed_dims + 100 * with_nan)
    out = []
    for i in range(k):
        shape = (40, 50) if (mixed_dims and i % 2 == 0) else (67, 93)
        a = (sky_image(rng, *shape, pad=False) * F32((1.0 + 0.3 * i) / 4000.0)).astype(F32)
        if with_nan and i == 0:
            a[5, 6] = np.nan
        a = np.ascontiguousarray(a)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _weights(k, out_of_range=False):
    w = [(i, 1.0 / (1 + i), 0.5 if i % 2 else 0.25, 0.1 * (i + 1)) for i in range(k)]
    if out_of_range:
        w.insert(1, (k, 5.0, 5.0, 5.0))            # channel_idx == n_channels: skipped (channel_blend.rs:20-23)
        w.append((k + 40, 9.0, 9.0, 9.0))
    return w


def _unfused_blend(ctx, dchans, weights, max_dim):
    rows, cols = max(c.shape[0] for c in dchans), max(c.shape[1] for c in dchans)
    arrays = [ctx.resample_image(c, rows, cols) if tuple(c.shape) != (rows, cols) else c for c in dchans]
    planes = ctx.blend_channels(arrays, weights, rows, cols)
    stats = [ctx.compute_image_stats(p) for p in planes]
    linked, _ = ctx.compute_linked_stf(*stats)
    return planes, ctx.render_rgb_preview(*planes, max_dim, stf=[linked] * 3, stats=stats), stats, linked


def _check_blend(ctx, oracle, chans, weights, max_dim, on_device=True):
    rows, cols = max(c.shape[0] for c in chans), max(c.shape[1] for c in chans)
    dchans = [_dev(c, 1) for c in chans]
    before = [_bits(c).copy() for c in dchans]
    ph, pw = ctx.preview_dims(rows, cols, max_dim)
    if on_device:
        outs, planes_guarded = _dev_planes((rows, cols), 1)
        rgb8, bytes_guarded = _dev_bytes((ph, pw, 3))
        res = ctx.blend_composite(dchans, weights, max_dim=max_dim, out=rgb8, out_planes=outs)
        assert planes_guarded() and bytes_guarded()
    else:
        res = ctx.blend_composite(list(chans), weights, max_dim=max_dim)
    assert (res.rows, res.cols, res.preview_rows, res.preview_cols) == (rows, cols, ph, pw)
    assert all(np.array_equal(_bits(c), b) for c, b in zip(dchans, before))                    # the originals are untouched
    u_planes, u_rgb8, u_stats, u_linked = _unfused_blend(ctx, dchans, weights, max_dim)
    o_planes, o_rgb8, o_stats, o_linked, o_resampled = R.blend_composite(oracle, list(chans), weights, max_dim)
    assert res.resampled == o_resampled
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(u_planes[c])) and np.array_equal(_bits(res.planes[c]), _bits(o_planes[c])), c
        check_stats(res.stats[c], u_stats[c])
        check_stats(res.stats[c], o_stats[c])
    check_stf(res.stf, u_linked)
    check_stf(res.stf, o_linked)
    got = _host(res.rgb8).reshape(ph, pw, 3)
    assert np.array_equal(got, _host(u_rgb8)) and np.array_equal(got, o_rgb8)
    return res


@pytest.mark.parametrize("max_dim", [4096, 37])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_blend_composite(ctx, oracle, k, max_dim):
    res = _check_blend(ctx, oracle, _channels(k), _weights(k), max_dim)
    assert not res.resampled


def test_blend_composite_host(ctx, oracle):
    _check_blend(ctx, oracle, _channels(3), _weights(3), 4096, on_device=False)


def test_blend_composite_weight_out_of_range(ctx, oracle):
    res = _check_blend(ctx, oracle, _channels(3), _weights(3, out_of_range=True), 4096)
    same = ctx.blend_composite(list(_channels(3)), _weights(3), want_rgb8=False)
    for c in range(3):
        assert np.array_equal(_bits(res.planes[c]), _bits(same.planes[c]))


@pytest.mark.parametrize("max_dim", [4096, 37])
def test_blend_composite_resample_branch(ctx, oracle, max_dim):
    """channels of 40 x 50 and 67 x 93 together: the small ones are resampled to 67 x 93"""
    res = _check_blend(ctx, oracle, _channels(3, mixed_dims=True), _weights(3), max_dim)
    assert res.resampled and (res.rows, res.cols) == (67, 93)


def test_blend_composite_largest_rows_and_largest_cols(ctx, oracle):
    """the output has the largest rows and the largest cols, which no single channel need have (blend.rs:149-150)"""
    rng = np.random.default_rng(5)
    chans = (rng.uniform(0.1, 0.9, (30, 80)).astype(F32), rng.uniform(0.1, 0.9, (60, 40)).astype(F32))
    res = _check_blend(ctx, oracle, chans, _weights(2), 4096)
    assert res.resampled and (res.rows, res.cols) == (60, 80)


def test_blend_composite_nan_reaches_the_planes(ctx, oracle):
    res = _check_blend(ctx, oracle, _channels(3, with_nan=True), _weights(3), 4096)
    for c in range(3):
        assert np.isnan(_host(res.planes[c])[5, 6]) and np.isnan(_host(res.planes[c])).sum() == 1


def test_blend_composite_asynchronous_form(ctx):
    import torch
    dchans = [_dev(c, 1) for c in _channels(3, mixed_dims=True)]
    want = ctx.blend_composite(dchans, _weights(3), max_dim=37)
    outs, planes_guarded = _dev_planes((67, 93), 1)
    rgb8, bytes_guarded = _dev_bytes((want.preview_rows, want.preview_cols, 3))
    res = ctx.blend_composite(dchans, _weights(3), max_dim=37, fetch=False, out=rgb8, out_planes=outs)
    assert res.stats is None and res.stf is None and res.resampled is None
    ctx.synchronize()
    torch.cuda.synchronize()
    assert planes_guarded() and bytes_guarded()
    for c in range(3):
        assert np.array_equal(_bits(outs[c]), _bits(want.planes[c]))
    assert np.array_equal(_host(rgb8).reshape(_host(want.rgb8).shape), _host(want.rgb8))


def test_blend_composite_errors(ctx):
    with pytest.raises(AstroBurstError) as e:
        ctx.blend_composite([], [])
    assert e.value.code == _lib.AB_ERR_INVALID and e.value.message == "No channel paths provided"      # blend.rs:139-141
    chans = list(_channels(3))
    cases = [dict(max_dim=0), dict(out_planes=[np.zeros((67, 92), F32)] * 3)]
    for kw in cases:
        with pytest.raises(AstroBurstError) as e:
            ctx.blend_composite(chans, _weights(3), **kw)
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message, kw
    with pytest.raises(AstroBurstError) as e:
        ctx.blend_composite(chans * 6, _weights(3))                                                     # 18 channels
    assert e.value.code == _lib.AB_ERR_INVALID
    assert ctx.blend_composite(chans, _weights(3)).rgb8.shape == (67, 93, 3)                            # and the context still works
