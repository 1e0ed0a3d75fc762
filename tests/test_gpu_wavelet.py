"""GPU a trous wavelet denoising (core/imaging/wavelet.rs, csrc/wavelet.hip) against the numpy restatement (tests/wavelet_restatement.py).

Bar: BIT-EXACT.  The reference computes every pixel in f32, one multiply and one add per tap in a fixed order, and the library is
built with -ffp-contract=off, so the output plane is compared through its uint32 view, noise_estimate with == as an f64 and
scales_processed as an integer.  No tolerance anywhere: a mismatch is a bug, not noise."""
import os

import numpy as np
import pytest

import wavelet_restatement as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (1, 77), (65, 1), (33, 65), (100, 129), (257, 63), (300, 517)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def noisy(rows, cols, seed=0, sky=300.0, sigma=20.0):
    """sky + Gaussian noise + a few bright blobs, all positive"""
    rng = np.random.default_rng(seed)
    img = rng.normal(sky, sigma, (rows, cols))
    for _ in range(max(1, rows * cols // 4000)):
        cy, cx, amp, s = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(200.0, 20000.0), rng.uniform(1.0, 4.0)
        yy, xx = np.mgrid[0:rows, 0:cols]
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return img.astype(F32)


def check(ctx, img, num_scales=5, thresholds=R.DEFAULT_THRESHOLDS, linear_denoise=True):
    got, scales, sigma = ctx.wavelet_denoise(img, num_scales, thresholds, linear_denoise)
    want, wscales, wsigma = R.wavelet_denoise(img, num_scales, thresholds, linear_denoise)
    assert got.shape == img.shape and got.dtype == np.float32
    assert isinstance(scales, int) and scales == wscales, (scales, wscales)
    assert sigma == wsigma, (sigma, wsigma)
    differ = bits(got) != bits(want)
    assert not differ.any(), (int(differ.sum()), np.argwhere(differ)[:4].tolist(), got[differ][:4], want[differ][:4])
    return got, scales, sigma


@pytest.mark.parametrize("num_scales", range(1, 9))
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes_and_scales(ctx, rows, cols, num_scales):
    check(ctx, noisy(rows, cols, seed=rows * 7 + cols), num_scales)


@pytest.mark.parametrize("num_scales,clamped", [(0, 1), (12, 8)])
def test_num_scales_is_clamped(ctx, num_scales, clamped):
    _, scales, _ = check(ctx, noisy(100, 129, seed=1), num_scales)
    assert scales == clamped


@pytest.mark.parametrize("linear_denoise", [True, False])
@pytest.mark.parametrize("num_scales", [4, 8])
@pytest.mark.parametrize("kind", ["empty", "one", "s_minus_2", "twelve"])
def test_threshold_list_lengths(ctx, kind, num_scales, linear_denoise):
    full = [3.0, 2.5, 2.0, 1.5, 1.0, 0.75, 0.5, 0.25, 9.0, 8.0, 7.0, 6.0]
    th = {"empty": [], "one": [2.25], "s_minus_2": full[:num_scales - 2], "twelve": full}[kind]
    check(ctx, noisy(100, 129, seed=2), num_scales, th, linear_denoise)


@pytest.mark.parametrize("linear_denoise", [True, False])
@pytest.mark.parametrize("thresholds", [[0.0] * 5, [-1.0, -0.5, 3.0, -2.0, 1.0], [3.0, float("nan"), 2.0, 1.5, 1.0], [float("nan")] * 5])
def test_zero_negative_and_nan_thresholds(ctx, thresholds, linear_denoise):
    check(ctx, noisy(100, 129, seed=3), 5, thresholds, linear_denoise)


def test_soft_and_hard_differ_on_every_pixel_of_a_noisy_plane(ctx):
    """(a build that ignores linear_denoise cannot pass both modes of the other tests: the restatement's two modes share no pixel)"""
    img = np.random.default_rng(4).normal(1000.0, 50.0, (100, 129)).astype(F32)
    # low thresholds: (almost) no detail is zeroed, and a soft-thresholded detail differs from the hard one by the threshold
    th = [0.01] * 5
    soft, _, _ = check(ctx, img, 5, th, True)
    hard, _, _ = check(ctx, img, 5, th, False)
    want_soft = R.wavelet_denoise(img, 5, th, True)[0]
    want_hard = R.wavelet_denoise(img, 5, th, False)[0]
    assert (bits(want_soft) != bits(want_hard)).mean() > 0.99
    assert (bits(soft) != bits(hard)).mean() > 0.99


@pytest.mark.parametrize("rows,cols", [(33, 65), (100, 129), (64, 64), (100, 130)])
def test_even_and_odd_counts_of_finite_details(ctx, rows, cols):
    """an odd-sized plane has an odd count; an even-sized one an even count (the f32 averaged median)"""
    img = noisy(rows, cols, seed=5)
    _, _, sigma = check(ctx, img, 3)
    d0 = img - R.atrous_smooth(img, 1)
    assert np.isfinite(d0).sum() % 2 == (rows * cols) % 2 and sigma > 0


def test_single_nan_pixel_leaves_an_odd_count(ctx):
    """one NaN in the interior of an even-sized plane poisons its 5 x 5 footprint of d_0: 64 * 64 - 25 finite details, an odd count"""
    img = noisy(64, 64, seed=6)
    img[30, 31] = np.nan
    d0 = img - R.atrous_smooth(img, 1)
    assert int(np.isfinite(d0).sum()) == 64 * 64 - 25
    got, _, sigma = check(ctx, img, 4)
    assert np.isfinite(got).all() and sigma > 0 and got[30, 31] == 0.0


@pytest.mark.parametrize("num_scales", [1, 5, 8])
@pytest.mark.parametrize("linear_denoise", [True, False])
def test_nan_and_inf_pixels_spread_through_the_footprint_and_come_out_zero(ctx, num_scales, linear_denoise):
    img = noisy(100, 129, seed=7)
    clean_sigma = R.wavelet_denoise(img, num_scales)[2]
    img[10, 12] = np.nan
    img[70, 100] = np.inf
    img[99, 0] = np.inf
    got, _, sigma = check(ctx, img, num_scales, R.DEFAULT_THRESHOLDS, linear_denoise)
    assert np.isfinite(got).all() and np.isfinite(sigma) and abs(sigma - clean_sigma) < 0.05 * clean_sigma
    assert got[10, 12] == 0.0 and got[70, 100] == 0.0 and got[99, 0] == 0.0
    assert got[8, 10] == 0.0 and got[12, 14] == 0.0  # the first scale's footprint of the NaN


def test_all_non_finite_plane(ctx):
    img = np.full((20, 30), np.nan, F32)
    got, _, sigma = check(ctx, img, 3)
    assert sigma == 0.0 and not got.any()


@pytest.mark.parametrize("linear_denoise", [True, False])
def test_subnormal_inputs(ctx, linear_denoise):
    """|pixels| ~ 1e-40: every product and sum is subnormal -- flushing denormals anywhere changes the bits"""
    rng = np.random.default_rng(8)
    img = (rng.uniform(0.5, 2.0, (100, 129)) * 1e-40).astype(F32)
    assert (img != 0).all() and (np.abs(img) < np.finfo(F32).tiny).all()
    got, _, sigma = check(ctx, img, 5, [0.0] * 5, linear_denoise)
    assert sigma > 0.0 and got.any()
    check(ctx, img, 5, R.DEFAULT_THRESHOLDS, linear_denoise)


def test_constant_plane(ctx):
    img = np.full((100, 129), 1234.5, F32)
    got, scales, sigma = check(ctx, img, 5)
    assert sigma == 0.0 and scales == 5
    assert np.array_equal(bits(got), bits(img))


def test_all_negative_plane(ctx):
    img = -noisy(100, 129, seed=9)
    got, _, sigma = check(ctx, img, 5)
    assert sigma > 0 and not got.any() and not np.signbit(got).any()


def test_host_device_and_torch_planes_agree_and_are_deterministic(ctx):
    import torch
    img = noisy(300, 517, seed=10)
    host, s, sigma = check(ctx, img, 8)
    dev, s_d, sigma_d = ctx.wavelet_denoise(torch.from_numpy(img).cuda(), 8)
    assert dev.is_cuda
    cpu_t, s_t, sigma_t = ctx.wavelet_denoise(torch.from_numpy(img), 8)
    again, s_a, sigma_a = ctx.wavelet_denoise(img, 8)
    into = torch.empty((300, 517), device="cuda")
    ret, s_o, sigma_o = ctx.wavelet_denoise(torch.from_numpy(img).cuda(), 8, out=into)
    assert ret is into
    assert s == s_d == s_t == s_a == s_o == 8 and sigma == sigma_d == sigma_t == sigma_a == sigma_o
    for other in (dev.cpu().numpy(), np.asarray(cpu_t), again, into.cpu().numpy()):
        assert np.array_equal(bits(host), bits(other))


def test_unaligned_device_planes(ctx):
    """planes that start 4 bytes into an allocation: the float4 paths must not be taken"""
    import torch
    img = noisy(96, 128, seed=11)
    want = R.wavelet_denoise(img, 6)[0]
    src = torch.empty(96 * 128 + 1, device="cuda")[1:].view(96, 128)
    src.copy_(torch.from_numpy(img))
    dst = torch.empty(96 * 128 + 1, device="cuda")[1:].view(96, 128)
    ctx.wavelet_denoise(src, 6, out=dst)
    assert np.array_equal(bits(dst.cpu().numpy()), bits(want))
    aligned, _, _ = ctx.wavelet_denoise(torch.from_numpy(img).cuda(), 6)
    assert np.array_equal(bits(aligned.cpu().numpy()), bits(want))


def _raw(ctx, img_plane, cfg, out_plane, res):
    import ctypes as C
    return ctx._L.ab_wavelet_denoise(ctx._h, C.byref(img_plane) if img_plane is not None else None, C.byref(cfg) if cfg is not None else None,
                                     C.byref(out_plane) if out_plane is not None else None, C.byref(res) if res is not None else None)


def test_invalid_arguments(ctx):
    import ctypes as C
    import torch
    import astroburst_amd as ab
    from astroburst_amd import _lib
    img = noisy(20, 30, seed=12)
    # through the Python layer: wrong output dims, overlapping planes, an empty image
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.wavelet_denoise(img, out=torch.empty((20, 31), device="cuda"))
    assert e.value.code == _lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.wavelet_denoise(img, out=np.empty((21, 30), F32))
    assert e.value.code == _lib.AB_ERR_INVALID
    d = torch.from_numpy(img).cuda()
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.wavelet_denoise(d, out=d)
    assert e.value.code == _lib.AB_ERR_INVALID
    big = torch.zeros(20 * 30 + 30, device="cuda")
    with pytest.raises(ab.AstroBurstError) as e:  # partial overlap: shifted by one row
        ctx.wavelet_denoise(big[:600].view(20, 30), out=big[30:].view(20, 30))
    assert e.value.code == _lib.AB_ERR_INVALID
    for shape in ((0, 4), (4, 0)):
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.wavelet_denoise(np.zeros(shape, F32))
        assert e.value.code == _lib.AB_ERR_INVALID
    # through the C ABI: null arguments, null data, a count without a list, 2^31 pixels
    out = np.empty_like(img)
    pi = _lib.Plane(C.c_void_p(img.ctypes.data), 20, 30, 0)
    po = _lib.Plane(C.c_void_p(out.ctypes.data), 20, 30, 0)
    cfg = _lib.WaveletConfigC(5, None, 0, 1)
    res = _lib.WaveletResultC()
    assert _raw(ctx, pi, cfg, po, res) == _lib.AB_OK and res.scales_processed == 5
    assert np.array_equal(bits(out), bits(R.wavelet_denoise(img, 5, [])[0]))
    assert ctx._L.ab_wavelet_denoise(None, C.byref(pi), C.byref(cfg), C.byref(po), C.byref(res)) == _lib.AB_ERR_INVALID
    for args in ((None, cfg, po, res), (pi, None, po, res), (pi, cfg, None, res), (pi, cfg, po, None)):
        assert _raw(ctx, *args) == _lib.AB_ERR_INVALID
    assert _raw(ctx, _lib.Plane(None, 20, 30, 0), cfg, po, res) == _lib.AB_ERR_INVALID
    assert _raw(ctx, pi, cfg, _lib.Plane(None, 20, 30, 0), res) == _lib.AB_ERR_INVALID
    assert _raw(ctx, pi, _lib.WaveletConfigC(5, None, 3, 1), po, res) == _lib.AB_ERR_INVALID
    for rows, cols in ((1 << 16, 1 << 15), (1 << 31, 1), (1, 1 << 31), (46341, 46341)):  # >= 2^31 pixels: rejected before any byte is read
        huge_i = _lib.Plane(C.c_void_p(img.ctypes.data), rows, cols, 0)
        huge_o = _lib.Plane(C.c_void_p(out.ctypes.data), rows, cols, 0)
        assert _raw(ctx, huge_i, cfg, huge_o, res) == _lib.AB_ERR_INVALID
    assert _raw(ctx, pi, cfg, po, res) == _lib.AB_OK  # the context is still usable


def test_cancel_and_progress(ctx):
    import astroburst_amd as ab
    img = noisy(50, 60, seed=13)
    ctx.request_cancel()
    try:
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.wavelet_denoise(img)
        assert e.value.code == ab._lib.AB_ERR_CANCELLED
    finally:
        ctx.clear_cancel()
    for num_scales in (1, 5, 8, 12):
        ticks = []
        ctx.set_progress_cb(lambda stage, cur, tot: ticks.append((stage, cur, tot)))
        try:
            _, scales, _ = ctx.wavelet_denoise(img, num_scales)
        finally:
            ctx.set_progress_cb(None)
        stages = R.progress_stages(num_scales)
        assert len(stages) == 2 * scales + 1
        assert ticks == [(s, i + 1, 2 * scales + 1) for i, s in enumerate(stages)], ticks
        assert ticks[-1] == ("reconstructing", 2 * scales + 1, 2 * scales + 1)


def test_cancel_from_a_tick_stops_at_that_stage(ctx):
    import astroburst_amd as ab
    img = noisy(50, 60, seed=14)
    ticks = []

    def cb(stage, cur, tot):
        ticks.append(stage)
        if stage == "thresholding scale 2/5":
            ctx.request_cancel()

    ctx.set_progress_cb(cb)
    try:
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.wavelet_denoise(img)
        assert e.value.code == ab._lib.AB_ERR_CANCELLED
    finally:
        ctx.set_progress_cb(None)
        ctx.clear_cancel()
    assert ticks[-1] == "thresholding scale 2/5" and "reconstructing" not in ticks
    check(ctx, img)  # and the context works again


# ---- both kernel forms (developer library: the hand-over between them is an ab_dev_env switch) -----------------------------------
def _under(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("rows,cols", SHAPES + [(64, 64), (130, 256)])
def test_fused_and_two_pass_forms_agree_bit_for_bit(ctx, dev_build, rows, cols):
    """the two-pass form at every step (what the release library runs) and every step the fused kernel can take (.. 32) through it,
    at several tile heights: identical bits, and the restatement's"""
    img = noisy(rows, cols, seed=rows + cols)
    img[rows // 2, cols // 3] = np.nan
    want, _, wsigma = R.wavelet_denoise(img, 8)
    default = ctx.wavelet_denoise(img, 8)
    runs = [default, _under({"AB_WAVELET_FUSED_MAX_STEP": "0"}, lambda: ctx.wavelet_denoise(img, 8))]
    for tile_rows in ("16", "32", "64", "128"):
        runs.append(_under({"AB_WAVELET_FUSED_MAX_STEP": "32", "AB_WAVELET_TILE_ROWS": tile_rows}, lambda: ctx.wavelet_denoise(img, 8)))
    for got, scales, sigma in runs:
        assert scales == 8 and sigma == wsigma
        assert np.array_equal(bits(got), bits(want))


# ---- full size -------------------------------------------------------------------------------------------------------------------
def _full_size_plane():
    rng = np.random.default_rng(15)
    img = rng.normal(300.0, 20.0, (4096, 4096)).astype(F32)
    img[1000:1016, 2000:2016] += 30000.0
    img[17, 4000] = np.nan
    return img


@pytest.mark.parametrize("num_scales", [5, 8])
def test_full_size_4096(ctx, num_scales):
    import torch
    dev = torch.from_numpy(_full_size_plane()).cuda()
    got, scales, sigma = ctx.wavelet_denoise(dev, num_scales)
    want, wscales, wsigma = R.wavelet_denoise_torch(dev, num_scales, device="cuda")
    assert scales == wscales == num_scales and sigma == wsigma, (scales, wscales, sigma, wsigma)
    differ = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(differ.any()), int(differ.sum())
    assert bool(torch.isfinite(got).all()) and sigma > 0


@pytest.mark.parametrize("fused_max_step", ["0", "1", "4", "16", "32"])
def test_full_size_4096_through_both_forms(ctx, dev_build, fused_max_step):
    """the 4096^2 plane with 8 scales through the two-pass form at every step (0), through the fused form up to step 32, and through
    hand-overs in between: the torch restatement's bits each time"""
    import torch
    dev = torch.from_numpy(_full_size_plane()).cuda()
    want, _, wsigma = R.wavelet_denoise_torch(dev, 8, device="cuda")
    got, scales, sigma = _under({"AB_WAVELET_FUSED_MAX_STEP": fused_max_step}, lambda: ctx.wavelet_denoise(dev, 8))
    assert scales == 8 and sigma == wsigma
    assert not bool((got.view(torch.int32) != want.view(torch.int32)).any())
