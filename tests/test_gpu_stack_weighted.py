"""GPU: ab_stack_weighted against tests/weighted_stack_restatement.py -- image and weight plane bit for bit (the NaN pattern included:
neither may hold one), the rejected count equal.  Small planes; the restatement of a case is computed once."""
import numpy as np
import pytest

import weighted_stack_restatement as wsr

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def make_frames(rng, n, rows, cols, nan_rate=0.01, cr_rate=0.01, zero_border=True, scale=1.0):   # tests/test_gpu_stack.py's recipe
    base = 1000.0 + 50.0 * rng.standard_normal((rows, cols))
    frames = []
    for k in range(n):
        f = (base + 12.0 * rng.standard_normal((rows, cols))).astype(np.float32) * np.float32(scale)
        hit = rng.random((rows, cols)) < cr_rate
        f[hit] *= rng.uniform(20, 50, hit.sum()).astype(np.float32)
        bad = rng.random((rows, cols)) < nan_rate
        f[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), bad.sum())
        if zero_border and k % 3 == 2:
            f[:2, :] = 0.0
            f[:, -3:] = 0.0
        frames.append(f)
    return frames


def random_params(rng, n):
    """weights in (0, 1], scales near 1, offsets of either sign; every third frame is read as it is"""
    w = 1.0 - rng.random(n)
    s = (1.0 + 0.05 * rng.standard_normal(n)).astype(np.float32)
    o = (30.0 * rng.standard_normal(n)).astype(np.float32)
    s[::3] = 1.0
    o[::3] = 0.0
    return w, s, o


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError(f"{what}: {bad.sum()} of {got.size} differ; first {idx.tolist()}: {[(got[tuple(i)], want[tuple(i)]) for i in idx]}")


def check(ctx, frames, w, s=None, o=None, sl=3.0, sh=3.0, it=5):
    """one call with the weight plane against the restatement -> what the library returned"""
    got, gw, rej = ctx.stack_weighted(frames, w, s, o, sl, sh, it, want_weight=True)
    want, ww, want_rej = wsr.stack_weighted(frames, w, s, o, sl, sh, it)
    assert_bits(got, want, "image")
    assert_bits(gw, ww, "weight plane")
    assert rej == want_rej
    return got, gw, rej


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64])
def test_every_padded_count_and_its_neighbour(ctx, n):
    """37 x 131 is no multiple of 64 pixels (the last wave is partly filled, the last block partly empty); every NP = 2 .. 64 and the
    count one above or below it"""
    rng = np.random.default_rng(700 + n)
    frames = make_frames(rng, n, 37, 131)
    w, s, o = random_params(rng, n)
    _, _, rej = check(ctx, frames, w, s, o)
    assert rej > 0 or n == 2                                    # (two samples: the MAD is their distance, nothing is ever clipped)
    assert ctx.stack_last_kernel_ms() > 0 and ctx.last_rejected() == rej


@pytest.mark.parametrize("sl,sh,it", [(3.0, 3.0, 0), (3.0, 3.0, 1), (2.0, 2.0, 5), (1.0, 4.0, 3), (0.5, 0.5, 10),
                                      (0.0, 0.0, 5), (-1.0, 3.0, 5), (3.0, INF, 5), (NAN, 3.0, 2)])
def test_parameter_sweep(ctx, sl, sh, it):
    rng = np.random.default_rng(5)
    frames = make_frames(rng, 12, 24, 70)
    w, s, o = random_params(rng, 12)
    check(ctx, frames, w, s, o, sl, sh, it)


def test_edge_pixels_with_weights(ctx):
    """tests/test_gpu_stack.py's twelve hand-built pixels, and four more: a normalised sample that overflows, everything clipped (the
    fallback), one finite sample after normalisation, -0.0 read as it is"""
    n, cols = 8, 16
    px = np.zeros((n, cols), np.float32)
    px[:, 0] = np.nan                                           # nothing finite -> 0.0, weight 0
    px[:, 1] = np.nan; px[3, 1] = 42.5                          # single finite -> itself, its frame's weight
    px[:, 2] = np.inf; px[1, 2] = -7.0; px[6, 2] = 9.0          # two finite
    px[:, 3] = 5.0                                              # constant: MAD 0 -> sigma floor 1e-10
    px[:, 4] = 5.0; px[2, 4] = 5.0000005                        # constant + 1 ulp outlier -> rejected
    px[:, 5] = [1, 1, 1, 1, 2, 2, 2, 2]                         # ties around the median
    px[:, 6] = [-3e38, 3e38, 1, 2, 3, 4, 5, 6]                  # dev overflows to inf
    px[:, 7] = [-1, -2, -3, -4, -5, -6, -7, -800]               # negatives + outlier
    px[:, 8] = [1e-40, 2e-40, 3e-40, 1e-39, 0, -0.0, 1e-45, 5e-41]   # subnormals
    px[:, 9] = [0, 0, 0, 0, 0, 0, 1000, 1001]                   # zero padding majority
    px[:, 10] = [100, 101, 99, 100, 5000, 6000, 7000, 100.5]    # many outliers: several iterations
    px[:, 11] = np.arange(8)
    px[:, 12] = [10, 11, 12, 13, 3e38, 14, 15, 16]              # frame 4 has scale 2: 3e38 * 2 = inf, dropped like a NaN
    px[:, 13] = [1, 1, 1, 1, 2, 2, 2, 2]                        # everything clipped under the last two settings below
    px[:, 14] = np.nan; px[5, 14] = -0.0                        # one sample, frame 5 is read as it is: -0.0 stays -0.0
    px[:, 15] = [7, 7, 7, 7, 7, 7, 7, 9]
    frames = [px[k].reshape(1, cols).copy() for k in range(n)]
    w = np.array([1.0, 0.5, 0.25, 0.125, 1.0, 0.75, 0.375, 0.0625])
    s = np.array([1, 1, 1, 1, 2, 1, 1, 1], np.float32)
    o = np.array([0, 0, 0, 0, 0, 0, 0.5, 0], np.float32)
    for sl, sh, it in [(3.0, 3.0, 5), (1.0, 1.0, 5), (3.0, 3.0, 1)]:
        got, gw, _ = check(ctx, frames, w, s, o, sl, sh, it)
    assert got[0, 0] == 0.0 and gw[0, 0] == 0.0
    assert got[0, 1] == np.float32(42.5) and gw[0, 1] == np.float32(0.125)
    assert np.signbit(got[0, 14]) and got[0, 14] == 0.0 and gw[0, 14] == np.float32(0.75)
    plain = [1.0] * n
    got, gw, _ = check(ctx, frames, w, None, None, 3.0, 3.0, 5)
    assert gw[0, 12] < np.float32(w.sum())                      # unscaled, 3e38 is finite and clipped
    # everything clipped: four samples of 1 and four of 2, median 2 (the upper one), MAD 1; with a negative sigma_high no deviation
    # passes `dev <= hi`, with a NaN sigma_low none passes `dev >= lo`: the fallback is the last centre, the median; weight 0
    got, gw, _ = check(ctx, frames, plain, None, None, 3.0, -1.0, 5)
    assert got[0, 13] == 2.0 and gw[0, 13] == 0.0
    got, gw, _ = check(ctx, frames, plain, None, None, NAN, 3.0, 5)
    assert got[0, 13] == 2.0 and gw[0, 13] == 0.0 and got[0, 0] == 0.0


def test_zero_weight_frames_take_part_in_nothing(ctx):
    """zero-weight frames scattered through the list, one of them full of outliers and non-finite values: the result is the stack of
    the remaining frames alone, bit for bit -- image, weight plane and rejected count"""
    rng = np.random.default_rng(41)
    frames = make_frames(rng, 14, 21, 67)
    frames[4] = (rng.random((21, 67)) * 1e6).astype(np.float32)
    frames[4][::3, ::5] = np.inf
    frames[9][:] = np.nan
    w, s, o = random_params(rng, 14)
    dead = [0, 4, 9, 13]
    w[dead] = 0.0
    got, gw, rej = check(ctx, frames, w, s, o)
    live = [k for k in range(14) if k not in dead]
    got2, gw2, rej2 = ctx.stack_weighted([frames[k] for k in live], w[live], s[live], o[live], want_weight=True)
    assert_bits(got, got2, "image")
    assert_bits(gw, gw2, "weight plane")
    assert rej == rej2


def test_active_frame_limit(ctx):
    import astroburst_amd as ab
    from astroburst_amd import _lib
    rng = np.random.default_rng(77)
    frames = make_frames(rng, 70, 9, 33)
    w, s, o = random_params(rng, 70)
    w[[3, 10, 11, 40, 68, 69]] = 0.0
    check(ctx, frames, w, s, o)                                 # 70 frames, 64 of them active
    w[3] = 0.5
    with pytest.raises(ab.AstroBurstError, match="64") as e:   # 65 active
        ctx.stack_weighted(frames, w, s, o)
    assert e.value.code == _lib.AB_ERR_UNSUPPORTED
    with pytest.raises(ab.AstroBurstError, match="No images to stack") as e:
        ctx.stack_weighted(frames, np.zeros(70))
    assert e.value.code == _lib.AB_ERR_INVALID
    check(ctx, frames[:1], [0.5], [1.5], [2.0])                 # one active frame: the normalised copy, non-finite samples -> 0
    # 2^31 pixels or more are refused before anything is read (the descriptors' dims are made up; the memory is one small frame)
    import ctypes as C
    big = _lib.Plane(C.c_void_p(frames[0].ctypes.data), 1 << 16, 1 << 15, 0)
    cfg = _lib.StackConfig(3.0, 3.0, 5, 0)
    rc = ctx._L.ab_stack_weighted(ctx._h, C.byref(big), ab.stack_frame_params(1, [1.0]), 1, C.byref(cfg), C.byref(big), None, None)
    assert rc == _lib.AB_ERR_INVALID


def test_ragged_planes_crop_top_left(ctx):
    rng = np.random.default_rng(11)
    dims = [(40, 50), (33, 64), (48, 41), (35, 45), (60, 60)]
    frames = [(1000 + 10 * rng.standard_normal(d)).astype(np.float32) for d in dims]
    frames[2][5, 7] = 5000.0
    frames[4][0, 0] = np.nan
    w, s, o = random_params(rng, 5)
    got, gw, rej = ctx.stack_weighted(frames, w, s, o, want_weight=True)
    assert got.shape == (33, 41)
    want, ww, want_rej = wsr.stack_weighted([f[:33, :41] for f in frames], w, s, o)
    assert_bits(got, want, "image")
    assert_bits(gw, ww, "weight plane")
    assert rej == want_rej and rej > 0


def test_host_and_device_planes_give_the_same_bytes(ctx):
    import torch
    rng = np.random.default_rng(23)
    frames = make_frames(rng, 10, 37, 131)
    w, s, o = random_params(rng, 10)
    got, gw, rej = check(ctx, frames, w, s, o)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    dgot, dgw, drej = ctx.stack_weighted(dev, w, s, o, want_weight=True)
    assert dgot.is_cuda and dgw.is_cuda
    assert_bits(dgot.cpu().numpy(), got, "image")
    assert_bits(dgw.cpu().numpy(), gw, "weight plane")
    assert drej == rej
    # without the weight plane the image is unchanged; without the count the call does not wait, and the count can be had later
    only, none = ctx.stack_weighted(dev, w, s, o, want_rejected=False)
    assert none is None and ctx.last_rejected() == rej
    assert_bits(only.cpu().numpy(), got, "image")
    honly, hrej = ctx.stack_weighted(frames, w, s, o)
    assert_bits(honly, got, "image")
    assert hrej == rej
    with pytest.raises(Exception, match="overlaps"):           # a device output over a device input is refused
        ctx.stack_weighted(dev, w, s, o, out=dev[2])


@pytest.mark.parametrize("n", [7, 32, 64])
def test_integer_frames_cross_check_without_the_restatement(ctx, ctx_exact, n):
    """integer-valued frames in [0, 4096): every f64 sum is exact, so the order of the final sum cannot show.  All weights 1: bit for
    bit the exact engine of ab_stack_sigma_clip, same rejected count.  Weights k / 8: the restatement.  All weights times 4: the
    image is unchanged bit for bit, the weight plane is four times as large."""
    rng = np.random.default_rng(900 + n)
    base = rng.integers(100, 3000, (29, 71))
    frames = [np.clip(base + rng.integers(-40, 41, base.shape), 0, 4095).astype(np.float32) for _ in range(n)]
    for k in range(0, n, 3):
        hit = rng.random(base.shape) < 0.04
        frames[k][hit] = rng.integers(0, 4096, hit.sum()).astype(np.float32)
        frames[k][rng.random(base.shape) < 0.02] = np.nan
    got, gw, rej = ctx.stack_weighted(frames, np.ones(n), want_weight=True)
    want, want_rej = ctx_exact.stack_sigma_clip(frames)
    assert_bits(got, want, "image against the exact engine")
    assert rej == want_rej and rej > 0
    assert np.all(gw == np.floor(gw)) and gw.max() <= n         # the weight plane counts the survivors
    w = rng.integers(1, 9, n) / 8.0
    got, gw, rej2 = check(ctx, frames, w)
    assert rej2 == rej                                          # the weights have no say in the rejection
    got4, gw4, rej4 = ctx.stack_weighted(frames, 4.0 * w, want_weight=True)
    assert_bits(got4, got, "image under scaled weights")
    assert_bits(gw4, 4.0 * gw, "weight plane under scaled weights")
    assert rej4 == rej


def test_scores_to_params_to_stack(ctx):
    """the chain the entry points were built for: analyze_subframes(normalize) -> stack_params_from_metrics("additive") ->
    stack_weighted, on device planes; held to the restatement fed the same parameters"""
    import torch
    import astroburst_amd as ab
    from astroburst_amd import synth
    rows = cols = 256
    y, x, flux = synth.star_catalog(rows, cols, 70, seed=3)
    cat = (y, x, flux * 25.0)
    host = [synth.make_frame(rows, cols, k, cat=cat, sky=200.0 + 35.0 * k, bad_patch_rate=1e-5).numpy() for k in range(5)]
    host.append(np.full((rows, cols), 100.0, np.float32))      # no stars at all: rejected by the scores
    dev = [torch.from_numpy(f).cuda() for f in host]
    metrics = ctx.analyze_subframes(dev, normalize=True)
    assert not metrics[5].accepted and sum(m.accepted for m in metrics) >= 3
    p = ab.stack_params_from_metrics(metrics, "additive")
    assert p.weights[5] == 0.0 and p.weights.max() == 1.0 and p.weights[p.reference] == 1.0
    assert np.count_nonzero(p.offsets) >= 2                     # the sky levels differ: the frames are brought to the reference's
    got, gw, rej = ctx.stack_weighted(dev, p.weights, p.scales, p.offsets, want_weight=True)
    want, ww, want_rej = wsr.stack_weighted(host, p.weights, p.scales, p.offsets)
    assert_bits(got.cpu().numpy(), want, "image")
    assert_bits(gw.cpu().numpy(), ww, "weight plane")
    assert rej == want_rej
