"""No GPU: (1) tests/weighted_stack_restatement.py -- what the GPU tests hold ab_stack_weighted to bit for bit -- against the oracle's
sigma_clip_combine; (2) ab_stack_params_from_metrics, host arithmetic in the library; (3) the Python wrapper's argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import weighted_stack_restatement as wsr

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


def oracle_per_pixel(oracle, frames, sl, sh, it):
    """oracle.sigma_clip_combine on the finite samples of every pixel, ascending order -> (image, rejected)"""
    cube = np.stack(frames).reshape(len(frames), -1)
    out = np.zeros(cube.shape[1], np.float32)
    rej = 0
    for p in range(cube.shape[1]):
        col = cube[:, p]
        out[p], r = oracle.sigma_clip_combine(col[np.isfinite(col)], sl, sh, it, order=oracle.ORDER_ASCENDING)
        rej += r
    return out.reshape(frames[0].shape), rej


def bit_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n,sl,sh,it", [(2, 3.0, 3.0, 5), (3, 3.0, 3.0, 5), (9, 2.0, 2.0, 5), (16, 1.0, 4.0, 3), (33, 0.5, 0.5, 10), (64, 3.0, 3.0, 5),
                                        (12, 3.0, 3.0, 0), (12, 3.0, 3.0, 1), (12, 0.0, 0.0, 5), (12, -1.0, 3.0, 5), (12, 3.0, INF, 5),
                                        (12, NAN, 3.0, 2)])
def test_restatement_with_unit_parameters_is_the_oracle_on_integer_samples(oracle, n, sl, sh, it):
    """integer-valued samples in [0, 4096): every f64 sum is exact, so the order of the final sum (frame order here, ascending value in
    the oracle) cannot show -- value and rejected count bit for bit"""
    rng = np.random.default_rng(300 + n)
    base = rng.integers(100, 3000, (9, 23))
    frames = [np.clip(base + rng.integers(-40, 41, base.shape), 0, 4095).astype(np.float32) for _ in range(n)]
    for k in range(0, n, 4):
        hit = rng.random(base.shape) < 0.05
        frames[k][hit] = rng.integers(0, 4096, hit.sum()).astype(np.float32)      # outliers
        frames[k][rng.random(base.shape) < 0.03] = np.nan
    got, wsum, rej = wsr.stack_weighted(frames, [1.0] * n, None, None, sl, sh, it)
    want, want_rej = oracle_per_pixel(oracle, frames, sl, sh, it)
    assert rej == want_rej
    assert bit_equal(got, want), np.argwhere(got != want)[:5]
    assert np.all(wsum == np.floor(wsum)) and wsum.max() <= n


@pytest.mark.parametrize("n", [2, 5, 12, 33, 64])
def test_restatement_with_unit_parameters_is_the_oracle_on_natural_data(oracle, n):
    """NaN, +-inf, cosmic rays, zero borders: the rejected counts are equal; the values agree to 1e-6 relative -- about ten f32 ulps for
    the one allowed difference, the order of the final f64 sum (reordering at most 64 doubles moves a value that is then rounded to
    f32 by at most one f32 ulp)"""
    rng = np.random.default_rng(400 + n)
    frames = make_frames(rng, n, 19, 45)
    got, _, rej = wsr.stack_weighted(frames, [1.0] * n)
    want, want_rej = oracle_per_pixel(oracle, frames, 3.0, 3.0, 5)
    assert rej == want_rej
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_restatement_weights_and_normalisation_by_hand():
    """three pixels worked out by hand"""
    f = [np.array([[10.0, 1.0, -0.0]], np.float32), np.array([[12.0, NAN, NAN]], np.float32), np.array([[1000.0, NAN, NAN]], np.float32),
         np.array([[14.0, 5.0, NAN]], np.float32)]
    # pixel 0: samples 10, 12, 1000 * 0.5 - 488 = 12, 14 + 1 = 15; zero-weight frame: none.  median 12, MAD = 2 -> nothing clipped at 3 sigma
    img, ws, rej = wsr.stack_weighted(f, [1.0, 2.0, 0.5, 0.25], [1.0, 1.0, 0.5, 1.0], [0.0, 0.0, -488.0, 1.0])
    assert rej == 0
    assert img[0, 0] == np.float32((10.0 + 24.0 + 6.0 + 3.75) / 3.75) and ws[0, 0] == np.float32(3.75)
    # pixel 1: two finite samples, 1 and 6 (weights 1 and 0.25)
    assert img[0, 1] == np.float32((1.0 + 1.5) / 1.25) and ws[0, 1] == np.float32(1.25)
    # pixel 2: one finite sample, read as it is: -0.0 stays -0.0, the weight sum is that frame's weight
    assert np.signbit(img[0, 2]) and img[0, 2] == 0.0 and ws[0, 2] == 1.0
    # a frame of weight 0 takes part in nothing
    img2, ws2, _ = wsr.stack_weighted(f, [1.0, 2.0, 0.0, 0.25], [1.0, 1.0, 0.5, 1.0], [0.0, 0.0, -488.0, 1.0])
    img3, ws3, _ = wsr.stack_weighted([f[0], f[1], f[3]], [1.0, 2.0, 0.25], None, [0.0, 0.0, 1.0])
    assert bit_equal(img2, img3) and bit_equal(ws2, ws3)


# ---- ab_stack_params_from_metrics through the library --------------------------------------------------------------------------------
def metric(weight, bg, accepted=True):
    import astroburst_amd as ab
    return ab.SubframeMetrics(50, 2.5, 0.3, 30.0, bg, 4.0, 0.01, weight, accepted)


def test_params_from_metrics_every_mode():
    import astroburst_amd as ab
    ms = [metric(0.5, 1000.0), metric(1.0, 1100.0), metric(0.75, 900.0)]
    p = ab.stack_params_from_metrics(ms, "none")
    assert p.reference == 1 and p.weights.tolist() == [0.5, 1.0, 0.75]
    assert p.scales.tolist() == [1.0, 1.0, 1.0] and p.offsets.tolist() == [0.0, 0.0, 0.0]
    p = ab.stack_params_from_metrics(ms, "additive")
    assert p.reference == 1 and p.weights.tolist() == [0.5, 1.0, 0.75] and p.scales.tolist() == [1.0, 1.0, 1.0]
    assert p.offsets.tolist() == [100.0, 0.0, 200.0] and p.offsets.dtype == np.float32
    p = ab.stack_params_from_metrics(ms, "multiplicative")
    assert p.reference == 1 and p.offsets.tolist() == [0.0, 0.0, 0.0]
    assert p.scales.tolist() == [np.float32(1100.0 / 1000.0), 1.0, np.float32(1100.0 / 900.0)]


def test_params_from_metrics_frames_that_take_no_part():
    import astroburst_amd as ab
    ms = [metric(0.9, 1000.0, accepted=False), metric(0.0, 1000.0), metric(NAN, 1000.0), metric(INF, 1000.0), metric(-0.5, 1000.0),
          metric(0.5, 1010.0), metric(0.5, 1020.0), metric(0.4, NAN), metric(0.3, -5.0), metric(0.3, 0.0)]
    p = ab.stack_params_from_metrics(ms, "additive")
    assert p.reference == 5                                    # the tie of 0.5 goes to the lower index
    assert p.weights.tolist() == [0, 0, 0, 0, 0, 0.5, 0.5, 0, 0.3, 0.3]     # a background that is not finite: weight 0
    assert p.offsets[6] == -10.0 and p.offsets[8] == 1015.0 and p.offsets[9] == 1010.0
    p = ab.stack_params_from_metrics(ms, "multiplicative")
    assert p.weights.tolist() == [0, 0, 0, 0, 0, 0.5, 0.5, 0, 0, 0]         # ... and a non-positive one in the multiplicative mode
    assert p.scales[6] == np.float32(1010.0 / 1020.0) and p.scales[8] == 1.0 and p.offsets.tolist() == [0.0] * 10
    p = ab.stack_params_from_metrics(ms, "none")                              # the backgrounds are not looked at
    assert p.weights.tolist() == [0, 0, 0, 0, 0, 0.5, 0.5, 0.4, 0.3, 0.3] and p.reference == 5


def test_params_from_metrics_errors():
    import astroburst_amd as ab
    from astroburst_amd import _lib
    for mode in ("additive", "multiplicative"):                              # the reference frame itself fails
        with pytest.raises(ab.AstroBurstError) as e:
            ab.stack_params_from_metrics([metric(1.0, NAN), metric(0.5, 1000.0)], mode)
        assert e.value.code == _lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError):
        ab.stack_params_from_metrics([metric(1.0, -1.0), metric(0.5, 1000.0)], "multiplicative")
    assert ab.stack_params_from_metrics([metric(1.0, -1.0), metric(0.5, 1000.0)], "additive").offsets.tolist() == [0.0, -1001.0]
    for ms in ([], [metric(0.0, 1000.0)], [metric(1.0, 1000.0, accepted=False)]):                    # nothing active
        with pytest.raises(ab.AstroBurstError) as e:
            ab.stack_params_from_metrics(ms, "none")
        assert e.value.code == _lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError, match="normalize"):              # a bad mode, in the wrapper ...
        ab.stack_params_from_metrics([metric(1.0, 1000.0)], "median")
    L = _lib.lib()                                                           # ... and in the library; null pointers
    m = (_lib.SubframeMetricsC * 1)(_lib.SubframeMetricsC(50, 2.5, 0.3, 30.0, 1000.0, 4.0, 0.01, 1.0, 1))
    out = (_lib.StackFrameParamC * 1)()
    ref = C.c_size_t(7)
    assert L.ab_stack_params_from_metrics(m, 1, 3, out, C.byref(ref)) == _lib.AB_ERR_INVALID
    assert L.ab_stack_params_from_metrics(m, 1, -1, out, C.byref(ref)) == _lib.AB_ERR_INVALID
    assert L.ab_stack_params_from_metrics(None, 1, 0, out, C.byref(ref)) == _lib.AB_ERR_INVALID
    assert L.ab_stack_params_from_metrics(m, 1, 0, None, C.byref(ref)) == _lib.AB_ERR_INVALID
    assert L.ab_stack_params_from_metrics(m, 1, 0, out, None) == _lib.AB_OK                      # out_reference is optional
    assert (out[0].weight, out[0].scale, out[0].offset) == (1.0, 1.0, 0.0)
    assert L.ab_stack_params_from_metrics(m, 1, 1, out, C.byref(ref)) == _lib.AB_OK and ref.value == 0


def test_frame_param_struct_layout():
    from astroburst_amd import _lib
    assert C.sizeof(_lib.StackFrameParamC) == 16
    assert (_lib.StackFrameParamC.weight.offset, _lib.StackFrameParamC.scale.offset, _lib.StackFrameParamC.offset.offset) == (0, 8, 12)


def test_wrapper_argument_checks_need_no_device():
    import astroburst_amd as ab
    from astroburst_amd import _lib
    p = ab.stack_frame_params(3, [1.0, 0.0, 0.5])
    assert [(q.weight, q.scale, q.offset) for q in p] == [(1.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.5, 1.0, 0.0)]
    p = ab.stack_frame_params(2, np.array([1, 2]), scales=[0.5, 2.0], offsets=np.array([-1.0, 3.0], np.float64))
    assert [(q.weight, q.scale, q.offset) for q in p] == [(1.0, 0.5, -1.0), (2.0, 2.0, 3.0)]
    for args in ((3, [1.0, 1.0]), (2, [1.0, 1.0], [1.0]), (2, [1.0, 1.0], None, [0.0, 0.0, 0.0]),       # counts
                 (2, [1.0, -1.0]), (2, [1.0, NAN]), (2, [INF, 1.0]),                                      # weights
                 (2, [1.0, 1.0], [1.0, NAN]), (2, [1.0, 1.0], [INF, 1.0]), (2, [1.0, 1.0], None, [0.0, -INF]),
                 (2, [1.0, 1.0], [1e39, 1.0])):                                                           # not finite as f32
        with pytest.raises(ab.AstroBurstError) as e:
            ab.stack_frame_params(*args)
        assert e.value.code == _lib.AB_ERR_INVALID, args
    assert math.isfinite(ab.stack_frame_params(1, [1e300])[0].weight)
