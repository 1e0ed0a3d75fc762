"""GPU FFT power spectrum (core/analysis/fft.rs, csrc/spectrum.hip) against the numpy restatement (tests/spectrum_restatement.py).

The library's FFT is its own, so nothing is bit for bit against the reference.  The bar, the same everywhere: T = f64 truth,
Y = the f32 radix-2 yardstick, G = the library, all on the same input;
    max |G - T|  <= max(4 * max |Y - T|,  4 ulp_f32(max |T|))
    mean |G - T| <= max(2 * mean |Y - T|, 1 ulp_f32(max |T|))
(the max over up to 10^6 bins is a tail statistic in which two correct f32 FFTs differ by a small factor; the mean is stable; the
ulp floors cover logf / sqrtf rounding where the FFT error is nil).  For fft2_forward the same on the complex values, the mean
replaced by the relative L2 error, <= 2 x the yardstick's.  Each check prints its ratios (G's error / Y's) before it asserts.
"""
import functools

import numpy as np
import pytest

import spectrum_restatement as R

pytestmark = pytest.mark.gpu

F32 = np.float32


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


def held_to_the_bar(G, T, Y, what, l2=False):
    G64 = G.astype(np.complex128 if l2 else np.float64)
    eg, ey = np.abs(G64 - T), np.abs(Y - T)
    top = float(np.abs(T).max())
    max_bound = max(4.0 * float(ey.max()), 4.0 * ulp32(top))
    if l2:
        nt = float(np.linalg.norm(T))
        g2, y2 = (float(np.linalg.norm(G64 - T)) / nt, float(np.linalg.norm(Y - T)) / nt) if nt > 0 else (float(np.linalg.norm(G64 - T)), 0.0)
        print(f"[spectrum-ratio] {what}: max {float(eg.max()):.3e} / {float(ey.max()):.3e} = {float(eg.max()) / max(float(ey.max()), 1e-300):.2f}; "
              f"relL2 {g2:.3e} / {y2:.3e} = {g2 / max(y2, 1e-300):.2f}")
        assert float(eg.max()) <= max_bound, (what, float(eg.max()), max_bound)
        if nt > 0:
            assert g2 <= max(2.0 * y2, ulp32(1.0)), (what, g2, y2)   # (relative: one ulp of 1 is the floor)
        else:
            assert g2 == 0.0
    else:
        mean_bound = max(2.0 * float(ey.mean()), ulp32(top))
        print(f"[spectrum-ratio] {what}: max {float(eg.max()):.3e} / {float(ey.max()):.3e} = {float(eg.max()) / max(float(ey.max()), 1e-300):.2f}; "
              f"mean {float(eg.mean()):.3e} / {float(ey.mean()):.3e} = {float(eg.mean()) / max(float(ey.mean()), 1e-300):.2f}")
        assert float(eg.max()) <= max_bound, (what, float(eg.max()), max_bound)
        assert float(eg.mean()) <= mean_bound, (what, float(eg.mean()), mean_bound)


# ---- fft2_forward ----------------------------------------------------------------------------------------------------------------
# the issue's buffers, plus both sides of every line length at which the line kernel changes form: up to 2048 points several lines
# share a workgroup (2048 / n of them); 4096, 8192 and 16384 are one line per workgroup with their own tile sizes
FFT_DIMS = [(1, 1), (1, 2), (2, 1), (4, 4), (2, 64), (64, 2), (512, 1024), (1024, 512), (2, 16384), (16384, 2), (4, 8192), (8192, 4),
            (2048, 4), (4, 2048), (4096, 2), (2, 4096)]


def image_for(fft_rows, fft_cols, fill):
    """fill: the image is the whole buffer; else rows < fft_rows and cols < fft_cols wherever the buffer leaves room"""
    if fill:
        rows, cols = fft_rows, fft_cols
    else:
        rows, cols = max(1, fft_rows - max(1, fft_rows // 5)), max(1, fft_cols - max(1, fft_cols // 3))
    return R.make_image(rows, cols, seed=fft_rows * 3 + fft_cols)


@functools.lru_cache(maxsize=None)
def fft_case(fft_rows, fft_cols, fill, window):
    img = image_for(fft_rows, fft_cols, fill)
    wy, wx = (R.hann_symmetric_f32(img.shape[0]), R.hann_symmetric_f32(img.shape[1])) if window else (None, None)
    T = R.fft2_forward_truth(img, window, fft_rows, fft_cols, wy, wx)
    Y = R.fft2_forward_yardstick(img, window, fft_rows, fft_cols, wy, wx)
    for a in (img, T, Y):
        a.setflags(write=False)
    return img, wy, wx, T, Y


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("fill", [True, False])
@pytest.mark.parametrize("fft_rows,fft_cols", FFT_DIMS)
def test_fft2_forward(ctx, fft_rows, fft_cols, fill, window):
    img, wy, wx, T, Y = fft_case(fft_rows, fft_cols, fill, window)
    G = ctx.fft2_forward(img, fft_rows, fft_cols, wy, wx)
    assert G.shape == (fft_rows, fft_cols) and G.dtype == np.complex64
    held_to_the_bar(G, T, Y, f"fft2 {fft_rows}x{fft_cols} image {img.shape[0]}x{img.shape[1]} window={int(window)}", l2=True)


@pytest.mark.parametrize("window", [False, True])
def test_fft2_small_image_in_a_64_buffer(ctx, window):
    img = R.make_image(3, 5, seed=11)
    wy, wx = (R.hann_symmetric_f32(3), R.hann_symmetric_f32(5)) if window else (None, None)
    G = ctx.fft2_forward(img, 64, 64, wy, wx)
    held_to_the_bar(G, R.fft2_forward_truth(img, window, 64, 64, wy, wx), R.fft2_forward_yardstick(img, window, 64, 64, wy, wx),
                    f"fft2 64x64 image 3x5 window={int(window)}", l2=True)


@pytest.mark.parametrize("window", [False, True])
def test_fft2_non_finite_pixels_are_zeros(ctx, window):
    img = R.make_image(50, 70, seed=5)
    bad = img.copy()
    holes = [(0, 0), (49, 69), (10, 33), (25, 1), (30, 30)]
    for k, (y, x) in enumerate(holes):
        bad[y, x] = [np.nan, np.inf, -np.inf][k % 3]
    zeroed = img.copy()
    for (y, x) in holes:
        zeroed[y, x] = 0.0
    wy, wx = (R.hann_symmetric_f32(50), R.hann_symmetric_f32(70)) if window else (None, None)
    a = ctx.fft2_forward(bad, 64, 128, wy, wx)
    b = ctx.fft2_forward(zeroed, 64, 128, wy, wx)
    assert np.isfinite(a.view(np.float32)).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("fft_rows,fft_cols", [(64, 128), (512, 1024), (4096, 2), (2, 16384)])
def test_fft2_host_and_device_planes_agree_and_repeat(ctx, fft_rows, fft_cols):
    """host plane == device plane bit for bit, the input is unmodified, a second call returns the same bits"""
    import torch
    img, wy, wx, _, _ = fft_case(fft_rows, fft_cols, False, True)
    host_in = np.array(img)
    h = ctx.fft2_forward(host_in, fft_rows, fft_cols, wy, wx)
    assert np.array_equal(host_in.view(np.uint32), img.view(np.uint32))
    dev_in = torch.from_numpy(np.array(img)).cuda()
    d = ctx.fft2_forward(dev_in, fft_rows, fft_cols, wy, wx)
    assert d.is_cuda and d.dtype == torch.complex64 and tuple(d.shape) == (fft_rows, fft_cols)
    d2 = ctx.fft2_forward(dev_in, fft_rows, fft_cols, wy, wx)
    assert np.array_equal(dev_in.cpu().numpy().view(np.uint32), img.view(np.uint32))
    dn = torch.view_as_real(d).cpu().numpy()
    assert np.array_equal(dn.view(np.uint32).reshape(-1), h.view(np.uint32).reshape(-1))
    assert torch.equal(torch.view_as_real(d).view(torch.int32), torch.view_as_real(d2).view(torch.int32))


# ---- compute_power_spectrum ------------------------------------------------------------------------------------------------------
PS_CASES = [((1, 1), 1), ((2, 2), 2), ((3, 5), 8), ((64, 64), 64), ((300, 200), 512), ((200, 300), 512), ((1024, 1024), 1024),
            ((1025, 1024), 2048), ((2049, 17), 4096)]


@functools.lru_cache(maxsize=None)
def ps_case(rows, cols, window):
    img = R.make_image(rows, cols, seed=rows + 2 * cols)
    T, Y = R.power_spectrum_truth(img, window), R.power_spectrum_yardstick(img, window)
    for a in (img, T, Y):
        a.setflags(write=False)
    return img, T, Y


@pytest.mark.parametrize("window", [True, False])
@pytest.mark.parametrize("shape,size", PS_CASES)
def test_compute_power_spectrum(ctx, shape, size, window):
    img, T, Y = ps_case(shape[0], shape[1], window)
    res = ctx.compute_power_spectrum(np.array(img), apply_window=window)
    disp = min(size, 1024)
    assert (res.display_rows, res.display_cols, res.original_size, res.windowed) == (disp, disp, size, window)
    assert res.spectrum.shape == (disp, disp) and res.spectrum.dtype == np.float32
    held_to_the_bar(res.spectrum, T, Y, f"spectrum image {shape[0]}x{shape[1]} buffer {size} window={int(window)}")
    if shape == (2, 2) and window:
        assert not res.spectrum.any()  # the 2-point Hann window is all zeros: the spectrum is identically zero


@pytest.mark.parametrize("shape", [(300, 200), (1025, 1024)])
def test_compute_power_spectrum_device_resident(ctx, shape):
    """device plane in, device-resident spectrum out (also into a caller's tensor): the host path's bits; a second call repeats"""
    import torch
    img, _, _ = ps_case(shape[0], shape[1], True)
    host = ctx.compute_power_spectrum(np.array(img)).spectrum
    dev_in = torch.from_numpy(np.array(img)).cuda()
    res = ctx.compute_power_spectrum(dev_in)
    assert res.spectrum.is_cuda and res.spectrum.dtype == torch.float32 and tuple(res.spectrum.shape) == host.shape
    assert np.array_equal(res.spectrum.cpu().numpy().view(np.uint32), host.view(np.uint32))
    out = torch.full(host.shape, -1.0, device="cuda")
    res2 = ctx.compute_power_spectrum(dev_in, out=out)
    assert res2.spectrum is out and torch.equal(out.view(torch.int32), res.spectrum.view(torch.int32))
    assert np.array_equal(dev_in.cpu().numpy().view(np.uint32), img.view(np.uint32))


def test_context_stays_usable_after_trim(ctx):
    """ab_ctx_trim releases the FFT workspaces and the twiddle tables; the next call rebuilds them and returns the same bits"""
    img, _, _ = ps_case(300, 200, True)
    a = ctx.compute_power_spectrum(np.array(img)).spectrum
    ctx.trim()
    b = ctx.compute_power_spectrum(np.array(img)).spectrum
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- spectrum_to_u8 --------------------------------------------------------------------------------------------------------------
def check_u8(ctx, plane):
    import torch
    want, mn, mx, dc = R.spectrum_to_u8(plane)
    got, gmn, gmx, gdc = ctx.spectrum_to_u8(plane)
    assert got.dtype == np.uint8 and got.shape == plane.shape
    assert (F32(gmn).view(np.uint32), F32(gmx).view(np.uint32), F32(gdc).view(np.uint32)) == (mn.view(np.uint32), mx.view(np.uint32), dc.view(np.uint32))
    assert np.array_equal(got, want), int((got != want).sum())
    dgot, dmn, dmx, ddc = ctx.spectrum_to_u8(torch.from_numpy(np.array(plane)).cuda())
    assert dgot.is_cuda and dgot.dtype == torch.uint8
    assert np.array_equal(dgot.cpu().numpy(), want) and (dmn, dmx, ddc) == (gmn, gmx, gdc)
    return got


@pytest.mark.parametrize("shape", [(64, 64), (1025, 1024)])
def test_spectrum_to_u8_of_the_librarys_own_spectrum(ctx, shape):
    """min, max, dc and every byte equal the numpy-f32 restatement of the command's arithmetic on the same plane; the plane holds
    its own maximum, whose byte is 254 or 255, whichever (max - min) * (255 / range) gives in f32"""
    img, _, _ = ps_case(shape[0], shape[1], True)
    plane = ctx.compute_power_spectrum(np.array(img)).spectrum
    got = check_u8(ctx, plane)
    assert got.max() in (254, 255) and got.min() == 0


def test_spectrum_to_u8_all_zero_windowed_image(ctx):
    """a 2 x 2 image under its Hann window is all zeros: range takes its floor of 1e-10 and every byte is 0"""
    plane = ctx.compute_power_spectrum(R.make_image(2, 2, seed=1)).spectrum
    assert not plane.any()
    got = check_u8(ctx, plane)
    assert not got.any()


def test_spectrum_to_u8_nan_and_saturation(ctx):
    plane = np.array([[0.0, 1.0, np.nan], [2.0, 0.5, 1.9999999]], F32)
    check_u8(ctx, plane)


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_context_usable(ctx):
    from astroburst_amd import _lib
    img = R.make_image(20, 30, seed=2)

    def rejected(fn):
        with pytest.raises(_lib.AstroBurstError) as e:
            fn()
        assert e.value.code == _lib.AB_ERR_INVALID and len(e.value.message) > 0
        return e.value.message

    assert "power" in rejected(lambda: ctx.fft2_forward(img, 48, 32))                      # non-power-of-two fft_rows
    assert "larger" in rejected(lambda: ctx.fft2_forward(img, 16, 32))                     # image larger than the buffer
    keep = []
    pi = ctx._plane(img, keep)
    wy = R.hann_symmetric_f32(20)
    out = np.empty((32, 32), np.complex64)
    import ctypes as C
    rc = ctx._L.ab_fft2_forward_f32(ctx._h, C.byref(pi), wy.ctypes.data_as(C.POINTER(C.c_float)), None, 32, 32, C.c_void_p(out.ctypes.data), 0)
    assert rc == _lib.AB_ERR_INVALID and b"both" in ctx._L.ab_last_error(ctx._h)            # only one window given
    assert "must be 32 x 32" in rejected(lambda: ctx.compute_power_spectrum(img, out=np.empty((64, 64), F32)))  # wrong spectrum dims
    G = ctx.fft2_forward(img, 32, 32)
    held_to_the_bar(G, R.fft2_forward_truth(img, False, 32, 32), R.fft2_forward_yardstick(img, False, 32, 32), "fft2 32x32 after errors", l2=True)
