"""The FFT power spectrum without a GPU: the library's two host-only functions (ab_power_spectrum_dims, ab_hann_symmetric_f32 -- the
GPU path multiplies by the latter's table, so this covers what the kernels read) against the restatement
(tests/spectrum_restatement.py), the reference's own hann_symmetric #[test]s (math/window.rs:128-154) transcribed, the restatement
checked against itself (its f32 radix-2 yardstick against its f64 truth, where DC and a cosine's peaks land, the Hermitian
symmetry of the unwindowed map), and the exported symbols."""
import ctypes
import os

import numpy as np
import pytest

import spectrum_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U = 2.0 ** -24  # the unit roundoff of f32


def _core():
    from astroburst_amd import core
    return core


# ---- ab_power_spectrum_dims ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,want", [((1, 1), (1, 1)), ((1000, 1024), (1024, 1024)), ((1025, 3), (2048, 1024)),
                                       ((13759, 12451), (16384, 1024)), ((2, 2), (2, 2)), ((3, 5), (8, 8)), ((16384, 16384), (16384, 1024))])
def test_power_spectrum_dims(dims, want):
    assert _core().power_spectrum_dims(*dims) == want
    assert R.power_spectrum_dims(*dims) == want


@pytest.mark.parametrize("dims,code", [((16385, 1), "AB_ERR_UNSUPPORTED"), ((1, 16385), "AB_ERR_UNSUPPORTED"), ((0, 5), "AB_ERR_INVALID"),
                                       ((5, -1), "AB_ERR_INVALID")])
def test_power_spectrum_dims_rejects(dims, code):
    from astroburst_amd import _lib
    with pytest.raises(_lib.AstroBurstError) as e:
        _core().power_spectrum_dims(*dims)
    assert e.value.code == getattr(_lib, code)
    # the C function itself, NULL outputs allowed
    assert _lib.lib().ab_power_spectrum_dims(dims[0], dims[1], None, None) == getattr(_lib, code)
    assert _lib.lib().ab_power_spectrum_dims(3, 5, None, None) == _lib.AB_OK


# ---- ab_hann_symmetric_f32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 128, 129, 12451])
def test_hann_matches_the_f32_restatement(n):
    """two cosf correctly rounded to 1 ulp, of the same f32 phase, differ by at most one ulp of a value <= 1 (1.2e-7), and
    0.5 * (1 - c) does not enlarge that"""
    got = _core().hann_symmetric_f32(n)
    want = R.hann_symmetric_f32(n)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1.2e-7
    if n == 1:
        assert got[0] == 1.0
    else:
        assert got[0] == 0.0 and got[-1] == 0.0  # the endpoints are zero: cosf(0) = cosf(2 pi as f32) = 1 exactly
    assert (got >= 0.0).all() and (got <= 1.0).all()


def test_hann_zero_length_and_null():
    from astroburst_amd import _lib
    assert _core().hann_symmetric_f32(0).shape == (0,)
    assert _lib.lib().ab_hann_symmetric_f32(0, None) == _lib.AB_OK
    assert _lib.lib().ab_hann_symmetric_f32(4, None) == _lib.AB_ERR_INVALID


# the reference's tests of hann_symmetric (window.rs:128-154), on the f32 table the library serves.  They are written for f64 with
# 1e-10; in f32 the phase carries a rounding error of up to ulp(2 pi) = 4.8e-7, |d cos| <= |d phase|, times 0.5, on each of the two
# values compared: 1e-6 bounds the sum.  Endpoints and the centre are exact in f32 (cosf of 0, of 2 pi as f32 and of pi as f32)
def test_hann_symmetric_endpoints_zero():
    w = _core().hann_symmetric_f32(128)
    assert abs(w[0]) < 1e-10 and abs(w[127]) < 1e-10


def test_hann_symmetric_peak_at_center():
    w = _core().hann_symmetric_f32(129)
    assert abs(w[64] - 1.0) < 1e-10


def test_hann_symmetric_symmetry():
    w = _core().hann_symmetric_f32(128).astype(np.float64)
    for i in range(64):
        assert abs(w[i] - w[127 - i]) < 1e-6, (i, w[i], w[127 - i])


def test_hann_f64_restatement_passes_the_reference_tests_as_written():
    w = R.hann_symmetric_f64(128)
    assert abs(w[0]) < 1e-10 and abs(w[127]) < 1e-10
    assert abs(R.hann_symmetric_f64(129)[64] - 1.0) < 1e-10
    assert np.abs(w[:64] - w[::-1][:64]).max() < 1e-10


# ---- the restatement against itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(64, 64), (300, 200)])
@pytest.mark.parametrize("window", [True, False])
def test_yardstick_against_truth(rows, cols, window):
    """Higham's worst-case bound for a radix-2 FFT with twiddles rounded once: relative L2 error <= log2(N) * eta, eta about 6 u.
    The 2-D transform is log2(size^2) layers.  For the map, |d ln(1 + m)| <= |dm|, and the mean |dm| is at most the rms error of
    the bins, i.e. the relative L2 error times the rms magnitude; on top, one ulp of the largest value for the f32 sqrt / log."""
    img = R.make_image(rows, cols, seed=rows + cols)
    size, _ = R.power_spectrum_dims(rows, cols)
    wy32, wx32 = (R.hann_symmetric_f32(rows), R.hann_symmetric_f32(cols)) if window else (None, None)
    T = R.fft2_forward_truth(img, window, size, size, wy32, wx32)
    Y = R.fft2_forward_yardstick(img, window, size, size, wy32, wx32)
    layers = 2 * int(np.log2(size))
    rel = np.linalg.norm(Y - T) / np.linalg.norm(T)
    assert rel <= layers * 6 * U, rel
    assert rel > 0.0  # (a yardstick that equals truth is not single precision)
    LT, LY = R.power_spectrum_truth(img, window), R.power_spectrum_yardstick(img, window)
    assert LT.shape == LY.shape == (size, size) and LY.dtype == np.float32 and LT.dtype == np.float64
    rms = np.sqrt(np.mean(np.abs(T) ** 2))
    # (windowed: the f32 window differs from the f64 one by up to 1.2e-7 per factor, another 4 u relative on every pixel)
    bound = (layers * 6 + 8) * U * rms + np.spacing(F32(LT.max()))
    assert np.abs(LY - LT).mean() <= bound, (np.abs(LY - LT).mean(), bound)


@pytest.mark.parametrize("rows,cols", [(64, 64), (300, 200), (5, 3)])
def test_dc_lands_at_the_centre(rows, cols):
    img = np.full((rows, cols), 7.0, F32)
    size, _ = R.power_spectrum_dims(rows, cols)
    for L in (R.power_spectrum_truth(img, False), R.power_spectrum_yardstick(img, False)):
        assert np.unravel_index(np.argmax(L), L.shape) == (size // 2, size // 2)
        assert abs(L[size // 2, size // 2] - np.log1p(7.0 * rows * cols)) < 1e-4


def test_a_cosine_gives_two_peaks_at_its_bins():
    n, ky, kx = 64, 5, 9
    yy, xx = np.mgrid[0:n, 0:n]
    img = np.cos(2.0 * np.pi * (ky * yy + kx * xx) / n).astype(F32)
    for L in (R.power_spectrum_truth(img, False), R.power_spectrum_yardstick(img, False)):
        top = set(map(tuple, np.argwhere(L > 0.5 * L.max()).tolist()))
        assert top == {(n // 2 + ky, n // 2 + kx), (n // 2 - ky, n // 2 - kx)}


@pytest.mark.parametrize("rows,cols", [(64, 64), (30, 20)])
def test_unwindowed_map_is_hermitian_symmetric(rows, cols):
    """a real input: |F[k]| = |F[-k]|; after the shift, L[r, c] == L[size - r, size - c] for r, c >= 1.  Truth holds it to f64
    rounding; the radix-2 yardstick, whose butterflies are not symmetric in k, to its own f32 error"""
    img = R.make_image(rows, cols, seed=3)
    size, _ = R.power_spectrum_dims(rows, cols)
    LT, LY = R.power_spectrum_truth(img, False), R.power_spectrum_yardstick(img, False)
    assert np.abs(LT[1:, 1:] - LT[1:, 1:][::-1, ::-1]).max() < 1e-9
    err = np.abs(LY - LT).max()
    assert np.abs(LY[1:, 1:].astype(np.float64) - LY[1:, 1:][::-1, ::-1]).max() <= 2 * err + 1e-12


def test_block_mean_of_the_restatement():
    """_display beyond 1024: each output is the mean of its s x s block of the shifted plane"""
    rng = np.random.default_rng(0)
    plane = rng.random((2048, 2048))
    d = R._display(plane, np.float64)
    sh = np.roll(plane, (1024, 1024), axis=(0, 1))
    assert d.shape == (1024, 1024)
    for (y, x) in [(0, 0), (5, 1023), (1023, 17), (512, 512)]:
        assert abs(d[y, x] - sh[2 * y:2 * y + 2, 2 * x:2 * x + 2].mean()) < 1e-15


def test_spectrum_to_u8_restatement_edges():
    v = np.array([[0.0, 1.0], [np.nan, 2.0]], F32)
    b, mn, mx, dc = R.spectrum_to_u8(v)
    assert (mn, mx, dc) == (0.0, 2.0, 2.0) and b.tolist() == [[0, 127], [0, 255]]
    b, mn, mx, dc = R.spectrum_to_u8(np.zeros((2, 2), F32))
    assert (mn, mx) == (0.0, 0.0) and not b.any()


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    from astroburst_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ab_power_spectrum_dims", "ab_hann_symmetric_f32", "ab_fft2_forward_f32", "ab_compute_power_spectrum", "ab_spectrum_to_u8"):
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols()
