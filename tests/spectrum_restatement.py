"""numpy restatement of the reference's FFT power spectrum (core/analysis/fft.rs:19-97, math/fft.rs:137-148 and :202-245,
math/window.rs:20-35, cmd/analysis/mod.rs:66-96), twice:

(a) TRUTH: the whole pipeline in float64 -- the window evaluated in f64, np.fft.fft2 on complex128;
(b) the SINGLE-PRECISION YARDSTICK: the same pipeline in f32 throughout, the f32 window as the reference computes it, and a plain
    recursive radix-2 FFT on complex64 whose twiddles are exp(-2 pi i k / n) evaluated in f64 and rounded to complex64, every
    intermediate cast back to complex64; magnitude, log, shift and block mean in f32.  Ordinary f32 butterflies are what rustfft
    is; np.fft on complex64 is several times more accurate than that and is deliberately not the yardstick.

The library is held to (a) with a bound derived from (b)'s own error (tests/test_gpu_spectrum.py).
"""
import numpy as np

MAX_DISPLAY_SIZE = 1024  # fft.rs:9
f32 = np.float32


def next_power_of_two(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


def power_spectrum_dims(rows: int, cols: int):
    """(original_size, display_size) of compute_power_spectrum (fft.rs:24-25, :53-57)"""
    size = next_power_of_two(max(rows, cols))
    return size, min(size, MAX_DISPLAY_SIZE)


# ---- windows (window.rs:20-35) ----
def hann_symmetric_f32(n: int) -> np.ndarray:
    """hann_symmetric::<f32>: every operation in f32, ((2 * pi) * i) / max(n - 1, 1), 0.5 * (1 - cos(phase))"""
    if n == 0:
        return np.zeros(0, f32)
    if n == 1:
        return np.ones(1, f32)
    two_pi = f32(2.0) * f32(np.pi)
    denom = max(f32(n - 1), f32(1.0))
    i = np.arange(n).astype(f32)
    phase = (two_pi * i).astype(f32) / denom
    return (f32(0.5) * (f32(1.0) - np.cos(phase.astype(f32)).astype(f32))).astype(f32)


def hann_symmetric_f64(n: int) -> np.ndarray:
    if n == 0:
        return np.zeros(0)
    if n == 1:
        return np.ones(1)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n) / max(n - 1, 1)))


# ---- prepare_windowed_buffer / prepare_buffer_no_window (fft.rs:202-245) ----
def prepare_buffer(image, win_y, win_x, fft_rows, fft_cols, dtype):
    """the zero-padded real buffer in `dtype` (f32: (v * wy) * wx in f32; f64: the same product of the f32 pixel in f64);
    non-finite pixels enter as 0"""
    image = np.asarray(image, f32)
    rows, cols = image.shape
    v = np.where(np.isfinite(image), image, f32(0)).astype(dtype)
    if win_y is not None:
        v = ((v * np.asarray(win_y, dtype)[:, None]).astype(dtype) * np.asarray(win_x, dtype)[None, :]).astype(dtype)
    buf = np.zeros((fft_rows, fft_cols), dtype)
    buf[:rows, :cols] = v
    return buf


# ---- the yardstick's FFT ----
def _twiddles_c64(n: int) -> np.ndarray:
    return np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)


def fft_radix2_c64(x: np.ndarray) -> np.ndarray:
    """plain recursive radix-2 decimation-in-time FFT along the last axis, complex64 at every step"""
    x = np.asarray(x, np.complex64)
    n = x.shape[-1]
    if n == 1:
        return x.copy()
    even = fft_radix2_c64(x[..., 0::2])
    odd = fft_radix2_c64(x[..., 1::2])
    t = (_twiddles_c64(n) * odd).astype(np.complex64)
    return np.concatenate([(even + t).astype(np.complex64), (even - t).astype(np.complex64)], axis=-1)


def fft2_yardstick(buf_f32: np.ndarray) -> np.ndarray:
    """forward_2d (fft.rs:137-148) with the radix-2 f32 FFT: rows, then columns"""
    a = fft_radix2_c64(buf_f32.astype(np.complex64))
    return np.ascontiguousarray(fft_radix2_c64(np.ascontiguousarray(a.T)).T)


def fft2_truth(buf_f64: np.ndarray) -> np.ndarray:
    return np.fft.fft2(buf_f64.astype(np.complex128))


def fft2_forward_truth(image, windowed, fft_rows, fft_cols, win_y=None, win_x=None):
    """ab_fft2_forward_f32's truth.  The windows are inputs of that entry point: truth takes the given f32 tables exactly"""
    wy = wx = None
    if windowed:
        wy, wx = np.asarray(win_y, np.float64), np.asarray(win_x, np.float64)
    return fft2_truth(prepare_buffer(image, wy, wx, fft_rows, fft_cols, np.float64))


def fft2_forward_yardstick(image, windowed, fft_rows, fft_cols, win_y=None, win_x=None):
    wy = wx = None
    if windowed:
        wy, wx = np.asarray(win_y, f32), np.asarray(win_x, f32)
    return fft2_yardstick(prepare_buffer(image, wy, wx, fft_rows, fft_cols, f32))


# ---- compute_power_spectrum_opts (fft.rs:23-68) ----
def _display(log_plane: np.ndarray, dtype) -> np.ndarray:
    """fftshift (fft.rs:39-50) and, beyond 1024^2, the s x s block mean (:70-97) in `dtype`"""
    size = log_plane.shape[0]
    shifted = np.roll(log_plane, (size // 2, size // 2), axis=(0, 1))  # out[r][c] = in[(r + half) % size][(c + half) % size]
    if size <= MAX_DISPLAY_SIZE:
        return np.ascontiguousarray(shifted)
    s = size // MAX_DISPLAY_SIZE
    blocks = shifted.reshape(MAX_DISPLAY_SIZE, s, MAX_DISPLAY_SIZE, s)
    sums = blocks.sum(axis=3, dtype=dtype).sum(axis=1, dtype=dtype)
    return (sums / dtype(s * s)).astype(dtype)


def power_spectrum_truth(image, apply_window=True) -> np.ndarray:
    image = np.asarray(image, f32)
    rows, cols = image.shape
    size, _ = power_spectrum_dims(rows, cols)
    wy = hann_symmetric_f64(rows) if apply_window else None
    wx = hann_symmetric_f64(cols) if apply_window else None
    F = fft2_truth(prepare_buffer(image, wy, wx, size, size, np.float64))
    return _display(np.log1p(np.abs(F)), np.float64)


def power_spectrum_yardstick(image, apply_window=True) -> np.ndarray:
    image = np.asarray(image, f32)
    rows, cols = image.shape
    size, _ = power_spectrum_dims(rows, cols)
    wy = hann_symmetric_f32(rows) if apply_window else None
    wx = hann_symmetric_f32(cols) if apply_window else None
    F = fft2_yardstick(prepare_buffer(image, wy, wx, size, size, f32))
    re, im = F.real.astype(f32), F.imag.astype(f32)
    mag = np.sqrt((re * re + im * im).astype(f32)).astype(f32)      # complex::norm (math/complex.rs:7-9)
    return _display(np.log((f32(1.0) + mag).astype(f32)).astype(f32), f32)  # (1.0 + mag).ln()


# ---- the command's per-pixel part (cmd/analysis/mod.rs:66-96) ----
def spectrum_to_u8(spectrum: np.ndarray):
    """(bytes, min, max, dc) in numpy f32: f32::min / f32::max skip a NaN; `as u8` truncates, saturates and sends NaN to 0"""
    v = np.asarray(spectrum, f32)
    mn = f32(np.fmin.reduce(v.ravel(), initial=f32(np.inf)))
    mx = f32(np.fmax.reduce(v.ravel(), initial=f32(-np.inf)))
    rng = f32(np.fmax(f32(mx - mn), f32(1e-10)))
    inv = f32(f32(255.0) / rng)
    x = ((v - mn).astype(f32) * inv).astype(f32)
    with np.errstate(invalid="ignore"):
        clipped = np.where(np.isnan(x), f32(0), np.clip(x, f32(0), f32(255)))
    rows, cols = v.shape
    return np.trunc(clipped).astype(np.uint8), mn, mx, f32(v[rows // 2, cols // 2])


def make_image(rows: int, cols: int, seed: int = 0) -> np.ndarray:
    """noise plus a few Gaussian blobs on a pedestal: what a calibrated frame looks like to an FFT"""
    rng = np.random.default_rng(seed)
    img = 100.0 + 5.0 * rng.standard_normal((rows, cols))
    yy, xx = np.mgrid[0:rows, 0:cols]
    for _ in range(6):
        cy, cx = rng.uniform(0, rows), rng.uniform(0, cols)
        sig = rng.uniform(1.0, 4.0)
        img += rng.uniform(200.0, 3000.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sig * sig))
    return img.astype(f32)
