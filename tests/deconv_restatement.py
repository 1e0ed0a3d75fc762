"""Independent restatement of core/analysis/deconvolution.rs (richardson_lucy :141-221, FftConvolver :36-124, apply_deringing
:223-245, generate_gaussian_psf :12-33), written from the Rust and used only as the checker.

The convolution is the reference's own: an FFT over a power-of-two buffer of next_pow2(rows + pr - 1) x next_pow2(cols + pc - 1)
(math/fft.rs:122-127), the image at [0, rows) x [0, cols), PSF tap (y, x) at ((y - pr/2) rem_euclid F, (x - pc/2) rem_euclid F),
the transpose through the conjugate spectrum, the real part of the window kept.  `dtype` switches the precision:
  float64 (complex128 FFTs)  the truth the GPU is held to;
  float32 (complex64 FFTs, f32 rounding where the Rust rounds)  stands in for the reference's own precision.
Rust's f32::max is np.fmax (NaN -> the other operand).  expf is glibc's, through ctypes, so the Gaussian PSF compares bit for bit.
"""
import ctypes
import math

import numpy as np

_libm = ctypes.CDLL("libm.so.6")
_libm.expf.argtypes = [ctypes.c_float]
_libm.expf.restype = ctypes.c_float

F64_MAX = float(np.finfo(np.float64).max)
EPSILON = np.float32(1e-6)     # :166
THRESHOLD = 1e-6               # convergence_threshold, :148


def expf(x) -> np.float32:
    return np.float32(_libm.expf(float(np.float32(x))))


def gaussian_psf(size: int, sigma: float) -> np.ndarray:
    """generate_gaussian_psf (:12-33): f32 throughout, row-major running sum, v / sum if sum > 0"""
    f = np.float32
    psf = np.zeros((size, size), f)
    center = f(size - 1) / f(2.0)
    sigma2 = f(2.0) * f(sigma) * f(sigma)
    total = f(0.0)
    with np.errstate(all="ignore"):
        for y in range(size):
            for x in range(size):
                dy = f(y) - center
                dx = f(x) - center
                val = expf(-((dx * dx + dy * dy) / sigma2))
                psf[y, x] = val
                total = f(total + val)
        if total > 0:
            psf = (psf / total).astype(f)
    return psf


def next_pow2(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


class Convolver:
    """FftConvolver (:36-124) in numpy"""

    def __init__(self, rows, cols, psf, dtype=np.float64):
        pr, pc = psf.shape
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.cdt = np.complex64 if dtype == np.float32 else np.complex128
        self.fr, self.fc = next_pow2(rows + pr - 1), next_pow2(cols + pc - 1)
        buf = np.zeros((self.fr, self.fc), self.cdt)
        ys = (np.arange(pr) - pr // 2) % self.fr      # rem_euclid, integer pr / 2
        xs = (np.arange(pc) - pc // 2) % self.fc
        buf[np.ix_(ys, xs)] = psf.astype(dtype)
        self.h = np.fft.fft2(buf)
        self.h_conj = np.conj(self.h)

    def _conv(self, image, spec):
        buf = np.zeros((self.fr, self.fc), self.cdt)
        buf[:self.rows, :self.cols] = image
        out = np.fft.ifft2(np.fft.fft2(buf) * spec)
        assert out.dtype == self.cdt
        return np.ascontiguousarray(out[:self.rows, :self.cols].real).astype(self.dtype)

    def forward(self, image):
        return self._conv(image, self.h)

    def transpose(self, image):
        return self._conv(image, self.h_conj)


def deringing(est, orig, threshold, dtype=np.float64):
    """apply_deringing (:223-245)"""
    f = dtype
    t = f(np.float32(threshold))
    upper = orig * (f(1.0) + t)
    lower = np.fmax(orig * (f(1.0) - t), f(0.0))
    return np.where(est > upper, upper, np.where(est < lower, lower, est)).astype(f)


def richardson_lucy(image, psf, iterations=20, regularization=0.001, deringing_on=True, deringing_threshold=0.1, dtype=np.float64):
    """-> (estimate, iterations_run, convergence, [convergence of every iteration run])"""
    f = dtype
    img = np.asarray(image, np.float32).astype(f)
    psf = np.asarray(psf, np.float32)
    rows, cols = img.shape
    est = img.copy()
    conv = Convolver(rows, cols, psf, f)
    lam = f(np.float32(regularization))          # `regularization as f32`
    inv_reg = f(1.0) / (f(1.0) + lam) if lam > 0 else f(1.0)
    eps = f(EPSILON)
    last, run, deltas = F64_MAX, 0, []
    with np.errstate(all="ignore"):
        for it in range(iterations):
            c = conv.forward(est)
            ratio = (img / (c + eps)).astype(f)
            cor = conv.transpose(ratio)
            new = np.fmax(est * cor * inv_reg, f(0.0)).astype(f)       # (old * cor * inv_reg).max(0.0)
            d = (new - est).astype(np.float64)                          # f32 subtraction, then widened
            sum_sq = float(np.sum(d * d))
            est = new
            if deringing_on:
                est = deringing(est, img, deringing_threshold, f)
            run = it + 1
            last = math.sqrt(sum_sq / (rows * cols)) if not math.isnan(sum_sq) else float("nan")
            deltas.append(last)
            if last < THRESHOLD and run >= 3:
                break
    return est, run, last, deltas


def richardson_lucy_torch(image, psf, iterations=20, regularization=0.001, deringing_on=True, deringing_threshold=0.1, dtype=None,
                          device="cuda"):
    """The same through torch.fft (float64 by default): the checker of full-size frames, on whichever device torch has."""
    import torch
    dtype = dtype or torch.float64
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    img = (image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image, np.float32))).to(device=device, dtype=dtype)
    psf = np.asarray(psf, np.float32)
    rows, cols = img.shape
    pr, pc = psf.shape
    fr, fc = next_pow2(rows + pr - 1), next_pow2(cols + pc - 1)
    buf = torch.zeros((fr, fc), dtype=cdt, device=device)
    ys = torch.as_tensor((np.arange(pr) - pr // 2) % fr, device=device)
    xs = torch.as_tensor((np.arange(pc) - pc // 2) % fc, device=device)
    buf[ys[:, None], xs[None, :]] = torch.as_tensor(psf).to(device=device, dtype=cdt)
    h = torch.fft.fft2(buf)
    del buf
    hc = torch.conj(h)

    def conv(x, spec):
        b = torch.zeros((fr, fc), dtype=cdt, device=device)
        b[:rows, :cols] = x
        return torch.fft.ifft2(torch.fft.fft2(b) * spec)[:rows, :cols].real.contiguous().to(dtype)

    np_f = np.float32 if dtype == torch.float32 else np.float64
    lam = float(np_f(np.float32(regularization)))
    inv_reg = float(np_f(1.0) / (np_f(1.0) + np_f(lam))) if lam > 0 else 1.0
    t = float(np_f(np.float32(deringing_threshold)))
    upper = img * (1.0 + t)
    lower = torch.clamp(img * (1.0 - t), min=0.0)
    est = img.clone()
    last, run, deltas = F64_MAX, 0, []
    for it in range(iterations):
        ratio = img / (conv(est, h) + float(EPSILON))
        new = est * conv(ratio, hc) * inv_reg
        new = torch.where(torch.isnan(new), torch.zeros_like(new), new).clamp(min=0.0)   # f32::max(_, 0.0)
        d = (new - est).to(torch.float64)
        sum_sq = float((d * d).sum())
        est = new
        if deringing_on:
            est = torch.where(est > upper, upper, torch.where(est < lower, lower, est))
        run = it + 1
        last = math.sqrt(sum_sq / (rows * cols))
        deltas.append(last)
        if last < THRESHOLD and run >= 3:
            break
    return est, run, last, deltas


def direct_conv(image, psf, transpose=False):
    """The linear convolution with a zero boundary that the FFT product equals on the kept window (float64, for small cases)"""
    img = np.asarray(image, np.float64)
    rows, cols = img.shape
    pr, pc = psf.shape
    out = np.zeros_like(img)
    pad = np.zeros((rows + 2 * pr, cols + 2 * pc))
    pad[pr:pr + rows, pc:pc + cols] = img
    for j in range(pr):
        for i in range(pc):
            dy, dx = j - pr // 2, i - pc // 2
            if transpose:
                out += float(psf[j, i]) * pad[pr + dy:pr + dy + rows, pc + dx:pc + dx + cols]
            else:
                out += float(psf[j, i]) * pad[pr - dy:pr - dy + rows, pc - dx:pc - dx + cols]
    return out
