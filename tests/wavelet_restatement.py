"""Independent restatement of core/imaging/wavelet.rs (wavelet_denoise :41-133, atrous_smooth_buffers :135-186, estimate_noise_sigma
:203-216, atrous_noise_scaling :218-225, soft / hard_threshold_slice :227-244), written from the Rust and used only as the checker.

Everything a pixel goes through is f32, one operation at a time: a product rounded to f32, then a sum rounded to f32, taps in the
order ki = 0 .. 4 from 0.0f (numpy's float32 arithmetic rounds once per operation, exactly what the Rust does without fused
multiply-add).  Borders clamp through index arrays.  Rust's signum is np.copysign(1, v) (+-1 for +-0; NaN only matters where the
value is NaN already).  The median is taken by a full sort, the even case averaged in f32 (math/median.rs:46-63).  The vertical
pass exists in both of the reference's routes -- straight, and through an explicit transpose (:157-172) -- so a test can pin that
the route changes no bit.  `wavelet_denoise_torch` is the same arithmetic as eager elementwise torch ops on a device (mul, then
add: two IEEE operations), for the full-size GPU test.
"""
import numpy as np

F32 = np.float32
B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0], np.float32) / np.float32(16.0)  # B3_KERNEL_1D (:35): each quotient is exact
MAD_TO_SIGMA = 1.4826                                                     # types/constants.rs:7
TRANSPOSE_THRESHOLD_STEP = 16                                             # (:38)
TRANSPOSE_THRESHOLD_ROWS = 256                                            # (:39)
NOISE_TABLE = (0.8908, 0.2007, 0.0856, 0.0413, 0.0205, 0.0103, 0.0051)    # (:219)
DEFAULT_THRESHOLDS = (3.0, 2.5, 2.0, 1.5, 1.0)                            # (:17-25)


def clamp_scales(num_scales: int) -> int:
    return min(max(int(num_scales), 1), 8)  # (:47)


def smooth_rows(src: np.ndarray, step: int) -> np.ndarray:
    """the horizontal pass (:144-155)"""
    cols = src.shape[1]
    x = np.arange(cols)
    total = np.zeros(src.shape, F32)
    with np.errstate(all="ignore"):
        for ki in range(5):
            cx = np.clip(x + (ki - 2) * step, 0, cols - 1)
            total = (total + (src[:, cx] * B3[ki]).astype(F32)).astype(F32)
    return total


def smooth_cols(h: np.ndarray, step: int) -> np.ndarray:
    """the vertical pass, straight route (:174-184)"""
    rows = h.shape[0]
    y = np.arange(rows)
    total = np.zeros(h.shape, F32)
    with np.errstate(all="ignore"):
        for ki in range(5):
            cy = np.clip(y + (ki - 2) * step, 0, rows - 1)
            total = (total + (h[cy, :] * B3[ki]).astype(F32)).astype(F32)
    return total


def smooth_cols_transposed(h: np.ndarray, step: int) -> np.ndarray:
    """the vertical pass through block_transpose (:157-172, :188-201): t[x * rows + y] = h[y * cols + x], taps read along t's rows"""
    rows, cols = h.shape
    t = np.ascontiguousarray(h.T)  # (cols, rows)
    y = np.arange(rows)
    total = np.zeros((rows, cols), F32)
    with np.errstate(all="ignore"):
        for ki in range(5):
            cy = np.clip(y + (ki - 2) * step, 0, rows - 1)
            total = (total + (t[:, cy].T * B3[ki]).astype(F32)).astype(F32)
    return total


def takes_transposed_route(rows: int, step: int) -> bool:
    return step > TRANSPOSE_THRESHOLD_STEP and rows > TRANSPOSE_THRESHOLD_ROWS  # (:157)


def atrous_smooth(src: np.ndarray, step: int, route: str = "reference") -> np.ndarray:
    """atrous_smooth_buffers (:135-186).  route: "reference" (the route the Rust takes for this size), "plain" or "transposed"."""
    h = smooth_rows(src, step)
    transposed = takes_transposed_route(src.shape[0], step) if route == "reference" else route == "transposed"
    return smooth_cols_transposed(h, step) if transposed else smooth_cols(h, step)


def median_f32(values: np.ndarray) -> np.float32:
    """median_f32_mut (math/median.rs:46-63) by a full sort"""
    n = values.size
    if n == 0:
        return F32(0.0)
    s = np.sort(values.astype(F32))
    if n % 2 == 0:
        return F32(F32(s[n // 2 - 1] + s[n // 2]) / F32(2.0))
    return F32(s[n // 2])


def estimate_noise_sigma(finest: np.ndarray) -> float:
    """estimate_noise_sigma (:203-216) -> f64"""
    v = finest.ravel()
    v = np.abs(v[np.isfinite(v)])
    if v.size == 0:
        return 0.0
    return float(np.float64(median_f32(v)) * np.float64(MAD_TO_SIGMA))


def noise_scaling(scale: int) -> float:
    """atrous_noise_scaling (:218-225)"""
    if scale < len(NOISE_TABLE):
        return NOISE_TABLE[scale]
    return NOISE_TABLE[6] / (2.0 ** (scale - 6))


def scale_thresholds(noise_sigma: float, thresholds, num_scales: int = 8) -> np.ndarray:
    """the per-scale f32 thresholds of (:93-99): ts * (f32)(noise_sigma * scaling(j)), the inner product in f64"""
    th = [F32(t) for t in thresholds]
    out = np.zeros(num_scales, F32)
    with np.errstate(all="ignore"):
        for j in range(num_scales):
            ts = th[j] if j < len(th) else (th[-1] if th else F32(1.0))
            out[j] = F32(ts * F32(np.float64(noise_sigma) * np.float64(noise_scaling(j))))
    return out


def soft_threshold(d: np.ndarray, t) -> np.ndarray:
    """soft_threshold_slice (:227-236)"""
    with np.errstate(all="ignore"):
        a = np.abs(d)
        shrunk = (np.copysign(F32(1.0), d) * (a - F32(t)).astype(F32)).astype(F32)
        return np.where(a <= F32(t), F32(0.0), shrunk).astype(F32)


def hard_threshold(d: np.ndarray, t) -> np.ndarray:
    """hard_threshold_slice (:238-244)"""
    with np.errstate(all="ignore"):
        return np.where(np.abs(d) <= F32(t), F32(0.0), d).astype(F32)


def progress_stages(num_scales: int):
    """the stage strings in the order the reference ticks them (:62-67, :86-91, :108-110); the total is their count, 2 S + 1"""
    s = clamp_scales(num_scales)
    return ([f"decomposing scale {i + 1}/{s}" for i in range(s)] + [f"thresholding scale {i + 1}/{s}" for i in range(s)]
            + ["reconstructing"])


def wavelet_denoise(image: np.ndarray, num_scales: int = 5, thresholds=DEFAULT_THRESHOLDS, linear_denoise: bool = True,
                    route: str = "reference"):
    """wavelet_denoise (:41-133) -> (denoised f32, scales_processed, noise_estimate f64)"""
    s = clamp_scales(num_scales)
    current = np.ascontiguousarray(image, dtype=F32)
    details = []
    with np.errstate(all="ignore"):
        for j in range(s):
            smoothed = atrous_smooth(current, 1 << j, route)
            details.append((current - smoothed).astype(F32))  # (:72-76)
            current = smoothed
        noise_sigma = estimate_noise_sigma(details[0])
        t = scale_thresholds(noise_sigma, thresholds, s)
        total = current.copy()
        for j in range(s):
            d = soft_threshold(details[j], t[j]) if linear_denoise else hard_threshold(details[j], t[j])
            total = (total + d).astype(F32)  # (:116-119: c_S, then d_0, d_1, ...)
        out = np.where(np.isfinite(total) & (total >= F32(0.0)), total, F32(0.0)).astype(F32)  # (:120)
    return out, s, noise_sigma


# ---- the same arithmetic as eager torch ops on a device ------------------------------------------------------------------------
def _smooth_torch(torch, src, step):
    rows, cols = src.shape
    taps = [float(v) for v in B3]  # (f32 values, exactly representable as Python floats; torch multiplies an f32 tensor by them in f32)
    x = torch.arange(cols, device=src.device)
    h = torch.zeros_like(src)
    for ki in range(5):
        cx = torch.clamp(x + (ki - 2) * step, 0, cols - 1)
        h = torch.add(h, torch.mul(src.index_select(1, cx), taps[ki]))
    y = torch.arange(rows, device=src.device)
    out = torch.zeros_like(src)
    for ki in range(5):
        cy = torch.clamp(y + (ki - 2) * step, 0, rows - 1)
        out = torch.add(out, torch.mul(h.index_select(0, cy), taps[ki]))
    return out


def wavelet_denoise_torch(image, num_scales: int = 5, thresholds=DEFAULT_THRESHOLDS, linear_denoise: bool = True, device="cuda"):
    """wavelet_denoise with every plane operation an eager f32 torch op on `device` -> (denoised tensor, scales, noise_estimate)"""
    import torch
    s = clamp_scales(num_scales)
    current = torch.as_tensor(image, dtype=torch.float32, device=device).contiguous()
    d0 = None
    planes = [current]
    for j in range(s):
        planes.append(_smooth_torch(torch, planes[-1], 1 << j))
    d0 = (planes[0] - planes[1]).flatten()
    v = d0[torch.isfinite(d0)].abs()
    n = int(v.numel())
    if n == 0:
        noise_sigma = 0.0
    else:
        srt = torch.sort(v).values
        del v
        if n % 2 == 0:
            med = F32(F32(F32(srt[n // 2 - 1].item()) + F32(srt[n // 2].item())) / F32(2.0))
        else:
            med = F32(srt[n // 2].item())
        del srt
        noise_sigma = float(np.float64(med) * np.float64(MAD_TO_SIGMA))
    del d0
    t = scale_thresholds(noise_sigma, thresholds, s)
    total = planes[s].clone()
    for j in range(s):
        d = planes[j] - planes[j + 1]
        a = d.abs()
        tj = float(t[j])
        if linear_denoise:
            kept = torch.mul(torch.copysign(torch.ones_like(d), d), torch.sub(a, tj))
        else:
            kept = d
        d = torch.where(a <= tj, torch.zeros_like(d), kept)
        total = torch.add(total, d)
    out = torch.where(torch.isfinite(total) & (total >= 0.0), total, torch.zeros_like(total))
    return out, s, noise_sigma
