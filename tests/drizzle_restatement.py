"""numpy restatement of core/stacking/drizzle.rs (drizzle_frame :46-122, push :38-45, finalize :124-199, the checks and dims of
drizzle_stack :231-279), written from the Rust: the SCATTER formulation.  Three forms:

  drizzle_loop     plain loops, the Rust line for line (tiny images only)
  drizzle          the same, vectorised: every contribution of every frame as arrays in the order the reference produces them (frame,
                   input row, input column, output row, output column), ranked per output pixel, rank >= cap dropped; the MAD clip
                   vectorised over the pixels with an active mask (no assumption about which samples a round keeps)
  gather_pixel     ONE output pixel's list and weight by walking, per frame, the input pixels that can reach it (the formulation the
                   GPU kernel uses, with a range of its own, deliberately generous); test_drizzle_cpu.py proves it equal to the scatter
                   lists element for element, and the full-size GPU test uses it on a sample of pixels

math.exp / math.sin are glibc's, as Rust's f64::exp / sin on this platform: the weights are the reference's.  Results also carry, per
output pixel, whether any candidate's weight lay within 1e-6 relative of the 1e-12 threshold (`threshold`), the pixel's own rejected
count, and whether the f64 sum behind its mean is exact (every partial sum representable: then the order of summation cannot matter).
The survivors are summed in ascending order of value (what oracle/orc_combine.c pins for the order select_nth_unstable leaves open)."""
import math
from dataclasses import dataclass

import numpy as np

SQUARE, GAUSSIAN, LANCZOS3 = 0, 1, 2
MAD_TO_SIGMA = 1.4826
W_MIN = 1e-12
F32 = np.float32


@dataclass
class Result:
    image: np.ndarray      # f32 (out_rows, out_cols)
    weight: np.ndarray     # f32
    rejected: int
    rejected_map: np.ndarray  # per-pixel rejected counts
    threshold: np.ndarray  # bool: a candidate weight within 1e-6 relative of 1e-12
    exact: np.ndarray      # bool: the mean's f64 sum is exact
    counts: np.ndarray     # samples kept per pixel
    dims: tuple            # (in_rows, in_cols, out_rows, out_cols)
    lists: list = None     # drizzle_loop / keep_lists: per-pixel [values], in push order
    wsum: np.ndarray = None  # f64 weight sums


def output_dims(shapes, scale, pixfrac):
    """drizzle_stack :231-279 -> (in_rows, in_cols, out_rows, out_cols, scale, pixfrac); ValueError with the reference's message."""
    n = len(shapes)
    if n == 0:
        raise ValueError("No images to drizzle")
    if n < 2:
        raise ValueError("Drizzle requires at least 2 frames for sub-pixel reconstruction")
    min_r, max_r = min(s[0] for s in shapes), max(s[0] for s in shapes)
    min_c, max_c = min(s[1] for s in shapes), max(s[1] for s in shapes)
    tol = int(float(max(min_r, min_c)) * 0.05)
    if max_r - min_r > tol or max_c - min_c > tol:
        raise ValueError(f"Frame dimensions vary too much (rows: {max_r - min_r}px, cols: {max_c - min_c}px, tolerance: {tol}px)")
    scale = min(max(float(scale), 1.0), 4.0)
    pixfrac = min(max(float(pixfrac), 0.1), 1.0)
    return min_r, min_c, int(math.ceil(min_r * scale)), int(math.ceil(min_c * scale)), scale, pixfrac


def clamp_index(i, n):
    return 0 if i < 0 else (n - 1 if i >= n else i)


def overlap_area(ax1, ay1, ax2, ay2, bx1, by1, bx2, by2):
    ox = max(min(ax2, bx2) - max(ax1, bx1), 0.0)
    oy = max(min(ay2, by2) - max(ay1, by1), 0.0)
    return ox * oy


def lanczos3(x):
    if abs(x) < 1e-12:
        return 1.0
    if abs(x) >= 3.0:
        return 0.0
    pi_x = math.pi * x
    pi_x_3 = pi_x / 3.0
    return (math.sin(pi_x) / pi_x) * (math.sin(pi_x_3) / pi_x_3)


def weight(kernel, cx, cy, half, ox, oy):
    if kernel == SQUARE:
        return overlap_area(cx - half, cy - half, cx + half, cy + half, float(ox), float(oy), ox + 1.0, oy + 1.0)
    if kernel == GAUSSIAN:
        ex, ey = ox + 0.5 - cx, oy + 0.5 - cy
        dist2 = ex * ex + ey * ey  # (:91-92 powi(2) is a multiplication: +inf for an offset of 1e300, where Python's ** raises)
        sigma = max(half, 0.5)
        return math.exp(-dist2 / (2.0 * sigma * sigma))
    return lanczos3(abs(ox + 0.5 - cx)) * lanczos3(abs(oy + 0.5 - cy))


def near_threshold(w):
    return abs(w - W_MIN) <= 1e-6 * W_MIN


def median_f32(vals):
    """median_f32_mut (math/median.rs:46-61) of a list of np.float32"""
    s = sorted(vals)
    n = len(s)
    if n == 0:
        return F32(0.0)
    if n % 2 == 0:
        return F32(F32(s[n // 2 - 1] + s[n // 2]) / F32(2.0))
    return s[n // 2]


def two_sum_exact(vals):
    """sequential f64 sum of `vals` and whether every partial sum was exact"""
    s, exact = 0.0, True
    for v in vals:
        v = float(v)
        t = s + v
        bb = t - s
        if (s - (t - bb)) + (v - bb) != 0.0:
            exact = False
        s = t
    return s, exact


def finalize_pixel(samples, wsum, sigma_low, sigma_high, iters):
    """finalize (:134-189) of one pixel -> (value f32, weight f32, rejected, exact)"""
    count = len(samples)
    if count == 0:
        return F32(0.0), F32(0.0), 0, True
    if count == 1:
        return F32(samples[0]), F32(wsum), 0, True
    sl, sh = F32(sigma_low), F32(sigma_high)
    active = [F32(v) for v in samples]
    rejected = 0
    with np.errstate(all="ignore"):
        for _ in range(iters):
            if len(active) < 3:
                break
            med = median_f32(active)
            mad = median_f32([F32(abs(F32(v - med))) for v in active])
            sigma = F32(max(float(mad) * MAD_TO_SIGMA, 1e-10))
            lo, hi = F32(-sl * sigma), F32(sh * sigma)
            kept = [v for v in active if bool(F32(v - med) >= lo) and bool(F32(v - med) <= hi)]
            removed = len(active) - len(kept)
            active = kept
            rejected += removed
            if removed == 0:
                break
    if not active:
        s, e1 = two_sum_exact(samples)
        _, e2 = two_sum_exact(sorted(samples))
        return F32(s / count), F32(wsum), rejected, e1 and e2
    s, e = two_sum_exact(sorted(active))
    return F32(s / len(active)), F32(wsum), rejected, e


def _prepare(frames, offsets, scale, pixfrac):
    in_rows, in_cols, out_rows, out_cols, scale, pixfrac = output_dims([f.shape for f in frames], scale, pixfrac)
    frames = [np.asarray(f, np.float32)[:in_rows, :in_cols] for f in frames]
    cap = max(2 * len(frames), 4)
    return frames, in_rows, in_cols, out_rows, out_cols, scale, pixfrac, cap


def drizzle_loop(frames, offsets, scale=2.0, pixfrac=0.7, kernel=SQUARE, sigma_low=3.0, sigma_high=3.0, iters=5):
    frames, in_rows, in_cols, out_rows, out_cols, scale, pixfrac, cap = _prepare(frames, offsets, scale, pixfrac)
    n_out = out_rows * out_cols
    lists = [[] for _ in range(n_out)]
    wsum = np.zeros(n_out, np.float64)
    thr = np.zeros(n_out, bool)
    half = pixfrac * scale * 0.5
    for f, img in enumerate(frames):
        dx, dy = -float(offsets[f][0]), -float(offsets[f][1])
        for iy in range(in_rows):
            for ix in range(in_cols):
                val = img[iy, ix]
                if not np.isfinite(val):
                    continue
                cx = (ix + dx) * scale
                cy = (iy + dy) * scale
                ox_min = clamp_index(math.floor(cx - half), out_cols)
                ox_max = clamp_index(math.ceil(cx + half), out_cols)
                oy_min = clamp_index(math.floor(cy - half), out_rows)
                oy_max = clamp_index(math.ceil(cy + half), out_rows)
                for oy in range(oy_min, oy_max + 1):
                    for ox in range(ox_min, ox_max + 1):
                        w = weight(kernel, cx, cy, half, ox, oy)
                        idx = oy * out_cols + ox
                        if near_threshold(w):
                            thr[idx] = True
                        if w > W_MIN and len(lists[idx]) < cap:
                            lists[idx].append(val)
                            wsum[idx] += w
    image = np.zeros(n_out, np.float32)
    wmap = np.zeros(n_out, np.float32)
    rej = np.zeros(n_out, np.int64)
    exact = np.ones(n_out, bool)
    for i in range(n_out):
        image[i], wmap[i], rej[i], exact[i] = finalize_pixel(lists[i], wsum[i], sigma_low, sigma_high, iters)
    shp = (out_rows, out_cols)
    return Result(image.reshape(shp), wmap.reshape(shp), int(rej.sum()), rej.reshape(shp), thr.reshape(shp), exact.reshape(shp),
                  np.array([len(l) for l in lists]).reshape(shp), (in_rows, in_cols, out_rows, out_cols), lists, wsum.reshape(shp))


_exp = np.frompyfunc(math.exp, 1, 1)
_lz = np.frompyfunc(lanczos3, 1, 1)


def _frame_contributions(img, dx, dy, scale, half, kernel, out_rows, out_cols):
    """every (idx, val, w, near-threshold) of one frame with the weight test still to come, in (iy, ix, oy, ox) order"""
    in_rows, in_cols = img.shape
    cx = (np.arange(in_cols, dtype=np.float64) + dx) * scale
    cy = (np.arange(in_rows, dtype=np.float64) + dy) * scale

    def window(c, n_out):
        lo = np.clip(np.floor(c - half), 0, n_out - 1).astype(np.int64)
        hi = np.clip(np.ceil(c + half), 0, n_out - 1).astype(np.int64)
        return lo, hi

    x0, x1 = window(cx, out_cols)
    y0, y1 = window(cy, out_rows)
    wx, wy = int((x1 - x0).max()) + 1, int((y1 - y0).max()) + 1
    iy, ix, ky, kx = np.meshgrid(np.arange(in_rows), np.arange(in_cols), np.arange(wy), np.arange(wx), indexing="ij")
    oy = y0[iy] + ky
    ox = x0[ix] + kx
    ok = (oy <= y1[iy]) & (ox <= x1[ix]) & np.isfinite(img)[iy, ix]
    iy, ix, oy, ox = iy[ok], ix[ok], oy[ok], ox[ok]  # (boolean indexing keeps C order: iy, ix, oy, ox)
    pcx, pcy = cx[ix], cy[iy]
    oxf, oyf = ox.astype(np.float64), oy.astype(np.float64)
    if kernel == SQUARE:
        w = (np.maximum(np.minimum(pcx + half, oxf + 1.0) - np.maximum(pcx - half, oxf), 0.0)
             * np.maximum(np.minimum(pcy + half, oyf + 1.0) - np.maximum(pcy - half, oyf), 0.0))
    elif kernel == GAUSSIAN:
        ex, ey = oxf + 0.5 - pcx, oyf + 0.5 - pcy
        with np.errstate(over="ignore"):  # (an offset of 1e300: +inf, as in the reference; the weight is exp(-inf) = 0)
            dist2 = ex * ex + ey * ey
        sigma = max(half, 0.5)
        arg = -dist2 / (2.0 * sigma * sigma)
        w = np.zeros_like(arg)
        sel = arg > -40.0  # (exp(-40) = 4e-18: far below the threshold and its 1e-6 window; glibc's exp on everything that can matter)
        w[sel] = _exp(arg[sel]).astype(np.float64)
    else:
        w = _lz(np.abs(oxf + 0.5 - pcx)).astype(np.float64) * _lz(np.abs(oyf + 0.5 - pcy)).astype(np.float64)
    return oy * out_cols + ox, img[iy, ix], w


def finalize_many(V, counts, wsum, sigma_low, sigma_high, iters):
    """finalize over all pixels at once.  V: (npix, cap) f32, row i's first counts[i] entries in push order."""
    npix, cap = V.shape
    sl, sh = F32(sigma_low), F32(sigma_high)
    col = np.arange(cap)[None, :]
    active = col < counts[:, None]
    rejected = np.zeros(npix, np.int64)
    running = counts >= 2
    rows = np.arange(npix)
    with np.errstate(all="ignore"):
        def masked_median(X, act):
            S = np.sort(np.where(act, X, F32(np.inf)), axis=1)
            m = act.sum(axis=1)
            mid = np.minimum(m // 2, cap - 1)
            right = S[rows, mid]
            left = S[rows, np.maximum(mid - 1, 0)]
            return np.where(m % 2 == 0, ((left + right) / F32(2.0)).astype(np.float32), right)

        for _ in range(iters):
            m = active.sum(axis=1)
            running &= m >= 3
            if not running.any():
                break
            med = masked_median(V, active)
            dev = (V - med[:, None]).astype(np.float32)
            mad = masked_median(np.abs(dev), active)
            sigma = np.maximum(mad.astype(np.float64) * MAD_TO_SIGMA, 1e-10).astype(np.float32)
            lo, hi = (-sl * sigma).astype(np.float32), (sh * sigma).astype(np.float32)
            keep = active & (dev >= lo[:, None]) & (dev <= hi[:, None])
            removed = m - keep.sum(axis=1)
            removed = np.where(running, removed, 0)
            active = np.where(running[:, None], keep, active)
            rejected += removed
            running &= removed > 0

    def seq_sum(X, act):  # sequential f64 sum over the columns, with the exactness of every step
        s = np.zeros(npix)
        exact = np.ones(npix, bool)
        Xd = np.where(act, X, 0.0).astype(np.float64)
        for k in range(cap):
            v = Xd[:, k]
            t = s + v
            bb = t - s
            exact &= ((s - (t - bb)) + (v - bb)) == 0.0
            s = t
        return s, exact

    none = (active.sum(axis=1) == 0) & (counts >= 2)
    allv = col < counts[:, None]
    order = np.argsort(np.where(allv, V, F32(np.inf)), axis=1, kind="stable")
    Vs = np.take_along_axis(V, order, axis=1)
    act_s = np.take_along_axis(np.where(none[:, None], allv, active), order, axis=1)
    s_asc, e_asc = seq_sum(Vs, act_s)
    s_push, e_push = seq_sum(V, allv)
    nact = act_s.sum(axis=1)
    s = np.where(none, s_push, s_asc)
    exact = np.where(none, e_push & e_asc, e_asc)
    with np.errstate(all="ignore"):
        image = (s / np.maximum(nact, 1)).astype(np.float32)
    image = np.where(counts == 0, F32(0.0), image)
    image = np.where(counts == 1, V[:, 0], image).astype(np.float32)
    wmap = np.where(counts == 0, 0.0, wsum).astype(np.float32)
    exact = np.where(counts <= 1, True, exact)
    return image, wmap, rejected, exact


def drizzle(frames, offsets, scale=2.0, pixfrac=0.7, kernel=SQUARE, sigma_low=3.0, sigma_high=3.0, iters=5, keep_lists=False):
    frames, in_rows, in_cols, out_rows, out_cols, scale, pixfrac, cap = _prepare(frames, offsets, scale, pixfrac)
    n_out = out_rows * out_cols
    half = pixfrac * scale * 0.5
    idx_l, val_l, w_l = [], [], []
    thr = np.zeros(n_out, bool)
    for f, img in enumerate(frames):
        idx, val, w = _frame_contributions(img, -float(offsets[f][0]), -float(offsets[f][1]), scale, half, kernel, out_rows, out_cols)
        thr[idx[np.abs(w - W_MIN) <= 1e-6 * W_MIN]] = True
        sel = w > W_MIN
        idx_l.append(idx[sel])
        val_l.append(val[sel])
        w_l.append(w[sel])
    idx, val, w = np.concatenate(idx_l), np.concatenate(val_l), np.concatenate(w_l)
    order = np.argsort(idx, kind="stable")  # groups by output pixel, keeps the push order inside a group
    idx, val, w = idx[order], val[order], w[order]
    start = np.searchsorted(idx, np.arange(n_out), side="left")
    rank = np.arange(idx.size) - start[idx]
    sel = rank < cap  # push (:38-45)
    idx, val, w, rank = idx[sel], val[sel], w[sel], rank[sel]
    V = np.zeros((n_out, cap), np.float32)
    W = np.zeros((n_out, cap), np.float64)
    V[idx, rank] = val
    W[idx, rank] = w
    counts = np.bincount(idx, minlength=n_out).astype(np.int64)
    wsum = np.zeros(n_out)
    for k in range(cap):  # the f64 weight sum in push order
        wsum = wsum + W[:, k]
    image, wmap, rej, exact = finalize_many(V, counts, wsum, sigma_low, sigma_high, iters)
    shp = (out_rows, out_cols)
    lists = [list(V[i, :counts[i]]) for i in range(n_out)] if keep_lists else None
    return Result(image.reshape(shp), wmap.reshape(shp), int(rej.sum()), rej.reshape(shp), thr.reshape(shp), exact.reshape(shp), counts.reshape(shp),
                  (in_rows, in_cols, out_rows, out_cols), lists, wsum.reshape(shp))


def gather_pixel(frames, offsets, oy, ox, scale=2.0, pixfrac=0.7, kernel=SQUARE):
    """One output pixel's (samples in push order, f64 weight sum) by walking the input pixels that can reach it.  `frames` may be
    larger than the cropped dims (they are cropped by indexing).  The candidate range is generous on purpose: everything within
    max(half + 1.5, reach) + 2 output pixels of the pixel's centre, reach = 7.5 sigma (Gaussian), 3 (Lanczos3), half + 0.5 (Square)."""
    in_rows, in_cols, out_rows, out_cols, scale, pixfrac = output_dims([f.shape for f in frames], scale, pixfrac)
    cap = max(2 * len(frames), 4)
    half = pixfrac * scale * 0.5
    reach = {SQUARE: half + 0.5, GAUSSIAN: 7.5 * max(half, 0.5), LANCZOS3: 3.0}[kernel]
    R = max(half + 1.5, reach) + 2.0
    samples, wsum = [], 0.0
    for f, img in enumerate(frames):
        if len(samples) >= cap:
            break
        dx, dy = -float(offsets[f][0]), -float(offsets[f][1])

        def cand(o, d, n_in):
            lo = max(int(math.floor((o + 0.5 - R) / scale - d)) - 1, 0)
            hi = min(int(math.ceil((o + 0.5 + R) / scale - d)) + 1, n_in - 1)
            return range(lo, hi + 1)

        for iy in cand(oy, dy, in_rows):
            cy = (iy + dy) * scale
            if not clamp_index(math.floor(cy - half), out_rows) <= oy <= clamp_index(math.ceil(cy + half), out_rows):
                continue
            for ix in cand(ox, dx, in_cols):
                val = img[iy, ix]
                if not np.isfinite(val):
                    continue
                cx = (ix + dx) * scale
                if not clamp_index(math.floor(cx - half), out_cols) <= ox <= clamp_index(math.ceil(cx + half), out_cols):
                    continue
                w = weight(kernel, cx, cy, half, ox, oy)
                if w > W_MIN and len(samples) < cap:
                    samples.append(val)
                    wsum += w
    return samples, wsum
