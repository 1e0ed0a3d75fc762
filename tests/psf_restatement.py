"""numpy / plain-Python restatement of core/imaging/psf_estimation.rs, operation for operation in f64 -- the checker of
ab_estimate_psf / ab_psf_select_stars (csrc/psf.hip), never the thing under test -- with the seeded fields the tests use.

Python floats and numpy float64 scalars / arrays are IEEE doubles and numpy never fuses a multiply with an add, so an elementwise
numpy expression written in the reference's order has the reference's bits.  SUMS the reference forms sequentially go through seq_sum
(np.cumsum(...)[-1], which adds one element after the other) or plain loops, never np.sum (pairwise)."""
import math
from dataclasses import dataclass, field

import numpy as np

DEFAULTS = dict(num_stars=30, cutout_radius=15, saturation_threshold=0.95, min_peak_fraction=0.10, max_ellipticity=0.3, edge_margin=30,
                max_center_distance_fraction=0.7)   # psf_estimation.rs:27-39

ERR_NO_STARS = "No stars detected in image"
ERR_NO_PASS = "No stars passed quality filters"
ERR_NO_CUTOUT = "Failed to extract star cutouts"


@dataclass
class Star:  # StarCandidate (:4-14)
    x: float
    y: float
    peak: float
    flux: float
    fwhm: float
    ellipticity: float
    distance_from_center: float
    snr: float

    def astuple(self):
        return (self.x, self.y, self.peak, self.flux, self.fwhm, self.ellipticity, self.distance_from_center, self.snr)


@dataclass
class Result:
    error: "str | None" = None
    kernel: "np.ndarray | None" = None          # (size, size) f32
    kernel_size: int = 0
    average_fwhm: float = 0.0
    average_ellipticity: float = 0.0
    stars_used: list = field(default_factory=list)
    stars_rejected: int = 0
    spread_pixels: float = 0.0
    stars_detected: int = 0
    stars_filtered: int = 0
    threshold: float = 0.0
    max_val: float = 0.0
    peaks: list = field(default_factory=list)   # (y, x) of every peak that survived `visited`, raster order
    cutouts_used: int = 0


def seq_sum(a) -> float:
    """0.0 + a[0] + a[1] + ... in index order"""
    a = np.asarray(a, dtype=np.float64).ravel()
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def rust_round(x: float) -> float:
    """f64::round: half away from zero (x - trunc(x) is exact)"""
    if not math.isfinite(x):
        return x
    t = float(math.trunc(x))
    if abs(x - t) >= 0.5:
        t += math.copysign(1.0, x)
    return t


def as_usize(x: float) -> int:
    """`as usize`: saturating, NaN -> 0"""
    if x != x or x <= 0.0:
        return 0
    return int(min(x, 1.8e19))


def as_i64(x: float) -> int:
    if x != x:
        return 0
    return int(max(min(x, 9.2e18), -9.2e18))


# ---- compute_image_stats (:158-188) ---------------------------------------------------------------------------------------------------
def image_stats(img):
    flat = np.ascontiguousarray(img, dtype=np.float32).ravel()
    n = float(flat.size)
    vf = flat.astype(np.float64)
    s = seq_sum(vf)
    sq = seq_sum(vf * vf)
    max_val = float(flat.max())
    mean = s / n
    var = (sq / n) - mean * mean
    stddev = math.sqrt(var) if var > 0.0 else 0.0
    mid = flat.size // 2
    median = float(np.partition(flat, mid)[mid])
    return dict(mean=mean, stddev=stddev, max_val=max_val, median=median, sum=s, sum_sq=sq)


def guard_band_empty(img, threshold, rel=1e-9) -> bool:
    """no pixel within rel * |threshold| of the detection threshold: a stddev that differs in its last bits cannot change a comparison"""
    v = np.asarray(img, dtype=np.float64)
    return not bool(np.any(np.abs(v - threshold) <= rel * abs(threshold)))


# ---- the measurements (:281-507) ------------------------------------------------------------------------------------------------------
def centroid_subpixel(img, x, y, radius=3):
    h, w = img.shape
    sum_x = sum_y = sum_w = 0.0
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w:
                val = float(img[ny, nx])
                sum_x += float(nx) * val
                sum_y += float(ny) * val
                sum_w += val
    if sum_w > 0.0:
        return sum_x / sum_w, sum_y / sum_w
    return float(x), float(y)


def subpixel_peak(img, ix, iy):
    h, w = img.shape
    if ix < 1 or iy < 1 or ix + 1 >= w or iy + 1 >= h:
        return float(img[iy, ix])

    def v(dy, dx):
        return float(img[iy + dy, ix + dx])
    c = v(0, 0)
    dx_val = (v(0, 1) - v(0, -1)) * 0.5
    dy_val = (v(1, 0) - v(-1, 0)) * 0.5
    dxx = v(0, 1) + v(0, -1) - 2.0 * c
    dyy = v(1, 0) + v(-1, 0) - 2.0 * c
    dxy = (v(1, 1) + v(-1, -1) - v(1, -1) - v(-1, 1)) * 0.25
    det = dxx * dyy - dxy * dxy
    if abs(det) < 1e-12 or det < 0.0:
        return c
    sx = -(dyy * dx_val - dxy * dy_val) / det
    sy = -(dxx * dy_val - dxy * dx_val) / det
    if abs(sx) > 1.0 or abs(sy) > 1.0:
        return c
    return c + 0.5 * (dx_val * sx + dy_val * sy)


def middle_half_mean(vals):
    """sorted, then the mean of [len / 4, max(3 len / 4, lo + 1)) summed in ascending order (:434-441, :499-506)"""
    vals = np.sort(np.asarray(vals, dtype=np.float64).ravel(), kind="stable")
    n = vals.size
    if n == 0:
        return 0.0
    lo = n // 4
    hi = min(max(3 * n // 4, lo + 1), n)
    clipped = vals[lo:hi]
    if clipped.size == 0:
        return 0.0
    return seq_sum(clipped) / float(clipped.size)


def estimate_local_bg(img, ix, iy, radius=10):
    h, w = img.shape
    inner_r2 = (float(radius) * 0.6) * (float(radius) * 0.6)
    outer_r2 = float(radius) * float(radius)
    vals = []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            py, px = iy + dy, ix + dx
            if py < 0 or py >= h or px < 0 or px >= w:
                continue
            d2 = float(dx * dx + dy * dy)
            if inner_r2 <= d2 <= outer_r2:
                vals.append(float(img[py, px]))
    return middle_half_mean(vals)


def measure_fwhm(img, x, y):
    h, w = img.shape
    ix, iy = as_usize(rust_round(x)), as_usize(rust_round(y))
    if ix >= w or iy >= h:
        return 4.0, 4.0
    peak = subpixel_peak(img, ix, iy)
    bg = estimate_local_bg(img, ix, iy, 10)
    net_peak = peak - bg
    if net_peak <= 0.0:
        return 4.0, 4.0
    threshold = bg + net_peak * 0.5
    m_xx = m_yy = m_xy = sum_w = 0.0
    for dy in range(-12, 13):
        for dx in range(-12, 13):
            py, px = iy + dy, ix + dx
            if py < 0 or py >= h or px < 0 or px >= w:
                continue
            val = float(img[py, px])
            if val < threshold:
                continue
            weight = val - bg
            fx = float(px) - x
            fy = float(py) - y
            m_xx += fx * fx * weight
            m_yy += fy * fy * weight
            m_xy += fx * fy * weight
            sum_w += weight
    if sum_w <= 0.0:
        return 4.0, 4.0
    sigma_xx, sigma_yy, sigma_xy = m_xx / sum_w, m_yy / sum_w, m_xy / sum_w
    trace = sigma_xx + sigma_yy
    det = sigma_xx * sigma_yy - sigma_xy * sigma_xy
    disc = math.sqrt(max(trace * trace - 4.0 * det, 0.0))
    lambda1 = max((trace + disc) / 2.0, 0.0)
    lambda2 = max((trace - disc) / 2.0, 0.0)
    fwhm_factor = 2.0 * math.sqrt(math.log(2.0) * 2.0)
    fwhm_major = min(max(fwhm_factor * math.sqrt(lambda1), 1.0), 30.0)
    fwhm_minor = min(max(fwhm_factor * math.sqrt(lambda2), 1.0), 30.0)
    return fwhm_major, fwhm_minor


def _window(img, x, y, radius):
    """the pixel window of aperture_flux / annulus_background (:449-452, :479-482) and its d2 plane, f64, elementwise"""
    h, w = img.shape
    y_min = as_usize(max(math.floor(y - radius), 0.0))
    y_max = min(as_usize(math.ceil(y + radius)), max(h - 1, 0))
    x_min = as_usize(max(math.floor(x - radius), 0.0))
    x_max = min(as_usize(math.ceil(x + radius)), max(w - 1, 0))
    if y_min > y_max or x_min > x_max:
        return None, None
    py = np.arange(y_min, y_max + 1, dtype=np.float64)[:, None]
    px = np.arange(x_min, x_max + 1, dtype=np.float64)[None, :]
    dx = px - x
    dy = py - y
    d2 = dx * dx + dy * dy
    return img[y_min:y_max + 1, x_min:x_max + 1], d2


def aperture_flux(img, x, y, radius):
    win, d2 = _window(img, x, y, radius)
    if win is None:
        return 0.0
    return seq_sum(win[d2 <= radius * radius].astype(np.float64))   # (boolean indexing of a C-ordered window: raster order)


def annulus_background(img, x, y, inner_r, outer_r):
    win, d2 = _window(img, x, y, outer_r)
    if win is None:
        return 0.0
    return middle_half_mean(win[(d2 >= inner_r * inner_r) & (d2 <= outer_r * outer_r)].astype(np.float64))


def annulus_count(img, x, y, inner_r, outer_r):
    win, d2 = _window(img, x, y, outer_r)
    return 0 if win is None else int(((d2 >= inner_r * inner_r) & (d2 <= outer_r * outer_r)).sum())


# ---- detect_stars_for_psf (:190-279) ------------------------------------------------------------------------------------------------------
def window_max(img, r=5):
    """max over the (2 r + 1)^2 window clipped at the image edge"""
    h, w = img.shape
    pad = np.full((h + 2 * r, w + 2 * r), -np.inf, dtype=np.float32)
    pad[r:r + h, r:r + w] = img
    out = np.full((h, w), -np.inf, dtype=np.float32)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            np.maximum(out, pad[dy:dy + h, dx:dx + w], out=out)
    return out


def detect_peaks(img, threshold, margin):
    """(y, x) of the pixels the raster walk measures: >= threshold, not visited, no strictly greater pixel in the 11 x 11 window"""
    h, w = img.shape
    is_max = (img.astype(np.float64) >= threshold) & (img == window_max(img, 5))
    visited = np.zeros((h, w), dtype=bool)
    peaks = []
    ys, xs = np.nonzero(is_max[margin:h - margin, margin:w - margin])
    for y, x in zip(ys + margin, xs + margin):   # (np.nonzero: raster order)
        if visited[y, x]:
            continue
        visited[max(y - 5, 0):y + 6, max(x - 5, 0):x + 6] = True
        peaks.append((int(y), int(x)))
    return peaks


def measure_star(img, x, y):
    """(:247-274) -> (Star, passes the fwhm / snr gate)"""
    h, w = img.shape
    cx, cy = float(w) / 2.0, float(h) / 2.0
    sub_x, sub_y = centroid_subpixel(img, x, y, 3)
    sub_peak = subpixel_peak(img, x, y)
    fwhm_major, fwhm_minor = measure_fwhm(img, sub_x, sub_y)
    fwhm = (fwhm_major + fwhm_minor) / 2.0
    big, small = max(fwhm_major, fwhm_minor), min(fwhm_minor, fwhm_major)
    ellipticity = 1.0 - small / big if big > 1e-10 else 0.0
    flux = aperture_flux(img, sub_x, sub_y, fwhm * 1.5)
    bg_flux = annulus_background(img, sub_x, sub_y, fwhm * 2.0, fwhm * 3.0)
    snr = flux / math.sqrt(bg_flux) if bg_flux > 0.0 else flux
    dist = math.sqrt((sub_x - cx) * (sub_x - cx) + (sub_y - cy) * (sub_y - cy))
    return Star(sub_x, sub_y, sub_peak, flux, fwhm, ellipticity, dist, snr), (fwhm > 1.5 and fwhm < 20.0 and snr > 10.0)


# ---- selection (:68-92, :509-516) ----------------------------------------------------------------------------------------------------------
def score_star(s):
    roundness_score = 1.0 - s.ellipticity
    snr_score = min(s.snr / 100.0, 1.0)
    center_score = 1.0 / (1.0 + s.distance_from_center / 500.0)
    fwhm_consistency = 1.0 / (1.0 + abs(s.fwhm - 4.0) / 4.0)
    return roundness_score * 0.35 + snr_score * 0.30 + center_score * 0.15 + fwhm_consistency * 0.20


def select_stars(stars, max_val, rows, cols, cfg):
    """-> (indices into `stars` of the selected ones in selection order, number that passed the filter)"""
    cx, cy = float(cols) / 2.0, float(rows) / 2.0
    max_dist = math.sqrt(cx * cx + cy * cy) * cfg["max_center_distance_fraction"]
    margin = float(cfg["edge_margin"])
    keep = []
    for i, s in enumerate(stars):
        norm_peak = s.peak / max_val
        in_bounds = s.x >= margin and s.y >= margin and s.x < float(cols - cfg["edge_margin"]) and s.y < float(rows - cfg["edge_margin"])
        if (in_bounds and norm_peak < cfg["saturation_threshold"] and norm_peak > cfg["min_peak_fraction"]
                and s.ellipticity < cfg["max_ellipticity"] and s.distance_from_center < max_dist):
            keep.append(i)
    keep.sort(key=lambda i: -score_star(stars[i]))   # (list.sort is stable; -score ascending = score descending, ties in input order)
    return keep[:cfg["num_stars"]], len(keep)


# ---- cutouts (:518-643) ------------------------------------------------------------------------------------------------------------------------
def extract_cutout(img, x, y, radius):
    h, w = img.shape
    size = radius * 2 + 1
    ix, iy = as_i64(rust_round(x)), as_i64(rust_round(y))
    xs, ys = ix - radius, iy - radius
    if xs < 0 or ys < 0 or xs + size > w or ys + size > h:
        return None
    return img[ys:ys + size, xs:xs + size].astype(np.float64)


def bilinear_shift(image, dx, dy):
    h, w = image.shape
    result = np.zeros((h, w), dtype=np.float64)

    def sample(yy, xx):
        return float(image[yy, xx]) if 0 <= yy < h and 0 <= xx < w else 0.0
    for y in range(h):
        for x in range(w):
            sx = float(x) - dx
            sy = float(y) - dy
            x0 = as_i64(math.floor(sx))
            y0 = as_i64(math.floor(sy))
            fx = sx - float(x0)
            fy = sy - float(y0)
            result[y, x] = (sample(y0, x0) * (1.0 - fx) * (1.0 - fy) + sample(y0, x0 + 1) * fx * (1.0 - fy)
                            + sample(y0 + 1, x0) * (1.0 - fx) * fy + sample(y0 + 1, x0 + 1) * fx * fy)
    return result


def subpixel_center(cutout):
    h, w = cutout.shape
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)[:, None]
    sum_x, sum_y, sum_w = seq_sum(xs * cutout), seq_sum(ys * cutout), seq_sum(cutout)
    if sum_w <= 0.0:
        return cutout.copy()
    cx, cy = sum_x / sum_w, sum_y / sum_w
    return bilinear_shift(cutout, (float(w) - 1.0) / 2.0 - cx, (float(h) - 1.0) / 2.0 - cy)


def normalize_cutout(cutout):
    s = seq_sum(cutout)
    return cutout / s if s > 0.0 else cutout.copy()


def compute_spread_radius(psf):
    h, w = psf.shape
    cx, cy = (float(w) - 1.0) / 2.0, (float(h) - 1.0) / 2.0
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)[:, None]
    r2 = (xs - cx) * (xs - cx) + (ys - cy) * (ys - cy)
    sum_r2_w, sum_w = seq_sum(r2 * psf), seq_sum(psf)
    return math.sqrt(sum_r2_w / sum_w) if sum_w > 0.0 else 0.0


# ---- estimate_psf (:52-134) + psf_to_kernel (:136-149) ----------------------------------------------------------------------------------------
def estimate_psf(img, threshold=None, **config) -> Result:
    """threshold=None: the reference's own median + 5 * stddev (sequential sums)"""
    cfg = dict(DEFAULTS, **config)
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape
    st = image_stats(img)
    if threshold is None:
        threshold = st["median"] + 5.0 * st["stddev"]
    res = Result(threshold=threshold, max_val=st["max_val"], kernel_size=2 * cfg["cutout_radius"] + 1)
    res.peaks = detect_peaks(img, threshold, cfg["edge_margin"])
    stars = []
    for (y, x) in res.peaks:
        s, ok = measure_star(img, x, y)
        if ok:
            stars.append(s)
    res.stars_detected = len(stars)
    if not stars:
        res.error = ERR_NO_STARS
        return res
    order, res.stars_filtered = select_stars(stars, st["max_val"], h, w, cfg)
    if not res.stars_filtered:
        res.error = ERR_NO_PASS
        return res
    selected = [stars[i] for i in order]
    size = res.kernel_size
    psf_sum = np.zeros((size, size), dtype=np.float64)
    count = 0
    for s in selected:
        cut = extract_cutout(img, s.x, s.y, cfg["cutout_radius"])
        if cut is not None:
            psf_sum = psf_sum + normalize_cutout(subpixel_center(cut))
            count += 1
    res.cutouts_used = count
    if count == 0:
        res.error = ERR_NO_CUTOUT
        return res
    psf_sum = psf_sum / float(count)
    final_psf = normalize_cutout(psf_sum)
    res.average_fwhm = seq_sum([s.fwhm for s in selected]) / float(len(selected))
    res.average_ellipticity = seq_sum([s.ellipticity for s in selected]) / float(len(selected))
    res.spread_pixels = compute_spread_radius(final_psf)
    res.kernel = final_psf.astype(np.float32)
    res.stars_used = selected
    res.stars_rejected = max(res.stars_filtered - count, 0)
    return res


# ---- fields ---------------------------------------------------------------------------------------------------------------------------------------
def gaussian_star(shape, y0, x0, amp, fwhm):
    sigma = fwhm / 2.3548200450309493
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return amp * np.exp(-((yy - y0) ** 2 + (xx - x0) ** 2) / (2.0 * sigma * sigma))


def make_field(rows, cols, positions, amps, fwhms, seed, sky=200.0, noise=True):
    """sky + Gaussian stars, Poisson counts, kept as integer-valued f32"""
    rng = np.random.default_rng(seed)
    model = np.full((rows, cols), sky, dtype=np.float64)
    for (y0, x0), a, f in zip(positions, amps, fwhms):
        model += gaussian_star((rows, cols), y0, x0, a, f)
    img = rng.poisson(model).astype(np.float64) if noise else np.rint(model)
    return img.astype(np.float32)


def field_a(seed=7):
    """192 x 256, 40 stars on a jittered 8 x 5 grid, FWHM 3-5 px, integer counts: one bright star sets max_val, the others sit
    between 10 % and 95 % of it"""
    rng = np.random.default_rng(seed)
    pos, amps, fw = [], [], []
    for j in range(5):
        for i in range(8):
            pos.append((40.0 + 26.0 * j + rng.uniform(-3, 3), 36.0 + 26.0 * i + rng.uniform(-3, 3)))
            amps.append(float(rng.uniform(6000.0, 30000.0)))
            fw.append(float(rng.uniform(3.0, 5.0)))
    amps[17] = 40000.0
    return make_field(192, 256, pos, amps, fw, seed + 1)


def plant_flat_core(img, y, x, value, half=1):
    img[y - half:y + half + 1, x - half:x + half + 1] = np.float32(value)


def ring_source(shape, y0, x0, amp, ring_radius, ring_sigma=1.5):
    """a defocused star: a ring of radius ring_radius under a narrow central spike (the local maximum) -- the second moments of the
    25 x 25 window then measure a FWHM of about 1.67 * ring_radius, which no Gaussian star inside that window reaches"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    r = np.sqrt((yy - y0) ** 2 + (xx - x0) ** 2)
    return amp * np.exp(-((r - ring_radius) ** 2) / (2.0 * ring_sigma ** 2)) + 1.25 * amp * np.exp(-(r ** 2) / (2.0 * 1.2 ** 2))


def _stamp(img, y, x, amp, fwhm, half=14):
    """an integer-rounded Gaussian stamp centred ON pixel (y, x): exactly symmetric, so two stamps of one kind have equal peaks"""
    yy, xx = np.mgrid[-half:half + 1, -half:half + 1].astype(np.float64)
    sigma = fwhm / 2.3548200450309493
    st = np.rint(amp * np.exp(-(yy * yy + xx * xx) / (2.0 * sigma * sigma))).astype(np.float32)
    img[y - half:y + half + 1, x - half:x + half + 1] += st


def field_c(seed=11):
    """Ties, 128 x 160 (edge_margin 20): integer Poisson sky, ordinary stars, and
       core   a 3 x 3 flat-topped core at (40..42, 50..52): nine equal candidates, the raster-first (40, 50) is measured
       pair   equal peaks at (70, 40) and (70, 43); and at (92, 123) and (90, 126), where the RIGHT one comes first in raster order
       chain  equal peaks at (100, 50), (100, 54), (100, 58): the middle one is suppressed, the third survives (8 > 5 from the first)
    -> (image, dict of the planted pixels)"""
    rng = np.random.default_rng(seed)
    img = rng.poisson(np.full((128, 160), 200.0)).astype(np.float32)
    for (y, x, a, f) in ((30, 100, 9000, 3.6), (60, 90, 30000, 4.0), (64, 120, 7000, 4.4), (84, 70, 12000, 3.2), (45, 130, 8000, 3.8)):
        _stamp(img, y, x, a, f)
    _stamp(img, 41, 51, 6000, 4.5)
    plant_flat_core(img, 41, 51, 8000.0)
    for (y, x) in ((70, 40), (70, 43), (92, 123), (90, 126), (100, 50), (100, 54), (100, 58)):
        _stamp(img, y, x, 5000, 4.0)
    for (y, x) in ((70, 40), (70, 43)):
        img[y, x] = 12000.0
    for (y, x) in ((92, 123), (90, 126)):
        img[y, x] = 12500.0
    for (y, x) in ((100, 50), (100, 54), (100, 58)):
        img[y, x] = 13000.0
    planted = dict(core_first=(40, 50), core_rest=[(40, 51), (40, 52), (41, 50), (41, 51), (41, 52), (42, 50), (42, 51), (42, 52)],
                   kept=[(70, 40), (90, 126), (100, 50), (100, 58)], suppressed=[(70, 43), (92, 123), (100, 54)])
    return img, planted


def field_d(variant, seed=5):
    """Odd shape 131 x 197, cutout_radius 7.  variant 1: edge_margin 20 -- peaks on the first and the last row and column inside the
    margin, and a defocused star (ring_source) whose background annulus leaves the image.  variant 2: edge_margin 5 < cutout_radius -- the same with a
    margin of 5, where the 25 x 25 window is clipped by the border too and extract_cutout refuses the stars nearest to it.
    -> (image, config)"""
    m = 20 if variant == 1 else 5
    rows, cols = 131, 197
    rng = np.random.default_rng(seed + variant)
    img = rng.poisson(np.full((rows, cols), 200.0)).astype(np.float32)
    big = np.zeros((rows + 80, cols + 80), dtype=np.float32)   # (stamps near the border are cut by the image edge)
    stars = [(m, 60, 9000, 3.5), (rows - 1 - m, 90, 10000, 4.0), (70, m, 8000, 3.8), (60, cols - 1 - m, 9500, 4.2),
             (66, 100, 30000, 4.0), (50, 70, 12000, 3.4), (85, 130, 11000, 4.6), (40, 150, 7000, 3.0)]
    for (y, x, a, f) in stars:
        _stamp(big, y + 40, x + 40, a, f, half=30)
    img += big[40:40 + rows, 40:40 + cols]
    img += np.rint(ring_source((rows, cols), m + 2, 120, 12000.0, 6.0)).astype(np.float32)   # FWHM ~ 10: an annulus out to ~30 px
    for (y, x, a, f) in stars[:4]:
        img[y, x] += 50.0   # (the peak pixel stays where it was planted whatever the noise)
    return img, dict(edge_margin=m, cutout_radius=7, max_center_distance_fraction=0.95, num_stars=6)


def field_e(seed=3):
    """Large annuli, 256 x 256: defocused stars (ring_source).  Ring radius 10.8 at (215, 215): FWHM ~ 18, kept, its annulus (out to
    ~53 px) clipped by the border; ring radius 16 at (60, 70): FWHM ~ 24, which the `< 20` gate rejects, ~9000 annulus samples clipped
    by the border.  The pixels of the rings are peaks of their own, with every size of annulus in between."""
    rng = np.random.default_rng(seed)
    model = np.full((256, 256), 200.0)
    model += ring_source((256, 256), 215, 215, 20000.0, 10.8)
    model += ring_source((256, 256), 60, 70, 20000.0, 16.0)
    model += gaussian_star((256, 256), 140.3, 120.6, 15000.0, 4.0) + gaussian_star((256, 256), 150.2, 60.4, 9000.0, 3.5)
    return rng.poisson(model).astype(np.float32)


def field_noise(seed=2):
    return np.random.default_rng(seed).poisson(np.full((96, 128), 200.0)).astype(np.float32)


def field_saturated(seed=4):
    """every star has a flat-topped core at the image's maximum: norm_peak = 1 fails the saturation filter"""
    rng = np.random.default_rng(seed)
    img = rng.poisson(np.full((128, 160), 200.0)).astype(np.float32)
    for (y, x) in ((40, 50), (64, 80), (80, 110), (50, 120)):
        _stamp(img, y, x, 40000, 4.0)
        plant_flat_core(img, y, x, 60000.0)
    return img
