"""warp_kernel_shared (csrc/resample.hip) restated in numpy: which transforms ab_warp_rows_device routes to it, and which waves of a
launch take its shared path.  Shared by test_warp_shared_taps_predicate.py (CPU: the shared path forms no address outside the taps
the per-pixel sampler would load) and test_gpu_warp_shared_taps.py (GPU: bit parity with the oracle; every class a case is named
for is populated at its shape).

The kernel: a workgroup is 256 output columns x K output rows, a lane owns one column and the K rows y0 .. y0 + K - 1 with
y0 = row0 + K * group (aligned to the band's first row), a wave is 64 consecutive columns.  A wave shares when every lane's K pixels
are live (column < out_cols, row inside the band), pass the reference's inside test, have their 4 x 4 footprint inside the source,
and see floor(sx) equal and floor(sy) consecutive over the K rows."""
import math

import numpy as np

import resample_cases as rc

WAVE, PIECE = 64, 256
KS = (2, 3, 4)
NAN = float("nan")


def routed(t):
    """ab_warp_rows_device: the shared-tap kernel only for tame transforms with |d - 1| <= 1/64 and |b| <= 1/64"""
    a, b, tx, c, d, ty = (float(v) for v in t)
    tame = all(math.isfinite(v) and abs(v) <= 1e150 for v in (a, b, tx, c, d, ty))
    return tame and abs(d - 1.0) <= 1.0 / 64.0 and abs(b) <= 1.0 / 64.0


def cvt_i32(f):
    """v_cvt_i32_f64 of a floor: saturating, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(f), 0.0, np.clip(f, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def pixel_classes(t, src_rows, src_cols, out_cols, row0, nrows):
    """per pixel of output rows [row0, row0 + nrows): (ix, iy, in, interior) with the kernel's own expressions"""
    a, b, tx, c, d, ty = (float(v) for v in t)
    x = np.arange(out_cols, dtype=np.float64)[None, :]
    y = np.arange(row0, row0 + nrows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        sx = a * x + b * y + tx
        sy = c * x + d * y + ty
        ix, iy = cvt_i32(np.floor(sx)), cvt_i32(np.floor(sy))
    inside = (ix >= 0) & (ix < src_cols - 1) & (iy >= 0) & (iy < src_rows - 1)   # the two unsigned compares
    interior = (ix >= 1) & (ix + 2 < src_cols) & (iy >= 1) & (iy + 2 < src_rows)
    return ix, iy, inside, interior


def share_map(classes, K):
    """classes of a band (pixel_classes) -> (share[groups, waves], any_sampled[groups, waves], ix0[groups, cols], iy0[groups, cols]):
    the kernel's wave-wide predicate for group height K, and the first row's floors of every lane"""
    ix, iy, inside, interior = classes
    nrows, cols = ix.shape
    groups = -(-nrows // K)
    pad_r, pad_c = groups * K - nrows, (-cols) % WAVE

    def grp(m, fill):  # -> [groups, K, padded cols]
        return np.pad(m, ((0, pad_r), (0, pad_c)), constant_values=fill).reshape(groups, K, cols + pad_c)

    live = grp(np.ones((nrows, cols), bool), False)
    g_ix, g_iy, g_in, g_int = grp(ix, 0), grp(iy, 0), grp(inside, False), grp(interior, False)
    k = np.arange(K)[None, :, None]
    ok = live & g_in & g_int & (g_ix == g_ix[:, :1]) & (g_iy == g_iy[:, :1] + k)
    lane_ok = ok.all(axis=1)                                                     # [groups, padded cols]
    share = lane_ok.reshape(groups, -1, WAVE).all(axis=2)
    any_sampled = (live & g_in).any(axis=1).reshape(groups, -1, WAVE).any(axis=2)
    return share, any_sampled, g_ix[:, 0, :cols], g_iy[:, 0, :cols]


def counts(t, src_dims, out_dims, K, row0=0, nrows=None):
    """(waves that share, waves that sample something and do not share) of one launch"""
    nrows = out_dims[0] - row0 if nrows is None else nrows
    share, any_sampled, _, _ = share_map(pixel_classes(t, src_dims[0], src_dims[1], out_dims[1], row0, nrows), K)
    return int(share.sum()), int((~share & any_sampled).sum())


# ---- the GPU test's source and transforms -----------------------------------------------------------------------------------------
SRC_DIMS = (80, 310)


def source():
    """a seeded uniform plane with a NaN patch, a +inf pixel, a -inf pixel and a zero block inside it"""
    img = np.random.default_rng(29).uniform(1.0, 2.0, SRC_DIMS).astype(np.float32)
    img[20:23, 100:130] = np.nan
    img[40, 200] = np.inf
    img[9, 37] = -np.inf
    img[50:60, 20:60] = 0.0
    return img


def rotation(deg, out_dims, tx, ty):
    return rc.about_centre(deg, 1.0, SRC_DIMS, out_dims, tx, ty)


# (id, transform as a function of the output dims, must some wave share, must some sampling wave not share, is it routed)
CASES = [
    ("a: pure sub-pixel shift", lambda o: (1.0, 0.0, 2.25, 0.0, 1.0, -1.5), True, None, True),
    # (sin 1 deg = 0.01745 is above the routing's 1/64 = 0.015625: the 1 deg case runs the per-pixel kernel although its coordinates
    # would let waves share; 0.85 deg (sin = 0.01483) is the same class on the shared-tap kernel)
    ("b: rotation of 1 deg about the centre + fractional shift", lambda o: rotation(1.0, (67, 300), 1.3, 2.6), True, True, False),
    ("b: rotation of 0.85 deg about the centre + fractional shift", lambda o: rotation(0.85, (67, 300), 1.3, 2.6), True, True, True),
    ("c: rotation of 0.05 deg + shift", lambda o: rotation(0.05, (67, 300), -3.7, 4.2), True, None, True),
    ("d: d = 1 - 2^-6: two rows of a group on one source row", lambda o: (1.0, 0.0, 3.25, 0.0, 1.0 - 2.0 ** -6, 0.5), None, True, True),
    ("e: d = 1 + 2^-6: a group skips a source row", lambda o: (1.0, 0.0, 3.25, 0.0, 1.0 + 2.0 ** -6, 0.5), None, True, True),
    ("f: ty = -2.5, tx = -1.5: rows that do not sample beside rows that do, clamped taps", lambda o: (1.0, 0.0, -1.5, 0.0, 1.0, -2.5),
     None, True, True),
    ("g: scale 0.5", lambda o: rc.about_centre(0.0, 0.5, SRC_DIMS, o), False, None, False),
    ("g: scale 2", lambda o: rc.about_centre(0.0, 2.0, SRC_DIMS, o), False, None, False),
    ("g: rotation of 45 deg", lambda o: rc.about_centre(45.0, 1.0, SRC_DIMS, o), False, None, False),
    ("h: a coefficient of 1e200", lambda o: (1.0, 0.0, 2.25, 1e200, 1.0, -1.5), False, None, False),
    ("h: a NaN coefficient", lambda o: (1.0, 0.0, NAN, 0.0, 1.0, -1.5), False, None, False),
]
OUT_COLS = (300, 256)
OUT_ROWS = (1, 2, 3, 4, 5, 7, 13, 67)
POPULATED_AT = (67, 300)   # the shape at which every case must populate the class it is named for
