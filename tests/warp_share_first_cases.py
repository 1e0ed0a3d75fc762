"""warp_kernel_shared's share-first predicate (csrc/resample.hip, LABNOTES 37) restated in numpy, and the inputs of the two tests that
hold it to the former one: test_warp_share_first_predicate.py (CPU: it marks the same waves as warp_shared_cases.share_map, and on
every sharing lane truncation is the floor and the fraction is exact and unclamped) and test_gpu_warp_share_first.py (GPU: bit
parity with the oracle on sources so small that the clamped bounds act, and on coordinates around 0, 1, src - 3 and far outside).

The kernel takes ix, iy as v_cvt_i32_f64 of the coordinate ITSELF (round toward zero, saturating, NaN -> 0) and a lane shares when
    (u32)(ix_0 - 1) < max(src_cols - 3, 0)   and   (u32)(iy_0 - 1) < max(src_rows - K - 2, 0)
    ix_k == ix_0   and   iy_k == iy_0 + k   (32-bit wrap)   for k = 1 .. K - 1,        and its column is below out_cols;
a wave shares when all its 64 lanes do and (scalar) the group's K rows lie inside the band."""
import math

import numpy as np

import warp_shared_cases as wc

U32 = 0xFFFFFFFF


def cvt_i32_trunc(s):
    """v_cvt_i32_f64 of the coordinate itself: toward zero, saturating, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s), 0.0, np.clip(np.trunc(s), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def coordinates(t, out_cols, row0, nrows):
    """(sx, sy) of output rows [row0, row0 + nrows) with the kernel's own expressions, columns padded to whole waves (a lane beyond
    out_cols computes its coordinates like any other)"""
    a, b, tx, c, d, ty = (float(v) for v in t)
    x = np.arange(out_cols + (-out_cols) % wc.WAVE, dtype=np.float64)[None, :]
    y = np.arange(row0, row0 + nrows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        return a * x + b * y + tx, c * x + d * y + ty


def share_first_map(coords, src_rows, src_cols, out_cols, nrows, K):
    """coordinates() of a band -> (share[groups, waves], lanes[groups, padded cols] of the sharing waves)"""
    groups = -(-nrows // K)
    pad_r = groups * K - nrows

    def grp(m):  # (a ragged last group is padded with rows that the scalar row test keeps from sharing)
        return np.pad(m, ((0, pad_r), (0, 0))).reshape(groups, K, -1)

    ix, iy = (grp(cvt_i32_trunc(s)) for s in coords)
    col_bound, row_bound = max(src_cols - 3, 0), max(src_rows - K - 2, 0)
    lane = (np.arange(ix.shape[2]) < out_cols)[None, :] & (((ix[:, 0] - 1) & U32) < col_bound) & (((iy[:, 0] - 1) & U32) < row_bound)
    for k in range(1, K):
        lane = lane & (ix[:, k] == ix[:, 0]) & ((iy[:, k] & U32) == ((iy[:, 0] + k) & U32))
    rows_live = (np.arange(groups) * K + K - 1 < nrows)[:, None]
    share = lane.reshape(groups, -1, wc.WAVE).all(axis=2) & rows_live
    return share, np.repeat(share, wc.WAVE, axis=1)


def fraction_is_exact(s):
    """per pixel: truncation is the floor (as a double and converted), floor(s) >= 1 and s <= 2 floor(s) -- so s - floor(s) is exact --
    and v_fract_f64's clamp min(s - floor(s), nextafter(1, 0)) does not act"""
    with np.errstate(all="ignore"):
        f = np.floor(s)
        return ((np.trunc(s) == f) & (cvt_i32_trunc(s) == f) & (f >= 1.0) & (s <= 2.0 * f) &
                (np.minimum(s - f, np.nextafter(1.0, 0.0)) == s - f))


def check_launch(t, src_dims, out_cols, row0, nrows):
    """one launch, K = 2, 3, 4: the same waves as the former predicate; trunc == floor and an exact, unclamped fraction for every
    pixel of every sharing lane -> {K: sharing waves}"""
    classes = wc.pixel_classes(t, src_dims[0], src_dims[1], out_cols, row0, nrows)
    coords = coordinates(t, out_cols, row0, nrows)
    pixel_ok = fraction_is_exact(coords[0]) & fraction_is_exact(coords[1])
    shared = {}
    for K in wc.KS:
        want = wc.share_map(classes, K)[0]
        share, lanes = share_first_map(coords, src_dims[0], src_dims[1], out_cols, nrows, K)
        assert np.array_equal(share, want), (t, src_dims, out_cols, row0, nrows, K, np.argwhere(share != want)[:4])
        shared[K] = int(share.sum())
        groups = lanes.shape[0]
        lane_ok = np.pad(pixel_ok, ((0, groups * K - nrows), (0, 0))).reshape(groups, K, -1).all(axis=1)
        assert (lane_ok | ~lanes).all(), (t, src_dims, out_cols, row0, nrows, K, np.argwhere(lanes & ~lane_ok)[:4])
    return shared


def bands_of(rows):
    """row0 in {0, 1, 2, rows - 1}, heights 1 .. 5 (1 .. K + 1 for every K the kernel is built for)"""
    return [(row0, n) for row0 in sorted({0, 1, 2, rows - 1}) for n in range(1, 6) if 0 <= row0 < rows and row0 + n <= rows]


# ---- the CPU test's random routed transforms --------------------------------------------------------------------------------------
SOURCES = ((5, 3), (5, 4), (6, 5), (4, 70), (7, 70), (8, 130), wc.SRC_DIMS)   # (rows, cols)
OFFSETS = (-2.5, -1.5, -0.75, -0.5, -1e-9, -1e-12, 0.0, 0.25, 0.5, 1.0, 1.25, 2.75, 1e9, -1e9, 2e9, 3e9, -3e9, 1e150)
PER_SOURCE = 60   # 7 x 60 = 420 transforms


def random_routed(seed=37):
    """(source dims, transform, output dims) x 420: every third one a pure shift, the others within the routing's |b|, |d - 1| <= 1/64"""
    rng = np.random.default_rng(seed)
    out = []
    for src in SOURCES:
        for i in range(PER_SOURCE):
            tx, ty = (float(v) for v in rng.choice(OFFSETS, 2))
            if i % 3 == 0:
                t = (1.0, 0.0, tx, 0.0, 1.0, ty)
            else:
                a, d = (1.0 + float(v) for v in rng.uniform(-1.0 / 64, 1.0 / 64, 2))
                b, c = (float(v) for v in rng.uniform(-1.0 / 64, 1.0 / 64, 2))
                t = (a, b, tx, c, d, ty)
            assert wc.routed(t), t
            dims = (int(rng.choice((1, 2, 3, 4, 5, 7, 13, 67))), int(rng.choice((64, 67, 130, 256, 300))))
            out.append((src, t, dims))
    return out


# ---- the GPU test's cases ---------------------------------------------------------------------------------------------------------
GPU_SOURCES = SOURCES[:-1]
GPU_OUT_DIMS = ((11, 300), (67, 67))


def gpu_source(dims):
    img = np.random.default_rng(41 + dims[0] * 1000 + dims[1]).uniform(1.0, 2.0, dims).astype(np.float32)
    if dims[1] >= 70:
        img[2, 30] = np.nan
        img[1, 50] = np.inf
    return img


def gpu_offsets(dims):
    """(tx, ty): first coordinates in (-1, 0); integer offsets (coordinates exactly on 0, on 1 and on src - 3 -- the last pixel whose
    footprint is interior -- further along the row and the column); fractions of 1 - 1e-12; the first pixel on src - 3; and far outside"""
    rows, cols = dims
    return ((-0.5, -0.75), (-1e-12, -1e-9), (0.0, 0.0), (1.0, 1.0), (1.25, 1.0), (1.0, 0.25), (2.75, 1.5), (float(cols - 3), float(rows - 3)),
            (1e9, 0.25), (0.25, 3e9), (-3e9, 1.0), (1e150, 1.0), (1.0, 1e150))


def gpu_transforms(dims):
    """each offset without and with a rotation of 0.05 deg (about the output's origin)"""
    co, si = math.cos(math.radians(0.05)), math.sin(math.radians(0.05))
    out = []
    for tx, ty in gpu_offsets(dims):
        out.append((1.0, 0.0, tx, 0.0, 1.0, ty))
        out.append((co, -si, tx, si, co, ty))
    return out
