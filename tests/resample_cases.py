"""The sampler's edge cases, shared by test_resample_restatement.py (oracle against the numpy restatement, CPU) and
test_gpu_resample_shapes.py (library against the oracle, GPU).  Every case names the class of the sampler it is there for and
carries a predicate over resample_restatement.sampler_classes -- computed from the RESTATEMENT's coordinates -- that must hold,
so that a case cannot silently test nothing."""
import math

import numpy as np

import resample_restatement as rs

NAN, INF = float("nan"), float("inf")


def pattern(rows, cols, seed=3, nan_patch=True):
    """align.rs:160-166's test pattern + unit noise + a NaN patch (NaNs go through the taps like any value)"""
    y = np.arange(rows, dtype=np.float32)[:, None]
    x = np.arange(cols, dtype=np.float32)[None, :]
    t3 = ((np.arange(rows)[:, None] * 7 + np.arange(cols)[None, :] * 13).astype(np.float32) * np.float32(0.01))
    img = (np.sin(y * np.float32(0.3)) * np.cos(x * np.float32(0.2)) * np.float32(1000.0) + np.float32(500.0)
           + np.sin(t3) * np.float32(200.0)).astype(np.float32)
    img = img + np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32)
    if nan_patch and rows > 12 and cols > 40:
        img[10:12, 20:40] = np.nan
    return img


def about_centre(deg, scale, src, out, tx=0.0, ty=0.0):
    """output (x, y) -> source: rotation by deg and `scale` taking the output's centre to the source's centre (+ tx, ty)"""
    c, s = math.cos(math.radians(deg)) * scale, math.sin(math.radians(deg)) * scale
    ocx, ocy = (out[1] - 1) / 2.0, (out[0] - 1) / 2.0
    scx, scy = (src[1] - 1) / 2.0, (src[0] - 1) / 2.0
    return (c, -s, scx - c * ocx + s * ocy + tx, s, c, scy - s * ocx - c * ocy + ty)


ROWS, COLS = 97, 141   # the edge cases' source

# (id, source dims, transform, output dims, predicate over (classes, sx, sy, sampled))
WARP_CASES = [
    ("identity", (ROWS, COLS), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (ROWS, COLS),
     lambda k, sx, sy, s: k["frac_zero_x"] == k["sampled"] > 0 and k["outside"] == ROWS + COLS - 1),
    ("integer translation: fraction exactly 0", (ROWS, COLS), (1.0, 0.0, 3.0, 0.0, 1.0, -2.0), (ROWS, COLS),
     lambda k, sx, sy, s: k["frac_zero_x"] == k["frac_zero_y"] == k["sampled"] > 0 and k["outside"] > 0),
    ("fraction 2^-52", (ROWS, COLS), (1.0, 0.0, 2.0 ** -52, 0.0, 1.0, 2.0 ** -52), (ROWS, COLS),
     lambda k, sx, sy, s: bool((s & (sx - np.floor(sx) == 2.0 ** -52)).any() and (s & (sy - np.floor(sy) == 2.0 ** -52)).any())),
    ("fraction 1 - 2^-53", (ROWS, COLS), (1.0, 0.0, 1.0 - 2.0 ** -53, 0.0, 1.0, 1.0 - 2.0 ** -53), (ROWS, COLS),
     lambda k, sx, sy, s: bool((s & (sx - np.floor(sx) == 1.0 - 2.0 ** -53)).any() and (s & (sy - np.floor(sy) == 1.0 - 2.0 ** -53)).any())),
    ("10 deg, scale 0.9 about the centre, output larger: all four borders inside one plane", (ROWS, COLS),
     about_centre(10.0, 0.9, (ROWS, COLS), (160, 230)), (160, 230),
     lambda k, sx, sy, s: min(k["outside"], k["ix_first"], k["ix_last"], k["iy_first"], k["iy_last"], k["waves_unclamped"],
                              k["waves_clamped_mixed"], k["waves_partly_outside"]) > 0),
    ("-2 deg, scale 1.03, output smaller", (ROWS, COLS), about_centre(-2.0, 1.03, (ROWS, COLS), (80, 100), 3.3, -1.1), (80, 100),
     lambda k, sx, sy, s: k["sampled"] > 0 and k["waves_unclamped"] > 0),
    ("0.4 deg and a translation", (ROWS, COLS), about_centre(0.4, 1.0, (ROWS, COLS), (ROWS, COLS), -6.2, 4.7), (100, 170),
     lambda k, sx, sy, s: k["sampled"] > 0 and k["outside"] > 0 and k["edge"] > 0),
    ("sx exactly cols - 1 (outside) next to cols - 2 (the last footprint)", (ROWS, COLS), (1.0, 0.0, 0.0, 0.0, 1.0, 0.5), (ROWS, COLS + 9),
     lambda k, sx, sy, s: bool((~s & (sx == COLS - 1)).any()) and k["ix_last"] > 0),
    ("sx exactly 0.0", (ROWS, COLS), (0.0, 0.0, 0.0, 0.0, 1.0, 0.25), (ROWS, COLS),
     lambda k, sx, sy, s: bool((s & (sx == 0.0) & ~np.signbit(sx)).any())),
    ("sx exactly -0.0: negative zero coefficients", (ROWS, COLS), (-0.0, -0.0, -0.0, 0.0, 1.0, 0.0), (96, 130),
     lambda k, sx, sy, s: bool((s & (sx == 0.0) & np.signbit(sx)).any())),
    ("sx just below cols - 1", (ROWS, COLS), (0.0, 0.0, math.nextafter(COLS - 1.0, 0.0), 0.0, 1.0, 0.75), (ROWS, 70),
     lambda k, sx, sy, s: k["ix_last"] > 0 and k["ix_last"] == k["sampled"]),
    ("sy just below rows - 1", (ROWS, COLS), (1.0, 0.0, 0.5, 0.0, 0.0, math.nextafter(ROWS - 1.0, 0.0)), (9, COLS),
     lambda k, sx, sy, s: k["iy_last"] > 0 and k["iy_last"] == k["sampled"]),
    ("sx in (-1, 0): floor -1 is outside", (ROWS, COLS), (1.0, 0.0, -0.5, 0.0, 1.0, -0.25), (ROWS, COLS),
     lambda k, sx, sy, s: bool((~s & (sx > -1.0) & (sx < 0.0)).any() and (~s & (sy > -1.0) & (sy < 0.0)).any()) and k["sampled"] > 0),
    ("coefficients 1e10: coordinates beyond 2^31", (ROWS, COLS), (1e10, 0.0, 0.5, 0.0, 1.0, 0.25), (ROWS, COLS),
     lambda k, sx, sy, s: bool((~s & (sx > 2.0 ** 31)).any()) and k["sampled"] == ROWS - 1),
    ("coefficients -1e10: coordinates below -2^31", (ROWS, COLS), (-1e10, 0.0, 3.5, -1e10, 1.0, 2.25), (ROWS, COLS),
     lambda k, sx, sy, s: bool((~s & (sx < -2.0 ** 31)).any() and (~s & (sy < -2.0 ** 31)).any()) and k["sampled"] > 0),
    ("a stride of 2^32: a wrapping 32-bit convert would land inside", (ROWS, COLS), (2.0 ** 32, 0.0, 5.5, 2.0 ** 32, 1.0, 7.25), (ROWS, COLS),
     lambda k, sx, sy, s: bool((~s & (np.mod(sx, 2.0 ** 32) == 5.5) & (sx > 2.0 ** 31)).any()) and k["sampled"] > 0),
    ("far translation: nothing inside", (ROWS, COLS), (1.0, 0.0, 1000.0, 0.0, 1.0, 1000.0), (ROWS, COLS),
     lambda k, sx, sy, s: k["sampled"] == 0),
    ("nan tx", (ROWS, COLS), (1.0, 0.0, NAN, 0.0, 1.0, 2.0), (96, 130), lambda k, sx, sy, s: k["sampled"] == 0 and bool(np.isnan(sx).all())),
    ("inf a", (ROWS, COLS), (INF, 0.0, 1.0, 0.0, 1.0, 2.0), (96, 130),
     lambda k, sx, sy, s: bool(np.isnan(sx[:, 0]).all() and np.isinf(sx[:, 1:]).all()) and k["sampled"] == 0),   # inf * 0 at x = 0
    ("1e200 a and b cancel to nan", (ROWS, COLS), (1e200, -1e200, 3.0, 0.0, 1.0, 0.5), (96, 130),
     lambda k, sx, sy, s: bool((~s & ~np.isfinite(sx)).any() or (~s & (np.abs(sx) > 1e150)).any())),
    ("ty beyond 1e150", (ROWS, COLS), (1.0, 0.0, 0.25, 1e-300, 1.0, 1e160), (96, 130), lambda k, sx, sy, s: k["sampled"] == 0),
    ("source of one row", (1, COLS), (1.0, 0.0, 0.25, 0.0, 1.0, 0.0), (5, COLS), lambda k, sx, sy, s: k["sampled"] == 0),
    ("source of one column", (ROWS, 1), (1.0, 0.0, 0.0, 0.0, 1.0, 0.25), (ROWS, 5), lambda k, sx, sy, s: k["sampled"] == 0),
    ("source of 2 x 2, output larger", (2, 2), (0.01, 0.0, 0.0, 0.0, 0.02, 0.0), (40, 90),
     lambda k, sx, sy, s: k["sampled"] == 40 * 90 and k["edge"] == k["sampled"] and k["ix_first"] == k["ix_last"] == k["sampled"]),
    ("source of 3 x 200, every tap row clamped", (3, 200), about_centre(1.0, 1.0, (3, 200), (6, 260)), (6, 260),
     lambda k, sx, sy, s: k["sampled"] > 0 and k["interior"] == 0),
]

# (id, source dims, (dy, dx), predicate over (classes of the rows x columns that sample, sy, sx, ok_y, ok_x))
SHIFT_CASES = [
    ("zero: the copy branch", (97, 133), (0.0, 0.0), None),
    ("|d| < 1e-12: the copy branch", (97, 133), (1e-13, -9.9e-13), None),
    ("|d| = 1e-12: sampled with a fraction of 1e-12", (97, 133), (1e-12, 0.0), lambda k, sy, sx, oy, ox: k["frac_zero_x"] == k["sampled"] > 0 and k["frac_zero_y"] < k["sampled"]),
    ("integer shift", (97, 133), (2.0, 3.0), lambda k, sy, sx, oy, ox: k["frac_zero_x"] == k["frac_zero_y"] == k["sampled"] > 0 and k["outside"] > 0),
    ("quarter pixel", (97, 133), (0.25, -0.75), lambda k, sy, sx, oy, ox: k["edge"] > 0 and k["waves_clamped_mixed"] > 0 and k["waves_unclamped"] > 0),
    ("general", (97, 133), (-7.3, 5.9), lambda k, sy, sx, oy, ox: k["outside"] > 0 and k["waves_partly_outside"] > 0),
    ("+0.5 exactly: sy = rows - 0.5 is still sampled", (97, 133), (0.5, 0.5),
     lambda k, sy, sx, oy, ox: bool(oy[-1] and sy[-1] == 96.5 and ox[-1] and sx[-1] == 132.5) and k["iy_beyond"] > 0 and k["ix_beyond"] > 0),
    ("-0.5 exactly: sy = -0.5 is still sampled", (97, 133), (-0.5, -0.5),
     lambda k, sy, sx, oy, ox: bool(oy[0] and sy[0] == -0.5 and ox[0] and sx[0] == -0.5) and k["iy_negative"] > 0 and k["ix_negative"] > 0),
    ("just past +0.5", (97, 133), (math.nextafter(0.5, 1.0), math.nextafter(-0.5, -1.0)),
     lambda k, sy, sx, oy, ox: bool(not oy[-1] or sy[-1] == 96.5) and bool(not ox[0])),
    ("far: most of the frame empty", (97, 133), (63.6, -70.2), lambda k, sy, sx, oy, ox: k["outside"] > k["sampled"] > 0),
    ("larger than the frame in y", (97, 133), (200.0, 0.3), lambda k, sy, sx, oy, ox: k["sampled"] == 0),
    ("larger than the frame in x", (97, 133), (0.25, -500.0), lambda k, sy, sx, oy, ox: k["sampled"] == 0),
    ("infinite shift", (97, 133), (INF, 0.0), lambda k, sy, sx, oy, ox: k["sampled"] == 0),
    ("nan dy: not the copy branch, not skipped; catmull_rom(nan) = 0.0 on every tap row", (97, 133), (NAN, 0.25),
     lambda k, sy, sx, oy, ox: bool(np.isnan(sy).all() and oy.all()) and k["sampled"] > 0 and k["iy_first"] == k["sampled"]),
    ("nan dx", (97, 133), (-1.5, NAN), lambda k, sy, sx, oy, ox: bool(np.isnan(sx).all() and ox.all()) and k["ix_first"] == k["sampled"] > 0),
    ("one row", (1, 300), (0.25, 1.5), lambda k, sy, sx, oy, ox: k["sampled"] > 0 and k["interior"] == 0),
    ("one column", (300, 1), (1.5, 0.25), lambda k, sy, sx, oy, ox: k["sampled"] > 0 and k["interior"] == 0),
    ("2 x 2", (2, 2), (0.3, -0.4), lambda k, sy, sx, oy, ox: k["sampled"] == 4 and k["interior"] == 0),
]

# (id, source dims, target dims, predicate over (classes, sy, sx))
RESAMPLE_CASES = [
    ("equal dims: copy", (100, 100), (100, 100), None),
    ("half", (200, 200), (100, 100), lambda k, sy, sx: k["sampled"] == 100 * 100 and k["frac_zero_x"] == 0),
    ("double", (50, 50), (100, 100), lambda k, sy, sx: k["ix_negative"] > 0 and k["iy_negative"] > 0),
    ("x 8 up", (33, 41), (264, 328), lambda k, sy, sx: k["ix_negative"] > 0 and k["ix_beyond"] > 0 and k["waves_unclamped"] > 0),
    ("/ 8 down", (264, 328), (33, 41), lambda k, sy, sx: k["interior"] == k["sampled"] and bool(sx[0] == 3.5)),
    ("prime dims", (37, 53), (83, 31), lambda k, sy, sx: k["edge"] > 0 and k["interior"] > 0),
    ("prime dims, larger", (301, 517), (1021, 769), lambda k, sy, sx: k["waves_clamped_mixed"] > 0 and k["waves_unclamped"] > 0),
    ("one source row", (1, 97), (5, 300), lambda k, sy, sx: k["interior"] == 0),
    ("one source column", (97, 1), (300, 5), lambda k, sy, sx: k["interior"] == 0),
    ("2 x 2 up", (2, 2), (64, 200), lambda k, sy, sx: k["interior"] == 0 and k["sampled"] == 64 * 200),
    ("to one pixel", (40, 60), (1, 1), lambda k, sy, sx: bool(sy[0] == 19.5 and sx[0] == 29.5)),
]


def warp_populates(case):
    _, src, t, out, pred = case
    sx, sy, inside = rs.warp_coords(t, src[0], src[1], out[1], 0, out[0])
    sx, sy = np.broadcast_to(sx, inside.shape), np.broadcast_to(sy, inside.shape)
    k = rs.sampler_classes(sx, sy, inside, src[0], src[1])
    return bool(pred(k, sx, sy, inside)), k


def shift_populates(case):
    _, src, (dy, dx), pred = case
    if pred is None:
        return abs(dy) < 1e-12 and abs(dx) < 1e-12, {}
    sy, sx, ok_y, ok_x = rs.shift_coords(src[0], src[1], dy, dx)
    k = rs.sampler_classes(sx[None, :], sy[:, None], ok_y[:, None] & ok_x[None, :], src[0], src[1])
    return bool(pred(k, sy, sx, ok_y, ok_x)), k


def resample_populates(case):
    _, src, dst, pred = case
    if pred is None:
        return src == dst, {}
    sy, sx = rs.resample_coords(src[0], src[1], dst[0], dst[1])
    k = rs.sampler_classes(sx[None, :], sy[:, None], np.ones(dst, bool), src[0], src[1])
    return bool(pred(k, sy, sx)), k
