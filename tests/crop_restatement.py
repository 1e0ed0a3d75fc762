"""numpy restatement of the compose wizard's crop step (cmd/compose/crop.rs), written independently of the kernels.

detect_valid_region_loops restates the four labelled loops of detect_valid_region (:14-62) literally, early exits included;
detect_valid_region is the vectorised form the GPU tests use on larger planes, cross-checked against the loops by
tests/test_crop_cpu.py.  crop_array (:64-71), the auto intersection (:103-122), the manual margins with saturating subtraction
(:123-126) and the reported dimensions and margins (:170-183) follow; the statistics come from the oracle's compute_image_stats.
Nothing here rounds: tests/test_gpu_crop.py holds the device to it with array_equal.
"""
from dataclasses import dataclass

import numpy as np

F32 = np.float32
AUTO_THRESHOLD = F32(1e-6)          # :12
USIZE_MAX = (1 << 64) - 1
NO_PATHS = "No paths provided for cropping"                  # :93
NO_OVERLAP = "Auto-crop found no valid overlapping region"   # :119


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def valid(arr, threshold):
    """arr[[r, c]].abs() > threshold (:20): strict, in f32; false for a NaN on either side"""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(arr, F32)) > F32(threshold)


def detect_valid_region_loops(arr, threshold):
    """the four loops, as written"""
    arr = np.asarray(arr, F32)
    thr = F32(threshold)
    rows, cols = arr.shape

    def hit(r, c):
        return bool(np.abs(arr[r, c]) > thr)

    top = 0
    done = False
    for r in range(rows):                # 'outer_top
        for c in range(cols):
            if hit(r, c):
                top = r
                done = True
                break
        if done:
            break
        top = r + 1

    bottom = rows
    done = False
    for r in reversed(range(rows)):      # 'outer_bot
        for c in range(cols):
            if hit(r, c):
                bottom = r + 1
                done = True
                break
        if done:
            break
        bottom = r

    left = 0
    done = False
    for c in range(cols):                # 'outer_left
        for r in range(rows):
            if hit(r, c):
                left = c
                done = True
                break
        if done:
            break
        left = c + 1

    right = cols
    done = False
    for c in reversed(range(cols)):      # 'outer_right
        for r in range(rows):
            if hit(r, c):
                right = c + 1
                done = True
                break
        if done:
            break
        right = c

    return top, bottom, left, right


def detect_valid_region(arr, threshold=AUTO_THRESHOLD):
    """the same result from the validity mask: first / last + 1 valid row and column, (rows, 0, cols, 0) without one"""
    m = valid(arr, threshold)
    rows, cols = m.shape
    r = np.flatnonzero(m.any(axis=1))
    c = np.flatnonzero(m.any(axis=0))
    if r.size == 0:
        return rows, 0, cols, 0
    return int(r[0]), int(r[-1]) + 1, int(c[0]), int(c[-1]) + 1


def clamp_box(shape, top, bottom, left, right):
    """(t, b, l, r) of crop_array (:65-69)"""
    rows, cols = shape
    t = min(top, rows)
    b = max(min(bottom, rows), t)
    l = min(left, cols)
    r = max(min(right, cols), l)
    return t, b, l, r


def crop_array(arr, top, bottom, left, right):
    t, b, l, r = clamp_box(arr.shape, top, bottom, left, right)
    return np.ascontiguousarray(np.asarray(arr, F32)[t:b, l:r])


def common_box(boxes):
    """the running (max top, min bottom, max left, min right) of :104-116"""
    t, b, l, r = 0, USIZE_MAX, 0, USIZE_MAX
    for bt, bb, bl, br in boxes:
        t, b, l, r = max(t, bt), min(b, bb), max(l, bl), min(r, br)
    return t, b, l, r


def sat_sub(a, b):
    return a - b if a > b else 0


@dataclass
class Plan:
    crop_box: tuple
    out_rows: int
    out_cols: int
    actual_top: int
    actual_bottom: int
    actual_left: int
    actual_right: int
    auto_detected: bool
    out_dims: tuple


def crop_channels_plan(planes, auto_detect=True, top=0, bottom=0, left=0, right=0, threshold=AUTO_THRESHOLD, detect=detect_valid_region):
    """:92-126 and :170-183; raises ValueError with the reference's message"""
    if len(planes) == 0:
        raise ValueError(NO_PATHS)
    rows0, cols0 = planes[0].shape
    if auto_detect:
        box = common_box([detect(p, threshold) for p in planes])
        if box[1] <= box[0] or box[3] <= box[2]:
            raise ValueError(NO_OVERLAP)
    else:
        box = (top, sat_sub(rows0, bottom), left, sat_sub(cols0, right))
    dims = []
    for p in planes:
        t, b, l, r = clamp_box(p.shape, *box)
        dims.append((b - t, r - l))
    return Plan(box, dims[0][0], dims[0][1], box[0], sat_sub(rows0, box[1]), box[2], sat_sub(cols0, box[3]), bool(auto_detect), tuple(dims))


def stats_row(st):
    return (st.min, st.max, st.median, st.mad, st.sigma, st.mean, st.valid_count)


def crop_channels(planes, plan, oracle=None):
    """:133-168: the cropped planes and, with the oracle, compute_image_stats of each (ImageStats::default() for an empty one)"""
    cropped = [crop_array(p, *plan.crop_box) for p in planes]
    if oracle is None:
        return cropped, None
    stats = [stats_row(oracle.compute_image_stats(c)) if c.size else (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0) for c in cropped]
    return cropped, stats


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def noise(shape, seed):
    """strictly positive noise well above AUTO_THRESHOLD: every pixel valid"""
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=F32) * F32(0.9) + F32(0.05)).astype(F32)


def bordered(shape, border, seed):
    """noise inside a zero border of (top, bottom, left, right) pixels -- what the warp leaves around a registered frame"""
    rows, cols = shape
    t, b, l, r = border
    out = np.zeros(shape, F32)
    if rows - t - b > 0 and cols - l - r > 0:
        out[t:rows - b, l:cols - r] = noise((rows - t - b, cols - l - r), seed)
    return out


def single(shape, r, c, value=1.0):
    out = np.zeros(shape, F32)
    out[r, c] = F32(value)
    return out
