"""Adversarial planes for the phase correlation (pure numpy / scipy, fixed seeds: no GPU, no library, no oracle import).

csrc/phase_corr.hip is tested elsewhere on smooth fields shifted by a few pixels: one clear maximum well inside the surface, a
spectrum far above the 1e-15 cut of the cross-power normalisation, min / max spread over every row.  The families built here leave
that regime on purpose.  Every builder returns the planes plus the CLAIM it makes about them:

  1 ties        target = -reference: the surface is exactly -1 at index 0 and exactly 0 elsewhere, so the maximum is tied over every
                index >= 1 and the first of them (index 1) must win; and a target that is non-zero only where the periodic Hann
                window is exactly 0: an all-zero surface, tied over every index, peak index 0
  2 border      exact shifts of 0 / +-1 px of one aperiodic field: the peak sits in row / column 0 or fr-1 / fc-1 of the surface and
                the 3-point refinement reads its circular neighbours
  3 cut         fields whose cross-power magnitudes straddle the 1e-15 cut: a share of the bins (between 5 % and 95 %) is zeroed
  4 deciding    constant planes in which ONE pixel decides is_constant_or_zero, placed where each loop of minmax_finite_kernel
                (two float4 loads in flight, the single-load remainder, the scalar tail, the grid-stride row loop) is the only
                reader; minmax_paths restates which loop reads which pixel
  5 thresholds  15 / 16 finite pixels, +-inf, |max - min| on either side of 1e-10f
  6 length one  transforms of length 1 (rows == 1 or cols == 1) and the smallest planes that are still correlated
  7 boxes       downsample boxes without a finite pixel
  8 rounds      stacks of 17 / 18 / 34 frames (rounds of 16 targets) with degenerate targets at the first and last place of a round
                and a whole degenerate round followed by a live one; a 520 x 300 round in which the live pairs are compacted twice
                (past the degenerate targets, then past the pairs that keep their coarse answer)
  9 tables      a sequence of dimensions that revisits the table cache's keys

Family 1 is pinned by the CPU oracle (oracle/orc_phasecorr.c, the kernel's butterflies) plus the closed form written down in
negated_pair, NOT by tests/phasecorr_restatement.py: numpy's FFT rounds differently, B = -A still holds there but the inverse
transform of the constant -1 leaves 1e-17-sized residues instead of exact zeros, and the tie is gone.  Every other family is held to
both.  tests/test_phasecorr_adversarial_cpu.py holds every fixture to its claim, so that a fixture that has drifted fails there and
the GPU test (tests/test_gpu_phasecorr_adversarial.py) cannot pass by testing nothing.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
K_BLOCK = 256                # minmax_finite_kernel / scale_peak_kernel: threads per workgroup
K_MINMAX_PARTIALS = 2048     # workgroups per plane of minmax_finite_kernel: rows beyond are reached by the grid stride
K_PARTIALS = 256             # workgroups per surface of scale_peak_kernel
K_BATCH = 16                 # pairs per round of ab_phase_correlate_many_device

_CACHE = {}


def next_pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def smooth_field():
    """one aperiodic field (smoothed noise, about +-500), made once: crops of it are exact shifts of each other"""
    if "field" not in _CACHE:
        from scipy.ndimage import gaussian_filter
        _CACHE["field"] = gaussian_filter(np.random.default_rng(1).standard_normal((1300, 1300)), 2.0).astype(F32) * F32(1000)
    return _CACHE["field"]


def shifted_crops(base, shape, shift, origin=(40, 50)):
    """(ref, tgt) with tgt(y, x) = ref(y - sy, x - sx), both cut from base"""
    (r, c), (sy, sx), (y0, x0) = shape, shift, origin
    return base[y0:y0 + r, x0:x0 + c].copy(), base[y0 - sy:y0 - sy + r, x0 - sx:x0 - sx + c].copy()


# ---- 1: exact ties ---------------------------------------------------------------------------------------------------------------
TIE_SHAPES = ((4, 4), (33, 17), (100, 75), (128, 128), (512, 512))
TIE_COARSE_TO_FINE = (520, 300)


def negated_pair(shape):
    """(reference, -reference, claim).  Negation is exact through the window and every butterfly, so B = -A bit for bit;
    pi = a.y b.x - a.x b.y is exactly 0 and sqrt(pr pr) == |pr|, so the cross power is exactly (-1, 0) in every bin, whose inverse
    transform is exact: -1 at index 0, 0 elsewhere.  The first maximum is index 1 = (py, px) = (0, 1): its x neighbours are -1 and 0
    (refinement -0.5, dx = 0.5), its y neighbours 0 and 0 (denominator 0, dy = 0); mean = -1/N, sigma = 1/sqrt(N) to rounding, so
    confidence = (0 + 1/N) sqrt(N) = 1/sqrt(N).  At 2 x 2 (correlate_single only: 4 pixels are degenerate for phase_correlate) both
    x neighbours of index 1 are the -1 and dx = 1.0."""
    rows, cols = shape
    ref = (np.random.default_rng(rows * 1000 + cols).standard_normal(shape) * 1000.0 + 5000.0).astype(F32)
    fr, fc = next_pow2(rows), next_pow2(cols)
    surface = np.zeros((fr, fc), np.float64)
    surface[0, 0] = -1.0
    claim = dict(surface=surface, peak_index=1, dx=1.0 if fc == 2 else 0.5, dy=0.0, confidence=1.0 / np.sqrt(float(fr * fc)))
    return ref, -ref, claim


def negated_pair_coarse_to_fine():
    """520 x 300: the downsampled planes are exact negations too and both passes tie.  Coarse (0.5, 0) scales to
    (0.5 * 300 / 512, 0); the target's crop centre round(150 + 0.29) = 150 is the reference's, so the pair is refined by (0.5, 0)."""
    ref, tgt, _ = negated_pair(TIE_COARSE_TO_FINE)
    return ref, tgt, dict(dx=0.5 * 300.0 / 512.0 + 0.5, dy=0.0, confidence=1.0 / 512.0)


def window_null_plane(n):
    """n x n, non-zero only in row 0 and column 0 where hann_periodic is exactly 0: >= 16 finite pixels and not constant (NOT
    degenerate), yet its windowed buffer is all zeros -> every cross-power bin is cut -> an all-zero surface, peak index 0"""
    rng = np.random.default_rng(n)
    p = np.zeros((n, n), F32)
    p[0, :] = (rng.standard_normal(n) * 1000.0).astype(F32)
    p[:, 0] = (rng.standard_normal(n) * 1000.0).astype(F32)
    return p


def window_null_pairs():
    """[(name, reference, target)]: the window-null plane as the target and as the reference of a normal field, 128 and 512 px"""
    out = []
    for n in (128, 512):
        field, null = smooth_field()[40:40 + n, 50:50 + n].copy(), window_null_plane(n)
        out += [(f"target-{n}", field, null), (f"reference-{n}", null, field)]
    return out


# ---- 2: peaks on the surface's border --------------------------------------------------------------------------------------------
BORDER_SHAPES = ((128, 128), (100, 75))                  # both transform at 128 x 128
# shift (sy, sx) of the target -> the surface's peak (py, px): minus the shift, wrapped
BORDER_SHIFTS = {(0, 0): (0, 0), (1, -1): (127, 1), (-1, 1): (1, 127), (0, 1): (0, 127), (-1, 0): (1, 0)}


def border_pair(shape, shift):
    return shifted_crops(smooth_field(), shape, shift)


# ---- 3: bins on both sides of the 1e-15 cut --------------------------------------------------------------------------------------
CUT_SHIFT = (3, -2)
CUT_FRACTION_BOUNDS = (0.05, 0.95)


def cut_pairs():
    """[(name, reference, target)], 128 x 128: the smooth field scaled by 1e-6 (range about 1e-3: far from the 1e-10 degenerate
    threshold; its steep spectrum falls through the cut) and white noise scaled by 1e-9 (a flat spectrum that sits on the cut)"""
    smooth = tuple(p * F32(1e-6) for p in shifted_crops(smooth_field(), (128, 128), CUT_SHIFT))
    noise = np.random.default_rng(3).standard_normal((140, 140)).astype(F32) * F32(1e-9)
    return [("smooth-1e-6",) + smooth, ("noise-1e-9",) + shifted_crops(noise, (128, 128), CUT_SHIFT, origin=(5, 5))]


# ---- 4: the pixel that decides is_constant_or_zero -------------------------------------------------------------------------------
def minmax_paths(rows, cols, ld, aligned=True):
    """Which loop of minmax_finite_kernel reads column x (an array of names, one per column) and which rows are reached only by
    the grid stride (a bool per row).  The float4 form needs a 16-byte aligned base and ld % 4 == 0; thread t then reads the float4s
    t + 512 k ('load-a') and t + 256 + 512 k ('load-b') while the second is inside the row, one more single float4 ('remainder'),
    and columns past the last whole float4 one by one ('tail'); otherwise every column is read one by one ('scalar')."""
    vec = aligned and ld % 4 == 0
    c4 = cols // 4 if vec else 0
    names = np.empty(cols, dtype=object)
    names[4 * c4:] = "tail" if vec else "scalar"
    j = np.arange(c4)
    per_f4 = np.where(j % (2 * K_BLOCK) >= K_BLOCK, "load-b", np.where(j + K_BLOCK < c4, "load-a", "remainder"))
    names[:4 * c4] = np.repeat(per_f4, 4)
    return names, np.arange(rows) >= min(K_MINMAX_PARTIALS, rows)


def field_of(shape, seed):
    """a normal field of exactly this shape (the shared field is too small for 2056 columns / 2050 rows)"""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 2.0).astype(F32) * F32(1000)


class Deciding:
    """target: constant 7.0 but for 9.0 at `pixel`; reference: a field of ref_shape.  The pair is correlated over the common
    window (rows, cols), the target's row stride is target.shape[1]; `path` / `strided` say which loop of minmax_finite_kernel is
    the only reader of the pixel when the target starts on a 16-byte boundary."""

    def __init__(self, name, shape, pixel, path, strided=False, ref_cols=None):
        self.name, self.pixel, self.path, self.strided = name, pixel, path, strided
        self.target = np.full(shape, 7.0, F32)
        self.target[pixel] = 9.0
        self.reference = field_of((shape[0], ref_cols or shape[1]), seed=shape[0] + shape[1])
        self.rows, self.cols, self.ld = shape[0], min(shape[1], self.reference.shape[1]), shape[1]

    def without_the_pixel(self):
        return np.full(self.target.shape, 7.0, F32)


def deciding_cases():
    """17 x 2054 has ld % 4 == 2: a contiguous plane of that width takes the one-by-one form, whatever the pixel.  The float4
    loops are reached by the same pixels in a target of 2056 columns: as wide as its reference (cols = ld = 2056), and against a
    2054-column reference (cols = 2054, ld = 2056: a row that ends in the scalar tail)."""
    return [
        Deciding("2054-tail", (17, 2054), (16, 2053), "scalar"),
        Deciding("2054-second-load", (17, 2054), (3, 1024 + 77), "scalar"),
        Deciding("2054-remainder", (17, 2054), (8, 2049), "scalar"),
        Deciding("grid-stride", (2050, 16), (2048, 5), "remainder", strided=True),
        Deciding("last-of-odd", (20, 30), (19, 29), "scalar"),
        Deciding("2056-first-load", (17, 2056), (11, 1023), "load-a"),
        Deciding("2056-second-load", (17, 2056), (3, 1024 + 77), "load-b"),
        Deciding("2056-remainder", (17, 2056), (8, 2053), "remainder"),
        Deciding("2056/2054-second-load", (17, 2056), (3, 2047), "load-b", ref_cols=2054),
        Deciding("2056/2054-remainder", (17, 2056), (8, 2049), "remainder", ref_cols=2054),
        Deciding("2056/2054-tail", (17, 2056), (16, 2053), "tail", ref_cols=2054),
    ]


RAGGED_WINDOW = (30, 46)      # the stack's common window: 46 is no multiple of 4 ...
RAGGED_SHAPE = (37, 52)       # ... the ragged frame's row stride 52 is


def ragged_stack_frames():
    """four frames; frame 2 is 37 x 52, constant inside the common 30 x 46 window and wild (noise, NaN, inf) in its padding:
    degenerate, offset (0, 0), whatever the padding holds.  The row's last whole float4 ends at column 43, columns 44 and 45 are
    the scalar tail, the padding starts inside the next float4."""
    base, rng = smooth_field(), np.random.default_rng(4)
    (r, c), shifts = RAGGED_WINDOW, [(0, 0), (2, -1), (0, 0), (-1, 2)]
    frames = [shifted_crops(base, (r, c), s, origin=(300, 400))[1] for s in shifts]
    ragged = (rng.standard_normal(RAGGED_SHAPE) * 1000.0).astype(F32)
    ragged[r:, ::3], ragged[::2, c:] = np.nan, np.inf
    ragged[:r, :c] = 100.0
    frames[2] = ragged
    return frames


# ---- 5: the thresholds themselves ------------------------------------------------------------------------------------------------
def threshold_cases():
    """[(name, reference, target, degenerate)]: fewer than 16 finite pixels or |max - min| < 1e-10f makes a plane degenerate"""
    rng = np.random.default_rng(5)
    small = (rng.standard_normal((4, 5)) * 1000.0 + 500.0).astype(F32)
    fifteen, sixteen, infs = small.copy(), small.copy(), small.copy()
    fifteen.ravel()[[0, 6, 7, 13, 19]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    sixteen.ravel()[[0, 6, 7, 13]] = [np.nan, np.inf, -np.inf, np.nan]
    infs.ravel()[[1, 5, 9, 12, 18]] = [np.inf, -np.inf, np.inf, -np.inf, np.inf]               # 15 finite, not a NaN among them
    field = smooth_field()[200:208, 300:308].copy()
    flat_with_inf = np.full((8, 8), 3.0, F32)                 # 60 finite pixels, all equal: +-inf must not enter min / max
    flat_with_inf[2, 3], flat_with_inf[5, 1], flat_with_inf[7, 7], flat_with_inf[0, 0] = np.inf, -np.inf, np.inf, -np.inf
    cases = [("15-finite", small, fifteen, True), ("16-finite", small, sixteen, False), ("15-finite-inf", small, infs, True),
             ("15-finite-reference", fifteen, small, True), ("flat-with-inf", field, flat_with_inf, True)]
    for v, degenerate in ((9e-11, True), (1.1e-10, False), (2e-10, False)):
        spike = np.zeros((8, 8), F32)
        spike[3, 4] = v
        cases.append((f"spike-{v:g}", field, spike, degenerate))
    return cases


# ---- 6: transform length 1 and the smallest planes -------------------------------------------------------------------------------
LENGTH_ONE_SHAPES = ((1, 16), (16, 1), (1, 64), (64, 1), (4, 4), (1, 600), (600, 1), (513, 16), (16, 513))
TOO_SMALL_SHAPES = ((3, 5), (1, 15))


def small_pair(shape):
    """crops of the field shifted by (1, -2), by 0 along an axis of length 1"""
    return shifted_crops(smooth_field(), shape, (1 if shape[0] > 1 else 0, -2 if shape[1] > 1 else 0), origin=(100, 120))


# ---- 7: downsample boxes with no finite pixel ------------------------------------------------------------------------------------
BOX_SHAPES = ((600, 800), (1024, 520), (1025, 520))
NAN_BLOCK = (slice(100, 140), slice(200, 260))      # 40 x 60
INF_BLOCK = (slice(300, 310), slice(50, 60))        # 10 x 10


def box_pair(shape):
    """(reference, target, holes): the target holds a NaN block and a +inf block; holes = for each block the rows / columns of
    the downsampled plane whose boxes lie wholly inside it (they must come out as 0.0f)"""
    ref, tgt = shifted_crops(field_of((shape[0] + 40, shape[1] + 40), seed=7), shape, (3, -4), origin=(20, 20))
    tgt[NAN_BLOCK], tgt[INF_BLOCK] = np.nan, np.inf
    sy, sx = shape[0] / min(512, shape[0]), shape[1] / min(512, shape[1])
    inside = lambda sl, s: slice(int(np.ceil(sl.start / s)), int(np.floor(sl.stop / s)))     # box o covers [floor(o s), ceil((o + 1) s))
    return ref, tgt, [(inside(b[0], sy), inside(b[1], sx)) for b in (NAN_BLOCK, INF_BLOCK)]


# ---- 8: batch rounds -------------------------------------------------------------------------------------------------------------
BATCH_SHAPE = (96, 128)
BATCH_SHIFTS = [(dy, dx) for dy in (-5, -3, -2, 0, 1, 2, 4) for dx in (-6, -4, -1, 3, 5)]      # 35 distinct, none (0, 0)


def degenerate_frame(kind, shape=BATCH_SHAPE):
    if kind == "constant":
        return np.full(shape, 100.0, F32)
    f = np.full(shape, np.nan, F32)
    if kind == "15-finite":
        f.ravel()[np.arange(15) * 801 + 7] = (np.arange(15) * 10.0 + 1.0).astype(F32)
    else:
        assert kind == "all-nan"
    return f


# name -> (frames, {frame index: kind of degenerate target}); frame k is target k - 1, round (k - 1) // 16, place (k - 1) % 16
MIXED_DEGENERATE = {1: "all-nan", 4: "constant"}
BATCH_LAYOUTS = {
    "one-round": (17, {1: "all-nan", 9: "constant", 16: "15-finite"}),                        # first, middle and last place
    "round-and-one": (18, {1: "15-finite", 16: "all-nan"}),                                   # the second round is one live pair
    "round-and-a-dead-one": (18, {2: "constant", 17: "all-nan"}),                             # ... is one degenerate pair
    "dead-middle-round": (34, {5: "constant", **{k: ("all-nan", "15-finite", "constant")[k % 3] for k in range(17, 33)}}),
    "coarse-to-fine-mixed": (8, MIXED_DEGENERATE),
}


# 520 x 300 (above 512: coarse-to-fine).  Row shifts 2 and -3 leave the target's 512-row crop whole (the pair is refined), 9 and -11
# push it over the border (the crops' sizes differ: the coarse answer is kept) -- so the round's live pairs are compacted twice, once
# past the degenerate targets (`live`) and once more past the pairs that keep their coarse answer (`fine`)
MIXED_SHAPE = (520, 300)
MIXED_SHIFTS = {2: (2, -3), 3: (9, 5), 5: (-3, 4), 6: (-11, -7), 7: (1, -1)}
MIXED_KEPT = {3, 6}           # frames whose coarse answer is kept


def mixed_batch_frames():
    """(frames, degenerate, kept): 8 frames = 7 targets of one round: dead, refined, kept, dead, refined, kept, refined"""
    base, rng = smooth_field(), np.random.default_rng(12)
    r, c = MIXED_SHAPE
    cut = lambda sy, sx: base[40 - sy:40 - sy + r, 50 - sx:50 - sx + c].copy()
    frames = [cut(0, 0)] + [None] * 7
    for k, shift in MIXED_SHIFTS.items():
        frames[k] = cut(*shift) + rng.standard_normal(MIXED_SHAPE).astype(F32)
    for k, kind in MIXED_DEGENERATE.items():
        frames[k] = degenerate_frame(kind, MIXED_SHAPE)
    return frames, dict(MIXED_DEGENERATE), set(MIXED_KEPT)


def crop_sizes_match(coarse_dx, coarse_dy, rows, cols):
    """phase_correlation.rs:66-80 from the coarse pass's (unscaled) shift: True = the centred 512 px crops of the reference and of
    the target have equal sizes and the pair is refined, False = the target's crop is clipped and the coarse answer is kept"""
    cy = min(max(rows // 2 + round_to_i32(coarse_dy * rows / 512.0), 0), rows - 1)
    cx = min(max(cols // 2 + round_to_i32(coarse_dx * cols / 512.0), 0), cols - 1)
    size = lambda c, n: min(c + 256, n) - max(c - 256, 0)
    return (size(cy, rows), size(cx, cols)) == (size(rows // 2, rows), size(cols // 2, cols))


def batch_frames(name):
    """(frames, degenerate): frame 0 is the reference, every live frame a crop at its own shift plus a little noise"""
    if name == "coarse-to-fine-mixed":
        return mixed_batch_frames()[:2]
    n, degenerate = BATCH_LAYOUTS[name]
    base, rng = smooth_field(), np.random.default_rng(8)
    r, c = BATCH_SHAPE
    cut = lambda sy, sx: base[700 - sy:700 - sy + r, 600 - sx:600 - sx + c].copy()
    frames = [cut(0, 0)] + [cut(*BATCH_SHIFTS[k - 1]) + rng.standard_normal(BATCH_SHAPE).astype(F32) for k in range(1, n)]
    for k, kind in degenerate.items():
        frames[k] = degenerate_frame(kind)
    return frames, degenerate


def round_to_i32(v):
    """`offset.round() as i32` (combine.rs:135-136): half away from zero, NaN -> 0"""
    return 0 if np.isnan(v) else int(np.sign(v) * np.floor(abs(v) + 0.5))


# ---- 9: the table cache ----------------------------------------------------------------------------------------------------------
TABLE_SEQUENCE = ((100, 75), (75, 100), (100, 75), (520, 300), (512, 300), (100, 75))


def table_pairs():
    """one (reference, target) per entry of TABLE_SEQUENCE; equal shapes get the SAME pair, so their surfaces must be identical"""
    pairs = {}
    for shape in TABLE_SEQUENCE:
        if shape not in pairs:
            pairs[shape] = shifted_crops(smooth_field(), shape, (2, -3), origin=(60 + len(pairs), 70))
    return [pairs[shape] for shape in TABLE_SEQUENCE]
