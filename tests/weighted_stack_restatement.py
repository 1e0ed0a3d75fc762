"""A plain numpy statement of ab_stack_weighted's definition (include/astroburst_hip.h), written from that definition and the
reference's sigma_clip_combine (core/stacking/combine.rs:14-92).  It is what the GPU kernel is held to bit for bit, and
tests/test_stack_weighted_cpu.py holds IT to the oracle.

Vectorised over the pixels only.  Everything whose order matters runs as an explicit loop: the f64 sums of iterations >= 1 over
the samples in ascending value order, the final weighted sums over the frames in ascending frame index.  np.sum is pairwise and is
used for integer counts only.  Every f32 step is an np.float32 operation; f64 is np.float64, one rounding per operation."""
import numpy as np

F = np.float32
D = np.float64
MAD_TO_SIGMA = 1.4826  # types/constants.rs:7


def normalise(frames, weights, scales, offsets):
    """-> (s [P, k] f32 normalised samples of the ACTIVE frames in frame order, w [k] f64).  A frame of scale 1 and offset 0 is read
    as it is; every other one is an f32 multiply followed by an f32 add."""
    act = [f for f in range(len(frames)) if weights[f] > 0]
    cols = []
    with np.errstate(all="ignore"):
        for f in act:
            p = np.asarray(frames[f], F).reshape(-1)
            if F(scales[f]) == F(1) and F(offsets[f]) == F(0):
                cols.append(p.copy())
            else:
                cols.append(((p * F(scales[f])).astype(F) + F(offsets[f])).astype(F))
    return np.stack(cols, axis=1), np.array([weights[f] for f in act], D)


def clip(s, sigma_low, sigma_high, max_iter):
    """sigma_clip_combine's rejection on every row of s [P, k] (non-finite entries take no part), with the sums of iterations >= 1
    in ascending value order.  -> (v [P, k] the samples sorted with +inf where not finite, alive [P, k] bool over v, m [P] finite
    count, rejected [P], last_center [P] f32)"""
    P, k = s.shape
    fin = np.isfinite(s)
    m = fin.sum(axis=1)
    v = np.sort(np.where(fin, s, F(np.inf)), axis=1)
    alive = np.arange(k)[None, :] < m[:, None]
    rejected = np.zeros(P, np.int64)
    last_center = np.full(P, np.nan, F)
    running = m >= 2                      # combine.rs:21-26: nothing to clip below two samples
    sl, sh = F(sigma_low), F(sigma_high)
    rows = np.arange(P)
    with np.errstate(all="ignore"):
        for it in range(int(max_iter)):
            length = alive.sum(axis=1)
            running = running & (length >= 2)          # :33-35
            if not running.any():
                break
            if it == 0:                                # :37-48
                med = v[rows, m // 2]
                devs = np.sort(np.where(alive, np.abs((v - med[:, None]).astype(F)), F(np.inf)), axis=1)
                mad = devs[rows, m // 2]
                sigma = np.maximum(mad.astype(D) * D(MAD_TO_SIGMA), D(1e-10)).astype(F)
                center = med
            else:                                      # :49-61
                nn = length.astype(D)
                S = np.zeros(P, D)
                for i in range(k):                     # ascending value order, one f64 add per sample
                    S = S + np.where(alive[:, i], v[:, i].astype(D), D(0))
                mean = S / np.maximum(nn, D(1))
                Q = np.zeros(P, D)
                for i in range(k):
                    d = v[:, i].astype(D) - mean
                    Q = Q + np.where(alive[:, i], d * d, D(0))
                variance = Q / np.maximum(nn - D(1), D(1))
                center = mean.astype(F)
                sigma = np.maximum(np.sqrt(variance), D(1e-10)).astype(F)
            last_center = np.where(running, center, last_center)   # :63
            lo = (-sl * sigma).astype(F)                             # :65-66
            hi = (sh * sigma).astype(F)
            dev = (v - center[:, None]).astype(F)
            ok = alive & (dev >= lo[:, None]) & (dev <= hi[:, None])   # :68-74
            removed = length - ok.sum(axis=1)
            alive = np.where(running[:, None], ok, alive)
            rejected = rejected + np.where(running, removed, 0)      # :76-78
            running = running & (removed != 0)                       # :80-82
    return v, alive, m, rejected, last_center


def stack_weighted(frames, weights, scales=None, offsets=None, sigma_low=3.0, sigma_high=3.0, max_iterations=5):
    """-> (image f32 [rows, cols], weight plane f32 [rows, cols], rejected).  frames: equally sized 2-D arrays."""
    n = len(frames)
    weights = [float(w) for w in weights]
    scales = [1.0] * n if scales is None else [float(x) for x in scales]
    offsets = [0.0] * n if offsets is None else [float(x) for x in offsets]
    shape = np.asarray(frames[0]).shape
    s, w = normalise(frames, weights, scales, offsets)
    P, k = s.shape
    v, alive, m, rejected, last_center = clip(s, sigma_low, sigma_high, max_iterations)
    length = alive.sum(axis=1)
    with np.errstate(all="ignore"):
        # the survivors are the values between the smallest and the largest one left; equal values share their fate
        lo_v = np.min(np.where(alive, v, F(np.inf)), axis=1)
        hi_v = np.max(np.where(alive, v, F(-np.inf)), axis=1)
        num = np.zeros(P, D)
        den = np.zeros(P, D)
        for f in range(k):                             # ascending frame index: one f64 multiply and one f64 add per frame
            keep = np.isfinite(s[:, f]) & (s[:, f] >= lo_v) & (s[:, f] <= hi_v)
            num = num + np.where(keep, w[f] * s[:, f].astype(D), D(0))
            den = den + np.where(keep, w[f], D(0))
        mean = (num / den).astype(F)
    fallback = np.where(np.isfinite(last_center), last_center, F(0))   # :85-88
    image = np.where(length == 0, fallback, mean).astype(F)
    wsum = np.where(length == 0, F(0), den.astype(F)).astype(F)
    one = m == 1                                       # :24-26: the sample itself
    if one.any():
        image[one] = v[one, 0]
    image[m == 0] = F(0)                               # :21-23
    wsum[m == 0] = F(0)
    return image.reshape(shape), wsum.reshape(shape), int(rejected.sum())
