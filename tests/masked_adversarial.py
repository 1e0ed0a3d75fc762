"""Named, seeded, read-only fixtures for the star mask and the masked stretch loop (csrc/masked_stretch.hip beyond its select).

Every kernel there is a 256-lane grid-stride loop over at most cu_count x 8 workgroups, and the paint kernel runs one workgroup per
star: the edges are n = 1, n around 256 and one full pass of the grid (cu_count x 2048 pixels, 524 288 on 256 CUs).  So every plane is
at most 65 x 257, except ONE 601 x 901 case per family (541 501 pixels: every loop turns once), named "...-big".

tests/test_masked_adversarial_cpu.py holds each fixture to what it is for (and the oracle to tests/masked_restatement.py on all of
them); tests/test_gpu_masked_adversarial.py runs them on the device.  Nothing here knows the library.

Star-mask families (stars are given, so every result is exact):
  S-shapes     stars placed relative to the plane, in groups (one case each, and "all" = every group in one list):
                 border   on each corner pixel (fwhm exactly min_fwhm: kept), half a pixel outside each edge, far outside (empty box),
                          fwhm exactly max_fwhm (kept), one f64 step outside each bound and NaN (dropped)
                 discs    integer coordinates with fwhm 2.0 (growth 2.5, softness 4: lattice points with d2 == 25 == r2_inner and
                          d2 == 81 == r2_outer exactly), two concentric stars, one whose box covers the whole plane
                 cluster  >= 200 stars inside a 24 x 24 patch
               Each group once more with softness 0 ("hard"): with a skirt, `<` for `<=` is INVISIBLE at both edges (d2 == r2_inner
               gives t = 0, value 1 either way; d2 == r2_outer gives t = 1, value 0, which is never written) -- only the hard disc,
               whose two radii coincide, tells the two apart.
  S-nonfinite  x or y NaN, +-inf, +-1e300, 5e18; degenerate growth / softness / fwhm bounds; fwhm +inf
  S-protect    luminance protection at seven ceilings over an image with NaN, +-inf, pixels at and one step above the ceiling and a
               ramp across the coverage threshold
  S-order      the 40 x 60 "all" list reversed and in three seeded shuffles

Stretch families (the mask is given): M-tiny, M-long, M-clamp, M-subnormal, M-range.  Shared-mask families (exact because the
detection finds no star): RGB-starless, RGB-mixed.
"""
from dataclasses import dataclass, field

import numpy as np

F = np.float32
SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (1, 255), (1, 256), (1, 257), (16, 16), (40, 60), (65, 257)]
BIG_SHAPE = (601, 901)
SHAPES = SMALL_SHAPES + [BIG_SHAPE]
S_MIN_FWHM = 0.1
NONFINITE = [float("nan"), float("inf"), float("-inf"), 1e300, -1e300, 5e18]
CEILINGS = [0.85, 0.999999, 0.0, -0.5, 1.0, 1.5, float("nan")]


def _ro(a):
    a = np.ascontiguousarray(a, dtype=F)
    a.flags.writeable = False
    return a


@dataclass(frozen=True)
class MaskCase:
    name: str
    image: np.ndarray
    stars: tuple
    cfg: dict
    group: str = ""
    strict_coverage: bool = True    # the configuration allows 0 < coverage < 1
    lattice: tuple = ()             # (x, y, r2_inner, r2_outer) of the star on integer coordinates


@dataclass(frozen=True)
class StretchCase:
    name: str
    image: np.ndarray
    mask: np.ndarray
    cfg: dict
    stars_masked: int = 7
    stops_in: tuple = ()            # M-long: the loop stops converged at an iteration in [lo, hi]

    @property
    def coverage(self):
        with np.errstate(invalid="ignore"):
            return float((self.mask > F(0.01)).mean())


@dataclass(frozen=True)
class RgbCase:
    name: str
    r: np.ndarray
    g: np.ndarray
    b: np.ndarray
    cfg: dict = field(default_factory=dict)


def same_planes(a, b):
    """equal through the uint32 views, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def shape_id(shape):
    return "big" if shape == BIG_SHAPE else f"{shape[0]}x{shape[1]}"


# ---- S-shapes ------------------------------------------------------------------------------------------------------------------------
def whole_plane_fwhm(h, w):
    """fwhm of a star at the plane's centre whose box (soft radius = max(h, w) / 2 + 0.5 at growth 2.5, softness 4) just covers the
    plane: the corners stay outside its disc"""
    return max((max(h, w) / 2.0 + 0.5 - 4.0) / 2.5, S_MIN_FWHM)


def shapes_max_fwhm(h, w):
    return max(30.0, float(np.ceil(whole_plane_fwhm(h, w))) + 1.0)


def lattice_star(h, w):
    """near the origin, away from the cluster and outside the whole-plane star's hard disc: (0, 7), (7, 0), (6, 7), (7, 6), (8, 3) and
    (3, 8) are at d2 = 25, (12, 3) and (3, 12) at d2 = 81"""
    return (3.0, 3.0, 2.0)


def shapes_groups(h, w):
    """{group: [(x, y, fwhm)]} for an h x w plane (min_fwhm = S_MIN_FWHM, max_fwhm = shapes_max_fwhm(h, w))"""
    lo, hi = S_MIN_FWHM, shapes_max_fwhm(h, w)
    big_r = hi * 2.5 + 4.0                                                   # soft radius of a star of fwhm max_fwhm at growth 2.5
    border = [(0.0, 0.0, lo), (w - 1.0, 0.0, lo), (0.0, h - 1.0, lo), (w - 1.0, h - 1.0, lo),                     # corner pixels
              (w * 0.3, -0.5, 1.0), (w * 0.7, h - 0.5, 1.0), (-0.5, h * 0.6, 1.0), (w - 0.5, h * 0.4, 1.0),       # half a pixel outside
              (-100.0, h * 0.5, 3.0), (w * 0.5, h + 4000.0, 3.0),                                                # far outside: empty box
              (w * 0.25 - big_r, h * 0.5, hi),                                                                    # fwhm == max_fwhm: kept
              (w * 0.5, h * 0.5, float(np.nextafter(lo, -np.inf))), (w * 0.5, h * 0.5, float(np.nextafter(hi, np.inf))),   # dropped
              (w * 0.5, h * 0.5, float("nan"))]                                                                   # dropped
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    discs = [lattice_star(h, w), (w * 0.75 + 0.3, h * 0.25 + 0.6, 1.5), (w * 0.75 + 0.3, h * 0.25 + 0.6, 0.75),
             (cx, cy, whole_plane_fwhm(h, w))]
    rng = np.random.default_rng(1000 * h + w)
    x0, y0 = max(0, w - 24 - 8), max(0, h - 24 - 6)                          # (the far end from the lattice star)
    cluster = [(float(rng.uniform(x0, x0 + 24)), float(rng.uniform(y0, y0 + 24)), float(rng.uniform(0.5, 2.0))) for _ in range(220)]
    return {"border": border, "discs": discs, "cluster": cluster, "all": border + discs + cluster}


def _shapes_image(h, w):
    return _ro(np.random.default_rng(h * 7 + w).uniform(0.0, 1.0, (h, w)))


def shapes_cases():
    out = []
    for (h, w) in SHAPES:
        img = _shapes_image(h, w)
        lx, ly, lf = lattice_star(h, w)
        for group, stars in shapes_groups(h, w).items():
            for edge, softness in (("soft", 4.0), ("hard", 0.0)):
                if (h, w) == BIG_SHAPE and (group, edge) != ("all", "soft"):
                    continue
                cfg = dict(growth_factor=2.5, softness=softness, min_fwhm=S_MIN_FWHM, max_fwhm=shapes_max_fwhm(h, w))
                r = lf * 2.5
                out.append(MaskCase(f"S-shapes-{shape_id((h, w))}-{group}-{edge}", img, tuple(stars), cfg, group,
                                    lattice=(lx, ly, r * r, (r + softness) ** 2) if group in ("discs", "all") else ()))
    return out


def order_cases():
    base = next(c for c in shapes_cases() if c.name == "S-shapes-40x60-all-soft")
    out = [MaskCase("S-order-reversed", base.image, tuple(reversed(base.stars)), base.cfg, "all")]
    for seed in (1, 2, 3):
        idx = np.random.default_rng(seed).permutation(len(base.stars))
        out.append(MaskCase(f"S-order-shuffle{seed}", base.image, tuple(base.stars[i] for i in idx), base.cfg, "all"))
    return base, out


# ---- S-nonfinite ---------------------------------------------------------------------------------------------------------------------
NONFINITE_CONFIGS = {  # name: (cfg, the configuration allows a coverage strictly inside (0, 1))
    "default": (dict(), True),
    "g0-s0": (dict(growth_factor=0.0, softness=0.0), True),
    "g0-s3": (dict(growth_factor=0.0, softness=3.0), True),
    "s0": (dict(softness=0.0), True),
    "g-1": (dict(growth_factor=-1.0), True),
    "gnan": (dict(growth_factor=float("nan")), False),        # every radius is NaN: nothing is painted
    "sinf": (dict(softness=float("inf")), False),             # every skirt is infinite: t = 0, the whole plane is 1
    "g1e6": (dict(growth_factor=1e6), True),
    "wide-fwhm": (dict(min_fwhm=-1.0, max_fwhm=1e9), True),
}


def nonfinite_cases():
    h, w = 40, 60
    img = _shapes_image(h, w)
    wild = [(v, 20.0, 2.0) for v in NONFINITE] + [(30.0, v, 2.0) for v in NONFINITE] + [(float("nan"), float("inf"), 3.0)]
    out = []
    for name, (cfg, strict) in NONFINITE_CONFIGS.items():
        growth, softness = cfg.get("growth_factor", 2.5), cfg.get("softness", 4.0)
        finite = []
        for k, fw in enumerate((2.0, 3.0) + ((-0.5, 1e8) if name == "wide-fwhm" else ())):
            sr = fw * growth + softness
            # a disc larger than the plane is placed to the left of it, so that its edge crosses the plane near x = 20 + 7 k
            x = 20.0 + 7.0 * k - sr if np.isfinite(sr) and sr > 15.0 else 12.0 + 20.0 * k
            finite.append((x, 15.0 + 6.0 * k, fw))
        out.append(MaskCase(f"S-nonfinite-{name}", img, tuple(wild[:6] + finite[:1] + wild[6:] + finite[1:]), cfg, strict_coverage=strict))
    stars = tuple(wild + [(30.0, 20.0, float("inf")), (12.0, 15.0, 2.0)])
    out.append(MaskCase("S-nonfinite-fwhm-inf", img, stars, dict(max_fwhm=float("inf")), strict_coverage=False))   # an infinite disc
    return out


# ---- S-protect -----------------------------------------------------------------------------------------------------------------------
def protect_cases():
    h, w = 40, 60
    stars = ((10.2, 8.7, 2.0), (45.5, 30.1, 3.0), (58.0, 2.0, 1.5), (30.0, 20.0, 0.5))
    out = []
    for ceiling in CEILINGS:
        rng = np.random.default_rng(31)
        img = rng.uniform(0.0, 1.2, (h, w)).astype(F)
        c = F(ceiling)
        if c == c:
            if c > F(0.9):                                    # (a ceiling near or above 1: lift part of the noise above it)
                img[:, 30:] += c
            inv = F(1.0) / (F(1.0) - c) if c < F(1.0) else F(1.0)
            img[39, :3] = c                                   # equal to the ceiling: untouched
            img[39, 3:6] = np.nextafter(c, F(np.inf))         # one step above
            e = np.linspace(0.05, 0.07, 41).astype(F)         # smoothstep(e) = 0.01 at e = 0.0589...: the coverage threshold
            img[38, :41] = c + e / inv
        img[0, 0], img[0, 1], img[0, 2] = np.nan, np.inf, -np.inf
        img[9, 10], img[30, 45] = np.nan, np.inf              # under the discs too
        tag = "nan" if c != c else repr(float(ceiling))
        out.append(MaskCase(f"S-protect-{tag}", _ro(img), stars, dict(luminance_protect=True, luminance_ceiling=ceiling, min_fwhm=0.5),
                            strict_coverage=bool(c == c)))
    return out


def mask_cases():
    return shapes_cases() + nonfinite_cases() + protect_cases() + order_cases()[1]


# ---- stretch -------------------------------------------------------------------------------------------------------------------------
T0 = dict(iterations=40, convergence_threshold=0.0)


def tiny_cases():
    out = []
    for (h, w) in SMALL_SHAPES:
        rng = np.random.default_rng(h * 131 + w)
        img = rng.uniform(0.01, 1.0, (h, w))
        mask = rng.choice(np.array([0.0, 0.0, 0.0, 0.3, 0.7, 1.0]), (h, w))
        for tag, cfg in (("default", dict()), ("t0", T0)):
            out.append(StretchCase(f"M-tiny-{shape_id((h, w))}-{tag}", _ro(img), _ro(mask), cfg))
    return out


def _long_plane(seed, shape=(40, 52)):
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.01, 1.0, shape)
    mask = np.where(rng.uniform(0, 1, shape) < 0.2, 1.0, 0.4)
    return _ro(img), _ro(mask)


# the chunk in which the loop must stop by its own decision, per protection: the last iteration of the first chunk of 32, inside the
# second, inside the third.  (Fixture CONDITIONS: the CPU test holds the restatement to them.)
SELF_STOPPING = ((1.8, (32, 32)), (2.0, (33, 64)), (2.2, (65, 96)))


def long_cases():
    img, mask = _long_plane(21)
    out = [StretchCase(f"M-long-t0-{n}", img, mask, dict(iterations=n, convergence_threshold=0.0)) for n in (31, 32, 33, 64, 65)]
    big_img, big_mask = _long_plane(22, BIG_SHAPE)
    out.append(StretchCase("M-long-t0-65-big", big_img, big_mask, dict(iterations=65, convergence_threshold=0.0)))
    for protection, window in SELF_STOPPING:
        out.append(StretchCase(f"M-long-self-{protection}", img, mask, dict(iterations=200, protection_amount=protection), stops_in=window))
    return out


CLAMP_MASK_VALUES = np.array([0.0, 0.3, 1.0, 1.5, 2.0, -1.0, np.nan])
# A pixel outside [0, 1] stays there only under a blend weight mask * protection > 1 (x > 1 stretches to 1 and becomes
# 1 + blend (x - 1); x < 0 stretches to 0 and becomes blend x): it grows from iteration to iteration.  Under any other weight it is back
# inside after the next blend.  So protection 0.85 and 2.0 (weights up to 1.7 and 4) end outside on BOTH sides -- a pixel goes above 1
# in an iteration that darkens and below 0 in one that brightens, and the three-fold weight of -1 in the draw makes the first iteration
# overshoot so that both happen -- and the clamp has work to do; protection -0.5 (weights <= 0.5) leaves [0, 1] in its first iterations
# and ENDS inside: the flag that a blend raised must have been taken back by the time the loop stops.
CLAMP_MASK_DRAW = np.array([0.0, 0.3, 1.0, 1.5, 2.0, -1.0, -1.0, -1.0, np.nan])


def clamp_cases():
    rng = np.random.default_rng(41)
    img = _ro(rng.uniform(0.01, 1.0, (24, 40)))
    mask = _ro(rng.choice(CLAMP_MASK_DRAW, (24, 40)))
    out = []
    for protection in (0.85, 2.0, -0.5):
        for tag, cfg in (("6", dict(iterations=6)), ("65", dict(iterations=65, convergence_threshold=0.0))):
            out.append(StretchCase(f"M-clamp-p{protection}-{tag}", img, mask, dict(protection_amount=protection, **cfg)))
    rng = np.random.default_rng(42)
    out.append(StretchCase("M-clamp-p2.0-6-big", _ro(rng.uniform(0.01, 1.0, BIG_SHAPE)), _ro(rng.choice(CLAMP_MASK_DRAW, BIG_SHAPE)),
                           dict(protection_amount=2.0, iterations=6)))
    return out


def subnormal_cases():
    rng = np.random.default_rng(51)
    img = rng.uniform(2e-7, 4e-7, (30, 41)).astype(F)
    img[3, 5], img[17, 20] = F(3e38), F(1.5e-7)               # range > 2^126: 1 / range is subnormal
    mask = np.where(rng.uniform(0, 1, img.shape) < 0.1, 0.8, 0.0)
    return [StretchCase("M-subnormal", _ro(img), _ro(mask), dict()),
            StretchCase("M-subnormal-t0", _ro(img), _ro(mask), dict(iterations=12, convergence_threshold=0.0))]


def range_cases():
    rng = np.random.default_rng(61)
    shape = (33, 47)
    img = rng.uniform(0.2, 0.9, shape).astype(F)
    flat = img.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[:60]] = rng.uniform(1e-9, 1e-7, 60).astype(F)    # in (0, 1e-7]: outside the range, but normalised
    flat[idx[60]] = F(1e-7)
    flat[idx[61:80]] = -rng.uniform(0.1, 2.0, 19).astype(F)
    flat[idx[80:84]] = F(-0.0)
    flat[idx[84:88]] = np.nan
    flat[idx[88:90]] = np.inf
    flat[idx[90:92]] = -np.inf
    mask = np.where(rng.uniform(0, 1, shape) < 0.15, 0.9, 0.1)
    equal = np.full(shape, 0.375, F)                          # every valid pixel equal: range < 1e-10, the output is all zeros
    equal.reshape(-1)[idx[:30]] = np.nan
    equal.reshape(-1)[idx[30:60]] = F(-1.0)
    none = np.full(shape, -2.0, F)                            # no valid pixel
    none.reshape(-1)[idx[:10]] = np.nan
    none.reshape(-1)[idx[10:20]] = rng.uniform(1e-9, 9e-8, 10).astype(F)
    none.reshape(-1)[idx[20:25]] = np.inf
    return [StretchCase("M-range-mixed", _ro(img), _ro(mask), dict()),
            StretchCase("M-range-mixed-t0", _ro(img), _ro(mask), T0),
            StretchCase("M-range-equal", _ro(equal), _ro(mask), dict()),
            StretchCase("M-range-none", _ro(none), _ro(mask), dict())]


def stretch_cases():
    return tiny_cases() + long_cases() + clamp_cases() + subnormal_cases() + range_cases()


# ---- shared mask ---------------------------------------------------------------------------------------------------------------------
def _starless(seed, shape):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.05, 1.1, shape).astype(F)
    r, g, b = base, (rng.uniform(0.05, 1.1, shape).astype(F) * F(0.8)).astype(F), (rng.uniform(0.05, 1.1, shape).astype(F) * F(1.15)).astype(F)
    g[3 % shape[0], 3 % shape[1]] = np.nan
    b[5 % shape[0], 7 % shape[1]] = np.inf
    return _ro(r), _ro(g), _ro(b)


def rgb_cases():
    r, g, b = _starless(70, (96, 128))
    out = [RgbCase("RGB-starless", r, g, b), RgbCase("RGB-starless-t0", r, g, b, T0)]
    rng = np.random.default_rng(72)
    noise = rng.uniform(0.05, 1.1, (96, 128)).astype(F)
    zeros = np.zeros((96, 128), F)
    zeros[rng.uniform(0, 1, zeros.shape) < 0.05] = F(-1.0)
    out.append(RgbCase("RGB-mixed", _ro(noise), _ro(zeros), _ro(np.full((96, 128), 0.5, F)), dict(luminance_ceiling=0.2)))
    out.append(RgbCase("RGB-starless-big", *_starless(73, BIG_SHAPE)))
    return out
