"""Crafted star lists for the triangle matcher (csrc/affine.hip: tri_build / tri_bin_scan / tri_scatter / tri_bucket_sort /
tri_group_windows / the vote kernels, and the host's triangle_votes + match_pairs_from_votes).  Pure numpy: no GPU, no oracle, no
library.  Every list the matcher had seen before was a set of centroids of a random synthetic field; each family here is built for
one place where such lists never go, and tests/test_triangle_cases_cpu.py asserts with the restatement (tests/affine_restatement.py)
that the family still goes there.

    N  counts: a rigidly moved, slightly noisy random field cut to 4 .. 130 stars on either side of a 60-star list (partial last
       group of 64 reference triangles, the 25 / 26-star switch of who clears the vote matrices, the 60-star voting limit), lists
       of 0 / 1 / 3 stars and a 12-star cluster in which no triangle survives the 15 px rule
    S  a shortest side of exactly 15.0 px (kept) and its twin a hair shorter (dropped)
    E  equal sides: lattices and a line -- isosceles / equilateral-key / collinear triangles, buckets of more than 1024 triangles
    B  ratio_mid around 82.9: the last ratio_mid bucket (4095) saturates
    T  pairs of triangles one step either side of the 0.02 tolerance, in adjacent buckets
    U  vote matrices whose greedy pass goes deep into the lazily sorted remainder of the host's pair list
    G  eleven targets of all kinds against one reference: a group of 8 and a group of 3

CASES maps a name to (reference list, target list); GROUP_REF / GROUP_TARGETS are family G.  want(ref, tgt) is the restatement's
vote matrix, computed once per process and list pair.  All coordinates lie inside a 4096-pixel frame.
"""
import math

import numpy as np

FRAME = 4096.0
TOLERANCE = 0.02
TRI_BINS = 4096


def tri_bin(mid):
    """the device's ratio_mid bucket (csrc/affine.hip: tri_bin), for the conditions the fixtures state about buckets"""
    b = (np.asarray(mid, np.float64) - 1.0) / (TOLERANCE * 1.0001)
    return np.where(b >= TRI_BINS - 1, TRI_BINS - 1, np.minimum(b, TRI_BINS - 1).astype(np.int64))


def _moved(xy, ang_deg, tx, ty):
    a = math.radians(ang_deg)
    c, s = math.cos(a), math.sin(a)
    return np.column_stack([c * xy[:, 0] - s * xy[:, 1] + tx, s * xy[:, 0] + c * xy[:, 1] + ty])


def lattice(nx, ny, step, x0=200.0, y0=300.0):
    """row-major nx x ny lattice"""
    return np.array([(x0 + step * i, y0 + step * j) for j in range(ny) for i in range(nx)], np.float64)


# ---- N ---------------------------------------------------------------------------------------------------------------------------
_rng = np.random.default_rng(20260)
BASE = np.column_stack([_rng.uniform(300.0, 3700.0, 130), _rng.uniform(300.0, 3700.0, 130)])
MOVED = _moved(BASE - 2000.0, 0.8, 2011.5, 1990.25) + _rng.normal(0.0, 0.05, BASE.shape)
N_COUNTS = (4, 5, 8, 9, 25, 26, 59, 60, 61, 120, 130)
REF60 = np.ascontiguousarray(BASE[:60])
EMPTY = np.zeros((0, 2))
CLUSTER = lattice(4, 3, 3.0, 1500.0, 1500.0)   # every separation <= sqrt(81 + 36) < 15: no triangle survives


def n_list(k):
    return np.ascontiguousarray(MOVED[:k])


# ---- S ---------------------------------------------------------------------------------------------------------------------------
_others = np.column_stack([_rng.uniform(400.0, 3600.0, 10), _rng.uniform(400.0, 3600.0, 10)])
S_EXACT = np.vstack([[(0.0, 0.0), (9.0, 12.0)], _others])            # sqrt(81 + 144) is exactly 15.0
S_SHORT = np.vstack([[(0.0, 0.0), (9.0, 12.0 - 1e-9)], _others])

# ---- E ---------------------------------------------------------------------------------------------------------------------------
LATTICE_8 = np.ascontiguousarray(lattice(8, 8, 20.0)[:60])
LATTICE_10X6 = lattice(10, 6, 15.0)
LATTICE_3X3 = lattice(3, 3, 15.0)
LINE_60 = np.array([(100.0 + 16.0 * i, 2048.0) for i in range(60)], np.float64)
SUBLATTICE_9X5 = lattice(9, 5, 20.0, 207.5, 296.75)



def _equilateral(ax, half):
    """A = (ax, 0), B = A + (2 half, 0), C = (ax + half, cy) with cy within a few ulps of half * sqrt(3) such that the three f64
    distances are EQUAL (a square lattice holds no equilateral triangle; this one ties all three keys of both three-element
    sorts).  A sits on the frame's first row because cy's ulp is finest there: a few steps of it always hit the side length."""
    def d(p, q):
        dx, dy = p[0] - q[0], p[1] - q[1]
        return math.sqrt(dx * dx + dy * dy)
    a, b = (ax, 0.0), (ax + 2.0 * half, 0.0)
    cy = half * math.sqrt(3.0)
    for _ in range(32):
        cy = math.nextafter(cy, -math.inf)
    for _ in range(64):
        c = (ax + half, cy)
        if d(a, c) == d(a, b) and d(b, c) == d(a, b):
            return [a, b, c]
        cy = math.nextafter(cy, math.inf)
    raise AssertionError("no exactly equilateral triangle near this size")


# two equilateral triangles of different sizes and two stars beside them
EQUILATERAL = np.array(_equilateral(512.0, 32.0) + _equilateral(1024.0, 56.0) + [(700.0, 1900.0), (2500.0, 640.0)], np.float64)

# ---- B ---------------------------------------------------------------------------------------------------------------------------
# two stars 15 px apart and 58 on a line 1240 + 0.25 k px away: only the 58 triangles that hold both close stars survive (every
# other one has a side between two line stars, < 15 px), and their ratio_mid runs from 82.67 to 83.62 across the last buckets
# (the close pair is a hair MORE than 15 px apart, so that this family does not depend on which way the 15 px comparison goes: S's job)
B_LIST = np.vstack([[(2000.0, 100.0), (2009.0, 112.000001)], [(2000.0 - 1240.0 - 0.25 * k, 100.0) for k in range(58)]])

# ---- U ---------------------------------------------------------------------------------------------------------------------------
U_A = np.column_stack([_rng.uniform(100.0, 3900.0, 60), _rng.uniform(100.0, 3900.0, 60)])
U_B = np.column_stack([_rng.uniform(100.0, 3900.0, 60), _rng.uniform(100.0, 3900.0, 60)])


# ---- T ---------------------------------------------------------------------------------------------------------------------------
# Four stars: A, B = A + (64, 0), C and a far star D.  The reference's triangle ABC is the right triangle with legs 64 and 96
# (ratio_mid 1.5, ratio_long 1.8028).  The target's C is searched for, in steps of one ulp of its coordinate, so that the f64
# difference of the ratios -- exactly as the matcher computes it -- is the nearest reachable value below 0.02 (the "in" twin) and
# the nearest above (the "out" twin).  0.02 itself is not reachable: it is not a multiple of 2^-52.  The far stars differ between
# the lists, so that no other triangle pair is anywhere near the tolerance.
_T_A = (600.0, 700.0)
T_REF = np.array([_T_A, (_T_A[0] + 64.0, _T_A[1]), (_T_A[0], _T_A[1] + 96.0), (3000.0, 1000.0)], np.float64)


def _ratios(a, b, c):
    def d(p, q):
        dx, dy = p[0] - q[0], p[1] - q[1]
        return math.sqrt(dx * dx + dy * dy)
    s = sorted([d(a, b), d(b, c), d(a, c)])
    return s[1] / s[0], s[2] / s[0]


def _t_target(c):
    return np.array([_T_A, (_T_A[0] + 64.0, _T_A[1]), c, (1000.0, 3000.0)], np.float64)


def _search(which, point_of, lo, hi):
    """point_of(u) -> C; the difference of ratio `which` (0 mid, 1 long) grows with u on [lo, hi] and crosses 0.02 there.  Bisect
    to the crossing, then walk ulp by ulp around it: -> (u_in, u_out), the arguments whose |difference| is the largest that is not
    > 0.02 and the smallest that is."""
    r0 = _ratios(*[tuple(p) for p in T_REF[:3]])

    def diff(u):
        return abs(r0[which] - _ratios(_T_A, (_T_A[0] + 64.0, _T_A[1]), point_of(u))[which])
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if diff(mid) > TOLERANCE:
            hi = mid
        else:
            lo = mid
    u = lo
    for _ in range(64):
        u = math.nextafter(u, -math.inf)
    best_in, best_out = None, None
    for _ in range(128):
        dv = diff(u)
        if dv > TOLERANCE:
            if best_out is None or dv < best_out[0]:
                best_out = (dv, u)
        elif best_in is None or dv > best_in[0]:
            best_in = (dv, u)
        u = math.nextafter(u, math.inf)
    return best_in[1], best_out[1]


def _t_lists():
    # ratio_mid: C = A + (0, y), y around 64 * 1.52 -- ratio_long differs by 0.0166, inside the tolerance
    y_in, y_out = _search(0, lambda y: (_T_A[0], _T_A[1] + y), 96.5, 98.0)
    # ratio_long: C = A + (-x, 96), x around 2.3 -- ratio_mid differs by 0.0004, far inside
    x_in, x_out = _search(1, lambda x: (_T_A[0] - x, _T_A[1] + 96.0), 1.0, 4.0)
    return {"mid in": _t_target((_T_A[0], _T_A[1] + y_in)), "mid out": _t_target((_T_A[0], _T_A[1] + y_out)),
            "long in": _t_target((_T_A[0] - x_in, _T_A[1] + 96.0)), "long out": _t_target((_T_A[0] - x_out, _T_A[1] + 96.0))}


T_TARGETS = _t_lists()

# ---- the cases -------------------------------------------------------------------------------------------------------------------
CASES = {}
for _k in N_COUNTS:
    CASES[f"N ref {_k} stars"] = (n_list(_k), REF60)
    CASES[f"N tgt {_k} stars"] = (REF60, n_list(_k))
for _name, _l in (("no", EMPTY), ("one", n_list(1)), ("three", n_list(3)), ("cluster", CLUSTER)):
    CASES[f"N ref {_name}"] = (_l, REF60)
    CASES[f"N tgt {_name}"] = (REF60, _l)
CASES["S exactly 15 px"] = (S_EXACT, S_EXACT)
CASES["S short of 15 px"] = (S_SHORT, S_SHORT)
CASES["S exact against short"] = (S_EXACT, S_SHORT)
CASES["E lattice 8x8"] = (LATTICE_8, LATTICE_8)
CASES["E lattice 10x6"] = (LATTICE_10X6, LATTICE_10X6)
CASES["E lattice 3x3"] = (LATTICE_3X3, LATTICE_3X3)
CASES["E line"] = (LINE_60, LINE_60)
CASES["E lattice 8x8 against 9x5"] = (LATTICE_8, SUBLATTICE_9X5)
CASES["E equilateral"] = (EQUILATERAL, EQUILATERAL)
CASES["B last bucket"] = (B_LIST, B_LIST)
for _name, _l in T_TARGETS.items():
    CASES[f"T {_name}"] = (T_REF, _l)
CASES["U unrelated"] = (U_A, U_B)
CASES["U lattice 8x8"] = CASES["E lattice 8x8"]

GROUP_REF = REF60
GROUP_TARGETS = [n_list(60), EMPTY, n_list(3), CLUSTER, LATTICE_8, n_list(61), B_LIST, n_list(25), n_list(26), T_TARGETS["mid in"],
                 n_list(130)]
for _i, _l in enumerate(GROUP_TARGETS):
    CASES[f"G target {_i + 1}"] = (GROUP_REF, _l)

FAMILY = {name: name[0] for name in CASES}

for _r, _t in CASES.values():
    for _l in (_r, _t):
        assert _l.shape[0] == 0 or (_l.min() >= 0.0 and _l.max() < FRAME)

# ---- the restatement's answers, once per process ---------------------------------------------------------------------------------
_WANT = {}


def want(ref, tgt):
    """the restatement's 64 x 64 vote matrix (uint32) of a pair of lists, cached on the lists' contents"""
    import affine_restatement as ar
    key = (np.ascontiguousarray(ref, np.float64).tobytes(), np.ascontiguousarray(tgt, np.float64).tobytes())
    if key not in _WANT:
        m = ar.triangle_votes(ref, tgt).astype(np.uint32)
        m.setflags(write=False)
        _WANT[key] = m
    return _WANT[key]


def want_case(name):
    return want(*CASES[name])
