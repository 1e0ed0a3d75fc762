"""Numpy restatement of the robust asinh preview and the byte renderers, the checker of tests/test_gpu_preview.py.

Restated line by line from the reference: math/simd.rs:9-23 (fast_asinh_scalar, is_valid), :28-84 (fast_log_avx2), :96-111
(fast_asinh_avx2), :115-158 (normalize_chunk_avx2), :160-214 (asinh_normalize_simd), :263-271 (find_minmax_simd's scalar statement),
math/median.rs:46-63 (median_f32_mut), infra/render/grayscale.rs:10-74 (the four renderers, write_png_l16's big-endian pairs) and
cmd/common.rs:242-261 (render_asinh_and_save's composition).  Every step is one np.float32 operation (numpy neither fuses nor
flushes subnormals), the bit steps go through uint32 / int32 views, the order statistics through np.sort, the rank products through
Python floats (f64) as the reference's `m as f64 * 0.01` does.

This restatement is NOT checked against a build of the Rust reference (no Rust toolchain is part of this project's environment);
tests/test_preview_cpu.py pins it by hand-worked values instead.

One definition replaces a host's bits: the scalar route's ln (the platform's logf in the reference) is the f32 rounding of the f64
log of the f32 argument, as include/astroburst_hip.h defines it.
"""
import numpy as np

F32 = np.float32
U32 = np.uint32
AVX2, SCALAR = 0, 1

PADDING_THRESHOLD = F32(1e-7)
MAD_TO_SIGMA = F32(1.4826)
LN_2 = F32(0.6931471805599453)
FRAC_1_SQRT_2 = F32(0.7071067811865476)
P = [F32(c) for c in (3.3333331174e-1, -2.4999993993e-1, 2.0000714765e-1, -1.6668057665e-1, 1.4249322787e-1, -1.2420140846e-1,
                      1.1676998740e-1, -1.1514610310e-1, 7.0376836292e-2)]
F32_MAX = np.finfo(F32).max


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def ulp_distance(a, b):
    """distance in representable f32 values (the sign-magnitude patterns mapped onto a line)"""
    def line(x):
        i = bits(x).astype(np.int64)
        return np.where(i >= 0x80000000, 0x80000000 - i, i)
    return np.abs(line(a) - line(b))


# ---- the map ----------------------------------------------------------------------------------------------------------------------
def fast_log(x):
    """fast_log_avx2 (simd.rs:28-84), one lane per element"""
    x = np.ascontiguousarray(x, F32)
    xi = x.view(U32)
    with np.errstate(all="ignore"):
        m = ((xi & U32(0x007FFFFF)) | U32(0x3F000000)).view(F32)
        e = (((xi & U32(0x7F800000)) >> U32(23)).astype(np.int32) - np.int32(0x7E)).astype(F32)
        lt = m < FRAC_1_SQRT_2
        m = np.where(lt, m + m, m)
        e = e - np.where(lt, F32(1), F32(0))
        f = m - F32(1)
        f2 = f * f
        f3 = f2 * f
        r = np.full(f.shape, P[8], F32)
        for p in P[7::-1]:
            r = r * f + p
        log1pf = (f - F32(0.5) * f2) + f3 * r
        out = e * LN_2 + log1pf
    assert out.dtype == F32
    return out


def fast_asinh_avx2(x):
    """fast_asinh_avx2 (simd.rs:96-111)"""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        inner = a + np.sqrt(a * a + F32(1))
    return (fast_log(inner).view(U32) | (x.view(U32) & U32(0x80000000))).view(F32)


def fast_asinh_scalar(x):
    """fast_asinh_scalar (simd.rs:9-18); ln by the definition (module docstring)"""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        x2 = x * x
        taylor = x * (F32(1) - x2 * (F32(1) / F32(6) - x2 * F32(3) / F32(40)))
        arg = ax + np.sqrt(ax * ax + F32(1))
        log = np.where(x >= 0, F32(1), F32(-1)) * np.log(arg.astype(np.float64)).astype(F32)
        out = np.where(ax < F32(0.5), taylor, log)
    assert out.dtype == F32
    return out


def is_valid(v):
    return np.isfinite(v) & (v > PADDING_THRESHOLD)


def _lanes_avx2(v, median, isa, low, high):
    """normalize_chunk_avx2's vector loop (simd.rs:133-145): max_ps / min_ps return their second operand on an unordered compare"""
    with np.errstate(all="ignore"):
        valid = (v == v) & (v > PADDING_THRESHOLD)
        raised = np.where(v > low, v, low)
        clamped = np.where(raised < high, raised, high)
        scaled = (clamped - median) * isa
    return np.where(valid, fast_asinh_avx2(scaled), F32(0)).astype(F32)


def _lanes_scalar(v, median, isa, low, high):
    """the scalar loop (simd.rs:148-157 = :203-211)"""
    with np.errstate(all="ignore"):
        clamped = np.where(v < low, low, np.where(v > high, high, v))
        scaled = isa * (clamped - median)
    return np.where(is_valid(v), fast_asinh_scalar(scaled), F32(0)).astype(F32)


def scaled_of(img, stats, route=SCALAR):
    """the asinh's argument per pixel (the scalar route's operand order unless route = AVX2), for the tests' own bookkeeping"""
    median, sigma, low, high = (F32(s) for s in stats[:4])
    with np.errstate(all="ignore"):
        isa = F32(10) / sigma
        v = np.ascontiguousarray(img, F32)
        clamped = np.where(v < low, low, np.where(v > high, high, v))
        return (clamped - median) * isa if route == AVX2 else isa * (clamped - median)


def preview_stats(img):
    """simd.rs:163-180 -> (median, sigma, low, high, m), all zero for m == 0"""
    flat = np.ascontiguousarray(img, F32).ravel()
    s = np.sort(flat[is_valid(flat)])
    m = int(s.size)
    if m == 0:
        return F32(0), F32(0), F32(0), F32(0), 0

    def median_f32(sorted_vals):  # median_f32_mut (math/median.rs:46-63)
        k = sorted_vals.size
        return sorted_vals[k // 2] if k % 2 else (sorted_vals[k // 2 - 1] + sorted_vals[k // 2]) / F32(2)

    with np.errstate(all="ignore"):
        median = F32(median_f32(s))
        dev = np.sort(np.abs(s - median))
        sigma = max(F32(median_f32(dev) * MAD_TO_SIGMA), F32(1e-10))
    low = s[int(float(m) * 0.01)]
    high = s[min(int(float(m) * 0.999), m - 1)]
    return median, F32(sigma), F32(low), F32(high), m


def normalize_with_stats(img, stats, route):
    """the map of asinh_normalize_simd with the given (median, sigma, low, high, m); m == 0 returns the input"""
    img = np.ascontiguousarray(img, F32)
    if int(stats[4]) == 0:
        return img.copy()
    median, sigma, low, high = (F32(s) for s in stats[:4])
    with np.errstate(all="ignore"):
        isa = F32(10) / sigma
    flat = img.ravel()
    out = _lanes_scalar(flat, median, isa, low, high)
    if route == AVX2:
        body = 8 * (flat.size // 8)  # counted from flat index 0
        out[:body] = _lanes_avx2(flat[:body], median, isa, low, high)
    return out.reshape(img.shape)


def robust_asinh_preview(img, route):
    """asinh_normalize_simd (simd.rs:160-214)"""
    return normalize_with_stats(img, preview_stats(img), route)


# ---- the renderers ------------------------------------------------------------------------------------------------------------------
def find_minmax(data):
    """find_minmax_simd's scalar statement (simd.rs:263-271)"""
    flat = np.ascontiguousarray(data, F32).ravel()
    fin = flat[np.isfinite(flat)]
    return (F32(fin.min()), F32(fin.max())) if fin.size else (F32_MAX, F32(-F32_MAX))


def _samples(x, top, bits_):
    """`as u8` / `as u16` of x.clamp(0, top): truncating, NaN -> 0; 16-bit samples as big-endian byte pairs"""
    with np.errstate(all="ignore"):
        q = np.where(np.isnan(x), F32(0), np.minimum(np.maximum(x, F32(0)), top))
        q = np.trunc(q).astype(np.uint32)
    if bits_ == 8:
        return q.astype(np.uint8)
    return q.astype(">u2").view(np.uint8).reshape(q.shape + (2,))


def render_grayscale(data, bits_=8):
    """render_grayscale / render_grayscale_16bit (grayscale.rs:10-50) -> (bytes, min, max)"""
    data = np.ascontiguousarray(data, F32)
    top = F32(255) if bits_ == 8 else F32(65535)
    mn, mx = find_minmax(data)
    with np.errstate(all="ignore"):
        rng = max(F32(mx - mn), F32(1e-10))
        inv = top / F32(rng)
        x = np.where(is_valid(data), (data - mn) * inv, F32(0))
    return _samples(x.astype(F32), top, bits_), mn, mx


def render_stretched(data, bits_=8):
    """render_stretched_8bit / _16bit (grayscale.rs:52-74): no validity test"""
    data = np.ascontiguousarray(data, F32)
    top = F32(255) if bits_ == 8 else F32(65535)
    with np.errstate(all="ignore"):
        c = np.where(data < 0, F32(0), np.where(data > 1, F32(1), data))  # f32::clamp: a NaN stays a NaN
        x = c * top
    return _samples(x.astype(F32), top, bits_)


def render_asinh_and_save(img, route):
    """cmd/common.rs:242-261 up to the encoder: render_grayscale(robust_asinh_preview(img))"""
    return render_grayscale(robust_asinh_preview(img, route), 8)[0]


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 7), (1, 8), (3, 5), (37, 53), (256, 256), (257, 129), (1031, 769))
OFFSET_SHAPE = (257, 129)   # taken again from device pointers offset by one and by three floats
INVALID_VALUES = np.array([np.nan, -np.inf, 0.0, -2.5, 1e-7], F32)  # (1e-7f itself is not above the threshold)


def star_field(shape, seed=0):
    """a sky of 100 +- 3 with a few dozen Gaussian stars: every pixel valid"""
    rows, cols = shape
    rng = np.random.default_rng(1000 * seed + rows * 31 + cols)
    img = rng.normal(100.0, 3.0, shape)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for _ in range(max(1, min(40, rows * cols // 200))):
        y, x, a, w = rng.uniform(0, rows), rng.uniform(0, cols), rng.uniform(50, 5000), rng.uniform(0.8, 2.5)
        img += a * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * w * w))
    return np.maximum(img, 1.0).astype(F32)


def with_parity(img, odd):
    """the plane with its valid count made odd / even by invalidating pixel 0 (planes of one pixel are left alone)"""
    img = img.copy()
    if img.size > 1 and (int(is_valid(img).sum()) % 2 == 1) != odd:
        img.flat[0] = np.nan
    return img


def tie_plane(shape):
    """distinct values with the four middle ranks made equal (even m): the median is the mean of two tied values"""
    n = shape[0] * shape[1]
    vals = (F32(10) + np.arange(n, dtype=F32) * F32(0.25)).astype(F32)
    if n % 2:
        vals[0] = np.nan
    order = np.flatnonzero(is_valid(vals))
    m = order.size
    if m >= 4:
        vals[order[m // 2 - 2:m // 2 + 2]] = vals[order[m // 2]]
    return np.random.default_rng(7).permutation(vals).reshape(shape)


def all_invalid_plane(shape):
    n = shape[0] * shape[1]
    return np.resize(INVALID_VALUES, n).reshape(shape)


def one_valid_plane(shape):
    img = all_invalid_plane(shape)
    img.flat[img.size // 2] = F32(5)
    return img


def constant_plane(shape):
    return np.full(shape, F32(3.25), F32)


def outlier_plane(shape):
    """a constant sky (MAD 0: sigma at its floor) with every 200th pixel at 1e9: above 0.1 % of the pixels, so `high` is an outlier
    and |scaled|^2 overflows f32"""
    img = np.full(shape, F32(100), F32)
    img.flat[::200] = F32(1e9)
    return img


def nonfinite_plane(shape):
    """a star field with NaN / +inf / -inf inside the 8-pixel chunks and in the n % 8 tail"""
    img = star_field(shape, 3)
    n = img.size
    bad = np.array([np.nan, np.inf, -np.inf], F32)
    body = 8 * (n // 8)
    for k in range(min(6, body)):             # inside the chunks (one pixel in three of the first two chunks)
        if k % 2 == 1 or body < 8:
            img.flat[k] = bad[k % 3]
    if n >= 64:
        img.flat[17], img.flat[18], img.flat[19] = bad
    for k in range(body, n):                  # the tail
        img.flat[k] = bad[(k - body) % 3] if (k - body) % 2 == 0 else img.flat[k]
    return img


def preview_cases(shape):
    """(name, plane) for the whole-preview tests"""
    return [
        ("stars_even", with_parity(star_field(shape, 1), False)),
        ("stars_odd", with_parity(star_field(shape, 2), True)),
        ("tie4", tie_plane(shape)),
        ("all_invalid", all_invalid_plane(shape)),
        ("one_valid", one_valid_plane(shape)),
        ("constant", constant_plane(shape)),
        ("outliers", outlier_plane(shape)),
        ("nonfinite", nonfinite_plane(shape)),
    ]


def stats_cases(shape):
    """(name, plane, stats) for the map with the caller's statistics: arguments the robust statistics of positive data cannot reach"""
    n = shape[0] * shape[1]
    rng = np.random.default_rng(n)
    # scaled = (v - 1) * 1e-37 with |v - 1| up to 0.05: subnormal (below 1.18e-38) and, for all but a v of exactly 1, non-zero
    sub = (F32(1) + rng.uniform(-0.05, 0.05, n)).astype(F32).reshape(shape)
    sub_stats = (F32(1), F32(1e38), F32(0.25), F32(4), n)
    # isa = 1: scaled = v - 100; every pixel, the tail's included, alternates around |scaled| = 0.5 with both signs
    edge = (F32(100) + np.resize(np.array([0.3, -0.3, 0.7, -0.7, 0.4999, -0.5, 0.5, 2.0, -45.0], F32), n)).astype(F32).reshape(shape)
    edge_stats = (F32(100), F32(10), F32(1), F32(1000), n)
    # a wide sweep of magnitudes through the log branch and fast_log's whole exponent range
    wide = np.exp(rng.uniform(np.log(1e-6), np.log(1e30), n)).astype(F32).reshape(shape)
    wide_stats = (F32(1), F32(0.01), F32(1e-7), F32(3e38), n)
    return [("subnormal_scaled", sub, sub_stats), ("around_half", edge, edge_stats), ("wide", wide, wide_stats)]


def render_plane(shape):
    """an input for the plain renderers: signed values around [0, 1] with invalid, negative and non-finite pixels mixed in"""
    n = shape[0] * shape[1]
    rng = np.random.default_rng(n + 5)
    img = rng.uniform(-0.25, 1.25, n).astype(F32)
    img[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, 1e-7, 1.0, 0.5], F32), img[::7].size)
    return img.reshape(shape)
