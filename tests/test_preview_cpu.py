"""Pins tests/preview_restatement.py -- the checker of tests/test_gpu_preview.py -- by values worked by hand, checks that the
fixtures have the properties their names claim, and the error returns of the preview section that need no device.  No GPU."""
import ctypes as C

import numpy as np

import preview_restatement as R

F32 = np.float32


def r32(x):
    """one f32 rounding of a Python-float (f64) result: exact for a single +, -, *, / or sqrt of f32 operands"""
    return float(F32(x))


# ---- fast_log / the AVX2 route's asinh ----------------------------------------------------------------------------------------------
def test_fast_log_of_powers_of_two_is_k_ln2():
    for k in (-126, -64, -10, -1, 1, 2, 3, 10, 24, 64, 127):
        got = R.fast_log(np.array([2.0 ** k], F32))[0]
        want = F32(k) * R.LN_2
        assert R.bits(got) == R.bits(want), (k, got, want)
    assert R.bits(R.fast_log(np.array([1.0], F32)))[0] == 0, "fast_log(1) is +0"


def test_overflow_value_is_128_ln2_with_either_sign():
    big = F32(128) * R.LN_2
    assert abs(float(big) - 88.72284) < 1e-5
    got = R.fast_asinh_avx2(np.array([1e20, -1e20, 3e38, -3e38, np.inf, -np.inf], F32))
    assert (R.bits(got) == R.bits(np.array([big, -big, big, -big, big, -big], F32))).all(), got
    # and the small end: inner rounds to 1 at or below 2^-24, the result is a zero that keeps the sign
    tiny = R.fast_asinh_avx2(np.array([2.0 ** -24, -2.0 ** -24, 1e-30, -1e-30, 0.0, -0.0], F32))
    assert (R.bits(tiny) == np.array([0, 0x80000000] * 3, np.uint32)).all(), tiny


def test_avx2_asinh_is_finite_and_sign_symmetric_over_a_sweep():
    rng = np.random.default_rng(20)
    mag = np.exp(rng.uniform(np.log(1e-44), np.log(3e38), 1 << 20))
    x = (mag * rng.choice([-1.0, 1.0], mag.size)).astype(F32)
    x[:6] = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], F32)
    pos, neg = R.fast_asinh_avx2(x), R.fast_asinh_avx2(-x)
    assert np.isfinite(pos).all()
    assert ((R.bits(pos) ^ R.bits(neg)) == 0x80000000).all()
    assert (pos[~np.signbit(x)] >= 0).all() and (pos[np.signbit(x)] <= 0).all()


def test_avx2_asinh_error_against_arcsinh():
    """0.5 <= |x| <= 1e18.  The bound is the route's own arithmetic: four f32 roundings stand between the exact value and the result
    (inner, the polynomial's log1p, e * LN_2, their sum), each at most 2^-24 relative to a result they do not exceed, on top of the
    polynomial's fit (a few 1e-8): 4 * 2^-23 = 4.8e-7.  Measured over this sweep: 2.13e-7."""
    rng = np.random.default_rng(0)
    x = np.exp(rng.uniform(np.log(0.5), np.log(1e18), 1 << 20)).astype(F32)
    x = np.concatenate([x, -x])
    got = R.fast_asinh_avx2(x).astype(np.float64)
    want = np.arcsinh(x.astype(np.float64))
    rel = np.abs(got - want) / np.abs(want)
    print(f"max relative error {rel.max():.3e} at x = {x[rel.argmax()]!r}")
    assert rel.max() < 4 * 2.0 ** -23


# ---- the scalar route ------------------------------------------------------------------------------------------------------------------
def test_scalar_taylor_branch_matches_a_hand_expansion():
    for x in (0.25, -0.375, 0.4999, 1e-3, -1e-20):
        x = float(F32(x))
        x2 = r32(x * x)
        inner = r32(r32(1.0 / 6.0) - r32(r32(x2 * 3.0) / 40.0))
        want = r32(x * r32(1.0 - r32(x2 * inner)))
        got = R.fast_asinh_scalar(np.array([x], F32))[0]
        assert R.bits(got) == R.bits(F32(want)), (x, got, want)
    # 0.25 * (1 - 0.0625 * (1/6 - 0.1875 / 40)) = 0.24746908...
    assert abs(float(R.fast_asinh_scalar(np.array([0.25], F32))[0]) - 0.24746908) < 3e-8


def test_scalar_log_branch_is_the_rounded_f64_log():
    for x in (0.5, -0.5, 1.0, 7.25, -1e6):
        x = float(F32(x))
        ax = abs(x)
        arg = r32(ax + r32(np.sqrt(r32(r32(ax * ax) + 1.0))))
        want = F32(np.copysign(1.0, x)) * F32(np.log(arg))
        assert R.bits(R.fast_asinh_scalar(np.array([x], F32))[0]) == R.bits(want), x
    assert np.isposinf(R.fast_asinh_scalar(np.array([1e20], F32))[0]) and np.isneginf(R.fast_asinh_scalar(np.array([-1e20], F32))[0])


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def test_median_and_mad_by_hand():
    junk = [np.nan, 0.0, -3.0, np.inf, 1e-7]
    # odd m: median 3, deviations {2, 1, 0, 1, 97} -> MAD 1; low = s[0], high = s[min(int(4.995), 4)]
    median, sigma, low, high, m = R.preview_stats(np.array([100, 1, 3] + junk + [4, 2], F32).reshape(2, 5))
    assert (m, median, sigma, low, high) == (5, 3.0, F32(1.4826), 1.0, 100.0)
    # even m: median (2 + 3) / 2, deviations {1.5, 0.5, 0.5, 2.5} -> MAD (0.5 + 1.5) / 2 = 1
    median, sigma, low, high, m = R.preview_stats(np.array([5, 1] + junk + [3, 2], F32).reshape(1, 9))
    assert (m, median, sigma, low, high) == (4, 2.5, F32(1.4826), 1.0, 5.0)
    # a MAD of zero leaves sigma at its floor
    assert R.preview_stats(np.full((3, 3), 7.0, F32))[1] == F32(1e-10)


def test_rank_indices():
    want = {1: (0, 0), 2: (0, 1), 99: (0, 98), 100: (1, 99), 101: (1, 100), 1000: (10, 999), 1001: (10, 999)}
    for m, (lo, hi) in want.items():
        vals = np.random.default_rng(m).permutation(np.arange(1, m + 1)).astype(F32).reshape(1, m)
        _, _, low, high, count = R.preview_stats(vals)
        assert (count, int(low) - 1, int(high) - 1) == (m, lo, hi), m


def test_no_valid_pixel_returns_the_input():
    img = R.all_invalid_plane((3, 5))
    assert R.preview_stats(img) == (0.0, 0.0, 0.0, 0.0, 0)
    for route in (R.AVX2, R.SCALAR):
        assert (R.bits(R.robust_asinh_preview(img, route)) == R.bits(img)).all()
        assert not R.render_asinh_and_save(img, route).any()


def test_plus_infinity_is_valid_in_the_avx2_body_only():
    img = np.array([[90, 100, np.inf, 110, 120, 95, 105, 115, 101, np.inf, 99]], F32)
    avx2, scalar = R.robust_asinh_preview(img, R.AVX2), R.robust_asinh_preview(img, R.SCALAR)
    high = R.preview_stats(img)[3]
    assert avx2[0, 2] == avx2[0, 4] > 0 and high == 120, "in a chunk +inf is clamped to `high`"
    assert avx2[0, 9] == 0 and scalar[0, 2] == 0 and scalar[0, 9] == 0
    neg = img.copy()
    neg[0, 2] = -np.inf
    assert R.robust_asinh_preview(neg, R.AVX2)[0, 2] == 0


def test_avx2_route_takes_the_scalar_formula_in_its_tail():
    img = R.star_field((9, 23), 4)   # 207 pixels: 25 chunks and a tail of 7
    avx2, scalar = R.robust_asinh_preview(img, R.AVX2), R.robust_asinh_preview(img, R.SCALAR)
    assert (R.bits(avx2).ravel()[200:] == R.bits(scalar).ravel()[200:]).all()
    assert (R.bits(avx2).ravel()[:200] != R.bits(scalar).ravel()[:200]).any(), "the two formulas differ in some last bit"


# ---- renderers -------------------------------------------------------------------------------------------------------------------------
def test_renderers_by_hand():
    img = np.array([[np.nan, 0.0, 1.0, 2.0, 3.0, -1.0, np.inf, 1e-7]], F32)
    got, mn, mx = R.render_grayscale(img, 8)          # min -1, max 3: inv = 63.75
    assert (mn, mx) == (-1.0, 3.0) and got.tolist() == [[0, 0, 127, 191, 255, 0, 0, 0]]
    got16 = R.render_grayscale(img, 16)[0]            # inv = 16383.75
    assert got16.shape == (1, 8, 2) and got16.view(">u2")[..., 0].tolist() == [[0, 0, 32767, 49151, 65535, 0, 0, 0]]
    assert got16[0, 2].tolist() == [0x7F, 0xFF], "big-endian pairs"
    s = np.array([[np.nan, -0.5, 0.0, 0.5, 1.0, 7.0, np.inf, -np.inf]], F32)
    assert R.render_stretched(s, 8).tolist() == [[0, 0, 0, 127, 255, 255, 255, 0]]
    assert R.render_stretched(s, 16).view(">u2")[..., 0].tolist() == [[0, 0, 0, 32767, 65535, 65535, 65535, 0]]
    # no finite pixel: min = f32::MAX, max = f32::MIN, every sample 0
    got, mn, mx = R.render_grayscale(np.array([[np.nan, np.inf]], F32))
    assert (mn, mx) == (R.F32_MAX, -R.F32_MAX) and not got.any()


# ---- the GPU tests' fixtures -------------------------------------------------------------------------------------------------------------
def test_fixtures_have_the_properties_their_names_claim():
    assert [s[0] * s[1] % 8 for s in R.SHAPES] == [1, 7, 0, 7, 1, 0, 1, 7]
    for shape in R.SHAPES:
        n = shape[0] * shape[1]
        cases = dict(R.preview_cases(shape))
        if n > 1:
            assert int(R.is_valid(cases["stars_even"]).sum()) % 2 == 0 and int(R.is_valid(cases["stars_odd"]).sum()) % 2 == 1
        assert not R.is_valid(cases["all_invalid"]).any() and int(R.is_valid(cases["one_valid"]).sum()) == 1
        if n >= 5:
            assert all(np.isnan(v) and np.isnan(cases["all_invalid"]).any() or (cases["all_invalid"] == v).any() for v in R.INVALID_VALUES)
        const = R.preview_stats(cases["constant"])
        assert const[1] == F32(1e-10) and not R.robust_asinh_preview(cases["constant"], R.AVX2).any()
        st = R.preview_stats(cases["outliers"])
        assert st[1] == F32(1e-10) and st[3] == F32(1e9)
        if n > 1:   # (a plane of one pixel is its own median)
            with np.errstate(all="ignore"):
                sc = R.scaled_of(cases["outliers"], st)
                assert np.isinf(sc.max() * sc.max()), "|scaled|^2 overflows"
        if n >= 8:
            tie = cases["tie4"]
            s = np.sort(tie[R.is_valid(tie)])
            m = s.size
            assert m % 2 == 0 and len(set(s[m // 2 - 2:m // 2 + 2].tolist())) == 1 and s[m // 2 - 3] < s[m // 2] < s[m // 2 + 2]
        if n >= 64:
            bad = cases["nonfinite"].ravel()
            body = 8 * (n // 8)
            for sel in (bad[:body], bad[body:]) if n % 8 >= 3 else (bad[:body],):
                assert np.isnan(sel).any() and np.isposinf(sel).any() and np.isneginf(sel).any()
        for name, img, stats in R.stats_cases(shape):
            with np.errstate(all="ignore"):
                sc = np.abs(R.scaled_of(img, stats)).ravel()
            if name == "subnormal_scaled":
                assert ((sc > 0) & (sc < np.finfo(F32).tiny)).mean() > 0.9
            if name == "around_half" and n >= 16 and n % 8 >= 2:
                tail = sc[8 * (n // 8):]
                assert (tail < 0.5).any() and (tail >= 0.5).any()
        rp = R.render_plane(shape).ravel()
        if n >= 64:
            assert np.isnan(rp).any() and np.isinf(rp).any() and (rp < 0).any() and (rp > 1).any()


# ---- error returns that need no device ----------------------------------------------------------------------------------------------------
def test_a_null_context_is_invalid_everywhere():
    from astroburst_amd import _lib
    L = _lib.lib()
    img = np.ones((2, 2), F32)
    p = _lib.Plane(C.c_void_p(img.ctypes.data), 2, 2, 0)
    st = _lib.AsinhStatsC()
    buf = (C.c_uint8 * 8)()
    assert L.ab_asinh_preview_stats(None, C.byref(p), C.byref(st)) == _lib.AB_ERR_INVALID
    assert L.ab_asinh_normalize_with_stats(None, C.byref(p), C.byref(st), 0, C.byref(p)) == _lib.AB_ERR_INVALID
    assert L.ab_robust_asinh_preview(None, C.byref(p), 0, C.byref(p), None) == _lib.AB_ERR_INVALID
    assert L.ab_render_asinh_preview(None, C.byref(p), 0, buf, 0, None) == _lib.AB_ERR_INVALID
    assert L.ab_render_grayscale(None, C.byref(p), 8, buf, 0, None, None) == _lib.AB_ERR_INVALID
    assert L.ab_render_stretched(None, C.byref(p), 8, buf, 0) == _lib.AB_ERR_INVALID
