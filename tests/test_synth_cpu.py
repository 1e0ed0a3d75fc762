"""The synthetic generator without a GPU: the ChaCha12 stream against published and hand-checked answers, the library's host entry
points (ab_synth_rng_f64, ab_synth_chacha_block, ab_synth_star_field, ab_synth_config_default) against the numpy restatement bit
for bit, the restatement itself against hand-worked cases, and the conditions the GPU tests' fixtures rest on."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_restatement as R  # noqa: E402


def _keystream_hex(words, nbytes):
    return np.asarray(words, "<u4").tobytes()[:nbytes].hex()


# ---- the stream --------------------------------------------------------------------------------------------------------------
def test_restatement_chacha_known_answers():
    z = [0] * 8
    assert _keystream_hex(R.chacha_blocks(z, 0, 1)[0], 32) == "9bf49a6a0755f953811fce125f2683d50429c3bb49e074147e0089a52eae155f"
    assert _keystream_hex(R.chacha_blocks(z, 1, 1)[0], 16) == "0bd58841203e74fe86fc71338ce0173d"
    assert _keystream_hex(R.chacha_blocks(z, 0, 2)[1], 16) == "0bd58841203e74fe86fc71338ce0173d"
    # the same quarter-round with 20 rounds: RFC 7539's all-zero vector
    assert _keystream_hex(R.chacha_blocks(z, 0, 1, rounds=20)[0], 16) == "76b8e0ada0f13d90405d6ae55386bd28"


def test_library_chacha_known_answers():
    import astroburst_amd as ab
    z = np.zeros(8, np.uint32)
    assert _keystream_hex(ab.synth_chacha_block(z, 0, 12), 32) == "9bf49a6a0755f953811fce125f2683d50429c3bb49e074147e0089a52eae155f"
    assert _keystream_hex(ab.synth_chacha_block(z, 1, 12), 16) == "0bd58841203e74fe86fc71338ce0173d"
    assert _keystream_hex(ab.synth_chacha_block(z, 0, 20), 16) == "76b8e0ada0f13d90405d6ae55386bd28"
    key = np.array(R.seed_key(42), np.uint32)
    for ctr in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 61):   # the counter's carry into word 13
        assert np.array_equal(ab.synth_chacha_block(key, ctr, 12), R.chacha_blocks(R.seed_key(42), ctr, 1)[0])
    with pytest.raises(ab.AstroBurstError):
        ab.synth_chacha_block(z, 0, 8)


SEEDED = {42: (0.5265574090027738, 0.5427252099031439, 0.6364650991438949),
          123: (0.17325464426155657, 0.15229643060221798, 0.9306584906609464),
          0: (0.7311134158637046, 0.7734601843532382, 0.025844634233355035)}


def test_seeded_first_draws():
    """first draws of three seeds from a second restatement of rand's algorithms (not verified against a Rust build)"""
    import astroburst_amd as ab
    for seed, want in SEEDED.items():
        assert tuple(R.rng_f64(seed, 0, 3)) == want
        assert tuple(ab.synth_rng_f64(seed, 0, 3)) == want
    assert abs(R.rng_f64(42, 3, 1)[0] - 0.40590176) < 1e-8


@pytest.mark.parametrize("seed", [0, 42, 123, 2 ** 64 - 1])
def test_rng_f64_equals_restatement(seed):
    import astroburst_amd as ab
    for skip in (0, 7, 31, 32, 2 ** 29, 2 ** 40):   # 32 draws = 64 words: rand_chacha refills four blocks at a time
        for n in (1, 9, 64):
            got, want = ab.synth_rng_f64(seed, skip, n), R.rng_f64(seed, skip, n)
            assert got.tobytes() == want.tobytes(), (seed, skip, n)
    assert ab.synth_rng_f64(seed, 5, 0).size == 0
    s = R.Stream(seed, chunk=16)
    assert [s.draw() for _ in range(40)] == list(R.rng_f64(seed, 0, 40))


# ---- star fields -------------------------------------------------------------------------------------------------------------
FIELDS = {"uniform": (R.uniform_field, ()), "king_cluster": (R.king_cluster, (50.0, 500.0)), "exponential_disk": (R.exponential_disk, (200.0, 60.0))}


@pytest.mark.parametrize("kind", sorted(FIELDS))
@pytest.mark.parametrize("n_stars", [0, 1, 37])
def test_star_field_equals_restatement(kind, n_stars):
    import astroburst_amd as ab
    fn, par = FIELDS[kind]
    got = ab.synth_star_field(field_type=(kind, *par), n_stars=n_stars)
    want = fn(*dict(R.DEFAULT_FIELD, n_stars=n_stars).values(), *par)
    assert got.shape == (n_stars, 5) and got.tobytes() == want.tobytes()
    if kind == "uniform" and n_stars:   # star 0 by hand: flux draw first, then x, y, temperature
        assert got[0, 0] == 0.5427252099031439 * 2048 and got[0, 1] == 0.6364650991438949 * 2048 and got[0, 2] == 0.0
        assert got[0, 4] == 3000.0 + 0.40590175823077668 * 27000.0
        a, b = math.pow(100.0, -1.5), math.pow(50000.0, -1.5)
        assert got[0, 3] == math.pow(a + 0.5265574090027738 * (b - a), 1.0 / -1.5)


def test_star_field_draw_order_and_other_seeds():
    import astroburst_amd as ab
    for seed in (0, 7, 2 ** 64 - 1):
        got = ab.synth_star_field(field_type=("exponential_disk", 150.0, 30.0), n_stars=5, seed=seed, width=300, height=200)
        want = R.exponential_disk(300, 200, 5, 100.0, 50000.0, seed, 150.0, 30.0)
        assert got.tobytes() == want.tobytes()
    # the disk puts stars outside the frame (what render_stars has to survive)
    far = R.exponential_disk(64, 64, 200, 100.0, 50000.0, 1, 400.0, 10.0)
    assert (far[:, 0] < -20).any() and (far[:, 0] > 84).any()


def test_star_field_rejects_what_would_not_terminate():
    import astroburst_amd as ab
    for par in ((0.0, 500.0), (50.0, 0.0), (-1.0, 10.0), (50.0, float("inf")), (float("nan"), 10.0), (1e200, 1.0)):
        with pytest.raises(ab.AstroBurstError) as e:
            ab.synth_star_field(field_type=("king_cluster", *par), n_stars=3)
        assert e.value.code == ab._lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError):
        ab.synth_star_field(field_type=(7,), n_stars=3)


def test_config_defaults_equal_the_reference():
    import astroburst_amd as ab
    c = ab.synth_config()
    assert (c.field.width, c.field.height, c.field.n_stars, c.field.flux_min, c.field.flux_max, c.field.seed) == (2048, 2048, 500, 100.0, 50000.0, 42)
    assert c.field_type.kind == ab._lib.AB_SYNTH_FIELD_UNIFORM
    assert (c.psf_type.kind, c.psf_type.fwhm) == (ab._lib.AB_SYNTH_PSF_GAUSSIAN, 3.0)
    n = c.noise
    assert (n.gain, n.readout_noise, n.sky_background, n.dark_current, n.exposure_time, n.bias_level, n.seed) == (1.5, 8.0, 200.0, 0.05, 300.0, 1000.0, 123)
    assert (c.apply_vignette, c.vignette_strength, c.n_frames) == (0, 0.3, 1)
    assert {k: getattr(n, k) for k in R.DEFAULT_NOISE} == R.DEFAULT_NOISE
    assert {k: getattr(c.field, k) for k in R.DEFAULT_FIELD} == R.DEFAULT_FIELD
    ab._lib.lib().ab_synth_config_default(None)   # NULL is ignored


def test_synth_adds_no_environment_variable():
    """the feature reads no environment variable: the release library's list stays the documented eight"""
    from astroburst_amd import _lib
    for name in ("synth.hip", "chacha12.hpp"):
        text = open(os.path.join(_lib.CSRC, name)).read()
        assert "getenv" not in text and "ab_env(" not in text and "ab_dev_env(" not in text, name


# ---- hand-worked cases of the restatement --------------------------------------------------------------------------------------
def test_restatement_one_star_gaussian_by_hand():
    """a star at a pixel centre of a 3 x 3 image: psf_sum = 1 + 4 e1 + 4 e2 with e1 = exp(-inv), e2 = exp(-2 inv)"""
    flux = 1000.0
    img, k = R.render_stars([(1.0, 1.0, 0.0, flux, 5000.0)], ("gaussian", 3.0), 3, 3)
    sigma = 3.0 / 2.3548
    inv = 1.0 / (2.0 * sigma * sigma)
    e1, e2 = math.exp(-1.0 * inv), math.exp(-2.0 * inv)
    s = e2 + e1 + e2 + e1 + 1.0 + e1 + e2 + e1 + e2   # raster order
    want = np.array([[e2, e1, e2], [e1, 1.0, e1], [e2, e1, e2]]) * (flux / s)
    assert np.array_equal(img, want.astype(np.float32)) and (k == 1).all()
    assert abs(float(img.astype(np.float64).sum()) - flux) < 9 * 0.5 * float(np.spacing(np.float32(flux / s)))


def test_restatement_stars_outside_contribute_nothing():
    w, h = 24, 16   # gaussian fwhm 3: psf_r = 6
    for x, y in ((-7.5, 8.0), (31.5, 8.0), (12.0, -7.5), (12.0, 23.5)):
        img, k = R.render_stars([(x, y, 0.0, 1e4, 5000.0)], ("gaussian", 3.0), w, h)
        assert not img.any() and not k.any(), (x, y)
    img, k = R.render_stars([(-5.5, 8.0, 0.0, 1e4, 5000.0)], ("gaussian", 3.0), w, h)   # its window's edge reaches column 0
    assert k[:, 0].any() and not k[:, 2:].any()


def test_restatement_draw_counts():
    p = dict(R.DEFAULT_NOISE, sky_background=0.0, dark_current=0.0, exposure_time=1.0, gain=1.0)
    info = {}
    R.apply_noise(np.array([[0.0, -3.0, np.nan]], np.float32), **p, info=info)   # lambda <= 0 (NaN.max(0) = 0): the read noise's two draws
    assert info["draws_per_pixel"] == [2, 2, 2]
    out = R.apply_noise(np.full((1, 40), 5.0, np.float32), **dict(p, readout_noise=0.0, bias_level=0.0), info=info)   # lambda = 5: Knuth's k + 1 draws + 2
    assert [d - 3 for d in info["draws_per_pixel"]] == [int(v) for v in out[0]]
    assert 2.0 < out.mean() < 8.0
    R.apply_noise(np.full((2, 3), 100.0, np.float32), **p, info=info)     # lambda >= 30: four
    assert info["draws_per_pixel"] == [4] * 6 and info["draws"] == 24


def test_restatement_moments_and_fixture_margins():
    """the fast route's contract needs every Gaussian-branch sample further from a half-integer than the f64 error of the product;
    every noise fixture of tests/test_gpu_synth.py keeps 1e-6"""
    info = {}
    out = R.apply_noise(np.zeros((64, 96), np.float32), **R.DEFAULT_NOISE, info=info)
    assert 4.8e-5 < info["min_margin"] < 5.0e-5 and info["draws"] == 4 * 64 * 96
    lam = 200.0 * 1.5 * 300.0 + 0.05 * 300.0
    assert abs(out.mean() - (lam + 1000.0) / 1.5) < 6 * math.sqrt(lam + 64.0) / 1.5 / math.sqrt(out.size)
    for name, (img, params) in R.noise_fixtures().items():
        info = {}
        R.apply_noise(img, **params, info=info)
        assert info["min_margin"] > 1e-6, (name, info["min_margin"])
        assert info["draws"] == 4 * img.size, name
    info = {}
    R.apply_noise(R.general_route_plane(), **R.GENERAL_PARAMS, info=info)   # the general route's fixture takes every branch
    d = np.array(info["draws_per_pixel"]).reshape(37, 53)
    assert d[5, 7] == 2 and d[20, 3] == 2 and d[0, 0] == 2 and (d[-1] == 4).all() and ((d != 2) & (d != 4)).any() and (d >= 2).all()


def test_restatement_flat_field_and_seeds():
    flat = R.generate_flat_field(7, 5, 1122, 0.3)
    u = R.rng_f64(1122, 0, 35).reshape(5, 7)
    cx, cy = 3.5, 2.5
    r = math.sqrt((6 - cx) ** 2 + (4 - cy) ** 2) / math.sqrt(cx * cx + cy * cy)
    assert flat[4, 6] == np.float32((1.0 - 0.3 * r * r) * (1.0 + u[4, 6] * 0.02 - 0.01))
    assert (R.generate_flat_field(2, 2, 5, 1e9) == np.float32(0.01)).sum() == 3      # the floor (pixel (1, 1) sits on the centre: r = 0)
    img = np.array([[2.0, 3.0, 4.0]], np.float32)
    assert np.array_equal(R.apply_flat_field(img, np.array([[1e-6, 0.0, 0.5]], np.float32)), np.array([[2.0, 3.0, 8.0]], np.float32))
    assert R.flat_seed(123) == 1122 and R.flat_seed(2 ** 64 - 1, 2) == 1000 and R.frame_noise_seed(2 ** 64 - 1, 1) == 7918


def test_noctx_entry_points_refuse_null():
    from astroburst_amd import _lib
    L = _lib.lib()
    assert L.ab_synth_rng_f64(1, 0, 4, None) == _lib.AB_ERR_INVALID
    assert L.ab_synth_star_field(None, None, 0, None) == _lib.AB_ERR_INVALID
    cfg = _lib.SynthConfigC()
    L.ab_synth_config_default(C.byref(cfg))
    n = C.c_size_t(0)
    assert L.ab_synth_star_field(C.byref(cfg), None, 0, C.byref(n)) == _lib.AB_OK and n.value == 500
    assert L.ab_synth_star_field(C.byref(cfg), None, 3, C.byref(n)) == _lib.AB_ERR_INVALID
