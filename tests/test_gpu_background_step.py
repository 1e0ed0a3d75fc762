"""The compose wizard's background step on the GPU (csrc/wizard_background.hip): ab_background_step and
ab_auto_stretch_preview_sampled, each case against two references.

Reference 1, the library's own unfused chain -- ab_extract_background, ab_auto_stretch_preview of each plane, the pick in numpy --
compared with ==: planes as bit patterns, bytes, sample_count, coeffs, both statistics and both STFs; the means alone to 1e-12
relative, the bar of tests/test_gpu_stats_stf.py (ab_auto_stretch_preview may take the register-resident statistics kernel, whose sum
has another order).

Reference 2, tests/background_step_restatement.py out of the oracle: tests/test_gpu_background.py's bar for the extraction (planes and
coefficients bit-exact, rms to 1e-12 relative), tests/test_gpu_stats_stf.py's for the statistics, the STF and the bytes (== but the
mean, 1e-12 relative).

Every non-error case was run through the oracle on the CPU first: each yields enough samples, and both ramps' models have pixels that
are not > 1e-7 (96 x 96: 2 671 of 9 216; 2001 x 2003: 1 118 299 of 4 008 003)."""
import ctypes as C

import numpy as np
import pytest

import background_step_restatement as R
from astroburst_amd import AstroBurstError, _lib
from test_gpu_background import sky

pytestmark = pytest.mark.gpu
F32 = np.float32


def ramp(rows, cols):
    """a third of the frame empty (zeros: cells skipped), the rest a steep ramp along x with a tilt along y: the fitted plane
    extrapolates below zero over the empty part"""
    rng = np.random.default_rng(rows)
    y, x = np.mgrid[0:rows, 0:cols]
    img = (x - 0.31 * cols) * (96.0 / cols) + 6.0 * y / rows + rng.normal(0, 0.05, (rows, cols))
    img[:, : cols // 3] = 0.0
    return img.astype(F32)


CASES = {   # name: (rows, cols, grid, degree, image builder)
    "64": (64, 64, 4, 1, lambda: sky(np.random.default_rng(64 * 31 + 64), 64, 64)),
    "301x517": (301, 517, 8, 3, lambda: sky(np.random.default_rng(301 * 31 + 517), 301, 517, zeros=True)),
    "257x130-deg0": (257, 130, 32, 0, lambda: sky(np.random.default_rng(257 * 31 + 130), 257, 130)),
    "2001x2003": (2001, 2003, 8, 2, lambda: sky(np.random.default_rng(2001), 2001, 2003)),
    "ramp96": (96, 96, 6, 1, lambda: ramp(96, 96)),
    "ramp2001x2003": (2001, 2003, 6, 1, lambda: ramp(2001, 2003)),     # the known range above the threshold with invalid model pixels
}
MODES = {"subtract": 0, "divide": 1}
_images, _chain, _restated = {}, {}, {}


def image(case):
    if case not in _images:
        _images[case] = CASES[case][4]()
        _images[case].setflags(write=False)
    return _images[case]


def kw(case):
    _, _, grid, degree, _ = CASES[case]
    return dict(grid_size=grid, poly_degree=degree, sigma_clip=2.5, iterations=3)


def chain(ctx, case, mode):
    """reference 1 at full size: (BackgroundResult on the host, {plane: (u8 of every pixel, stats, stf)})"""
    import torch
    if (case, mode) not in _chain:
        bg = ctx.extract_background(dev_plane(image(case)), mode=mode, **kw(case))
        prev = {}
        for name, plane in (("corrected", bg.corrected), ("model", bg.model)):
            u8, st, stf = ctx.auto_stretch_preview(plane)
            prev[name] = (u8.cpu().numpy(), st, stf)
        bg.corrected, bg.model = bg.corrected.cpu().numpy(), bg.model.cpu().numpy()
        _chain[(case, mode)] = (bg, prev)
    return _chain[(case, mode)]


def restated(oracle, case, mode):
    """reference 2 at full size (max_dim = the larger dim: the pick is applied per test)"""
    if (case, mode) not in _restated:
        rows, cols = CASES[case][:2]
        _restated[(case, mode)] = R.background_step(oracle, image(case), mode=MODES[mode], max_dim=max(rows, cols), **kw(case))
    return _restated[(case, mode)]


def pick(u8, max_dim):
    rows, cols = u8.shape
    dst_w, dst_h = R.pick_dims(cols, rows, max_dim)
    if (dst_h, dst_w) == (rows, cols):
        return u8
    return u8[np.ix_(R.pick_indices(rows, dst_h), R.pick_indices(cols, dst_w))]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def dev_plane(a, off=0):
    """a device plane that starts `off` floats into its allocation"""
    import torch
    buf = torch.empty(a.size + off, dtype=torch.float32, device="cuda")
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))     # (a copy: the cached images are read-only)
    return v


def dev_empty(shape, off=0):
    import torch
    n = int(np.prod(shape))
    return torch.full((n + off,), -7.0, dtype=torch.float32, device="cuda")[off:off + n].view(shape)


def dev_bytes(n, off=0):
    import torch
    return torch.full((n + off + 8,), 0xAB, dtype=torch.uint8, device="cuda")[off:off + n]


def same_stats(got, want, exact_mean=False):
    assert got.valid_count == want.valid_count
    assert got.min == want.min and got.max == want.max
    assert got.median == want.median, (got.median, want.median)
    assert got.mad == want.mad and got.sigma == want.sigma
    if exact_mean:
        assert got.mean == want.mean
    else:
        assert abs(got.mean - want.mean) <= 1e-12 * abs(want.mean)


def same_stf(got, want):
    assert (got.shadow, got.midtone, got.highlight) == (want.shadow, want.midtone, want.highlight)


def check_step(ctx, oracle, got, case, mode, max_dim, model=True, corrected_u8=True, model_u8=True):
    rows, cols = CASES[case][:2]
    bg, prev = chain(ctx, case, mode)
    want = restated(oracle, case, mode)
    dst_w, dst_h = R.pick_dims(cols, rows, max_dim)
    assert (got.rows, got.cols, got.preview_rows, got.preview_cols) == (rows, cols, dst_h, dst_w)
    # reference 1: ==
    assert got.sample_count == bg.sample_count and np.array_equal(got.coeffs, bg.coeffs) and got.rms_residual == bg.rms_residual
    assert np.array_equal(bits(host(got.corrected)), bits(bg.corrected))
    if model:
        assert np.array_equal(bits(host(got.model)), bits(bg.model))
    else:
        assert got.model is None
    for name, u8, st, stf, on in (("corrected", got.corrected_u8, got.corrected_stats, got.corrected_stf, corrected_u8),
                                  ("model", got.model_u8, got.model_stats, got.model_stf, model_u8)):
        same_stats(st, prev[name][1])
        same_stf(stf, prev[name][2])
        if on:
            assert host(u8).shape == (dst_h, dst_w) and np.array_equal(host(u8).reshape(dst_h, dst_w), pick(prev[name][0], max_dim)), name
        else:
            assert u8 is None
    # reference 2
    assert got.sample_count == want.sample_count and np.array_equal(got.coeffs, want.coeffs)
    assert got.rms_residual == pytest.approx(want.rms_residual, rel=1e-12, abs=1e-300)
    assert np.array_equal(host(got.corrected), want.corrected, equal_nan=True)
    if model:
        assert np.array_equal(host(got.model), want.model, equal_nan=True)
    same_stats(got.corrected_stats, want.corrected_stats)
    same_stats(got.model_stats, want.model_stats)
    same_stf(got.corrected_stf, want.corrected_stf)
    same_stf(got.model_stf, want.model_stf)
    if corrected_u8:
        assert np.array_equal(host(got.corrected_u8), pick(want.corrected_u8, max_dim))
    if model_u8:
        assert np.array_equal(host(got.model_u8), pick(want.model_u8, max_dim))


STEP = [("64", "subtract", 4096), ("64", "divide", 4096),
        ("301x517", "subtract", 4096), ("301x517", "subtract", 128), ("301x517", "subtract", 1),
        ("301x517", "divide", 4096), ("301x517", "divide", 128), ("301x517", "divide", 1),
        ("257x130-deg0", "subtract", 4096), ("257x130-deg0", "subtract", 100),
        ("2001x2003", "subtract", 4096), ("2001x2003", "subtract", 512),
        ("ramp96", "subtract", 4096), ("ramp96", "divide", 4096), ("ramp96", "subtract", 40),
        ("ramp2001x2003", "subtract", 512)]


@pytest.mark.parametrize("case,mode,max_dim", STEP, ids=[f"{c}-{m}-{d}" for c, m, d in STEP])
def test_step_is_the_chain_and_the_restatement(ctx, oracle, case, mode, max_dim):
    got = ctx.background_step(dev_plane(image(case)), mode=mode, max_dim=max_dim, **kw(case))
    check_step(ctx, oracle, got, case, mode, max_dim)


@pytest.mark.parametrize("max_dim", [4096, 128, 1])
@pytest.mark.parametrize("plane_off,byte_off", [(0, 3), (1, 0), (1, 3)])
def test_step_at_unaligned_addresses(ctx, oracle, max_dim, plane_off, byte_off):
    """301 x 517 (columns no multiple of 4): planes one float and bytes three bytes into their allocations"""
    case, (rows, cols) = "301x517", CASES["301x517"][:2]
    dst_w, dst_h = R.pick_dims(cols, rows, max_dim)
    cu8, mu8 = dev_bytes(dst_h * dst_w, byte_off), dev_bytes(dst_h * dst_w, byte_off)
    got = ctx.background_step(dev_plane(image(case), plane_off), max_dim=max_dim, out_corrected=dev_empty((rows, cols), plane_off),
                              out_model=dev_empty((rows, cols), plane_off), out_corrected_u8=cu8, out_model_u8=mu8, **kw(case))
    got.corrected_u8, got.model_u8 = cu8.view(dst_h, dst_w), mu8.view(dst_h, dst_w)
    check_step(ctx, oracle, got, case, "subtract", max_dim)


def test_degenerate_range_of_a_constant_model(ctx, oracle):
    """degree 0: min == max, the statistics fall back to their own scan (stats.rs:36-38)"""
    got = ctx.background_step(dev_plane(image("257x130-deg0")), **kw("257x130-deg0"))
    m = host(got.model)
    assert m.min() == m.max() and got.model_stats.min == got.model_stats.max == float(m[0, 0]) and got.model_stats.valid_count == m.size
    assert got.model_stats.mad == 0.0


@pytest.mark.parametrize("case", ["ramp96", "ramp2001x2003"])
@pytest.mark.parametrize("mode", ["subtract", "divide"])
def test_model_that_crosses_zero(ctx, oracle, case, mode):
    """the model's pixels that are not > 1e-7: zero bytes in its preview, left out of valid_count and of the range"""
    max_dim = 4096 if case == "ramp96" else 512
    got = ctx.background_step(dev_plane(image(case)), mode=mode, max_dim=max_dim, **kw(case))
    m = host(got.model)
    valid = np.isfinite(m) & (m > F32(1e-7))
    assert 0 < int(valid.sum()) < m.size and (m <= 0).any()
    assert got.model_stats.valid_count == int(valid.sum())
    assert got.model_stats.min == float(m[valid].min()) > 0.0 and got.model_stats.max == float(m[valid].max())
    assert not host(got.model_u8)[pick(~valid, max_dim)].any() and host(got.model_u8)[pick(valid, max_dim)].any()
    if mode == "divide":            # |bg| <= 1e-10 keeps the pixel (background.rs:370-376); the two references hold every other pixel
        keep = np.abs(m) <= F32(1e-10)
        assert np.array_equal(bits(host(got.corrected)[keep]), bits(image(case)[keep]))
    check_step(ctx, oracle, got, case, mode, max_dim)


def test_without_a_model_plane(ctx, oracle):
    got = ctx.background_step(dev_plane(image("301x517")), max_dim=128, want_model=False, **kw("301x517"))
    check_step(ctx, oracle, got, "301x517", "subtract", 128, model=False)


@pytest.mark.parametrize("which", ["corrected", "model", "neither"])
def test_each_preview_output_is_optional(ctx, oracle, which):
    on = dict(corrected_u8=which == "corrected", model_u8=which == "model")
    got = ctx.background_step(dev_plane(image("64")), mode="divide", want_corrected_u8=on["corrected_u8"], want_model_u8=on["model_u8"], **kw("64"))
    check_step(ctx, oracle, got, "64", "divide", 4096, **on)


@pytest.mark.parametrize("max_dim", [4096, 128])
def test_host_planes(ctx, oracle, max_dim):
    got = ctx.background_step(image("301x517"), mode="divide", max_dim=max_dim, **kw("301x517"))
    assert all(isinstance(x, np.ndarray) for x in (got.corrected, got.model, got.corrected_u8, got.model_u8))
    check_step(ctx, oracle, got, "301x517", "divide", max_dim)


def test_without_info_the_outputs_are_the_same(ctx, oracle):
    import torch
    got = ctx.background_step(dev_plane(image("301x517")), max_dim=128, fetch=False, **kw("301x517"))
    torch.cuda.synchronize()
    bg, prev = chain(ctx, "301x517", "subtract")
    assert got.sample_count is None and got.corrected_stats is None
    assert np.array_equal(bits(host(got.corrected)), bits(bg.corrected)) and np.array_equal(bits(host(got.model)), bits(bg.model))
    assert np.array_equal(host(got.corrected_u8), pick(prev["corrected"][0], 128)) and np.array_equal(host(got.model_u8), pick(prev["model"][0], 128))


# ---- ab_auto_stretch_preview_sampled alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dim", [4096, 128, 1])
@pytest.mark.parametrize("where", ["device", "device+1+3", "host"])
def test_sampled_preview_is_the_preview_at_the_picked_pixels(ctx, oracle, max_dim, where):
    img = image("301x517")
    rows, cols = img.shape
    dst_w, dst_h = R.pick_dims(cols, rows, max_dim)
    full, st, stf = ctx.auto_stretch_preview(dev_plane(img))
    out = dev_bytes(dst_h * dst_w, 3) if where == "device+1+3" else None
    src = img if where == "host" else dev_plane(img, 1 if where == "device+1+3" else 0)
    u8, gst, gstf = ctx.auto_stretch_preview_sampled(src, max_dim=max_dim, out=out)
    assert isinstance(u8, np.ndarray) == (where == "host")
    assert np.array_equal(host(u8).reshape(dst_h, dst_w), pick(full.cpu().numpy(), max_dim))
    same_stats(gst, st)
    same_stf(gstf, stf)
    wu8, wst, wstf = R.preview_sampled(oracle, img, max_dim)
    assert np.array_equal(host(u8).reshape(dst_h, dst_w), wu8)
    same_stats(gst, wst)
    same_stf(gstf, wstf)


def test_sampled_preview_without_a_fetch_and_with_a_config(ctx, oracle):
    import torch
    img = image("301x517")
    u8, st, stf = ctx.auto_stretch_preview_sampled(dev_plane(img), max_dim=128, fetch=False)
    torch.cuda.synchronize()
    assert st is None and stf is None and np.array_equal(host(u8), R.preview_sampled(oracle, img, 128)[0])
    u8, st, stf = ctx.auto_stretch_preview_sampled(dev_plane(img), max_dim=128, target_bg=0.1, shadow_k=-1.5)
    full, fst, fstf = ctx.auto_stretch_preview(dev_plane(img), target_bg=0.1, shadow_k=-1.5)
    same_stf(stf, fstf)
    same_stf(stf, oracle.auto_stf(oracle.compute_image_stats(img), 0.1, -1.5))
    assert np.array_equal(host(u8), pick(full.cpu().numpy(), 128))


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def _raw_step(ctx, img, cfg, max_dim, corr, model, cu8, mu8, dev, info=None):
    ctx._check(ctx._L.ab_background_step(ctx._h, img, cfg, max_dim, corr, model, cu8, mu8, dev, info))


def test_errors_leave_the_context_usable(ctx, oracle):
    a = np.ones((64, 64), F32)
    o, m = np.zeros((64, 64), F32), np.zeros((64, 64), F32)
    by = np.zeros(64 * 64 * 2, np.uint8)
    P = lambda arr, r=64, c=64: C.byref(_lib.Plane(C.c_void_p(arr.ctypes.data), r, c, 0))  # noqa: E731
    cfg = C.byref(_lib.BackgroundConfigC(4, 1, 2.5, 3, 0))
    b0, b1 = C.c_void_p(by.ctypes.data), C.c_void_p(by.ctypes.data + 4096)
    # the reference's own error (background.rs:71-77), matched on its first 30 characters
    zeros = np.zeros((64, 64), F32)
    try:
        oracle.extract_background(zeros, 4, 1, 2.5, 3, 0)
        raise AssertionError("the oracle accepted an empty image")
    except ValueError as e:
        assert str(e).startswith("Not enough background samples")
        with pytest.raises(AstroBurstError, match=str(e)[:30].replace("(", r"\(")):
            ctx.background_step(zeros, grid_size=4, poly_degree=1)
    with pytest.raises(AstroBurstError, match="Image too small for grid_size=8"):
        ctx.background_step(np.ones((16, 16), F32), grid_size=8)
    with pytest.raises(AstroBurstError, match="poly_degree"):
        ctx.background_step(a, poly_degree=6)
    # arguments, before anything touches the device
    for args, msg in (((None, cfg, 4096, P(o), None, b0, b1, 0), "null image plane"),
                      ((P(a), None, 4096, P(o), None, b0, b1, 0), "null configuration"),
                      ((P(a), cfg, 4096, None, None, b0, b1, 0), "null corrected plane"),
                      ((P(a), cfg, 4096, P(o, 64, 63), None, b0, b1, 0), "the corrected plane must be 64 x 64"),
                      ((P(a), cfg, 4096, P(o), P(m, 32, 128), b0, b1, 0), "the model plane must be 64 x 64"),
                      ((P(a, 65536, 32768), cfg, 4096, P(o, 65536, 32768), None, None, None, 0), "2\\^31 pixels or more"),
                      ((P(a), cfg, 0, P(o), None, b0, b1, 0), "max_dim must be >= 1"),
                      ((P(a), cfg, -5, P(o), None, b0, b1, 0), "max_dim must be >= 1"),
                      ((P(a), cfg, 4096, P(a), None, b0, b1, 0), "an output overlaps an input"),
                      ((P(a), cfg, 4096, P(o), P(o), b0, b1, 0), "two outputs overlap"),
                      ((P(a), cfg, 4096, P(o), P(m), b0, C.c_void_p(by.ctypes.data + 4095), 0), "two outputs overlap"),
                      ((P(a), cfg, 4096, P(o), None, C.c_void_p(a.ctypes.data + 5), None, 0), "an output overlaps an input")):
        with pytest.raises(AstroBurstError, match=msg):
            _raw_step(ctx, *args)
    assert not o.any() and not m.any() and not by.any()
    st, stf = _lib.ImageStatsC(), _lib.StfParamsC()
    L, h = ctx._L, ctx._h
    for args, msg in (((None, None, 4096, b0, 0), "null image plane"), ((P(a), None, 4096, None, 0), "null output bytes"),
                      ((P(a), None, 0, b0, 0), "max_dim must be >= 1"), ((P(a, 65536, 32768), None, 4096, b0, 0), "2\\^31 pixels or more"),
                      ((P(a), None, 4096, C.c_void_p(a.ctypes.data + 16380), 0), "an output overlaps an input")):
        with pytest.raises(AstroBurstError, match=msg):
            ctx._check(L.ab_auto_stretch_preview_sampled(h, *args, C.byref(st), C.byref(stf)))
    assert not by.any()
    # one good call after them
    got = ctx.background_step(dev_plane(image("64")), **kw("64"))
    check_step(ctx, oracle, got, "64", "subtract", 4096)
