"""GPU drizzle (core/stacking/drizzle.rs, csrc/drizzle.hip) through the C ABI against the numpy restatement (tests/drizzle_restatement.py).

Bar.  Square: weight map and rejected_pixels bit for bit; image bit for bit on every pixel whose survivor sum is exact in f64, within
1 f32 ulp elsewhere.  Most inputs are multiples of 2^-8 below 2^14, so EVERY sum is exact and the whole image is held bit for bit; one
natural-data case exercises the 1-ulp clause.  Gaussian / Lanczos3: the same on all but the "threshold pixels" (a candidate weight within
1e-6 relative of the 1e-12 cut: the device's f64 exp / sin are not glibc's), which may number at most 1e-3 of the output pixels per
case; the weight map is held to 1e-6 relative; rejected_pixels is compared after taking the threshold pixels' counts out.

Measured on one MI355X (every case below): no pixel of any Gaussian / Lanczos3 case lies in the threshold window (share 0.0; the share
is printed in each assertion message), so nothing was left out of any comparison, and all 226 cases hold the bar above."""
import numpy as np
import pytest

import drizzle_restatement as R

pytestmark = pytest.mark.gpu

SETTINGS = [(2.0, 0.7), (1.0, 1.0), (1.5, 0.5), (3.0, 0.9), (4.0, 1.0), (2.5, 0.1)]
FRAME_COUNTS = [2, 3, 5, 16, 32, 33, 64, 200]  # <= 32 frames: lists in LDS; >= 33: the long-list path
KERNELS = [R.SQUARE, R.GAUSSIAN, R.LANCZOS3]


def make_frames(n, rows, cols, seed, ragged=False, natural=False):
    """a smooth scene (so that the MAD clip has something to reject against) + hot pixels + NaN / +-inf pixels; values are multiples
    of 2^-8 below 2^14 unless `natural`: then full-mantissa f32 over some sixty binades"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows + 1, 0:cols + 1]
    scene = 900.0 + 40.0 * np.sin(yy / 3.0) + 30.0 * np.cos(xx / 4.0)
    frames = []
    for k in range(n):
        r, c = (rows + (k % 2), cols + ((k // 2) % 2)) if ragged else (rows, cols)
        f = scene[:r, :c] + rng.normal(0.0, 2.0, (r, c))
        hot = rng.random((r, c)) < 0.03
        f[hot] += rng.uniform(2000.0, 15000.0, int(hot.sum()))
        if natural:  # (f32 samples of one magnitude always sum exactly in f64: it takes ~2^30 between the largest and the smallest)
            f = f * np.exp(rng.normal(0.0, 10.0, (r, c)))
        f = f.astype(np.float32) if natural else (np.round(f * 256.0) / 256.0).astype(np.float32)
        bad = rng.random((r, c))
        f[bad < 0.01] = np.nan
        f[(bad >= 0.01) & (bad < 0.015)] = np.inf
        f[(bad >= 0.015) & (bad < 0.02)] = -np.inf
        frames.append(f)
    return frames


def make_offsets(n, rows, cols, seed):
    """frame 0 at (0, 0); then fractional, integer, negative, partly and wholly off the field, in turn"""
    rng = np.random.default_rng(seed + 1000)
    off = [(0.0, 0.0)]
    for k in range(1, n):
        kind = k % 6
        if kind == 1:
            off.append(tuple(rng.uniform(-3.0, 3.0, 2)))
        elif kind == 2:
            off.append((float(rng.integers(-3, 4)), float(rng.integers(-3, 4))))
        elif kind == 3:
            off.append((-rng.uniform(0.1, 2.0), -rng.uniform(0.1, 2.0)))
        elif kind == 4:
            off.append((cols - rng.uniform(0.5, 4.0), -(rows - rng.uniform(0.5, 4.0))))  # a corner of the frame stays on the field
        elif kind == 5:
            off.append((cols + rng.uniform(1.0, 9.0), rng.uniform(-1.0, 1.0)) if k % 12 == 5 else (rng.uniform(-0.5, 0.5), -(rows + 7.25)))
        else:
            off.append(tuple(rng.uniform(-0.5, 0.5, 2)))
    return off


def ulp_close(a, b):
    return (a == b) | (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64))


def to_np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def compare(got, want, kernel, n_frames, what):
    img, wgt = to_np(got.image), to_np(got.weight_map)
    assert img.shape == want.image.shape == (want.dims[2], want.dims[3]) and img.dtype == np.float32, what
    assert got.input_dims == want.dims[:2] and got.output_dims == want.dims[2:] and got.frame_count == n_frames, what
    assert np.isfinite(img).all() and np.isfinite(wgt).all(), what
    if kernel == R.SQUARE:
        keep = np.ones(img.shape, bool)
        assert np.array_equal(wgt, want.weight), (what, int((wgt != want.weight).sum()))
        assert got.rejected_pixels == want.rejected, (what, got.rejected_pixels, want.rejected)
        share = 0.0
    else:
        thr = want.threshold
        share = float(thr.mean())
        msg = f"{what}: threshold-pixel share {share:.3g}"
        assert share <= 1e-3, msg
        keep = ~thr
        werr = np.abs(wgt.astype(np.float64) - want.weight) <= 1e-6 * np.abs(want.weight)
        assert werr[keep].all(), (msg, int((~werr[keep]).sum()))
        lo = want.rejected - int(want.rejected_map[thr].sum())
        hi = lo + int(thr.sum()) * max(2 * n_frames, 4)
        assert lo <= got.rejected_pixels <= hi, (msg, got.rejected_pixels, lo, hi)
    ex = want.exact & keep
    assert np.array_equal(img[ex], want.image[ex]), (what, share, int((img[ex] != want.image[ex]).sum()), int(ex.sum()))
    rest = keep & ~want.exact
    assert ulp_close(img[rest], want.image[rest]).all(), (what, share)
    return share


def run_case(ctx, frames, offsets, scale, pixfrac, kernel, sl=3.0, sh=3.0, iters=5, what=""):
    want = R.drizzle(frames, offsets, scale, pixfrac, kernel, sl, sh, iters)
    got = ctx.drizzle_frames(frames, offsets, scale, pixfrac, kernel, sl, sh, iters)
    compare(got, want, kernel, len(frames), f"{what} kernel={kernel} scale={scale} pixfrac={pixfrac} n={len(frames)} sl={sl} sh={sh} it={iters}")
    return got, want


@pytest.mark.parametrize("n", FRAME_COUNTS)
@pytest.mark.parametrize("scale,pixfrac", SETTINGS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_against_restatement(ctx, kernel, scale, pixfrac, n):
    rows, cols = (23, 37) if n <= 33 else (11, 21)  # (out dims 23 x 37 .. 92 x 148: never a multiple of the 4 x 64 tile)
    frames = make_frames(n, rows, cols, seed=n)
    _, want = run_case(ctx, frames, make_offsets(n, rows, cols, seed=n), scale, pixfrac, kernel)
    assert want.exact.all()  # the inputs make every sum exact: the whole image was held bit for bit


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_cap_bites_and_rejection_happens(ctx, kernel):
    """the cases above are only worth their name if the cap drops pushes and the clip rejects samples"""
    frames = make_frames(5, 23, 37, seed=5)
    _, want = run_case(ctx, frames, make_offsets(5, 23, 37, seed=5), 1.0, 1.0, kernel)
    assert want.rejected > 0 and (want.counts == 10).any()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [4, 34])
def test_ragged_frames_are_cropped_by_stride(ctx, kernel, n):
    frames = make_frames(n, 23, 37, seed=77, ragged=True)
    assert len({f.shape for f in frames}) == 4
    run_case(ctx, frames, make_offsets(n, 23, 37, seed=77), 2.0, 0.7, kernel, what="ragged")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [6, 40])
def test_natural_data_within_one_ulp(ctx, kernel, n):
    frames = make_frames(n, 23, 37, seed=9, natural=True)
    off = make_offsets(n, 23, 37, seed=9)
    run_case(ctx, frames, off, 2.0, 0.7, kernel, what="natural")
    _, want = run_case(ctx, frames, off, 2.0, 0.7, kernel, iters=0, what="natural, every sample summed")
    assert not want.exact.all()  # (the 1-ulp clause was exercised)


@pytest.mark.parametrize("iters", [0, 1, 5])
@pytest.mark.parametrize("sl,sh", [(3.0, 3.0), (0.0, 0.0), (0.0, 2.0), (float("nan"), 3.0), (3.0, float("nan")), (float("inf"), 1.0), (1.0, float("inf")),
                                   (-1.0, 3.0), (0.5, 0.5)])
@pytest.mark.parametrize("n", [5, 40])
def test_sigma_settings(ctx, n, sl, sh, iters):
    frames = make_frames(n, 13, 22, seed=3)
    off = make_offsets(n, 13, 22, seed=3)
    for kernel in KERNELS:
        run_case(ctx, frames, off, 2.0, 0.7, kernel, sl, sh, iters)


@pytest.mark.parametrize("scale,pixfrac", [(0.3, 0.0), (9.0, 5.0), (-1.0, -2.0), (float("inf"), float("inf"))])
def test_config_outside_the_clamps(ctx, scale, pixfrac):
    frames = make_frames(4, 13, 22, seed=4)
    off = make_offsets(4, 13, 22, seed=4)
    got, want = run_case(ctx, frames, off, scale, pixfrac, R.SQUARE)
    assert got.output_scale == min(max(scale, 1.0), 4.0)


def test_count_zero_and_one_pixels(ctx):
    """pixfrac 0.1 at scale 4: most output pixels receive nothing (0, 0), and with two frames many receive one sample"""
    frames = make_frames(2, 13, 22, seed=6)
    got, want = run_case(ctx, frames, [(0.0, 0.0), (0.37, -0.21)], 4.0, 0.1, R.SQUARE)
    assert (want.counts == 0).any() and (want.counts == 1).any()
    assert (to_np(got.image)[want.counts == 0] == 0).all() and (to_np(got.weight_map)[want.counts == 0] == 0).all()


def test_more_output_rows_than_one_band(ctx):
    """the LDS path enqueues 1024 output rows at a time: 1200 rows cross a band"""
    frames = make_frames(3, 300, 21, seed=8)
    run_case(ctx, frames, [(0.0, 0.0), (0.4, 250.3), (-1.6, -0.7)], 4.0, 1.0, R.SQUARE, what="bands")


def sample_check(frames, offsets, img, wgt, pixels, scale, pixfrac, kernel):
    for oy, ox in pixels:
        s, w = R.gather_pixel(frames, offsets, int(oy), int(ox), scale, pixfrac, kernel)
        v, wv, _, exact = R.finalize_pixel(s, w, 3.0, 3.0, 5)
        assert wgt[oy, ox] == wv, (oy, ox, wgt[oy, ox], wv)
        assert img[oy, ox] == v if exact else ulp_close(np.float32(img[oy, ox]), np.float32(v)), (oy, ox, img[oy, ox], v)


def test_long_lists_over_several_runs(ctx):
    """40 frames (lists of up to 80) on 960 x 1000 output pixels: the long-list path works through the output in runs of 838 656
    pixels; a seeded sample on both sides of the run boundary against the per-pixel gather"""
    import torch
    n, rows, cols = 40, 240, 250
    rng = np.random.default_rng(40)
    frames = [(rng.integers(200 * 256, 300 * 256, (rows, cols)) / 256.0).astype(np.float32) for _ in range(n)]
    for f in frames:
        f[rng.random((rows, cols)) < 0.01] = 9000.0
    off = [(0.0, 0.0)] + [tuple(rng.uniform(-2.0, 2.0, 2)) for _ in range(n - 1)]
    got = ctx.drizzle_frames([torch.from_numpy(f).cuda() for f in frames], off, 4.0, 1.0, "square")
    img, wgt = to_np(got.image), to_np(got.weight_map)
    assert img.shape == (960, 1000) and got.rejected_pixels > 0
    p = np.concatenate([rng.integers(0, 960 * 1000, 300), np.arange(838656 - 20, 838656 + 20), [0, 999, 959 * 1000, 960 * 1000 - 1]])
    sample_check(frames, off, img, wgt, [(int(i) // 1000, int(i) % 1000) for i in p], 4.0, 1.0, R.SQUARE)


def test_host_and_device_planes_and_two_runs_give_the_same_bytes(ctx):
    import torch
    for n, kernel in ((5, "square"), (5, "gaussian"), (36, "lanczos3")):
        frames = make_frames(n, 23, 37, seed=11, ragged=True)
        off = make_offsets(n, 23, 37, seed=11)
        a = ctx.drizzle_frames(frames, off, 2.0, 0.7, kernel)
        b = ctx.drizzle_frames(frames, off, 2.0, 0.7, kernel)
        d = ctx.drizzle_frames([torch.from_numpy(f).cuda() for f in frames], off, 2.0, 0.7, kernel)
        assert isinstance(a.image, np.ndarray) and d.image.is_cuda and d.weight_map.is_cuda
        for other in (b, d):
            assert to_np(other.image).tobytes() == a.image.tobytes() and to_np(other.weight_map).tobytes() == a.weight_map.tobytes()
            assert other.rejected_pixels == a.rejected_pixels
        # a NULL weight plane = not wanted
        c = ctx.drizzle_frames(frames, off, 2.0, 0.7, kernel, want_weight=False)
        assert c.weight_map is None and c.image.tobytes() == a.image.tobytes() and c.rejected_pixels == a.rejected_pixels


def test_errors_and_cancel(ctx):
    import astroburst_amd as ab
    frames = make_frames(3, 13, 22, seed=12)
    off = [(0.0, 0.0)] * 3
    for bad_frames, bad_off in (([], []), (frames[:1], off[:1]), ([frames[0], np.zeros((20, 22), np.float32)], off[:2])):
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.drizzle_frames(bad_frames, bad_off)
        assert e.value.code == ab._lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.drizzle_frames(frames, [(0.0, 0.0), (float("nan"), 0.0), (0.0, 0.0)])
    assert e.value.code == ab._lib.AB_ERR_INVALID and "finite" in str(e.value)
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.drizzle_frames(frames, off, kernel=7)
    assert e.value.code == ab._lib.AB_ERR_INVALID
    with pytest.raises(ab.AstroBurstError) as e:
        ctx.drizzle_frames(frames, off, out=np.zeros((5, 5), np.float32))
    assert e.value.code == ab._lib.AB_ERR_INVALID
    ctx.request_cancel()
    try:
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.drizzle_frames(frames, off)
        assert e.value.code == ab._lib.AB_ERR_CANCELLED
        with pytest.raises(ab.AstroBurstError) as e:
            ctx.drizzle_stack(frames, align=True)
        assert e.value.code == ab._lib.AB_ERR_CANCELLED
    finally:
        ctx.clear_cancel()
    ticks = []
    ctx.set_progress_cb(lambda stage, cur, tot: ticks.append((stage, cur, tot)))
    try:
        ctx.drizzle_frames(frames, off)
    finally:
        ctx.set_progress_cb(None)
    assert any(stage.startswith("drizzle ") for stage, _, _ in ticks), ticks


# ---- drizzle_stack ----------------------------------------------------------------------------------------------------------------
def star_frames(shifts, flat_frame=None, rows=320, cols=384):
    from astroburst_amd import synth
    y, x, flux = synth.star_catalog(rows, cols, 220, seed=5)
    cat = (y, x, flux * 30.0)
    frames = [synth.make_frame(rows, cols, k, cat=cat, shift=s, bad_patch_rate=0.0, cosmic_rate=0.0).numpy() for k, s in enumerate(shifts)]
    if flat_frame is not None:
        frames[flat_frame] = np.full((rows, cols), 1200.0, np.float32)
    return frames


def test_stack_without_alignment_equals_frames_with_zero_offsets(ctx):
    frames = make_frames(6, 23, 37, seed=21, ragged=True)
    for kernel in ("square", "gaussian"):
        a = ctx.drizzle_stack(frames, 2.0, 0.7, kernel, align=False)
        b = ctx.drizzle_frames(frames, [(0.0, 0.0)] * 6, 2.0, 0.7, kernel)
        assert a.offsets == [(0.0, 0.0)] * 6
        assert a.image.tobytes() == b.image.tobytes() and a.weight_map.tobytes() == b.weight_map.tobytes() and a.rejected_pixels == b.rejected_pixels


@pytest.mark.parametrize("method", ["phase_correlation", "zncc"])
def test_stack_with_alignment(ctx, method):
    """offsets = ab_phase_correlate's, or the affine estimate's (tx, ty) where the confidence is below 2.0 and always for Zncc; the
    result = ab_drizzle_frames fed those offsets, byte for byte.  The low-confidence branch is forced with a CONSTANT frame
    (is_constant_or_zero, phase_correlation.rs:42-48: confidence 0); pure noise does not do it -- the peak of a noise surface stands
    ~8.7 sigma above its mean (tests/phasecorr_restatement.py on N(1200, 15) against this star field), far above the 2.0 threshold."""
    frames = star_frames([(0.0, 0.0), (2.5, -1.75), (-0.6, 3.3), (0.0, 0.0)], flat_frame=3)
    got = ctx.drizzle_stack(frames, 2.0, 0.7, "square", align=True, alignment_method=method, num_threads=8)
    assert got.offsets[0] == (0.0, 0.0)
    low = 0
    for k in range(1, 4):
        dx, dy, conf = ctx.phase_correlate(frames[0], frames[k])
        if method == "zncc" or conf < 2.0:
            t = ctx.align_channel_affine(frames[0], frames[k], num_threads=8).transform
            want = (t[2], t[5])
            low += conf < 2.0
        else:
            want = (dx, dy)
        assert got.offsets[k] == want, (k, got.offsets[k], want, conf)
    assert low >= 1  # the constant frame did take the low-confidence branch
    assert got.offsets[1] != (0.0, 0.0) and got.offsets[2] != (0.0, 0.0), got.offsets  # (not a comparison of zeros with zeros)
    if method == "zncc":  # (the star matcher finds the shifts to a fraction of a pixel; how close ab_phase_correlate comes is its own tests' subject)
        assert abs(abs(got.offsets[1][0]) - 1.75) < 0.3 and abs(abs(got.offsets[1][1]) - 2.5) < 0.3, got.offsets
    again = ctx.drizzle_frames(frames, got.offsets, 2.0, 0.7, "square")
    assert again.image.tobytes() == got.image.tobytes() and again.weight_map.tobytes() == got.weight_map.tobytes()
    assert again.rejected_pixels == got.rejected_pixels


# ---- full size --------------------------------------------------------------------------------------------------------------------
def test_full_size_10_frames_4096(ctx):
    """10 x 4096^2 at scale 2 / pixfrac 0.7 / Square (the reference's default and its paper's example): a seeded sample of 4096
    output pixels, a quarter of them on the four borders, against the per-pixel gather"""
    import torch
    n, size = 10, 4096
    g = torch.Generator().manual_seed(10)
    frames = [(torch.randint(200 * 256, 300 * 256, (size, size), generator=g, dtype=torch.int32).float() / 256.0) for _ in range(n)]
    for f in frames:
        f[torch.rand((size, size), generator=g) < 0.002] = 12000.0
        f[torch.rand((size, size), generator=g) < 0.0005] = float("nan")
    rng = np.random.default_rng(10)
    off = [(0.0, 0.0)] + [tuple(rng.uniform(-4.0, 4.0, 2)) for _ in range(n - 1)]
    got = ctx.drizzle_frames([f.cuda() for f in frames], off, 2.0, 0.7, "square")
    img, wgt = got.image.cpu().numpy(), got.weight_map.cpu().numpy()
    o = 2 * size
    assert img.shape == (o, o) and got.rejected_pixels > 0
    inner = [(int(a), int(b)) for a, b in rng.integers(0, o, (3072, 2))]
    edge = [(0, int(v)) for v in rng.integers(0, o, 256)] + [(o - 1, int(v)) for v in rng.integers(0, o, 256)]
    edge += [(int(v), 0) for v in rng.integers(0, o, 256)] + [(int(v), o - 1) for v in rng.integers(0, o, 252)]
    edge += [(0, 0), (0, o - 1), (o - 1, 0), (o - 1, o - 1)]
    sample_check([f.numpy() for f in frames], off, img, wgt, inner + edge, 2.0, 0.7, R.SQUARE)
