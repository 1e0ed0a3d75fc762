"""GPU parity for the star mask and the masked stretch vs the CPU oracle.

Bar: with the detection given (generate_star_mask_from_detection, masked_stretch_with_mask) every
output is bit-exact -- mask, stretched image, iteration count, final background, coverage.  The
end-to-end entry points run the GPU star detection first, whose f64 centroids / FWHM differ from the
BFS-ordered oracle at ~1e-15 relative (see ab_detect_stars): the mask may then differ in a handful of
edge pixels, so those tests bound the mismatch instead (<= 1e-5 of the pixels, values <= 1e-5)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def star_field(rng, rows, cols, n_stars, background=0.02, noise=0.002, fwhm=3.5, amp_hi=0.9):
    img = rng.normal(background, noise, (rows, cols))
    sig = fwhm / 2.3548
    for _ in range(n_stars):
        cy, cx, amp = rng.uniform(8, rows - 8), rng.uniform(8, cols - 8), rng.uniform(0.05, amp_hi)
        y0, y1, x0, x1 = max(int(cy) - 12, 0), int(cy) + 13, max(int(cx) - 12, 0), int(cx) + 13
        yy, xx = np.mgrid[y0:min(y1, rows), x0:min(x1, cols)]
        img[y0:y1, x0:x1] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig))
    return img.clip(1e-5, None).astype(np.float32)


STARS = [(150.3, 100.7, 4.0), (2.1, 3.2, 3.0), (298.9, 198.5, 6.5), (100.0, 50.0, 1.0), (60.0, 60.0, 31.0),
         (-30.0, -30.0, 5.0), (400.0, 100.0, 5.0), (152.0, 103.0, 2.0), (20.5, 180.25, 29.0), (151.0, 101.0, 4.0)]


@pytest.mark.parametrize("protect", [False, True])
@pytest.mark.parametrize("growth,softness", [(2.5, 4.0), (1.0, 0.0), (3.0, 12.5)])
def test_star_mask_from_detection_bit_exact(ctx, oracle, protect, growth, softness):
    rng = np.random.default_rng(0)
    img = rng.uniform(0.0, 1.2, (200, 300)).astype(np.float32)
    img[4, 4] = np.nan
    img[5, 5] = np.inf
    img[6, 6] = -np.inf
    kw = dict(growth_factor=growth, softness=softness, luminance_protect=protect, luminance_ceiling=0.85, stars=STARS)
    want = oracle.generate_star_mask(img, **kw)
    got = ctx.generate_star_mask(img, **kw)
    assert got.stars_masked == want.stars_masked == 8
    assert np.array_equal(got.mask, want.mask)
    assert got.coverage_fraction == want.coverage_fraction


def test_star_mask_no_stars_and_many_stars(ctx, oracle):
    img = np.full((64, 96), 0.5, np.float32)
    got = ctx.generate_star_mask(img, stars=[])
    assert got.stars_masked == 0 and got.coverage_fraction == 0.0 and not got.mask.any()
    rng = np.random.default_rng(2)
    stars = [(rng.uniform(-5, 1030), rng.uniform(-5, 520), rng.uniform(1.0, 12.0)) for _ in range(3000)]
    img = rng.uniform(0, 1, (512, 1024)).astype(np.float32)
    want = oracle.generate_star_mask(img, stars=stars, luminance_protect=True, luminance_ceiling=0.9)
    got = ctx.generate_star_mask(img, stars=stars, luminance_protect=True, luminance_ceiling=0.9)
    assert got.stars_masked == want.stars_masked
    assert np.array_equal(got.mask, want.mask) and got.coverage_fraction == want.coverage_fraction


def result_equal(got, want):
    assert got.iterations_run == want.iterations_run and got.converged == want.converged
    assert got.final_background == want.final_background
    img = got.image.cpu().numpy() if hasattr(got.image, "cpu") else got.image
    assert np.array_equal(img, want.image)
    assert got.stars_masked == want.stars_masked and got.mask_coverage == want.mask_coverage


@pytest.mark.parametrize("rows,cols", [(160, 240), (333, 517), (1024, 1536), (2100, 2000)])
@pytest.mark.parametrize("cfg", [dict(), dict(iterations=3, target_background=0.12, protection_amount=1.0),
                                 dict(iterations=25, target_background=0.4, protection_amount=0.3, convergence_threshold=1e-7)])
def test_masked_stretch_with_mask_bit_exact(ctx, oracle, rows, cols, cfg):
    rng = np.random.default_rng(rows + cols)
    img = star_field(rng, rows, cols, 80)
    img[0, 0] = np.nan
    img[1, 1] = -1.0
    img[2, 2] = np.inf
    stars = [(rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(1.5, 8.0)) for _ in range(60)]
    m_or = oracle.generate_star_mask(img, stars=stars, luminance_protect=True)
    m_gp = ctx.generate_star_mask(img, stars=stars, luminance_protect=True)
    assert np.array_equal(m_or.mask, m_gp.mask)
    result_equal(ctx.masked_stretch(img, mask=m_gp, **cfg), oracle.masked_stretch(img, mask=m_or, **cfg))


def test_masked_stretch_degenerate(ctx, oracle):
    from astroburst_amd.core import StarMaskResult
    flat = np.full((32, 32), 0.5, np.float32)
    zero = np.zeros_like(flat)
    result_equal(ctx.masked_stretch(flat, mask=StarMaskResult(zero, 0, 0.0)),
                 oracle.masked_stretch(flat, mask=oracle.StarMaskResult(zero, 0, 0.0)))
    full = np.ones_like(flat)                                        # everything masked -> bg 0.0, no pixels to select
    img = np.random.default_rng(3).uniform(0.1, 0.9, flat.shape).astype(np.float32)
    result_equal(ctx.masked_stretch(img, mask=StarMaskResult(full, 5, 1.0)),
                 oracle.masked_stretch(img, mask=oracle.StarMaskResult(full, 5, 1.0)))
    result_equal(ctx.masked_stretch(img, iterations=0, mask=StarMaskResult(zero, 0, 0.0)),
                 oracle.masked_stretch(img, iterations=0, mask=oracle.StarMaskResult(zero, 0, 0.0)))


def close_images(got, want):
    bad = got != want
    assert bad.mean() <= 1e-5, f"{bad.sum()} differing pixels"
    assert np.abs(got - want).max() <= 1e-5


def test_end_to_end_mask_and_stretch(ctx, oracle):
    img = star_field(np.random.default_rng(5), 384, 512, 70)
    m_or, m_gp = oracle.generate_star_mask(img), ctx.generate_star_mask(img)
    assert m_gp.stars_masked == m_or.stars_masked > 20
    close_images(m_gp.mask, m_or.mask)
    assert abs(m_gp.coverage_fraction - m_or.coverage_fraction) <= 1e-5
    want, got = oracle.masked_stretch(img), ctx.masked_stretch(img)
    assert got.iterations_run == want.iterations_run and got.converged == want.converged
    assert got.stars_masked == want.stars_masked
    assert abs(got.final_background - want.final_background) <= 1e-6
    close_images(got.image, want.image)


def test_rgb_shared(ctx, oracle):
    import torch
    rng = np.random.default_rng(6)
    base = star_field(rng, 256, 320, 50)
    r, g, b = base, (base * np.float32(0.8)).astype(np.float32), (base * np.float32(1.15)).astype(np.float32)
    g[3, 3] = np.nan
    want = oracle.masked_stretch_rgb_shared(r, g, b)
    got = ctx.masked_stretch_rgb_shared(*[torch.from_numpy(x).cuda() for x in (r, g, b)])
    assert got[3].stars_masked == want[3].stars_masked
    assert abs(got[3].coverage_fraction - want[3].coverage_fraction) <= 1e-5
    for gch, wch in zip(got[:3], want[:3]):
        assert gch.iterations_run == wch.iterations_run and gch.converged == wch.converged
        close_images(gch.image.cpu().numpy(), wch.image)
    with pytest.raises(Exception, match="Channel dimension mismatch"):
        ctx.masked_stretch_rgb_shared(r, g[:-1], b)


def test_full_size_properties(ctx):
    """4096^2: output in [0,1], background lands on the target, masked cores stay below the unmasked stretch."""
    img = star_field(np.random.default_rng(9), 4096, 4096, 600)
    res = ctx.masked_stretch(img)
    assert res.converged and abs(res.final_background - 0.25) < 1e-5
    assert res.stars_masked > 300 and 0.0 < res.mask_coverage < 0.2
    assert float(res.image.min()) >= 0.0 and float(res.image.max()) <= 1.0
    sky = res.image[res.image < 0.5]
    assert abs(float(np.median(sky)) - 0.25) < 0.01


def test_a_large_iteration_ceiling_costs_what_the_loop_runs(ctx, oracle):
    """the device-resident chain used to enqueue six launches for EVERY configured iteration (the reference breaks at
    convergence, masked_stretch.rs:82-91): iterations = 200 000 meant 1.2 M no-op launches per channel.  Iterations are now enqueued
    32 at a time with a look at the loop state in between: same result as the oracle, in a fraction of a second."""
    import time
    rng = np.random.default_rng(77)
    img = star_field(rng, 333, 517, 60)
    stars = [(rng.uniform(0, 517), rng.uniform(0, 333), rng.uniform(1.5, 8.0)) for _ in range(40)]
    m_or = oracle.generate_star_mask(img, stars=stars, luminance_protect=True)
    m_gp = ctx.generate_star_mask(img, stars=stars, luminance_protect=True)
    want = oracle.masked_stretch(img, mask=m_or, iterations=200000)
    # (the loop stops after 3 iterations on this field: the enqueue never reaches its second chunk here.  Loops that do -- running out
    # or stopping by their own decision in the second and third chunk -- are tests/test_gpu_masked_adversarial.py's M-long family)
    assert want.iterations_run < 64
    t0 = time.perf_counter()
    got = ctx.masked_stretch(img, mask=m_gp, iterations=200000)
    assert time.perf_counter() - t0 < 5.0
    result_equal(got, want)
    rgb = [img, (img * np.float32(0.8)).astype(np.float32), (img * np.float32(0.6)).astype(np.float32)]
    t0 = time.perf_counter()
    r, g, b, _ = ctx.masked_stretch_rgb_shared(*rgb, iterations=200000)
    assert time.perf_counter() - t0 < 10.0
    r10, g10, b10, _ = ctx.masked_stretch_rgb_shared(*rgb, iterations=want.iterations_run + 40)
    for a, c in ((r, r10), (g, g10), (b, b10)):
        assert a.iterations_run == c.iterations_run and a.final_background == c.final_background and np.array_equal(np.asarray(a.image), np.asarray(c.image))
