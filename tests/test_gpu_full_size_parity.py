"""BASELINE.json's sizes against the CPU ORACLE, whole planes: what test_gpu_full_size.py holds through properties only.

  warp / shift / resample   4096 x 4096 (8 pieces of 512 columns per row: no re-deal), 4096 x 4100 (9), 13 759 x 12 451 (25: the
                            form C3 runs), a registration-like transform and a 3 degree one; the row-band form at C3 size; bit for bit
  registration              4096^2 at the bench's star density (reference + 5 targets through register_frames) and the C3 pair of
                            test_c3_star_align_leg_at_nircam_size: method, matched stars, inliers equal to the oracle's, coefficients
                            within 1e-8 (the bar of test_gpu_detect_affine.py), then the warped plane bit for bit
  C5 at 8192^2              statistics, background, masked stretch (own and shared mask), SCNR, SPCC at the bars of the small tests
  C3 statistics             compute_image_stats + auto_stf + apply_stf of the 171 Mpix warped plane

Inputs come from astroburst_amd.synth with fixed seeds, on the device, and are copied to the host once for the oracle.  Every warp
output is pre-filled with a sentinel; a failure names the first differing (y, x), its piece and the pixels never written.

The 64-frame stack is not here: its oracle does need minutes (test_gpu_full_size.py keeps its crops).

Measured on an MI355X machine (16 CPUs for the oracle): `pytest -m gpu` over the whole suite 456 s, of which this file 72 s and
test_gpu_resample_shapes.py 6 s -- 378 s without the two, so they add 21 %, under the third they were allowed; nothing was dropped.
The oracle at C3 size: align_channel_affine 15.8 s, compute_image_stats 2.2 s, warp_image 0.40 s, shift_image_subpixel 0.44 s,
apply_stf 0.04 s; at 8192^2: masked_stretch_rgb_shared 16.7 s, masked_stretch 7.0 s, spcc_calibrate_rgb 3.8 s, extract_background
2.3 s; align_channel_affine at 4096^2 2.1 - 2.2 s per pair.  Every registration here came out EQUAL to the oracle's in all six
coefficients (difference 0.0), C3 included: the 1e-8 bar was not needed, let alone widened."""
import math
import time

import numpy as np
import pytest

from test_gpu_resample_shapes import SENTINEL, assert_same

pytestmark = pytest.mark.gpu

C3 = (13759, 12451)


@pytest.fixture
def tctx(ctx):
    """the session context on torch's current stream (the planes are produced by torch kernels)"""
    ctx.use_torch_stream()
    yield ctx
    import torch
    torch.cuda.synchronize()
    ctx.use_own_stream()


def timed(label, fn):
    """the oracle's calls are what this file costs: print each (visible with -s / on failure)"""
    t0 = time.perf_counter()
    out = fn()
    print(f"[oracle time] {label}: {time.perf_counter() - t0:.2f} s", flush=True)
    return out


def rigid(deg, tx, ty, rows, cols):
    """output (x, y) -> source: rotation by deg about the frame's centre + (tx, ty)"""
    a = math.radians(deg)
    ca, sa = math.cos(a), math.sin(a)
    cx, cy = (cols - 1) / 2.0, (rows - 1) / 2.0
    return (ca, -sa, cx - ca * cx + sa * cy + tx, sa, ca, cy - sa * cx - ca * cy + ty)


def star_frame(rows, cols, k, cat, T=None, **kw):
    """frame k of a field seen through T (a star at reference (x, y) lands at T(x, y)), as bench.py makes its frames"""
    from astroburst_amd import synth
    y, x, flux = cat
    if T is not None:
        y, x = T[3] * x + T[4] * y + T[5], T[0] * x + T[1] * y + T[2]
    import torch
    deterministic = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)                           # (index_add_ over overlapping patches: the same frame every run)
    try:
        truth = 200.0 + synth.render_stars(rows, cols, (y, x, flux), device="cuda")
    finally:
        torch.use_deterministic_algorithms(deterministic)
    return synth.make_frame(rows, cols, k, device="cuda", truth=truth, **kw)


def whole_warp_equals_oracle(ctx, oracle, dev, host, T, what):
    import torch
    rows, cols = host.shape
    got = ctx.warp_image(dev, T, rows, cols, out=torch.full((rows, cols), SENTINEL, device="cuda"))
    want = timed(f"warp_image {rows} x {cols} {what}", lambda: oracle.warp_image(host, T, rows, cols))
    assert_same(got, want, 512, f"warp {rows} x {cols} ({(cols + 511) // 512} pieces per row) {what}")
    assert (want != 0.0).mean() > 0.9                                  # (the oracle's plane: the transform keeps the frame in view)
    return got, want


# ---- warp / shift / resample ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="class")
def c3_frame():
    """one 171 Mpix frame with stars, cosmic rays and NaN patches, on the device and on the host; freed after TestC3Plane"""
    import torch
    from astroburst_amd import synth
    rows, cols = C3
    y, x, flux = synth.star_catalog(rows, cols, 6000, seed=31)
    dev = star_frame(rows, cols, 1, (y, x, flux * 60.0))
    pair = [dev, dev.cpu().numpy()]
    del dev
    yield pair
    pair.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rows,cols", [(4096, 4096), (4096, 4100)])
def test_whole_plane_warp_at_8_and_9_pieces_per_row(tctx, oracle, rows, cols):
    from astroburst_amd import synth
    y, x, flux = synth.star_catalog(rows, cols, 2000, seed=cols)
    dev = star_frame(rows, cols, 1, (y, x, flux * 25.0))
    host = dev.cpu().numpy()
    assert np.isnan(host).any()                                        # NaN patches go through the taps like any value
    for what, T in (("0.02 deg + (5.5, -3.25)", rigid(0.02, 5.5, -3.25, rows, cols)), ("3 deg", rigid(3.0, 5.5, -3.25, rows, cols))):
        whole_warp_equals_oracle(tctx, oracle, dev, host, T, what)


class TestC3Plane:
    """one 13 759 x 12 451 frame: 25 pieces of 512 columns per row, 49 of 256"""

    def test_whole_plane_warp_at_c3_size_25_pieces_per_row(self, tctx, oracle, c3_frame):
        dev, host = c3_frame
        whole_warp_equals_oracle(tctx, oracle, dev, host, rigid(0.02, 5.5, -3.25, *C3), "0.02 deg + (5.5, -3.25)")

    def test_whole_plane_warp_at_c3_size_3_degrees(self, tctx, oracle, c3_frame):
        dev, host = c3_frame
        whole_warp_equals_oracle(tctx, oracle, dev, host, rigid(3.0, 5.5, -3.25, *C3), "3 deg")

    def test_row_bands_at_c3_size_reassemble_to_the_whole_warp(self, tctx, c3_frame):
        """eight bands of output rows, each from the band of SOURCE rows warp_source_rows names (the row-band scheme's ingest):
        reassembled, the whole warp -- whose equality with the oracle is the test above"""
        import torch
        ctx = tctx
        dev, _ = c3_frame
        rows, cols = C3
        T = rigid(0.02, 5.5, -3.25, rows, cols)
        whole = ctx.warp_image(dev, T, rows, cols)
        out = torch.full((rows, cols), SENTINEL, device="cuda")
        for g in range(8):
            row0, row1 = g * rows // 8, (g + 1) * rows // 8
            s0, sn = ctx.warp_source_rows(T, rows, cols, cols, row0, row1 - row0)
            assert 0 < sn < rows // 8 + 64                                 # a band + its halo, not the frame
            ctx.warp_image_rows_from_band(dev[s0:s0 + sn], s0, rows, T, rows, row0, out[row0:row1])
        assert_same(out, whole.cpu().numpy(), 512, "eight row bands at 13 759 x 12 451")

    def test_shift_at_c3_size(self, tctx, oracle, c3_frame):
        import torch
        dev, host = c3_frame
        got = tctx.shift_image_subpixel(dev, -3.25, 5.5, out=torch.full(C3, SENTINEL, device="cuda"))
        want = timed("shift_image_subpixel 13 759 x 12 451", lambda: oracle.shift_image_subpixel(host, -3.25, 5.5))
        assert_same(got, want, 256, "shift 13 759 x 12 451 (49 pieces per row)")

    def test_statistics_and_stf_of_the_c3_warped_plane(self, tctx, oracle, c3_frame):
        from test_gpu_stats_stf import check_stats
        ctx = tctx
        dev, _ = c3_frame
        warped = ctx.warp_image(dev, rigid(0.02, 5.5, -3.25, *C3), *C3)
        host = warped.cpu().numpy()
        wst = timed("compute_image_stats 13 759 x 12 451", lambda: oracle.compute_image_stats(host))
        st = ctx.compute_image_stats(warped)
        check_stats(st, wst)
        p, wp = ctx.auto_stf(st), oracle.auto_stf(wst)
        assert (p.shadow, p.midtone, p.highlight) == (wp.shadow, wp.midtone, wp.highlight)
        want = timed("apply_stf 13 759 x 12 451", lambda: oracle.apply_stf(host, wp, wst))
        assert np.array_equal(ctx.apply_stf(warped, p, st).cpu().numpy(), want)


@pytest.mark.parametrize("src,dst", [((8192, 8192), (4096, 6000)), ((1600, 1600), (4096, 4096))])
def test_resample_at_size(tctx, oracle, src, dst):
    import torch
    from astroburst_amd import synth
    dev = synth.make_frame(src[0], src[1], 2, device="cuda")
    host = dev.cpu().numpy()
    got = tctx.resample_image(dev, *dst, out=torch.full(dst, SENTINEL, device="cuda"))
    want = timed(f"resample_image {src} -> {dst}", lambda: oracle.resample_image(host, *dst))
    assert_same(got, want, 256, f"resample {src} -> {dst}")


# ---- registration ------------------------------------------------------------------------------------------------------------------
def registration_equals_oracle(ctx, oracle, ref, targets, names):
    """register_frames against oracle.align_channel_affine pair by pair, on the default chain (no frame redone), and the warp
    with the library's own transform against the oracle's warp with that same transform"""
    rows, cols = ref.shape
    ref_h = ref.cpu().numpy()
    before = ctx.fallback_counts()
    got = ctx.register_frames(ref, targets, num_threads=8)
    after = ctx.fallback_counts()
    assert (after["frames_redone"], after["tile_slots"]) == (before["frames_redone"], before["tile_slots"]), (before, after)
    for name, t, g in zip(names, targets, got):
        t_h = t.cpu().numpy()
        want = timed(f"align_channel_affine {rows} x {cols} [{name}]", lambda: oracle.align_channel_affine(ref_h, t_h, num_threads=8))
        print(f"[registration] {name}: library {g}\n[registration] {name}: oracle  {want}\n[registration] {name}: max |coefficient difference| "
              f"{np.abs(np.array(g.transform) - np.array(want.transform)).max():.3e}", flush=True)
        assert g.method == want.method and g.matched_stars == want.matched_stars and g.inliers == want.inliers, (name, g, want)
        assert np.allclose(g.transform, want.transform, rtol=0, atol=1e-8), (name, g.transform, want.transform)
        assert g.method in ("affine", "rigid"), (name, g)             # a star match, not the phase-correlation fallback
        whole_warp_equals_oracle(ctx, oracle, t, t_h, g.transform, f"[{name}, the library's transform]")
    return got, ref_h


def test_registration_at_4096_bench_density_equals_the_oracle(tctx, oracle):
    """16 x 16 whole background tiles, the bench's field (360 stars / Mpix at 25 x flux): a translated target, one that was itself
    warped (zero bands along two edges), one with NaN patches and cosmic rays, one rotated 0.3 degrees, one registration-like"""
    from astroburst_amd import synth
    from test_gpu_detect_affine import compare_stars
    ctx = tctx
    rows = cols = 4096
    y, x, flux = synth.star_catalog(rows, cols, max(8, int(360.0 * rows * cols / 1e6)))
    cat = (y, x, flux * 25.0)
    ref = star_frame(rows, cols, 0, cat, bad_patch_rate=0.0, cosmic_rate=1e-4)
    quiet = dict(bad_patch_rate=0.0, cosmic_rate=1e-4)
    moved = star_frame(rows, cols, 2, cat, rigid(0.0, -3.0, 2.0, rows, cols), **quiet)
    targets = [
        star_frame(rows, cols, 1, cat, rigid(0.0, 2.25, -1.5, rows, cols), **quiet),
        ctx.warp_image(moved, (1.0, 0.0, 7.5, 0.0, 1.0, -4.25), rows, cols),
        star_frame(rows, cols, 3, cat, rigid(0.0, -1.75, 0.4, rows, cols), bad_patch_rate=1e-6, cosmic_rate=1e-4),
        star_frame(rows, cols, 4, cat, rigid(0.3, 1.0, 2.0, rows, cols), **quiet),
        star_frame(rows, cols, 5, cat, rigid(0.02, 5.5, -3.25, rows, cols), **quiet),
    ]
    del moved
    assert float((targets[1][:, -7:] == 0.0).float().mean()) == 1.0 and float((targets[1][:4] == 0.0).float().mean()) == 1.0
    assert bool(targets[2].isnan().any())
    _, ref_h = registration_equals_oracle(ctx, oracle, ref, targets, ["translated", "warped before: zero bands", "NaN patches and cosmic rays",
                                                                      "rotated 0.3 deg", "0.02 deg + (5.5, -3.25)"])
    # the reference's own star list, as align_channel_affine detects it (normalised frame, 3.5 sigma)
    norm = oracle.normalize_for_detection(ref_h)
    want, wm, ws = timed("detect_stars 4096 x 4096", lambda: oracle.detect_stars(norm, 3.5))
    got, gm, gs = ctx.detect_stars(norm, 3.5)
    assert (gm, gs) == (wm, ws) and len(want) > 1000
    compare_stars(got, want)


def test_registration_at_c3_size_equals_the_oracle(tctx, oracle):
    """the pair of test_c3_star_align_leg_at_nircam_size (6000 stars x 60 flux, 0.02 degrees): the 54 x 49 tile grid with a ragged
    last row and column, the largest candidate-list workspace and 32-bit pixel indices, against the oracle"""
    from astroburst_amd import synth
    rows, cols = C3
    y, x, flux = synth.star_catalog(rows, cols, 6000, seed=31)
    cat = (y, x, flux * 60.0)
    ref = star_frame(rows, cols, 0, cat, bad_patch_rate=0.0)
    tgt = star_frame(rows, cols, 1, cat, rigid(0.02, 5.5, -3.25, rows, cols), bad_patch_rate=0.0)
    registration_equals_oracle(tctx, oracle, ref, [tgt], ["the C3 pair"])


# ---- C5 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="class")
def c5_planes():
    """the C5 field of test_gpu_full_size.py, on the device and on the host; freed after TestC5"""
    import torch
    from test_gpu_full_size import star_field_gpu
    planes = star_field_gpu(8192, 8192, 20000, 5, gains=(1.0, 0.8, 1.25))
    pair = [planes, [p.cpu().numpy() for p in planes]]
    del planes
    yield pair
    pair.clear()
    torch.cuda.empty_cache()


def close_images(got, want):                                           # test_gpu_masked.py's bar
    bad = got != want
    assert bad.mean() <= 1e-5, f"{bad.sum()} differing pixels"
    assert np.abs(got - want).max() <= 1e-5


class TestC5:
    """3 x 8192 x 8192, the field of test_c5_narrowband_8192_masked_stretch_scnr_spcc"""

    def test_c5_statistics_and_background_at_8192(self, tctx, oracle, c5_planes):
        from test_gpu_background import assert_parity
        from test_gpu_stats_stf import check_stats
        ctx = tctx
        (red, green, blue), (hr, hg, hb) = c5_planes
        check_stats(ctx.compute_image_stats(green), timed("compute_image_stats 8192 x 8192", lambda: oracle.compute_image_stats(hg)))
        want = timed("extract_background 8192 x 8192", lambda: oracle.extract_background(hr))
        got = ctx.extract_background(red)
        got.model, got.corrected = got.model.cpu().numpy(), got.corrected.cpu().numpy()
        assert_parity(got, want)

    def test_c5_masked_stretch_at_8192(self, tctx, oracle, c5_planes):
        ctx = tctx
        (red, green, blue), (hr, hg, hb) = c5_planes
        want = timed("masked_stretch 8192 x 8192", lambda: oracle.masked_stretch(hg))
        got = ctx.masked_stretch(green)
        assert got.iterations_run == want.iterations_run and got.converged == want.converged
        assert got.stars_masked == want.stars_masked > 300
        assert abs(got.final_background - want.final_background) <= 1e-6
        close_images(got.image.cpu().numpy(), want.image)

    def test_c5_shared_mask_stretch_and_scnr_at_8192(self, tctx, oracle, c5_planes):
        ctx = tctx
        (red, green, blue), (hr, hg, hb) = c5_planes
        want = timed("masked_stretch_rgb_shared 3 x 8192 x 8192", lambda: oracle.masked_stretch_rgb_shared(hr, hg, hb))
        got = ctx.masked_stretch_rgb_shared(red, green, blue)
        assert got[3].stars_masked == want[3].stars_masked
        assert abs(got[3].coverage_fraction - want[3].coverage_fraction) <= 1e-5
        for gch, wch in zip(got[:3], want[:3]):
            assert gch.iterations_run == wch.iterations_run and gch.converged == wch.converged
            close_images(gch.image.cpu().numpy(), wch.image)
        # SCNR on the library's own stretched planes, bit for bit (test_gpu_color.py)
        sr, sg, sb = (x.image.clone() for x in got[:3])
        hs = [x.cpu().numpy() for x in (sr, sg, sb)]
        ctx.apply_scnr_inplace(sr, sg, sb, "average", 0.8, True)
        wr, wg, wb = timed("apply_scnr 3 x 8192 x 8192", lambda: oracle.apply_scnr(*hs, "average", 0.8, True))
        for a, b in ((sr, wr), (sg, wg), (sb, wb)):
            assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)

    def test_c5_spcc_at_8192(self, tctx, oracle, c5_planes):
        from test_gpu_spcc import numbers
        (red, green, blue), (hr, hg, hb) = c5_planes
        want = timed("spcc_calibrate_rgb 3 x 8192 x 8192", lambda: oracle.spcc_calibrate_rgb(hr, hg, hb, 0.3))
        got = tctx.spcc_calibrate_rgb(red, green, blue, 0.3)
        assert (got.stars_matched, got.stars_total) == (want.stars_matched, want.stars_total) and got.stars_matched >= 50
        assert got.g_factor == 1.0
        assert np.allclose(numbers(got), numbers(want), rtol=1e-9, atol=0)
