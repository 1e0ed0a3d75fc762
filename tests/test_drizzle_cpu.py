"""Drizzle without a GPU: the restatement (tests/drizzle_restatement.py) against hand-computed cases; its vectorised form against its
plain loops; the per-output-pixel GATHER (the formulation csrc/drizzle.hip uses) against the scatter's lists element for element,
border pixels and frames shifted partly and wholly off the field included; the library's host-only ab_drizzle_output_dims; and the
kernels' code for gfx950 (no scratch, no spills)."""
import os
import re
import subprocess

import numpy as np
import pytest

import drizzle_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astroburst_amd", "csrc")
KERNELS = [R.SQUARE, R.GAUSSIAN, R.LANCZOS3]


def grid(rows, cols, base):
    return (base + np.arange(rows * cols, dtype=np.float32).reshape(rows, cols) / 4.0).astype(np.float32)


def both(frames, offsets, *a, **k):
    """drizzle_loop and the vectorised drizzle must agree on everything; returns the loop's result"""
    x = R.drizzle_loop(frames, offsets, *a, **k)
    y = R.drizzle(frames, offsets, *a, **k, keep_lists=True)
    assert x.image.tobytes() == y.image.tobytes() and x.weight.tobytes() == y.weight.tobytes()
    assert x.rejected == y.rejected and np.array_equal(x.rejected_map, y.rejected_map)
    assert np.array_equal(x.threshold, y.threshold) and np.array_equal(x.exact, y.exact) and np.array_equal(x.counts, y.counts)
    assert [[float(v) for v in l] for l in x.lists] == [[float(v) for v in l] for l in y.lists]
    assert x.wsum.tobytes() == y.wsum.tobytes()
    return x


# ---- hand-computed cases ---------------------------------------------------------------------------------------------------------
def test_scale_2_pixfrac_1_zero_offset_is_weight_one_per_frame_and_the_mean_of_two():
    """half = 1, c = 2 i: the footprint [2 i - 1, 2 i + 1] covers output pixels 2 i - 1 and 2 i whole, so output pixel o takes input
    pixel (o + 1) // 2 with weight 1 x 1 per frame; the last output row / column would need input index `rows` / `cols`: nothing"""
    a, b = grid(5, 6, 10.0), grid(5, 6, 20.0)
    r = both([a, b], [(0, 0), (0, 0)], 2.0, 1.0, R.SQUARE)
    assert r.dims == (5, 6, 10, 12)
    iy, ix = (np.arange(9) + 1) // 2, (np.arange(11) + 1) // 2
    want = ((a[np.ix_(iy, ix)].astype(np.float64) + b[np.ix_(iy, ix)]) / 2.0).astype(np.float32)
    assert np.array_equal(r.image[:9, :11], want) and (r.weight[:9, :11] == 2.0).all() and (r.counts[:9, :11] == 2).all()
    for edge in (r.image[9], r.image[:, 11], r.weight[9], r.weight[:, 11], r.counts[9], r.counts[:, 11]):
        assert (edge == 0).all()
    assert r.rejected == 0


def test_quarter_pixel_offset_has_the_known_overlap_areas_and_count_one_pixels():
    """scale 2, pixfrac 0.5 (half = 0.5).  Frame 0: c = 2 i, footprint [2 i - 0.5, 2 i + 0.5]: output 2 i - 1 and 2 i, overlap 0.5
    each.  Frame 1 reported at dx = +0.25 (drizzle_frame gets -0.25): c = 2 i - 0.5, footprint [2 i - 1, 2 i]: output 2 i - 1 whole,
    and 2 i is in the window (ceil(2 i) = 2 i) with overlap 0 -> not pushed.  In y both frames give 0.5.  So odd output columns hold
    two samples with weight 0.5 * 0.5 + 1 * 0.5, even ones frame 0's sample alone with weight 0.25."""
    a, b = grid(4, 5, 10.0), grid(4, 5, 50.0)
    r = both([a, b], [(0, 0), (0.25, 0.0)], 2.0, 0.5, R.SQUARE)
    for oy in range(7):
        iy = (oy + 1) // 2
        for ox in range(10):
            ix = (ox + 1) // 2
            if ix >= 5:
                assert r.counts[oy, ox] == 0 and r.image[oy, ox] == 0 and r.weight[oy, ox] == 0
            elif ox % 2 == 1:
                assert r.counts[oy, ox] == 2 and r.weight[oy, ox] == np.float32(0.75)
                assert r.image[oy, ox] == np.float32((float(a[iy, ix]) + float(b[iy, ix])) / 2.0)
            else:
                assert r.counts[oy, ox] == 1 and r.weight[oy, ox] == np.float32(0.25) and r.image[oy, ox] == a[iy, ix]
    assert (r.counts[7] == 0).all()


def test_an_outlier_frame_is_rejected_by_the_mad_clip_and_counted():
    """scale 2 / pixfrac 0.5 / no offsets: one sample per frame and pixel, weight 0.25.  Samples 10, 10.25, 9.75, 10, 1000: median 10,
    MAD 0.25, sigma 0.37065, the 1000 goes; then 9.75 .. 10.25: MAD (0 + 0.25) / 2, sigma 0.1853, 3 sigma = 0.556: all stay; mean 10"""
    frames = [np.full((3, 4), v, np.float32) for v in (10.0, 10.25, 9.75, 10.0, 1000.0)]
    r = both(frames, [(0, 0)] * 5, 2.0, 0.5, R.SQUARE)
    assert (r.image[:5, :7] == 10.0).all() and (r.weight[:5, :7] == 1.25).all() and (r.rejected_map[:5, :7] == 1).all()
    assert r.rejected == 35
    # one round only: the same; no rounds: the outlier stays in the mean
    assert both(frames, [(0, 0)] * 5, 2.0, 0.5, R.SQUARE, 3.0, 3.0, 1).rejected == 35
    r0 = both(frames, [(0, 0)] * 5, 2.0, 0.5, R.SQUARE, 3.0, 3.0, 0)
    assert r0.rejected == 0 and (r0.image[:5, :7] == np.float32(1040.0 / 5.0)).all()


def test_the_cap_keeps_the_first_2n_pushes_and_their_weights_only():
    """scale 1 / pixfrac 1: every interior output pixel receives four pushes of weight 0.25 from frame 0 (input rows o, o + 1 x columns
    o, o + 1, in that order) -- the cap of max(2 * 2, 4) = 4 is reached, and all of frame 1 is dropped, weight included"""
    a, b = grid(5, 6, 10.0), grid(5, 6, 500.0)
    r = both([a, b], [(0, 0), (0.25, 0.0)], 1.0, 1.0, R.SQUARE)
    assert r.dims == (5, 6, 5, 6)
    for oy in range(4):
        for ox in range(5):
            i = oy * 6 + ox
            assert [float(v) for v in r.lists[i]] == [float(a[oy, ox]), float(a[oy, ox + 1]), float(a[oy + 1, ox]), float(a[oy + 1, ox + 1])]
            assert r.weight[oy, ox] == 1.0
    # the last row / column: two pushes per frame (overlap 0.5 x 0.5 from one side only), so frame 1 does get in there
    assert r.counts[4, 2] == 4 and any(float(v) >= 500.0 for v in r.lists[4 * 6 + 2])


def test_finalize_sigma_corner_cases():
    s = [np.float32(v) for v in (1.0, 2.0, 3.0, 4.0, 100.0)]
    assert R.finalize_pixel([], 0.0, 3, 3, 5)[:3] == (0.0, 0.0, 0)
    assert R.finalize_pixel(s[:1], 0.3, 3, 3, 5)[:3] == (1.0, np.float32(0.3), 0)
    assert R.finalize_pixel(s[:2], 1.0, 0.0, 0.0, 5)[2] == 0  # fewer than 3 active: no round
    v, _, rej, _ = R.finalize_pixel(s, 1.0, float("nan"), 3.0, 5)  # NaN bound: every comparison fails, nothing survives -> mean of all
    assert rej == 5 and v == np.float32(110.0 / 5.0)
    v, _, rej, _ = R.finalize_pixel(s, 1.0, float("inf"), float("inf"), 5)
    assert rej == 0 and v == np.float32(22.0)
    v, _, rej, _ = R.finalize_pixel(s, 1.0, 0.0, 0.0, 5)  # only dev == 0 survives: the median itself
    assert rej == 4 and v == 3.0


def test_finalize_many_equals_finalize_pixel():
    rng = np.random.default_rng(2)
    cap = 12
    counts = rng.integers(0, cap + 1, 400)
    V = np.zeros((400, cap), np.float32)
    for i, c in enumerate(counts):
        V[i, :c] = np.round(rng.normal(100.0, 3.0, c) * 16.0) / 16.0
        if c and rng.random() < 0.5:
            V[i, rng.integers(0, c)] = 5000.0
    wsum = rng.random(400)
    for sl, sh, it in ((3.0, 3.0, 5), (0.0, 0.0, 5), (float("nan"), 2.0, 3), (1.0, float("inf"), 1), (-1.0, 3.0, 5), (0.5, 0.5, 0)):
        img, w, rej, ex = R.finalize_many(V, counts, wsum, sl, sh, it)
        for i, c in enumerate(counts):
            want = R.finalize_pixel(list(V[i, :c]), wsum[i], sl, sh, it)
            assert (img[i], w[i], rej[i], ex[i]) == want, (i, sl, sh, it)


# ---- loops == vectorised == gather -----------------------------------------------------------------------------------------------
def awkward_case(seed, n=5, rows=6, cols=8):
    rng = np.random.default_rng(seed)
    frames = [(rng.integers(0, 1 << 14, (rows, cols)) / 256.0).astype(np.float32) for k in range(n)]
    frames[1][2, 3] = np.nan
    frames[2][0, 0] = np.inf
    frames[0][rows - 1, cols - 1] = -np.inf
    # fractional, integer, partly off the field (a corner stays), wholly off it
    offsets = [(0.0, 0.0), tuple(rng.uniform(-3, 3, 2)), (2.0, -1.0), (cols - 1.3, -(rows - 2.6)), (cols + 4.5, 0.3)][:n]
    return frames, offsets


@pytest.mark.parametrize("scale,pixfrac", [(2.0, 0.7), (1.0, 1.0), (1.5, 0.5), (3.0, 0.9), (4.0, 1.0), (2.5, 0.1)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_gather_equals_scatter_element_for_element(kernel, scale, pixfrac):
    frames, offsets = awkward_case(int(scale * 10) + kernel)
    r = both(frames, offsets, scale, pixfrac, kernel)
    _, _, out_rows, out_cols = r.dims
    dropped = 0
    for oy in range(out_rows):
        for ox in range(out_cols):
            s, w = R.gather_pixel(frames, offsets, oy, ox, scale, pixfrac, kernel)
            assert [float(v) for v in s] == [float(v) for v in r.lists[oy * out_cols + ox]], (oy, ox)
            assert w == r.wsum[oy, ox], (oy, ox)
            dropped += len(s) == 10
    if (scale, pixfrac) == (1.0, 1.0):
        assert dropped > 0  # (the cap was reached somewhere: the order of the pushes mattered)


def test_clamped_footprints_pile_up_on_the_border():
    """a frame shifted wholly off the field still reaches the border pixels under the Gaussian kernel (clamp_index clamps onto the
    border and the weight alone decides), and not under Square (no overlap)"""
    frames = [np.full((6, 8), 7.0, np.float32), np.full((6, 8), 9.0, np.float32)]
    off = [(0.0, 0.0), (8.6, 0.0)]  # frame 1's pixels land 0.6 .. 8.6 input pixels left of the field
    g = both(frames, off, 2.0, 1.0, R.GAUSSIAN)
    q = both(frames, off, 2.0, 1.0, R.SQUARE)
    assert any(9.0 in [float(v) for v in g.lists[oy * 16]] for oy in range(12))
    assert not any(9.0 in [float(v) for v in l] for l in q.lists)
    assert not any(9.0 in [float(v) for v in g.lists[oy * 16 + ox]] for oy in range(12) for ox in range(1, 16))


# ---- the library, host-only ------------------------------------------------------------------------------------------------------
def test_output_dims_through_the_library():
    import astroburst_amd as ab
    from astroburst_amd.core import drizzle_output_dims
    assert drizzle_output_dims([(14, 17), (14, 17)], 2.0, 0.7) == (14, 17, 28, 34)
    assert drizzle_output_dims([(14, 17), (14, 17)], 2.5, 0.7) == (14, 17, 35, 43)
    assert drizzle_output_dims([(14, 17), (14, 17)], 1.5, 0.7) == (14, 17, 21, 26)
    assert drizzle_output_dims([(14, 17), (14, 17)], 0.2, 0.7)[2:] == (14, 17) and drizzle_output_dims([(14, 17), (14, 17)], 9.0, 0.7)[2:] == (56, 68)
    # cropped to the minimum dims; tolerance (max(min_rows, min_cols) as f64 * 0.05) as usize = 5 for 100 x 104
    assert drizzle_output_dims([(100, 109), (105, 104), (102, 106)], 2.0, 0.7) == (100, 104, 200, 208)
    assert drizzle_output_dims(np.zeros((3, 8, 9), np.float32), 3.0, 1.0) == (8, 9, 24, 27)
    for shapes, scale in (([(14, 17)] * 2, 2.0), ([(100, 109), (105, 104)], 2.0), ([(40, 40), (41, 42)], 1.5)):
        assert drizzle_output_dims(shapes, scale, 0.7) == R.output_dims(shapes, scale, 0.7)[:4]
    for bad, text in (([], "No images to drizzle"), ([(14, 17)], "at least 2 frames"), ([(100, 104), (106, 104)], "vary too much"),
                      ([(100, 104), (100, 110)], "vary too much"), ([(4, 4)] * 32768, "")):
        with pytest.raises(ab.AstroBurstError) as e:
            drizzle_output_dims(bad)
        assert e.value.code == ab._lib.AB_ERR_INVALID and text in str(e.value)
        if len(bad) < 32768:
            with pytest.raises(ValueError, match=text):
                R.output_dims(bad, 2.0, 0.7)
    with pytest.raises(ab.AstroBurstError):
        drizzle_output_dims([(4, 4)] * 2, float("nan"), 0.7)
    assert drizzle_output_dims([(4, 4)] * 32767) == (4, 4, 8, 8)


# ---- the kernels, compiled for gfx950 with the Makefile's flags --------------------------------------------------------------------
def test_gather_kernels_have_no_scratch_and_fit_four_waves_per_simd(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in base
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *base, "-w", "--save-temps", "-c", os.path.join(CSRC, "drizzle.hip"), "-o",
                    os.path.join(tmp_path, "drizzle.o")], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lst = open(os.path.join(tmp_path, "drizzle-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_spill_count:\s+\d+", lst, re.S)}
    gather = [n for n in meta if "dz_gather_kernel" in n]
    assert len(gather) == 15, sorted(meta)  # ({LDS with a network of 8, 16, 32, 64 wires}, long-list) x {Square, Gaussian, Lanczos3}
    for name in gather:
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[name]).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta[name]).group(1))
        body = re.split(r"^%s:" % re.escape(name), lst, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert scratch == 0 and "scratch_" not in body, (name, scratch)
        assert vgprs <= 128, (name, vgprs)  # 512 / 128: four waves per SIMD by registers
    spills = re.findall(r"\.name:\s+(\S+)\n.*?\.vgpr_spill_count:\s+(\d+)", lst, re.S)
    assert spills and all(int(n) == 0 for _, n in spills), spills
