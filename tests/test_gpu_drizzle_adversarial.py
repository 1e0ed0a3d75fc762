"""csrc/drizzle.hip on the cases of tests/drizzle_adversarial.py: sample lists designed value by value (exact clip-threshold ties on
both sides, MAD == 0 and the 1e-10 floor, duplicates across the median, subnormal and near-FLT_MAX samples, up to 16 acting clip
rounds, every count up to every cap, the sign of a single zero) at the first and the last cap of every sorting-network width and on
the heap-sort path, and frame geometries designed offset by offset (footprint edges exactly on and a few ulp either side of integers,
output axes of length 1, offsets up to 1e300, frames 0.01 px either side of the Gaussian reach, outputs that are whole workgroups).
tests/test_drizzle_adversarial_cpu.py holds every case to what it claims; which kernel decision each family pins is listed there
and in tests/drizzle_adversarial.py.

Bar: that of tests/test_gpu_drizzle.py, through its `compare`, against tests/drizzle_restatement.py (computed once per case, never
modified).  Square: weight map and rejected_pixels bit for bit; image bit for bit where the f64 sum is exact, within 1 f32 ulp
elsewhere.  Gaussian / Lanczos3: the same outside the threshold pixels, of which there may be 1e-3 of the output at most.  One
check is stricter than `compare`: a pixel that received a single sample returns that sample's BITS (-0.0 stays -0.0).

Measured on one MI355X: all 240 cases (141 designed-list calls, 99 geometry calls) hold the bar; the largest threshold-pixel share
over the 67 Gaussian / Lanczos3 cases is 0.0, so no pixel was left out of any comparison.  The whole file runs in under 4 s.

Also measured there, once, with builds of csrc/drizzle.hip in which ONE decision was changed (not kept in the tree).  The families that
then fail, none of which tests/test_gpu_drizzle.py notices unless marked (*):
  `>` for `>=` at t_lo, `<` for `<=` at t_hi (*)        A1d A1g A2 A4z A5z A5d A8 (every call)
  no 1e-10 floor under sigma                            A2 A4d A8;   sigma = fmaxf(mad * 1.4826f, 1e-10f) in f32: A1g
  the median's average of two samples in f64            A5d;         the MAD's average in f64: A5o
  a run of the MAD merge read after it has run out      A3 A8 (the run-out lists)
  no fall-back when nothing survives (*)                A4z A5z
  a finite pad in the sorting network instead of +inf   A5z A5d A5o
  a single sample returned as sample + 0.0f             A8
  sigma_iterations clamped to 12, or cut to an int      A6
  subnormals flushed (-fgpu-flush-denormals-to-zero)    A4z A4d
  ceil(x) - 1 for floor(x) / floor(x) + 1 for ceil(x) in the window test (*)      B1a B1b B2 B3 B4
  a border pixel given the interior's candidate radius (*)                        B1a B2 B4 B5
  a Gaussian reach of 5 sigma (*)                       B2 B4
Three changes no case can see, because nothing observable depends on them: which side the MAD merge takes on a TIE (the two
candidates are equal), `pad` = 0 (a candidate within rounding of the radius has a weight far below 1e-12), and a Gaussian reach of
7.40 instead of 7.44 sigma (the candidate range is rounded outward to whole input pixels, which absorbs up to `scale` output pixels)."""
import numpy as np
import pytest

import drizzle_adversarial as DA
import drizzle_restatement as R
from test_gpu_drizzle import compare, to_np

pytestmark = pytest.mark.gpu

DESIGNED = DA.designed_cases()
GEOMETRY = DA.geometry_cases()


def ids(cases):
    return [c.name for c in cases]


def run(ctx, case, device=False):
    frames = list(case.frames)
    if device:
        import torch
        frames = [torch.from_numpy(np.array(f)).cuda() for f in frames]
    want = DA.wanted(case)
    got = ctx.drizzle_frames(frames, list(case.offsets), case.scale, case.pixfrac, case.kernel, case.sl, case.sh, case.iters)
    share = compare(got, want, case.kernel, len(case.frames), case.name)
    assert share == float(want.threshold.mean()) or case.kernel == R.SQUARE
    return got, want


@pytest.mark.parametrize("case", DESIGNED, ids=ids(DESIGNED))
def test_designed_lists(ctx, case):
    got, want = run(ctx, case)
    img = to_np(got.image)
    single = want.counts == 1
    assert np.array_equal(DA.bits(img)[single], DA.bits(want.image)[single]), case.name     # the sample itself, sign of zero included
    for oy, ox, vals, tag in case.designed:      # (compare has covered these pixels; this names the list that differs)
        if want.exact[oy, ox]:
            assert img[oy, ox] == want.image[oy, ox], (case.name, tag, img[oy, ox], want.image[oy, ox])


@pytest.mark.parametrize("case", GEOMETRY, ids=ids(GEOMETRY))
def test_geometry(ctx, case):
    got, want = run(ctx, case)
    assert want.exact.all() and np.array_equal(to_np(got.image)[~want.threshold], want.image[~want.threshold]), case.name


def test_device_planes_give_the_same_bytes(ctx):
    """one case per path (network of 8, 16, 32, 64 wires; heap sort) and one per geometry family, from device tensors"""
    names = ["A1d-n4", "A2-n8", "A5z-n16", "A6-n32-it1000", "A4z-n33", "B1b-s2.5-p0.5-gaussian", "B2-1x1-n33-lanczos3", "B3-1e300-gaussian"]
    for case in (c for c in DESIGNED + GEOMETRY if c.name in names):
        host = ctx.drizzle_frames(list(case.frames), list(case.offsets), case.scale, case.pixfrac, case.kernel, case.sl, case.sh, case.iters)
        dev, _ = run(ctx, case, device=True)
        assert dev.image.is_cuda
        assert to_np(dev.image).tobytes() == host.image.tobytes() and to_np(dev.weight_map).tobytes() == host.weight_map.tobytes()
        assert dev.rejected_pixels == host.rejected_pixels

