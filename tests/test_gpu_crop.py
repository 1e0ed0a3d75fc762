"""HIP parity of the compose wizard's crop step (csrc/crop.hip) on one MI355X: ab_detect_valid_region(s), ab_crop_array,
ab_crop_channels_plan and ab_crop_channels against tests/crop_restatement.py (numpy + the oracle's compute_image_stats; pinned by
tests/test_crop_cpu.py).

There are no tolerances here: boxes and dims are compared with ==, planes through their uint32 views with array_equal, the
statistics field by field with ==.

The shapes are the smallest at which the kernels can go wrong.  Both kernels walk the flat pixel index of a dense plane: up to three
pixels precede the first 16-byte boundary, then groups of four, one per lane.  How many workgroups a plane gets depends on the
device's CU count and on the library's grid constants, so nothing here assumes it: a workgroup's span is a whole number of 256-lane
sweeps, hence every span boundary lies a multiple of 1024 pixels past the head, and the single-pixel sweep visits ALL of those.  At
70 x 2100 and 2100 x 70 (147 000 pixels) and at 65 x 257 both kernels run several workgroups on any device.  A group that crosses a row
end takes another path than one inside a row, so cols = 1, 5, 7, 70 and cols = 1, 2, 3 mod 4 are all here, and device planes are also
taken 1 to 3 floats past an aligned address.
"""
import itertools

import numpy as np
import pytest

import crop_restatement as R
from astroburst_amd import AstroBurstError, _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (64, 64), (65, 257), (33, 1022), (33, 1023), (70, 2100), (2100, 70)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
BORDERS = [(0, 0, 0, 0), (1, 0, 2, 3), (2, 3, 0, 1), (0, 2, 1, 0), (5, 1, 4, 7)]   # (top, bottom, left, right), each on its own


def _dev(a, offset=0):
    """the array on the device; offset > 0: at a pointer `offset` floats past a 256-byte aligned allocation"""
    import torch
    a = np.array(a, dtype=F32, copy=True, order="C")
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.zeros(a.size + offset + 64, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() == buf.data_ptr() + 4 * offset and view.is_contiguous()
    return view


def _dev_out(shape, offset, fill=np.nan):
    """an output plane of `shape` at `offset` floats past a 256-byte boundary, and the whole allocation (filled, with a guard band)"""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + offset + 64,), fill, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf[offset:offset + n].view(shape), buf


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_bits(got, want, what):
    got, want = _host(got), np.asarray(want, F32)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    assert np.array_equal(R.bits(got), R.bits(want)), f"{what}: {(R.bits(got) != R.bits(want)).sum()} of {want.size} pixels differ"


def assert_guard(whole, offset, n, what, fill_is_nan=True):
    whole = _host(whole)
    outside = np.concatenate([whole[:offset], whole[offset + n:]])
    assert np.isnan(outside).all() if fill_is_nan else not outside.any(), f"{what}: wrote outside the output"


def assert_stats(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert R.stats_row(g) == tuple(w), f"{what}, plane {i}: {R.stats_row(g)} != {tuple(w)}"


def assert_plan(got, want, what):
    assert tuple(got.crop_box) == tuple(want.crop_box), f"{what}: box {tuple(got.crop_box)} != {want.crop_box}"
    for k in ("out_rows", "out_cols", "actual_top", "actual_bottom", "actual_left", "actual_right", "auto_detected", "out_dims"):
        assert getattr(got, k) == getattr(want, k), f"{what}: {k} {getattr(got, k)} != {getattr(want, k)}"


# ---- ab_detect_valid_region --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_box_of_noise_inside_a_zero_border(ctx, shape):
    """a zero border of its own width on each side (0 included) around noise, host planes and device planes at every alignment"""
    for k, border in enumerate(BORDERS):
        a = R.bordered(shape, border, 100 + k)
        want = R.detect_valid_region(a)
        assert tuple(ctx.detect_valid_region(a)) == want, f"host {border}"
        for off in range(4):
            d = _dev(a, off)
            assert tuple(ctx.detect_valid_region(d)) == want, f"device +{off} {border}"
            assert_bits(d, a, f"the input after the call, +{off} {border}")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_all_invalid_and_all_valid_planes(ctx, shape):
    rows, cols = shape
    for off in (0, 3):
        assert tuple(ctx.detect_valid_region(_dev(np.zeros(shape, F32), off))) == (rows, 0, cols, 0)
        assert tuple(ctx.detect_valid_region(_dev(R.noise(shape, 1), off))) == (0, rows, 0, cols)
    assert tuple(ctx.detect_valid_region(np.zeros(shape, F32))) == (rows, 0, cols, 0)
    assert tuple(ctx.detect_valid_region(R.noise(shape, 1))) == (0, rows, 0, cols)


def _single_pixel_sweep(ctx, shape, flat_positions, offsets):
    import torch
    rows, cols = shape
    for off in offsets:
        d = _dev(np.zeros(shape, F32), off)
        flat = d.view(-1)
        for i in flat_positions:
            flat[i] = 1.0
            r, c = divmod(i, cols)
            assert tuple(ctx.detect_valid_region(d)) == (r, r + 1, c, c + 1), f"{shape} +{off}: the only valid pixel is at ({r}, {c})"
            flat[i] = 0.0
        assert not torch.count_nonzero(d).item()


def test_a_single_valid_pixel_at_every_lane_of_the_first_and_last_wave_of_a_row(ctx):
    """every column residue mod 64 of the first and the last wave's worth of a row, in the first, a middle and the last row"""
    shape = (3, 2100)
    cols = shape[1]
    columns = list(range(64)) + list(range(cols - 64, cols))
    _single_pixel_sweep(ctx, shape, [c for c in columns] + [cols + c for c in columns] + [2 * cols + c for c in columns], (0, 1))


@pytest.mark.parametrize("shape", [(70, 2100), (2100, 70), (65, 257)], ids=["70x2100", "2100x70", "65x257"])
def test_a_single_valid_pixel_at_the_edges_of_the_workgroups(ctx, shape):
    """a single valid pixel around every place a workgroup's span can begin or end: each multiple of 1024 pixels of the flat index (256
    lanes x 4 pixels, the unit spans are made of), five pixels either side to cover the up to three head pixels of an unaligned base,
    and both ends of the plane.  These are also the first and last rows any workgroup sees."""
    n = shape[0] * shape[1]
    marks = set(range(0, n, 1024)) | {256, n}
    pos = sorted({m + d for m in marks for d in range(-5, 6) if 0 <= m + d < n})
    _single_pixel_sweep(ctx, shape, pos, (0, 1, 2, 3))


def test_special_values_and_thresholds(ctx):
    """NaN, +-inf, -0.0 and values at the threshold; NaN, negative, zero and +inf thresholds (tests/test_crop_cpu.py's cases)"""
    thr = F32(0.25)
    for v, t, want in ((thr, thr, (3, 0, 3, 0)), (-thr, thr, (3, 0, 3, 0)), (np.nextafter(thr, F32(1)), thr, (1, 2, 1, 2)),
                       (F32(0.1), 0.1, (3, 0, 3, 0)), (np.nan, 1e-6, (3, 0, 3, 0)), (np.inf, 1e-6, (1, 2, 1, 2)), (-np.inf, 1e-6, (1, 2, 1, 2)),
                       (np.inf, np.inf, (3, 0, 3, 0)), (1.0, np.nan, (3, 0, 3, 0))):
        a = R.single((3, 3), 1, 1, v)
        assert R.detect_valid_region(a, t) == want
        assert tuple(ctx.detect_valid_region(a, t)) == want, (v, t)
        assert tuple(ctx.detect_valid_region(_dev(a), t)) == want, (v, t)
    neg0 = np.full((4, 4), -0.0, F32)
    assert tuple(ctx.detect_valid_region(_dev(neg0), 0.0)) == (4, 0, 4, 0)
    assert tuple(ctx.detect_valid_region(_dev(neg0), -1.0)) == (0, 4, 0, 4)
    rng = np.random.default_rng(11)
    specials = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-6, -1e-6, 2e-6, 0.5, -0.5], F32)
    for k in range(48):
        shape = (int(rng.integers(1, 12)), int(rng.integers(1, 40)))
        a = specials[rng.integers(0, specials.size, shape)]
        a[rng.random(shape) < rng.random()] = 0.0
        t = [1e-6, 0.0, -1.0, np.nan, np.inf, 0.5][k % 6]
        want = R.detect_valid_region(a, t)
        assert tuple(ctx.detect_valid_region(_dev(a, k % 4), t)) == want, (a, t)
        assert tuple(ctx.detect_valid_region(a, t)) == want, (a, t)


# ---- ab_detect_valid_regions -------------------------------------------------------------------------------------------------------------
def _batch_planes(shapes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k, s in enumerate(shapes):
        border = tuple(int(rng.integers(0, max(2, min(s) // 3))) for _ in range(4))
        out.append(R.bordered(s, border, seed + k))
    return out


@pytest.mark.parametrize("shapes", [[(65, 257)] * 3, [(65, 257)] * 7, [(70, 2100), (33, 1023), (3, 5)], [(9, 13)] * 19,
                                    [(1, 1), (7, 1), (64, 64), (1, 7)]],
                         ids=["3 equal", "7 equal", "3 different", "19 equal (two launches)", "4 tiny different"])
def test_batched_detection_equals_the_single_plane_results(ctx, shapes):
    planes = _batch_planes(shapes, 7)
    want_each = [R.detect_valid_region(p) for p in planes]
    want_common = R.common_box(want_each)
    dev = [_dev(p, k % 4) for k, p in enumerate(planes)]
    for src, what in ((dev, "device"), (planes, "host"), ([d if k % 2 else p for k, (d, p) in enumerate(zip(dev, planes))], "mixed")):
        each, common = ctx.detect_valid_regions(src)
        assert [tuple(b) for b in each] == want_each and tuple(common) == want_common, what
        assert [tuple(ctx.detect_valid_region(p)) for p in src] == want_each, f"{what}: one plane at a time"
        each, common = ctx.detect_valid_regions(src, want_common=False)
        assert [tuple(b) for b in each] == want_each and common is None, f"{what}: out_common NULL"
        each, common = ctx.detect_valid_regions(src, want_each=False)
        assert each is None and tuple(common) == want_common, f"{what}: out_each NULL"
        assert ctx.detect_valid_regions(src, want_each=False, want_common=False) == (None, None)
    for d, p in zip(dev, planes):
        assert_bits(d, p, "the inputs after the calls")


def test_batched_detection_with_a_threshold_and_empty_planes(ctx):
    planes = [R.single((6, 9), 2, 3, 0.5), np.zeros((4, 4), F32), R.single((6, 9), 5, 8, -2.0)]
    for t in (1e-6, 0.5, 3.0, -1.0, np.nan):
        want = [R.detect_valid_region(p, t) for p in planes]
        each, common = ctx.detect_valid_regions([_dev(p) for p in planes], t)
        assert [tuple(b) for b in each] == want and tuple(common) == R.common_box(want), t


# ---- ab_crop_array -----------------------------------------------------------------------------------------------------------------------
def _payload(shape, seed):
    """every bit pattern is a pixel: NaNs with payloads, denormals, both zeros"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(F32)


def test_crop_at_every_alignment_of_source_and_destination(ctx):
    """every (left mod 4, width mod 4) with widths 1 .. 9, the source 0 and 1 floats and the output 0 .. 3 floats past an aligned
    address: the rows of both sit at every alignment mod 4 floats, independently of each other.  NaN payloads survive; not one float
    outside the output is written."""
    src = _payload((11, 40), 3)
    devs = {off: _dev(src, off) for off in (0, 1)}
    for left, width, in_off, out_off in itertools.product(range(4), range(1, 10), (0, 1), range(4)):
        box = (2, 9, left + 4, left + 4 + width)
        want = R.crop_array(src, *box)
        out, whole = _dev_out(want.shape, out_off)
        ctx.crop_array(devs[in_off], box, out=out)
        what = f"left {left + 4} width {width} source +{in_off} output +{out_off}"
        assert_bits(out, want, what)
        assert_guard(whole, out_off, want.size, what)
    for off, d in devs.items():
        assert_bits(d, src, "the input after the calls")


@pytest.mark.parametrize("shape,box", [((9, 1500), (1, 8, 101, 1400)), ((70, 2100), (3, 66, 50, 2049)), ((2100, 70), (100, 2000, 3, 68)),
                                       ((65, 257), (0, 65, 0, 257))], ids=["7x1299", "63x1999", "1900x65", "whole 65x257"])
def test_crop_wider_than_a_workgroups_sweep_and_over_several_workgroups(ctx, shape, box):
    src = _payload(shape, 4)
    want = R.crop_array(src, *box)
    for in_off, out_off in ((0, 0), (1, 3), (2, 1), (3, 2)):
        out, whole = _dev_out(want.shape, out_off)
        ctx.crop_array(_dev(src, in_off), box, out=out)
        assert_bits(out, want, f"source +{in_off} output +{out_off}")
        assert_guard(whole, out_off, want.size, f"source +{in_off} output +{out_off}")
    assert_bits(ctx.crop_array(src, box), want, "host")
    assert_bits(ctx.crop_array(_dev(src), box), want, "device, allocated by the call")


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (3, 5), (64, 64)], ids=["1x1", "1x7", "7x1", "3x5", "64x64"])
def test_crop_windows_at_the_edges_whole_clamped_and_empty(ctx, shape):
    rows, cols = shape
    src = _payload(shape, 5)
    d = _dev(src, 1)
    boxes = [(0, rows, 0, cols),                                    # the whole plane
             (0, max(rows - 1, 1), 0, cols), (min(1, rows - 1), rows, 0, cols), (0, rows, 0, max(cols - 1, 1)), (0, rows, min(1, cols - 1), cols),
             (0, rows + 5, 0, cols + 9), (0, 1 << 40, 0, 1 << 40),  # larger than the plane: clamped
             (rows, rows + 3, 0, cols), (0, rows, cols + 2, cols + 4), (rows // 2, rows // 2, 0, cols), (0, rows, cols, 0), (rows, 0, cols, 0)]
    for box in boxes:
        want = R.crop_array(src, *box)
        assert_bits(ctx.crop_array(d, box), want, f"device {box}")
        assert_bits(ctx.crop_array(src, box), want, f"host {box}")
    assert_bits(d, src, "the input after the calls")


def test_crop_rejects_an_output_of_the_wrong_dims(ctx):
    import torch
    src = _dev(R.noise((8, 10), 6))
    for shape in ((4, 5), (5, 4), (5, 6), (4, 6), (0, 5)):
        with pytest.raises(AstroBurstError) as e:
            ctx.crop_array(src, (1, 6, 2, 7), out=torch.empty(shape, dtype=torch.float32, device="cuda"))
        assert e.value.code == _lib.AB_ERR_INVALID and "must be 5 x 5" in e.value.message
    with pytest.raises(AstroBurstError) as e:                        # a clamped box: the output has the clamped dims
        ctx.crop_array(src, (1, 60, 2, 70), out=torch.empty((59, 68), dtype=torch.float32, device="cuda"))
    assert e.value.code == _lib.AB_ERR_INVALID and "must be 7 x 8" in e.value.message
    with pytest.raises(AstroBurstError) as e:
        ctx.crop_array(R.noise((8, 10), 6), (1, 6, 2, 7), out=np.empty((5, 6), F32))
    assert e.value.code == _lib.AB_ERR_INVALID


# ---- ab_crop_channels_plan / ab_crop_channels --------------------------------------------------------------------------------------------
def _check_channels(ctx, oracle, planes, device, **mode):
    want_plan = R.crop_channels_plan(planes, **mode)
    want_cropped, want_stats = R.crop_channels(planes, want_plan, oracle)
    src = [_dev(p, k % 4) for k, p in enumerate(planes)] if device else planes
    what = f"{'device' if device else 'host'} {mode}"
    plan = ctx.crop_channels_plan(src, **mode)
    assert_plan(plan, want_plan, what)
    cropped, stats = ctx.crop_channels(src, plan)
    for k, (c, w) in enumerate(zip(cropped, want_cropped)):
        assert_bits(c, w, f"{what}, plane {k}")
        assert hasattr(c, "is_cuda") == device
    assert_stats(stats, want_stats, what)
    cropped, stats = ctx.crop_channels(src, plan, want_stats=False)
    assert stats is None
    for k, (c, w) in enumerate(zip(cropped, want_cropped)):
        assert_bits(c, w, f"{what}, stats NULL, plane {k}")
    for s, p in zip(src, planes):
        assert_bits(s, p, f"{what}: the inputs after the calls")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_crop_channels_auto_mode(ctx, oracle, device):
    same = [R.bordered((65, 257), b, 20 + k) for k, b in enumerate([(2, 1, 3, 0), (0, 3, 1, 2), (4, 0, 0, 5)])]
    _check_channels(ctx, oracle, same, device)
    ragged = [R.bordered((70, 2100), (3, 2, 7, 1), 30), R.bordered((33, 1023), (1, 0, 9, 0), 31), R.bordered((64, 1500), (0, 4, 2, 3), 32)]
    _check_channels(ctx, oracle, ragged, device)
    _check_channels(ctx, oracle, [R.bordered((9, 13), (1, 2, 3, 4), 40 + k) for k in range(7)], device)
    _check_channels(ctx, oracle, [R.single((5, 9), 2, 4, 0.5)], device, threshold=0.25)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_crop_channels_manual_mode(ctx, oracle, device):
    planes = [R.noise((65, 257), 50), R.noise((40, 300), 51), R.noise((90, 31), 52)]     # per-plane outputs of different dims
    _check_channels(ctx, oracle, planes, device, auto_detect=False, top=1, bottom=2, left=3, right=1)
    _check_channels(ctx, oracle, planes, device, auto_detect=False)
    # margins larger than the plane: no emptiness check, zero-area outputs, ImageStats::default()
    _check_channels(ctx, oracle, planes, device, auto_detect=False, top=9, bottom=500, left=2, right=500)
    _check_channels(ctx, oracle, planes, device, auto_detect=False, top=50, bottom=0, left=40, right=0)   # empty for plane 1 and 2 only


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_crop_channels_error_strings(ctx, device):
    wrap = _dev if device else (lambda a: a)
    with pytest.raises(AstroBurstError) as e:
        ctx.crop_channels_plan([wrap(R.single((8, 8), 1, 1)), wrap(R.single((8, 8), 6, 6))])
    assert e.value.code == _lib.AB_ERR_INVALID and e.value.message == R.NO_OVERLAP
    with pytest.raises(AstroBurstError) as e:
        ctx.crop_channels_plan([wrap(np.zeros((4, 4), F32))])
    assert e.value.message == R.NO_OVERLAP
    with pytest.raises(AstroBurstError) as e:                       # rows overlap, columns only touch
        ctx.crop_channels_plan([wrap(R.single((8, 8), 1, 5)), wrap(R.single((8, 8), 1, 6))])
    assert e.value.message == R.NO_OVERLAP
    for call in (lambda: ctx.crop_channels_plan([]), lambda: ctx.crop_channels_plan([], auto_detect=False),
                 lambda: ctx.crop_channels([], R.crop_channels_plan([np.ones((2, 2), F32)]))):
        with pytest.raises(AstroBurstError) as e:
            call()
        assert e.value.code == _lib.AB_ERR_INVALID and e.value.message == R.NO_PATHS


def test_crop_channels_rejects_outputs_of_the_wrong_dims(ctx):
    import torch
    src = [_dev(R.noise((8, 10), 60)), _dev(R.noise((6, 12), 61))]
    plan = ctx.crop_channels_plan(src, auto_detect=False, top=1, bottom=1, left=2, right=3)
    assert plan.out_dims == ((6, 5), (5, 5))
    outs = [torch.empty((6, 5), dtype=torch.float32, device="cuda"), torch.empty((6, 5), dtype=torch.float32, device="cuda")]
    with pytest.raises(AstroBurstError) as e:
        ctx.crop_channels(src, plan, outs=outs)
    assert e.value.code == _lib.AB_ERR_INVALID and "plane 1 must be 5 x 5" in e.value.message


def test_crop_channels_above_four_million_pixels_takes_the_histogram_statistics(ctx, oracle):
    """2100 x 2100 with a thin border: 2095 x 2097 = 4 393 215 cropped pixels > 4 000 000, the statistics' histogram route"""
    planes = [R.bordered((2100, 2100), (2, 3, 1, 2), 70), R.bordered((2100, 2100), (1, 0, 0, 1), 71)]
    want_plan = R.crop_channels_plan(planes)
    assert want_plan.out_dims == ((2095, 2097),) * 2
    want_cropped, want_stats = R.crop_channels(planes, want_plan, oracle)
    src = [_dev(p) for p in planes]
    plan = ctx.crop_channels_plan(src)
    assert_plan(plan, want_plan, "2100 x 2100")
    cropped, stats = ctx.crop_channels(src, plan)
    for k in range(2):
        assert_bits(cropped[k], want_cropped[k], f"plane {k}")
        assert_bits(src[k], planes[k], f"input {k} after the calls")
    assert_stats(stats, want_stats, "2100 x 2100")
