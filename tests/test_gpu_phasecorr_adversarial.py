"""GPU parity on the adversarial planes of tests/phasecorr_adversarial.py: exact peak ties, peaks on the surface's border, bins on
both sides of the 1e-15 cut, the pixel that decides is_constant_or_zero in every loop of minmax_finite_kernel, the thresholds
themselves, transforms of length 1, downsample boxes without a finite pixel, the batch driver's rounds, the table cache.

The bars are those of tests/test_gpu_phasecorr.py and nothing looser: the correlation surface is the oracle's bit for bit, dx and dy
are == the oracle's, the confidence is within 1e-9 relative (its variance reduction runs in another order), stack_images' offsets
are == the pairwise results and the oracle's.  tests/test_phasecorr_adversarial_cpu.py holds every fixture to its claim without a
GPU and shows which mistake in the kernel each family catches."""
import ctypes as C

import numpy as np
import pytest

import phasecorr_adversarial as PA

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = (0.0, 0.0, 0.0)


def check(got, ref):
    assert got[0] == ref[0] and got[1] == ref[1], (got, ref)
    assert abs(got[2] - ref[2]) <= 1e-9 * max(1.0, abs(ref[2])), (got, ref)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_single(ctx, oracle, ref, tgt):
    """correlate_single with its surface, against the oracle's; returns the oracle's (dx, dy, confidence, surface)"""
    got, want = ctx.correlate_single(ref, tgt, want_surface=True), oracle.correlate_single(ref, tgt, want_surface=True)
    assert same_bits(got[3], want[3]), f"surface: {np.count_nonzero(got[3] != want[3])} elements differ, max |d| = {np.abs(got[3] - want[3]).max()}"
    check(got[:3], want[:3])
    return want


# ---- 1: exact ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PA.TIE_SHAPES + ((2, 2),))
def test_negated_pair_first_of_the_tied_maxima_wins(ctx, oracle, shape):
    ref, tgt, claim = PA.negated_pair(shape)
    dx, dy, conf, surface = ctx.correlate_single(ref, tgt, want_surface=True)
    assert np.array_equal(surface, claim["surface"])                                   # the closed form: -1, then zeros
    assert (dx, dy) == (claim["dx"], claim["dy"]) and abs(conf - claim["confidence"]) <= 1e-9
    want = check_single(ctx, oracle, ref, tgt)
    assert want[:2] == (claim["dx"], claim["dy"])
    pair = ctx.phase_correlate(ref, tgt)
    if shape == (2, 2):
        assert pair == ZERO                                                            # four pixels: degenerate
    else:
        assert pair[:2] == (claim["dx"], claim["dy"])
        check(pair, want[:3])


def test_negated_pair_ties_in_both_passes_of_the_coarse_to_fine_driver(ctx, oracle):
    ref, tgt, claim = PA.negated_pair_coarse_to_fine()
    got = ctx.phase_correlate(ref, tgt)
    assert got[:2] == (claim["dx"], claim["dy"]) == (0.79296875, 0.0) and abs(got[2] - claim["confidence"]) <= 1e-9
    check(got, oracle.phase_correlate(ref, tgt))


@pytest.mark.parametrize("name,ref,tgt", PA.window_null_pairs(), ids=lambda v: v if isinstance(v, str) else "")
def test_all_zero_surface_peaks_at_index_zero(ctx, oracle, name, ref, tgt):
    dx, dy, conf, surface = ctx.correlate_single(ref, tgt, want_surface=True)
    assert not np.any(surface)
    assert (dx, dy, conf) == ZERO              # a peak at any other index unwraps to a non-zero shift
    check_single(ctx, oracle, ref, tgt)
    assert ctx.phase_correlate(ref, tgt) == ZERO == oracle.phase_correlate(ref, tgt)


# ---- 2: border peaks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", list(PA.BORDER_SHIFTS))
@pytest.mark.parametrize("shape", PA.BORDER_SHAPES)
def test_border_peak_reads_its_circular_neighbours(ctx, oracle, shape, shift):
    ref, tgt = PA.border_pair(shape, shift)
    want = check_single(ctx, oracle, ref, tgt)
    assert divmod(int(np.argmax(want[3])), 128) == PA.BORDER_SHIFTS[shift]
    check(ctx.phase_correlate(ref, tgt), want[:3])


# ---- 3: the cut ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,tgt", PA.cut_pairs(), ids=lambda v: v if isinstance(v, str) else "")
def test_bins_on_both_sides_of_the_cut(ctx, oracle, name, ref, tgt):
    want = check_single(ctx, oracle, ref, tgt)
    assert want[2] != 0.0
    check(ctx.phase_correlate(ref, tgt), want[:3])


# ---- 4: the deciding pixel -------------------------------------------------------------------------------------------------------
DECIDING = PA.deciding_cases()


@pytest.mark.parametrize("case", DECIDING, ids=lambda c: c.name)
def test_deciding_pixel_is_seen(ctx, oracle, case):
    want = oracle.phase_correlate(case.reference, case.target)
    assert want[2] != 0.0
    check(ctx.phase_correlate(case.reference, case.target), want)
    assert ctx.phase_correlate(case.reference, case.without_the_pixel()) == ZERO


def unaligned(plane):
    """a device copy of the plane that starts 4 bytes into its allocation"""
    import torch
    t = torch.empty(plane.size + 1, device="cuda")[1:].view(*plane.shape)
    t.copy_(torch.from_numpy(plane))
    assert t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("case", DECIDING, ids=lambda c: c.name)
def test_deciding_pixel_is_seen_in_unaligned_device_planes(ctx, oracle, case):
    """the float4 loops must not be taken, and the answer is unchanged"""
    import torch
    want = oracle.phase_correlate(case.reference, case.target)
    ref = torch.from_numpy(case.reference).cuda()
    check(ctx.phase_correlate(ref, unaligned(case.target)), want)
    check(ctx.phase_correlate(unaligned(case.reference), torch.from_numpy(case.target).cuda()), want)
    assert ctx.phase_correlate(ref, unaligned(case.without_the_pixel())) == ZERO
    torch.cuda.synchronize()


def test_ragged_frame_constant_in_the_window_is_degenerate(ctx, oracle):
    """the frame differs from a constant only in its padding, which must not be read: row stride 52, 46 columns in the window"""
    frames = PA.ragged_stack_frames()
    assert ctx.phase_correlate(frames[0], frames[2]) == ZERO
    pairs = [ctx.phase_correlate(frames[0], f) for f in frames[1:]]
    offsets = ctx.stack_images(frames, align=True).offsets
    assert offsets == [(0, 0)] + [(PA.round_to_i32(dy), PA.round_to_i32(dx)) for dx, dy, _ in pairs]
    assert offsets == oracle.stack_images_align(frames)[2] and offsets[2] == (0, 0) and offsets[1] != (0, 0) != offsets[3]


# ---- 5: thresholds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,tgt,degenerate", PA.threshold_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_thresholds_of_is_constant_or_zero(ctx, oracle, name, ref, tgt, degenerate):
    got, want = ctx.phase_correlate(ref, tgt), oracle.phase_correlate(ref, tgt)
    check(got, want)
    assert (got == ZERO) == degenerate and (degenerate or got[2] != 0.0)


# ---- 6: length one ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PA.LENGTH_ONE_SHAPES)
def test_length_one_and_smallest_planes(ctx, oracle, shape):
    ref, tgt = PA.small_pair(shape)
    want = oracle.phase_correlate(ref, tgt)
    assert want[2] != 0.0
    if max(shape) <= 512:
        assert check_single(ctx, oracle, ref, tgt)[:3] == want
    check(ctx.phase_correlate(ref, tgt), want)


@pytest.mark.parametrize("shape", PA.TOO_SMALL_SHAPES)
def test_fewer_than_16_pixels_is_degenerate(ctx, oracle, shape):
    ref, tgt = PA.small_pair(shape)
    assert ctx.phase_correlate(ref, tgt) == ZERO == oracle.phase_correlate(ref, tgt)


# ---- 7: boxes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PA.BOX_SHAPES)
def test_boxes_without_a_finite_pixel(ctx, oracle, shape):
    ref, tgt, _ = PA.box_pair(shape)
    want = oracle.phase_correlate(ref, tgt)
    assert want[2] != 0.0
    check(ctx.phase_correlate(ref, tgt), want)
    check(ctx.phase_correlate(tgt, ref), oracle.phase_correlate(tgt, ref))


# ---- 8: batch rounds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PA.BATCH_LAYOUTS))
def test_batch_rounds_with_degenerate_targets(ctx, oracle, name):
    frames, degenerate = PA.batch_frames(name)
    pairs = [ctx.phase_correlate(frames[0], f) for f in frames[1:]]
    for k, (dx, dy, conf) in enumerate(pairs, start=1):
        if k in degenerate:
            assert (dx, dy, conf) == ZERO, (k, degenerate[k])
        else:                                                   # the noise keeps every shift away from a rounding tie
            assert min(abs(abs(v) % 1.0 - 0.5) for v in (dx, dy)) > 1e-3, (k, dx, dy)
            check((dx, dy, conf), oracle.phase_correlate(frames[0], frames[k]))
    pairwise = [(0, 0)] + [(PA.round_to_i32(dy), PA.round_to_i32(dx)) for dx, dy, _ in pairs]
    offsets = ctx.stack_images(frames, align=True).offsets
    assert offsets == pairwise
    assert offsets == oracle.stack_images_align(frames)[2]
    live = [offsets[k] for k in range(1, len(frames)) if k not in degenerate]
    assert len(set(live)) == len(live) and (0, 0) not in live    # distinct: a pair landing in another's slot shows
    assert all(offsets[k] == (0, 0) for k in degenerate)


# ---- 9: the table cache ----------------------------------------------------------------------------------------------------------
def test_table_cache_across_changes_of_dimensions(ctx, oracle):
    surfaces = []
    for ref, tgt in PA.table_pairs():
        if max(ref.shape) <= 512:
            surfaces.append(ctx.correlate_single(ref, tgt, want_surface=True)[3])
            check_single(ctx, oracle, ref, tgt)                 # (a second call at the same dimensions: a hit)
        else:
            surfaces.append(None)
            check(ctx.phase_correlate(ref, tgt), oracle.phase_correlate(ref, tgt))
    assert same_bits(surfaces[0], surfaces[5]) and same_bits(surfaces[0], surfaces[2])
    assert same_bits(surfaces[0], oracle.correlate_single(*PA.table_pairs()[0], want_surface=True)[3])


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_context_goes_on(ctx, oracle):
    from astroburst_amd import _lib
    a, b = PA.border_pair((100, 75), (1, -1))
    plane = lambda p, rows=None, cols=None: _lib.Plane(C.c_void_p(p.ctypes.data), rows or p.shape[0], cols or p.shape[1], 0)
    res = _lib.PhaseCorrelationResultC()
    single = lambda pa, pb, out=res: ctx._L.ab_correlate_single(ctx._h, C.byref(pa) if pa else None, C.byref(pb) if pb else None,
                                                                  C.byref(out) if out else None, None)
    pair = lambda pa, pb, out=res: ctx._L.ab_phase_correlate(ctx._h, C.byref(pa) if pa else None, C.byref(pb) if pb else None,
                                                               C.byref(out) if out else None)
    wide = np.zeros((4, 513), F32)
    tall = np.zeros((513, 4), F32)
    assert single(plane(a), plane(b, rows=99)) == _lib.AB_ERR_INVALID                  # unequal shapes
    assert single(plane(a), plane(b, cols=74)) == _lib.AB_ERR_INVALID
    assert single(plane(wide), plane(wide)) == _lib.AB_ERR_INVALID                     # a dimension above 512
    assert single(plane(tall), plane(tall)) == _lib.AB_ERR_INVALID
    for args in ((None, plane(b)), (plane(a), None), (plane(a), plane(b), None)):
        assert single(*args) == _lib.AB_ERR_INVALID
        assert pair(*args) == _lib.AB_ERR_INVALID
    assert ctx._L.ab_phase_correlate(None, C.byref(plane(a)), C.byref(plane(b)), C.byref(res)) == _lib.AB_ERR_INVALID
    for rows, cols in ((0, 75), (100, 0)):             # an empty reference: ab_stage_in refuses it before anything is allocated or copied
        assert pair(_lib.Plane(C.c_void_p(a.ctypes.data), rows, cols, 0), plane(b)) == _lib.AB_ERR_INVALID
    assert single(plane(a), plane(b)) == _lib.AB_OK and pair(plane(a), plane(b)) == _lib.AB_OK
    check((res.dx, res.dy, res.confidence), oracle.phase_correlate(a, b))
    check_single(ctx, oracle, a, b)
