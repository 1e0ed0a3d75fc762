"""The fixtures of tests/phasecorr_adversarial.py held to what they claim (no GPU), against the CPU oracle (oracle/orc_phasecorr.c, the
kernel's butterflies) and the independent numpy restatement (tests/phasecorr_restatement.py).  A fixture that has drifted fails
here, so the GPU test (tests/test_gpu_phasecorr_adversarial.py) cannot pass by testing nothing.

The second half restates the parts of csrc/phase_corr.hip that the fixtures aim at -- the peak's three-level reduction, the loops
of minmax_finite_kernel, the circular neighbours, the batch driver's compaction -- as small numpy models with one mistake that
can be switched on, and shows that every mistake changes the answer on the fixtures (and that the models without a mistake give
the oracle's answer)."""
import numpy as np
import pytest

import phasecorr_adversarial as PA
import phasecorr_restatement as R

F32 = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def close_to_restatement(got, want):
    """the existing bar between the oracle and the restatement (tests/test_oracle_phasecorr_cases.py)"""
    return (abs(got[0] - want[0]) <= 1e-6 and abs(got[1] - want[1]) <= 1e-6 and abs(got[2] - want[2]) <= 1e-6 * max(1.0, abs(want[2])))


def both(oracle, ref, tgt):
    got, want = oracle.phase_correlate(ref, tgt), R.phase_correlate(ref, tgt)
    assert close_to_restatement(got, want), (ref.shape, got, want)
    return got


# ---- 1: exact ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PA.TIE_SHAPES + ((2, 2),))
def test_negated_pair_surface_is_minus_one_then_zeros(oracle, shape):
    ref, tgt, claim = PA.negated_pair(shape)
    assert np.array_equal(tgt, -ref) and np.abs(ref).min() > 0
    dx, dy, conf, surface = oracle.correlate_single(ref, tgt, want_surface=True)
    assert surface.ravel()[0] == -1.0 and np.count_nonzero(surface) == 1 and np.array_equal(surface, claim["surface"])
    assert int(np.argmax(surface)) == claim["peak_index"] == 1 and (surface.ravel()[1:] == surface.max()).all()      # the tie
    assert (dx, dy) == (claim["dx"], claim["dy"])
    assert abs(conf - claim["confidence"]) <= 1e-12
    if shape != (2, 2):
        assert oracle.phase_correlate(ref, tgt) == (dx, dy, conf)
        assert (claim["dx"], claim["dy"]) == (0.5, 0.0)
    else:
        assert (claim["dx"], claim["dy"], claim["confidence"]) == (1.0, 0.0, 0.5)
        assert oracle.phase_correlate(ref, tgt) == (0.0, 0.0, 0.0)                  # four pixels: degenerate


def test_negated_pair_confidences_are_the_stated_ones():
    want = {(4, 4): 0.25, (33, 17): 1.0 / np.sqrt(64.0 * 32.0), (100, 75): 0.0078125, (128, 128): 0.0078125, (512, 512): 0.001953125}
    for shape in PA.TIE_SHAPES:
        assert PA.negated_pair(shape)[2]["confidence"] == want[shape]
    assert abs(want[(33, 17)] - 0.0221) < 5e-5


def test_negated_pair_coarse_to_fine_ties_in_both_passes(oracle):
    ref, tgt, claim = PA.negated_pair_coarse_to_fine()
    assert ref.shape == (520, 300) and (claim["dx"], claim["dy"]) == (0.79296875, 0.0)
    ds_ref, ds_tgt = oracle.area_downsample(ref, 512, 300), oracle.area_downsample(tgt, 512, 300)
    assert np.array_equal(ds_tgt, -ds_ref)
    assert oracle.correlate_single(ds_ref, ds_tgt)[:2] == (0.5, 0.0)
    assert oracle.correlate_single(ref[4:516], tgt[4:516])[:2] == (0.5, 0.0)        # the centred crops: rows 260 +- 256
    dx, dy, conf = oracle.phase_correlate(ref, tgt)
    assert (dx, dy) == (claim["dx"], claim["dy"]) and abs(conf - claim["confidence"]) <= 1e-12


def test_the_restatement_does_not_tie():
    """why family 1 rests on the oracle and the closed form: with numpy's FFT the zeros are 1e-17-sized residues"""
    ref, tgt, _ = PA.negated_pair((128, 128))
    wy = R.hann_periodic(128)
    fa, fb = np.fft.fft2(R._windowed(ref, wy, wy, 128, 128)), np.fft.fft2(R._windowed(tgt, wy, wy, 128, 128))
    assert np.array_equal(fb, -fa)
    prod = fa * np.conj(fb)
    corr = np.fft.ifft2(prod / np.abs(prod)).real
    assert abs(corr[0, 0] + 1.0) < 1e-12 and np.abs(corr.ravel()[1:]).max() < 1e-12 and np.count_nonzero(corr) > 1


@pytest.mark.parametrize("name,ref,tgt", PA.window_null_pairs(), ids=lambda v: v if isinstance(v, str) else "")
def test_window_null_plane_gives_an_all_zero_surface(oracle, name, ref, tgt):
    null = tgt if name.startswith("target") else ref
    n = null.shape[0]
    assert R.hann_periodic(n)[0] == 0.0 and not np.any(null[1:, 1:]) and np.count_nonzero(null) >= 2 * n - 8
    assert not R._is_constant_or_zero(null) and not R._is_constant_or_zero(ref) and not R._is_constant_or_zero(tgt)
    dx, dy, conf, surface = oracle.correlate_single(ref, tgt, want_surface=True)
    assert not np.any(surface) and int(np.argmax(surface)) == 0
    assert (dx, dy, conf) == (0.0, 0.0, 0.0) == oracle.phase_correlate(ref, tgt) == R.phase_correlate(ref, tgt)


# ---- 2: border peaks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", list(PA.BORDER_SHIFTS))
@pytest.mark.parametrize("shape", PA.BORDER_SHAPES)
def test_border_peak_is_where_it_is_meant_to_be(oracle, shape, shift):
    ref, tgt = PA.border_pair(shape, shift)
    dx, dy, conf, surface = oracle.correlate_single(ref, tgt, want_surface=True)
    assert surface.shape == (128, 128)
    py, px = divmod(int(np.argmax(surface)), 128)
    assert (py, px) == PA.BORDER_SHIFTS[shift] and (py in (0, 127) or px in (0, 127))
    assert (surface == surface.max()).sum() == 1 and conf > 20.0
    assert abs(dy + shift[0]) < 0.5 and abs(dx + shift[1]) < 0.5
    both(oracle, ref, tgt)
    # the oracle's refinement is the restatement's (circular neighbours); a neighbour clamped at the border gives another shift
    wrapped = (R._unwrap(px, 128) + R._refine_1d(surface, py, px, False), R._unwrap(py, 128) + R._refine_1d(surface, py, px, True))
    assert wrapped == (dx, dy)
    assert clamped_refinement(surface, py, px) != (dx, dy)


def clamped_refinement(s, py, px):
    """the 3-point refinement with neighbours that stop at the border instead of wrapping around"""
    fr, fc = s.shape

    def refine(c, p, n):
        denom = 2.0 * (2.0 * c - p - n)
        return 0.0 if abs(denom) < 1e-15 else min(max((p - n) / denom, -0.5), 0.5)
    c = s[py, px]
    return (R._unwrap(px, fc) + refine(c, s[py, max(px - 1, 0)], s[py, min(px + 1, fc - 1)]),
            R._unwrap(py, fr) + refine(c, s[max(py - 1, 0), px], s[min(py + 1, fr - 1), px]))


# ---- 3: the 1e-15 cut ------------------------------------------------------------------------------------------------------------
def cross_power_magnitudes(ref, tgt):
    """|A conj(B)| per bin from the restatement's numpy spectra"""
    rows, cols = ref.shape
    fr, fc = R._next_pow2(rows), R._next_pow2(cols)
    wy, wx = R.hann_periodic(rows), R.hann_periodic(cols)
    return np.abs(np.fft.fft2(R._windowed(ref, wy, wx, fr, fc)) * np.conj(np.fft.fft2(R._windowed(tgt, wy, wx, fr, fc))))


@pytest.mark.parametrize("name,ref,tgt", PA.cut_pairs(), ids=lambda v: v if isinstance(v, str) else "")
def test_cut_pairs_have_bins_on_both_sides(oracle, name, ref, tgt):
    assert ref.shape == tgt.shape == (128, 128) and not R._is_constant_or_zero(ref) and not R._is_constant_or_zero(tgt)
    mag = cross_power_magnitudes(ref, tgt)
    fraction = float((mag <= R.EPSILON).mean())
    print(f"{name}: {fraction:.3f} of the bins at or below the cut")
    lo, hi = PA.CUT_FRACTION_BOUNDS
    assert lo <= fraction <= hi, fraction
    # bins within 10 % of the cut on either side: a cut that has moved by that much zeroes other bins
    assert ((mag > 0.9 * R.EPSILON) & (mag <= R.EPSILON)).sum() >= 16 and ((mag > R.EPSILON) & (mag < 1.1 * R.EPSILON)).sum() >= 16
    got = both(oracle, ref, tgt)
    assert got[2] != 0.0


# ---- 4: the deciding pixel -------------------------------------------------------------------------------------------------------
DECIDING = PA.deciding_cases()


@pytest.mark.parametrize("case", DECIDING, ids=lambda c: c.name)
def test_deciding_pixel_decides(oracle, case):
    y, x = case.pixel
    assert case.target[y, x] == 9.0 and (np.delete(case.target.ravel(), y * case.target.shape[1] + x) == 7.0).all()
    assert y < case.rows and x < case.cols and case.reference.shape[0] == case.rows                # the common window keeps the pixel
    # (the oracle alone: where the refinement crop misses the pixel it correlates a windowed CONSTANT, whose spectrum is rounding
    # noise in all but a few bins -- the two FFTs then disagree by 0.03 px on two of these planes; the verdict is what is claimed)
    assert not R._is_constant_or_zero(case.target[:case.rows, :case.cols]) and not R._is_constant_or_zero(case.reference)
    got = oracle.phase_correlate(case.reference, case.target)
    assert got[2] != 0.0
    flat = case.without_the_pixel()
    assert oracle.phase_correlate(case.reference, flat) == (0.0, 0.0, 0.0) == R.phase_correlate(case.reference, flat)


@pytest.mark.parametrize("case", DECIDING, ids=lambda c: c.name)
def test_deciding_pixel_is_read_by_the_loop_it_names(case):
    """... and by no other: a minmax_finite_kernel without that loop calls the plane degenerate"""
    y, x = case.pixel
    names, strided = PA.minmax_paths(case.rows, case.cols, case.ld)
    assert names[x] == case.path and bool(strided[y]) == case.strided
    window = case.target[:case.rows, :case.cols]

    def degenerate(read):
        fin = window[read & np.isfinite(window)]
        return fin.size < 16 or abs(F32(fin.max()) - F32(fin.min())) < F32(1e-10)
    everything = np.ones(window.shape, bool)
    assert not degenerate(everything)
    assert degenerate(everything & (names != case.path)[None, :])
    if case.strided:
        assert degenerate(everything & ~strided[:, None])
    unaligned = PA.minmax_paths(case.rows, case.cols, case.ld, aligned=False)[0]
    assert (unaligned == "scalar").all()


def test_the_deciding_cases_cover_every_loop():
    assert {c.path for c in DECIDING} == {"scalar", "load-a", "load-b", "remainder", "tail"} and any(c.strided for c in DECIDING)
    names = PA.minmax_paths(17, 2054, 2056)[0]
    assert [names[x] for x in (0, 1023, 1024, 2047, 2048, 2051, 2052, 2053)] == ["load-a"] * 2 + ["load-b"] * 2 + ["remainder"] * 2 + ["tail"] * 2
    assert (PA.minmax_paths(17, 2054, 2054)[0] == "scalar").all()                    # ld % 4 == 2
    names = PA.minmax_paths(17, 2056, 2056)[0]
    assert names[2047] == "load-b" and (names[2048:] == "remainder").all()
    assert (PA.minmax_paths(2050, 16, 16)[0] == "remainder").all() and PA.minmax_paths(2050, 16, 16)[1].sum() == 2


def test_ragged_frame_is_constant_in_the_window_only(oracle):
    frames = PA.ragged_stack_frames()
    r, c = PA.RAGGED_WINDOW
    ragged = frames[2]
    assert ragged.shape == PA.RAGGED_SHAPE and ragged.shape[1] % 4 == 0 and c % 4 != 0
    assert (min(f.shape[0] for f in frames), min(f.shape[1] for f in frames)) == (r, c)
    assert (ragged[:r, :c] == 100.0).all() and np.isinf(ragged[:r, c:]).any() and np.isnan(ragged[r:]).any()
    assert not R._is_constant_or_zero(ragged[:r, :c + 1]) and not R._is_constant_or_zero(ragged[:r + 1, :c])
    names = PA.minmax_paths(r, c, ragged.shape[1])[0]
    assert (names[:44] != "tail").all() and (names[44:] == "tail").all()
    assert oracle.phase_correlate(frames[0], ragged) == (0.0, 0.0, 0.0) == R.phase_correlate(frames[0], ragged)
    offsets = oracle.stack_images_align(frames)[2]
    assert offsets[0] == offsets[2] == (0, 0) and offsets[1] != (0, 0) and offsets[3] != (0, 0) and offsets[1] != offsets[3]


# ---- 5: thresholds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ref,tgt,degenerate", PA.threshold_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_threshold_cases(oracle, name, ref, tgt, degenerate):
    assert (R._is_constant_or_zero(ref) or R._is_constant_or_zero(tgt)) == degenerate
    got = both(oracle, ref, tgt)
    assert (got == (0.0, 0.0, 0.0)) == degenerate and (degenerate or got[2] != 0.0)
    finite = int(np.isfinite(tgt).sum())
    if name.startswith("15-finite") and not name.endswith("reference"):
        assert finite == 15 and tgt.shape == (4, 5)
    if name == "16-finite":
        assert finite == 16 and tgt.shape == (4, 5) and np.isinf(tgt).sum() == 2
    if name == "15-finite-inf":
        assert np.isinf(tgt).sum() == 5 and not np.isnan(tgt).any()
    if name == "flat-with-inf":
        assert finite == 60 and np.isinf(tgt).sum() == 4 and np.unique(tgt[np.isfinite(tgt)]).size == 1


def test_spike_values_straddle_the_f32_threshold():
    t = F32(1e-10)
    assert abs(F32(9e-11) - F32(0)) < t and not abs(F32(1.1e-10) - F32(0)) < t and not abs(F32(2e-10) - F32(0)) < t


# ---- 6: length one ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PA.LENGTH_ONE_SHAPES)
def test_length_one_and_smallest_planes(oracle, shape):
    ref, tgt = PA.small_pair(shape)
    assert ref.shape == tgt.shape == shape and ref.size >= 16
    got = both(oracle, ref, tgt)
    assert got[2] != 0.0
    if max(shape) <= 512:
        assert oracle.correlate_single(ref, tgt) == got
    if shape[0] == 1:
        assert got[1] == 0.0
    if shape[1] == 1:
        assert got[0] == 0.0


@pytest.mark.parametrize("shape", PA.TOO_SMALL_SHAPES)
def test_fewer_than_16_pixels_is_degenerate(oracle, shape):
    ref, tgt = PA.small_pair(shape)
    assert ref.size == 15 and both(oracle, ref, tgt) == (0.0, 0.0, 0.0)


# ---- 7: boxes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PA.BOX_SHAPES)
def test_boxes_without_a_finite_pixel_are_zero(oracle, shape):
    ref, tgt, holes = PA.box_pair(shape)
    assert ref.shape == tgt.shape == shape and np.isnan(tgt).sum() == 40 * 60 and np.isinf(tgt).sum() == 100
    ds = oracle.area_downsample(tgt, 512, 512)
    assert np.isfinite(ds).all()
    for ys, xs in holes:
        assert ys.stop - ys.start >= 4 and xs.stop - xs.start >= 4 and not np.any(ds[ys, xs])
    assert (ds == 0.0).sum() == sum((ys.stop - ys.start) * (xs.stop - xs.start) for ys, xs in holes)     # and nowhere else
    assert np.array_equal(ds, R.area_downsample(tgt, 512, 512))
    got = both(oracle, ref, tgt) if shape == PA.BOX_SHAPES[0] else oracle.phase_correlate(ref, tgt)
    assert got[2] != 0.0
    sy = shape[0] / 512.0
    assert (sy == int(sy)) == (shape[0] == 1024)                # box edges on exact (1024) and inexact (600, 1025) multiples


# ---- 8: batch rounds -------------------------------------------------------------------------------------------------------------
def driver_model(pairwise, dead, mistake="", kept=None):
    """ab_phase_correlate_many_device's bookkeeping: rounds of 16 targets, the live ones compacted, results written back through
    `live`; above 512 px (kept is not None: the targets whose coarse answer is kept) the pairs that are refined are compacted once
    more and written back through live[fine[j]].  pairwise[i] = the single pair's result of target i, dead = the degenerate
    targets.  Mistakes: "unshifted" writes result k of a round to place k instead of live[k]; "unshifted-fine" writes refined result
    j to live[j] instead of live[fine[j]]; "stop" ends at a round without a live pair instead of going on."""
    out = [(0.0, 0.0, 0.0)] * len(pairwise)
    for base in range(0, len(pairwise), PA.K_BATCH):
        nb = min(PA.K_BATCH, len(pairwise) - base)
        live = [i for i in range(nb) if base + i not in dead]
        if not live:
            if mistake == "stop":
                break
            continue
        place = lambda k: base + (k if mistake == "unshifted" else live[k])
        fine = []
        for k, i in enumerate(live):
            if kept is None or base + i in kept:
                out[place(k)] = pairwise[base + i]
            else:
                fine.append(k)
        for j, k in enumerate(fine):
            out[place(j if mistake == "unshifted-fine" else k)] = pairwise[base + live[k]]
    return out


@pytest.mark.parametrize("name", list(PA.BATCH_LAYOUTS))
def test_batch_layouts(oracle, name):
    frames, degenerate = PA.batch_frames(name)
    n = len(frames)
    assert n == PA.BATCH_LAYOUTS[name][0] and all(f.shape == frames[0].shape for f in frames)
    assert frames[0].shape == (PA.MIXED_SHAPE if name == "coarse-to-fine-mixed" else PA.BATCH_SHAPE)
    pairs = [oracle.phase_correlate(frames[0], f) for f in frames[1:]]
    for k in range(1, n):
        kind = degenerate.get(k)
        assert (pairs[k - 1] == (0.0, 0.0, 0.0)) == (kind is not None)
        if kind == "all-nan":
            assert np.isnan(frames[k]).all()
        elif kind == "15-finite":
            assert np.isfinite(frames[k]).sum() == 15 and np.unique(frames[k][np.isfinite(frames[k])]).size == 15
        elif kind == "constant":
            assert np.unique(frames[k]).size == 1
        else:
            dx, dy, _ = pairs[k - 1]
            assert min(abs(abs(v) % 1.0 - 0.5) for v in (dx, dy)) > 1e-3                    # away from a rounding tie
            if name != "coarse-to-fine-mixed":
                assert (PA.round_to_i32(dy), PA.round_to_i32(dx)) == tuple(-s for s in PA.BATCH_SHIFTS[k - 1])
    offsets = oracle.stack_images_align(frames)[2]
    assert offsets == [(0, 0)] + [(PA.round_to_i32(dy), PA.round_to_i32(dx)) for dx, dy, _ in pairs]
    live = [offsets[k] for k in range(1, n) if k not in degenerate]
    assert len(set(live)) == len(live) and (0, 0) not in live
    # the driver's bookkeeping: right as it is, wrong with either mistake
    dead = {k - 1 for k in degenerate}
    assert driver_model(pairs, dead) == pairs
    assert driver_model(pairs, dead, "unshifted") != pairs
    if name == "dead-middle-round":
        assert driver_model(pairs, dead, "stop") != pairs


def test_mixed_batch_compacts_twice(oracle):
    """the 520 x 300 round: which pairs are refined and which keep their coarse answer is as stated, and the driver's second
    compaction (`fine`) matters on it"""
    frames, degenerate, kept = PA.mixed_batch_frames()
    rows, cols = PA.MIXED_SHAPE
    ds = [None if k in degenerate else oracle.area_downsample(f, 512, cols) for k, f in enumerate(frames)]
    for k in range(1, len(frames)):
        if k in degenerate:
            continue
        cdx, cdy, _ = oracle.correlate_single(ds[0], ds[k])
        assert PA.crop_sizes_match(cdx, cdy, rows, cols) == (k not in kept), k
    live = [k for k in range(1, len(frames)) if k not in degenerate]
    assert [k in kept for k in live] == [False, True, False, True, False]
    pairs = [oracle.phase_correlate(frames[0], f) for f in frames[1:]]
    dead, kept0 = {k - 1 for k in degenerate}, {k - 1 for k in kept}
    assert driver_model(pairs, dead, kept=kept0) == pairs
    for mistake in ("unshifted", "unshifted-fine"):
        assert driver_model(pairs, dead, mistake, kept=kept0) != pairs


def test_batch_layouts_cover_the_places_the_issue_names():
    place = lambda k: ((k - 1) // PA.K_BATCH, (k - 1) % PA.K_BATCH)
    one, two, dead_one, middle = (PA.BATCH_LAYOUTS[k] for k in ("one-round", "round-and-one", "round-and-a-dead-one", "dead-middle-round"))
    assert one[0] - 1 == 16 and two[0] - 1 == 17 and middle[0] - 1 == 33
    assert {place(k) for k in one[1]} >= {(0, 0), (0, 15)} and {place(k) for k in two[1]} == {(0, 0), (0, 15)}
    assert place(17) == (1, 0) and 17 in dead_one[1] and 17 not in two[1]
    assert {k for k in middle[1] if place(k)[0] == 1} == set(range(17, 33)) and 33 not in middle[1] and place(33) == (2, 0)
    assert {"all-nan", "15-finite", "constant"} == set(one[1].values()) == {middle[1][k] for k in range(17, 33)}
    assert len(set(PA.BATCH_SHIFTS)) == len(PA.BATCH_SHIFTS) >= 33 and (0, 0) not in PA.BATCH_SHIFTS


# ---- 9: tables -------------------------------------------------------------------------------------------------------------------
def test_table_sequence(oracle):
    pairs = PA.table_pairs()
    assert [p[0].shape for p in pairs] == list(PA.TABLE_SEQUENCE)
    assert pairs[0][0] is pairs[2][0] is pairs[5][0] and pairs[0][1] is pairs[5][1]
    assert PA.TABLE_SEQUENCE[1] == PA.TABLE_SEQUENCE[0][::-1]               # same pixel count, same padded size, other windows
    assert PA.TABLE_SEQUENCE[4] == (512, 300)                               # the dims of 520 x 300's coarse pass: a hit in set 0
    for ref, tgt in pairs:
        assert both(oracle, ref, tgt)[2] > 20.0


# ---- the peak reduction, restated with its mistakes ------------------------------------------------------------------------------
NONE = 0x7FFFFFFF


def peak_model(surface, mistake=""):
    """scale_peak_kernel + peak_finish_kernel on a finished surface: the first maximum per thread over the grid-stride loop, the LDS
    tree (maximum value, lowest index among equals), the sequential walk over the workgroups' partials.  Mistakes: "thread" keeps
    the LAST maximum per thread, "tree" / "finish" keep the higher index on a tie there."""
    v = surface.ravel()
    n = v.size
    pg = min(PA.K_PARTIALS, (n + PA.K_BLOCK - 1) // PA.K_BLOCK)
    stride = pg * PA.K_BLOCK
    iters = (n + stride - 1) // stride
    padded = np.full(iters * stride, -np.inf)
    padded[:n] = v
    grid = padded.reshape(iters, pg, PA.K_BLOCK)
    k = (iters - 1 - np.argmax(grid[::-1], axis=0)) if mistake == "thread" else np.argmax(grid, axis=0)
    best = np.take_along_axis(grid, k[None], axis=0)[0]
    idx = k * stride + np.arange(pg)[:, None] * PA.K_BLOCK + np.arange(PA.K_BLOCK)[None, :]
    idx = np.where(idx < n, idx, NONE)

    def takes(a_best, a_idx, b_best, b_idx, higher):
        tie = (b_idx > a_idx) if higher else (b_idx < a_idx)
        return (b_idx != NONE) & ((a_idx == NONE) | (b_best > a_best) | ((b_best == a_best) & tie))
    off = PA.K_BLOCK // 2
    while off >= 1:
        t = takes(best[:, :off], idx[:, :off], best[:, off:2 * off], idx[:, off:2 * off], mistake == "tree")
        best[:, :off] = np.where(t, best[:, off:2 * off], best[:, :off])
        idx[:, :off] = np.where(t, idx[:, off:2 * off], idx[:, :off])
        off //= 2
    b, i = -np.finfo(np.float64).max, NONE
    for g in range(pg):
        if takes(b, i, best[g, 0], idx[g, 0], mistake == "finish"):
            b, i = best[g, 0], idx[g, 0]
    return 0 if i == NONE else int(i)


def tie_surfaces(oracle):
    out = [(shape, PA.negated_pair(shape)[2]["surface"]) for shape in PA.TIE_SHAPES]
    return out + [((n, n), np.zeros((n, n))) for n in (128, 512)]


def test_peak_model_finds_the_first_maximum(oracle):
    for shape, surface in tie_surfaces(oracle):
        assert peak_model(surface) == int(np.argmax(surface))
    for shape, shift in (((128, 128), (1, -1)), ((100, 75), (0, 0))):
        surface = oracle.correlate_single(*PA.border_pair(shape, shift), want_surface=True)[3]
        for mistake in ("", "thread", "tree", "finish"):          # a single maximum: no mistake shows, which is why ties are needed
            assert peak_model(surface, mistake) == int(np.argmax(surface))


@pytest.mark.parametrize("mistake", ["thread", "tree", "finish"])
def test_tied_surfaces_catch_a_tie_kept_on_the_higher_index(oracle, mistake):
    caught = {shape: peak_model(surface, mistake) != int(np.argmax(surface)) for shape, surface in tie_surfaces(oracle)[:5]}
    assert caught[(512, 512)]                       # 4 elements per thread, 256 threads, 256 workgroups: every level ties
    if mistake == "tree":
        assert all(caught.values())                 # every size ties inside a workgroup
    if mistake == "finish":
        assert caught[(128, 128)] and caught[(100, 75)] and not caught[(4, 4)]      # 64 workgroups; one workgroup
    if mistake == "thread":
        assert not caught[(128, 128)]               # one element per thread below 512 x 512
    zeros = np.zeros((512, 512))
    assert peak_model(zeros, mistake) != 0


# ---- the cut, restated with its mistakes -----------------------------------------------------------------------------------------
def surface_model(oracle, ref, tgt, cut=lambda mag: mag > R.EPSILON):
    """correlate_single's surface with the oracle's own transforms and the cross power of complex.rs:27-44 written out"""
    rows, cols = ref.shape
    fr, fc = R._next_pow2(rows), R._next_pow2(cols)
    wy, wx = R.hann_periodic(rows), R.hann_periodic(cols)
    a, b = oracle.fft2d(R._windowed(ref, wy, wx, fr, fc)), oracle.fft2d(R._windowed(tgt, wy, wx, fr, fc))
    pr, pi = a.real * b.real + a.imag * b.imag, a.imag * b.real - a.real * b.imag
    mag = np.sqrt(pr * pr + pi * pi)
    keep = cut(mag)
    safe = np.where(keep, mag, 1.0)
    cross = np.where(keep, pr / safe, 0.0) + 1j * np.where(keep, pi / safe, 0.0)
    return oracle.fft2d(cross, inverse=True).real, mag


@pytest.mark.parametrize("name,ref,tgt", PA.cut_pairs(), ids=lambda v: v if isinstance(v, str) else "")
def test_cut_pairs_catch_a_cut_that_has_moved_but_not_its_equality(oracle, name, ref, tgt):
    want = oracle.correlate_single(ref, tgt, want_surface=True)[3]
    got, mag = surface_model(oracle, ref, tgt)
    assert np.abs(got - want).max() <= 1e-15                     # (numpy's cos and libm's may differ in the window's last bit)
    lo, hi = PA.CUT_FRACTION_BOUNDS
    assert lo <= float((mag <= R.EPSILON).mean()) <= hi
    for wrong in (lambda m: m > 1.1 * R.EPSILON, lambda m: m > 0.9 * R.EPSILON, lambda m: m * m > R.EPSILON, lambda m: m >= 0.0):
        with np.errstate(invalid="ignore", divide="ignore"):
            assert not np.array_equal(surface_model(oracle, ref, tgt, wrong)[0], got)
    # `>=` in place of `>` differs for a bin whose magnitude IS the double 1e-15, and only there: none of 16384 continuous
    # magnitudes is, so these planes cannot tell the two apart (nor can a constructed one: the simplest spectrum, a single windowed
    # pixel per plane, has |A conj(B)| = |a b|, a product of two f32 with at most 48 significant bits -- 1e-15 needs 52)
    assert not (mag == R.EPSILON).any()
    assert same_bits(surface_model(oracle, ref, tgt, lambda m: m >= R.EPSILON)[0], got)
    m, e = np.frexp(R.EPSILON)
    assert int(m * 2 ** 53) % 2 ** 5 != 0
