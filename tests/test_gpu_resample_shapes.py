"""GPU parity of warp / shift / resample over every LAUNCH-SHAPE class and every class of the sampler, bit for bit against the oracle
(which test_resample_restatement.py pins to an independent numpy restatement of the Rust).

warp_kernel takes 512 output columns per workgroup, shift_kernel and resample_kernel 256; xcd_band_piece (csrc/resample.hip) re-deals
the workgroups over eight contiguous runs whenever the pieces per row are not a multiple of 8.  The per-function files stop at two
pieces per row (16 for resample), so a re-deal that wrote a piece twice and another never would pass them.  Here: pieces per row
g in {1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 33}, the last piece ragged (g * piece - 5 columns) and full, rows in {1, 7, 64, 67, 1031}
(total pieces a multiple of 8 and not, eight runs of unequal length), host planes and device planes, every output pre-filled with a
sentinel so that a piece never written shows, and the row-band forms (whose grid has the band's rows, not the output's: another
re-deal for the same pixels).  A failure names the first differing (y, x) and the piece it lies in.
(Host planes are staged through a device buffer of the library's own: an unwritten piece shows there as stale values, on device planes
as the sentinel.)

The edge cases (tests/resample_cases.py) each assert from the restatement's coordinates that the class they are named for is
populated."""
import numpy as np
import pytest

import resample_cases as rc

pytestmark = pytest.mark.gpu

SENTINEL = -1.0
PIECES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 33)
ROWS = (1, 7, 64, 67, 1031)


def assert_same(got, want, piece, what):
    """bit for bit (NaN where NaN); the message names the first differing pixel, its piece and how many pixels were never written"""
    if hasattr(got, "cpu"):
        got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want, equal_nan=True):
        return
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    y, x = (int(v) for v in np.argwhere(bad)[0])
    pieces = sorted({(int(py), int(px) // piece) for py, px in np.argwhere(bad)[:100000]})
    raise AssertionError(f"{what}: {int(bad.sum())} pixels differ, first at (y={y}, x={x}) in piece {x // piece} of its row "
                         f"(got {got[y, x]!r}, want {want[y, x]!r}); {int((bad & (got == SENTINEL)).sum())} of them still hold the "
                         f"sentinel (never written); pieces (row, piece) touched: {pieces[:12]}{' ...' if len(pieces) > 12 else ''}")


@pytest.fixture(scope="module")
def base():
    """one positive random plane the sweep cuts its sources from (sampled pixels are then non-zero, untouched ones 0.0)"""
    return np.random.default_rng(11).uniform(1.0, 2.0, (ROWS[-1] + 8, PIECES[-1] * 512 + 3)).astype(np.float32)


def bands_of(rows):
    """(row0, nrows): row0 in {0, 1, rows - 1, a middle band}"""
    out = {(0, min(rows, 3)), (rows - 1, 1), (rows // 3, max(rows // 2, 1))}
    if rows > 1:
        out.add((1, min(rows - 1, 9)))
    return sorted(out)


def run_warp(ctx, oracle, src, t, out_dims, what, bands=True):
    """whole warp on host and device planes + the band forms on the device, all against the oracle"""
    import torch
    rows, cols = out_dims
    want = oracle.warp_image(src, t, rows, cols)
    got = ctx.warp_image(src, t, rows, cols, out=np.full((rows, cols), SENTINEL, np.float32))
    assert_same(got, want, 512, f"warp {what} -> {rows} x {cols}, host planes")
    src_d = torch.from_numpy(src).cuda()
    got = ctx.warp_image(src_d, t, rows, cols, out=torch.full((rows, cols), SENTINEL, device="cuda"))
    assert_same(got, want, 512, f"warp {what} -> {rows} x {cols}, device planes")
    for row0, n in (bands_of(rows) if bands else ()):
        band = ctx.warp_image_rows(src_d, t, rows, row0, torch.full((n, cols), SENTINEL, device="cuda"))
        assert_same(band, want[row0:row0 + n], 512, f"warp_image_rows {what} -> rows [{row0}, {row0 + n}) of {rows} x {cols}")
    return want


def run_shift(ctx, oracle, src, dy, dx, what):
    import torch
    want = oracle.shift_image_subpixel(src, dy, dx)
    got = ctx.shift_image_subpixel(src, dy, dx, out=np.full(src.shape, SENTINEL, np.float32))
    assert_same(got, want, 256, f"shift {what} {src.shape}, host planes")
    got = ctx.shift_image_subpixel(torch.from_numpy(src).cuda(), dy, dx, out=torch.full(src.shape, SENTINEL, device="cuda"))
    assert_same(got, want, 256, f"shift {what} {src.shape}, device planes")
    return want


def run_resample(ctx, oracle, src, dst, what):
    import torch
    want = oracle.resample_image(src, *dst)
    got = ctx.resample_image(src, *dst, out=np.full(dst, SENTINEL, np.float32))
    assert_same(got, want, 256, f"resample {what} {src.shape} -> {dst}, host planes")
    got = ctx.resample_image(torch.from_numpy(src).cuda(), *dst, out=torch.full(dst, SENTINEL, device="cuda"))
    assert_same(got, want, 256, f"resample {what} {src.shape} -> {dst}, device planes")
    return want


# ---- the launch shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", PIECES)
def test_warp_every_piece_of_every_launch_shape(ctx, oracle, base, g):
    """source (rows + 8) x (cols + 3); sx = 0.9999 x + 2.5 and sy = y + 1.25 + 4 x / cols stay inside it for every output pixel, with
    both fractions changing along a row: every pixel of every piece is sampled, so none may be left at 0.0 either"""
    for cols in (512 * g - 5, 512 * g):
        for rows in ROWS:
            src = np.ascontiguousarray(base[:rows + 8, :cols + 3])
            t = (0.9999, 0.0, 2.5, 4.0 / cols, 1.0, 1.25)
            want = run_warp(ctx, oracle, src, t, (rows, cols), f"g = {g}")
            assert (want != 0.0).all()                                  # (of the oracle's plane: the sweep leaves no piece idle)


@pytest.mark.parametrize("g", PIECES)
def test_shift_every_piece_of_every_launch_shape(ctx, oracle, base, g):
    for cols in (256 * g - 5, 256 * g):
        for rows in ROWS:
            src = np.ascontiguousarray(base[:rows, :cols])
            want = run_shift(ctx, oracle, src, 0.3, -1.7, f"g = {g}")
            assert (want[:, 2:] != 0.0).all()                           # sx = x - 1.7 < -0.5 for x in {0, 1} only


@pytest.mark.parametrize("g", PIECES)
def test_resample_every_piece_of_every_launch_shape(ctx, oracle, base, g):
    for cols in (256 * g - 5, 256 * g):
        for rows in ROWS:
            src = np.ascontiguousarray(base[:rows + 3, :(cols * 3) // 4 + 2])
            want = run_resample(ctx, oracle, src, (rows, cols), f"g = {g}")
            assert (want != 0.0).all()


# ---- the sampler's classes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.WARP_CASES, ids=[c[0] for c in rc.WARP_CASES])
def test_warp_sampler_classes(ctx, oracle, case):
    name, src, t, out, _ = case
    ok, classes = rc.warp_populates(case)
    assert ok, (name, classes)
    run_warp(ctx, oracle, rc.pattern(*src), t, out, name)


@pytest.mark.parametrize("case", rc.SHIFT_CASES, ids=[c[0] for c in rc.SHIFT_CASES])
def test_shift_sampler_classes(ctx, oracle, case):
    name, src, (dy, dx), _ = case
    ok, classes = rc.shift_populates(case)
    assert ok, (name, classes)
    run_shift(ctx, oracle, rc.pattern(*src), dy, dx, name)


@pytest.mark.parametrize("case", rc.RESAMPLE_CASES, ids=[c[0] for c in rc.RESAMPLE_CASES])
def test_resample_sampler_classes(ctx, oracle, case):
    name, src, dst, _ = case
    ok, classes = rc.resample_populates(case)
    assert ok, (name, classes)
    img = rc.pattern(*src)
    img[src[0] // 2, src[1] // 3] = np.nan
    run_resample(ctx, oracle, img, dst, name)


def test_warp_classes_across_many_pieces(ctx, oracle, base):
    """a 1 degree / scale 0.9 rotation about the centre of a plane 9 pieces wide (all four borders crossed): the clamped and the
    unclamped footprints, pixels outside and the re-deal in one launch (the class counts from the restatement's coordinates)"""
    import resample_restatement as rs
    src_dims, out = (300, 4000), (331, 4603)
    t = rc.about_centre(1.0, 0.9, src_dims, out)
    sx, sy, inside = rs.warp_coords(t, src_dims[0], src_dims[1], out[1], 0, out[0])
    k = rs.sampler_classes(sx, sy, inside, *src_dims)
    assert min(k["outside"], k["ix_first"], k["ix_last"], k["iy_first"], k["iy_last"], k["waves_unclamped"], k["waves_clamped_mixed"],
               k["waves_partly_outside"]) > 0, k
    src = np.ascontiguousarray(base[:300, :4000])
    src[150:153, 2000:2040] = np.nan
    run_warp(ctx, oracle, src, t, out, "1 deg across 9 pieces")
