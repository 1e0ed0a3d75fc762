"""GPU parity of the shared-tap warp kernel (warp_kernel_shared, csrc/resample.hip) with the oracle, bit for bit (NaN where NaN),
every output pre-filled with a sentinel so that a pixel never written shows.

One lane of that kernel owns one output column and K consecutive output rows, groups are aligned to the band's first row, and a
wave either shares its source taps or runs the per-pixel body for each of its rows.  So per transform class (warp_shared_cases.py:
pure shift, small rotations with column crossings, rows that repeat or skip a source row, rows that do not sample beside rows that
do, and the transforms the routing keeps on the per-pixel kernel) every output shape runs as a whole warp on host and on device
planes, as row bands with row0 in {0, 1, 2, 3, rows - 1} and heights 1 .. 5 (1, K - 1, K, K + 1 for every K the kernel is built for:
groups start off the image's multiples of K and end ragged), and as ab_warp_image_rows_from_band on a copy of exactly the source rows
ab_warp_source_rows names -- the shared path may read no row beyond them.  That the classes are populated at these shapes is asserted
on the CPU (test_warp_shared_taps_predicate.py) and again here for the case's largest shape."""
import numpy as np
import pytest

import warp_shared_cases as wc
from test_gpu_resample_shapes import SENTINEL, assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def src():
    return wc.source()


@pytest.fixture(scope="module")
def src_dev(src):
    import torch
    return torch.from_numpy(src).cuda()


def bands_of(rows):
    return [(row0, n) for row0 in sorted({0, 1, 2, 3, rows - 1}) for n in range(1, 6) if row0 < rows and row0 + n <= rows]


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_shared_tap_warp_matches_the_oracle(ctx, oracle, src, src_dev, case):
    import torch
    name, make, must_share, must_not_share, is_routed = case
    for cols in wc.OUT_COLS:
        t = make((wc.POPULATED_AT[0], cols))
        assert wc.routed(t) == is_routed, (name, t)
        for K in wc.KS:  # the class the case is named for, from the kernel's coordinate expressions
            sharing, not_sharing = wc.counts(t, wc.SRC_DIMS, (wc.POPULATED_AT[0], cols), K)
            assert not (must_share is True) or sharing > 0, (name, cols, K)
            assert not (must_share is False and name.startswith("g")) or sharing == 0, (name, cols, K)
            assert not must_not_share or not_sharing > 0, (name, cols, K)
        for rows in wc.OUT_ROWS:
            t = make((rows, cols))
            what = f"{name} -> {rows} x {cols}"
            want = oracle.warp_image(src, t, rows, cols)
            got = ctx.warp_image(src, t, rows, cols, out=np.full((rows, cols), SENTINEL, np.float32))
            assert_same(got, want, wc.PIECE, f"warp {what}, host planes")
            got = ctx.warp_image(src_dev, t, rows, cols, out=torch.full((rows, cols), SENTINEL, device="cuda"))
            assert_same(got, want, wc.PIECE, f"warp {what}, device planes")
            # the band forms: every band writes its own rows of one sentinel-filled plane, compared after a single copy back
            bands = bands_of(rows)
            starts = np.cumsum([0] + [n for _, n in bands])
            plain = torch.full((int(starts[-1]), cols), SENTINEL, device="cuda")
            hulled = torch.full((int(starts[-1]), cols), SENTINEL, device="cuda")
            for (row0, n), at in zip(bands, starts):
                ctx.warp_image_rows(src_dev, t, rows, row0, plain[at:at + n])
                s0, sn = ctx.warp_source_rows(t, wc.SRC_DIMS[0], wc.SRC_DIMS[1], cols, row0, n)
                band = src_dev[s0:s0 + sn].clone() if sn else torch.empty((0, wc.SRC_DIMS[1]), device="cuda")
                ctx.warp_image_rows_from_band(band, s0, wc.SRC_DIMS[0], t, rows, row0, hulled[at:at + n])
            plain, hulled = plain.cpu().numpy(), hulled.cpu().numpy()
            for (row0, n), at in zip(bands, starts):
                assert_same(plain[at:at + n], want[row0:row0 + n], wc.PIECE, f"warp_image_rows {what}, rows [{row0}, {row0 + n})")
                assert_same(hulled[at:at + n], want[row0:row0 + n], wc.PIECE,
                            f"warp_image_rows_from_band {what}, rows [{row0}, {row0 + n}) from exactly their source rows")
