"""GPU parity of the share-first warp kernel (warp_kernel_shared, csrc/resample.hip, LABNOTES 37) with the oracle, bit for bit (NaN where
NaN) on sentinel-filled outputs, on the inputs test_gpu_warp_shared_taps.py does not reach: sources of K + 2 and K + 3 rows and of 3, 4
and 5 columns (the predicate's bounds are 0 or 1 there, and the host keeps the per-pixel kernel below 4 columns or K + 3 rows),
coordinates in (-1, 0) -- which truncate to 0 where the floor is -1 --, exactly on 0, 1 and src - 3, fractions of 1 - 1e-12, and
coordinates at 1e9, 3e9 and 1e150 (beyond the int range: everything outside, zeros).  Each offset without and with a rotation of
0.05 deg; whole warps on host and device planes, and row bands with row0 in {0, 1, 2, rows - 1} and heights 1 .. 5.  That these inputs
are routed to the kernel and reach its shared path is asserted on the CPU (test_warp_share_first_predicate.py)."""
import numpy as np
import pytest

import warp_share_first_cases as sf
import warp_shared_cases as wc
from test_gpu_resample_shapes import SENTINEL, assert_same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dims", sf.GPU_SOURCES, ids=[f"{r}x{c}" for r, c in sf.GPU_SOURCES])
def test_share_first_warp_matches_the_oracle(ctx, oracle, dims):
    import torch
    src = sf.gpu_source(dims)
    src_dev = torch.from_numpy(src).cuda()
    for t in sf.gpu_transforms(dims):
        for rows, cols in sf.GPU_OUT_DIMS:
            what = f"source {dims}, {t} -> {rows} x {cols}"
            want = oracle.warp_image(src, t, rows, cols)
            got = ctx.warp_image(src, t, rows, cols, out=np.full((rows, cols), SENTINEL, np.float32))
            assert_same(got, want, wc.PIECE, f"warp {what}, host planes")
            got = ctx.warp_image(src_dev, t, rows, cols, out=torch.full((rows, cols), SENTINEL, device="cuda"))
            assert_same(got, want, wc.PIECE, f"warp {what}, device planes")
            # every band writes its own rows of one sentinel-filled plane, compared after a single copy back
            bands = sf.bands_of(rows)
            starts = np.cumsum([0] + [n for _, n in bands])
            plane = torch.full((int(starts[-1]), cols), SENTINEL, device="cuda")
            for (row0, n), at in zip(bands, starts):
                ctx.warp_image_rows(src_dev, t, rows, row0, plane[at:at + n])
            plane = plane.cpu().numpy()
            for (row0, n), at in zip(bands, starts):
                assert_same(plane[at:at + n], want[row0:row0 + n], wc.PIECE, f"warp_image_rows {what}, rows [{row0}, {row0 + n})")
