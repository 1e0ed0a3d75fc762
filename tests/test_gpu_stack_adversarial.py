"""GPU parity of the kappa-sigma stacks on adversarial pixels (tests/stack_adversarial.py) against the CPU oracle.

The generated data of tests/test_gpu_stack.py sums exactly in every order and never puts a sample on a clip threshold, so it cannot
see a `<` written for `<=`, a sigma one ulp off, or a tree sum that misses the contract under cancellation.  These pixels can:

  T, E  exact arithmetic (ties on the threshold, edge pixels): every engine owes the oracle's values bit for bit and its rejected
        count (the one E pixel whose survivor sum is inexact is held to the W assertions).
  W, M  inexact sums, the moment switch: the exact engine and the workgroup-per-pixel kernel bit for bit; the default engine its
        per-pixel contract -- rejected count equal, every value within 1e-5 relative (no allowance for differing pixels: that
        describes natural data).  Each set holds pixels of one side of the wave-uniform raw / centred moment switch.
  B     the batch stack: bit for bit, per-frame rejection counts equal.

Every frame count in stack_adversarial.N_LIST (both sides of every kernel class edge), host and device planes, a pixel count that is
a multiple of 16 and one that is not, the row-band, single-vector, median-combine and one-rank frame-sharded entry points.
"""
import numpy as np
import pytest
import torch

import stack_adversarial as sa
from astroburst_amd.core import BatchStackConfig

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(params=["fast", "exact", "deep"])
def engine(request, ctx, ctx_exact, ctx_deep):
    """(context, bit_exact from n frames on): the default engine (bit for bit beyond 4096 frames: the workgroup-per-pixel kernel's
    ascending sums), AB_STACK_EXACT=1 (bit for bit everywhere, sigma-inf pixels included), and the default engine with the
    workgroup-per-pixel kernel from 65 frames on"""
    return {"fast": (ctx, 4097), "exact": (ctx_exact, 0), "deep": (ctx_deep, 65)}[request.param]


@pytest.fixture(scope="module")
def comm(ctx):
    import astroburst_amd as ab
    c = ab.Comm(ctx, ab.Comm.unique_id(), 1, 0)
    assert (c.rank, c.size) == (0, 1)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a, F32))
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def assert_bits(got, want, where=""):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        idx = np.argwhere(g != w)[:5]
        got, want = np.asarray(got), np.asarray(want)
        raise AssertionError(f"{where}: {(g != w).sum()} of {g.size} differ; first {idx.tolist()}: "
                             f"{[(got[tuple(i)], want[tuple(i)]) for i in idx]}")


def _strict_mask(pixels, shape):
    """per plane position: True where the pixel's arithmetic is exact (T, E but the tagged one, B)"""
    P = len(pixels)
    flags = np.array([p.family in "TEB" and not p.meta.get("inexact", False) for p in pixels])
    return flags[np.arange(int(np.prod(shape))) % P].reshape(shape)


def check_stack(got, want, rej, wrej, pixels, bit_exact, where, inf_bits=False):
    """T/E positions bit for bit on every engine; the rest bit for bit where bit_exact, within the contract elsewhere.  The E pixels
    whose sigma overflows (+-3e38 kept next to small samples, see stack_adversarial.family_E) are outside any relative contract: their
    count is held everywhere, their bits only where inf_bits (AB_STACK_EXACT=1)."""
    got = np.asarray(got)
    assert rej == wrej, f"{where}: rejected {rej} != oracle {wrej}"
    P = len(pixels)
    loose = np.array([p.meta.get("sigma_inf", False) for p in pixels])[np.arange(got.size) % P].reshape(got.shape)
    if inf_bits:
        loose[:] = False
    assert np.isfinite(got[loose]).all(), where
    if bit_exact:
        assert_bits(got[~loose], want[~loose], where)
        return
    strict = _strict_mask(pixels, got.shape)
    assert_bits(got[strict], want[strict], where + " (exact-arithmetic pixels)")
    rest = ~strict & ~loose
    np.testing.assert_allclose(got[rest], want[rest], rtol=1e-5, atol=0, err_msg=where)


@pytest.mark.parametrize("family", ["T", "W", "M", "E"])
@pytest.mark.parametrize("n", sa.N_LIST)
def test_adversarial_stack(engine, oracle, n, family):
    """stack_sigma_clip over host planes and torch device planes, both layouts"""
    ctx, exact_from = engine
    exact = n >= exact_from
    for fs in sa.fixture_sets(family, n):
        pixels = fs.all_pixels()
        for layout in ("mult16", "odd"):
            frames, _ = sa.pack(pixels, layout)
            want, wrej = oracle.stack_images(frames, fs.sl, fs.sh, fs.it)
            where = f"{family} n={n} {layout} sl={fs.sl} sh={fs.sh} it={fs.it}"
            got, rej = ctx.stack_sigma_clip(frames, fs.sl, fs.sh, fs.it)
            check_stack(got, want, rej, wrej, pixels, exact, where + " host", exact_from == 0)
            dev = [torch.from_numpy(f).cuda() for f in frames]
            got, rej = ctx.stack_sigma_clip(dev, fs.sl, fs.sh, fs.it)
            check_stack(got.cpu().numpy(), want, rej, wrej, pixels, exact, where + " device", exact_from == 0)


@pytest.mark.parametrize("n", sa.N_LIST)
def test_adversarial_row_band(ctx, ctx_exact, oracle, n):
    """stack_sigma_clip_rows: rows 1 .. 2 of a 3-row stack of the T, W, M and E pixels == those rows of the oracle's stack"""
    for c, exact in ((ctx, False), (ctx_exact, True)):
        for family in "TWME":
            for fs in sa.fixture_sets(family, n)[:2]:
                pixels = fs.all_pixels()
                frames, _ = sa.pack(pixels, "rows", rows=3)
                want, _ = oracle.stack_images(frames, fs.sl, fs.sh, fs.it)
                _, wrej = oracle.stack_images([f[1:3] for f in frames], fs.sl, fs.sh, fs.it)
                dev = [torch.from_numpy(f).cuda() for f in frames]
                band, rej = c.stack_sigma_clip_rows(dev, 1, 2, fs.sl, fs.sh, fs.it)
                # (the band's pixels are the same fixture pixels shifted by one row: the strict mask is of the band's own positions)
                rolled = [pixels[(k + frames[0].shape[1]) % len(pixels)] for k in range(len(pixels))]
                check_stack(band.cpu().numpy(), want[1:3], rej, wrej, rolled, exact, f"rows {family} n={n} it={fs.it}", exact)


@pytest.mark.parametrize("n", sa.N_LIST)
def test_adversarial_sigma_clip_combine(ctx, oracle, n):
    """sigma_clip_combine on single vectors: the first ties of each iteration and their twins, and the edge pixels, bit for bit"""
    fs_t = sa.fixture_sets("T", n)
    picks = []
    for iteration in (0, 1):
        for fs in fs_t:
            px = [p for p in fs.pixels if p.meta["iteration"] == iteration][:1]
            picks += [(fs, p) for p in px] + [(fs, p.twin) for p in px]
            if px:
                break
    fs_e = sa.fixture_sets("E", n)[0]
    picks += [(fs_e, p) for p in fs_e.pixels if not p.meta.get("inexact", False)][:6 if n > 1024 else 16]
    for fs, p in picks:
        got, rej = ctx.sigma_clip_combine(p.values, fs.sl, fs.sh, fs.it)
        want, wrej = oracle.stack_images([np.array([[x]], F32) for x in p.values], fs.sl, fs.sh, fs.it)
        assert rej == wrej, (p.name, rej, wrej)
        assert_bits(np.array([got], F32), want[0], p.name)


@pytest.mark.parametrize("n", sa.N_LIST)
def test_adversarial_median_combine(ctx, ctx_deep, oracle, n):
    """median_combine of the edge pixels (overflows, subnormals, -0.0, zero majorities, NaN / inf), both layouts, bit for bit"""
    pixels = [p for p in sa.fixture_sets("E", n)[0].pixels]
    for layout in ("mult16", "odd"):
        frames, _ = sa.pack(pixels, layout)
        want = oracle.median_combine(frames)
        for c in (ctx, ctx_deep):
            assert_bits(c.median_combine(frames), want, f"median n={n} {layout}")
            dev = [torch.from_numpy(f).cuda() for f in frames]
            assert_bits(c.median_combine(dev).cpu().numpy(), want, f"median n={n} {layout} device")


@pytest.mark.parametrize("n", sa.N_LIST)
def test_adversarial_batch_stack(ctx, ctx_deep, oracle, n):
    """sigma_clipped_mean_stack on z == kappa ties (rejected) and their one-ulp-inside (kept) and -outside twins: bit for bit, per-frame
    rejection counts equal; the default dispatch and the workgroup-per-pixel kernel"""
    sets = sa.fixture_sets("B", n)
    if n >= 8:
        assert sets
    for fs in sets:
        pixels = fs.all_pixels()
        for layout in ("mult16", "odd"):
            frames, _ = sa.pack(pixels, layout)
            want, wrej = oracle.sigma_clipped_mean_stack(frames, fs.sl, fs.sh, fs.it)
            for c in (ctx, ctx_deep):
                got, rej = c.sigma_clipped_mean_stack(frames, BatchStackConfig(fs.sl, fs.sh, fs.it))
                where = f"B n={n} {layout} sl={fs.sl} sh={fs.sh} it={fs.it}"
                assert rej == wrej, where
                assert_bits(got, want, where)


@pytest.mark.parametrize("n", sa.N_LIST)
def test_adversarial_frame_sharded(ctx, comm, oracle, n):
    """the one-rank frame-sharded stack (partial sums -> RCCL all-reduce -> divide) == the two-level oracle, T and E pixels bit for
    bit, W and M within the default engine's contract"""
    for family in "TWME":
        for fs in sa.fixture_sets(family, n)[:2]:
            pixels = fs.all_pixels()
            frames, _ = sa.pack(pixels, "mult16")
            s, cnt, wrej = oracle.stack_partial(frames, fs.sl, fs.sh, fs.it)
            want = np.where(cnt > 0, (s / np.maximum(cnt, 1)).astype(F32), F32(0))
            dev = [torch.from_numpy(f).cuda() for f in frames]
            out = torch.empty(frames[0].shape, device="cuda")
            _, rej = ctx.stack_sigma_clip_sharded(comm, dev, out, fs.sl, fs.sh, fs.it, want_rejected=True)
            check_stack(out.cpu().numpy(), want, rej, wrej, pixels, False, f"sharded {family} n={n} it={fs.it}")
