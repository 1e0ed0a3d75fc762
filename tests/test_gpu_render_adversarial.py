"""The preview / tile-pyramid / IPC renderers (csrc/render.hip) on one MI355X against the numpy restatement written from the Rust
(render_restatement.py; pinned against the C oracle by test_render_restatement_cpu.py) on the adversarial fixtures of render_cases.py:
rounding ties of v * 255 and of (v - gmin) * inv_range, preview dimensions that round from x.5, previews narrower than one lane,
2 x 2 cells whose f64 sum depends on the order, values on the 1e-7 validity cut, saturating percentile ranks, 1-pixel sliver tiles.

Every comparison is exact: bytes, bounds, level tables, preview dimensions.  The one exception is the sign of a zero data_min /
data_max in the IPC header, which is unspecified (include/astroburst_hip.h): the two fixtures that have one compare those two
fields by value."""
import struct

import numpy as np
import pytest

import render_cases as rc
import render_restatement as R
from astroburst_amd import AstroBurstError, _lib
from astroburst_amd.core import ImageStats, StfParams

pytestmark = pytest.mark.gpu

STF = [StfParams(*p) for p in rc.STF]
STATS = [ImageStats(**s) for s in rc.STATS]
OFFSETS = (0, 1, 3)   # floats past a 256-byte aligned allocation: 1 and 3 sit off every 8- and 16-byte boundary


def _dev(a, offset=0):
    """the array on the device; offset > 0: at a pointer `offset` elements past a 256-byte aligned allocation"""
    import torch
    a = np.array(a, copy=True, order="C")   # (the cached fixtures are read-only)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() == buf.data_ptr() + offset * a.itemsize and view.is_contiguous()
    return view


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_bytes(got, want, what):
    got = _host(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} != {want.shape}"
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: got {got.ravel()[bad[0]]} want {want.ravel()[bad[0]]}"


def assert_ipc(got, want: bytes, by_value, what):
    got = _host(got).tobytes()
    assert len(got) == len(want) and got[:8] == want[:8], (what, struct.unpack("<II", got[:8]), struct.unpack("<II", want[:8]))
    g, w = struct.unpack("<ff", got[8:16]), struct.unpack("<ff", want[8:16])
    assert g == w if by_value else got[8:16] == want[8:16], (what, g, w)
    assert_bytes(np.frombuffer(got[16:], np.uint8), np.frombuffer(want[16:], np.uint8), what)


def _previews(ctx, planes, max_dim, what):
    """plain and STF previews of host planes and of device planes at every offset, the first device form twice"""
    want = R.render_rgb_preview(*planes, max_dim)
    want_stf = R.render_rgb_preview(*planes, max_dim, rc.STF, rc.STATS_NS)
    assert ctx.preview_dims(planes[0].shape[0], planes[0].shape[1], max_dim) == want.shape[:2], what
    assert_bytes(ctx.render_rgb_preview(*planes, max_dim), want, f"{what} host")
    assert_bytes(ctx.render_rgb_preview(*planes, max_dim, STF, STATS), want_stf, f"{what} host stf")
    for off in OFFSETS:
        dev = [_dev(p, off) for p in planes]
        got = ctx.render_rgb_preview(*dev, max_dim)
        assert got.is_cuda
        assert_bytes(got, want, f"{what} device + {off}")
        assert_bytes(ctx.render_rgb_preview(*dev, max_dim, STF, STATS), want_stf, f"{what} device + {off} stf")
        if off == 0:
            assert_bytes(ctx.render_rgb_preview(*dev, max_dim), want, f"{what} device, second call")


def _rgb_pyramids(ctx, planes, ts, what, offsets=OFFSETS):
    want, wl = R.generate_tile_pyramid_rgb(*planes, ts)
    want_stf, _ = R.generate_tile_pyramid_rgb(*planes, ts, rc.STF, rc.STATS_NS)
    got, gl = ctx.generate_tile_pyramid_rgb(*planes, ts)
    assert gl == wl, what
    assert_bytes(got, want, f"{what} host")
    assert_bytes(ctx.generate_tile_pyramid_rgb(*planes, ts, STF, STATS)[0], want_stf, f"{what} host stf")
    for off in offsets:
        dev = [_dev(p, off) for p in planes]
        assert_bytes(ctx.generate_tile_pyramid_rgb(*dev, ts)[0], want, f"{what} device + {off}")
        assert_bytes(ctx.generate_tile_pyramid_rgb(*dev, ts, STF, STATS)[0], want_stf, f"{what} device + {off} stf")
    assert_bytes(ctx.generate_tile_pyramid_rgb(*planes, ts)[0], want, f"{what} host, second call")


def _mono_pyramid(ctx, a, ts, what, offsets=OFFSETS):
    want, wl, wb = R.generate_tile_pyramid(a, ts)
    got, gl, gb = ctx.generate_tile_pyramid(a, ts)
    assert gl == wl and gb == wb, (what, gb, wb)
    assert_bytes(got, want, f"{what} host")
    for off in offsets:
        got, gl, gb = ctx.generate_tile_pyramid(_dev(a, off), ts)
        assert gl == wl and gb == wb, (what, off, gb, wb)
        assert_bytes(got, want, f"{what} device + {off}")
    got, _, gb = ctx.generate_tile_pyramid(a, ts)
    assert gb == wb
    assert_bytes(got, want, f"{what} host, second call")
    return want


# ---- quantisation ties ------------------------------------------------------------------------------------------------------------
def test_quantisation_ties_truncating_previews(ctx):
    planes = rc.quantisation_planes()
    _previews(ctx, planes, 64, "fits")          # render_rgb: every value once
    _previews(ctx, planes, 20, "scaled")
    # the fixture does tell truncation from rounding on the device's own bytes: the fine level of a one-tile pyramid is the rounded map
    rows, cols = rc.QUANT_SHAPE
    trunc = _host(ctx.render_rgb_preview(*planes, 64))
    rounded = _host(ctx.generate_tile_pyramid_rgb(*planes, 64)[0]).reshape(64, 64, 3)[:rows, :cols]
    assert (trunc != rounded).sum() >= 3 * 255


@pytest.mark.parametrize("ts", [64, 8, 3])
def test_quantisation_ties_rounding_tiles(ctx, ts):
    _rgb_pyramids(ctx, rc.quantisation_planes(), ts, f"ts {ts}")


@pytest.mark.parametrize("case", rc.MONO_PLANES, ids=[c[0] for c in rc.MONO_PLANES])
def test_mono_tile_ties(ctx, case):
    a = case[1]()
    assert case[2](), case[0]
    assert ctx.tile_percentile_bounds(a) == R.percentile_bounds(a)
    _mono_pyramid(ctx, a, rc.MONO_TS, case[0])
    _mono_pyramid(ctx, a, 64, case[0] + ", one tile", offsets=(0,))


# ---- preview geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.GEOMETRY, ids=rc.GEOMETRY_IDS)
def test_preview_geometry(ctx, case):
    rows, cols, max_dim, dims, _, _ = case
    assert rc.geometry_populates(case)
    assert ctx.preview_dims(rows, cols, max_dim) == dims
    _previews(ctx, rc.index_planes(rows, cols), max_dim, f"{rows}x{cols}@{max_dim}")


# ---- downsample -------------------------------------------------------------------------------------------------------------------
def test_downsample_2x(ctx):
    assert rc.downsample_populates()
    for name, a in rc.downsample_planes():
        want = R.downsample_2x(a)
        for got in [ctx.tile_downsample_2x(a)] + [ctx.tile_downsample_2x(_dev(a, off)) for off in OFFSETS] + [ctx.tile_downsample_2x(a)]:
            got = _host(got)
            assert got.shape == want.shape and got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, got, want)


# ---- percentile bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", rc.PCT_PAIRS, ids=rc.PCT_IDS)
def test_percentile_bounds(ctx, pct):
    planes = [(n, a) for n, a, _ in rc.PERCENTILE_PLANES] + [(n, make()) for n, make, _ in rc.MONO_PLANES]
    for name, a in planes:
        want = R.percentile_bounds(a, *pct)
        assert ctx.tile_percentile_bounds(a, *pct) == want, (name, "host")
        for off in OFFSETS:
            assert ctx.tile_percentile_bounds(_dev(a, off), *pct) == want, (name, "device", off)
        assert ctx.tile_percentile_bounds(a, *pct) == want, (name, "host, second call")


# ---- IPC --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.IPC_CASES, ids=rc.IPC_IDS)
def test_ipc(ctx, case):
    name, _, max_dim, pred, by_value = case
    a = rc.ipc_plane(case)
    want = R.ipc_encode(a, max_dim)
    assert pred(want), name
    assert_ipc(ctx.ipc_encode_with_header(a, max_dim), want, by_value, f"{name} host")
    for off in OFFSETS:
        got = ctx.ipc_encode_with_header(_dev(a, off), max_dim)
        assert got.is_cuda
        assert_ipc(got, want, by_value, f"{name} device + {off}")
    assert_ipc(ctx.ipc_encode_with_header(a, max_dim), want, by_value, f"{name} host, second call")


# ---- pyramids ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.PYRAMIDS, ids=rc.PYRAMID_IDS)
def test_pyramids(ctx, case):
    rows, cols, ts, nl, _, _ = case
    assert rc.pyramid_populates(case)
    for ch in (1, 3):
        assert ctx.tile_pyramid_layout(rows, cols, ts, ch) == R.pyramid_layout(rows, cols, ts, ch)
    assert ctx.tile_compute_num_levels(cols, rows, ts) == nl
    offsets = (0,) if ts == 1024 else OFFSETS          # (3 MiB of tiles per call there)
    _mono_pyramid(ctx, rc.mono_plane(rows, cols), ts, "mono", offsets)
    _rgb_pyramids(ctx, rc.rgb_planes(rows, cols), ts, "rgb", offsets)


def test_pyramid_after_trim(ctx):
    """the render workspace (the 2x chain's ping-pong buffer) is released by trim() and allocated again by the next pyramid"""
    rows, cols, ts = 257, 129, 2
    a, planes = rc.mono_plane(rows, cols), rc.rgb_planes(rows, cols)
    want_mono = R.generate_tile_pyramid(a, ts)[0]
    want_rgb = R.generate_tile_pyramid_rgb(*planes, ts)[0]
    dev, dev3 = _dev(a), [_dev(p) for p in planes]
    for _ in range(2):
        assert_bytes(ctx.generate_tile_pyramid(dev, ts)[0], want_mono, "mono")
        assert_bytes(ctx.generate_tile_pyramid_rgb(*dev3, ts)[0], want_rgb, "rgb")
        ctx.trim()
    assert_bytes(ctx.generate_tile_pyramid_rgb(*dev3, ts)[0], want_rgb, "rgb after trim")
    assert_bytes(ctx.generate_tile_pyramid(a, ts)[0], want_mono, "mono, host plane after trim")


# ---- output addresses -------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def _refused(call, n):
    """`call(out)` with a device buffer of n bytes at an address that is 1 past a multiple of 4: AB_ERR_INVALID, buffer untouched"""
    import torch
    for shift in (1, 2, 3):
        buf = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = buf[shift:shift + n]
        assert out.data_ptr() % 4 == shift and out.is_contiguous()
        with pytest.raises(AstroBurstError) as e:
            call(out)
        assert e.value.code == _lib.AB_ERR_INVALID, e.value
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), f"shift {shift}: the refused call wrote into the buffer"
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")   # and the aligned `out` is used and returned
    got = call(buf[4:4 + n])
    assert got.data_ptr() == buf.data_ptr() + 4 and bool((buf[:4] == SENTINEL).all()) and bool((buf[4 + n:] == SENTINEL).all())
    return got


def test_misaligned_device_output_is_refused_untouched(ctx):
    planes = rc.index_planes(37, 53)
    dev3 = [_dev(p) for p in planes]
    ph, pw = R.preview_dims(37, 53, 20)[:2]
    got = _refused(lambda out: ctx.render_rgb_preview(*dev3, 20, out=out), ph * pw * 3)
    assert_bytes(got.view(ph, pw, 3), R.render_rgb_preview(*planes, 20), "preview into out=")
    a = rc.index_plane(37, 53)
    got = _refused(lambda out: ctx.ipc_encode_with_header(_dev(a), 20, out=out), 16 + 4 * ph * pw)
    assert_ipc(got, R.ipc_encode(a, 20), False, "ipc into out=")
    m = rc.mono_plane(63, 32)
    want, _, wb = R.generate_tile_pyramid(m, 31)
    got = _refused(lambda out: ctx.generate_tile_pyramid(_dev(m), 31, out=out)[0], want.size)
    assert_bytes(got, want, "mono pyramid into out=")
    r3 = rc.rgb_planes(63, 32)
    want, _ = R.generate_tile_pyramid_rgb(*r3, 31)
    got = _refused(lambda out: ctx.generate_tile_pyramid_rgb(*[_dev(p) for p in r3], 31, out=out)[0], want.size)
    assert_bytes(got, want, "rgb pyramid into out=")
    # a host `out` of any address is staged, and one of the wrong size or type never reaches the library
    host = np.full(ph * pw * 3 + 1, SENTINEL, np.uint8)
    assert_bytes(ctx.render_rgb_preview(*planes, 20, out=host[1:]).reshape(ph, pw, 3), R.render_rgb_preview(*planes, 20), "host out=")
    assert host[0] == SENTINEL
    with pytest.raises(AstroBurstError, match="contiguous uint8"):
        ctx.render_rgb_preview(*planes, 20, out=host)


# ---- level arithmetic (host only) -------------------------------------------------------------------------------------------------
def test_level_arithmetic(ctx):
    for m, ts in rc.LEVEL_ARGS:
        want = R.compute_num_levels(m, 1, ts)
        assert ctx.tile_compute_num_levels(m, 1, ts) == ctx.tile_compute_num_levels(1, m, ts) == want, (m, ts)
    levels, total = ctx.tile_pyramid_layout(1, 2 ** 31, 1, 1)
    assert len(levels) == 32 == _lib.MAX_TILE_LEVELS and (levels, total) == R.pyramid_layout(1, 2 ** 31, 1, 1)
    with pytest.raises(AstroBurstError) as e:
        ctx.tile_pyramid_layout(1, 2 ** 32, 1, 1)
    assert e.value.code == _lib.AB_ERR_INVALID and R.compute_num_levels(2 ** 32, 1, 1) == 33
    a = rc.mono_plane(8, 8)
    tiles, levels, bounds = ctx.generate_tile_pyramid(a, 4096)
    want, wl, wb = R.generate_tile_pyramid(a, 4096)
    assert levels == wl and bounds == wb
    assert_bytes(tiles, want, "tile_size 4096")
    with pytest.raises(AstroBurstError) as e:
        ctx.generate_tile_pyramid(a, 4097)
    assert e.value.code == _lib.AB_ERR_INVALID
    with pytest.raises(AstroBurstError) as e:
        ctx.generate_tile_pyramid_rgb(a, a, a, 4097)
    assert e.value.code == _lib.AB_ERR_INVALID
