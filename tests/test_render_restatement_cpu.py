"""The numpy restatement of the preview / tile-pyramid / IPC renderers (render_restatement.py, written from the Rust) against the C
oracle (oracle/orc_render.c) on the adversarial fixtures of render_cases.py, byte for byte -- and every fixture's predicate.

The single exception to byte equality is the header of the two zero-sign IPC fixtures: the sign of a zero data_min / data_max is
unspecified (include/astroburst_hip.h), so those two fields are compared by value.

What this found: orc_tile_percentile_bounds converted the rank with a plain C cast, which is undefined for a negative, NaN or
too-large product; on x86-64 a pct of -0.25 or NaN gave rank n - 1 where the reference's saturating `as usize` gives 0, and a
pct of 1e30 gave rank 0 where the reference gives n - 1.  The cases "-0.25,0.999", "nan,nan" and "0.001,1e30" of
test_oracle_percentile_bounds fail without the saturating conversion, and only those."""
import struct

import numpy as np
import pytest

import render_cases as rc
import render_restatement as R

F32 = np.float32


def _stf(oracle):
    return [oracle.StfParams(*p) for p in rc.STF], [oracle.ImageStats(**s) for s in rc.STATS]


def _same_ipc(got: bytes, want: bytes, by_value: bool, what):
    assert len(got) == len(want), what
    assert got[:8] == want[:8], what
    if by_value:
        assert struct.unpack("<ff", got[8:16]) == struct.unpack("<ff", want[8:16]), what
    else:
        assert got[8:16] == want[8:16], (what, struct.unpack("<ff", got[8:16]), struct.unpack("<ff", want[8:16]))
    assert got[16:] == want[16:], what


# ---- the fixtures test what they claim --------------------------------------------------------------------------------------------
def test_every_fixture_populates_its_edge():
    assert rc.quantisation_populates()
    for name, _, pred in rc.MONO_PLANES:
        assert pred(), name
    for case in rc.GEOMETRY:
        assert rc.geometry_populates(case), case
    assert rc.last_lane_pixels() == {1, 2, 3, 4}
    assert rc.downsample_populates()
    for name, plane, pred in rc.PERCENTILE_PLANES:
        assert pred(plane), name
    assert rc.saturating_ranks_populate()
    for case in rc.IPC_CASES:
        assert case[3](R.ipc_encode(rc.ipc_plane(case), case[2])), case[0]
    for case in rc.PYRAMIDS:
        assert rc.pyramid_populates(case), case


def test_the_rust_conversions():
    assert [R.rust_round(v) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 0.49999999999999994, 2.4999999999999996, 4503599627370497.0)] == \
        [1.0, 2.0, 3.0, -1.0, -3.0, 0.0, 2.0, 4503599627370497.0]
    assert [R.sat_usize(v) for v in (float("nan"), -0.25, -1e300, 0.999, 999.0, 1e30, float("inf"))] == \
        [0, 0, 0, 0, 999, 2 ** 64 - 1, 2 ** 64 - 1]
    x = np.array([0.5, 1.5, 2.5, -0.5, 0.49999997, 8388607.5, np.inf, np.nan], F32)
    got = R.round_half_away(x)
    assert list(got[:7]) == [1.0, 2.0, 3.0, -1.0, 0.0, 8388608.0, np.inf] and np.isnan(got[7])
    assert list(R.as_u8(np.array([-1.0, -0.0, 0.99, 254.99, 255.0, 1e9, np.inf, -np.inf, np.nan], F32))) == [0, 0, 0, 254, 255, 255, 255, 0, 0]
    c = R.clamp_f32(np.array([np.nan, -0.0, -1.0, 2.0], F32), 0.0, 1.0)
    assert np.isnan(c[0]) and np.signbit(c[1]) and list(c[1:]) == [0.0, 0.0, 1.0]


def test_the_two_find_minmax_branches_differ_on_the_named_plane(oracle):
    a = rc.AVX2_PLANE
    assert R.find_minmax_portable(a) == (-3.0, F32(1e-8))
    assert R.find_minmax_avx2(a) == (-np.inf, np.inf)
    assert R.percentile_bounds(a, fallback=R.find_minmax_avx2) != R.percentile_bounds(a)
    assert oracle.tile_percentile_bounds(a) == R.percentile_bounds(a)          # the project takes the portable branch
    b = np.array([[np.inf, -1.0, 2.0]], F32)                                    # fewer than eight: both branches test is_finite
    assert R.find_minmax_avx2(b) == R.find_minmax_portable(b) == (-1.0, 2.0)


# ---- oracle == restatement --------------------------------------------------------------------------------------------------------
def test_oracle_quantisation(oracle):
    r, g, b = rc.quantisation_planes()
    stf, st = _stf(oracle)
    rows, cols = rc.QUANT_SHAPE
    for max_dim in (64, 20):
        assert np.array_equal(oracle.render_rgb_preview(r, g, b, max_dim), R.render_rgb_preview(r, g, b, max_dim))
        assert np.array_equal(oracle.render_rgb_preview(r, g, b, max_dim, stf, st), R.render_rgb_preview(r, g, b, max_dim, rc.STF, rc.STATS_NS))
    full = R.render_rgb_preview(r, g, b, 64)
    tiles, levels = R.generate_tile_pyramid_rgb(r, g, b, 64)
    rounded = tiles.reshape(64, 64, 3)[:rows, :cols]
    assert len(levels) == 1 and (full != rounded).sum() >= 3 * 255             # every tie, in every channel
    for ts in (64, 8):
        got, gl = oracle.generate_tile_pyramid_rgb(r, g, b, ts)
        want, wl = R.generate_tile_pyramid_rgb(r, g, b, ts)
        assert gl == wl and np.array_equal(got, want)
        got, _ = oracle.generate_tile_pyramid_rgb(r, g, b, ts, stf, st)
        want, _ = R.generate_tile_pyramid_rgb(r, g, b, ts, rc.STF, rc.STATS_NS)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("case", rc.MONO_PLANES, ids=[c[0] for c in rc.MONO_PLANES])
def test_oracle_mono_tiles(oracle, case):
    a = case[1]()
    got, gl, gb = oracle.generate_tile_pyramid(a, rc.MONO_TS)
    want, wl, wb = R.generate_tile_pyramid(a, rc.MONO_TS)
    assert gb == wb and gl == wl and len(wl) == 3
    assert np.array_equal(got, want)
    fine = want[wl[2]["offset"]:].reshape(4, 4, rc.MONO_TS, rc.MONO_TS)          # the packing against one render_tile at a time
    for ty, tx in ((0, 0), (2, 1), (3, 3)):
        assert np.array_equal(fine[ty, tx], R.render_tile(a, tx, ty, rc.MONO_TS, *wb)), (ty, tx)


@pytest.mark.parametrize("case", rc.GEOMETRY, ids=rc.GEOMETRY_IDS)
def test_oracle_preview_geometry(oracle, case):
    rows, cols, max_dim, dims, _, _ = case
    assert oracle.preview_dims(rows, cols, max_dim) == dims == R.preview_dims(rows, cols, max_dim)[:2]
    r, g, b = rc.index_planes(rows, cols)
    stf, st = _stf(oracle)
    assert np.array_equal(oracle.render_rgb_preview(r, g, b, max_dim), R.render_rgb_preview(r, g, b, max_dim))
    assert np.array_equal(oracle.render_rgb_preview(r, g, b, max_dim, stf, st), R.render_rgb_preview(r, g, b, max_dim, rc.STF, rc.STATS_NS))


def test_oracle_downsample(oracle):
    for name, a in rc.downsample_planes():
        got, want = oracle.tile_downsample_2x(a), R.downsample_2x(a)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("pct", rc.PCT_PAIRS, ids=rc.PCT_IDS)
def test_oracle_percentile_bounds(oracle, pct):
    for name, a, _ in rc.PERCENTILE_PLANES:
        assert oracle.tile_percentile_bounds(a, *pct) == R.percentile_bounds(a, *pct), name
    for name, make, _ in rc.MONO_PLANES:
        assert oracle.tile_percentile_bounds(make(), *pct) == R.percentile_bounds(make(), *pct), name


@pytest.mark.parametrize("case", rc.IPC_CASES, ids=rc.IPC_IDS)
def test_oracle_ipc(oracle, case):
    a = rc.ipc_plane(case)
    _same_ipc(oracle.ipc_encode_with_header(a, case[2]), R.ipc_encode(a, case[2]), case[4], case[0])


@pytest.mark.parametrize("case", rc.PYRAMIDS, ids=rc.PYRAMID_IDS)
def test_oracle_pyramids(oracle, case):
    rows, cols, ts = case[:3]
    stf, st = _stf(oracle)
    a = rc.mono_plane(rows, cols)
    got, gl, gb = oracle.generate_tile_pyramid(a, ts)
    want, wl, wb = R.generate_tile_pyramid(a, ts)
    assert gl == wl and gb == wb and np.array_equal(got, want)
    r, g, b = rc.rgb_planes(rows, cols)
    got, gl = oracle.generate_tile_pyramid_rgb(r, g, b, ts)
    want, wl = R.generate_tile_pyramid_rgb(r, g, b, ts)
    assert gl == wl and np.array_equal(got, want)
    got, _ = oracle.generate_tile_pyramid_rgb(r, g, b, ts, stf, st)
    want, _ = R.generate_tile_pyramid_rgb(r, g, b, ts, rc.STF, rc.STATS_NS)
    assert np.array_equal(got, want)


def test_oracle_level_arithmetic(oracle):
    for m, ts in rc.LEVEL_ARGS:
        want = R.compute_num_levels(m, 1, ts)
        assert oracle.tile_compute_num_levels(m, 1, ts) == oracle.tile_compute_num_levels(1, m, ts) == want, (m, ts)
    assert [R.compute_num_levels(n, n, 256) for n in (256, 257, 512, 513, 1024)] == [1, 2, 2, 3, 3]   # tiles.rs:487-494 and one over
    levels, total = R.pyramid_layout(1, 2 ** 31, 1, 1)
    assert len(levels) == 32 and total == sum(L["width"] for L in levels) and levels[0]["width"] == 1
    assert oracle.tile_pyramid_layout(1, 2 ** 31, 1, 1) == (levels, total)
    assert R.compute_num_levels(2 ** 32, 1, 1) == 33
