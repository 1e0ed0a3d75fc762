"""CPU pins of tests/rgb_export_restatement.py (the checker of tests/test_gpu_rgb_export.py) on hand-written vectors, and the one
host-only entry point of csrc/rgb_export.hip, ab_rgb_packed_bytes, through the library."""
import ctypes as C

import numpy as np
import pytest

import rgb_export_restatement as R

F32 = np.float32


def _row(vals):
    return np.array([vals], F32)


# ---- the packers -----------------------------------------------------------------------------------------------------------------
def test_packers_on_hand_written_values():
    v = _row([np.nan, -1.0, 2.0, np.inf, 1.0, 0.5, -np.inf, 0.0, -0.0])
    z = np.zeros_like(v)
    assert R.pack_rgb(v, z, z, R.PACK_8)[0, :, 0].tolist() == [0, 0, 255, 255, 255, 127, 0, 0, 0]        # 0.5 * 255 = 127.5 truncates
    assert R.pack_rgb(v, z, z, R.PACK_8_ROUND)[0, :, 0].tolist() == [0, 0, 255, 255, 255, 128, 0, 0, 0]  # and rounds away from zero
    be = R.pack_rgb(v, z, z, R.PACK_16BE)
    assert be.shape == (1, 9, 6)
    assert (be[0, :, 0].astype(int) * 256 + be[0, :, 1]).tolist() == [0, 0, 65535, 65535, 65535, 32767, 0, 0, 0]
    assert be[0, 4, :2].tolist() == [0xFF, 0xFF]
    assert not be[..., 2:].any()


def test_rounding_is_half_away_from_zero_not_half_even():
    x = np.array([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 0.49999997, 254.5, 2.4999998], F32)
    assert R.round_half_away(x).tolist() == [1.0, 2.0, 3.0, 4.0, 127.0, 128.0, 0.0, 255.0, 2.0]
    assert R.round_half_away(np.array([-0.5, -2.5], F32)).tolist() == [-1.0, -3.0]
    # through the packer: 0.5f * 255f is exactly 127.5 and 0.1f * 255f = 25.5 exactly (0.1f is just above 0.1, the product rounds down to it)
    v = np.array([[0.5, 0.1]], F32)
    assert (v * F32(255.0)).tolist() == [[127.5, 25.5]]
    assert R.pack_rgb(v, v, v, R.PACK_8_ROUND)[0, :, 1].tolist() == [128, 26] and R.pack_rgb(v, v, v, R.PACK_8)[0, :, 1].tolist() == [127, 25]


def test_sixteen_bit_byte_order_and_interleave():
    s = F32(0x1234 + 0.25) / F32(65535.0)
    assert int(F32(s) * F32(65535.0)) == 0x1234
    r, g, b = _row([s, 0.0]), _row([0.0, 1.0]), _row([1.0, s])
    be = R.pack_rgb(r, g, b, R.PACK_16BE)
    assert be[0, 0].tolist() == [0x12, 0x34, 0x00, 0x00, 0xFF, 0xFF]
    assert be[0, 1].tolist() == [0x00, 0x00, 0xFF, 0xFF, 0x12, 0x34]
    assert np.array_equal(be.reshape(1, 2, 3, 2).view(">u2")[..., 0], [[[0x1234, 0, 65535], [0, 65535, 0x1234]]])
    u8 = R.pack_rgb(_row([0.1, 0.2]), _row([0.3, 0.4]), _row([0.5, 0.6]), R.PACK_8)
    assert u8.reshape(-1).tolist() == [25, 76, 127, 51, 102, 153]    # R, G, B of pixel 0, then of pixel 1


def test_ramp_case_separates_round_from_truncate():
    ramp = R.cases((2, 7))["ramp"]
    a, b = R.pack_rgb(ramp, ramp, ramp, R.PACK_8), R.pack_rgb(ramp, ramp, ramp, R.PACK_8_ROUND)
    assert (a != b).mean() > 0.4 and (np.abs(a.astype(int) - b.astype(int)) <= 1).all()


# ---- process_drizzle_rgb ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(7)
    return [(rng.random((5, 7), dtype=F32) * F32(0.8) + F32(0.05 * (c + 1))).astype(F32) for c in range(3)]


def test_no_balance_no_stretch_is_the_identity_stf_per_channel(oracle, planes):
    got = R.process_drizzle_rgb(oracle, *planes, white_balance="none", auto_stretch=False)
    assert got["wb_factors"] == (1.0, 1.0, 1.0) and (got["rows"], got["cols"]) == (5, 7) and not got["scnr_applied"]
    for c in range(3):
        st = oracle.compute_image_stats(planes[c])
        want = oracle.apply_stf_f32(planes[c], oracle.StfParams(0.0, 0.5, 1.0), st)
        assert np.array_equal(R.bits(got["stretched"][c]), R.bits(want))
        assert np.array_equal(R.bits(got["wb"][c]), R.bits(planes[c]))
        assert got["stf"][c] == (0.0, 0.5, 1.0) and got["stats_wb"][c] == R.stats_tuple(st)
        assert got["chan_stats"][c] == (st.min, st.max, st.median, st.mean)
    assert np.array_equal(got["rgb8"], R.pack_rgb(*got["stretched"], R.PACK_8_ROUND))


def test_an_absent_channel_is_a_zero_plane_with_finite_multipliers(oracle, planes):
    got = R.process_drizzle_rgb(oracle, planes[0], None, planes[2], white_balance="auto", auto_stretch=True, linked_stf=True)
    assert np.isfinite(got["wb_factors"]).all()
    assert not got["wb"][1].any() and not got["stretched"][1].any()
    assert got["chan_stats"][1] == (0.0, 0.0, 0.0, 0.0) and got["stats_wb"][1][6] == 0
    assert got["stf"][0] == got["stf"][1] == got["stf"][2]


def test_differing_dims_are_cropped_top_left(oracle, planes):
    rng = np.random.default_rng(8)
    big = rng.random((6, 9), dtype=F32)
    tall = rng.random((8, 7), dtype=F32)
    got = R.process_drizzle_rgb(oracle, big, planes[1], tall, white_balance="none", auto_stretch=False)
    assert (got["rows"], got["cols"]) == (5, 7)
    assert np.array_equal(got["wb"][0], big[:5, :7]) and np.array_equal(got["wb"][2], tall[:5, :7])
    same = R.process_drizzle_rgb(oracle, big[:5, :7], planes[1], tall[:5, :7], white_balance="none", auto_stretch=False)
    assert np.array_equal(got["rgb8"], same["rgb8"])


def test_linked_merge_divides_by_three(oracle, planes):
    """the drizzle path's merge is a true f32 division; the multiplication by 1 / 3 that process_rgb uses differs in the last bit"""
    a, b, c = planes
    div = ((a + b) + c) / F32(3.0)
    mul = ((a + b) + c) * (F32(1.0) / F32(3.0))
    assert (R.bits(div) != R.bits(mul)).any()
    got = R.process_drizzle_rgb(oracle, a, b, c, white_balance="none", auto_stretch=True, linked_stf=True)
    p = oracle.auto_stf(oracle.compute_image_stats(div.astype(F32)))
    assert got["stf"][0] == (p.shadow, p.midtone, p.highlight)


# ---- ab_rgb_packed_bytes: host-only --------------------------------------------------------------------------------------------------
def test_rgb_packed_bytes_through_the_library():
    import astroburst_amd as ab
    from astroburst_amd import _lib
    assert ab.rgb_packed_bytes(5, 7, ab.RGB_PACK_8) == 105
    assert ab.rgb_packed_bytes(5, 7, ab.RGB_PACK_8_ROUND) == 105
    assert ab.rgb_packed_bytes(5, 7, ab.RGB_PACK_16BE) == 210
    assert ab.rgb_packed_bytes(13759, 12451, ab.RGB_PACK_16BE) == 13759 * 12451 * 6
    assert ab.rgb_packed_bytes(1, (1 << 31) - 1, ab.RGB_PACK_8) == 3 * ((1 << 31) - 1)
    L = _lib.lib()
    n = C.c_size_t(0)
    for rows, cols, pack in ((0, 7, 0), (5, 0, 0), (-1, 7, 0), (5, 7, 3), (5, 7, -1), (1 << 16, 1 << 15, 0), (1, 1 << 31, 2)):
        assert L.ab_rgb_packed_bytes(rows, cols, pack, C.byref(n)) == _lib.AB_ERR_INVALID, (rows, cols, pack)
        with pytest.raises(ab.AstroBurstError):
            ab.rgb_packed_bytes(rows, cols, pack)
    assert L.ab_rgb_packed_bytes(5, 7, 0, None) == _lib.AB_ERR_INVALID
