"""The host-only half of the open-file view (csrc/view.hip): ab_downsample_histogram and ab_histogram_bin_edges against
tests/view_restatement.py, which is itself pinned by hand-computed cases here, and the argument errors of the entry points that exist
without a context.  Every comparison is ==: integers, or the same f64 operations."""
import ctypes as C

import numpy as np
import pytest

import view_restatement as V
from astroburst_amd import _lib

U32 = np.uint32
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def bins65536():
    a = np.random.default_rng(512).integers(0, 5000, 65536, dtype=np.int64).astype(U32)
    a[65535] = 4321   # (never zero: the dropped top bin must show in the sums)
    a.setflags(write=False)
    return a


def _down(L, bins, target):
    bins = np.ascontiguousarray(bins, dtype=U32)
    out = np.full(max(1, min(target, bins.size)) + 1, 0xDEADBEEF, U32)   # one guard word
    n = C.c_size_t(0)
    rc = L.ab_downsample_histogram(bins.ctypes.data_as(U32P), bins.size, target, out.ctypes.data_as(U32P), C.byref(n))
    assert rc == _lib.AB_OK
    assert out[n.value] == 0xDEADBEEF
    return out[:n.value]


# ---- the restatement, by hand ---------------------------------------------------------------------------------------------------
def test_restatement_hand_cases():
    # 7 -> 3: ratio = 7 / 3 = 2.3333333333333335; starts 0, 2, 4 (int(2.33), int(4.67)); the last end is int(3 * ratio) = int(7.0) = 7
    assert V.ranges(7, 3) == [(0, 2), (2, 4), (4, 7)]
    assert V.downsample([1, 2, 3, 4, 5, 6, 7], 3).tolist() == [3, 7, 18]
    # 8 -> 2: an exact ratio, a clean partition
    assert V.downsample([1, 2, 3, 4, 5, 6, 7, 8], 2).tolist() == [10, 26]
    # target >= len: the copy
    assert V.downsample([4, 5], 2).tolist() == [4, 5] and V.downsample([4, 5], 9).tolist() == [4, 5]
    # saturation: 0xFFFFFFF0 + 0x20 saturates, the next bin does not
    assert V.downsample([0xFFFFFFF0, 0x20, 1, 2], 2).tolist() == [0xFFFFFFFF, 3]
    # 65536 -> 49: ratio = 1337.4693877551020 and 49 * ratio rounds to 65535.99999999999: the last source bin belongs to nobody
    assert V.ranges(65536, 49)[-1] == (64198, 65535) and V.dropped_tail(65536, 49) == 1
    assert V.dropped_tail(65536, 512) == 0 and V.dropped_tail(65536, 1000) == 0
    # edges: 4 bins over [1, 3] step 0.5; a range below 1e-10 repeats dmin
    assert V.bin_edges(1.0, 3.0, 4).tolist() == [1.0, 1.5, 2.0, 2.5, 3.0]
    assert V.bin_edges(2.0, 2.0 + 5e-11, 3).tolist() == [2.0] * 4
    assert V.bin_edges(5.0, 1.0, 2).tolist() == [5.0] * 3   # a negative range is below 1e-10 too


def test_restatement_dropped_targets():
    """the issue's count: 9841 targets below 65 536 lose the last source bin (never more than one), the smallest 49, 98, 103, 107, 161"""
    tails = np.array([V.dropped_tail(65536, t) for t in range(1, 65536)])
    assert set(np.unique(tails)) == {0, 1}
    lost = np.nonzero(tails)[0] + 1
    assert lost.size == 9841 and lost[:5].tolist() == [49, 98, 103, 107, 161]


# ---- ab_downsample_histogram ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [1, 2, 49, 98, 512, 1000, 16384, 65535, 65536, 100000])
def test_downsample_65536(L, bins65536, target):
    got = _down(L, bins65536, target)
    assert got.size == min(target, 65536)
    assert np.array_equal(got, V.downsample(bins65536, target))
    total = int(bins65536.astype(np.uint64).sum())
    if target == 49:
        assert int(got.astype(np.uint64).sum()) == total - int(bins65536[65535])
    if target == 512:
        assert int(got.astype(np.uint64).sum()) == total


@pytest.mark.parametrize("n_bins", [1, 7, 513])
def test_downsample_other_lengths(L, n_bins):
    bins = np.random.default_rng(n_bins).integers(0, 1 << 20, n_bins).astype(U32)
    for target in sorted({1, 2, 3, n_bins - 1, n_bins, n_bins + 1, 512} - {0}):
        assert np.array_equal(_down(L, bins, target), V.downsample(bins, target)), (n_bins, target)


def test_downsample_saturates(L):
    bins = np.full(64, 0xFFFFFF00, U32)
    bins[5] = 3
    bins[63] = 0xFFFFFFFF
    for target in (1, 7, 16, 63):
        got = _down(L, bins, target)
        assert np.array_equal(got, V.downsample(bins, target))
        assert got.max() == 0xFFFFFFFF
    assert _down(L, bins, 1)[0] == 0xFFFFFFFF                # 64 bins of ~2^32 in one: no wrap
    assert np.array_equal(_down(L, bins, 64), bins)          # the copy keeps every word


def test_downsample_dropped_tail_every_target(L, bins65536):
    """all 65 535 targets below 65 536: the output's sum is the input's minus the top bins the restatement says nobody covers"""
    wide = bins65536.astype(np.uint64)
    total = int(wide.sum())
    src = bins65536.ctypes.data_as(U32P)
    out = np.zeros(65536, U32)
    dst = out.ctypes.data_as(U32P)
    n = C.c_size_t(0)
    for target in range(1, 65536):
        assert L.ab_downsample_histogram(src, 65536, target, dst, C.byref(n)) == _lib.AB_OK and n.value == target
        tail = V.dropped_tail(65536, target)
        assert int(out[:target].sum(dtype=np.uint64)) == total - int(wide[65536 - tail:].sum()), target


# ---- ab_histogram_bin_edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dmin,dmax,bins", [(0.0, 1.0, 1), (1.0, 3.0, 4), (-5.25, 1e6 / 3.0, 512), (1000.123, 64000.7, 65536),
                                             (2.0, 2.0 + 5e-11, 7), (2.0, 2.0, 3), (5.0, 1.0, 2), (0.0, 1e-10, 4)])
def test_bin_edges(L, dmin, dmax, bins):
    out = np.full(bins + 2, -7.0)
    assert L.ab_histogram_bin_edges(dmin, dmax, bins, out.ctypes.data_as(C.POINTER(C.c_double))) == _lib.AB_OK
    assert out[bins + 1] == -7.0
    assert np.array_equal(out[:bins + 1], V.bin_edges(dmin, dmax, bins))


def test_python_wrappers(bins65536):
    import astroburst_amd as ab
    assert np.array_equal(ab.downsample_histogram(bins65536, 512), V.downsample(bins65536, 512))
    assert np.array_equal(ab.downsample_histogram(bins65536, 100000), bins65536)
    assert np.array_equal(ab.histogram_bin_edges(1.0, 3.0, 4), V.bin_edges(1.0, 3.0, 4))
    with pytest.raises(ab.AstroBurstError):
        ab.downsample_histogram(bins65536, 0)
    with pytest.raises(ab.AstroBurstError):
        ab.histogram_bin_edges(0.0, 1.0, 0)


# ---- argument errors without a context -------------------------------------------------------------------------------------------
def test_argument_errors(L):
    bins = np.ones(8, U32)
    out = np.zeros(8, U32)
    n = C.c_size_t(99)
    p, o = bins.ctypes.data_as(U32P), out.ctypes.data_as(U32P)
    INV = _lib.AB_ERR_INVALID
    assert L.ab_downsample_histogram(None, 8, 4, o, C.byref(n)) == INV
    assert L.ab_downsample_histogram(p, 8, 4, None, C.byref(n)) == INV
    assert L.ab_downsample_histogram(p, 8, 4, o, None) == INV
    assert L.ab_downsample_histogram(p, 0, 4, o, C.byref(n)) == INV
    assert L.ab_downsample_histogram(p, 8, 0, o, C.byref(n)) == INV
    assert n.value == 99 and not out.any()
    edges = np.zeros(4)
    assert L.ab_histogram_bin_edges(0.0, 1.0, 3, None) == INV
    assert L.ab_histogram_bin_edges(0.0, 1.0, 0, edges.ctypes.data_as(C.POINTER(C.c_double))) == INV
    # the device entry points refuse a NULL context before they look at anything else
    img = np.ones((2, 2), np.float32)
    pl = _lib.Plane(C.c_void_p(img.ctypes.data), 2, 2, 0)
    cfg = _lib.FitsViewConfigC()
    L.ab_fits_view_config_default(None)            # a no-op
    L.ab_fits_view_config_default(C.byref(cfg))
    assert (cfg.stf.target_bg, cfg.stf.shadow_k, cfg.hist_bins) == (0.25, -2.8, 512)
    u8 = np.zeros(12, np.uint8)
    assert L.ab_display_histogram(None, C.byref(pl), 0.0, 1.0, 512, C.c_void_p(out.ctypes.data), 0, C.byref(n)) == INV
    assert L.ab_process_fits_view(None, C.byref(pl), C.byref(cfg), C.c_void_p(u8.ctypes.data), 0, C.c_void_p(out.ctypes.data), 0, None) == INV
    assert L.ab_process_rgb_fits_view(None, C.byref(pl), C.byref(pl), C.byref(pl), C.byref(cfg), 4096, C.c_void_p(u8.ctypes.data), 0,
                                      C.c_void_p(out.ctypes.data), 0, None) == INV
    assert n.value == 99 and not u8.any()
