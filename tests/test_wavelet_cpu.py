"""A trous wavelet denoising without a GPU: the reference's own #[test]s (wavelet.rs:246-362; its test_block_transpose is covered by the two-routes test below) against the restatement
(tests/wavelet_restatement.py) and, where they concern the threshold arithmetic, against the library; the two routes of the vertical
pass bit for bit; the library's host-only threshold function bit for bit against the restatement; the exported symbols; and the
kernels' code for gfx950, which must hold no f32 fused multiply-add (the bit-exact contract rests on it)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import wavelet_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astroburst_amd", "csrc")
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pseudo_noise(seed):
    """tests::pseudo_noise (:250-253): a u64 LCG step, its top 31 bits as f32 over u32::MAX as f32, centred, doubled"""
    x = (int(seed) * 6364136223846793005 + 1442695040888963407) % (1 << 64)
    return F32(F32(F32(F32(x >> 33) / F32(4294967295)) - F32(0.5)) * F32(2.0))


def _lib_thresholds(noise_sigma, thresholds):
    from astroburst_amd.core import wavelet_scale_thresholds
    return wavelet_scale_thresholds(noise_sigma, thresholds)


# ---- the reference's tests, transcribed ------------------------------------------------------------------------------------------
def test_b3_kernel_sums_to_one():
    total = F32(0.0)
    for v in R.B3:
        total = F32(total + v)
    assert abs(float(total) - 1.0) < 1e-6
    assert [float(v) for v in R.B3] == [0.0625, 0.25, 0.375, 0.25, 0.0625]


def test_atrous_smooth_preserves_flat():
    smoothed = R.atrous_smooth(np.full((32, 32), 100.0, F32), 1)
    assert (np.abs(smoothed[2:30, 2:30] - 100.0) < 0.01).all()


def test_wavelet_roundtrip_flat():
    out, scales, _ = R.wavelet_denoise(np.full((64, 64), 50.0, F32), 3, [0.0, 0.0, 0.0], True)
    assert scales == 3 and (np.abs(out[4:60, 4:60] - 50.0) < 0.1).all()


def test_soft_threshold():
    got = R.soft_threshold(np.array([-5.0, -1.0, 0.5, 1.0, 3.0, 10.0], F32), 2.0)
    assert (np.abs(got - np.array([-3.0, 0.0, 0.0, 0.0, 1.0, 8.0], F32)) < 1e-6).all()


def test_noise_reduction():
    image = np.full((64, 64), 100.0, F32)
    for y in range(64):
        for x in range(64):
            image[y, x] = F32(image[y, x] + F32(pseudo_noise(y * 64 + x) * F32(5.0)))
    out, _, sigma = R.wavelet_denoise(image, 4, [3.0, 2.0, 1.5, 1.0], True)
    orig_var = ((image[4:60, 4:60].astype(np.float64) - 100.0) ** 2).mean()
    den_var = ((out[4:60, 4:60].astype(np.float64) - 100.0) ** 2).mean()
    assert den_var < orig_var, (den_var, orig_var)
    # the thresholds that run consumed, as the library derives them from the same sigma
    assert np.array_equal(bits(_lib_thresholds(sigma, [3.0, 2.0, 1.5, 1.0])[:4]), bits(R.scale_thresholds(sigma, [3.0, 2.0, 1.5, 1.0], 4)))


def test_estimate_noise_sigma():
    noise = np.array([pseudo_noise(i) for i in range(10000)], F32)
    sigma = R.estimate_noise_sigma(noise)
    assert 0.0 < sigma < 2.0, sigma


# ---- the restatement's own fine print --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(300, 517), (257, 63), (33, 65), (1, 77), (65, 1)])
@pytest.mark.parametrize("step", [1, 4, 16, 32, 128])
def test_both_routes_of_the_vertical_pass_agree_bit_for_bit(rows, cols, step):
    rng = np.random.default_rng(rows + step)
    img = rng.normal(300.0, 20.0, (rows, cols)).astype(F32)
    img[rows // 3, cols // 2] = np.inf
    h = R.smooth_rows(img, step)
    assert np.array_equal(bits(R.smooth_cols(h, step)), bits(R.smooth_cols_transposed(h, step)))
    assert R.takes_transposed_route(rows, step) == (step >= 32 and rows >= 257)


def test_the_two_routes_give_the_same_denoised_plane():
    img = np.random.default_rng(5).normal(300.0, 20.0, (300, 517)).astype(F32)
    a = R.wavelet_denoise(img, 8, route="plain")
    b = R.wavelet_denoise(img, 8, route="transposed")
    c = R.wavelet_denoise(img, 8)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[0]), bits(c[0])) and a[1:] == b[1:] == c[1:]


def test_signum_is_not_numpy_sign_and_nan_stays_nan():
    d = np.array([0.0, -0.0, np.nan, 3.0, -3.0, np.inf, -np.inf], F32)
    soft = R.soft_threshold(d, -1.0)  # a negative threshold: nothing is zeroed, +-0 move by signum(+-0) * 1 = +-1
    assert soft[0] == 1.0 and soft[1] == -1.0 and np.isnan(soft[2]) and soft[3] == 4.0 and soft[4] == -4.0
    assert soft[5] == np.inf and soft[6] == -np.inf
    hard = R.hard_threshold(d, 3.0)
    assert np.array_equal(bits(hard[[0, 1, 3, 4]]), bits(np.zeros(4, F32))) and np.isnan(hard[2]) and hard[5] == np.inf
    # a NaN threshold fails every `<=`: soft -> NaN, hard -> the value
    assert np.isnan(R.soft_threshold(np.array([1.0], F32), np.nan)[0]) and R.hard_threshold(np.array([1.0], F32), np.nan)[0] == 1.0


def test_median_even_and_odd_and_empty():
    assert R.median_f32(np.array([], F32)) == 0.0
    assert R.median_f32(np.array([3.0, 1.0, 2.0], F32)) == 2.0
    a, b = F32(1.0000001), F32(1.0000004)
    assert R.median_f32(np.array([5.0, a, b, 0.5], F32)) == F32(F32(a + b) / F32(2.0))
    assert R.estimate_noise_sigma(np.array([np.nan, np.inf, -np.inf], F32)) == 0.0
    assert R.estimate_noise_sigma(np.array([np.nan, -2.0, np.inf], F32)) == 2.0 * 1.4826


def test_progress_stages():
    assert R.progress_stages(2) == ["decomposing scale 1/2", "decomposing scale 2/2", "thresholding scale 1/2", "thresholding scale 2/2",
                                    "reconstructing"]
    assert len(R.progress_stages(0)) == 3 and len(R.progress_stages(12)) == 17


# ---- the library's host-only threshold function ---------------------------------------------------------------------------------
SIGMAS = [0.0, 1e-30, 1e-12, 3.7e-5, 0.013, 1.0, 1.4826, 7.25, 1234.5678, 6.5e4, 3.3e37, 1e39, 1e300, float("inf"), float("nan"), -2.5]
LISTS = [
    [],                                                  # empty: 1.0 at every scale
    [2.5],                                               # shorter than S: the last entry carries on
    [3.0, 2.5, 2.0],
    [3.0, 2.5, 2.0, 1.5, 1.0],                           # the default
    [3.0, 2.5, 2.0, 1.5, 1.0, 0.75, 0.5, 0.25],          # exactly eight
    [3.0, 2.5, 2.0, 1.5, 1.0, 0.75, 0.5, 0.25, 9.0, 8.0, 7.0, 6.0],  # longer than S: as its first eight
    [0.0, -1.5, float("nan"), 1e-3, float("inf")],       # zero, negative, NaN, inf entries
    [0.1, 0.7, 1.3, 0.3333333, 2.718281828, 1e-7, 1e7, 0.9999999],
]


@pytest.mark.parametrize("thresholds", LISTS, ids=[str(i) for i in range(len(LISTS))])
def test_scale_thresholds_are_bit_identical_to_the_restatement(thresholds):
    for sigma in SIGMAS:
        got = _lib_thresholds(sigma, thresholds)
        want = R.scale_thresholds(sigma, thresholds, 8)
        assert got.dtype == np.float32 and got.shape == (8,)
        same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (sigma, thresholds, got, want)


def test_scale_thresholds_sweep_of_sigmas():
    rng = np.random.default_rng(11)
    for sigma in np.concatenate([10.0 ** rng.uniform(-8, 6, 400), rng.uniform(0, 100, 400)]):
        got = _lib_thresholds(float(sigma), R.DEFAULT_THRESHOLDS)
        assert np.array_equal(bits(got), bits(R.scale_thresholds(float(sigma), R.DEFAULT_THRESHOLDS, 8))), sigma


def test_scale_thresholds_follow_the_table_and_halve_beyond_it():
    got = _lib_thresholds(1.0, [1.0])
    assert [float(v) for v in got[:7]] == [float(F32(v)) for v in R.NOISE_TABLE]
    assert got[7] == F32(0.0051 / 2.0)
    assert np.array_equal(bits(_lib_thresholds(2.0, LISTS[5])), bits(_lib_thresholds(2.0, LISTS[4])))


def test_scale_thresholds_reject_null_arguments():
    from astroburst_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_float * 8)()
    cfg = _lib.WaveletConfigC(5, None, 0, 1)
    assert L.ab_wavelet_scale_thresholds(1.0, ctypes.byref(cfg), out) == _lib.AB_OK and out[0] == F32(0.8908)
    assert L.ab_wavelet_scale_thresholds(1.0, None, out) == _lib.AB_ERR_INVALID
    assert L.ab_wavelet_scale_thresholds(1.0, ctypes.byref(cfg), None) == _lib.AB_ERR_INVALID
    cfg = _lib.WaveletConfigC(5, None, 3, 1)  # a count without a list
    assert L.ab_wavelet_scale_thresholds(1.0, ctypes.byref(cfg), out) == _lib.AB_ERR_INVALID


def test_new_symbols_are_exported_and_declared():
    from astroburst_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ab_wavelet_denoise", "ab_wavelet_scale_thresholds"):
        assert hasattr(L, name), name
        assert name in _lib.declared_symbols(), name
    import astroburst_amd as ab
    assert callable(ab.Context.wavelet_denoise) and callable(ab.core.wavelet_scale_thresholds)


# ---- the kernels, compiled for gfx950 with the Makefile's flags ---------------------------------------------------------------
def test_kernels_hold_no_f32_fused_multiply_add(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in base
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *base, "-w", "--save-temps", "-c", os.path.join(CSRC, "wavelet.hip"), "-o",
                    os.path.join(tmp_path, "wavelet.o")], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lst = open(os.path.join(tmp_path, "wavelet-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_spill_count:\s+\d+", lst, re.S)}
    for family, count in (("wt_row_kernel", 1), ("wt_col_kernel", 2), ("wt_fused_kernel", 2), ("wt_reconstruct_kernel", 2)):
        names = [n for n in meta if family in n]
        assert len(names) == count, (family, sorted(meta))
        for name in names:
            body = re.split(r"^%s:" % re.escape(name), lst, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
            for fused in ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32", "v_mad_f32", "v_mac_f32", "v_fma_mix", "v_dot2c_f32"):
                assert fused not in body, (name, fused)
            assert "v_mul_f32" in body or "v_pk_mul_f32" in body or family == "wt_reconstruct_kernel", name  # the taps are really multiplied
            assert "v_add_f32" in body or "v_pk_add_f32" in body, name
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[name]).group(1)) == 0, name
            assert "scratch_" not in body, name
    spills = re.findall(r"\.name:\s+(\S+)\n.*?\.vgpr_spill_count:\s+(\d+)", lst, re.S)
    assert all(int(n) == 0 for _, n in spills), spills
