"""Richardson-Lucy deconvolution without a GPU: the reference's own #[test]s (deconvolution.rs:252-343) against the restatement
(tests/deconv_restatement.py), the library's host-only Gaussian PSF bit for bit against glibc's expf, the claim the GPU kernels rest
on (the reference's padded FFT product == the direct convolution with a zero boundary), and the kernels' code for gfx950."""
import os
import re
import subprocess

import numpy as np
import pytest

import deconv_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astroburst_amd", "csrc")


def _lib_psf(size, sigma):
    from astroburst_amd.core import generate_gaussian_psf
    return generate_gaussian_psf(size, sigma)


# ---- the reference's tests, transcribed ------------------------------------------------------------------------------------------
def test_gaussian_psf_normalized():
    psf = _lib_psf(15, 2.0)
    total = np.float32(0.0)
    for v in psf.ravel():
        total = np.float32(total + v)
    assert abs(float(total) - 1.0) < 1e-5


def test_gaussian_psf_center_peak():
    psf = _lib_psf(15, 2.0)
    assert (psf <= psf[7, 7] + np.float32(1e-7)).all()


def test_fft_convolver_identity():
    rows = cols = 64
    psf = np.zeros((3, 3), np.float32)
    psf[1, 1] = 1.0
    image = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
    res = R.Convolver(rows, cols, psf, np.float32).forward(image)
    assert (np.abs(res[1:-1, 1:-1] - image[1:-1, 1:-1]) < 0.5).all()


def test_rl_returns_result():
    size = 32
    psf = _lib_psf(5, 1.0)
    y, x = np.mgrid[0:size, 0:size]
    image = ((y * size + x).astype(np.float32) / np.float32(size * size) + np.float32(0.01)).astype(np.float32)
    est, run, conv, _ = R.richardson_lucy(image, psf, 5, 0.001, False, 0.1, np.float32)
    assert 0 < run <= 5 and np.isfinite(conv) and est.shape == (size, size)


def test_deringing_bidirectional():
    original = np.full((16, 16), 100.0, np.float32)
    est = original.copy()
    est[5, 5] = 200.0
    est[8, 8] = 10.0
    out = R.deringing(est, original, 0.1, np.float32)
    assert abs(out[5, 5] - 110.0) < 1e-4 and abs(out[8, 8] - 90.0) < 1e-4 and abs(out[0, 0] - 100.0) < 1e-4


def _l2_delta(prev, curr):  # compute_l2_delta (:126-139)
    d = (curr - prev).astype(np.float64)
    return float(np.sqrt(np.sum(d * d) / prev.size))


def test_l2_delta():
    a = np.ones((10, 10), np.float32)
    assert _l2_delta(a, a) < 1e-10
    assert abs(_l2_delta(a, np.full((10, 10), 2.0, np.float32)) - 1.0) < 1e-10


# ---- the library's Gaussian PSF -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 2, 3, 5, 15, 16, 31, 63])
@pytest.mark.parametrize("sigma", [0.3, 1.0, 2.0, 10.0])
def test_gaussian_psf_is_bit_identical_to_the_expf_restatement(size, sigma):
    got = _lib_psf(size, sigma)
    want = R.gaussian_psf(size, sigma)
    assert got.dtype == np.float32 and got.shape == (size, size)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_gaussian_psf_rejects_size_zero():
    import astroburst_amd as ab
    with pytest.raises(ab.AstroBurstError):
        _lib_psf(0, 2.0)


# ---- what the GPU kernels compute instead of the FFT --------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,pr,pc", [(40, 52, 15, 15), (23, 17, 4, 6), (16, 20, 31, 31), (1, 9, 5, 3), (9, 1, 2, 7), (12, 12, 1, 1)])
def test_padded_fft_product_is_the_direct_convolution(rows, cols, pr, pc):
    rng = np.random.default_rng(rows * 1000 + pc)
    img = rng.uniform(0.5, 2.0, (rows, cols))
    psf = rng.uniform(0.0, 1.0, (pr, pc)).astype(np.float32)
    cv = R.Convolver(rows, cols, psf, np.float64)
    for transpose in (False, True):
        fft = cv.transpose(img) if transpose else cv.forward(img)
        np.testing.assert_allclose(fft, R.direct_conv(img, psf, transpose), rtol=1e-12, atol=1e-12)


def test_the_restatement_f32_stays_close_to_f64():
    """the reference's precision (complex64 FFTs) against the truth: the scale of the GPU tolerance"""
    rng = np.random.default_rng(3)
    img = (300.0 + rng.normal(0, 5, (60, 72))).astype(np.float32)
    img[20:23, 30:33] += 5000.0
    psf = R.gaussian_psf(15, 2.0)
    a, ra, ca, _ = R.richardson_lucy(img, psf, 20, 0.001, True, 0.1, np.float32)
    b, rb, cb, _ = R.richardson_lucy(img, psf, 20, 0.001, True, 0.1, np.float64)
    assert ra == rb == 20
    assert (np.abs(a - b) / np.maximum(np.abs(b), 1.0)).max() < 1e-4
    assert abs(ca - cb) <= 1e-4 * cb


# ---- the kernels, compiled for gfx950 with the Makefile's flags ---------------------------------------------------------------
def test_tiled_kernels_use_packed_fma_and_no_scratch(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-ffp-contract=off" in base
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *base, "-w", "--save-temps", "-c", os.path.join(CSRC, "deconv.hip"), "-o",
                    os.path.join(tmp_path, "deconv.o")], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lst = open(os.path.join(tmp_path, "deconv-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = {m.group(1): m.group(2) for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.vgpr_spill_count:\s+\d+", lst, re.S)}
    tiled = [n for n in meta if "rl_tiled_kernel" in n]
    assert len(tiled) == 2, sorted(meta)
    for name in tiled:
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta[name]).group(1))
        assert scratch == 0, (name, scratch)
        body = re.split(r"^%s:" % re.escape(name), lst, maxsplit=1, flags=re.M)[1].split(".Lfunc_end", 1)[0]
        assert body.count("v_pk_fma_f32") >= 64, (name, body.count("v_pk_fma_f32"))
        assert "scratch_" not in body, name
    spills = re.findall(r"\.name:\s+(\S+)\n.*?\.vgpr_spill_count:\s+(\d+)", lst, re.S)
    assert all(int(n) == 0 for _, n in spills), spills
