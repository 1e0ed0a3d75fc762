"""The whole-plane radix selects (csrc/plane_select.hip, and the device-resident copy in csrc/masked_stretch.hip) on the adversarial
planes of tests/select_adversarial.py: ranks on the first / last element of a bin, middle ranks split between two bins at every
level, long ties, values that must not be counted, several rank groups through the reused histograms.

Bar: BIT FOR BIT, everywhere (rms_residual alone keeps test_gpu_background's rel = 1e-12).  Through the select go
ab_tile_percentile_bounds, the bounds (and so every byte) of ab_generate_tile_pyramid, the global median / MAD / model median of
ab_extract_background, ab_wavelet_denoise's noise estimate, and every iteration of ab_masked_stretch_with_mask -- the last in both
forms of its level 1 (the blend pass's predicted histogram, and, under the developer switch AB_MS_NO_PREDICT, a pass of its own).
tests/test_select_adversarial_cpu.py holds the fixtures to what they claim."""
import numpy as np
import pytest

import select_adversarial as SA
import wavelet_restatement as WR
from astroburst_amd import AstroBurstError
from test_gpu_background import assert_parity
from test_gpu_masked import result_equal
from test_gpu_wavelet import _under, check as wavelet_check

pytestmark = pytest.mark.gpu

F32 = np.float32
POPULATIONS = SA.populations()
FAMILIES = ["L0", "BINADE", "L1", "L2", "TOP", "FLOOR", "four", "tie", "q16"]
_oracle_bounds = {}


def pair_bits(pair):
    return tuple(int(b) for b in SA.bits_of(np.array(pair, F32)))


def family(name):
    return [p for p in POPULATIONS if p.name.startswith(name + "-")]


def wanted_bounds(oracle, pop, lo_pct, hi_pct):
    """the numpy statement, and the oracle's answer (computed once per population and percentile pair) equal to it"""
    k = (pop.name, lo_pct, hi_pct)
    if k not in _oracle_bounds:
        want = pair_bits(SA.percentile_statement(pop.values, lo_pct, hi_pct))
        assert pair_bits(oracle.tile_percentile_bounds(pop.values.reshape(1, -1), lo_pct, hi_pct)) == want, k
        _oracle_bounds[k] = want
    return _oracle_bounds[k]


# ---- percentile bounds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_percentile_bounds_bit_for_bit(ctx, oracle, name):
    import torch
    pops = family(name)
    assert pops
    for pop in pops:
        for plane in pop.planes():
            dev = torch.from_numpy(plane).cuda()
            for lo_pct, hi_pct in SA.PCT_PAIRS:
                want = wanted_bounds(oracle, pop, lo_pct, hi_pct)
                for src, what in ((plane, "host"), (dev, "device")):
                    got = pair_bits(ctx.tile_percentile_bounds(src, lo_pct, hi_pct))
                    assert got == want, (pop.name, plane.shape, what, lo_pct, hi_pct, [hex(b) for b in got], [hex(b) for b in want])


def test_percentile_bounds_without_a_candidate_take_the_min_max_branch(ctx, oracle):
    import torch
    for name, plane in SA.no_candidate_planes().items():
        for lo_pct, hi_pct in SA.PCT_PAIRS:
            want = pair_bits(SA.percentile_statement(plane, lo_pct, hi_pct))
            assert pair_bits(oracle.tile_percentile_bounds(plane, lo_pct, hi_pct)) == want
            assert pair_bits(ctx.tile_percentile_bounds(plane, lo_pct, hi_pct)) == want, (name, lo_pct, hi_pct)
            assert pair_bits(ctx.tile_percentile_bounds(torch.from_numpy(plane).cuda(), lo_pct, hi_pct)) == want, (name, lo_pct, hi_pct)


def test_percentile_bounds_repeat_and_survive_a_trim(ctx, oracle):
    """the same population twice in a row (the same call back to back), between two others, and again after ctx.trim(): the three
    pinned histograms and the device histogram are reused from call to call and from rank group to rank group"""
    import torch
    big = next(p for p in POPULATIONS if p.name == "L0-big")
    four = next(p for p in POPULATIONS if p.name == "four-1000")
    q16 = next(p for p in POPULATIONS if p.name.startswith("q16-"))
    dev = {p.name: torch.from_numpy(p.values.reshape(1, -1)).cuda() for p in (big, four, q16)}

    def run():
        return [pair_bits(ctx.tile_percentile_bounds(dev[p.name], lo, hi)) for lo, hi in SA.PCT_PAIRS for p in order]

    order = (big, big, four, four, big, q16, q16, four)
    want = [wanted_bounds(oracle, p, lo, hi) for lo, hi in SA.PCT_PAIRS for p in order]
    first, second = run(), run()
    ctx.trim()
    third = run()
    assert first == want and second == want and third == want


def test_big_population_as_a_plane_and_from_the_host(ctx, oracle):
    """600 001 candidates: more than one grid stride, no multiple of the block, the deciding copies at the first and the last pixel"""
    big = next(p for p in POPULATIONS if p.name == "L0-big")
    lower, upper, _ = SA.PAIRS["L0"]
    for plane in big.planes():
        for lo_pct, hi_pct in SA.PCT_PAIRS:
            assert pair_bits(ctx.tile_percentile_bounds(plane, lo_pct, hi_pct)) == wanted_bounds(oracle, big, lo_pct, hi_pct)
    assert pair_bits(ctx.tile_percentile_bounds(big.values.reshape(1, -1), 0.5, 0.5)) == pair_bits((lower, lower))
    assert pair_bits(ctx.tile_percentile_bounds(big.values[1:].reshape(1, -1), 0.5, 0.5)) == pair_bits((upper, upper))
    assert pair_bits(ctx.tile_percentile_bounds(big.values[:-1].reshape(1, -1), 0.5, 0.5)) == pair_bits((upper, upper))


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------
def test_pyramid_on_tied_bounds(ctx, oracle):
    import torch
    plane = SA.pyramid_plane()
    want, wl, wb = oracle.generate_tile_pyramid(plane, 256)
    assert pair_bits(wb) == pair_bits(SA.percentile_statement(plane, 0.001, 0.999))
    got, gl, gb = ctx.generate_tile_pyramid(plane, 256)
    assert gl == wl and pair_bits(gb) == pair_bits(wb)
    assert np.array_equal(got, want)
    dev, _, db = ctx.generate_tile_pyramid(torch.from_numpy(plane).cuda(), 256)
    assert pair_bits(db) == pair_bits(wb) and np.array_equal(dev.cpu().numpy(), want)


# ---- background ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("mode", ["subtract", "divide"])
@pytest.mark.parametrize("case", SA.background_cases(), ids=lambda c: c.name)
def test_background_parity(ctx, oracle, case, mode, iterations):
    kw = dict(grid_size=case.grid, poly_degree=case.degree, sigma_clip=case.sigma_clip, iterations=iterations)
    try:
        want = oracle.extract_background(case.image, mode={"subtract": 0, "divide": 1}[mode], **kw)
    except ValueError as e:
        assert case.name == "B6-scattered" and "(0)" in str(e)
        with pytest.raises(AstroBurstError) as got:
            ctx.extract_background(case.image, mode=mode, **kw)
        assert got.value.message == str(e), (str(e), got.value.message)   # the same message with the same count
        return
    assert case.name != "B6-scattered"
    got = ctx.extract_background(case.image, mode=mode, **kw)
    assert_parity(got, want)
    assert np.array_equal(SA.bits_of(got.model), SA.bits_of(want.model)) and np.array_equal(SA.bits_of(got.corrected), SA.bits_of(want.corrected))
    if case.name == "B1" and iterations == 1:
        assert got.sample_count == case.grid ** 2 - 2
    if case.name == "B3":
        assert np.unique(got.model).size == 1


# ---- wavelet ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,plane,parity", SA.wavelet_planes(), ids=lambda v: v if isinstance(v, str) else "")
def test_wavelet_noise_estimate_on_tied_details(ctx, name, plane, parity):
    _, _, sigma = wavelet_check(ctx, plane, 3)
    assert sigma > 0 and sigma == WR.wavelet_denoise(plane, 3)[2]
    wavelet_check(ctx, plane, 5, WR.DEFAULT_THRESHOLDS, False)


# ---- masked stretch --------------------------------------------------------------------------------------------------------------
MASKED = SA.masked_planes()
_oracle_stretch = {}


def stretch_both(ctx, oracle, name, img, mask, target, protection):
    from astroburst_amd.core import StarMaskResult
    coverage = float((mask > F32(0.01)).mean())
    k = (name, target, protection)
    if k not in _oracle_stretch:      # (shared between the default form and the switch: computed once, never modified)
        _oracle_stretch[k] = oracle.masked_stretch(img, mask=oracle.StarMaskResult(mask, 7, coverage), target_background=target,
                                                   protection_amount=protection)
    got = ctx.masked_stretch(img, mask=StarMaskResult(mask, 7, coverage), target_background=target, protection_amount=protection)
    result_equal(got, _oracle_stretch[k])
    assert np.array_equal(SA.bits_of(got.image), SA.bits_of(_oracle_stretch[k].image))


@pytest.mark.parametrize("target", SA.MS_TARGETS)
@pytest.mark.parametrize("name,img,mask", MASKED, ids=lambda v: v if isinstance(v, str) else "")
def test_masked_stretch_on_few_levels(ctx, oracle, name, img, mask, target):
    for protection in SA.MS_PROTECTIONS:
        stretch_both(ctx, oracle, name, img, mask, target, protection)


@pytest.mark.parametrize("target", SA.MS_TARGETS)
@pytest.mark.parametrize("name,img,mask", MASKED, ids=lambda v: v if isinstance(v, str) else "")
def test_masked_stretch_level1_in_a_pass_of_its_own(ctx, oracle, dev_build, name, img, mask, target):
    """AB_MS_NO_PREDICT (developer library, read per call): the blend pass's prediction is never declared valid, so level 1 of every
    median is histogrammed by its own pass -- the same bits as the oracle's, hence as the default form's"""
    def run():
        for protection in SA.MS_PROTECTIONS:
            stretch_both(ctx, oracle, name, img, mask, target, protection)

    _under({"AB_MS_NO_PREDICT": "1"}, run)
