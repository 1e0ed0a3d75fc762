"""csrc/masked_stretch.hip beyond its select, on the fixtures of tests/masked_adversarial.py: the star paint and the luminance
protection (planes smaller than a workgroup, stars on and outside every edge, NaN / infinite / 1e300 coordinates, any order), the
chunked enqueue past its first 32 iterations (threshold-0 loops that run out, loops that stop by their own decision in the second and
third chunk), the clamp pass and its flag (masks and protections outside [0, 1]), subnormal normalisations, degenerate ranges, and the
shared-mask form on starless fields, where it is exact.

Bar: EXACT, everywhere.  Planes through their uint32 views (a NaN equal to a NaN), every scalar with ==.  The reference is
oracle.generate_star_mask(..., stars=...) / oracle.masked_stretch(..., mask=...), computed once per fixture and never modified;
tests/test_masked_adversarial_cpu.py holds it to tests/masked_restatement.py and the fixtures to what they claim.  Host planes and
device planes; device outputs at 0 .. 3 floats past a 256-byte boundary inside a NaN-filled allocation, nothing outside them written."""
import numpy as np
import pytest

import masked_adversarial as MA
from astroburst_amd import AstroBurstError, _lib
from astroburst_amd.core import StarMaskResult
from test_gpu_crop import _dev_out, _host, assert_guard
from test_gpu_wavelet import _under

pytestmark = pytest.mark.gpu

F32 = np.float32
MASK_CASES = MA.mask_cases()
STRETCH_CASES = MA.stretch_cases()
RGB_CASES = MA.rgb_cases()
_oracle_mask, _oracle_stretch, _oracle_rgb = {}, {}, {}


def ids(cases):
    return [c.name for c in cases]


def named(cases, name):
    return next(c for c in cases if c.name == name)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=F32)).cuda()


def wanted_mask(oracle, case):
    if case.name not in _oracle_mask:
        _oracle_mask[case.name] = oracle.generate_star_mask(case.image, stars=list(case.stars), **case.cfg)
    return _oracle_mask[case.name]


def wanted_stretch(oracle, case):
    if case.name not in _oracle_stretch:
        _oracle_stretch[case.name] = oracle.masked_stretch(case.image, mask=oracle.StarMaskResult(case.mask, case.stars_masked, case.coverage),
                                                           **case.cfg)
    return _oracle_stretch[case.name]


def wanted_rgb(oracle, case):
    if case.name not in _oracle_rgb:
        _oracle_rgb[case.name] = oracle.masked_stretch_rgb_shared(case.r, case.g, case.b, **case.cfg)
    return _oracle_rgb[case.name]


def assert_mask(got, want, what):
    assert got.stars_masked == want.stars_masked, what
    assert got.coverage_fraction == want.coverage_fraction, (what, got.coverage_fraction, want.coverage_fraction)
    g = _host(got.mask)
    assert not np.isnan(g).any() and np.array_equal(g.view(np.uint32), want.mask.view(np.uint32)), \
        f"{what}: {(g.view(np.uint32) != want.mask.view(np.uint32)).sum()} of {g.size} mask pixels differ"


def assert_stretch(got, want, what):
    assert (got.iterations_run, got.converged) == (want.iterations_run, want.converged), (what, got.iterations_run, want.iterations_run)
    assert got.final_background == want.final_background, (what, got.final_background, want.final_background)
    assert got.stars_masked == want.stars_masked and got.mask_coverage == want.mask_coverage, what
    g = _host(got.image)
    assert MA.same_planes(g, want.image), f"{what}: {(~((g == want.image) | (np.isnan(g) & np.isnan(want.image)))).sum()} of {g.size} pixels differ"


# ---- star mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MASK_CASES, ids=ids(MASK_CASES))
def test_star_mask_equals_the_oracle(ctx, oracle, case):
    want = wanted_mask(oracle, case)
    stars = list(case.stars)
    pristine = case.image.copy()
    assert_mask(ctx.generate_star_mask(case.image, stars=stars, **case.cfg), want, f"{case.name}, host")
    assert MA.same_planes(case.image, pristine)
    dimg = dev(case.image)
    assert_mask(ctx.generate_star_mask(dimg, stars=stars, **case.cfg), want, f"{case.name}, device")
    n = case.image.size
    for offset in range(4):                       # the output inside a NaN-filled allocation: nothing outside the plane is written
        out, whole = _dev_out(case.image.shape, offset)
        got = ctx.generate_star_mask(dimg, stars=stars, out=out, **case.cfg)
        assert got.mask is out
        assert_mask(got, want, f"{case.name}, device, offset {offset}")
        assert_guard(whole, offset, n, f"{case.name}, offset {offset}")
    assert MA.same_planes(_host(dimg), pristine)


def test_star_order_does_not_matter(ctx, oracle):
    base, orders = MA.order_cases()
    want = wanted_mask(oracle, base)
    dimg = dev(base.image)
    first = _host(ctx.generate_star_mask(dimg, stars=list(base.stars), **base.cfg).mask)
    for case in orders:
        got = ctx.generate_star_mask(dimg, stars=list(case.stars), **case.cfg)
        assert np.array_equal(_host(got.mask).view(np.uint32), first.view(np.uint32)), case.name
        assert_mask(got, want, case.name)


# ---- masked stretch --------------------------------------------------------------------------------------------------------------
def run_stretch(ctx, case, image, mask, **extra):
    return ctx.masked_stretch(image, mask=StarMaskResult(mask, case.stars_masked, case.coverage), **case.cfg, **extra)


@pytest.mark.parametrize("case", STRETCH_CASES, ids=ids(STRETCH_CASES))
def test_masked_stretch_equals_the_oracle(ctx, oracle, case):
    want = wanted_stretch(oracle, case)
    pristine_img, pristine_mask = case.image.copy(), case.mask.copy()
    assert_stretch(run_stretch(ctx, case, case.image, case.mask), want, f"{case.name}, host")
    assert MA.same_planes(case.image, pristine_img) and MA.same_planes(case.mask, pristine_mask)
    dimg, dmask = dev(case.image), dev(case.mask)
    assert_stretch(run_stretch(ctx, case, dimg, dmask), want, f"{case.name}, device")
    n = case.image.size
    for offset in range(4):
        out, whole = _dev_out(case.image.shape, offset)
        got = run_stretch(ctx, case, dimg, dmask, out=out)
        assert got.image is out
        assert_stretch(got, want, f"{case.name}, device, offset {offset}")
        assert_guard(whole, offset, n, f"{case.name}, offset {offset}")
    assert MA.same_planes(_host(dimg), pristine_img) and MA.same_planes(_host(dmask), pristine_mask)


LONG_AND_CLAMP = [c for c in STRETCH_CASES if c.name.startswith(("M-long", "M-clamp"))]


@pytest.mark.parametrize("case", LONG_AND_CLAMP, ids=ids(LONG_AND_CLAMP))
def test_long_loops_with_level1_in_a_pass_of_its_own(ctx, oracle, dev_build, case):
    """AB_MS_NO_PREDICT (developer library, read per call): level 1 of every median takes its own pass -- the same results"""
    want = wanted_stretch(oracle, case)
    dimg, dmask = dev(case.image), dev(case.mask)

    def run():
        assert_stretch(run_stretch(ctx, case, dimg, dmask), want, f"{case.name}, device, no prediction")
        assert_stretch(run_stretch(ctx, case, case.image, case.mask), want, f"{case.name}, host, no prediction")

    _under({"AB_MS_NO_PREDICT": "1"}, run)


# ---- shared mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RGB_CASES, ids=ids(RGB_CASES))
def test_shared_mask_on_a_starless_field_is_exact(ctx, oracle, case):
    *want, want_mask = wanted_rgb(oracle, case)
    assert want_mask.stars_masked == 0
    planes = (case.r, case.g, case.b)
    devs = [dev(p) for p in planes]
    n = case.r.size

    def check(got, what):
        *chans, shared = got
        assert (shared.stars_masked, shared.coverage_fraction) == (0, want_mask.coverage_fraction), what
        for k, (g, w) in enumerate(zip(chans, want)):
            assert_stretch(g, w, f"{case.name}, {what}, channel {k}")

    check(ctx.masked_stretch_rgb_shared(*planes, **case.cfg), "host")
    check(ctx.masked_stretch_rgb_shared(*devs, **case.cfg), "device")
    outs = [_dev_out(case.r.shape, offset) for offset in (1, 2, 3)]
    got = ctx.masked_stretch_rgb_shared(*devs, outs=[o for o, _ in outs], **case.cfg)
    check(got, "device, guarded outputs")
    for offset, (_, whole) in zip((1, 2, 3), outs):
        assert_guard(whole, offset, n, f"{case.name}, offset {offset}")
    # the same as the pieces: luminance, the mask of an empty detection, one stretch per channel
    mask_cfg = dict(growth_factor=case.cfg.get("mask_growth", 2.5), softness=case.cfg.get("mask_softness", 4.0), luminance_protect=True,
                    luminance_ceiling=case.cfg.get("luminance_ceiling", 0.85))
    mask = ctx.generate_star_mask(ctx.luminance(*devs), stars=[], **mask_cfg)
    assert_mask(mask, want_mask, f"{case.name}, pieces")
    for k, (d, g) in enumerate(zip(devs, got[:3])):
        piece = ctx.masked_stretch(d, mask=mask, **case.cfg)
        assert (piece.iterations_run, piece.converged, piece.final_background, piece.stars_masked, piece.mask_coverage) == \
               (g.iterations_run, g.converged, g.final_background, g.stars_masked, g.mask_coverage), (case.name, k)
        assert MA.same_planes(_host(piece.image), _host(g.image)), (case.name, k)
    for d, p in zip(devs, planes):
        assert MA.same_planes(_host(d), p)


# ---- state between calls ---------------------------------------------------------------------------------------------------------
def test_state_does_not_leak_between_calls(ctx, oracle):
    """a 65-iteration loop, a 1 x 1 plane, a clamped plane, the 65-iteration loop again: workspaces grow and are reused, the loop state
    and the histograms start afresh"""
    long65 = named(STRETCH_CASES, "M-long-t0-65")
    order = [long65, named(STRETCH_CASES, "M-tiny-1x1-default"), named(STRETCH_CASES, "M-clamp-p2.0-65"), long65,
             named(STRETCH_CASES, "M-long-self-2.2"), named(STRETCH_CASES, "M-clamp-p-0.5-6"), long65]
    planes = {c.name: (dev(c.image), dev(c.mask)) for c in order}
    got = [run_stretch(ctx, c, *planes[c.name]) for c in order]
    for c, g in zip(order, got):
        assert_stretch(g, wanted_stretch(oracle, c), c.name)
    first = got[0]
    for again in (got[3], got[6]):
        assert (again.iterations_run, again.converged, again.final_background) == (first.iterations_run, first.converged, first.final_background)
        assert np.array_equal(_host(again.image).view(np.uint32), _host(first.image).view(np.uint32))


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def invalid(fn):
    with pytest.raises(AstroBurstError) as e:
        fn()
    assert e.value.code == _lib.AB_ERR_INVALID, e.value


def test_bad_dimensions_are_refused_and_touch_nothing(ctx, oracle):
    import torch
    case = named(STRETCH_CASES, "M-tiny-16x16-default")
    img, mask = dev(case.image), dev(case.mask)
    sm = StarMaskResult(mask, case.stars_masked, case.coverage)
    for shape in ((0, 16), (16, 0), (0, 0)):
        z = np.zeros(shape, F32)
        zm = StarMaskResult(z, 0, 0.0)
        invalid(lambda: ctx.generate_star_mask(z))
        invalid(lambda: ctx.generate_star_mask(z, stars=[(1.0, 1.0, 2.0)]))
        invalid(lambda: ctx.masked_stretch(z))
        invalid(lambda: ctx.masked_stretch(z, mask=zm))
        invalid(lambda: ctx.masked_stretch_rgb_shared(z, z, z))
    wrong, whole = _dev_out((16, 15), 1)
    wrong_mask = StarMaskResult(torch.zeros((15, 16), device="cuda"), 0, 0.0)
    invalid(lambda: ctx.generate_star_mask(img, out=wrong))
    invalid(lambda: ctx.generate_star_mask(img, stars=[(8.0, 8.0, 2.0)], out=wrong))
    invalid(lambda: ctx.masked_stretch(img, out=wrong))
    invalid(lambda: ctx.masked_stretch(img, mask=sm, out=wrong))
    invalid(lambda: ctx.masked_stretch(img, mask=wrong_mask))
    right = [_dev_out((16, 16), k) for k in (0, 2)]
    invalid(lambda: ctx.masked_stretch_rgb_shared(img, img, img, outs=[right[0][0], wrong, right[1][0]]))
    invalid(lambda: ctx.masked_stretch_rgb_shared(img, img[:15].contiguous(), img))
    for w in (whole, right[0][1], right[1][1]):
        assert torch.isnan(w).all()                # the outputs are as they were
    assert_stretch(ctx.masked_stretch(img, mask=sm, **case.cfg), wanted_stretch(oracle, case), "after the refusals")
