"""HIP parity of the fused tone preview (csrc/tone.hip, ab_apply_tone_composite) on one MI355X.

Three references:
  1 the library's own unfused chain (tone_restatement.unfused_chain: apply_stf_f32 x 3 -> apply_levels x 3 -> apply_curve x 3 ->
    apply_scnr_inplace -> render_rgb_preview): the same arithmetic on the same device, so planes and bytes are compared with
    array_equal (equal_nan), no tolerance;
  2 the oracle composition (tone_restatement.compose) where levels are not applied: every operation is an IEEE basic operation or a
    table lookup, so array_equal again;
  3 the oracle composition where levels are applied: the device pow and the host pow may differ in the last f64 bit, which can move an
    f32 rounding.  Planes of a case without curves: rtol 1e-6, atol 1e-30 (test_gpu_color.py::test_levels' tolerance for this pow).
    Bytes of every levels case: at most 1 byte in 10^4 may differ, each by exactly 1 (these cases use only the identity LUT and the
    S-curve, whose steps between neighbouring LUT entries stay far below 1 / 255, so one moved LUT index cannot move a byte by more).
    The largest small plane (67 x 131 x 3 = 26 331 bytes) keeps that cap from being vacuous.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import tone_restatement as T
from astroburst_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
# (shape, max_dim): both ratios non-integer; preview rows round to 0 -> 1; the same transposed; single pixels; no sampling with cols
# not a multiple of 4; exact fit
SHAPES = [((150, 203), 64), ((9, 1000), 7), ((1000, 9), 7), ((1, 1), 4), ((1, 5), 4), ((67, 131), 4096), ((64, 64), 64)]
SHAPE_IDS = [f"{s[0]}x{s[1]}@{m}" for s, m in SHAPES]
TURN = (1450, 1501)   # 2 176 450 px: more quads than the 2048 x 256 lanes of the largest grid, so every grid-stride loop turns

SCNR_ALL = {f"scnr_{m}_{'preserve' if p else 'plain'}": dict(scnr=dict(method=m, amount=0.7, preserve_luminance=p))
            for m in ("average", "maximum") for p in (False, True)}
DENOMINATOR = ((0.0, 2.0, 1.0),) * 3   # midtone 2: the MTF's denominator 3 x - 2 vanishes at the f64 nearest 2 / 3 (test_gpu_rgb_export.py:138)
# name -> (configuration, which statistics)
GPU_TABLE = {
    **{n: (T.PLAN_TABLE[n], "own") for n in ("auto_unlinked", "auto_linked", "one_explicit_linked", "levels_identity_within", "levels_gamma_just_outside",
                                             "levels_one_channel", "levels_three", "curves_some_empty", "curves_one_off_with_empty_and_diagonal",
                                             "curves_three_collinear", "curves_s_and_none", "curves_unsorted_duplicate_x", "scnr_amount_1e-7",
                                             "scnr_amount_2e-7", "everything")},
    **{n: (c, "own") for n, c in SCNR_ALL.items()},
    "levels_and_s_curve_linked": (dict(linked_stf=True, levels=(None, (0.05, 2.2, 0.95), None), curves=(None, T.S_CURVE, None)), "own"),
    "denominator_scnr": (dict(stf=DENOMINATOR, scnr=dict(method="maximum", amount=1.0, preserve_luminance=True)), "denominator"),
    "denominator_levels_scnr": (dict(stf=DENOMINATOR, levels=((0.1, 1.8, 0.9), None, None), scnr=dict(method="average", amount=0.6)), "denominator"),
    "denominator_curves": (dict(stf=DENOMINATOR, curves=(None, T.S_CURVE, None)), "denominator"),
    "flat_statistics": (dict(levels=(None, None, (0.0, 0.8, 1.0))), "flat"),
    "flat_statistics_linked": (dict(linked_stf=True, scnr=dict(method="average", amount=1.0)), "flat"),
}


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _dev(a, offset=1):
    """the array on the device, `offset` floats past a 256-byte boundary (1: one float past a 16-byte boundary)"""
    import torch
    a = np.array(a, copy=True, order="C")
    buf = torch.empty(a.size + offset + 64, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view


def _host_off(a):
    """a host copy that starts one float past a 16-byte boundary"""
    buf = np.empty(a.size + 8, F32)
    k = ((4 - buf.ctypes.data) % 16) // 4
    view = buf[k:k + a.size].reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 16 == 4 and view.flags.c_contiguous
    return view


def _dev_bytes(shape, offset):
    """a zeroed uint8 device buffer of `shape` at `offset` bytes past a 256-byte boundary, and the whole allocation (with a guard band)"""
    import torch
    n = int(np.prod(shape))
    buf = torch.zeros(n + offset + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf[offset:offset + n].view(shape), buf


@functools.lru_cache(maxsize=None)
def _planes(shape):
    """three planes from one seeded uniform(-0.2, 1.3) with NaN, +-inf, -0.0, 0, 1e-8 (below the padding threshold) and 1.0 planted"""
    rng = np.random.default_rng(20260 + 7 * shape[0] + shape[1])
    out = []
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-8, 1.0]
    n = shape[0] * shape[1]
    for c in range(3):
        a = rng.uniform(-0.2, 1.3, shape).astype(F32)
        flat = a.reshape(-1)
        if n >= 64:
            pos = rng.choice(n, 4 * len(special), replace=False)
            for i, p in enumerate(pos):
                flat[p] = special[i % len(special)]
            flat[pos[0] + 1 if pos[0] + 1 < n else 0] = 1.0   # (1.0 right beside a NaN: both in one group of four)
        elif n > 1:
            flat[c % n] = special[(2 * c) % len(special)]
            flat[(c + 2) % n] = 1.0
        else:
            flat[0] = [1.0, np.nan, 0.4][c]
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _own_stats(shape):
    from oracle import pyoracle
    return tuple(pyoracle.compute_image_stats(x) for x in _planes(shape))


def _stats(oracle, shape, kind):
    if kind == "own":
        return list(_own_stats(shape))
    return T.denominator_stats(oracle) if kind == "denominator" else T.flat_stats(oracle)


def _same(got, want):
    return np.array_equal(_host(got), np.asarray(want), equal_nan=True)


def assert_same(got, want, what):
    got, want = _host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} != {want.dtype} {want.shape}"
    if not np.array_equal(got, want, equal_nan=True):
        bad = np.flatnonzero(~((got == want) | ((got != got) & (want != want))).ravel())
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: got {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}")


def assert_bytes_within_one_in_1e4(got, want, what):
    got, want = _host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, what
    d = np.abs(got.astype(np.int16) - want.astype(np.int16)).ravel()
    ndiff = int(np.count_nonzero(d))
    print(f"{what}: {ndiff} of {d.size} bytes differ, max step {int(d.max()) if d.size else 0}")
    assert d.size == 0 or int(d.max()) <= 1, f"{what}: a byte differs by {int(d.max())}"
    assert ndiff * 10 ** 4 <= d.size, f"{what}: {ndiff} of {d.size} bytes differ (more than 1 in 10^4)"


def assert_against_oracle(got_planes, got_bytes, want_planes, want_bytes, pl, what):
    if not pl["levels_applied"]:
        for c in range(3):
            assert_same(got_planes[c], want_planes[c], f"{what}: oracle plane {c}")
        assert_same(got_bytes, want_bytes, f"{what}: oracle bytes")
        return
    if not pl["curves_applied"]:
        for c in range(3):
            np.testing.assert_allclose(_host(got_planes[c]), want_planes[c], rtol=1e-6, atol=1e-30, equal_nan=True, err_msg=f"{what}: oracle plane {c}")
    assert_bytes_within_one_in_1e4(got_bytes, want_bytes, f"{what}: oracle bytes")


def assert_info(ctx, info, stats, cfg, shape, max_dim, what):
    plan, _ = ctx.tone_plan(stats, **cfg)
    assert (info.stf, info.norm, info.levels_applied, info.curves_applied, info.scnr_applied) == \
        (plan.stf, plan.norm, plan.levels_applied, plan.curves_applied, plan.scnr_applied), what
    assert (info.rows, info.cols) == shape and (info.preview_rows, info.preview_cols) == ctx.preview_dims(shape[0], shape[1], max_dim), what


def _check(ctx, oracle, shape, max_dim, name, out_off):
    cfg, kind = GPU_TABLE[name]
    r, g, b = _planes(shape)
    stats = _stats(oracle, shape, kind)
    what = f"{name} {shape} max_dim {max_dim}"
    want_planes, want_bytes, pl = T.compose(oracle, r, g, b, stats, max_dim, **cfg)
    dev = [_dev(x) for x in (r, g, b)]
    chain_planes, chain_bytes = T.unfused_chain(ctx, *[d.clone() for d in dev], stats, max_dim, **cfg)
    above = want_bytes.shape[:2] != shape
    # device inputs, planes and bytes (two launches above max_dim)
    full = ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, want_planes=True, **cfg)
    assert full.rgb8.shape == want_bytes.shape, what
    for c in range(3):
        assert_same(full.planes[c], _host(chain_planes[c]), f"{what}: chain plane {c}")
    assert_same(full.rgb8, _host(chain_bytes), f"{what}: chain bytes")
    assert_against_oracle(full.planes, full.rgb8, want_planes, want_bytes, pl, what)
    assert_info(ctx, full.info, stats, cfg, shape, max_dim, what)
    # device inputs, bytes only, at a byte offset of the output (sampled above max_dim): equal to the pick of the planes above
    out, whole = _dev_bytes(want_bytes.shape, out_off)
    only = ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, out=out, **cfg)
    assert only.planes is None and only.rgb8 is out
    assert_same(out, _host(chain_bytes), f"{what}: bytes only at +{out_off}")
    if above:
        assert_same(out, _host(ctx.render_rgb_preview(*full.planes, max_dim)), f"{what}: sampled against the pick of the full planes")
    whole = _host(whole)
    assert not whole[:out_off].any() and not whole[out_off + want_bytes.size:].any(), f"{what}: wrote outside the output"
    assert_info(ctx, only.info, stats, cfg, shape, max_dim, what)
    # host inputs one float past a 16-byte boundary, host outputs
    hosted = ctx.apply_tone_composite(*[_host_off(x) for x in (r, g, b)], stats, max_dim=max_dim, want_planes=True, **cfg)
    assert isinstance(hosted.rgb8, np.ndarray) and isinstance(hosted.planes[0], np.ndarray)
    for c in range(3):
        assert_same(hosted.planes[c], _host(full.planes[c]), f"{what}: host plane {c}")
    assert_same(hosted.rgb8, _host(full.rgb8), f"{what}: host bytes")
    assert_same(ctx.apply_tone_composite(r, g, b, stats, max_dim=max_dim, **cfg).rgb8, _host(full.rgb8), f"{what}: host bytes only")


@pytest.mark.parametrize("name", list(GPU_TABLE))
def test_fused_tone_equals_the_chain_and_the_oracle(ctx, oracle, name):
    for i, (shape, max_dim) in enumerate(SHAPES):
        _check(ctx, oracle, shape, max_dim, name, (i + len(name)) % 4)


@pytest.mark.parametrize("name", ["auto_unlinked", "levels_one_channel", "everything"])
@pytest.mark.parametrize("shape_dim", SHAPES, ids=SHAPE_IDS)
def test_bytes_at_every_offset_of_the_output(ctx, oracle, shape_dim, name):
    """out_rgb8 at byte offsets 0, 1, 2 and 3 of a device buffer, sampled and full: the same bytes, nothing outside them"""
    (shape, max_dim), (cfg, kind) = shape_dim, GPU_TABLE[name]
    stats = _stats(oracle, shape, kind)
    dev = [_dev(x) for x in _planes(shape)]
    want = _host(ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, **cfg).rgb8)
    for off in range(4):
        for planes in (False, True):
            out, whole = _dev_bytes(want.shape, off)
            res = ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, want_planes=planes, out=out, **cfg)
            assert_same(out, want, f"+{off} bytes, planes {planes}")
            whole = _host(whole)
            assert not whole[:off].any() and not whole[off + want.size:].any(), f"+{off}: wrote outside the output"
            if planes:
                assert_same(ctx.render_rgb_preview(*res.planes, max_dim), want, f"+{off}: the pick of the returned planes")


def test_planes_without_bytes(ctx, oracle):
    (shape, max_dim), (cfg, kind) = SHAPES[0], GPU_TABLE["everything"]
    stats = _stats(oracle, shape, kind)
    dev = [_dev(x) for x in _planes(shape)]
    both = ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, want_planes=True, **cfg)
    alone = ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, want_planes=True, want_rgb8=False, **cfg)
    assert alone.rgb8 is None
    for c in range(3):
        assert_same(alone.planes[c], _host(both.planes[c]), f"plane {c}")


@pytest.mark.parametrize("name", ["auto_unlinked", "everything"])
def test_when_the_grid_loops_turn(ctx, oracle, name):
    """more pixels than one pass of the persistent grid (three workgroups per CU with the LUTs in LDS, eight without): full size and
    sampled at max_dim 512"""
    cfg, kind = GPU_TABLE[name]
    r, g, b = _planes(TURN)
    stats = _stats(oracle, TURN, kind)
    dev = [_dev(x) for x in (r, g, b)]
    want_planes, want_bytes, pl = T.compose(oracle, r, g, b, stats, 4096, **cfg)
    chain_planes, chain_bytes = T.unfused_chain(ctx, *[d.clone() for d in dev], stats, 4096, **cfg)
    full = ctx.apply_tone_composite(*dev, stats, max_dim=4096, want_planes=True, **cfg)
    for c in range(3):
        assert_same(full.planes[c], _host(chain_planes[c]), f"chain plane {c}")
    assert_same(full.rgb8, _host(chain_bytes), "chain bytes")
    assert_against_oracle(full.planes, full.rgb8, want_planes, want_bytes, pl, f"{name} {TURN}")
    small = ctx.apply_tone_composite(*dev, stats, max_dim=512, **cfg)
    assert_same(small.rgb8, _host(ctx.render_rgb_preview(*full.planes, 512)), "sampled at 512 against the pick of the full planes")
    assert_info(ctx, small.info, stats, cfg, TURN, 512, name)


def test_a_second_call_with_other_curves_uses_them(ctx, oracle):
    """the LUTs stay on the device between calls and are uploaded again only when they change: change them, change them back"""
    (shape, max_dim), kind = SHAPES[5], "own"
    stats = _stats(oracle, shape, kind)
    dev = [_dev(x) for x in _planes(shape)]
    a, b = GPU_TABLE["curves_s_and_none"][0], GPU_TABLE["curves_unsorted_duplicate_x"][0]
    first = _host(ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, **a).rgb8)
    other = _host(ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, **b).rgb8)
    again = _host(ctx.apply_tone_composite(*dev, stats, max_dim=max_dim, **a).rgb8)
    assert_same(again, first, "the first curves again")
    assert_same(other, T.compose(oracle, *_planes(shape), stats, max_dim, **b)[1], "the other curves")
    assert not np.array_equal(first, other)


def test_invalid_arguments_with_a_live_context(ctx, oracle):
    """NULL arguments, max_dim 0, both outputs NULL, mismatched dims, an output over an input: AB_ERR_INVALID with a message, and the
    outputs stay as they were"""
    import torch
    L, h = ctx._L, ctx._h
    shape = (8, 12)
    t = [torch.rand(shape, device="cuda") for _ in range(3)]
    small = torch.rand((8, 11), device="cuda")
    p = [_lib.Plane(C.c_void_p(x.data_ptr()), *shape, 1) for x in t]
    ps = _lib.Plane(C.c_void_p(small.data_ptr()), 8, 11, 1)
    st = (_lib.ImageStatsC * 3)(*[_lib.ImageStatsC(0.0, 1.0, 0.3, 0.05, 0.07, 0.35, 96)] * 3)
    cfg, info = _lib.ToneConfigC(), _lib.ToneInfoC()
    L.ab_tone_config_default(C.byref(cfg))
    out = torch.zeros(8 * 12 * 3, dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(shape, device="cuda") for _ in range(3)]
    po = (_lib.Plane * 3)(*[_lib.Plane(C.c_void_p(x.data_ptr()), *shape, 1) for x in outs])
    po_bad = (_lib.Plane * 3)(po[0], _lib.Plane(C.c_void_p(outs[1].data_ptr()), 12, 8, 1), po[2])
    po_over = (_lib.Plane * 3)(po[0], po[1], _lib.Plane(C.c_void_p(t[0].data_ptr()), *shape, 1))
    ob = C.c_void_p(out.data_ptr())
    r, g, b = (C.byref(x) for x in p)
    cases = {
        "null R": (None, g, b, st, C.byref(cfg), 64, None, ob),
        "null B": (r, g, None, st, C.byref(cfg), 64, None, ob),
        "null statistics": (r, g, b, None, C.byref(cfg), 64, None, ob),
        "null configuration": (r, g, b, st, None, 64, None, ob),
        "max_dim 0": (r, g, b, st, C.byref(cfg), 0, None, ob),
        "max_dim -3": (r, g, b, st, C.byref(cfg), -3, None, ob),
        "both outputs null": (r, g, b, st, C.byref(cfg), 64, None, None),
        "G of other dims": (r, C.byref(ps), b, st, C.byref(cfg), 64, None, ob),
        "an output plane of other dims": (r, g, b, st, C.byref(cfg), 64, po_bad, ob),
        "an output plane over an input": (r, g, b, st, C.byref(cfg), 64, po_over, ob),
        "the bytes over an input": (r, g, b, st, C.byref(cfg), 2, None, C.c_void_p(t[1].data_ptr())),
    }
    before = [x.clone() for x in t]
    for what, (a0, a1, a2, s, c, md, planes, bytes_) in cases.items():
        rc = L.ab_apply_tone_composite(h, a0, a1, a2, s, c, md, planes, bytes_, 1, C.byref(info))
        assert rc == _lib.AB_ERR_INVALID, what
        assert L.ab_last_error(h), what
    torch.cuda.synchronize()
    assert not out.any().item() and not any(x.any().item() for x in outs)
    assert all(torch.equal(x, y) for x, y in zip(t, before))
    rc = L.ab_apply_tone_composite(h, r, g, b, st, C.byref(cfg), 64, po, ob, 1, None)   # info is optional; and the context still works
    assert rc == _lib.AB_OK
    ctx.synchronize()
    assert out.any().item()
