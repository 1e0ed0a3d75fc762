"""HIP parity of the colour finish (csrc/rgb_export.hip) on one MI355X: the RGB packers, the fused stretch + pack, the export
command's stretch_and_render, process_drizzle_rgb and drizzle_rgb, against tests/rgb_export_restatement.py (numpy + the oracle's
existing functions; pinned by tests/test_rgb_export_cpu.py).

There are no tolerances here: bytes are compared with array_equal, f32 planes through their uint32 views, scalars with ==.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import rgb_export_restatement as R
from astroburst_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL_SHAPES = R.SHAPES + [R.BIG]
SHAPE_IDS = ["x".join(map(str, s)) for s in ALL_SHAPES]
PACK_IDS = ["u8", "u8round", "u16be"]


def _dev(a, offset=0):
    """the array on the device; offset > 0: at a pointer `offset` elements past a 256-byte aligned allocation"""
    import torch
    a = np.array(a, copy=True, order="C")   # (the cached fixtures are read-only)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + offset + 64, dtype=torch.from_numpy(a).dtype, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() == buf.data_ptr() + offset * a.itemsize and view.is_contiguous()
    return view


def _dev_bytes(shape, offset):
    """a zeroed uint8 device buffer of `shape` at `offset` bytes past a 256-byte boundary, and the whole allocation (with a guard band)"""
    import torch
    n = int(np.prod(shape))
    buf = torch.zeros(n + offset + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf[offset:offset + n].view(shape), buf


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_bytes(got, want, what):
    got = _host(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} != {want.shape}"
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: got {got.ravel()[bad[0]]} want {want.ravel()[bad[0]]}"


def assert_bits(got, want, what):
    got, want = _host(got), np.asarray(want, F32)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: got {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def _cases(shape):
    out = R.cases(shape)
    for v in out.values():
        v.setflags(write=False)
    return out


def _triple(shape, names):
    c = _cases(shape)
    return [c[n] for n in names]


# ---- ab_render_rgb ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", R.PACKS, ids=PACK_IDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_render_rgb_host_and_device(ctx, shape, pack):
    for names in R.TRIPLES:
        r, g, b = _triple(shape, names)
        want = R.pack_rgb(r, g, b, pack)
        assert_bytes(ctx.render_rgb(r, g, b, pack), want, f"host {names}")
        assert_bytes(ctx.render_rgb(_dev(r), _dev(g), _dev(b), pack), want, f"device {names}")


@pytest.mark.parametrize("pack", R.PACKS, ids=PACK_IDS)
@pytest.mark.parametrize("shape", [(1, 3), (1, 5), (5, 13), (33, 65)], ids=["1x3", "1x5", "5x13", "33x65"])
def test_render_rgb_at_any_address(ctx, shape, pack):
    """device inputs 1 and 3 floats past a 256-byte boundary, device outputs 1, 2 and 3 bytes past one: the same bytes, and not one
    byte outside the output"""
    r, g, b = _triple(shape, R.TRIPLES[0])
    want = R.pack_rgb(r, g, b, pack)
    for in_off, out_off in itertools.product((0, 1, 3), (0, 1, 2, 3)):
        out, whole = _dev_bytes(want.shape, out_off)
        ctx.render_rgb(_dev(r, in_off), _dev(g, in_off), _dev(b, (in_off * 2) % 4), pack, out=out)
        assert_bytes(out, want, f"inputs +{in_off} floats, output +{out_off} bytes")
        whole = _host(whole)
        assert not whole[:out_off].any() and not whole[out_off + want.size:].any(), f"+{in_off} / +{out_off}: wrote outside the output"


def test_render_rgb_truncating_equals_the_full_size_preview(ctx):
    for shape in ((5, 13), (33, 65)):
        r, g, b = (_dev(x) for x in _triple(shape, R.TRIPLES[0]))
        assert_bytes(ctx.render_rgb(r, g, b, R.PACK_8), _host(ctx.render_rgb_preview(r, g, b, max(shape))), f"{shape}")


def test_render_rgb_when_the_grid_loop_turns(ctx):
    c = R.cases(R.TURN)
    r, g, b = c["uniform"], c["nasty"], c["ramp"]
    dr, dg, db = _dev(r), _dev(g), _dev(b)
    for pack in R.PACKS:
        assert_bytes(ctx.render_rgb(dr, dg, db, pack), R.pack_rgb(r, g, b, pack), f"pack {pack}")


# ---- ab_render_rgb_stf -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", R.PACKS, ids=PACK_IDS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=SHAPE_IDS)
def test_render_rgb_stf_auto_parameters(ctx, oracle, shape, pack):
    for names in R.TRIPLES[:2]:
        planes = _triple(shape, names)
        st = [oracle.compute_image_stats(x) for x in planes]
        stf = [oracle.auto_stf(s) for s in st]
        want = R.pack_rgb(*[oracle.apply_stf_f32(x, p, s) for x, p, s in zip(planes, stf, st)], pack)
        assert_bytes(ctx.render_rgb_stf(*planes, stf, st, pack), want, f"host {names}")
        dev = [_dev(x) for x in planes]
        assert_bytes(ctx.render_rgb_stf(*dev, stf, st, pack), want, f"device {names}")
        # the library's own unfused chain
        chain = ctx.render_rgb(*[ctx.apply_stf_f32(x, p, s) for x, p, s in zip(dev, stf, st)], pack)
        assert_bytes(chain, want, f"apply_stf_f32 x 3 + render_rgb {names}")


@pytest.mark.parametrize("pack", R.PACKS, ids=PACK_IDS)
def test_render_rgb_stf_zero_mtf_denominator(ctx, oracle, pack):
    """midtone 2, shadow 0, highlight 1: the MTF's denominator (2 m - 1) x - m is 3 x - 2, exactly 0 where the normalised value is the
    f64 nearest 2 / 3 (pixel 1.0 with min 0 and max 1.5: 1 / 1.5 rounds to it and 3 x rounds to 2).  The quotient is +inf there, which the
    packer's clamp sends to the top sample; its neighbours come out huge, negative or ordinary.  The bytes follow from the same IEEE
    operations as the reference's."""
    x = np.array([[1.0, 0.999999, 1.000001, 0.5, 1.2, 1.5, 0.0, 1e-8, 1.0, 0.25, np.nan, 1.0, 0.75]], F32)
    st = oracle.ImageStats(0.0, 1.5, 0.6, 0.1, 0.15, 0.6, 13)
    p = oracle.StfParams(0.0, 2.0, 1.0)
    s = oracle.apply_stf_f32(x, p, st)
    assert np.isposinf(s[0, 0]) and np.isposinf(s[0, 8])
    want = R.pack_rgb(s, s, s, pack)
    assert want[0, 0, 0] == 255
    assert_bytes(ctx.render_rgb_stf(_dev(x), _dev(x), _dev(x), [p] * 3, [st] * 3, pack), want, "device")
    assert_bytes(ctx.render_rgb_stf(x, x, x, [p] * 3, [st] * 3, pack), want, "host")


# ---- ab_export_rgb ---------------------------------------------------------------------------------------------------------------------
def _check_export(ctx, oracle, planes, bits, stf, device):
    want, winfo = R.stretch_and_render(oracle, *planes, bits, stf)
    src = [_dev(x) for x in planes] if device else planes
    got, info = ctx.export_rgb(*src, bits=bits, stf=stf)
    what = f"bits {bits} {'explicit' if stf else 'linked'} {'device' if device else 'host'}"
    assert (info.rows, info.cols, info.resampled) == (winfo["rows"], winfo["cols"], winfo["resampled"]), what
    assert [R.stats_tuple(s) for s in info.stats] == winfo["stats"], what
    assert [(p.shadow, p.midtone, p.highlight) for p in info.stf] == winfo["stf"], what
    assert_bytes(got, want, what)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("shape", [(1, 1), (5, 13), (33, 65)], ids=["1x1", "5x13", "33x65"])
def test_export_rgb(ctx, oracle, shape, bits):
    explicit = [oracle.StfParams(0.01, 0.2, 0.95), oracle.StfParams(0.0, 0.35, 1.0), oracle.StfParams(0.05, 0.5, 0.9)]
    for names in R.TRIPLES[:2]:
        planes = _triple(shape, names)
        for stf in (None, explicit):
            _check_export(ctx, oracle, planes, bits, stf, device=True)
        _check_export(ctx, oracle, planes, bits, None, device=False)


@pytest.mark.parametrize("bits", [8, 16])
def test_export_rgb_resamples_to_the_largest_dims(ctx, oracle, bits):
    rng = np.random.default_rng(3)
    planes = [rng.random(s, dtype=F32) for s in ((16, 16), (12, 16), (16, 10))]
    _check_export(ctx, oracle, planes, bits, None, device=True)
    _check_export(ctx, oracle, planes, bits, None, device=False)


# ---- ab_process_drizzle_rgb --------------------------------------------------------------------------------------------------------------
WB = {"auto": "auto", "none": "none", "manual": (1.0, 0.7, 1.3)}
STRETCH = {"linked": (True, True), "unlinked": (True, False), "off": (False, False)}
SCNR = {"noscnr": None, "average": dict(method="average", amount=0.8, preserve_luminance=True), "maximum": dict(method="maximum", amount=1.0)}


def _check_process(ctx, oracle, planes, wb, stretch, scnr, device=True, want=(True, True, True), what=""):
    auto, linked = STRETCH[stretch]
    ref = R.process_drizzle_rgb(oracle, *planes, white_balance=WB[wb], auto_stretch=auto, linked_stf=linked, scnr=SCNR[scnr])
    src = [None if x is None else (_dev(x) if device else x) for x in planes]
    got = ctx.process_drizzle_rgb(*src, white_balance=WB[wb], auto_stretch=auto, linked_stf=linked, scnr=SCNR[scnr], want_stretched=want[0],
                                  want_wb=want[1], want_rgb8=want[2])
    what = f"{what} {wb} {stretch} {scnr} {'device' if device else 'host'} want={want}"
    assert (got.rows, got.cols) == (ref["rows"], ref["cols"]), what
    assert got.wb_factors == ref["wb_factors"], what
    assert [(p.shadow, p.midtone, p.highlight) for p in got.stf] == ref["stf"], what
    assert [tuple(c) for c in got.chan_stats] == ref["chan_stats"], what
    assert [R.stats_tuple(s) for s in got.stats_wb] == ref["stats_wb"], what
    assert got.scnr_applied == ref["scnr_applied"], what
    assert (got.stretched is not None, got.wb is not None, got.rgb8 is not None) == tuple(want), what
    for c in range(3):
        if want[0]:
            assert_bits(got.stretched[c], ref["stretched"][c], f"{what}: stretched {'RGB'[c]}")
        if want[1]:
            assert_bits(got.wb[c], ref["wb"][c], f"{what}: wb {'RGB'[c]}")
    if want[2]:
        assert_bytes(got.rgb8, ref["rgb8"], f"{what}: rgb8")


@pytest.mark.parametrize("scnr", list(SCNR))
@pytest.mark.parametrize("stretch", list(STRETCH))
@pytest.mark.parametrize("wb", list(WB))
def test_process_drizzle_rgb_every_mode(ctx, oracle, wb, stretch, scnr):
    _check_process(ctx, oracle, _triple((33, 65), R.TRIPLES[0]), wb, stretch, scnr)


@pytest.mark.parametrize("shape", [s for s in ALL_SHAPES if s != (33, 65)], ids=[i for i in SHAPE_IDS if i != "33x65"])
def test_process_drizzle_rgb_other_shapes(ctx, oracle, shape):
    _check_process(ctx, oracle, _triple(shape, R.TRIPLES[0]), "auto", "linked", "average")
    _check_process(ctx, oracle, _triple(shape, R.TRIPLES[1]), "manual", "off", "noscnr")
    _check_process(ctx, oracle, _triple(shape, R.TRIPLES[2]), "none", "unlinked", "maximum", device=False)


@pytest.mark.parametrize("absent", [0, 1, 2])
def test_process_drizzle_rgb_absent_channel(ctx, oracle, absent):
    planes = _triple((33, 65), R.TRIPLES[0])
    planes[absent] = None
    _check_process(ctx, oracle, planes, "auto", "linked", "average", what=f"absent {absent}")
    _check_process(ctx, oracle, planes, "manual", "unlinked", "noscnr", device=False, what=f"absent {absent}")


def test_process_drizzle_rgb_crops_top_left(ctx, oracle):
    rng = np.random.default_rng(11)
    planes = [rng.random(s, dtype=F32) for s in ((33, 65), (31, 65), (33, 60))]
    for device in (True, False):
        _check_process(ctx, oracle, planes, "auto", "linked", "average", device=device, what="cropped")
        _check_process(ctx, oracle, planes, "none", "off", "noscnr", device=device, what="cropped")


@pytest.mark.parametrize("want", [w for w in itertools.product((True, False), repeat=3) if w != (True, True, True)],
                         ids=lambda w: "".join("swb"[i] if x else "-" for i, x in enumerate(w)))
def test_process_drizzle_rgb_nullable_outputs(ctx, oracle, want):
    _check_process(ctx, oracle, _triple((5, 13), R.TRIPLES[0]), "auto", "linked", "average", want=want)
    _check_process(ctx, oracle, _triple((5, 13), R.TRIPLES[0]), "manual", "unlinked", "maximum", device=False, want=want)


# ---- ab_drizzle_rgb ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drizzle_frames():
    from astroburst_amd import synth
    cat = synth.star_catalog(24, 20, 6, seed=9)
    out = []
    for c in range(3):
        out.append([synth.make_frame(24, 20, 10 * c + k, cat=cat, sky=200.0 + 40.0 * c, bad_patch_rate=0.0).numpy() for k in range(3)])
    return out


DRZ = dict(scale=2.0, pixfrac=0.7, kernel="square", align=False)


def _check_drizzle_rgb(ctx, lists, device, **mode):
    src = [None if fr is None else [_dev(f) if device else f for f in fr] for fr in lists]
    got = ctx.drizzle_rgb(*src, **DRZ, **mode)
    images = [None if fr is None or len(fr) < 2 else ctx.drizzle_stack(fr, want_weight=False, **DRZ) for fr in src]
    want = ctx.process_drizzle_rgb(*[None if d is None else d.image for d in images], want_stretched=False, **mode)
    p = got.processed
    assert (p.rows, p.cols) == (want.rows, want.cols) == (48, 40)
    assert (p.wb_factors, p.stf, p.chan_stats, p.stats_wb, p.scnr_applied) == (want.wb_factors, want.stf, want.chan_stats, want.stats_wb, want.scnr_applied)
    for c in range(3):
        assert_bits(p.wb[c], _host(want.wb[c]), f"wb {'RGB'[c]}")
        if images[c] is None:
            assert got.channels[c] is None
        else:
            d = images[c]
            assert got.channels[c] == (d.frame_count, d.output_scale, d.input_dims, d.output_dims, d.rejected_pixels)
    assert_bytes(p.rgb8, _host(want.rgb8), "rgb8")
    return got


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_drizzle_rgb_equals_stack_then_process(ctx, device):
    frames = _drizzle_frames()
    got = _check_drizzle_rgb(ctx, frames, device, white_balance="auto", auto_stretch=True, linked_stf=True,
                             scnr=dict(method="average", amount=0.8, preserve_luminance=True))
    assert _host(got.processed.rgb8).std() > 0
    _check_drizzle_rgb(ctx, frames, device, white_balance="none", auto_stretch=True, linked_stf=False, scnr=None)


def test_drizzle_rgb_short_and_missing_lists(ctx):
    import astroburst_amd as ab
    r, g, b = _drizzle_frames()
    got = _check_drizzle_rgb(ctx, [r, g[:1], b], True, white_balance="auto", auto_stretch=True, linked_stf=True, scnr=None)  # one frame: absent
    assert got.channels[1] is None and not _host(got.processed.wb[1]).any()
    _check_drizzle_rgb(ctx, [r, None, b], True, white_balance="auto", auto_stretch=True, linked_stf=False, scnr=None)
    with pytest.raises(ab.AstroBurstError, match=r"Need at least 2 channels for RGB drizzle \(got 1\)"):
        ctx.drizzle_rgb(r, None, None, **DRZ)
    with pytest.raises(ab.AstroBurstError, match="All channels failed or have fewer than 2 frames"):
        ctx.drizzle_rgb(r[:1], g[:1], None, **DRZ)
    # the same two through the C ABI
    keep = []
    pr = ctx._planes(r, keep)
    dcfg = _lib.DrizzleConfigC(2.0, 0.7, 0, 3.0, 3.0, 5, 0, 0, 8)
    cfg = _lib.DrizzleRgbConfigC()
    res, info = (_lib.DrizzleResultC * 3)(), _lib.ProcessedDrizzleRgbInfoC()
    L = _lib.lib()
    assert L.ab_drizzle_rgb(ctx._h, pr, 3, None, 0, None, 0, C.byref(dcfg), C.byref(cfg), None, None, 0, res, C.byref(info)) == _lib.AB_ERR_INVALID
    assert b"Need at least 2 channels for RGB drizzle (got 1)" in L.ab_last_error(ctx._h)
    assert L.ab_drizzle_rgb(ctx._h, pr, 1, pr, 1, pr, 0, C.byref(dcfg), C.byref(cfg), None, None, 0, res, C.byref(info)) == _lib.AB_ERR_INVALID
    assert b"All channels failed or have fewer than 2 frames" in L.ab_last_error(ctx._h)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_with_a_message(ctx):
    L = _lib.lib()
    keep = []
    a = np.zeros((4, 6), F32)
    p, q = ctx._plane(a, keep), ctx._plane(np.zeros((4, 5), F32), keep)
    out = np.zeros(4 * 6 * 6, np.uint8)
    o = C.c_void_p(out.ctypes.data)
    stf, st = (_lib.StfParamsC * 3)(), (_lib.ImageStatsC * 3)()
    ecfg, einfo = _lib.RgbExportConfigC(), _lib.RgbExportInfoC()
    ecfg.bits = 8
    dcfg, dinfo = _lib.DrizzleRgbConfigC(), _lib.ProcessedDrizzleRgbInfoC()
    P = C.byref
    small = (_lib.Plane * 3)(*[_lib.Plane(C.c_void_p(a.ctypes.data), 4, 5, 0)] * 3)

    def refused(rc, what):
        assert rc == _lib.AB_ERR_INVALID, what
        assert L.ab_last_error(ctx._h), what

    refused(L.ab_render_rgb(ctx._h, None, P(p), P(p), 0, o, 0), "null plane")
    refused(L.ab_render_rgb(ctx._h, P(p), P(p), P(p), 0, None, 0), "null output")
    refused(L.ab_render_rgb(ctx._h, P(p), P(q), P(p), 0, o, 0), "wrong dims")
    refused(L.ab_render_rgb(ctx._h, P(p), P(p), P(p), 3, o, 0), "bad pack")
    refused(L.ab_render_rgb(ctx._h, P(p), P(p), P(p), -1, o, 0), "bad pack")
    refused(L.ab_render_rgb_stf(ctx._h, P(p), P(p), P(p), None, st, 0, o, 0), "null stf")
    refused(L.ab_render_rgb_stf(ctx._h, P(p), P(p), P(p), stf, None, 0, o, 0), "null stats")
    refused(L.ab_render_rgb_stf(ctx._h, P(p), P(p), P(p), stf, st, 5, o, 0), "bad pack")
    refused(L.ab_export_rgb(ctx._h, P(p), P(p), None, P(ecfg), o, 0, P(einfo)), "null plane")
    refused(L.ab_export_rgb(ctx._h, P(p), P(p), P(p), None, o, 0, P(einfo)), "null cfg")
    refused(L.ab_export_rgb(ctx._h, P(p), P(p), P(p), P(ecfg), o, 0, None), "null info")
    ecfg.bits = 12
    refused(L.ab_export_rgb(ctx._h, P(p), P(p), P(p), P(ecfg), o, 0, P(einfo)), "bits = 12")
    refused(L.ab_process_drizzle_rgb(ctx._h, None, None, None, P(dcfg), None, None, o, 0, P(dinfo)), "no channel")
    refused(L.ab_process_drizzle_rgb(ctx._h, P(p), P(p), P(p), None, None, None, o, 0, P(dinfo)), "null cfg")
    refused(L.ab_process_drizzle_rgb(ctx._h, P(p), P(p), P(p), P(dcfg), None, None, o, 0, None), "null info")
    refused(L.ab_process_drizzle_rgb(ctx._h, P(p), P(q), P(p), P(dcfg), None, (_lib.Plane * 3)(*[p] * 3), o, 0, P(dinfo)), "out_wb of the wrong dims")
    refused(L.ab_process_drizzle_rgb(ctx._h, P(p), P(p), P(p), P(dcfg), small, None, o, 0, P(dinfo)), "out_stretched of the wrong dims")
    dcfg.white_balance = 3
    refused(L.ab_process_drizzle_rgb(ctx._h, P(p), P(p), P(p), P(dcfg), None, None, o, 0, P(dinfo)), "bad white balance")
    # a device output over a device input plane (5 x 7: a head, whole four-pixel groups and loose pixels)
    import torch
    t = [torch.rand((5, 7), device="cuda") for _ in range(3)]
    before = [x.clone() for x in t]
    d = [_lib.Plane(C.c_void_p(x.data_ptr()), 5, 7, 1) for x in t]
    refused(L.ab_render_rgb(ctx._h, P(d[0]), P(d[1]), P(d[2]), 0, C.c_void_p(t[2].data_ptr()), 1), "a device output over a device input")
    assert b"an output overlaps an input plane" in L.ab_last_error(ctx._h)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(t, before))
    for fn in (L.ab_render_rgb, L.ab_render_rgb_stf, L.ab_export_rgb, L.ab_process_drizzle_rgb, L.ab_drizzle_rgb):   # a NULL context
        nothing = [0 if t in (C.c_int32, C.c_int64, C.c_size_t) else None for t in fn.argtypes]
        assert fn(*nothing) == _lib.AB_ERR_INVALID
    # and the context still works
    assert_bytes(ctx.render_rgb(a, a, a), np.zeros((4, 6, 3), np.uint8), "after the errors")
