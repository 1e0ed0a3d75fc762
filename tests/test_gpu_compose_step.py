"""The RGB Compose panel on the GPU (csrc/compose_step.hip: ab_compose_rgb; tone.hip: ab_restretch_composite), each case against two
references.

Reference 1, the library's own unfused chain -- ab_process_rgb -> ab_resample_image -> ab_compute_image_stats -> ab_auto_stf ->
ab_apply_stf_f32 -> ab_apply_lrgb -> ab_render_rgb_preview -- compared with ==: planes as bit patterns, bytes, offsets, STFs and
statistics; the means alone to 1e-12 relative, the bar of tests/test_gpu_stats_stf.py (the chain's statistics may take the
register-resident kernel, whose sum has another order).

Reference 2, tests/compose_step_restatement.py out of the oracle, at the bars of tests/test_gpu_compose.py: on the phase-correlation
path and without alignment everything is bit-exact (the mean too up to 4 000 000 pixels, where both sides take the exact route; 1e-12
relative above, tests/test_gpu_stats_stf.py's bar for the histogram route); on the affine path the offsets agree to 1e-9 and the
planes differ at fewer than 2e-3 of the pixels by less than 2e-3 -- that case carries no L, so that apply_lrgb's ratio does not
amplify the bar.

Shapes: 5 x 7 and 37 x 53 with every plane one float off 16-byte alignment and the bytes at offsets 0-3 (head, tail, groups, unaligned
dwords); 301 x 517 at max_dim 128 and 64 with and without out_planes (the pick; one and two launches); 128 x 160 star fields under
both registrations, with G at 96 x 120 and with R absent; 2001 x 2003 at max_dim 1024 with L at 1000 x 1001 (4 008 003 pixels: the
histogram statistics route).  The special values -- NaN, +-inf, a negative, 0, 1e-7 and its two f32 neighbours -- sit in every
channel and in L, at different pixels per plane.

Every non-error case was run through the oracle on the CPU first (build() and expectations() below need no GPU), and each asserts
from the restatement, before anything is compared, that its branches are taken: some but not all pixels have lum_old < 1e-10; where
SCNR is configured it changes a pixel; where L is given with both weights above zero the clamp of lrgb.rs:39-41 receives a value
above 1.  With a lightness weight of 0 the ratio is lum_old / lum_old = 1 and the clamp receives the stretched channel itself, which
never exceeds 1; with a chrominance weight of 0 it receives L, which exceeds 1 only when L goes in unstretched (auto_stretch off, L's
values reach 2).  Those two weight pairs are asserted to clamp exactly then."""
import ctypes as C

import numpy as np
import pytest

import compose_step_restatement as R
from astroburst_amd import AstroBurstError, ImageStats, StfParams, _lib
from test_gpu_compose import star_field

pytestmark = pytest.mark.gpu
F32 = np.float32
TINY = F32(1e-7)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.5, 0.0, TINY, np.nextafter(TINY, F32(0)), np.nextafter(TINY, F32(1))], F32)
EXACT_LIMIT = 4_000_000     # stats.rs:18

AVG = dict(method="average", amount=0.8)
MAXP = dict(method="maximum", amount=1.0, preserve_luminance=True)
GIVEN = (StfParams(0.02, 0.3, 0.9), None, StfParams(0.1, 0.2, 0.8))
NEAR_ONE = 1.00000001       # f32: 1.0 -- the skip rule of rgb.rs:127-130 and the reuse of the statistics already taken

# name: shape, source ("noise" | "stars"), channel dims override, L (None | "same" | (rows, cols)), weights, max_dim, process_rgb keywords
CFG = {
    "auto":        dict(kw=dict(align=False)),
    "none-linked": dict(l="same", w=(1.0, 1.0), kw=dict(align=False, white_balance="none", linked_stf=True, scnr=AVG)),
    "manual-given": dict(l="other", w=(0.35, 0.6), kw=dict(align=False, white_balance=(1.3, NEAR_ONE, 0.7), auto_stretch=False, stf=GIVEN, scnr=MAXP)),
    "merge-only":  dict(l="same", w=(0.0, 1.0), kw=dict(align=False, white_balance=(NEAR_ONE, 1.0, NEAR_ONE), linked_stf=True)),
    "no-launch":   dict(l="other", w=(1.0, 0.0), kw=dict(align=False, white_balance=(NEAR_ONE, NEAR_ONE, 1.0), scnr=AVG)),
    "absent-stf":  dict(l="same", w=(1.0, 1.0), kw=dict(align=False, auto_stretch=False, scnr=MAXP)),
    "auto-lother": dict(l="other", w=(0.35, 0.6), kw=dict(align=False, white_balance="none")),
    "raw-l-10":    dict(l="same", w=(1.0, 0.0), kw=dict(align=False, auto_stretch=False, stf=GIVEN)),
    "raw-l-01":    dict(l="other", w=(0.0, 1.0), kw=dict(align=False, auto_stretch=False, white_balance="none")),
    "given-no-l":  dict(kw=dict(align=False, auto_stretch=False, stf=GIVEN, scnr=AVG)),
}
# L absent / same dims / other dims, each with auto_stretch on and off: "auto" / "none-linked" / "auto-lother" and "given-no-l" /
# "absent-stf" / "manual-given".
# ("merge-only": nothing is scaled and the STF is linked, so the white-balance launch only merges; "no-launch": nothing scaled, unlinked)


def case(shape, cfg, max_dim=4096, source="noise", dims=None, absent=None, **over):
    d = dict(shape=shape, source=source, dims=dims or {}, absent=absent, l=None, w=(1.0, 1.0), max_dim=max_dim)
    d.update(CFG[cfg])
    d["kw"] = dict(d["kw"])
    d["kw"].update(over)
    return d


CASES = {}
for _cfg in CFG:
    CASES[f"37x53-{_cfg}"] = case((37, 53), _cfg)
for _cfg in ("auto", "none-linked", "manual-given", "raw-l-01", "given-no-l"):
    CASES[f"5x7-{_cfg}"] = case((5, 7), _cfg)
for _cfg in ("none-linked", "manual-given"):
    for _md in (128, 64):
        CASES[f"301x517-{_cfg}-{_md}"] = case((301, 517), _cfg, _md)
CASES["301x517-given-no-l-64"] = case((301, 517), "given-no-l", 64)
CASES["stars-phase"] = case((128, 160), "none-linked", source="stars", align=True, white_balance="auto")
CASES["stars-affine"] = case((128, 160), "auto", source="stars", align=True, align_method="affine", num_threads=4, scnr=AVG)
CASES["stars-g-resampled"] = case((128, 160), "auto-lother", source="stars", dims={1: (96, 120)}, align=True, white_balance="auto", scnr=MAXP)
CASES["stars-r-absent"] = case((128, 160), "none-linked", source="stars", absent=0, align=True, white_balance="auto", linked_stf=False)
CASES["2001x2003"] = case((2001, 2003), "none-linked", 1024)
CASES["2001x2003"]["l"] = (1000, 1001)

_built, _expected, _chain = {}, {}, {}


def sprinkle(plane, i):
    """plane i of r, g, b, l: the special values at its first pixels (rotated by 2 i + 1, so that they meet different values in the other
    planes), a run of zeros that every plane shares (lum_old == 0), then two pixels of pure green (SCNR has something to take whatever
    the stretch does to the channels) and two of pure red under the brightest L (lum_old far below r: apply_lrgb's ratio passes 1),
    these again in the last row"""
    flat = plane.reshape(-1)
    k = len(SPECIALS)
    flat[:k] = np.roll(SPECIALS, 2 * i + 1)
    flat[k:k + 5] = 0.0
    flat[k + 5:k + 7] = [0.051, 0.9, 0.051, 0.5][i]
    flat[k + 7:k + 9] = [0.95, 0.051, 0.051, 2.0][i]
    if i == 3:
        plane[-2:, :] = 2.0          # (an L of other dims is resampled: its last rows stay the brightest under the channels' last row)
    else:
        flat[-4:-2] = [0.95, 0.051, 0.051][i]
    return plane


def build(name):
    """(l, r, g, b) on the host, read-only; absent planes are None"""
    if name in _built:
        return _built[name]
    c = CASES[name]
    rows, cols = c["shape"]
    out = []
    for i in range(4):      # r, g, b, l
        shape = c["dims"].get(i, (rows, cols))
        if i == 3:
            if c["l"] is None:
                out.append(None)
                continue
            if c["l"] == "same":
                shape = (rows, cols)
            elif isinstance(c["l"], tuple):
                shape = c["l"]
            else:   # "other": smaller, but larger for 5 x 7 -- a 3 x 4 L would be special values only and resample to NaN everywhere
                shape = (rows * 3 // 4, cols * 2 // 3) if rows >= 16 else (2 * rows + 1, 2 * cols - 1)
        if c["source"] == "stars":
            shift = [(0.0, 0.0), (1.5, -2.25), (-0.75, 1.0), (0.5, 0.5)][i]
            p = star_field(1, shape[0], shape[1], 40, shift=tuple(s * shape[0] / rows for s in shift), scale=[1.0, 0.8, 1.3, 1.6][i], noise_seed=2 + i)
            if i == 1:
                p[40:60, 50:80] *= F32(1.6)          # a green cast for SCNR
            if i == 3:
                p[30:50, 20:60] += F32(0.4)          # L far above the channels: the ratio pushes them past 1
            p[20:28, 20:28] = 0.0                    # lum_old == 0 inside, whatever the registration interpolates at the rim
            p[5, 5] = np.nan
        else:
            rng = np.random.default_rng(rows * 1000 + cols * 10 + i)
            y, x = np.mgrid[0:shape[0], 0:shape[1]]
            p = (0.05 + 0.6 * rng.uniform(0, 1, shape) * (0.3 + 0.7 * x / shape[1]) + 0.1 * y / shape[0]).astype(F32)
            if i == 1:
                p[:, shape[1] // 2:] *= F32(2.5)     # a green cast for SCNR
            if i == 3:
                p = (p * F32(2.5)).astype(F32)       # L reaches 2: past the clamp when it goes in unstretched
            sprinkle(p, i)
        out.append(np.ascontiguousarray(p, F32))
    planes = [out[3], out[0], out[1], out[2]]
    if c["absent"] is not None:
        planes[1 + c["absent"]] = None
    for p in planes:
        if p is not None:
            p.setflags(write=False)
    _built[name] = tuple(planes)
    return _built[name]


def expectations(oracle, name):
    """reference 2 at full size (max_dim = the larger dim; the pick is applied per test), after asserting that the case takes the
    branches it is there for.  Needs no GPU."""
    if name in _expected:
        return _expected[name]
    c = CASES[name]
    l, r, g, b = build(name)
    lw, cw = c["w"]
    want = R.compose_rgb(oracle, l, r, g, b, lw, cw, max_dim=max(c["shape"]), **c["kw"])
    n = want.rgb.rows * want.rgb.cols
    with np.errstate(all="ignore"):
        lum_old = want.rgb.r * F32(0.2126) + want.rgb.g * F32(0.7152) + want.rgb.b * F32(0.0722)
    dark = int(np.count_nonzero(lum_old < F32(1e-10)))
    assert 0 < dark < n, (name, dark, n)
    if c["kw"].get("scnr"):
        plain = oracle.process_rgb(r, g, b, **{k: v for k, v in c["kw"].items() if k != "scnr"})
        assert not np.array_equal(plain.g, want.rgb.g, equal_nan=True), name
    if l is not None:
        clamped = R.branches(want, lw, cw)[2]
        raw_l = not c["kw"].get("auto_stretch", True)
        assert clamped == (lw > 0 and (cw > 0 or raw_l)), name
    _expected[name] = want
    return want


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def dev_plane(a, off=0):
    """a device plane that starts `off` floats into its allocation (torch allocations are at least 256-byte aligned)"""
    import torch
    if a is None:
        return None
    buf = torch.empty(a.size + off, dtype=torch.float32, device="cuda")
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    return v


def dev_empty(shape, off=0):
    import torch
    n = int(np.prod(shape))
    return torch.full((n + off,), -7.0, dtype=torch.float32, device="cuda")[off:off + n].view(shape)


def dev_bytes(n, off=0):
    import torch
    return torch.full((n + off + 8,), 0xAB, dtype=torch.uint8, device="cuda")[off:off + n]


def pick(rgb8, max_dim):
    rows, cols = rgb8.shape[:2]
    dst_h, dst_w = pick_dims(rows, cols, max_dim)
    if (dst_h, dst_w) == (rows, cols):
        return rgb8
    ys = [int(min(d * (rows / dst_h), rows - 1.0)) for d in range(dst_h)]      # helpers.rs:297-309
    xs = [int(min(d * (cols / dst_w), cols - 1.0)) for d in range(dst_w)]
    return rgb8[np.ix_(ys, xs)]


def pick_dims(rows, cols, max_dim):
    from background_step_restatement import pick_dims as wh
    w, h = wh(cols, rows, max_dim)
    return h, w


def chain(ctx, name):
    """reference 1 at full size, on the device: dict(pre, planes, rgb8 of every pixel, info of process_rgb, l_stats, l_stf)"""
    if name in _chain:
        return _chain[name]
    c = CASES[name]
    l, r, g, b = (dev_plane(x) for x in build(name))
    p = ctx.process_rgb(r, g, b, **c["kw"])
    planes = [p.r, p.g, p.b]
    l_stats = l_stf = None
    if l is not None:
        lm = ctx.resample_image(l, p.rows, p.cols) if tuple(l.shape) != (p.rows, p.cols) else l
        if c["kw"].get("auto_stretch", True):
            l_stats = ctx.compute_image_stats(lm)
            l_stf = ctx.auto_stf(l_stats)
            lm = ctx.apply_stf_f32(lm, l_stf, l_stats)
        ctx.apply_lrgb(lm, *planes, *c["w"])
    rgb8 = ctx.render_rgb_preview(*planes, max(c["shape"]))
    _chain[name] = dict(pre=[host(x) for x in p.pre_stretch], planes=[host(x) for x in planes], rgb8=host(rgb8), p=p, l_stats=l_stats, l_stf=l_stf)
    return _chain[name]


def same_stats(got, want, exact_mean):
    assert got.valid_count == want.valid_count
    assert got.min == want.min and got.max == want.max
    assert got.median == want.median, (got.median, want.median)
    assert got.mad == want.mad and got.sigma == want.sigma
    if exact_mean:
        assert got.mean == want.mean
    else:
        assert abs(got.mean - want.mean) <= 1e-12 * abs(want.mean)


def same_chan_stats(got, want, exact_mean):
    for a, b in zip(got, want):
        assert a[:3] == b[:3]
        assert a[3] == b[3] if exact_mean else abs(a[3] - b[3]) <= 1e-12 * abs(b[3])


def same_stf(got, want):
    assert (got.shadow, got.midtone, got.highlight) == (want.shadow, want.midtone, want.highlight)


def check(ctx, oracle, got, name, planes, affine=False):
    c = CASES[name]
    want = expectations(oracle, name)           # (asserts the case's branches first)
    ref = chain(ctx, name)
    rows, cols = want.rgb.rows, want.rgb.cols
    dst_h, dst_w = pick_dims(rows, cols, c["max_dim"])
    assert (got.rows, got.cols, got.preview_rows, got.preview_cols) == (rows, cols, dst_h, dst_w)
    assert got.lrgb_applied == (c["l"] is not None) and got.l_resampled == want.l_resampled
    # reference 1: ==
    p = ref["p"]
    assert got.offset_g == p.offset_g and got.offset_b == p.offset_b
    assert got.scnr_applied == p.scnr_applied and got.resampled == p.resampled
    for ch in range(3):
        assert np.array_equal(bits(host(got.pre_stretch[ch])), bits(ref["pre"][ch])), ch
        if planes:
            assert np.array_equal(bits(host(got.planes[ch])), bits(ref["planes"][ch])), ch
        same_stf(got.stf[ch], p.stf[ch])
        same_stats(got.stats_wb[ch], p.stats_wb[ch], False)
    same_chan_stats(got.channel_stats, p.channel_stats, False)
    if not planes:
        assert got.planes is None
    assert host(got.rgb8).shape == (dst_h, dst_w, 3) and np.array_equal(host(got.rgb8), pick(ref["rgb8"], c["max_dim"]))
    if ref["l_stats"] is not None:
        same_stats(got.l_stats, ref["l_stats"], False)
        same_stf(got.l_stf, ref["l_stf"])
    else:
        assert got.l_stats is None and got.l_stf is None
    # reference 2
    exact_mean = rows * cols <= EXACT_LIMIT
    assert got.scnr_applied == want.rgb.scnr_applied and got.resampled == want.rgb.resampled
    if affine:
        assert np.allclose(got.offset_g, want.rgb.offset_g, atol=1e-9) and np.allclose(got.offset_b, want.rgb.offset_b, atol=1e-9)
        for ch in range(3):
            for a, b in ((host(got.pre_stretch[ch]), want.rgb.pre_stretch[ch]), (host(got.planes[ch]), want.planes[ch])):
                with np.errstate(invalid="ignore"):
                    d = np.abs(a - b)
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.mean(bits(a) != bits(b)) < 2e-3 and np.nanmax(d) < 2e-3
        return
    assert got.offset_g == want.rgb.offset_g and got.offset_b == want.rgb.offset_b
    for ch in range(3):
        assert np.array_equal(host(got.pre_stretch[ch]), want.rgb.pre_stretch[ch], equal_nan=True)
        if planes:
            assert np.array_equal(host(got.planes[ch]), want.planes[ch], equal_nan=True)
        same_stf(got.stf[ch], want.rgb.stf[ch])
        same_stats(got.stats_wb[ch], want.rgb.stats_wb[ch], exact_mean)
    same_chan_stats(got.channel_stats, want.rgb.channel_stats, exact_mean)
    assert np.array_equal(host(got.rgb8), pick(want.rgb8, c["max_dim"]))
    if want.l_stats is not None:
        same_stats(got.l_stats, want.l_stats, exact_mean)
        same_stf(got.l_stf, want.l_stf)


def run(ctx, name, planes, off=0, byte_off=0, fetch=True, on_host=False):
    c = CASES[name]
    rows, cols = c["shape"]
    ins = build(name) if on_host else [dev_plane(x, off) for x in build(name)]
    dst_h, dst_w = pick_dims(rows, cols, c["max_dim"])
    kw = {}
    if not on_host:
        kw = dict(out_pre=tuple(dev_empty((rows, cols), off) for _ in range(3)), out=dev_bytes(dst_h * dst_w * 3, byte_off))
        if planes:
            kw["out_planes"] = tuple(dev_empty((rows, cols), off) for _ in range(3))
    got = ctx.compose_rgb(*ins, lrgb_lightness=c["w"][0], lrgb_chrominance=c["w"][1], max_dim=c["max_dim"], want_planes=planes, fetch=fetch, **kw, **c["kw"])
    got.rgb8 = host(got.rgb8).reshape(dst_h, dst_w, 3)
    return got


SMALL = [n for n in CASES if n.startswith(("37x53", "5x7"))]


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes_one_float_off_alignment(ctx, oracle, name):
    """every configuration at 37 x 53 and five at 5 x 7 (fewer pixels than one workgroup has lanes: head, one or no group, tail), each
    plane one float into its allocation, the bytes at offsets 0-3 in turn"""
    for byte_off in range(4):
        check(ctx, oracle, run(ctx, name, planes=True, off=1, byte_off=byte_off), name, planes=True)


@pytest.mark.parametrize("name", ["37x53-none-linked", "5x7-manual-given"])
def test_aligned_planes_take_the_wide_accesses(ctx, oracle, name):
    check(ctx, oracle, run(ctx, name, planes=True, off=0, byte_off=0), name, planes=True)
    check(ctx, oracle, run(ctx, name, planes=False, off=0, byte_off=1), name, planes=False)


@pytest.mark.parametrize("planes", [False, True], ids=["pick-only", "planes-then-pick"])
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("301x517")])
def test_the_pick(ctx, oracle, name, planes):
    """301 x 517 above max_dim: without out_planes only the picked pixels are finished (one launch), with them two launches"""
    check(ctx, oracle, run(ctx, name, planes=planes, off=1, byte_off=3), name, planes=planes)


@pytest.mark.parametrize("name", ["stars-phase", "stars-g-resampled", "stars-r-absent"])
def test_star_fields_phase_correlation(ctx, oracle, name):
    check(ctx, oracle, run(ctx, name, planes=True), name, planes=True)


def test_star_fields_affine(ctx, oracle):
    want = expectations(oracle, "stars-affine")
    assert abs(abs(want.rgb.offset_g[0]) - 1.5) < 0.3 and abs(abs(want.rgb.offset_g[1]) - 2.25) < 0.3   # a real star match
    check(ctx, oracle, run(ctx, "stars-affine", planes=True), "stars-affine", planes=True, affine=True)


def test_histogram_statistics_route(ctx, oracle):
    """2001 x 2003 = 4 008 003 pixels: every statistics chain takes the histogram route; linked STF, L at 1000 x 1001, max_dim 1024"""
    check(ctx, oracle, run(ctx, "2001x2003", planes=False, off=1, byte_off=2), "2001x2003", planes=False)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------
def test_device_outputs_without_info(ctx, oracle):
    """fetch=False: info NULL, device inputs and outputs -- nothing is fetched, the outputs are the same"""
    for name in ("37x53-none-linked", "37x53-auto", "301x517-manual-given-64"):
        got = run(ctx, name, planes=False, fetch=False)
        assert got.stf is None and got.stats_wb is None and got.l_stats is None
        ref, c = chain(ctx, name), CASES[name]
        expectations(oracle, name)
        for ch in range(3):
            assert np.array_equal(bits(host(got.pre_stretch[ch])), bits(ref["pre"][ch]))
        assert np.array_equal(got.rgb8, pick(ref["rgb8"], c["max_dim"]))


@pytest.mark.parametrize("name", ["37x53-manual-given", "5x7-none-linked", "301x517-none-linked-128"])
def test_host_inputs(ctx, oracle, name):
    got = run(ctx, name, planes=True, on_host=True)
    assert all(isinstance(x, np.ndarray) for x in got.pre_stretch + got.planes) and isinstance(got.rgb8, np.ndarray)
    check(ctx, oracle, got, name, planes=True)


def test_want_nothing_but_the_pre_stretch_planes(ctx, oracle):
    name = "37x53-none-linked"
    c = CASES[name]
    got = ctx.compose_rgb(*[dev_plane(x) for x in build(name)], lrgb_lightness=1.0, lrgb_chrominance=1.0, want_rgb8=False, **c["kw"])
    assert got.rgb8 is None and got.planes is None
    ref = chain(ctx, name)
    for ch in range(3):
        assert np.array_equal(bits(host(got.pre_stretch[ch])), bits(ref["pre"][ch]))
        same_stats(got.stats_wb[ch], ref["p"].stats_wb[ch], False)


def untouched(*arrays):
    for a in arrays:
        a = host(a)
        assert np.all(a == (F32(-7.0) if a.dtype == np.float32 else 0xAB))


def test_refusals_leave_the_outputs_untouched(ctx):
    import torch
    l, r, g, b = (dev_plane(x) for x in build("37x53-none-linked"))
    rows, cols = 37, 53
    kw = dict(align=False)

    def outs():
        return tuple(dev_empty((rows, cols)) for _ in range(3)), tuple(dev_empty((rows, cols)) for _ in range(3)), dev_bytes(rows * cols * 3)

    pre, planes, by = outs()
    with pytest.raises(AstroBurstError, match=r"Need at least 2 channels for RGB compose \(got 1\)"):
        ctx.compose_rgb(l, r, None, None, out_pre=pre, out_planes=planes, out=by, **kw)
    with pytest.raises(AstroBurstError, match=r"Need at least 2 channels for RGB compose \(got 0\)"):
        ctx.compose_rgb(l, None, None, None, out_pre=pre, out_planes=planes, want_rgb8=False, **kw)   # (no channel, no preview dims)
    with pytest.raises(AstroBurstError, match=r"Channel dimension ratio 13\.2x exceeds 8x limit\. R=53x37 G=4x4\. Check channel assignments\."):
        ctx.compose_rgb(None, r, dev_plane(np.ones((4, 4), F32)), None, out_pre=pre, out_planes=planes, out=by, **kw)
    with pytest.raises(AstroBurstError, match="max_dim must be >= 1"):
        ctx.compose_rgb(l, r, g, b, max_dim=0, out_pre=pre, out_planes=planes, out=by[:3], **kw)    # (the binding sizes the bytes as 1 x 1)
    untouched(*pre, *planes, by)
    # dimensions
    with pytest.raises(AstroBurstError, match="the output G plane must be 37 x 53"):
        ctx.compose_rgb(l, r, g, b, out_pre=(pre[0], dev_empty((53, 37)), pre[2]), out=by, **kw)
    with pytest.raises(AstroBurstError, match="the output B plane must be 37 x 53"):
        ctx.compose_rgb(l, r, g, b, out_pre=pre, out_planes=(planes[0], planes[1], dev_empty((36, 53))), out=by, **kw)
    huge = _lib.Plane(C.c_void_p(r.data_ptr()), 65536, 32768, 1)
    info = _lib.ComposeRgbInfoC()
    cfg = ctx._rgb_compose_config("none", True, (None, None, None), False, False, "phase_correlation", None, 8)
    keep = []
    ppre = (_lib.Plane * 3)(*[ctx._out_plane(x, keep, rows, cols) for x in pre])
    pr, pg = ctx._plane(r, keep), ctx._plane(g, keep)
    f = ctx._L.ab_compose_rgb
    assert f(ctx._h, None, C.byref(huge), C.byref(huge), None, C.byref(cfg), 1.0, 1.0, 4096, ppre, None, None, 1, C.byref(info)) == _lib.AB_ERR_INVALID
    assert "2^31" in ctx._L.ab_last_error(ctx._h).decode()
    assert f(ctx._h, None, C.byref(pr), C.byref(pg), None, None, 1.0, 1.0, 4096, ppre, None, None, 1, C.byref(info)) == _lib.AB_ERR_INVALID
    assert "null configuration" in ctx._L.ab_last_error(ctx._h).decode()
    assert f(ctx._h, None, C.byref(pr), C.byref(pg), None, C.byref(cfg), 1.0, 1.0, 4096, None, None, None, 1, C.byref(info)) == _lib.AB_ERR_INVALID
    assert "null pre-stretch output planes" in ctx._L.ab_last_error(ctx._h).decode()
    untouched(*pre, *planes, by)
    # overlaps: an output over an input, over another output, the bytes over L; on the host too (the span_of form)
    with pytest.raises(AstroBurstError, match="an output overlaps an input plane"):
        ctx.compose_rgb(l, r, g, b, out_pre=(g, pre[1], pre[2]), out=by, **kw)
    with pytest.raises(AstroBurstError, match="an output overlaps an input plane"):
        ctx.compose_rgb(l, r, g, b, out_pre=pre, out_planes=(planes[0], l, planes[2]), out=by, **kw)
    with pytest.raises(AstroBurstError, match="two outputs overlap"):
        ctx.compose_rgb(l, r, g, b, out_pre=pre, out_planes=(planes[0], pre[1], planes[2]), out=by, **kw)
    with pytest.raises(AstroBurstError, match="two outputs overlap"):
        ctx.compose_rgb(l, r, g, b, out_pre=(pre[0], pre[0], pre[2]), out=by, **kw)
    with pytest.raises(AstroBurstError, match="an output overlaps an input plane"):
        ctx.compose_rgb(l, r, g, b, out_pre=pre, out=l.view(-1).view(torch.uint8)[: rows * cols * 3], **kw)
    untouched(*pre, *planes, by)
    hl, hr, hg, hb = (np.array(x) for x in build("37x53-none-linked"))
    before = hg.copy()
    hpre = tuple(np.full((rows, cols), -7.0, F32) for _ in range(3))
    with pytest.raises(AstroBurstError, match="an output overlaps an input plane"):
        ctx.compose_rgb(hl, hr, hg, hb, out_pre=(hpre[0], hg, hpre[2]), **kw)
    assert np.array_equal(bits(hg), bits(before))
    untouched(hpre[0], hpre[2])


# ---- restretch_composite_cmd ---------------------------------------------------------------------------------------------------------------
def restretch_inputs():
    rng = np.random.default_rng(77)
    rows, cols = 61, 83
    r, g, b = (rng.uniform(0.0, 0.8, (rows, cols)).astype(F32) for _ in range(3))
    g = (g * F32(1.4)).astype(F32)
    for i, p in enumerate((r, g, b)):
        sprinkle(p, i)
    return r, g, b


RESTRETCH_STF = [StfParams(0.02, 0.3, 0.9), StfParams(0.0, 0.5, 1.0), StfParams(0.1, 0.2, 0.8)]


def stats_of(ctx, planes):
    return [ctx.compute_image_stats(p) for p in planes]


@pytest.mark.parametrize("max_dim", [4096, 32], ids=["full", "sampled"])
def test_restretch_is_the_tone_editor_for_an_amount_above_its_threshold(ctx, max_dim):
    planes = [dev_plane(p, 1) for p in restretch_inputs()]
    st = stats_of(ctx, planes)
    scnr = dict(method="average", amount=0.5, preserve_luminance=True)
    for want_planes in (False, True):
        tone = ctx.apply_tone_composite(*planes, st, stf=RESTRETCH_STF, scnr=scnr, max_dim=max_dim, want_planes=want_planes)
        got_planes, got = ctx.restretch_composite(*planes, st, RESTRETCH_STF, scnr=scnr, max_dim=max_dim, want_planes=want_planes)
        assert tone.info.scnr_applied and np.array_equal(host(got), host(tone.rgb8))
        if want_planes:
            assert all(np.array_equal(bits(host(a)), bits(host(b))) for a, b in zip(got_planes, tone.planes))


@pytest.mark.parametrize("max_dim", [4096, 32], ids=["full", "sampled"])
@pytest.mark.parametrize("amount", [0.0, 1e-8, -0.25, float("nan"), 0.5, None], ids=["0", "1e-8", "-0.25", "nan", "0.5", "no-config"])
def test_restretch_is_the_unfused_chain(ctx, oracle, amount, max_dim):
    """ab_apply_stf_f32 x 3 + ab_apply_scnr_inplace + ab_render_rgb_preview: apply_scnr_inplace's own threshold decides, so 0, 1e-8 and
    -0.25 change nothing and a NaN amount goes through (every green pixel becomes NaN, byte 0) -- where the tone editor skips SCNR"""
    host_planes = restretch_inputs()
    planes = [dev_plane(p, 1) for p in host_planes]
    st = stats_of(ctx, planes)
    scnr = None if amount is None else dict(method="maximum", amount=amount, preserve_luminance=True)
    ref = [ctx.apply_stf_f32(p, s, t) for p, s, t in zip(planes, RESTRETCH_STF, st)]
    if scnr is not None:
        ctx.apply_scnr_inplace(*ref, **scnr)
    want = ctx.render_rgb_preview(*ref, max_dim)
    got_planes, got = ctx.restretch_composite(*planes, st, RESTRETCH_STF, scnr=scnr, max_dim=max_dim, want_planes=True)
    assert np.array_equal(host(got), host(want))
    assert all(np.array_equal(bits(host(a)), bits(host(b))) for a, b in zip(got_planes, ref))
    _, only = ctx.restretch_composite(*planes, st, RESTRETCH_STF, scnr=scnr, max_dim=max_dim)
    assert np.array_equal(host(only), host(want))
    if amount is not None and amount != amount:
        assert np.all(np.isnan(host(got_planes[1]))) and not host(got)[..., 1].any()
        tone = ctx.apply_tone_composite(*planes, st, stf=RESTRETCH_STF, scnr=scnr, max_dim=max_dim)
        assert not tone.info.scnr_applied and not np.array_equal(host(tone.rgb8), host(got))
        return
    # the restatement (statistics out of the oracle: the bytes depend on them)
    ost = [oracle.compute_image_stats(p) for p in host_planes]
    for a, b in zip(st, ost):
        same_stats(a, b, True)
    ostf = [oracle.StfParams(p.shadow, p.midtone, p.highlight) for p in RESTRETCH_STF]
    rp, rby = R.restretch(oracle, *host_planes, ost, ostf, scnr=scnr, max_dim=max_dim)
    assert np.array_equal(host(got), rby) and all(np.array_equal(host(a), b, equal_nan=True) for a, b in zip(got_planes, rp))


def test_restretch_refusals(ctx):
    planes = [dev_plane(p) for p in restretch_inputs()]
    st = [ImageStats(0.0, 1.0, 0.5, 0.1, 0.1, 0.5, 10)] * 3
    with pytest.raises(AstroBurstError, match="max_dim must be >= 1"):
        ctx.restretch_composite(*planes, st, RESTRETCH_STF, max_dim=0)
    with pytest.raises(AstroBurstError, match="the G plane is"):
        ctx.restretch_composite(planes[0], dev_plane(np.ones((4, 4), F32)), planes[2], st, RESTRETCH_STF)
    with pytest.raises(AstroBurstError, match="nothing to do"):
        ctx.restretch_composite(*planes, st, RESTRETCH_STF, want_rgb8=False)
