"""compute_image_stats' three rank-finding mechanisms (csrc/stats.hip: the exact path's radix select and the chain's block_find_rank;
csrc/stats_resident.hpp: the two-level descent) and the STF stretch behind them (csrc/stf.hip) on the adversarial planes of
tests/stats_adversarial.py: ranks on the first / last element of a bin, on 64-bin group edges and 256-bin coarse edges, middle
ranks of values AND of deviations split between two bins at every level of the select, refine histograms that do not hold the rank
(resolve_rank_in_hist's fall-through), known ranges that miss the data, both sides of the 4 000 000 px limit, planes and outputs
that do not start on a 16-byte boundary.

Bar: BIT FOR BIT against the numpy statement on min, max, median, mad, sigma and valid_count; the mean within 1e-12 relative (the
reference's f64 summation order is unspecified); every histogram bin; every stretched byte against the CPU oracle.
tests/test_stats_adversarial_cpu.py holds the fixtures to what they claim and the statement to the oracle."""
import numpy as np
import pytest

import select_adversarial as SA
import stats_adversarial as A
import stats_protocol as SP
from test_gpu_stats_stf import hist_engine  # noqa: F401  (the fixture: AB_STATS_CHAIN = 0 / 1, read by the library per call)

pytestmark = pytest.mark.gpu

F32 = np.float32
_expected = {}     # fixture name -> dict: computed once, shared between the tests and the engines, never modified


def bits64(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def check(got, st: dict, what):
    """got: ImageStats of the library; st: the statement's dict"""
    assert got.valid_count == st["valid_count"], (what, got, st)
    for k in ("min", "max", "median", "mad", "sigma"):
        assert bits64(getattr(got, k)) == bits64(st[k]), (what, k, getattr(got, k), st[k])
    assert abs(got.mean - st["mean"]) <= 1e-12 * abs(st["mean"]), (what, got.mean, st["mean"])


def same_stats(a, b, what):
    """two results of the library, bit for bit (the mean included)"""
    assert a.valid_count == b.valid_count, (what, a, b)
    for k in ("min", "max", "median", "mad", "sigma", "mean"):
        assert bits64(getattr(a, k)) == bits64(getattr(b, k)), (what, k, a, b)


def expected(fx, oracle=None):
    """the statement of the fixture; with `oracle` also the pass-2 histogram and, where the range is the scanned one, what the
    preview must deliver: oracle.apply_stf(img, oracle.auto_stf(st), st) on the oracle's own statistics (equal to the statement's)"""
    e = _expected.setdefault(fx.name, {})
    if "st" not in e:
        e["st"], e["trace"] = A.statement(fx.plane(), fx.known)
    if oracle is not None and fx.path == "hist" and "hist" not in e:
        st = e["st"]
        rng = max(st["max"] - st["min"], 1e-30)
        with np.errstate(invalid="ignore"):
            e["hist"] = SP.value_pass(fx.plane().ravel(), st["min"], SP.HIST_BINS / rng)
    if oracle is not None and "u8" not in e and not (e["trace"] or {}).get("known", False):
        ost = oracle.compute_image_stats(fx.plane())
        assert all(bits64(getattr(ost, k)) == bits64(e["st"][k]) for k in ("min", "max", "median", "mad", "sigma")), (fx.name, ost, e["st"])
        e["ost"], e["stf"] = ost, oracle.auto_stf(ost)
        e["u8"] = oracle.apply_stf(fx.plane(), e["stf"], ost)
    return e


def to_device(plane):
    import torch
    return torch.tensor(plane, device="cuda")      # (a copy: the cached planes are read-only)


def family(name, prefix):
    return [f for f in A.FIXTURES if f.family == name and f.name.startswith(prefix)]


# ---- exact path ------------------------------------------------------------------------------------------------------------------
EXACT_GROUPS = ([("exact/select", f"select/{p}-") for p in ("L0", "BINADE", "L1", "L2", "TOP", "FLOOR", "four", "tie", "q16")]
                + [("exact/deviation", f"deviation/{p}-") for p in A.DEV_PAIRS] + [("exact/limit", "limit/4000000"), ("hist/known-range", "known/exact-path")])


@pytest.mark.parametrize("fam,prefix", EXACT_GROUPS, ids=[g[1].rstrip("-") for g in EXACT_GROUPS])
def test_exact_path_bit_for_bit(ctx, fam, prefix):
    fxs = [f for f in family(fam, prefix) if f.path == "exact"]
    assert fxs
    for fx in fxs:
        plane = fx.plane()
        st = expected(fx)["st"]
        dev = to_device(plane)
        for src, what in ((plane, "host"), (dev, "device")):
            if fx.known:      # a known range on a plane of <= 4 000 000 px: the exact path all the same (stats.rs:32-34)
                check(ctx.compute_image_stats_with_known_range(src, *fx.known), st, (fx.name, what, "known"))
            check(ctx.compute_image_stats(src), st, (fx.name, what))


def test_exact_path_state_is_reused_from_call_to_call(ctx):
    """two planes with different medians, an even and an odd count, alternately on one context and once more after a trim: the
    select's histograms, ranks and prefixes live in one state block that every call reuses"""
    fxs = [A.BY_NAME["deviation/L0-600002-even/row"], A.BY_NAME["select/L0-big/square"], A.BY_NAME["select/q16-50000/row"]]
    devs = [to_device(f.plane()) for f in fxs]
    want = [expected(f)["st"] for f in fxs]
    assert len({w["median"] for w in want}) == 3

    def run():
        for it in range(6):
            k = it % 3
            check(ctx.compute_image_stats(devs[k]), want[k], (fxs[k].name, it))

    run()
    ctx.trim()
    run()


# ---- histogram path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", A.HIST, ids=lambda f: f.name)
def test_hist_path_bit_for_bit(ctx, oracle, fx, hist_engine):
    import torch
    plane = fx.plane()
    e = expected(fx, oracle)
    st = e["st"]
    dev = to_device(plane)
    what = (fx.name, hist_engine)
    if fx.known:
        check(ctx.compute_image_stats_with_known_range(dev, *fx.known), st, what + ("known", "device"))
        check(ctx.compute_image_stats_with_known_range(plane, *fx.known), st, what + ("known", "host"))
    else:
        check(ctx.compute_image_stats(dev), st, what + ("device",))
        check(ctx.compute_image_stats(plane), st, what + ("host",))
        # the scanned range handed in as a known one is the same computation (stats.rs:25-41)
        check(ctx.compute_image_stats_with_known_range(dev, st["min"], st["max"]), st, what + ("known = scanned",))
    # pass 2 bin for bin (stats.rs:260-300)
    h, s, c = ctx.stats_value_hist(dev, st["min"], st["max"])
    rh, rs, rc = e["hist"]
    assert c == rc and np.array_equal(h.astype(np.int64), rh) and abs(s - rs) <= 1e-12 * abs(rs), what
    if "u8" not in e:       # (a known range that holds: the preview always scans its own)
        assert fx.known and e["trace"]["known"]
        return
    # auto_stretch_preview: statistics, STF parameters and every byte; the output poisoned first
    out = torch.full(plane.shape, 0x5A, dtype=torch.uint8, device="cuda")
    u8, gst, gp = ctx.auto_stretch_preview(dev, out=out)
    check(gst, st, what + ("preview",))
    p = e["stf"]
    assert (bits64(gp.shadow), bits64(gp.midtone), bits64(gp.highlight)) == (bits64(p.shadow), bits64(p.midtone), bits64(p.highlight)), what
    assert np.array_equal(u8.cpu().numpy(), e["u8"]), what
    out.fill_(0x5A)
    u8b, none_st, none_p = ctx.auto_stretch_preview(dev, out=out, fetch=False)       # (always the chain)
    ctx.synchronize()
    assert none_st is None and none_p is None and np.array_equal(u8b.cpu().numpy(), e["u8"]), what


def test_hist_path_workspace_is_reused_from_call_to_call(ctx, oracle, hist_engine):
    """two fixtures with different medians alternately, six calls on one context, and once more after ctx.trim(): the histograms,
    the resident engine's slab and the state block are reused from call to call (a stale row or count would be the other plane's)"""
    import torch
    fxs = [A.BY_NAME["edge/256-last-3999998"], A.BY_NAME["dev-edge/4096-1000001"]]
    es = [expected(f, oracle) for f in fxs]
    assert es[0]["st"]["median"] != es[1]["st"]["median"]
    devs = [to_device(f.plane()) for f in fxs]
    out = torch.empty(fxs[0].plane().shape, dtype=torch.uint8, device="cuda")

    def run():
        for it in range(6):
            k = it & 1
            check(ctx.compute_image_stats(devs[k]), es[k]["st"], (fxs[k].name, hist_engine, it))
            out.fill_(0x5A)
            u8, gst, _ = ctx.auto_stretch_preview(devs[k], out=out)
            check(gst, es[k]["st"], (fxs[k].name, hist_engine, it, "preview"))
            assert np.array_equal(u8.cpu().numpy(), es[k]["u8"]), (fxs[k].name, hist_engine, it)

    run()
    ctx.trim()
    run()


# ---- planes that do not start on a 16-byte boundary ------------------------------------------------------------------------------
def offset_view(src, k):
    """the plane as a contiguous view that starts k elements into a fresh allocation (torch allocations are 256-byte aligned)"""
    import torch
    base = torch.full((src.numel() + k,), 0x5A if src.dtype == torch.uint8 else -7.0, dtype=src.dtype, device="cuda")
    view = base[k:].view(src.shape)
    view.copy_(src)
    assert base.data_ptr() % 16 == 0 and view.data_ptr() == base.data_ptr() + k * src.element_size() and view.is_contiguous()
    return base, view


UNALIGNED = ("deviation/L0-600002-even/square", "edge/256-last-3999998")   # a fixture of each path


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_device_planes_give_the_aligned_results(ctx, oracle, name, k, hist_engine):
    """torch.empty(n + k)[k:].view(rows, cols) is a contiguous device plane that Context._plane accepts; the statistics take their
    scalar loops (stream_pixels; the resident engine hands the plane to the chain) and the three STF kernels theirs.  Everything
    must be the aligned call's, bit for bit -- the mean too: both fixtures hold multiples of 2^-25 below 4, whose f64 sum is exact
    in any order.  Then the same with the u8 output one byte and the f32 output four bytes into their allocations."""
    import torch
    fx = A.BY_NAME[name]
    plane = fx.plane()
    e = expected(fx, oracle)
    dev = to_device(plane)
    what = (name, k, hist_engine)
    # the aligned calls (held to the statement and the oracle)
    st = ctx.compute_image_stats(dev)
    check(st, e["st"], what)
    u8, pst, p = ctx.auto_stretch_preview(dev)
    same_stats(pst, st, what)
    want_u8 = u8.cpu().numpy()
    assert np.array_equal(want_u8, e["u8"]), what
    assert np.array_equal(ctx.apply_stf(dev, p, st).cpu().numpy(), want_u8), what
    want_f32 = ctx.apply_stf_f32(dev, p, st).cpu().numpy()
    assert np.array_equal(SA.bits_of(want_f32), SA.bits_of(oracle.apply_stf_f32(plane, e["stf"], e["ost"]))), what

    base, view = offset_view(dev, k)
    same_stats(ctx.compute_image_stats(view), st, what)
    for src, src_what in ((view, "unaligned in"), (dev, "aligned in")):
        for ko in ((0, 1) if src is view else (1,)):       # the outputs aligned, then 1 byte / 4 bytes into their allocations
            w = what + (src_what, ko)
            ob, ov = offset_view(torch.zeros(plane.shape, dtype=torch.uint8, device="cuda"), ko)
            g8, gst, gp = ctx.auto_stretch_preview(src, out=ov)
            same_stats(gst, st, w)
            assert (gp.shadow, gp.midtone, gp.highlight) == (p.shadow, p.midtone, p.highlight), w
            assert g8.data_ptr() == ov.data_ptr() and np.array_equal(ov.cpu().numpy(), want_u8), w
            ov.fill_(0x5A)
            ctx.auto_stretch_preview(src, out=ov, fetch=False)
            ctx.synchronize()
            assert np.array_equal(ov.cpu().numpy(), want_u8), w
            ov.fill_(0x5A)
            ctx.apply_stf(src, p, st, out=ov)
            assert np.array_equal(ov.cpu().numpy(), want_u8), w
            assert bool((ob[:ko] == 0x5A).all()), w           # nothing written in front of the plane
            fb, fv = offset_view(torch.zeros(plane.shape, dtype=torch.float32, device="cuda"), ko)
            ctx.apply_stf_f32(src, p, st, out=fv)
            assert np.array_equal(SA.bits_of(fv.cpu().numpy()), SA.bits_of(want_f32)), w
            assert bool((fb[:ko] == -7.0).all()), w
    assert bool((base[:k] == -7.0).all()) and np.array_equal(SA.bits_of(view.cpu().numpy()), SA.bits_of(plane)), what      # the input: untouched
    # in place on the unaligned plane (apply_stf_inplace, stf.rs:147-155)
    ctx.apply_stf_f32(view, p, st, out=view)
    assert np.array_equal(SA.bits_of(view.cpu().numpy()), SA.bits_of(want_f32)), what
