"""HIP parity of the robust asinh preview and the byte renderers (csrc/preview.hip) on one MI355X against the numpy restatement of
math/simd.rs:9-214 and infra/render/grayscale.rs (tests/preview_restatement.py; pinned by tests/test_preview_cpu.py).

Statistics, the AVX2 route and the scalar route's Taylor branch: bit for bit, through uint32 views.  The scalar route's log branch (and
so the AVX2 route's n % 8 tail): the rule tests/test_gpu_cube.py applies to the same construction -- within 1 f32 ulp of the definition
(the f32 rounding of the f64 log) and not bit-identical on at most 2 values per 2^21.  Every renderer: byte for byte.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import preview_restatement as R
from astroburst_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
ROUTES = (R.AVX2, R.SCALAR)
SHAPE_IDS = ["x".join(map(str, s)) for s in R.SHAPES]


def _dev(a, offset=0):
    """the array on the device; offset > 0: at a pointer `offset` elements past a 256-byte aligned allocation"""
    import torch
    a = np.array(a, copy=True, order="C")   # (the cached fixtures are read-only)
    if not offset:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() == buf.data_ptr() + offset * a.itemsize and view.is_contiguous()
    return view


def _dev_empty(shape, dtype, offset):
    import torch
    n = int(np.prod(shape))
    buf = torch.zeros(n + offset, dtype=dtype, device="cuda")
    return buf[offset:offset + n].view(shape)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _stats_tuple(st):
    return (F32(st.median), F32(st.sigma), F32(st.low), F32(st.high), int(st.valid_count))


def assert_stats(got, want, what):
    got = _stats_tuple(got) if not isinstance(got, tuple) else got
    assert got[4] == want[4], f"{what}: valid_count {got[4]} != {want[4]}"
    g, w = np.array(got[:4], F32), np.array(want[:4], F32)
    assert (R.bits(g) == R.bits(w)).all(), f"{what}: got {g!r} want {w!r}"


def assert_bits(got, want, what):
    got, want = _host(got), np.asarray(want, F32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(R.bits(got).ravel() != R.bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: got {got.ravel()[bad[0]]!r} want {want.ravel()[bad[0]]!r}"


def assert_bytes(got, want, what):
    got = _host(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} != {want.shape}"
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: got {got.ravel()[bad[0]]} want {want.ravel()[bad[0]]}"


def assert_map(got, img, stats, route, what):
    """the map against the restatement: bit for bit outside the scalar formula's log branch, the cube's rule inside it"""
    got = _host(got)
    want = R.normalize_with_stats(img, stats, route)
    n = img.size
    log_branch = np.zeros(n, bool)
    if stats[4] > 0:
        with np.errstate(all="ignore"):
            log_branch = R.is_valid(img).ravel() & ~(np.abs(R.scaled_of(img, stats)).ravel() < F32(0.5))
        if route == R.AVX2:
            log_branch[:8 * (n // 8)] = False
    g, w = got.ravel(), want.ravel()
    exact = ~log_branch
    bad = np.flatnonzero(exact & (R.bits(g) != R.bits(w)))
    assert bad.size == 0, f"{what}: {bad.size} of {int(exact.sum())} exact values differ, first at {bad[0]}: got {g[bad[0]]!r} want {w[bad[0]]!r}"
    if log_branch.any():
        d = R.ulp_distance(g[log_branch], w[log_branch])
        differ = int((d > 0).sum())
        cap = 2 * max(1, -(-n // (1 << 21)))
        assert d.max() <= 1, f"{what}: {int(d.max())} ulp from the definition in the log branch"
        assert differ <= cap, f"{what}: {differ} log-branch values of {int(log_branch.sum())} are not bit-identical (cap {cap})"


@functools.lru_cache(maxsize=None)
def _cases(shape):
    """name -> (plane, restated statistics, {route: restated bytes of render_asinh_and_save}); computed once, never modified"""
    out = {}
    for name, img in R.preview_cases(shape):
        img.setflags(write=False)
        out[name] = (img, R.preview_stats(img), {route: R.render_asinh_and_save(img, route) for route in ROUTES})
    return out


CASE_NAMES = [name for name, _ in R.preview_cases((1, 8))]


# ---- the preview ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_preview_matches_the_restatement(ctx, shape, case):
    img, want_stats, want_bytes = _cases(shape)[case]
    dimg = _dev(img)
    assert_stats(ctx.asinh_preview_stats(dimg), want_stats, f"{case} stats device")
    assert_stats(ctx.asinh_preview_stats(img), want_stats, f"{case} stats host")
    for route in ROUTES:
        what = f"{case} {shape} route {route}"
        preview, st = ctx.robust_asinh_preview(dimg, route, want_stats=True)
        assert_stats(st, want_stats, f"{what} stats_out")
        assert_map(preview, img, want_stats, route, f"{what} device")
        hpreview = ctx.robust_asinh_preview(img, route)
        assert_bits(hpreview, _host(preview), f"{what} host plane against device plane")
        # the map alone: out of place, and in place on a copy
        alone = ctx.asinh_normalize_with_stats(dimg, want_stats, route)
        assert_bits(alone, _host(preview), f"{what} normalize_with_stats")
        inplace = dimg.clone()
        assert ctx.asinh_normalize_with_stats(inplace, want_stats, route, out=inplace) is inplace
        assert_bits(inplace, _host(preview), f"{what} in place")
        # the fused render: the restatement's bytes, and the bytes of the unfused pair on the GPU
        fused, st = ctx.render_asinh_preview(dimg, route, want_stats=True)
        assert_stats(st, want_stats, f"{what} render stats_out")
        assert_bytes(fused, want_bytes[route], f"{what} fused render")
        assert_bytes(ctx.render_grayscale(preview), _host(fused), f"{what} unfused pair")
        assert_bytes(ctx.render_asinh_preview(img, route), _host(fused), f"{what} fused render, host plane")


@pytest.mark.parametrize("offset", (1, 3))
def test_unaligned_device_planes(ctx, offset):
    """257 x 129 from device pointers offset by one and by three floats (outputs offset too): the 8-pixel boundary of the AVX2 route
    is counted from index 0, not from the pointer's alignment"""
    shape = R.OFFSET_SHAPE
    import torch
    for case in ("stars_odd", "nonfinite", "outliers"):
        img, want_stats, want_bytes = _cases(shape)[case]
        dimg = _dev(img, offset)
        assert dimg.data_ptr() % 16 == 4 * offset
        assert_stats(ctx.asinh_preview_stats(dimg), want_stats, f"{case} stats")
        for route in ROUTES:
            what = f"{case} offset {offset} route {route}"
            out = _dev_empty(shape, torch.float32, 4 - offset)           # (a different misalignment than the input's)
            ctx.robust_asinh_preview(dimg, route, out=out)
            assert_map(out, img, want_stats, route, what)
            inplace = _dev(img, offset)
            ctx.asinh_normalize_with_stats(inplace, want_stats, route, out=inplace)
            assert_bits(inplace, _host(out), f"{what} in place")
            u8 = _dev_empty(shape, torch.uint8, offset)                  # (bytes at an odd address)
            ctx.render_asinh_preview(dimg, route, out=u8)
            assert_bytes(u8, want_bytes[route], f"{what} fused render")
    rp = R.render_plane(shape)
    drp = _dev(rp, offset)
    for bits_ in (8, 16):
        for out_offset in (0, offset, 2):
            out = _dev_empty(shape if bits_ == 8 else shape + (2,), torch.uint8, out_offset)
            assert_bytes(ctx.render_grayscale(drp, bits_, out=out), R.render_grayscale(rp, bits_)[0], f"grayscale {bits_} out offset {out_offset}")
            out = _dev_empty(shape if bits_ == 8 else shape + (2,), torch.uint8, out_offset)
            assert_bytes(ctx.render_stretched(drp, bits_, out=out), R.render_stretched(rp, bits_), f"stretched {bits_} out offset {out_offset}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_map_with_the_callers_statistics(ctx, shape):
    """arguments the robust statistics of positive data cannot produce: a subnormal `scaled`, tail pixels on both sides of
    |scaled| = 0.5, magnitudes through fast_log's whole exponent range"""
    for name, img, stats in R.stats_cases(shape):
        dimg = _dev(img)
        for route in ROUTES:
            got = ctx.asinh_normalize_with_stats(dimg, stats, route)
            assert_map(got, img, stats, route, f"{name} {shape} route {route}")
            assert_bits(ctx.asinh_normalize_with_stats(img, stats, route), _host(got), f"{name} host plane")
    # no valid pixel by the caller's word: a copy of the input, NaN payloads included
    img = R.all_invalid_plane(shape)
    assert_bits(ctx.asinh_normalize_with_stats(_dev(img), (0, 0, 0, 0, 0), R.AVX2), img, "valid_count == 0")


# ---- the plain renderers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_plain_renderers_match_byte_for_byte(ctx, shape):
    planes = [("mixed", R.render_plane(shape)), ("stars", R.star_field(shape, 5)), ("no_finite", np.full(shape, np.nan, F32)),
              ("all_invalid", R.all_invalid_plane(shape)), ("huge_range", np.resize(np.array([3e38, -3e38, 1.0, 2.0], F32), shape[0] * shape[1]).reshape(shape))]
    for name, img in planes:
        dimg = _dev(img)
        for bits_ in (8, 16):
            want, mn, mx = R.render_grayscale(img, bits_)
            got, gmn, gmx = ctx.render_grayscale(dimg, bits_, want_range=True)
            assert_bytes(got, want, f"{name} grayscale {bits_} device")
            assert (F32(gmn), F32(gmx)) == (mn, mx), f"{name}: range {(gmn, gmx)} != {(mn, mx)}"
            assert_bytes(ctx.render_grayscale(img, bits_), want, f"{name} grayscale {bits_} host")
            want = R.render_stretched(img, bits_)
            assert_bytes(ctx.render_stretched(dimg, bits_), want, f"{name} stretched {bits_} device")
            assert_bytes(ctx.render_stretched(img, bits_), want, f"{name} stretched {bits_} host")
            if bits_ == 16:
                assert (_host(got).view(">u2")[..., 0] == R.render_grayscale(img, 16)[0].view(">u2")[..., 0]).all()


# ---- error returns ------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(ctx):
    L, h, INVALID = ctx._L, ctx._h, _lib.AB_ERR_INVALID
    img = np.ones((4, 6), F32)
    out = np.zeros((4, 6), F32)
    buf = (C.c_uint8 * 64)()

    def plane(a, rows=4, cols=6):
        return _lib.Plane(C.c_void_p(a.ctypes.data if a is not None else None), rows, cols, 0)

    p, po, st = plane(img), plane(out), _lib.AsinhStatsC(1.0, 1.0, 0.5, 2.0, 24)
    null_data, no_rows, no_cols, small = plane(None), plane(img, 0, 6), plane(img, 4, -1), plane(out, 3, 6)
    ref = C.byref
    # NULL arguments
    assert L.ab_asinh_preview_stats(h, None, ref(st)) == INVALID and L.ab_asinh_preview_stats(h, ref(p), None) == INVALID
    assert L.ab_asinh_preview_stats(h, ref(null_data), ref(st)) == INVALID
    assert L.ab_asinh_normalize_with_stats(h, None, ref(st), 0, ref(po)) == INVALID
    assert L.ab_asinh_normalize_with_stats(h, ref(p), None, 0, ref(po)) == INVALID
    assert L.ab_asinh_normalize_with_stats(h, ref(p), ref(st), 0, None) == INVALID
    assert L.ab_robust_asinh_preview(h, None, 0, ref(po), None) == INVALID and L.ab_robust_asinh_preview(h, ref(p), 0, None, None) == INVALID
    assert L.ab_render_asinh_preview(h, None, 0, buf, 0, None) == INVALID and L.ab_render_asinh_preview(h, ref(p), 0, None, 0, None) == INVALID
    assert L.ab_render_grayscale(h, None, 8, buf, 0, None, None) == INVALID and L.ab_render_grayscale(h, ref(p), 8, None, 0, None, None) == INVALID
    assert L.ab_render_stretched(h, None, 8, buf, 0) == INVALID and L.ab_render_stretched(h, ref(p), 8, None, 0) == INVALID
    # dims < 1
    for bad in (no_rows, no_cols):
        assert L.ab_asinh_preview_stats(h, ref(bad), ref(st)) == INVALID
        assert L.ab_asinh_normalize_with_stats(h, ref(bad), ref(st), 0, ref(po)) == INVALID
        assert L.ab_robust_asinh_preview(h, ref(bad), 0, ref(po), None) == INVALID
        assert L.ab_render_asinh_preview(h, ref(bad), 0, buf, 0, None) == INVALID
        assert L.ab_render_grayscale(h, ref(bad), 8, buf, 0, None, None) == INVALID
        assert L.ab_render_stretched(h, ref(bad), 8, buf, 0) == INVALID
    # an output that does not match; an output that overlaps the image without being it
    assert L.ab_asinh_normalize_with_stats(h, ref(p), ref(st), 0, ref(small)) == INVALID
    assert L.ab_robust_asinh_preview(h, ref(p), 0, ref(small), None) == INVALID
    two = np.ones((5, 6), F32)
    shifted = _lib.Plane(C.c_void_p(two.ctypes.data + 24), 4, 6, 0)
    assert L.ab_asinh_normalize_with_stats(h, ref(plane(two)), ref(st), 0, ref(shifted)) == INVALID
    # a route outside {0, 1}; bits outside {8, 16}
    for route in (-1, 2):
        assert L.ab_asinh_normalize_with_stats(h, ref(p), ref(st), route, ref(po)) == INVALID
        assert L.ab_robust_asinh_preview(h, ref(p), route, ref(po), None) == INVALID
        assert L.ab_render_asinh_preview(h, ref(p), route, buf, 0, None) == INVALID
    for bits_ in (0, 12, 32):
        assert L.ab_render_grayscale(h, ref(p), bits_, buf, 0, None, None) == INVALID
        assert L.ab_render_stretched(h, ref(p), bits_, buf, 0) == INVALID
    # statistics f32::clamp would panic on
    for bad in (_lib.AsinhStatsC(1.0, 1.0, 2.0, 0.5, 24), _lib.AsinhStatsC(float("nan"), 1.0, 0.5, 2.0, 24)):
        assert L.ab_asinh_normalize_with_stats(h, ref(p), ref(bad), 0, ref(po)) == INVALID
    assert b"" != L.ab_last_error(h)
    # and the context still works
    assert L.ab_robust_asinh_preview(h, ref(p), 0, ref(po), None) == _lib.AB_OK
    assert (R.bits(out) == R.bits(R.robust_asinh_preview(img, R.AVX2))).all()
