"""What a change of who releases an entry point's staged planes can break and the value tests do not see (csrc/entry_host.hpp's
Scope in the older half of the C ABI): one table of entry points, at least one per converted file, on planes of 5 x 7 (no 16-byte
group) and 33 x 65 (a head, groups and a tail).

1. host planes and device planes give bit-identical outputs (the host route is the one that owns temporaries);
2. a refused call leaves the context usable: the same good call before and after it, bit-identical -- where an entry point refuses
   after it has staged something, that refusal is the one taken;
3. host inputs with a device output, and the reverse, equal the all-device result (entry points whose wrapper takes `out`).

No value is compared to the oracle here: the restatement tests do that.  No test reads device memory totals."""
import dataclasses

import numpy as np
import pytest

from astroburst_amd import AstroBurstError, ImageStats, StfParams

pytestmark = pytest.mark.gpu

SMALL, BIG = (5, 7), (33, 65)
BOTH = (SMALL, BIG)


def _torch():
    import torch
    return torch


def to_host(a):
    return np.array(a, copy=True)


def to_dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


to_host.device, to_dev.device = False, True


def other_side(like, device):
    """an uninitialised array of `like`'s shape and dtype on the host or the device"""
    if device:
        return _torch().empty(like.shape, dtype=getattr(_torch(), str(like.dtype)), device="cuda")
    return np.empty(like.shape, like.dtype)


def wrong_size(device, rows, cols):
    """a float32 output plane whose own dims reach the library (a numpy output travels with the dims the wrapper gives it)"""
    return _torch().empty((rows, cols), dtype=_torch().float32, device="cuda" if device else "cpu")


def flatten(x, into=None):
    """every array, tensor and number of a result, in order, as numpy arrays"""
    into = [] if into is None else into
    if x is None:
        return into
    if dataclasses.is_dataclass(x):
        x = [getattr(x, f.name) for f in dataclasses.fields(x)]
    if isinstance(x, dict):
        x = list(x.values())
    if isinstance(x, (tuple, list)):
        for v in x:
            flatten(v, into)
    elif hasattr(x, "cpu"):
        into.append(x.cpu().numpy())
    elif isinstance(x, (str, bytes)):
        into.append(np.frombuffer(x.encode() if isinstance(x, str) else x, np.uint8))
    else:
        into.append(np.asarray(x))
    return into


def same_bits(a, b):
    a, b = flatten(a), flatten(b)
    return len(a) == len(b) and all(p.shape == q.shape and p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(a, b))


def plane(shape, seed, lo=0.05, hi=0.95):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)


def stars_plane(shape=BIG):
    """a few round stars on a faint noisy sky"""
    rows, cols = shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = 0.02 + 0.002 * np.random.default_rng(11).standard_normal(shape)
    for cy, cx, amp in ((9.0, 12.0, 0.6), (16.3, 40.2, 0.5), (23.6, 25.4, 0.55), (11.2, 52.7, 0.45), (24.1, 54.3, 0.4)):
        img += amp * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * 1.6 ** 2))
    return img.astype(np.float32)


def stats_of(a):
    a = a.astype(np.float64)
    med = float(np.median(a))
    mad = float(np.median(np.abs(a - med)))
    return ImageStats(float(a.min()), float(a.max()), med, mad, mad * 1.4826, float(a.mean()), a.size)


STF = StfParams(0.1, 0.3, 0.9)


def cube_stats():
    from astroburst_amd.core import GlobalCubeStats
    return GlobalCubeStats(0.4, 0.2, 0.1, 0.9)


def asinh_stats():
    from astroburst_amd.core import AsinhStats
    return AsinhStats(0.4, 0.2, 0.1, 0.9, 35)


# ---- the table: run(ctx, put, shape, out=None) -> result; refuse(ctx, put, shape) makes a call the library refuses -----------------
def c_scale(ctx, put, s, out=None):
    return ctx.scale(put(plane(s, 1)), 1.5, out=out)


def r_scale(ctx, put, s):
    ctx.scale(put(plane(s, 1)), 1.5, out=wrong_size(put.device, s[0] + 1, s[1]))


def c_levels(ctx, put, s, out=None):
    return ctx.apply_levels(put(plane(s, 2)), 0.1, 1.7, 0.8, out=out)


def c_blend(ctx, put, s):
    return ctx.blend_channels([put(plane(s, 3)), put(plane(s, 4))], [(0, 1.0, 0.0, 0.25), (1, 0.0, 1.0, 0.5), (7, 1.0, 1.0, 1.0)], s[0], s[1])


def r_blend(ctx, put, s):
    ctx.blend_channels([put(plane(s, 3)), put(plane((s[0] - 1, s[1]), 4))], [(0, 1.0, 0.0, 0.25)], s[0], s[1])


def c_luminance(ctx, put, s, out=None):
    return ctx.luminance(put(plane(s, 5)), put(plane(s, 6)), put(plane(s, 7)), out=out)


def r_luminance(ctx, put, s):
    ctx.luminance(put(plane(s, 5)), put(plane((s[0], s[1] + 1), 6)), put(plane(s, 7)))


def c_calibrate(ctx, put, s, out=None):
    return ctx.calibrate_image(put(plane(s, 8)), put(plane(s, 9, 0.0, 0.01)), put(plane(s, 10, 0.0, 0.02)), put(plane(s, 11, 0.8, 1.2)), 1.5, out=out)


def r_calibrate(ctx, put, s):  # reaches unary_map's check after the three masters are staged
    ctx.calibrate_image(put(plane(s, 8)), put(plane(s, 9, 0.0, 0.01)), put(plane(s, 10, 0.0, 0.02)), put(plane(s, 11, 0.8, 1.2)), 1.5,
                        out=wrong_size(put.device, s[0], s[1] + 1))


def c_scnr(ctx, put, s):
    r, g, b = put(plane(s, 12)), put(plane(s, 13)), put(plane(s, 14))
    ctx.apply_scnr_inplace(r, g, b, "average", 0.8, True)
    return r, g, b


def c_lrgb(ctx, put, s):
    r, g, b = put(plane(s, 15)), put(plane(s, 16)), put(plane(s, 17))
    ctx.apply_lrgb(put(plane(s, 18)), r, g, b, 0.7, 0.6)
    return r, g, b


def r_lrgb(ctx, put, s):
    ctx.apply_lrgb(put(plane((s[0] + 1, s[1]), 18)), put(plane(s, 15)), put(plane(s, 16)), put(plane(s, 17)))


def c_synth_lum(ctx, put, s, out=None):
    return ctx.synthesize_luminance(put(plane(s, 19)), put(plane(s, 20)), put(plane(s, 21)), out=out)


def r_synth_lum(ctx, put, s):
    ctx.synthesize_luminance(put(plane(s, 19)), put(plane(s, 20)), put(plane((s[0], s[1] - 1), 21)))


def c_cal_channel(ctx, put, s):
    a = plane(s, 22)
    return ctx.calibrate_channel(put(a), 1.25, stats_of(a))


def c_master_flat(ctx, put, s):  # three frames less a bias and a dark: the per-frame scope, then the flat's normalisation
    return ctx.create_master("flat", [put(plane(s, 23 + i, 0.4, 0.9)) for i in range(3)], put(plane(s, 26, 0.0, 0.01)), put(plane(s, 27, 0.0, 0.02)))


def c_master_dark(ctx, put, s):
    return ctx.create_master("dark", [put(plane(s, 23 + i)) for i in range(3)], put(plane(s, 26, 0.0, 0.01)))


def r_master(ctx, put, s):
    ctx.create_master("flat", [put(plane(s, 23)), put(plane((s[0], s[1] + 1), 24)), put(plane(s, 25))], put(plane(s, 26, 0.0, 0.01)),
                      put(plane(s, 27, 0.0, 0.02)))


def c_stf_u8(ctx, put, s, out=None):
    a = plane(s, 28)
    return ctx.apply_stf(put(a), STF, stats_of(a), out=out)


def c_stf_f32(ctx, put, s, out=None):
    a = plane(s, 29)
    return ctx.apply_stf_f32(put(a), STF, stats_of(a), out=out)


def r_stf_f32(ctx, put, s):
    a = plane(s, 29)
    ctx.apply_stf_f32(put(a), STF, stats_of(a), out=wrong_size(put.device, s[0] + 2, s[1]))


def c_fits_encode(ctx, put, s):
    a = plane(s, 30)
    bz, bs = ctx.fits_compute_bzero_bscale(put(a))
    return bz, bs, ctx.fits_encode_pixels(put(a), 16, bz, bs), ctx.fits_encode_pixels(put(a), -32), ctx.fits_encode_pixels(put(a), -64)


def _raw(s, dtype):
    return np.random.default_rng(31).integers(0, 30000, s).astype(dtype).view(np.uint8).reshape(-1)


def c_fits_decode(ctx, put, s, out=None):
    return ctx.fits_decode_pixels(put(_raw(s, ">i2")), s[0], s[1], 16, 1.5, 32768.0, out=out)


def r_fits_decode(ctx, put, s):
    ctx.fits_decode_pixels(put(_raw(s, ">i2")), s[0] + 1, s[1], 16)


def c_shift(ctx, put, s, out=None):
    return ctx.shift_image_subpixel(put(plane(s, 32)), 0.3, -0.7, out=out)


def r_shift(ctx, put, s):
    ctx.shift_image_subpixel(put(plane(s, 32)), 0.3, -0.7, out=wrong_size(put.device, s[0], s[1] + 3))


def c_warp(ctx, put, s, out=None):
    return ctx.warp_image(put(plane(s, 33)), (0.98, 0.05, 0.4, -0.05, 1.01, -0.3), s[0] + 1, s[1] + 2, out=out)


def c_resample(ctx, put, s, out=None):
    return ctx.resample_image(put(plane(s, 34)), 2 * s[0] - 1, s[1] + 3, out=out)


def r_resample(ctx, put, s):
    ctx.resample_image(put(plane(s, 34)), 0, s[1])


def _sky(s):
    y, x = np.mgrid[0:s[0], 0:s[1]].astype(np.float32)
    return (0.2 + 0.003 * y + 0.002 * x).astype(np.float32) + plane(s, 35, 0.0, 0.01)


def c_background_model(ctx, put, s):
    return ctx.extract_background(put(_sky(s)), grid_size=4, poly_degree=1, want_model=True)


def c_background_plain(ctx, put, s):
    return ctx.extract_background(put(_sky(s)), grid_size=4, poly_degree=1, mode="divide", want_model=False)


def r_background(ctx, put, s):  # one cell gives one sample at most: ab_background_sample_fit refuses, the image already staged
    ctx.extract_background(put(_sky(SMALL)), grid_size=1, poly_degree=0)


def c_subframe(ctx, put, s):
    return ctx.analyze_subframe(put(stars_plane(s)))


def c_phase(ctx, put, s):
    a = plane(s, 36)
    return ctx.phase_correlate(put(a), put(np.roll(a, (1, 2), (0, 1))))


def c_correlate_single(ctx, put, s):
    a = plane(s, 37)
    return ctx.correlate_single(put(a), put(np.roll(a, (1, 1), (0, 1))), want_surface=True)


def r_correlate_single(ctx, put, s):
    ctx.correlate_single(put(plane(s, 37)), put(plane((s[0], s[1] + 1), 38)))


def c_preview_stats(ctx, put, s):
    return ctx.asinh_preview_stats(put(plane(s, 39)))


def c_preview_normalize(ctx, put, s, out=None):
    return ctx.asinh_normalize_with_stats(put(plane(s, 40)), asinh_stats(), out=out)


def c_preview_robust(ctx, put, s, out=None):
    return ctx.robust_asinh_preview(put(plane(s, 41)), route=1, out=out, want_stats=True)


def r_preview_robust(ctx, put, s):
    ctx.robust_asinh_preview(put(plane(s, 41)), out=wrong_size(put.device, s[0] + 1, s[1]))


def c_preview_render(ctx, put, s, out=None):
    return ctx.render_asinh_preview(put(plane(s, 42)), out=out, want_stats=True)


def c_render_gray16(ctx, put, s, out=None):
    return ctx.render_grayscale(put(plane(s, 43)), 16, out=out, want_range=True)


def c_render_stretched(ctx, put, s, out=None):
    return ctx.render_stretched(put(plane(s, 44, -0.2, 1.2)), 8, out=out)


def r_render_bits(ctx, put, s):
    ctx.render_stretched(put(plane(s, 44)), 12, out=other_side(np.empty(s, np.uint8), put.device))


def c_ipc(ctx, put, s, out=None):
    return ctx.ipc_encode_with_header(put(plane(s, 45)), 0, out=out)


def c_ipc_sampled(ctx, put, s):
    return ctx.ipc_encode_with_header(put(plane(s, 45)), 4)


def r_ipc(ctx, put, s):
    ctx.ipc_encode_with_header(put(plane(s, 45)), -1)


def c_tile_down(ctx, put, s):
    return ctx.tile_downsample_2x(put(plane(s, 46)))


def c_tile_bounds(ctx, put, s):
    return ctx.tile_percentile_bounds(put(plane(s, 47)), 0.01, 0.99)


def c_tile_pyramid(ctx, put, s, out=None):
    tiles, levels, bounds = ctx.generate_tile_pyramid(put(plane(s, 48)), 16, out=out)
    return tiles, bounds


def _cube(s):
    c = np.random.default_rng(49).uniform(0.05, 0.95, (4,) + tuple(s)).astype(np.float32)
    c[1, 0, 0] = 0.0
    return c


def c_cube_mean(ctx, put, s, out=None):
    return ctx.collapse_mean(put(_cube(s)), out=out)


def c_cube_median(ctx, put, s, out=None):
    return ctx.collapse_median(put(_cube(s)), out=out)


def r_cube(ctx, put, s):
    ctx.collapse_mean(put(_cube(s)), out=wrong_size(put.device, s[0], s[1] + 1))


def c_cube_normalize(ctx, put, s, out=None):
    return ctx.normalize_with_global(put(plane(s, 50)), cube_stats(), out=out)


def r_cube_normalize(ctx, put, s):
    ctx.normalize_with_global(put(plane(s, 50)), cube_stats(), out=wrong_size(put.device, s[0] + 1, s[1]))


def _pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def c_fft2(ctx, put, s, out=None):
    return ctx.fft2_forward(put(plane(s, 51)), _pow2(s[0]), _pow2(s[1]), ctx.hann_symmetric_f32(s[0]), ctx.hann_symmetric_f32(s[1]), out=out)


def c_power_spectrum(ctx, put, s, out=None):
    return ctx.compute_power_spectrum(put(plane(s, 52)), True, out=out)


def r_power_spectrum(ctx, put, s):
    ctx.compute_power_spectrum(put(plane(s, 52)), True, out=wrong_size(put.device, 3, 3))


def c_spectrum_u8(ctx, put, s, out=None):
    return ctx.spectrum_to_u8(put(plane(s, 53, 0.0, 9.0)), out=out)


def _psf3():
    from astroburst_amd.core import generate_gaussian_psf
    return generate_gaussian_psf(3, 0.8)


def c_deconv(ctx, put, s, out=None):
    return ctx.richardson_lucy(put(plane(s, 54)), put(_psf3()), iterations=3, out=out)


def r_deconv(ctx, put, s):
    ctx.richardson_lucy(put(plane(s, 54)), put(_psf3()), iterations=3, out=wrong_size(put.device, s[0], s[1] + 1))


def c_wavelet(ctx, put, s, out=None):
    return ctx.wavelet_denoise(put(plane(s, 55)), num_scales=2, thresholds=(3.0, 2.0), out=out)


def r_wavelet(ctx, put, s):
    ctx.wavelet_denoise(put(plane(s, 55)), num_scales=2, thresholds=(3.0, 2.0), out=wrong_size(put.device, s[0] + 1, s[1]))


def c_psf(ctx, put, s, out=None):
    return ctx.estimate_psf(put(stars_plane(s)), out=out, num_stars=3, cutout_radius=3, edge_margin=4)


def r_psf(ctx, put, s):
    ctx.estimate_psf(put(stars_plane(s)), out=wrong_size(put.device, 5, 5), num_stars=3, cutout_radius=3, edge_margin=4)


STARS = np.array([[2.0, 3.0, 900.0, 0.0, 0.0], [3.5, 1.25, 400.0, 0.0, 0.0]])


def c_synth_render(ctx, put, s, out=None):
    return ctx.synth_render_stars(STARS, ("gaussian", 2.0), s[0], s[1], out=out, device=put.device)


def c_synth_flat(ctx, put, s, out=None):
    return ctx.synth_flat_field(s[0], s[1], 7, 0.3, out=out, device=put.device)


def c_synth_apply_flat(ctx, put, s):
    return ctx.synth_apply_flat_field(put(plane(s, 56)), put(plane(s, 57, 0.5, 1.0)))


def r_synth_apply_flat(ctx, put, s):
    ctx.synth_apply_flat_field(put(plane(s, 56)), put(plane((s[0], s[1] + 1), 57, 0.5, 1.0)))


def c_synth_noise(ctx, put, s, out=None):
    return ctx.synth_apply_noise(put(plane(s, 58, 50.0, 900.0)), out=out, seed=5)


def c_synth_stack(ctx, put, s):  # one output staged and finished per frame
    r = ctx.synth_generate_stack(device=put.device, want_truth=True, n_frames=3, apply_vignette=True, vignette_strength=0.2, height=s[0], width=s[1],
                                 n_stars=4, seed=9)
    return r.frames, r.truth, r.stars, r.frames_on_host


def _frames(put, s):
    return [put(plane(s, 60 + i)) for i in range(3)]


OFFSETS = [(0.0, 0.0), (0.25, -0.5), (-0.4, 0.3)]


def c_drizzle_weight(ctx, put, s):
    r = ctx.drizzle_frames(_frames(put, s), OFFSETS, want_weight=True)
    return r.image, r.weight_map, r.rejected_pixels


def c_drizzle_plain(ctx, put, s):
    r = ctx.drizzle_frames(_frames(put, s), OFFSETS, kernel="gaussian", want_weight=False)
    assert r.weight_map is None
    return r.image, r.rejected_pixels


def r_drizzle(ctx, put, s):
    ctx.drizzle_frames(_frames(put, s), [(0.0, 0.0), (float("nan"), 0.0), (0.0, 0.0)])


# name, run, the shapes it takes, its refusal (None: the wrapper offers none that reaches the library), takes `out`
TABLE = [
    ("color.scale", c_scale, BOTH, r_scale, True),
    ("color.levels", c_levels, BOTH, None, True),
    ("color.blend_channels", c_blend, BOTH, r_blend, False),
    ("color.luminance", c_luminance, BOTH, r_luminance, True),
    ("color.calibrate_image", c_calibrate, BOTH, r_calibrate, True),
    ("color.scnr", c_scnr, BOTH, None, False),
    ("extras.apply_lrgb", c_lrgb, BOTH, r_lrgb, False),
    ("extras.synthesize_luminance", c_synth_lum, BOTH, r_synth_lum, True),
    ("extras.calibrate_channel", c_cal_channel, BOTH, None, False),
    ("extras.create_master_flat", c_master_flat, BOTH, r_master, False),
    ("extras.create_master_dark", c_master_dark, BOTH, None, False),
    ("stf.apply_stf_u8", c_stf_u8, BOTH, None, False),   # (its wrapper takes an output of the image's kind only)
    ("stf.apply_stf_f32", c_stf_f32, BOTH, r_stf_f32, True),
    ("fits.encode", c_fits_encode, BOTH, None, False),
    ("fits.decode", c_fits_decode, BOTH, r_fits_decode, True),
    ("resample.shift", c_shift, BOTH, r_shift, True),
    ("resample.warp", c_warp, BOTH, None, True),
    ("resample.resample", c_resample, BOTH, r_resample, True),
    ("background.with_model", c_background_model, (BIG,), r_background, False),   # (5 x 7 has one cell: never enough samples)
    ("background.no_model", c_background_plain, (BIG,), r_background, False),
    ("subframe.analyze", c_subframe, (BIG,), None, False),
    ("phase_corr.phase_correlate", c_phase, BOTH, None, False),
    ("phase_corr.correlate_single", c_correlate_single, BOTH, r_correlate_single, False),
    ("preview.stats", c_preview_stats, BOTH, None, False),
    ("preview.normalize", c_preview_normalize, BOTH, None, True),
    ("preview.robust", c_preview_robust, BOTH, r_preview_robust, True),
    ("preview.render_asinh", c_preview_render, BOTH, None, True),
    ("preview.grayscale16", c_render_gray16, BOTH, None, True),
    ("preview.stretched", c_render_stretched, BOTH, r_render_bits, True),
    ("render.ipc", c_ipc, BOTH, r_ipc, True),
    ("render.ipc_sampled", c_ipc_sampled, BOTH, None, False),
    ("render.tile_downsample", c_tile_down, BOTH, None, False),
    ("render.tile_bounds", c_tile_bounds, BOTH, None, False),
    ("render.tile_pyramid", c_tile_pyramid, BOTH, None, True),
    ("cube.collapse_mean", c_cube_mean, BOTH, r_cube, True),
    ("cube.collapse_median", c_cube_median, BOTH, None, True),
    ("cube.normalize_frame", c_cube_normalize, BOTH, r_cube_normalize, True),
    ("spectrum.fft2", c_fft2, BOTH, None, True),
    ("spectrum.power_spectrum", c_power_spectrum, BOTH, r_power_spectrum, True),
    ("spectrum.to_u8", c_spectrum_u8, BOTH, None, True),
    ("deconv.richardson_lucy", c_deconv, BOTH, r_deconv, True),
    ("wavelet.denoise", c_wavelet, BOTH, r_wavelet, True),
    ("psf.estimate", c_psf, (BIG,), r_psf, True),                                  # (it needs stars inside the edge margin)
    ("synth.render_stars", c_synth_render, BOTH, None, True),
    ("synth.flat_field", c_synth_flat, BOTH, None, True),
    ("synth.apply_flat_field", c_synth_apply_flat, BOTH, r_synth_apply_flat, False),
    ("synth.apply_noise", c_synth_noise, BOTH, None, True),
    ("synth.generate_stack", c_synth_stack, BOTH, None, False),
    ("drizzle.frames_weight", c_drizzle_weight, BOTH, r_drizzle, False),
    ("drizzle.frames_plain", c_drizzle_plain, BOTH, None, False),
]

CASES = [pytest.param(run, s, id=f"{name}-{s[0]}x{s[1]}") for name, run, shapes, _, _ in TABLE for s in shapes]
REFUSALS = [pytest.param(run, refuse, s, id=f"{name}-{s[0]}x{s[1]}") for name, run, shapes, refuse, _ in TABLE if refuse for s in shapes]
MIXED = [pytest.param(run, s, id=f"{name}-{s[0]}x{s[1]}") for name, run, shapes, _, has_out in TABLE if has_out for s in shapes]


@pytest.fixture(scope="module")
def device_results(ctx):
    """the all-device result of every (entry point, shape), computed once and left unchanged"""
    cache = {}

    def get(run, shape):
        key = (run.__name__, shape)
        if key not in cache:
            cache[key] = flatten(run(ctx, to_dev, shape))
        return cache[key]
    return get


@pytest.mark.parametrize("run,shape", CASES)
def test_host_planes_equal_device_planes(ctx, device_results, run, shape):
    assert same_bits(run(ctx, to_host, shape), device_results(run, shape))


@pytest.mark.parametrize("put", [to_host, to_dev], ids=["host", "device"])
@pytest.mark.parametrize("run,refuse,shape", REFUSALS)
def test_refused_call_leaves_the_context_usable(ctx, run, refuse, shape, put):
    before = flatten(run(ctx, put, shape))
    with pytest.raises(AstroBurstError):
        refuse(ctx, put, shape)
    assert same_bits(run(ctx, put, shape), before)


@pytest.mark.parametrize("run,shape", MIXED)
def test_mixed_residency(ctx, device_results, run, shape):
    want = device_results(run, shape)
    first = want[0]  # the plane, bytes or spectrum the entry point writes: every wrapper returns it first
    for put in (to_host, to_dev):  # host inputs with a device output, then the reverse
        assert same_bits(run(ctx, put, shape, out=other_side(first, not put.device)), want)
