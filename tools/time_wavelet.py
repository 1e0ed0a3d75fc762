"""Developer tool: time wavelet denoising (csrc/wavelet.hip) on device planes: 4096^2 with 5 and with 8 scales and the C3 plane size
(13759 x 12451) with 5 scales; the eager f32 torch restatement (tests/wavelet_restatement.py) on the same GPU as the external
yardstick.  One JSON line.

call_ms = median over SAMPLES samples of (wall time of CALLS back-to-back calls, ending in a device synchronise) / CALLS, after a
warm-up; spread_ms = max - min of those samples.  Configurations that are compared are sampled in turn (A B C A B C ...), not one
after the other.  Traffic floor = the plane moves the algorithm needs (2 per fused scale, 4 per two-pass scale, 1 for d_0, 3 for its
select's passes, S + 2 for the reconstruction) x the plane's bytes over the 8.0 TB/s HBM peak (fraction_of_traffic_floor) and over
the 6.29 TB/s a float4 copy reaches on this part (fraction_of_copy_ceiling: the bound a streaming kernel can actually meet).

Under the developer library (AB_LIB_PATH=.../libastroburst_hip_dev.so) the hand-over between the fused and the two-pass form is
swept as well: fused_max_step 0 (two passes throughout), 1, 2, 4, 8, 16, 32 -- the difference between neighbours is what fusing that
one step gains -- and the fused kernel's tile height.  WAVELET_ONLY=4096x5 (or 4096x8, c3x5) restricts the run and WAVELET_NO_SWEEP=1 /
WAVELET_SKIP_TORCH=1 leave the sweep / the torch yardstick out, e.g. under rocprofv3 (tools/wavelet_kernel_stats.py then gives the
per-scale kernel times).  Results are kept as profiles/wavelet_time.json and profiles/wavelet_kernel_stats.txt."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import wavelet_restatement as R  # noqa: E402
import astroburst_amd as ab  # noqa: E402

CALLS = int(os.environ.get("WAVELET_CALLS", "10"))
SAMPLES = int(os.environ.get("WAVELET_SAMPLES", "7"))
ONLY = os.environ.get("WAVELET_ONLY")
HBM_PEAK = 8.0e12
COPY_CEILING = 6.29e12  # what a float4 device copy reaches on this part (MI355X_MICROARCH: 79 % of the peak)
FUSED_TO = 0  # the library's hand-over (csrc/wavelet.hip: kFusedMaxStepDefault; 0 = every scale takes the two-pass form)


def plane_moves(scales, fused_max_step):
    fused = sum(1 for j in range(scales) if (1 << j) <= fused_max_step)
    return 2 * fused + 4 * (scales - fused) + 1 + 3 + (scales + 2)


def sample(fn):
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / CALLS


def interleaved(configs):
    """configs: {name: (env, fn)} -> {name: (median, spread)}; every sample of every configuration runs under its own environment"""
    ts = {k: [] for k in configs}
    for rnd in range(SAMPLES + 1):
        for name, (env, fn) in configs.items():
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                t = sample(fn)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            if rnd > 0:  # (round 0 warms every configuration up)
                ts[name].append(t)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in ts.items()}


ctx = ab.Context(0)
ctx.use_torch_stream()
dev = ab.is_dev_build()
sweep = dev and not os.environ.get("WAVELET_NO_SWEEP")
res = {"calls_per_sample": CALLS, "samples": SAMPLES, "developer_library": dev, "hbm_peak_tb_s": HBM_PEAK / 1e12}
for label, rows, cols, scales in (("4096x5", 4096, 4096, 5), ("4096x8", 4096, 4096, 8), ("c3x5", 13759, 12451, 5)):
    if ONLY and ONLY != label:
        continue
    g = torch.Generator(device="cuda").manual_seed(5)
    img = (300.0 + torch.randn((rows, cols), device="cuda", generator=g) * 20.0).float()
    out = torch.empty_like(img)
    th = R.DEFAULT_THRESHOLDS

    def call():
        ctx.wavelet_denoise(img, scales, th, True, out=out)

    configs = {"default": ({}, call)}
    if sweep:
        for m in (0, 1, 2, 4, 8, 16, 32):
            configs[f"fused_max_step_{m}"] = ({"AB_WAVELET_FUSED_MAX_STEP": str(m)}, call)
        for tr in (32, 128):
            configs[f"tile_rows_{tr}"] = ({"AB_WAVELET_TILE_ROWS": str(tr)}, call)
    got = interleaved(configs)
    nbytes = rows * cols * 4
    entry = {"rows": rows, "cols": cols, "scales": scales}
    for name, (ms, spread) in got.items():
        m = FUSED_TO if not name.startswith("fused_max_step_") else int(name.rsplit("_", 1)[1])
        floor_ms = plane_moves(scales, m) * nbytes / HBM_PEAK * 1e3
        entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4), "plane_moves": plane_moves(scales, m),
                       "traffic_floor_ms": round(floor_ms, 4), "fraction_of_traffic_floor": round(floor_ms / ms, 4),
                       "fraction_of_copy_ceiling": round(floor_ms * HBM_PEAK / COPY_CEILING / ms, 4)}
    if not os.environ.get("WAVELET_SKIP_TORCH"):
        t = [0.0]

        def torch_call():
            t[0] = R.wavelet_denoise_torch(img, scales, th, True, device="cuda")[2]

        torch_call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            torch_call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        entry["torch_eager_f32_ms"] = round(statistics.median(ts), 3)
        entry["noise_estimate_matches_torch"] = t[0] == ctx.wavelet_denoise(img, scales, th, True, out=out)[2]
    res[label] = entry
    del img, out
    torch.cuda.empty_cache()
print(json.dumps(res))
