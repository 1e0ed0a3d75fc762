"""Developer tool: time the synthetic generator's device entry points (csrc/synth.hip) on device-resident planes -- 4096^2, the size
the reference's serial apply_noise walks with one ChaCha12 generator -- and, in the same run, a plane copy as the yardstick.  One
JSON line.  Run it in a fresh process.

call_ms = median over --samples samples of the time per call: HIP events on the stream around --calls back-to-back calls, after one
warm-up round.  spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...).

traffic_floor_ms = the bytes an entry has to move over the measured copy rate (--copy-gbs, default 6290 GB/s): 4 B per pixel written
for the flat field, 8 B (one read, one write) for the noise, 4 B written for the rendering (its star tables are a few KB).  The
kernels are expected to be issue-bound, not traffic-bound: fraction_of_traffic_floor says how far."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import astroburst_amd as ab  # noqa: E402


def sample(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def interleaved(entries, samples, calls):
    ts = {k: [] for k in entries}
    for rnd in range(samples + 1):
        for name, fn in entries.items():
            t = sample(fn, calls)
            if rnd > 0:  # (round 0 warms every entry up)
                ts[name].append(t)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--stars", type=int, default=500)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--copy-gbs", type=float, default=6290.0)
    args = ap.parse_args()
    rows = cols = args.size
    rate = args.copy_gbs * 1e9
    ctx = ab.Context(0)
    ctx.use_torch_stream()
    cfg = ab.synth_config(width=cols, height=rows, n_stars=args.stars, n_frames=args.frames)
    stars = ab.synth_star_field(cfg)
    truth = ctx.synth_render_stars(stars, ("gaussian", 3.0), rows, cols, device=True)
    flat = torch.empty_like(truth)
    noisy = torch.empty_like(truth)
    copy_dst = torch.empty_like(truth)
    entries = {
        "render_stars": lambda: ctx.synth_render_stars(stars, ("gaussian", 3.0), rows, cols, out=truth),
        "flat_field": lambda: ctx.synth_flat_field(rows, cols, 1122, 0.3, out=flat),
        "apply_noise": lambda: ctx.synth_apply_noise(truth, out=noisy),
        "generate_stack": lambda: ctx.synth_generate_stack(cfg, device=True, want_truth=False),
        "copy": lambda: copy_dst.copy_(truth),
    }
    px = rows * cols
    floors = {"render_stars": 4 * px, "flat_field": 4 * px, "apply_noise": 8 * px, "generate_stack": 8 * px * args.frames + 4 * px, "copy": 8 * px}
    first = ctx.synth_generate_stack(cfg, device=True, want_truth=False)
    got = interleaved(entries, args.samples, args.calls)
    res = {"rows": rows, "cols": cols, "stars": int(stars.shape[0]), "frames": args.frames, "frames_on_host": first.frames_on_host,
           "calls_per_sample": args.calls, "samples": args.samples, "copy_rate_GBs": args.copy_gbs}
    for name, (ms, spread) in got.items():
        floor_ms = floors[name] / rate * 1e3
        res[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4), "traffic_floor_ms": round(floor_ms, 4),
                     "fraction_of_traffic_floor": round(floor_ms / ms, 4)}
    res["apply_noise"]["Mpx_per_s"] = round(px / got["apply_noise"][0] / 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
