"""Developer tool: time every spectral-cube entry point (csrc/cube.hip, plane_select.hip's cube form) on device-resident cubes: a
JWST-like cube (3000 x 64 x 64) and a MUSE-like cube (3600 x 320 x 320, 1.47 GB).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of device time per call: HIP events on the stream around CALLS back-to-back calls, after one
warm-up round of every entry (global_stats reads its histograms back, so its events enclose the host's part of the descent too).
spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...), not one after the other.

traffic_floor_ms = the bytes the entry's pass list has to move over the measured copy rate (`python bench.py --full` reports it as
measured_copy_GBs; CUBE_COPY_GBS overrides the 6290 GB/s default, which is what a float4 copy reaches on this part):
    collapse_mean          1 read of the cube + the plane
    collapse_median        4 reads of the cube (one per 8-bit digit) + the plane
    global_stats (step s)  the sampled frames x (1 + 2 passes for the first rank's descent + 2 per further distinct prefix; reported
                           for the common case of three ranks in three different level-0 bins: 7) + 3 for the deviations' select
    normalize_frame        1 read + 1 write of the frame
    export_frames (step s) 2 reads of the sampled frames + their bytes
    extract_spectrum       one 64-byte sector per plane + depth * 4
CUBE_ONLY=jwst (or muse) restricts the run."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import astroburst_amd as ab  # noqa: E402

CALLS = int(os.environ.get("CUBE_CALLS", "5"))
SAMPLES = int(os.environ.get("CUBE_SAMPLES", "5"))
ONLY = os.environ.get("CUBE_ONLY")
COPY_RATE = float(os.environ.get("CUBE_COPY_GBS", "6290")) * 1e9


def sample(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / CALLS


def interleaved(entries):
    ts = {k: [] for k in entries}
    for rnd in range(SAMPLES + 1):
        for name, fn in entries.items():
            t = sample(fn)
            if rnd > 0:  # (round 0 warms every entry up)
                ts[name].append(t)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in ts.items()}


def main():
    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9}
    for label, (depth, rows, cols) in (("jwst", (3000, 64, 64)), ("muse", (3600, 320, 320))):
        if ONLY and ONLY != label:
            continue
        g = torch.Generator(device="cuda").manual_seed(21)
        cube = torch.randn((depth, rows, cols), device="cuda", generator=g)
        cube[torch.rand((depth, rows, cols), device="cuda", generator=g) < 0.03] = float("nan")   # IFU cubes carry NaN borders
        plane, voxels = rows * cols, depth * rows * cols
        step = ab.core.cube_streaming_step(depth)
        sampled = -(-depth // step)
        out_plane = torch.empty((rows, cols), device="cuda")
        out_bytes = torch.empty((depth, rows, cols), dtype=torch.uint8, device="cuda")
        out_bytes_s = torch.empty((-(-depth // 10), rows, cols), dtype=torch.uint8, device="cuda")
        out_spec = torch.empty((depth,), device="cuda")
        stats = ctx.compute_global_stats(cube)
        frame = cube[depth // 2]
        entries = {
            "collapse_mean": lambda: ctx.collapse_mean(cube, out=out_plane),
            "collapse_median": lambda: ctx.collapse_median(cube, out=out_plane),
            "global_stats_eager": lambda: ctx.compute_global_stats(cube),
            "global_stats_streaming": lambda: ctx.compute_global_stats_streaming(cube),
            "normalize_frame": lambda: ctx.normalize_with_global(frame, stats, out=out_plane),
            "export_frames_step1": lambda: ctx.export_cube_frames(cube, stats, 1, out=out_bytes),
            "export_frames_step10": lambda: ctx.export_cube_frames(cube, stats, 10, out=out_bytes_s),
            "extract_spectrum": lambda: ctx.extract_spectrum(cube, rows // 2, cols // 2, out=out_spec),
        }
        floor_bytes = {
            "collapse_mean": 4 * voxels + 4 * plane,
            "collapse_median": 4 * 4 * voxels + 4 * plane,
            "global_stats_eager": (7 + 3) * 4 * voxels,
            "global_stats_streaming": (7 + 3) * 4 * sampled * plane,
            "normalize_frame": 8 * plane,
            "export_frames_step1": (2 * 4 + 1) * voxels,
            "export_frames_step10": (2 * 4 + 1) * -(-depth // 10) * plane,
            "extract_spectrum": 64 * depth + 4 * depth,
        }
        entry = {"depth": depth, "rows": rows, "cols": cols, "cube_MB": round(4 * voxels / 1e6, 1), "streaming_step": step}
        for name, (ms, spread) in interleaved(entries).items():
            floor_ms = floor_bytes[name] / COPY_RATE * 1e3
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4), "traffic_floor_ms": round(floor_ms, 4),
                           "fraction_of_traffic_floor": round(floor_ms / ms, 4)}
        res[label] = entry
        del cube, out_bytes, out_bytes_s
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
