"""Developer tool: time the compose wizard's crop step (csrc/crop.hip) on device-resident planes: 4096 x 4096 and 13759 x 12451 (a full
mosaic, 685 MB per channel).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of device time per call: HIP events on the stream around CALLS back-to-back calls, after one
warm-up round of every entry.  spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...).  The planes
are noise inside a zero border of about 1 % per side, what the warp leaves around a registered channel.

    detect_one              ab_detect_valid_region of one plane: 4 B read per pixel; the call ends in the four-word read-back and a
                            synchronise, both inside the events
    detect_three            ab_detect_valid_regions of three planes in one launch: 12 B per pixel of one plane
    crop_90                 ab_crop_array of the centred 90 % x 90 % window: 8 B per OUTPUT pixel
    crop_channels           ab_crop_channels of three planes to the detected box, stats = NULL: one launch, 24 B per output pixel
    crop_channels_stats     the same with the statistics of the three cropped planes (read back: the host's part is inside the events)
    statistics              ab_compute_image_stats x 3 of the cropped planes: what crop_channels_stats adds
traffic_floor_ms = those bytes over the measured copy rate (CROP_COPY_GBS overrides the 6290 GB/s a float4 copy reaches on this part).
CROP_ONLY=4096 (or mosaic) restricts the run.

The detection calls end in a read-back and a synchronise, so their call time holds a fixed host round trip; the kernels alone are read
from a kernel trace, one size at a time (both sizes launch the capped grid):
    CROP_ONLY=4096 rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_crop.py
    python tools/time_crop.py --kernels DIR
prints calls / median / min / max in microseconds per kernel and grid size."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("CROP_CALLS", "5"))
SAMPLES = int(os.environ.get("CROP_SAMPLES", "5"))
ONLY = os.environ.get("CROP_ONLY")
COPY_RATE = float(os.environ.get("CROP_COPY_GBS", "6290")) * 1e9
KERNELS = ("bbox_init_kernel", "bbox_kernel", "crop_kernel")


def kernel_summary(directory):
    import csv
    import glob
    from collections import defaultdict
    per = defaultdict(list)
    for f in glob.glob(directory + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if not any(k in name for k in KERNELS):
                continue
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            per[(short, r.get("Grid_Size_X", r.get("Grid_Size", "?")))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (short, grid), v in sorted(per.items()):
        print(f"{short:24s} grid_x {grid:>9}  calls {len(v):4d}  median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f} us")


def main():
    import torch

    import astroburst_amd as ab

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

    def channel(rows, cols, seed, border):
        g = torch.Generator(device="cuda").manual_seed(seed)
        img = torch.zeros((rows, cols), device="cuda")
        t, b, l, r = border
        img[t:rows - b, l:cols - r] = torch.rand((rows - t - b, cols - l - r), device="cuda", generator=g) * 0.9 + 0.05
        return img

    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        e = max(rows, cols) // 100
        planes = [channel(rows, cols, 40 + c, (e + c, e // 2, e - c, e + 2 * c)) for c in range(3)]
        plan = ctx.crop_channels_plan(planes)
        outs = [torch.empty(d, dtype=torch.float32, device="cuda") for d in plan.out_dims]
        out_px = sum(d[0] * d[1] for d in plan.out_dims)
        win = ab.CropBox(rows // 20, rows - rows // 20, cols // 20, cols - cols // 20)
        win_out = torch.empty((win.bottom - win.top, win.right - win.left), dtype=torch.float32, device="cuda")
        entries = {
            "detect_one": (lambda: ctx.detect_valid_region(planes[0]), 4 * n),
            "detect_three": (lambda: ctx.detect_valid_regions(planes), 12 * n),
            "crop_90": (lambda: ctx.crop_array(planes[0], win, out=win_out), 8 * win_out.numel()),
            "crop_channels": (lambda: ctx.crop_channels(planes, plan, want_stats=False, outs=outs), 8 * out_px),
            "crop_channels_stats": (lambda: ctx.crop_channels(planes, plan, want_stats=True, outs=outs), None),
            "statistics": (lambda: [ctx.compute_image_stats(o) for o in outs], None),
        }
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "box": list(plan.crop_box), "window_90": list(win)}
        for name, (ms, spread) in interleaved({k: v[0] for k, v in entries.items()}).items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
            nbytes = entries[name][1]
            if nbytes is not None:
                floor_ms = nbytes / COPY_RATE * 1e3
                entry[name].update(bytes=nbytes, traffic_floor_ms=round(floor_ms, 4), fraction_of_traffic_floor=round(floor_ms / ms, 4))
        res[label] = entry
        del planes, outs, win_out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--kernels":
        kernel_summary(sys.argv[2])
    else:
        main()
