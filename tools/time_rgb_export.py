"""Developer tool: time the colour finish (csrc/rgb_export.hip) on device-resident planes: 4096 x 4096 and 13759 x 12451 (a full
mosaic, 685 MB per channel).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of device time per call: HIP events on the stream around CALLS back-to-back calls, after one
warm-up round of every entry.  spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...).

    render_rgb_*            the packer alone on three stretched planes (12 B read + 3 / 6 B written per pixel)
    render_rgb_stf_8 / _16  apply_stf_f32 x 3 + the packer in one launch: 15 / 18 B per pixel
    chain_unfused           the same picture through the entry points that existed before the fused kernel: ab_apply_stf_f32 x 3 (8 B per
                            pixel each), ab_apply_scnr_inplace (24 B), ab_render_rgb_preview at full size (12 + 3 B): 63 B per pixel
    process_drizzle_rgb     ab_process_drizzle_rgb whole, rgb8 output only: the statistics (read back, so the host's part is inside the
                            events), the white-balance launch and the finish launch
    statistics              ab_compute_image_stats x 3: what process_drizzle_rgb spends before its two launches when no channel is scaled
traffic_floor_ms = those bytes over the measured copy rate (RGBX_COPY_GBS overrides the 6290 GB/s a float4 copy reaches on this part).

The finish launch of process_drizzle_rgb WITHOUT its statistics has no entry point of its own; it is read from a kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_rgb_export.py
    python tools/time_rgb_export.py --kernels DIR
prints calls / median / min / max in microseconds per kernel of the finish and of the unfused chain.  Both image sizes launch the
capped grid, so trace one size at a time: RGBX_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("RGBX_CALLS", "5"))
SAMPLES = int(os.environ.get("RGBX_SAMPLES", "5"))
ONLY = os.environ.get("RGBX_ONLY")
COPY_RATE = float(os.environ.get("RGBX_COPY_GBS", "6290")) * 1e9
KERNELS = ("rgb_finish_kernel", "merge3_div_kernel", "stf_f32_kernel", "scnr_kernel", "preview_rgb_kernel")


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
        print(f"{short:44s} grid_x {grid:>9}  calls {len(v):4d}  median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f} us")


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

    def channel(rows, cols, seed, level):
        g = torch.Generator(device="cuda").manual_seed(seed)
        img = torch.randn((rows, cols), device="cuda", generator=g) * 0.01 + level
        stars = torch.rand((rows, cols), device="cuda", generator=g) < 5e-4
        img[stars] += torch.empty(int(stars.sum()), device="cuda").exponential_(4.0, generator=g)
        img[torch.rand((rows, cols), device="cuda", generator=g) < 0.01] = float("nan")
        return img

    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9}
    scnr = dict(method="average", amount=0.8, preserve_luminance=True)
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        planes = [channel(rows, cols, 40 + c, 0.10 + 0.02 * c) for c in range(3)]
        stats = [ctx.compute_image_stats(p) for p in planes]
        stf = [ctx.auto_stf(s) for s in stats]
        stretched = [ctx.apply_stf_f32(p, q, s) for p, q, s in zip(planes, stf, stats)]
        tmp = [torch.empty_like(p) for p in planes]
        out8 = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        out16 = torch.empty((rows, cols, 6), dtype=torch.uint8, device="cuda")

        def chain():
            for p, q, s, t in zip(planes, stf, stats, tmp):
                ctx.apply_stf_f32(p, q, s, out=t)
            ctx.apply_scnr_inplace(*tmp, **scnr)
            ctx.render_rgb_preview(*tmp, max(rows, cols))

        entries = {
            "render_rgb_u8": (lambda: ctx.render_rgb(*stretched, ab.RGB_PACK_8, out=out8), 15),
            "render_rgb_u8round": (lambda: ctx.render_rgb(*stretched, ab.RGB_PACK_8_ROUND, out=out8), 15),
            "render_rgb_u16be": (lambda: ctx.render_rgb(*stretched, ab.RGB_PACK_16BE, out=out16), 18),
            "render_rgb_stf_8": (lambda: ctx.render_rgb_stf(*planes, stf, stats, ab.RGB_PACK_8, out=out8), 15),
            "render_rgb_stf_16": (lambda: ctx.render_rgb_stf(*planes, stf, stats, ab.RGB_PACK_16BE, out=out16), 18),
            "chain_unfused": (chain, 63),
            "process_drizzle_rgb": (lambda: ctx.process_drizzle_rgb(*planes, white_balance="none", auto_stretch=True, linked_stf=False, scnr=scnr,
                                                                    want_stretched=False, want_wb=False), None),
            "statistics": (lambda: [ctx.compute_image_stats(p) for p in planes], None),
        }
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1)}
        for name, (ms, spread) in interleaved({k: v[0] for k, v in entries.items()}).items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
            per_px = entries[name][1]
            if per_px is not None:
                floor_ms = per_px * n / COPY_RATE * 1e3
                entry[name].update(bytes_per_pixel=per_px, traffic_floor_ms=round(floor_ms, 4), fraction_of_traffic_floor=round(floor_ms / ms, 4))
        res[label] = entry
        del planes, stretched, tmp, out8, out16
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--kernels":
        kernel_summary(sys.argv[2])
    else:
        main()
