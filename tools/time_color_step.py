"""Developer tool: time the compose wizard's colour and blend steps (csrc/wizard_color.hip) against the chains of older entry points they
replace, on device-resident planes: 4096 x 4096 and 13759 x 12451 (a full mosaic, 685 MB per channel).  One JSON line.  Run it in a
fresh process.

call_ms = median over SAMPLES samples of the time per call: a host clock around CALLS back-to-back calls that ends in a device
synchronise (every entry synchronises by itself as well: it returns the statistics), after one warm-up round of every entry.
spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...), fused and unfused in the same process.

    color_chain_<s>   ab_calibrate_channel x 3 (a scale kernel, a statistics chain and a synchronisation each), ab_apply_scnr_inplace,
                      ab_compute_image_stats of G (SCNR) or of all three (SCNR + preserve_luminance), ab_compute_linked_stf on the host,
                      ab_render_rgb_preview(stf x 3, stats): calibrate_and_scnr_cmd as INTEGRATION.md had it
    color_step_<s>    ab_calibrate_and_scnr: one chain, one synchronisation
  <s> = none (no SCNR), scnr (average neutral, amount 0.8), preserve (maximum neutral, amount 1, preserve_luminance)
    blend_chain       ab_blend_channels (three channels, nine weights), ab_compute_image_stats x 3, ab_compute_linked_stf,
                      ab_render_rgb_preview(stf x 3, stats)
    blend_step        ab_blend_composite
All at max_dim = 4096 (MAX_PREVIEW_DIM, cmd/common.rs:16), as the commands run.  The chains' intermediate planes come from torch's
caching allocator (three torch.empty per call, microseconds); the fused calls write into planes allocated once.
traffic_floor_ms = the bytes the fused call cannot avoid over the measured copy rate (COLOR_COPY_GBS overrides the 6290 GB/s a float4
copy reaches on this part): 24 B per pixel for the planes' kernel (blend: 12 B read for three channels, 12 B written), ONE read of each
final plane for its statistics chain (it makes several), and the preview's picked lines and bytes.  COLOR_ONLY=4096 (or mosaic)
restricts the run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("COLOR_CALLS", "3"))
SAMPLES = int(os.environ.get("COLOR_SAMPLES", "5"))
ONLY = os.environ.get("COLOR_ONLY")
COPY_RATE = float(os.environ.get("COLOR_COPY_GBS", "6290")) * 1e9
PREVIEW = 4096   # MAX_PREVIEW_DIM (cmd/common.rs:16)
FACTORS = (1.7, 0.6, 1.25)
SCNR = {"none": None, "scnr": dict(method="average", amount=0.8), "preserve": dict(method="maximum", amount=1.0, preserve_luminance=True)}
WEIGHTS = [(0, 1.0, 0.1, 0.0), (1, 0.2, 1.0, 0.1), (2, 0.0, 0.15, 1.0)]


def main():
    import numpy as np
    import torch

    import astroburst_amd as ab

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    def interleaved(entries):
        ts = {k: [] for k in entries}
        for rnd in range(SAMPLES + 1):
            for name, fn in entries.items():
                t = sample(fn)
                if rnd > 0:  # (round 0 warms every entry up)
                    ts[name].append(t)
        return {k: (statistics.median(v), max(v) - min(v)) for k, v in ts.items()}

    def channel(rows, cols, seed, level):
        """a composite's channel: sky around `level`, stars up to a few times 1, 1 % NaN"""
        g = torch.Generator(device="cuda").manual_seed(seed)
        img = torch.randn((rows, cols), device="cuda", generator=g) * 0.01 + level
        stars = torch.rand((rows, cols), device="cuda", generator=g) < 1e-3
        img[stars] += torch.rand(int(stars.sum()), device="cuda", generator=g) * 3.0
        img[torch.rand((rows, cols), device="cuda", generator=g) < 0.01] = float("nan")
        return img

    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9, "max_dim": PREVIEW}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        planes = [channel(rows, cols, 70 + c, 0.2 + 0.1 * c) for c in range(3)]
        orig_stats = [ctx.compute_image_stats(p) for p in planes]
        outs = [torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3)]
        ph, pw = ctx.preview_dims(rows, cols, PREVIEW)
        rgb8 = torch.empty((ph, pw, 3), dtype=torch.uint8, device="cuda")
        keep = [None]

        def color_chain(scnr):
            f32 = [float(np.float32(f)) for f in FACTORS]
            scaled, stats = [], []
            for p, f, s in zip(planes, f32, orig_stats):
                o, st = ctx.calibrate_channel(p, f, s)
                scaled.append(o), stats.append(st)
            if scnr is not None:
                ctx.apply_scnr_inplace(*scaled, method=scnr["method"], amount=scnr["amount"], preserve_luminance=scnr.get("preserve_luminance", False))
                if scnr.get("preserve_luminance", False):
                    stats = [ctx.compute_image_stats(o) for o in scaled]
                else:
                    stats[1] = ctx.compute_image_stats(scaled[1])
            linked, _ = ctx.compute_linked_stf(*stats)
            ctx.render_rgb_preview(*scaled, PREVIEW, stf=[linked] * 3, stats=stats, out=rgb8)
            keep[0] = linked

        def color_step(scnr):
            keep[0] = ctx.calibrate_and_scnr(*planes, orig_stats, FACTORS, scnr, max_dim=PREVIEW, out=rgb8, out_planes=outs).stf

        def blend_chain():
            blended = ctx.blend_channels(planes, WEIGHTS, rows, cols)
            stats = [ctx.compute_image_stats(o) for o in blended]
            linked, _ = ctx.compute_linked_stf(*stats)
            ctx.render_rgb_preview(*blended, PREVIEW, stf=[linked] * 3, stats=stats, out=rgb8)
            keep[0] = linked

        def blend_step():
            keep[0] = ctx.blend_composite(planes, WEIGHTS, max_dim=PREVIEW, out=rgb8, out_planes=outs).stf

        if (ph, pw) != (rows, cols):
            lines_per_row = -(-cols * 4 // 128) if cols / pw < 32 else pw
            preview_bytes = 3 * ph * lines_per_row * 128 + 3 * ph * pw
        else:
            preview_bytes = 15 * n
        floor = 24 * n + 12 * n + preview_bytes
        entries = {}
        for key, scnr in SCNR.items():
            entries[f"color_chain_{key}"] = (lambda s=scnr: color_chain(s))
            entries[f"color_step_{key}"] = (lambda s=scnr: color_step(s))
        entries["blend_chain"] = blend_chain
        entries["blend_step"] = blend_step
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "preview": [ph, pw], "floor_bytes": floor,
                 "traffic_floor_ms": round(floor / COPY_RATE * 1e3, 4)}
        for name, (ms, spread) in interleaved(entries).items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
            if "_step" in name:
                entry[name]["fraction_of_traffic_floor"] = round(floor / COPY_RATE * 1e3 / ms, 4)
        for key in SCNR:
            entry[f"color_step_{key}_over_chain"] = round(entry[f"color_chain_{key}"]["call_ms"] / entry[f"color_step_{key}"]["call_ms"], 2)
        entry["blend_step_over_chain"] = round(entry["blend_chain"]["call_ms"] / entry["blend_step"]["call_ms"], 2)
        res[label] = entry
        del planes, outs, rgb8
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
