"""Developer tool: time the compose wizard's tone preview (csrc/tone.hip) on device-resident planes: 4096 x 4096 and 13759 x 12451 (a
full mosaic, 685 MB per channel).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of device time per call: HIP events on the stream around CALLS back-to-back calls, after one
warm-up round of every entry.  spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...).

    chain_unfused     the command through the entry points that existed before the fused kernel: ab_apply_stf_f32 x 3 (8 B per pixel
                      each), ab_apply_levels x 3 (8 B), ab_apply_curve x 3 (8 B; each uploads its LUT and waits for it), ab_apply_scnr_inplace
                      (24 B), ab_render_rgb_preview (12 + 3 B at full size): 108 B per pixel, eleven launches
    fused_full        ab_apply_tone_composite, bytes only, max_dim = the longer side: one launch, 12 B read + 3 B written per pixel
    fused_sampled     the same at max_dim 4096 (the mosaic only): one launch over the 4096 x 3707 pixels the preview picks; its traffic
                      floor is the 128-byte lines those pixels lie in (every line of a picked row while the column ratio is below 32
                      floats) plus the bytes written
    fused_no_levels   fused_full without the levels stage (no f64 pow): what the three pow per pixel cost
    fused_stf_only    fused_full with the STF alone: ab_render_rgb_stf's work through this kernel
traffic_floor_ms = those bytes over the measured copy rate (TONE_COPY_GBS overrides the 6290 GB/s a float4 copy reaches on this part).
TONE_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("TONE_CALLS", "5"))
SAMPLES = int(os.environ.get("TONE_SAMPLES", "5"))
ONLY = os.environ.get("TONE_ONLY")
COPY_RATE = float(os.environ.get("TONE_COPY_GBS", "6290")) * 1e9
PREVIEW = 4096   # MAX_PREVIEW_DIM (cmd/common.rs)
S_CURVE = [(0.0, 0.0), (0.25, 0.15), (0.5, 0.5), (0.75, 0.85), (1.0, 1.0)]


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
    levels = ((0.02, 1.6, 0.95), (0.0, 1.3, 1.0), (0.01, 0.8, 0.9))
    curves = (S_CURVE, None, S_CURVE)
    scnr = dict(method="average", amount=0.8, preserve_luminance=True)
    tone = dict(levels=levels, curves=curves, scnr=scnr)
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        planes = [channel(rows, cols, 40 + c, 0.10 + 0.02 * c) for c in range(3)]
        stats = [ctx.compute_image_stats(p) for p in planes]
        info, luts = ctx.tone_plan(stats, **tone)
        t1 = [torch.empty_like(p) for p in planes]
        t2 = [torch.empty_like(p) for p in planes]
        full_dim = max(rows, cols)
        out_full = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        ph, pw = ctx.preview_dims(rows, cols, PREVIEW)
        out_small = torch.empty((ph, pw, 3), dtype=torch.uint8, device="cuda")

        def chain():
            for c in range(3):
                ctx.apply_stf_f32(planes[c], info.stf[c], info.norm[c], out=t1[c])
            for c in range(3):
                ctx.apply_levels(t1[c], *levels[c], out=t2[c])
            for c in range(3):
                ctx.apply_curve(t2[c], luts[c], out=t1[c])
            ctx.apply_scnr_inplace(*t1, **scnr)
            ctx.render_rgb_preview(*t1, full_dim, out=out_full)

        entries = {
            "chain_unfused": (chain, 108 * n),
            "fused_full": (lambda: ctx.apply_tone_composite(*planes, stats, max_dim=full_dim, out=out_full, **tone), 15 * n),
            "fused_no_levels": (lambda: ctx.apply_tone_composite(*planes, stats, max_dim=full_dim, out=out_full, curves=curves, scnr=scnr), 15 * n),
            "fused_stf_only": (lambda: ctx.apply_tone_composite(*planes, stats, max_dim=full_dim, out=out_full), 15 * n),
        }
        if (ph, pw) != (rows, cols):
            lines_per_row = -(-cols * 4 // 128) if cols / pw < 32 else pw
            touched = 3 * ph * lines_per_row * 128 + 3 * ph * pw
            entries["fused_sampled"] = (lambda: ctx.apply_tone_composite(*planes, stats, max_dim=PREVIEW, out=out_small, **tone), touched)
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "preview": [ph, pw]}
        for name, (ms, spread) in interleaved({k: v[0] for k, v in entries.items()}).items():
            nbytes = entries[name][1]
            floor_ms = nbytes / COPY_RATE * 1e3
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4), "bytes": nbytes, "traffic_floor_ms": round(floor_ms, 4),
                           "fraction_of_traffic_floor": round(floor_ms / ms, 4)}
        entry["fused_full_over_chain"] = round(entry["chain_unfused"]["call_ms"] / entry["fused_full"]["call_ms"], 2)
        if "fused_sampled" in entry:
            entry["sampled_over_fused_full"] = round(entry["fused_full"]["call_ms"] / entry["fused_sampled"]["call_ms"], 2)
        res[label] = entry
        del planes, t1, t2, out_full, out_small
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
