"""Developer tool: time the compose wizard's stretch step (csrc/wizard_stretch.hip) against the chains of older entry points it replaces,
on device-resident planes: 4096 x 4096 and 13759 x 12451 (a full mosaic, 685 MB per channel).  One JSON line.  Run it in a fresh
process.

call_ms = median over SAMPLES samples of the time per call: a host clock around CALLS back-to-back calls that ends in a device
synchronise, after one warm-up round of every entry.  spread_ms = max - min of the samples.  The entries are sampled in turn
(A B C A B C ...), fused and unfused in the same process.

    composite_chain         ab_compute_image_stats x 3 (a median and MAD chain and a synchronisation each), ab_arcsinh_rgb_range on the
                            host, ab_arcsinh_stretch_with_stats x 3, ab_render_rgb_preview(stf NULL): arcsinh_stretch_composite_cmd
    composite_step          ab_arcsinh_stretch_composite without planes (what the command keeps): the range pass, then the picked pixels
    composite_step_cached   the same with global_min / global_max given (cached statistics): no range pass
    composite_step_planes   the same with out_planes: the range pass, then one kernel for planes and bytes
    rgb_chain / rgb_step    the planes alone: the first two stages of the chain against ab_arcsinh_stretch_rgb
    view_chain / view_step  ab_compute_image_stats, ab_arcsinh_stretch_with_stats, ab_auto_stretch_preview against ab_arcsinh_stretch_view
    masked_<m>_chain/_step  ab_masked_stretch_rgb_shared (m = shared) or ab_masked_stretch x 3 (m = each), ab_render_rgb_preview(stf NULL)
                            against ab_masked_stretch_composite without planes; STRETCH_MASKED=0 leaves them out
All at max_dim = 4096 (MAX_PREVIEW_DIM, cmd/common.rs:16), as the commands run; factor 20.  The chains' intermediate planes come from
torch's caching allocator; the fused calls write into planes allocated once.
traffic_floor_ms = the bytes the fused call cannot avoid over the measured copy rate (STRETCH_COPY_GBS overrides the 6290 GB/s a float4
copy reaches on this part): 12 B per pixel for the range pass, 24 B more with planes, and the preview's picked 128-byte lines and its
bytes (every pixel once and 3 B when the image fits max_dim).  STRETCH_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("STRETCH_CALLS", "3"))
SAMPLES = int(os.environ.get("STRETCH_SAMPLES", "5"))
ONLY = os.environ.get("STRETCH_ONLY")
MASKED = os.environ.get("STRETCH_MASKED", "1") != "0"
COPY_RATE = float(os.environ.get("STRETCH_COPY_GBS", "6290")) * 1e9
PREVIEW = 4096   # MAX_PREVIEW_DIM (cmd/common.rs:16)
FACTOR = 20.0


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
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9, "max_dim": PREVIEW, "factor": FACTOR}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        planes = [channel(rows, cols, 70 + c, 0.2 + 0.1 * c) for c in range(3)]
        outs = [torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3)]
        ph, pw = ctx.preview_dims(rows, cols, PREVIEW)
        rgb8 = torch.empty((ph, pw, 3), dtype=torch.uint8, device="cuda")
        u8 = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        cached = ab.arcsinh_rgb_range(*[ctx.compute_image_stats(p) for p in planes])
        f32 = float(np.float32(FACTOR))
        keep = [None]

        def stretched_chain():
            gmin, gmax = ab.arcsinh_rgb_range(*[ctx.compute_image_stats(p) for p in planes])
            return [ctx.arcsinh_stretch_with_stats(p, gmin, gmax, f32, 1.0) for p in planes]

        def composite_chain():
            ctx.render_rgb_preview(*stretched_chain(), PREVIEW, out=rgb8)

        def rgb_chain():
            keep[0] = stretched_chain()

        def view_chain():
            st = ctx.compute_image_stats(planes[0])
            plane = ctx.arcsinh_stretch_with_stats(planes[0], float(np.float32(st.min)), float(np.float32(st.max)), f32, 1.0)
            keep[0] = ctx.auto_stretch_preview(plane, out=u8)

        def masked_chain(shared):
            if shared:
                stretched = [r.image for r in ctx.masked_stretch_rgb_shared(*planes)[:3]]
            else:
                stretched = [ctx.masked_stretch(p).image for p in planes]
            ctx.render_rgb_preview(*stretched, PREVIEW, out=rgb8)

        entries = {
            "composite_chain": composite_chain,
            "composite_step": lambda: ctx.arcsinh_stretch_composite(*planes, FACTOR, max_dim=PREVIEW, out=rgb8),
            "composite_step_cached": lambda: ctx.arcsinh_stretch_composite(*planes, FACTOR, max_dim=PREVIEW, global_range=cached, out=rgb8),
            "composite_step_planes": lambda: ctx.arcsinh_stretch_composite(*planes, FACTOR, max_dim=PREVIEW, out=rgb8, out_planes=outs),
            "rgb_chain": rgb_chain,
            "rgb_step": lambda: ctx.arcsinh_stretch_rgb(*planes, f32, out_planes=outs),
            "view_chain": view_chain,
            "view_step": lambda: ctx.arcsinh_stretch_view(planes[0], FACTOR, out=u8, out_plane=outs[0]),
        }
        if MASKED:
            for key, shared in (("shared", True), ("each", False)):
                entries[f"masked_{key}_chain"] = (lambda s=shared: masked_chain(s))
                entries[f"masked_{key}_step"] = (lambda s=shared: ctx.masked_stretch_composite(*planes, shared_mask=s, max_dim=PREVIEW, out=rgb8))

        if (ph, pw) != (rows, cols):
            lines_per_row = -(-cols * 4 // 128) if cols / pw < 32 else pw
            preview_bytes = 3 * ph * lines_per_row * 128 + 3 * ph * pw
        else:
            preview_bytes = 15 * n
        floors = {"composite_step": 12 * n + preview_bytes, "composite_step_cached": preview_bytes,
                  "composite_step_planes": 12 * n + 24 * n + (3 * ph * pw if (ph, pw) == (rows, cols) else preview_bytes), "rgb_step": 12 * n + 24 * n}
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "preview": [ph, pw]}
        for name, (ms, spread) in interleaved(entries).items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
            if name in floors:
                entry[name]["traffic_floor_ms"] = round(floors[name] / COPY_RATE * 1e3, 4)
        for step, chain in (("composite_step", "composite_chain"), ("composite_step_cached", "composite_chain"), ("composite_step_planes", "composite_chain"),
                            ("rgb_step", "rgb_chain"), ("view_step", "view_chain"), ("masked_shared_step", "masked_shared_chain"),
                            ("masked_each_step", "masked_each_chain")):
            if step in entry:
                entry[f"{step}_over_chain"] = round(entry[chain]["call_ms"] / entry[step]["call_ms"], 2)
        res[label] = entry
        del planes, outs, rgb8, u8
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
