"""Developer tool: time the compose wizard's background step (csrc/wizard_background.hip) against the chain of older entry points it
replaces, on device-resident planes: 4096 x 4096 and 13759 x 12451 (a full mosaic, 685 MB).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of the time per call: a host clock around CALLS back-to-back calls that ends in a device
synchronise, after one warm-up round of every entry.  spread_ms = max - min of the samples.  The entries are sampled in turn
(A B C A B C ...), fused and unfused in the same process.

    chain              ab_extract_background, ab_auto_stretch_preview of the corrected plane and of the model (every pixel to a byte),
                       the pick of both on the host side of the binding (a torch gather on the device): extract_background_cmd
    step               ab_background_step with device planes and device bytes
    step_no_model      the same with out_model NULL (the model lives in the context's workspace)
    extract            ab_extract_background alone
    preview_chain      ab_auto_stretch_preview + the pick, of the corrected plane
    preview_sampled    ab_auto_stretch_preview_sampled of it
    model_stats_scan   ab_compute_image_stats of the model: the statistics with their own range pass (the parent's handling)
    model_stats_known  ab_compute_image_stats_with_known_range of it with the range the surface kernel folds: what the folded range is
                       worth on its own is the difference of the two
All at grid 8, degree 3, max_dim = 4096 (MAX_PREVIEW_DIM, cmd/common.rs:16), as the command runs.
traffic_floor_ms = the bytes the fused call cannot avoid over the measured copy rate (BGSTEP_COPY_GBS overrides the 6290 GB/s a float4
copy reaches on this part): the image read by the two global selects (3 passes each) and once by the cell medians' windows (a
quarter of it), the model written, read by its median (3 passes), model and image read and the corrected plane written by the
correction, each plane read by its statistics (scan where there is one, histogram, MAD histogram: 3 and 2 passes above 4 000 000 px),
and the previews' picked 128-byte lines and bytes.  BGSTEP_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("BGSTEP_CALLS", "3"))
SAMPLES = int(os.environ.get("BGSTEP_SAMPLES", "5"))
ONLY = os.environ.get("BGSTEP_ONLY")
COPY_RATE = float(os.environ.get("BGSTEP_COPY_GBS", "6290")) * 1e9
PREVIEW = 4096   # MAX_PREVIEW_DIM (cmd/common.rs:16)
GRID, DEGREE = 8, 3


def main():
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

    def frame(rows, cols, seed):
        """sky on a gradient, sparse stars, 1 % NaN"""
        g = torch.Generator(device="cuda").manual_seed(seed)
        y = torch.linspace(-0.5, 0.5, rows, device="cuda")[:, None]
        x = torch.linspace(-0.5, 0.5, cols, device="cuda")[None, :]
        img = 300.0 + 80.0 * y - 40.0 * x + 35.0 * x * x + torch.randn((rows, cols), device="cuda", generator=g) * 3.0
        stars = torch.rand((rows, cols), device="cuda", generator=g) < 1e-3
        img[stars] += torch.rand(int(stars.sum()), device="cuda", generator=g) * 5000.0
        img[torch.rand((rows, cols), device="cuda", generator=g) < 0.01] = float("nan")
        return img.contiguous()

    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9, "max_dim": PREVIEW, "grid": GRID, "degree": DEGREE}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        img = frame(rows, cols, 90)
        corrected = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        model = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        ph, pw = ctx.preview_dims(rows, cols, PREVIEW)
        cu8 = torch.empty((ph, pw), dtype=torch.uint8, device="cuda")
        mu8 = torch.empty((ph, pw), dtype=torch.uint8, device="cuda")
        full = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        sampled = (ph, pw) != (rows, cols)
        sy = torch.clamp((torch.arange(ph, device="cuda", dtype=torch.float64) * (rows / ph)), max=float(rows - 1)).to(torch.int64)
        sx = torch.clamp((torch.arange(pw, device="cuda", dtype=torch.float64) * (cols / pw)), max=float(cols - 1)).to(torch.int64)
        kw = dict(grid_size=GRID, poly_degree=DEGREE)
        keep = [None]

        def pick(u8, out):
            if sampled:
                torch.index_select(u8.index_select(0, sy), 1, sx, out=out)
            else:
                out.copy_(u8)

        def preview_chain(plane, out):
            u8, st, stf = ctx.auto_stretch_preview(plane, out=full)
            pick(u8, out)
            return st

        def chain():
            bg = ctx.extract_background(img, **kw)
            keep[0] = (preview_chain(bg.corrected, cu8), preview_chain(bg.model, mu8))

        first = ctx.background_step(img, max_dim=PREVIEW, out_corrected=corrected, out_model=model, out_corrected_u8=cu8, out_model_u8=mu8, **kw)
        known = (first.model_stats.min, first.model_stats.max)
        entries = {
            "chain": chain,
            "step": lambda: ctx.background_step(img, max_dim=PREVIEW, out_corrected=corrected, out_model=model, out_corrected_u8=cu8, out_model_u8=mu8, **kw),
            "step_no_model": lambda: ctx.background_step(img, max_dim=PREVIEW, want_model=False, out_corrected=corrected, out_corrected_u8=cu8,
                                                         out_model_u8=mu8, **kw),
            "extract": lambda: ctx.extract_background(img, **kw),
            "preview_chain": lambda: preview_chain(corrected, cu8),
            "preview_sampled": lambda: ctx.auto_stretch_preview_sampled(corrected, max_dim=PREVIEW, out=cu8),
            "model_stats_scan": lambda: ctx.compute_image_stats(model),
            "model_stats_known": lambda: ctx.compute_image_stats_with_known_range(model, *known),
        }
        if sampled:
            lines_per_row = -(-cols * 4 // 128) if cols / pw < 32 else pw
            preview_bytes = ph * lines_per_row * 128 + ph * pw
        else:
            preview_bytes = 5 * n
        hist = n > 4_000_000
        passes = 6 * 4 + 1 + 4 + 3 * 4 + 12 + ((3 + 2) * 4 if hist else 2 * 4)   # selects, cells, model, its median, correction, two statistics
        floors = {"step": passes * n + 2 * preview_bytes, "step_no_model": passes * n + 2 * preview_bytes,
                  "preview_sampled": (3 if hist else 1) * 4 * n + preview_bytes}
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "preview": [ph, pw]}
        for name, (ms, spread) in interleaved(entries).items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
            if name in floors:
                entry[name]["traffic_floor_ms"] = round(floors[name] / COPY_RATE * 1e3, 4)
        for step, ch in (("step", "chain"), ("step_no_model", "chain"), ("preview_sampled", "preview_chain")):
            entry[f"{step}_over_chain"] = round(entry[ch]["call_ms"] / entry[step]["call_ms"], 2)
        entry["folded_range_ms"] = round(entry["model_stats_scan"]["call_ms"] - entry["model_stats_known"]["call_ms"], 4)
        res[label] = entry
        del img, corrected, model, cu8, mu8, full
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
