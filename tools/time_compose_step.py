"""Developer tool: time the RGB Compose panel's fused calls (csrc/compose_step.hip: ab_compose_rgb; tone.hip: ab_restretch_composite)
against the chains of older entry points they replace, on device-resident planes: 4096 x 4096 and 13759 x 12451 (a full mosaic,
685 MB per plane).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of the time per call: a host clock around CALLS back-to-back calls that ends in a device
synchronise, after one warm-up round of every entry.  spread_ms = max - min of the samples.  The entries are sampled in turn
(A B C A B C ...), fused and unfused in the same process.

Per alignment case (off, phase correlation) and configuration
    plain    unlinked auto-STF, no L, no SCNR
    full     linked auto-STF, L at three quarters of the dims, SCNR average with preserve_luminance
the entries
    chain            ab_process_rgb (with the pre-stretch planes), then for `full` ab_resample_image, ab_compute_image_stats,
                     ab_auto_stf, ab_apply_stf_f32 and ab_apply_lrgb, then ab_render_rgb_preview: compose_rgb_cmd
    fused            ab_compose_rgb with device planes, device bytes and info, out_planes NULL
    fused_planes     the same with out_planes
and, once per size,
    restretch_chain  ab_apply_stf_f32 x 3 + ab_apply_scnr_inplace + ab_render_rgb_preview: restretch_composite_cmd
    restretch        ab_restretch_composite without planes
All at max_dim = 4096 (MAX_PREVIEW_DIM, cmd/common.rs:16), white balance auto, as the command runs.
The two sides are not allocated alike: the fused entries write into planes and bytes allocated once, while the chain's Python methods
allocate their outputs on every call (process_rgb's six planes have no `out=`; resample_image and apply_stf_f32 one plane each)
through torch's caching allocator, which serves them from its pool without a device allocation after the warm-up round.  That is
microseconds of host time per call against milliseconds, but it does tilt toward the fused side.
traffic_floor_ms = the bytes the fused call's pass list cannot avoid over the measured copy rate (COMPOSE_COPY_GBS overrides the
6290 GB/s a float4 copy reaches on this part), alignment off: each channel copied into its pre-stretch plane (8 B per pixel), one
statistics chain per channel before white balance and one per scaled channel, combined plane and L after it (2 passes of 4 B up to
4 000 000 pixels, 3 + 2 above), the white-balance launch (8 B per scaled channel, 4 B per channel it only reads, 4 B for the combined
plane), L's resample (its own size read, the composite's written), and the finish: 12 B (16 with L) read, 12 B written with planes,
3 B of bytes -- or, above max_dim without planes, only the picked 128-byte lines and the preview's bytes.  Two channels are taken as
scaled (white balance auto keeps the reference channel).  COMPOSE_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("COMPOSE_CALLS", "2"))
SAMPLES = int(os.environ.get("COMPOSE_SAMPLES", "5"))
ONLY = os.environ.get("COMPOSE_ONLY")
COPY_RATE = float(os.environ.get("COMPOSE_COPY_GBS", "6290")) * 1e9
PREVIEW = 4096   # MAX_PREVIEW_DIM (cmd/common.rs:16)
SCNR = dict(method="average", amount=0.8, preserve_luminance=True)
CONFIGS = {"plain": dict(kw=dict(), l=False), "full": dict(kw=dict(linked_stf=True, scnr=SCNR), l=True)}


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

    def frame(rows, cols, seed, scale, roll):
        """a smooth sky with structure for the phase correlation, sparse stars, the same scene rolled by a few pixels per channel"""
        g = torch.Generator(device="cuda").manual_seed(7)
        y = torch.linspace(-0.5, 0.5, rows, device="cuda")[:, None]
        x = torch.linspace(-0.5, 0.5, cols, device="cuda")[None, :]
        img = 0.05 + 0.02 * y - 0.01 * x + 0.01 * torch.sin(40.0 * x) * torch.cos(31.0 * y)
        stars = torch.rand((rows, cols), device="cuda", generator=g) < 1e-3
        img[stars] += torch.rand(int(stars.sum()), device="cuda", generator=g) * 0.8
        img = torch.roll(img, roll, (0, 1)) * scale
        g2 = torch.Generator(device="cuda").manual_seed(seed)
        return (img + torch.randn((rows, cols), device="cuda", generator=g2) * 0.002).float().contiguous()

    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9, "max_dim": PREVIEW}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        r = frame(rows, cols, 1, 1.0, (0, 0))
        g = frame(rows, cols, 2, 0.8, (2, -3))
        b = frame(rows, cols, 3, 1.3, (-1, 2))
        lr, lc = rows * 3 // 4, cols * 3 // 4
        l = frame(lr, lc, 4, 1.6, (0, 0))
        pre = tuple(torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3))
        planes = tuple(torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3))
        ph, pw = ctx.preview_dims(rows, cols, PREVIEW)
        by = torch.empty((ph, pw, 3), dtype=torch.uint8, device="cuda")
        sampled = (ph, pw) != (rows, cols)
        hist = n > 4_000_000
        chain_pass = (5 if hist else 2) * 4
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "preview": [ph, pw], "l_dims": [lr, lc]}

        def picked(n_planes):
            lines_per_row = -(-cols * 4 // 128) if cols / pw < 32 else pw
            return n_planes * ph * lines_per_row * 128 + 3 * ph * pw

        def floor(cfg, with_planes):
            has_l, linked = cfg["l"], bool(cfg["kw"].get("linked_stf"))
            t = 3 * 8 * n + 3 * chain_pass * n                       # the copies into out_pre, the statistics before white balance
            t += 2 * 8 * n + (4 * n + 4 * n if linked else 0)        # the white-balance launch
            t += (2 + linked + has_l) * chain_pass * n               # the statistics after it
            t += (4 * lr * lc + 4 * n) if has_l else 0               # L's resample
            src = 3 + has_l
            if with_planes:
                t += 4 * src * n + 12 * n + (picked(3) if sampled else 3 * n)
            else:
                t += picked(src) if sampled else 4 * src * n + 3 * n
            return t

        for align_label, align_kw in (("align_off", dict(align=False)), ("phase", dict(align=True, align_method="phase_correlation"))):
            for cfg_label, cfg in CONFIGS.items():
                kw = dict(cfg["kw"], **align_kw)
                lp = l if cfg["l"] else None

                def chain(kw=kw, lp=lp):
                    p = ctx.process_rgb(r, g, b, **kw)
                    if lp is not None:
                        lm = ctx.resample_image(lp, rows, cols)
                        st = ctx.compute_image_stats(lm)
                        stf = ctx.auto_stf(st)
                        lm = ctx.apply_stf_f32(lm, stf, st)
                        ctx.apply_lrgb(lm, p.r, p.g, p.b, 1.0, 1.0)
                    ctx.render_rgb_preview(p.r, p.g, p.b, PREVIEW, out=by)

                entries = {
                    "chain": chain,
                    "fused": lambda kw=kw, lp=lp: ctx.compose_rgb(lp, r, g, b, max_dim=PREVIEW, out_pre=pre, out=by, **kw),
                    "fused_planes": lambda kw=kw, lp=lp: ctx.compose_rgb(lp, r, g, b, max_dim=PREVIEW, out_pre=pre, out_planes=planes, out=by, **kw),
                }
                sub = {}
                for name, (ms, spread) in interleaved(entries).items():
                    sub[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
                for name, with_planes in (("fused", False), ("fused_planes", True)):
                    sub[f"{name}_over_chain"] = round(sub["chain"]["call_ms"] / sub[name]["call_ms"], 2)
                    if not align_kw["align"]:
                        sub[name]["traffic_floor_ms"] = round(floor(cfg, with_planes) / COPY_RATE * 1e3, 4)
                entry[f"{align_label}_{cfg_label}"] = sub

        # the STF slider loop over the composite the panel caches
        first = ctx.compose_rgb(None, r, g, b, max_dim=PREVIEW, out_pre=pre, out=by, align=False)
        stats, stf = list(first.stats_wb), list(first.stf)
        tmp = tuple(torch.empty((rows, cols), dtype=torch.float32, device="cuda") for _ in range(3))

        def restretch_chain():
            for src, dst, p, s in zip(pre, tmp, stf, stats):
                ctx.apply_stf_f32(src, p, s, out=dst)
            ctx.apply_scnr_inplace(*tmp, **SCNR)
            ctx.render_rgb_preview(*tmp, PREVIEW, out=by)

        entries = {"restretch_chain": restretch_chain,
                   "restretch": lambda: ctx.restretch_composite(*pre, stats, stf, scnr=SCNR, max_dim=PREVIEW, out=by)}
        for name, (ms, spread) in interleaved(entries).items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
        entry["restretch"]["traffic_floor_ms"] = round((picked(3) if sampled else 15 * n) / COPY_RATE * 1e3, 4)
        entry["restretch_over_chain"] = round(entry["restretch_chain"]["call_ms"] / entry["restretch"]["call_ms"], 2)
        res[label] = entry
        del r, g, b, l, pre, planes, tmp, by
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
