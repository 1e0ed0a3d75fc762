"""Developer tool: time the open-file view (csrc/view.hip) against the chains it replaces, on device-resident planes: 4096 x 4096 and
13759 x 12451 (a full mosaic, 685 MB per channel).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of the time per call: a host clock around CALLS back-to-back calls that ends in a device
synchronise (half of the entries synchronise by themselves: they return scalars or host bins), after one warm-up round of every
entry.  spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...).

    hist_unfused       ab_build_histogram(65536) -- one global atomic per pixel, 256 KiB to the host -- and the host fold to 512
    display_histogram  ab_display_histogram(512): the display bins in LDS, 2 KiB to the host.  Floor: 4 B per pixel
    mono_chain         ab_auto_stretch_preview (statistics, auto_stf, apply_stf; one synchronisation) + hist_unfused (another)
    mono_view          ab_process_fits_view(512): one chain, one synchronisation.  Floor: one read for the statistics + 5 B
    rgb_chain          ab_compute_image_stats x 3 + ab_apply_tone_composite (default configuration) + hist_unfused of R
    rgb_view           ab_process_rgb_fits_view(512): one chain, one synchronisation.  Floor: one read per channel + 15 B
both rgb entries at max_dim = the longer side (every pixel packed); the mosaic also at max_dim 4096 (rgb_chain_4096, rgb_view_4096: the
preview picks 4096 x 3707 pixels; floor: one read per channel, the 128-byte lines the picked pixels lie in, the bytes written, and
4 B per pixel for R's histogram pass).
The floors count a statistics chain as ONE read of its plane -- it makes several -- so a view's fraction of its floor says how far the
whole command is from a single streaming pass, not how good its last kernel is (rocprofv3 --kernel-trace gives that kernel alone).
traffic_floor_ms = those bytes over the measured copy rate (VIEW_COPY_GBS overrides the 6290 GB/s a float4 copy reaches on this part).
VIEW_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = int(os.environ.get("VIEW_CALLS", "3"))
SAMPLES = int(os.environ.get("VIEW_SAMPLES", "5"))
ONLY = os.environ.get("VIEW_ONLY")
COPY_RATE = float(os.environ.get("VIEW_COPY_GBS", "6290")) * 1e9
PREVIEW = 4096   # MAX_PREVIEW_DIM (cmd/common.rs:16)
BINS = 512       # HISTOGRAM_BINS_DISPLAY (types/constants.rs:9)


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

    def channel(rows, cols, seed, level):
        """a sky frame: background in two or three of the 512 display bins, stars up to the full well, 1 % NaN"""
        g = torch.Generator(device="cuda").manual_seed(seed)
        img = torch.randn((rows, cols), device="cuda", generator=g) * 30.0 + level
        stars = torch.rand((rows, cols), device="cuda", generator=g) < 1e-3
        img[stars] += torch.rand(int(stars.sum()), device="cuda", generator=g) * 60000.0
        img[torch.rand((rows, cols), device="cuda", generator=g) < 0.01] = float("nan")
        return img

    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9, "hist_bins": BINS}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        n = rows * cols
        planes = [channel(rows, cols, 50 + c, 1000.0 + 200.0 * c) for c in range(3)]
        st0 = ctx.compute_image_stats(planes[0])
        full_dim = max(rows, cols)
        u8 = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        rgb_full = torch.empty((rows, cols, 3), dtype=torch.uint8, device="cuda")
        ph, pw = ctx.preview_dims(rows, cols, PREVIEW)
        rgb_small = torch.empty((ph, pw, 3), dtype=torch.uint8, device="cuda")
        bins_host = [None]

        def hist_unfused(img=planes[0]):
            bins_host[0] = ctx.downsample_histogram(ctx.build_histogram(img, 65536, st0.min, st0.max), BINS)

        def display(img=planes[0]):
            bins_host[0] = ctx.display_histogram(img, st0.min, st0.max, BINS).cpu()

        def mono_chain():
            ctx.auto_stretch_preview(planes[0], out=u8)
            hist_unfused()

        def mono_view():
            bins_host[0] = ctx.process_fits_view(planes[0], hist_bins=BINS, out=u8).bins.cpu()

        def rgb_chain(max_dim, out):
            stats = [ctx.compute_image_stats(p) for p in planes]
            ctx.apply_tone_composite(*planes, stats, max_dim=max_dim, out=out)
            hist_unfused()

        def rgb_view(max_dim, out):
            bins_host[0] = ctx.process_rgb_fits_view(*planes, hist_bins=BINS, max_dim=max_dim, out=out).bins.cpu()

        entries = {
            "hist_unfused": (hist_unfused, 4 * n),
            "display_histogram": (display, 4 * n),
            "mono_chain": (mono_chain, 4 * n + 5 * n + 4 * n),
            "mono_view": (mono_view, 4 * n + 5 * n),
            "rgb_chain": (lambda: rgb_chain(full_dim, rgb_full), 12 * n + 15 * n + 4 * n),
            "rgb_view": (lambda: rgb_view(full_dim, rgb_full), 12 * n + 15 * n),
        }
        if (ph, pw) != (rows, cols):
            lines_per_row = -(-cols * 4 // 128) if cols / pw < 32 else pw
            touched = 3 * ph * lines_per_row * 128 + 3 * ph * pw
            entries["rgb_chain_4096"] = (lambda: rgb_chain(PREVIEW, rgb_small), 12 * n + touched + 4 * n)
            entries["rgb_view_4096"] = (lambda: rgb_view(PREVIEW, rgb_small), 12 * n + touched + 4 * n)
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "preview": [ph, pw]}
        for name, (ms, spread) in interleaved({k: v[0] for k, v in entries.items()}).items():
            nbytes = entries[name][1]
            floor_ms = nbytes / COPY_RATE * 1e3
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4), "bytes": nbytes, "traffic_floor_ms": round(floor_ms, 4),
                           "fraction_of_traffic_floor": round(floor_ms / ms, 4)}
        for fused, chain in (("display_histogram", "hist_unfused"), ("mono_view", "mono_chain"), ("rgb_view", "rgb_chain"),
                             ("rgb_view_4096", "rgb_chain_4096")):
            if fused in entry:
                entry[f"{fused}_over_{chain}"] = round(entry[chain]["call_ms"] / entry[fused]["call_ms"], 2)
        res[label] = entry
        del planes, u8, rgb_full, rgb_small
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
