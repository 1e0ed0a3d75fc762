"""Developer tool: time the robust asinh preview and its renderers (csrc/preview.hip) on device-resident planes: 4096 x 4096 (the
bench's stacked plane) and 13759 x 12451 (a full mosaic, 685 MB).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of device time per call: HIP events on the stream around CALLS back-to-back calls, after one
warm-up round of every entry (the statistics read their histograms back, so the events enclose the host's part of the descent too).
spread_ms = max - min of the samples.  The entries are sampled in turn (A B C A B C ...), not one after the other.

traffic_floor_ms = the bytes the entry's pass list has to move over the measured copy rate (`python bench.py --full` reports it as
measured_copy_GBs; PREVIEW_COPY_GBS overrides the 6290 GB/s default, which is what a float4 copy reaches on this part):
    stats            P reads of the plane: 1 (the top 11 bits and the count) + one per distinct prefix the four ranks pass through at
                     the two lower levels + the same for the deviations' select.  P is computed here from the plane itself
                     (stats_plane_passes in the output), by the rule plane_select.hip's descent follows.
    normalize        1 read + 1 write of the plane (the map alone, with the statistics given)
    render_fused     stats + 2 reads of the plane + its bytes (ab_render_asinh_preview)
    render_unfused   stats + 1 read + 1 write (the map) + 2 reads + the bytes (ab_robust_asinh_preview, then ab_render_grayscale)
    grayscale_8      2 reads + the bytes;  stretched_8: 1 read + the bytes
PREVIEW_ONLY=4096 (or mosaic) restricts the run."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import astroburst_amd as ab  # noqa: E402

CALLS = int(os.environ.get("PREVIEW_CALLS", "5"))
SAMPLES = int(os.environ.get("PREVIEW_SAMPLES", "5"))
ONLY = os.environ.get("PREVIEW_ONLY")
COPY_RATE = float(os.environ.get("PREVIEW_COPY_GBS", "6290")) * 1e9


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


def select_passes(sorted_vals, ranks):
    """histogram passes of the 11/11/10 select for these ranks of the sorted non-negative candidates: the first level once, then one
    pass per distinct 11-bit prefix and one per distinct 22-bit prefix the ranks fall into"""
    keys = sorted_vals[torch.tensor(sorted(set(ranks)), device=sorted_vals.device)].view(torch.int32).tolist()
    return 1 + len({k >> 21 for k in keys}) + len({k >> 10 for k in keys})


def stats_passes(img):
    v = img.flatten()
    s = torch.sort(v[torch.isfinite(v) & (v > 1e-7)]).values
    m = s.numel()
    mid = [m // 2] if m % 2 else [m // 2 - 1, m // 2]
    passes = select_passes(s, mid + [int(float(m) * 0.01), min(int(float(m) * 0.999), m - 1)])
    median = s[mid[0]] if m % 2 else (s[mid[0]] + s[mid[1]]) / 2
    d = torch.sort((s - median).abs()).values
    return passes + select_passes(d, mid)


def star_field(rows, cols):
    g = torch.Generator(device="cuda").manual_seed(33)
    img = torch.randn((rows, cols), device="cuda", generator=g) * 3.0 + 100.0
    stars = torch.rand((rows, cols), device="cuda", generator=g) < 5e-4
    img[stars] += torch.empty(int(stars.sum()), device="cuda").exponential_(1 / 2000.0, generator=g)
    img[torch.rand((rows, cols), device="cuda", generator=g) < 0.02] = float("nan")   # registration borders / rejected pixels
    return img


def main():
    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9}
    for label, (rows, cols) in (("4096", (4096, 4096)), ("mosaic", (13759, 12451))):
        if ONLY and ONLY != label:
            continue
        img = star_field(rows, cols)
        n = rows * cols
        passes = stats_passes(img)
        torch.cuda.empty_cache()
        out_plane = torch.empty((rows, cols), device="cuda")
        out_u8 = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
        st = ctx.asinh_preview_stats(img)
        unit = torch.rand((rows, cols), device="cuda") * 1.5 - 0.25

        def unfused(route):
            ctx.robust_asinh_preview(img, route, out=out_plane)
            ctx.render_grayscale(out_plane, 8, out=out_u8)

        entries = {
            "stats": lambda: ctx.asinh_preview_stats(img),
            "normalize_avx2": lambda: ctx.asinh_normalize_with_stats(img, st, ab.ASINH_ROUTE_AVX2, out=out_plane),
            "normalize_scalar": lambda: ctx.asinh_normalize_with_stats(img, st, ab.ASINH_ROUTE_SCALAR, out=out_plane),
            "render_fused_avx2": lambda: ctx.render_asinh_preview(img, ab.ASINH_ROUTE_AVX2, out=out_u8),
            "render_fused_scalar": lambda: ctx.render_asinh_preview(img, ab.ASINH_ROUTE_SCALAR, out=out_u8),
            "render_unfused_avx2": lambda: unfused(ab.ASINH_ROUTE_AVX2),
            "grayscale_8": lambda: ctx.render_grayscale(unit, 8, out=out_u8),
            "stretched_8": lambda: ctx.render_stretched(unit, 8, out=out_u8),
        }
        stats_bytes = passes * 4 * n
        floor_bytes = {
            "stats": stats_bytes,
            "normalize_avx2": 8 * n,
            "normalize_scalar": 8 * n,
            "render_fused_avx2": stats_bytes + (2 * 4 + 1) * n,
            "render_fused_scalar": stats_bytes + (2 * 4 + 1) * n,
            "render_unfused_avx2": stats_bytes + 8 * n + (2 * 4 + 1) * n,
            "grayscale_8": (2 * 4 + 1) * n,
            "stretched_8": (4 + 1) * n,
        }
        entry = {"rows": rows, "cols": cols, "plane_MB": round(4 * n / 1e6, 1), "valid_count": st.valid_count, "stats_plane_passes": passes}
        for name, (ms, spread) in interleaved(entries).items():
            floor_ms = floor_bytes[name] / COPY_RATE * 1e3
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4), "traffic_floor_ms": round(floor_ms, 4),
                           "fraction_of_traffic_floor": round(floor_ms / ms, 4)}
        res[label] = entry
        del img, out_plane, out_u8, unit
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
