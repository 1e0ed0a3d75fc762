"""Developer tool: time ab_estimate_psf (csrc/psf.hip) on device-resident star fields -- 4096^2 and 13759 x 12451, a few thousand
Gaussian stars on an integer-valued noisy sky -- and, on the same plane in the same run, compute_image_stats as the yardstick (the
library's own whole-plane statistics: what a pass list over one plane costs here).  One JSON line.  Run it in a fresh process.

call_ms = median over SAMPLES samples of the time per call: HIP events on the stream around CALLS back-to-back calls, after one
warm-up round (both entries read results back, so the events enclose the host's part too: the suppression walk, the selection).
spread_ms = max - min of the samples.  The two entries are sampled in turn (A B A B ...).

traffic_floor_ms = the bytes the pass list has to move over the measured copy rate (PSF_COPY_GBS overrides the 6290 GB/s default):
five reads of the plane -- statistics, three histogram levels of the median select, the candidate pass; the per-star kernels touch
a few hundred KB.  PSF_ONLY=4096 (or full) restricts the run."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import astroburst_amd as ab  # noqa: E402

CALLS = int(os.environ.get("PSF_CALLS", "3"))
SAMPLES = int(os.environ.get("PSF_SAMPLES", "5"))
ONLY = os.environ.get("PSF_ONLY")
COPY_RATE = float(os.environ.get("PSF_COPY_GBS", "6290")) * 1e9


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


def star_field(rows, cols, n_stars, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.randn((rows, cols), device="cuda", generator=g).mul_(14.0).add_(200.0).round_()
    ys = torch.randint(40, rows - 40, (n_stars,), generator=g, device="cuda").tolist()
    xs = torch.randint(40, cols - 40, (n_stars,), generator=g, device="cuda").tolist()
    amp = torch.rand((n_stars,), generator=g, device="cuda").mul_(25000.0).add_(5000.0).tolist()
    fwhm = torch.rand((n_stars,), generator=g, device="cuda").mul_(2.0).add_(3.0).tolist()
    d = torch.arange(-12, 13, device="cuda", dtype=torch.float32)
    r2 = d[:, None] ** 2 + d[None, :] ** 2
    for y, x, a, f in zip(ys, xs, amp, fwhm):
        sigma = f / 2.3548
        img[y - 12:y + 13, x - 12:x + 13] += torch.round(a * torch.exp(-r2 / (2.0 * sigma * sigma)))
    img[rows // 2, cols // 2] += 60000.0   # one brighter pixel sets max_val: the stars sit between 10 % and 95 % of it
    return img


def main():
    ctx = ab.Context(0)
    ctx.use_torch_stream()
    res = {"calls_per_sample": CALLS, "samples": SAMPLES, "copy_rate_GBs": COPY_RATE / 1e9}
    for label, (rows, cols, n_stars) in (("4096", (4096, 4096, 2000)), ("full", (13759, 12451, 4000))):
        if ONLY and ONLY != label:
            continue
        img = star_field(rows, cols, n_stars, 5)
        out = torch.empty((31, 31), device="cuda")
        first = ctx.estimate_psf(img, out=out)
        entries = {"estimate_psf": lambda: ctx.estimate_psf(img, out=out), "compute_image_stats": lambda: ctx.compute_image_stats(img)}
        got = interleaved(entries)
        floor_ms = 5 * 4 * rows * cols / COPY_RATE * 1e3
        entry = {"rows": rows, "cols": cols, "planted_stars": n_stars, "stars_detected": first.stars_detected, "stars_filtered": first.stars_filtered,
                 "stars_used": len(first.stars_used), "average_fwhm": round(first.average_fwhm, 3)}
        for name, (ms, spread) in got.items():
            entry[name] = {"call_ms": round(ms, 4), "spread_ms": round(spread, 4)}
        entry["estimate_psf"]["traffic_floor_ms"] = round(floor_ms, 4)
        entry["estimate_psf"]["fraction_of_traffic_floor"] = round(floor_ms / got["estimate_psf"][0], 4)
        entry["psf_over_stats"] = round(got["estimate_psf"][0] / got["compute_image_stats"][0], 3)
        res[label] = entry
        del img
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
