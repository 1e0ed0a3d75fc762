"""Developer tool: time ab_drizzle_frames (csrc/drizzle.hip) on 10 and 32 device frames of 4096^2, scale 2 / pixfrac 0.7 (the reference's
default; its paper's example is the 10-frame case), each kernel.  One JSON line.

ms = median wall time of one call (7 calls after a warm-up, joins included: the call reads rejected_pixels back).  The traffic floor
the figure stands against: 4 N P bytes of frames read + 8 P scale^2 bytes of image and weight map written, at the 8 TB/s HBM rate
DESIGN.md uses (P = input pixels per frame)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from astroburst_amd import Context  # noqa: E402

SIZE = int(os.environ.get("DRIZZLE_SIZE", "4096"))
COUNTS = [int(v) for v in os.environ.get("DRIZZLE_FRAMES", "10,32").split(",")]
KERNELS = os.environ.get("DRIZZLE_KERNELS", "square,gaussian,lanczos3").split(",")
ITERS = int(os.environ.get("DRIZZLE_ITERS", "5"))  # sigma_iterations (0: no clipping round, the sort and the mean remain)
CALLS = 7
SCALE, PIXFRAC = 2.0, 0.7
HBM = 8e12


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


ctx = Context(0)
ctx.use_torch_stream()
g = torch.Generator(device="cuda").manual_seed(7)
nmax = max(COUNTS)
frames = []
for k in range(nmax):
    f = 300.0 + torch.randn((SIZE, SIZE), device="cuda", generator=g) * 5.0
    f += 20000.0 * (torch.rand((SIZE, SIZE), device="cuda", generator=g) > 0.999)
    frames.append(f.float())
rng = np.random.default_rng(7)
offsets = [(0.0, 0.0)] + [tuple(rng.uniform(-4.0, 4.0, 2)) for _ in range(nmax - 1)]
o = int(np.ceil(SIZE * SCALE))
out = torch.empty((o, o), device="cuda")
wgt = torch.empty((o, o), device="cuda")
res = {"rows": SIZE, "cols": SIZE, "scale": SCALE, "pixfrac": PIXFRAC, "sigma_iterations": ITERS, "calls": CALLS}
for n in COUNTS:
    floor_ms = (4.0 * n * SIZE * SIZE + 8.0 * SIZE * SIZE * SCALE * SCALE) / HBM * 1e3
    for kernel in KERNELS:
        rej = []

        def call():
            rej.append(ctx.drizzle_frames(frames[:n], offsets[:n], SCALE, PIXFRAC, kernel, 3.0, 3.0, ITERS, out=out, out_weight=wgt).rejected_pixels)

        ms, best = timed(call, CALLS)
        assert len(set(rej)) == 1, rej
        res[f"n{n}_{kernel}"] = {"ms": round(ms, 3), "min_ms": round(best, 3), "traffic_floor_ms": round(floor_ms, 3), "times_floor": round(ms / floor_ms, 2),
                                 "rejected_pixels": rej[0]}
print(json.dumps(res))
