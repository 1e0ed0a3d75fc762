"""Developer tool: ab_stack_weighted against ab_stack_sigma_clip on the same frames (run on the GPU box).

64, 32 and 16 synthetic 4096 x 4096 frames (the bench's recipe: stars, shot noise, cosmic rays, NaN patches, borders) whose sky level
drifts from frame to frame; weights spread over [0.25, 1], additive offsets that bring every sky to frame 0's.  Three launches per
frame count, each read from ab_stack_last_kernel_ms (the library's own events around its kernels), the median of five:
  weighted   ab_stack_weighted
  exact      ab_stack_sigma_clip on a context created with AB_STACK_EXACT=1 -- the same clipping arithmetic, no second copy, no sweep
  default    ab_stack_sigma_clip on the default engine
and the traffic floor, (4 N P + 8 P) bytes at the 6.29 TB/s copy rate."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import astroburst_amd as ab  # noqa: E402
from astroburst_amd import synth  # noqa: E402

R = C = int(os.environ.get("SIZE", 4096))
COPY_TBS = 6.29

ctx = ab.Context(0)
os.environ["AB_STACK_EXACT"] = "1"
ctx_exact = ab.Context(0)
del os.environ["AB_STACK_EXACT"]
for c in (ctx, ctx_exact):
    c.use_torch_stream()

truth = torch.full((R, C), 200.0, device="cuda") + synth.render_stars(R, C, synth.star_catalog(R, C, max(8, int(360 * R * C / 1e6))), device="cuda")
frames = [synth.make_frame(R, C, k, device="cuda", truth=truth, border=16 if k % 10 == 9 else 0) + float(3 * (k % 13)) for k in range(64)]
weights = np.linspace(0.25, 1.0, 64)[(np.arange(64) * 29) % 64]
offsets = np.array([-3.0 * (k % 13) for k in range(64)], np.float32)
out = torch.empty((R, C), device="cuda")


def median_ms(context, call):
    call()
    ms = []
    for _ in range(5):
        call()
        ms.append(context.stack_last_kernel_ms())
    return statistics.median(ms)


for n in (64, 32, 16):
    fr, w, o = frames[:n], weights[:n], offsets[:n]
    tw = median_ms(ctx, lambda: ctx.stack_weighted(fr, w, None, o, out=out, want_rejected=False))
    rej_w = ctx.last_rejected()
    tww = median_ms(ctx, lambda: ctx.stack_weighted(fr, w, None, o, out=out, want_weight=True, want_rejected=False))
    te = median_ms(ctx_exact, lambda: ctx_exact.stack_sigma_clip(fr, out=out, want_rejected=False))
    td = median_ms(ctx, lambda: ctx.stack_sigma_clip(fr, out=out, want_rejected=False))
    floor = (4 * n + 8) * R * C / (COPY_TBS * 1e12) * 1e3
    print(f"{n:2d} x {R}x{C}: weighted {tw:7.3f} ms (with the weight plane {tww:7.3f})   exact engine {te:7.3f} ms   default engine {td:7.3f} ms   "
          f"traffic floor {floor:6.3f} ms   rejected/px {rej_w / (R * C):.3f}")
