"""Developer tool: time Richardson-Lucy (csrc/deconv.hip) on a 4096^2 device plane, 20 iterations, Gaussian PSFs 15 (sigma 2) and 31
(sigma 4); the same RL through a torch.fft float32 restatement on the GPU as the FFT alternative's figure.  One JSON line.

ms_per_iteration = median wall time of one call (>= 5 calls after a warm-up, joins included) / iterations.  FLOP = the algorithmic
2 (multiply + add) x 2 (forward + transpose) x pr x pc x rows x cols per iteration; the f32 vector peak is 157.3 TFLOP/s."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deconv_restatement as R  # noqa: E402
from astroburst_amd import Context  # noqa: E402

ROWS = COLS = int(os.environ.get("DECONV_SIZE", "4096"))
ITERS = 20
CALLS = 7
PEAK_TF = 157.3


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


ctx = Context(0)
ctx.use_torch_stream()
g = torch.Generator(device="cuda").manual_seed(5)
img = (300.0 + torch.rand((ROWS, COLS), device="cuda", generator=g) * 40000.0 * (torch.rand((ROWS, COLS), device="cuda", generator=g) > 0.999)
       + torch.randn((ROWS, COLS), device="cuda", generator=g) * 5.0).float()
out = torch.empty_like(img)
res = {"rows": ROWS, "cols": COLS, "iterations": ITERS, "calls": CALLS}
for size, sigma in ((15, 2.0), (31, 4.0)):
    psf = torch.from_numpy(R.gaussian_psf(size, sigma)).cuda()
    runs = []

    def call():
        runs.append(ctx.richardson_lucy(img, psf, ITERS, 0.001, True, 0.1, out=out)[1])

    ms = timed(call, CALLS)
    assert set(runs) == {ITERS}, runs
    flop = 4.0 * size * size * ROWS * COLS
    it_ms = ms / ITERS
    # (the restatement reads its f64 delta back every iteration, as the reference's loop does: one join per iteration)
    fft_ms = timed(lambda: R.richardson_lucy_torch(img, psf.cpu().numpy(), ITERS, 0.001, True, 0.1, dtype=torch.float32), 3) / ITERS
    res[f"psf{size}"] = {"ms_per_iteration": round(it_ms, 4), "gflop_per_iteration": round(flop / 1e9, 3),
                         "tflops": round(flop / (it_ms * 1e-3) / 1e12, 2), "fraction_of_f32_peak": round(flop / (it_ms * 1e-3) / 1e12 / PEAK_TF, 4),
                         "torch_fft_f32_ms_per_iteration": round(fft_ms, 4)}
print(json.dumps(res))
