"""Developer tool: time the FFT power spectrum (csrc/spectrum.hip) on device planes -- 1024^2, 4096^2, 8192^2 and the C3 frame
13759 x 12451 (a 16384^2 buffer) -- with the Hann window on.  One JSON line.

ms = median wall time of one ab_compute_power_spectrum call (>= 5 calls after a warm-up, the call's own synchronise included).
hbm_floor_ms = the bytes the pass list moves (below) over the 8 TB/s HBM peak: the least time the memory system could take.
torch_fft2_c64_ms = torch.fft.fft2 on a size^2 complex64 buffer that is already padded, as an outside reference for the transform
alone (no window, no padding pass, no log / shift / block mean); null where this torch build does not offer it.

--kernels-only SIZE: a warm-up and three calls at one size and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/time_spectrum.py --kernels-only 4096`."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from astroburst_amd import Context  # noqa: E402
from astroburst_amd.core import power_spectrum_dims  # noqa: E402

SHAPES = [(1024, 1024), (4096, 4096), (8192, 8192), (13759, 12451)]
CALLS = 7
HBM_PEAK = 8.0e12


def pass_bytes(rows, cols):
    """HBM bytes of one call, pass by pass (csrc/spectrum.hip): the row pass reads the f32 image and writes its rows' spectra (8 B a
    point, the image's rows only); the transpose reads those and writes the whole size^2 plane; the column pass reads and writes it
    in place; the final kernel reads it and writes the display plane"""
    size, disp = power_spectrum_dims(rows, cols)
    row_pass = 4 * rows * cols + 8 * rows * size
    transpose = 8 * rows * size + 8 * size * size
    col_pass = 16 * size * size
    final = 8 * size * size + 4 * disp * disp
    return {"row_pass": row_pass, "transpose": transpose, "column_pass": col_pass, "log_shift_mean": final,
            "total": row_pass + transpose + col_pass + final}


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def frame(rows, cols):
    g = torch.Generator(device="cuda").manual_seed(rows + cols)
    return (300.0 + torch.randn((rows, cols), device="cuda", generator=g) * 5.0
            + 40000.0 * (torch.rand((rows, cols), device="cuda", generator=g) > 0.999)).float()


def main():
    ctx = Context(0)
    ctx.use_torch_stream()
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels-only":
        n = int(sys.argv[2])
        img = frame(n, n)
        for _ in range(4):
            ctx.compute_power_spectrum(img)
        torch.cuda.synchronize()
        print(json.dumps({"kernels_only": n, "calls": 4}))
        return
    res = {"calls": CALLS, "hbm_peak_tb_s": HBM_PEAK / 1e12, "sizes": {}}
    for rows, cols in SHAPES:
        size, disp = power_spectrum_dims(rows, cols)
        img = frame(rows, cols)
        out = torch.empty((disp, disp), device="cuda")
        med, lo, hi = timed(lambda: ctx.compute_power_spectrum(img, True, out=out), CALLS)
        b = pass_bytes(rows, cols)
        entry = {"buffer": size, "display": disp, "ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                 "hbm_bytes": b, "hbm_floor_ms": round(b["total"] / HBM_PEAK * 1e3, 3)}
        del img
        ctx.trim()  # (the 16384^2 workspaces are 4 GiB: give them back before torch allocates its own)
        try:
            buf = torch.zeros((size, size), dtype=torch.complex64, device="cuda")
            buf.real.normal_(generator=torch.Generator(device="cuda").manual_seed(1))
            entry["torch_fft2_c64_ms"] = round(timed(lambda: torch.fft.fft2(buf), 5)[0], 3)
            del buf
        except Exception as e:  # this torch build has no FFT backend for the shape, or no memory for its workspace
            entry["torch_fft2_c64_ms"] = None
            entry["torch_fft2_note"] = f"{type(e).__name__}: {str(e)[:120]}"
        torch.cuda.empty_cache()
        res["sizes"][f"{rows}x{cols}"] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
