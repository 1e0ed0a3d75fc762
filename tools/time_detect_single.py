"""Developer tool: time single-frame detect_stars and normalize_for_detection on device-resident 1024^2 and 4096^2 frames
(run on the GPU box; AB_LIB_PATH=<variant .so> for A/B runs).  One warm call, then REPS (default 30) calls timed one by one
(each call ends in its own host join, detect_stars; normalize_for_detection is followed by a device synchronise); prints one JSON
line with the median, the quartiles and the extremes in ms, and a digest of the results for comparing two libraries."""
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import astroburst_amd as ab  # noqa: E402
from astroburst_amd import synth  # noqa: E402

REPS = int(os.environ.get("REPS", 30))
ctx = ab.Context(0)
ctx.use_torch_stream()
out = {"lib": os.path.basename(os.environ.get("AB_LIB_PATH", "libastroburst_hip.so")), "reps": REPS}
for side in (1024, 4096):
    y, x, flux = synth.star_catalog(side, side, max(50, 6000 * side * side // 4096 ** 2), seed=3)
    frame = synth.make_frame(side, side, 0, cat=(y, x, flux * 25.0), device="cuda", bad_patch_rate=0.0)
    norm = torch.empty_like(frame)
    torch.cuda.synchronize()
    for name, fn in (("detect_stars", lambda: ctx.detect_stars(frame, 5.0)), ("normalize_for_detection", lambda: ctx.normalize_for_detection(frame, out=norm))):
        res = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        q = statistics.quantiles(ms, n=4)
        if name == "detect_stars":
            stars, med, sig = res
            digest = hashlib.sha256(repr([(s.x, s.y, s.flux, s.fwhm, s.eccentricity, s.peak, s.snr, s.npix) for s in stars] + [med, sig]).encode()).hexdigest()[:16]
            extra = {"stars": len(stars)}
        else:
            digest = hashlib.sha256(res.cpu().numpy().tobytes()).hexdigest()[:16]
            extra = {}
        out[f"{name}_{side}"] = dict(median=round(statistics.median(ms), 4), q1=round(q[0], 4), q3=round(q[2], 4), min=round(min(ms), 4), max=round(max(ms), 4),
                                     digest=digest, **extra)
print(json.dumps(out), flush=True)
