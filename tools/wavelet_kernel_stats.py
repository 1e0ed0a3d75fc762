"""Developer tool: per-scale kernel times of wavelet denoising from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_wavelet.py
    python tools/wavelet_kernel_stats.py DIR

Reads every *kernel_trace.csv under DIR.  A call ends at wt_reconstruct_kernel; within a call the wt_* kernels are numbered per name
in launch order, which is the order of the scales (wt_fused_kernel<false> #0 is the first fused scale after scale 0, wt_row_kernel #0
the first two-pass scale, ...).  Prints calls / median / min / max in microseconds per (kernel, ordinal), with the launch's LDS size
and grid so that the steps can be told apart."""
import csv
import glob
import statistics
import sys
from collections import defaultdict

rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
seen, per = defaultdict(int), defaultdict(list)
for r in rows:
    name = r["Kernel_Name"]
    if "wt_" not in name and "plane_select" not in name:
        continue
    short = name.split("(")[0].replace("(anonymous namespace)::", "").replace("void ", "")
    key = (short, seen[short], r.get("LDS_Block_Size", "?"), r.get("Grid_Size_X", r.get("Grid_Size", "?")))
    per[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    seen[short] += 1
    if "wt_reconstruct" in short:
        seen.clear()
for (short, ordinal, lds, grid), v in per.items():
    print(f"{short:34s} #{ordinal} lds {lds:>6} grid_x {grid:>9}  calls {len(v):4d}  median {statistics.median(v):8.1f}  min {min(v):8.1f}  max {max(v):8.1f} us")
