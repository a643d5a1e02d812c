#!/usr/bin/env python3
"""profiles/stoi_bench_kernels.txt from a kernel trace of tools/stoi_bench.py.

  rocprofv3 --kernel-trace --stats -d DIR -- python tools/stoi_bench.py --sizes 128 --rounds 3 --out /dev/null
  python tools/stoi_kernel_times.py DIR [--out FILE]

Reads the `kernels` view of the result database rocprofv3 leaves under DIR (sqlite), groups the rn_stoi_* launches into calls -- a call
starts at its resample launch, whose grid says whether the noisy plane was there -- and writes per kernel the median duration over the
calls with min - max and its share of the five launches.
"""
from __future__ import annotations

import argparse
import glob
import os
import sqlite3
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["rn_stoi_resample_kernel", "rn_stoi_keep_kernel", "rn_stoi_bands_kernel", "rn_stoi_segments_kernel", "rn_stoi_sum_kernel"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_bench_kernels.txt"))
    a = ap.parse_args()
    dbs = sorted(glob.glob(os.path.join(a.dir, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no result database under {a.dir}")
    rows = sqlite3.connect(dbs[0]).execute(
        "select name, duration, grid_x, grid_y, grid_z, workgroup_x from kernels where name like 'rn_stoi%' order by start").fetchall()
    calls = []
    for name, duration, gx, gy, gz, wx in rows:
        if name == ORDER[0]:
            calls.append({"in": gz == 3, "rows": gy, "tiles": gx // wx})
        if calls:
            calls[-1][name] = duration / 1e3
    calls = [c for c in calls if all(k in c for k in ORDER)]
    if not calls:
        raise SystemExit("no complete STOI call in the trace")
    lines = [f"STOI call, kernel by kernel: rocprofv3 --kernel-trace on tools/stoi_bench.py, {calls[0]['rows']} rows, "
             f"{calls[0]['tiles']} resample tiles a signal; a run of its own (tools/stoi_kernel_times.py)",
             "microseconds per launch, median over the calls of the job (min - max), and the share of the five launches together", ""]
    for has_in in (True, False):
        cs = [c for c in calls if c["in"] == has_in]
        if not cs:
            continue
        med = {k: statistics.median(c[k] for c in cs) for k in ORDER}
        total = sum(med.values())
        lines.append(f"{'with' if has_in else 'without'} the noisy plane ({len(cs)} calls), five launches {total:.0f} us")
        for k in ORDER:
            v = [c[k] for c in cs]
            lines.append(f"  {k:<26} {med[k]:>9.1f} ({min(v):.1f} - {max(v):.1f}) {100 * med[k] / total:>5.1f} %")
        lines.append("")
    text = "\n".join(lines)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
