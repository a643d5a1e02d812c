#!/usr/bin/env python3
"""Cost of the float-network runtime (include/rnnoise_amd_fnet.h: rnnoise_amd_fnet_process_device).

  python tools/fnet_bench.py [--rounds R] [--warmup W] [--sizes N,...] [--gru H,...] [--frames T,...] [--out FILE] [--no-trace]

cond_size 128 with gru_size 384 and 256, at 128, 1,024, 4,096 and 16,384 rows, calls of 1 and of 10 frames of N(0, 1) features
resident in HBM: HIP events on one torch stream around ONE call, the median of R rounds with min - max, for
  fnet     fnet.FloatNetRuntime (librnnoise_amd_fnet.so), max_frames = the call's frames
  torch    float_net.FloatNet.forward, gru_impl "torch"
  stack    float_net.FloatNet.forward, gru_impl "stack" (librnnoise_amd_gru_stack.so under torch's convolutions and heads)
on the same features, the three alternating within a round, every one past its warm-up frames.  Per case: ms per call, frames per
second (rows x frames / time) and the runtime's launches per call (the header's formula).  Then the split front / GRUs / heads of the
runtime's time from one rocprofv3 --kernel-trace run of this file's --trace-child mode (a fresh process; skipped with --no-trace or
where rocprofv3 is missing).  Writes the table to FILE (default profiles/fnet_bench.txt) and prints it.  Without a GPU it fails: a
number that was not measured is not reported.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COND = 128


def _net(gru, impl="torch"):
    import torch

    from rnnoise_amd import float_net
    torch.manual_seed(gru)
    return float_net.FloatNet(COND, gru, gru_impl=impl).eval()


def trace_child(gru, rows, frames, calls):
    """what the trace run runs: `calls` calls of the runtime alone, past the warm-up"""
    import torch

    from rnnoise_amd import fnet
    dev = torch.device("cuda", 0)
    rt = fnet.FloatNetRuntime(_net(gru), device=0, max_frames=frames)
    x = torch.randn((rows, frames, 65), device=dev)
    for _ in range(calls + 4):
        rt(x)
    torch.cuda.synchronize()
    rt.close()


def trace_split(gru, rows, frames, calls=10):
    """-> {front, grus, heads: share of the runtime's kernel time} from one rocprofv3 --kernel-trace run, or None"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace-child",
               f"{gru},{rows},{frames},{calls}"]
        if subprocess.run(cmd, capture_output=True, text=True, timeout=600).returncode != 0:
            return None
        total = {"front": 0.0, "grus": 0.0, "heads": 0.0}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name, dt = row["Kernel_Name"], float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
                if "rn_fnet_gru" in name:
                    total["grus"] += dt
                elif "rn_fnet_heads" in name:
                    total["heads"] += dt
                elif "rn_fnet_gather" in name or "rn_fnet_conv" in name:
                    total["front"] += dt
        s = sum(total.values())
        return {k: v / s for k, v in total.items()} if s > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="128,1024,4096,16384")
    ap.add_argument("--gru", default="384,256")
    ap.add_argument("--frames", default="1,10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fnet_bench.txt"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(*[int(v) for v in a.trace_child.split(",")])
    import torch

    from rnnoise_amd import fnet
    if not torch.cuda.is_available():
        sys.exit("fnet_bench: no GPU: nothing measured")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    lines = [f"float-network runtime: ms per call, median of {a.rounds} rounds (min - max), HIP events around one call; cond_size {COND}; "
             "fnet: librnnoise_amd_fnet.so, torch / stack: FloatNet.forward with that gru_impl; same features, alternating in one job",
             "kfps: thousand row-frames per second; launches: the runtime's per call", "",
             f"{'gru':>4} {'rows':>6} {'frames':>6} {'path':<6} {'ms/call':>9} {'min':>9} {'max':>9} {'kfps':>10} {'launches':>8} {'MB':>8}"]
    for gru in [int(v) for v in a.gru.split(",")]:
        nets = {"torch": _net(gru).to(dev), "stack": _net(gru, "stack").to(dev)}
        for rows in [int(v) for v in a.sizes.split(",")]:
            for frames in [int(v) for v in a.frames.split(",")]:
                x = torch.randn((rows, frames, 65), device=dev)
                rt = fnet.FloatNetRuntime(nets["torch"], device=0, max_frames=frames)
                paths = {"fnet": lambda: rt(x), "torch": lambda: nets["torch"](x), "stack": lambda: nets["stack"](x)}
                for n in nets.values():
                    n.reset()
                with torch.no_grad():
                    for _ in range(a.warmup + 4):  # (past the four warm-up frames of every path)
                        for fn in paths.values():
                            fn()
                    times = {k: [] for k in paths}
                    for _ in range(a.rounds):
                        for k, fn in paths.items():
                            times[k].append(timed(fn))
                for k, v in times.items():
                    med = statistics.median(v)
                    launches = fnet.launches_formula(frames, frames, 1000) if k == "fnet" else ""
                    mb = f"{fnet.nbytes(COND, gru, rows, frames) / 2 ** 20:.0f}" if k == "fnet" else ""
                    lines.append(f"{gru:>4} {rows:>6} {frames:>6} {k:<6} {med:>9.3f} {min(v):>9.3f} {max(v):>9.3f} {rows * frames / med:>10.1f} "
                                 f"{launches:>8} {mb:>8}")
                rt.close()
                del x
                torch.cuda.empty_cache()
    if not a.no_trace:
        lines += ["", "the runtime's kernel time by part (one rocprofv3 --kernel-trace run each, 14 calls): gather + conv1 + conv2 | GRUs | heads"]
        for gru, rows, frames in ((384, 4096, 1), (384, 4096, 10), (384, 16384, 10)):
            split = trace_split(gru, rows, frames)
            lines.append(f"{gru:>4} {rows:>6} {frames:>6}  " + ("not measured (rocprofv3 did not run)" if split is None else
                                                               f"front {100 * split['front']:.1f} %  GRUs {100 * split['grus']:.1f} %  heads {100 * split['heads']:.1f} %"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
