#!/usr/bin/env python3
"""Cost of the per-stream suppression controls (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls), one JSON line on stdout.

  python tools/controls_bench.py [--steps K] [--warmup W] [--rounds R] [--configs N:F,...] [--only none|table]

Step time of the device-resident lock-step call without a control table and with a random one (every stream gated, floored, or both)
at 65,536 streams in 20-frame calls (the pipelined schedule) and at 4,096 streams in one-frame calls.  The two batches of a size are
timed in alternation, R rounds each, and the median per-step time of each is reported with their ratio.  Device buffers, HIP events on
one torch stream; input PCM is noise resident in HBM.  --configs / --only restrict the run (for a kernel-trace run of one form).
"""
from __future__ import annotations

import argparse
import json
import lzma
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="timed frames per round (a multiple of the frames per call)")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="65536:20,4096:1", help="streams:frames-per-call pairs")
    ap.add_argument("--only", choices=["none", "table"], default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    res = {"rounds": a.rounds, "steps": a.steps}

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for cfg in a.configs.split(","):
        n, F = (int(v) for v in cfg.split(":"))
        g = torch.Generator(device=dev).manual_seed(n + F)
        pcm = (torch.randn((F, n, 480), generator=g, device=dev) * 3000).round()
        out = torch.empty_like(pcm)
        vad = torch.empty((F, n), device=dev)
        gains = torch.empty((F, n, 32), device=dev)
        rng = np.random.default_rng(n)
        table = np.stack([rng.choice([0.0, 0.1, 0.01], n), rng.choice([0.0, 0.5, 0.9], n), rng.integers(0, 20, n)], 1)
        batches = {}
        for kind in ("none", "table"):
            if a.only and kind != a.only:
                continue
            b = capi.Batch(model, n)
            if kind == "table":
                b.set_stream_controls(np.ascontiguousarray(table, np.float32))
            batches[kind] = b
        fns = {k: (lambda b=b: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream))
               for k, b in batches.items()}
        calls = max(1, a.steps // F)
        for fn in fns.values():
            timed(fn, max(1, a.warmup // F))
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, calls) / (calls * F))
        row = {"frames_per_call": F}
        for k, v in ms.items():
            med = statistics.median(v)
            row[k] = {"ms_per_step": round(med, 4), "spread_ms": round(max(v) - min(v), 4), "M_frames_per_s": round(n / med / 1e3, 2)}
        if len(ms) == 2:
            row["table_vs_none"] = round(row["table"]["ms_per_step"] / row["none"]["ms_per_step"], 4)
        res[f"streams_{n}"] = row
        for b in batches.values():
            b.close()
        del pcm, out, vad, gains
    print(json.dumps(res))


if __name__ == "__main__":
    main()
