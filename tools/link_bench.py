#!/usr/bin/env python3
"""Cost of linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link), one JSON line on stdout.

  python tools/link_bench.py [--steps K] [--warmup W] [--rounds R] [--streams N,...] [--links K,...] [--frames-per-call F]

Step time of the device-resident lock-step call at link counts 1 (no link), 2 and 8, at 65,536 and 4,096 streams in 20-frame calls (the
pipelined schedule).  The batches of a size are timed in alternation, R rounds each, and the median per-step time of each is reported
with its ratio to K = 1.  Device buffers, HIP events on one torch stream; input PCM is noise resident in HBM, a different signal per
row.  --streams / --links restrict the run (for a kernel-trace run of one link count: K3's own time comes from there).
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
    ap.add_argument("--streams", default="65536,4096")
    ap.add_argument("--links", default="1,2,8")
    ap.add_argument("--frames-per-call", type=int, default=20)
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    F = a.frames_per_call
    links = [int(k) for k in a.links.split(",")]
    res = {"rounds": a.rounds, "steps": a.steps, "frames_per_call": F}

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for n in (int(v) for v in a.streams.split(",")):
        g = torch.Generator(device=dev).manual_seed(n + F)
        pcm = (torch.randn((F, n, 480), generator=g, device=dev) * 3000).round()
        out = torch.empty_like(pcm)
        vad = torch.empty((F, n), device=dev)
        gains = torch.empty((F, n, 32), device=dev)
        batches = {}
        for k in links:
            b = capi.Batch(model, n)
            b.set_gain_link(k)
            batches[k] = b
        fns = {k: (lambda b=b: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream))
               for k, b in batches.items()}
        calls = max(1, a.steps // F)
        for fn in fns.values():
            timed(fn, max(1, a.warmup // F))
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn, calls) / (calls * F))
        row = {}
        for k, v in ms.items():
            med = statistics.median(v)
            row[f"k{k}"] = {"ms_per_step": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                            "M_frames_per_s": round(n / med / 1e3, 2)}
        if 1 in ms:
            for k in ms:
                if k != 1:
                    row[f"k{k}"]["vs_k1"] = round(row[f"k{k}"]["ms_per_step"] / row["k1"]["ms_per_step"], 4)
        res[f"streams_{n}"] = row
        for b in batches.values():
            b.close()
        del pcm, out, vad, gains
    print(json.dumps(res))


if __name__ == "__main__":
    main()
