#!/usr/bin/env python3
"""Cost of the stream-list calls (include/rnnoise_amd.h: rnnoise_batch_process_device_list), one JSON line on stdout.

  python tools/list_bench.py [--frames-per-call F ...] [--rows R ...] [--steps K] [--warmup W]

On a 65,536-stream batch, for n listed rows: ms per step of the list call (compact [F][n][480] buffers), of the masked call with
the same n streams present (full-size buffers), and of a masked all-present call on a fresh batch of n streams -- the floor a list
call is held to.  Device buffers, HIP events on one torch stream; input PCM is noise resident in HBM before timing starts.
"""
from __future__ import annotations

import argparse
import json
import lzma
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 4096, 16384, 65536])
    ap.add_argument("--frames-per-call", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--steps", type=int, default=32, help="timed frames per configuration (a multiple of every --frames-per-call)")
    ap.add_argument("--warmup", type=int, default=16)
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    N = a.batch
    res = {"batch": N, "unit": "ms per step (one frame of every listed / present stream)"}

    def timed(fn, F):
        for _ in range(max(1, a.warmup // F)):
            fn()
        calls = max(1, a.steps // F)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return round(e0.elapsed_time(e1) / (calls * F), 4)

    big = capi.Batch(model, N)
    for F in a.frames_per_call:
        g = torch.Generator(device=dev).manual_seed(F)
        pcm = (torch.randn((F, N, 480), generator=g, device=dev) * 3000).round()
        out, vad, gains = torch.empty_like(pcm), torch.empty((F, N), device=dev), torch.empty((F, N, 32), device=dev)
        for n in a.rows:
            streams = torch.randperm(N, generator=g, device=dev)[:n].to(torch.int32)
            rows = pcm[:, :n].contiguous()
            mask = torch.zeros((F, N), dtype=torch.uint8, device=dev)
            mask[:, streams.long()] = 1
            ones = torch.ones((F, n), dtype=torch.uint8, device=dev)
            row = {}
            row["list"] = timed(lambda: big.process_list_device(out.data_ptr(), rows.data_ptr(), vad.data_ptr(), gains.data_ptr(),
                                                                streams.data_ptr(), n, 0, F, h), F)
            row["masked_same_presence"] = timed(lambda: big.process_masked_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(),
                                                                                  gains.data_ptr(), mask.data_ptr(), F, h), F)
            small = capi.Batch(model, n)
            row["masked_all_fresh_batch_of_n"] = timed(lambda: small.process_masked_device(out.data_ptr(), rows.data_ptr(), vad.data_ptr(),
                                                                                            gains.data_ptr(), ones.data_ptr(), F, h), F)
            small.close()
            row["list_vs_fresh_batch"] = round(row["list"] / row["masked_all_fresh_batch_of_n"], 3)
            row["masked_vs_list"] = round(row["masked_same_presence"] / row["list"], 2)
            res[f"F{F}_rows{n}"] = row
            print(f"# F={F} rows={n}: {row}", file=sys.stderr, flush=True)
        del pcm, out, vad, gains
    big.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
