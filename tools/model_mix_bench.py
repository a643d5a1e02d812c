#!/usr/bin/env python3
"""Cost of several models in one batch (include/rnnoise_amd.h: rnnoise_batch_add_model), one table on stdout.

  python tools/model_mix_bench.py [--frames-per-call F] [--steps K] [--warmup W] [--streams 4096,65536] [--cases 0,1,2,3,4]

For each batch size and slot map: ms per step of the pipelined device call (frames-per-call frames per call, HIP events on one
torch stream), then K2 -- the network's device time per step, every slot's launches summed (rnnoise_batch_kernel_ms ms[1]) -- from a
second, timed pass.  Cases: one model; two slots added with every stream on slot 0; two models on whole 64-stream groups; two models
interleaved stream by stream; eight models interleaved.  Device buffers; input PCM is noise resident in HBM before timing starts.
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
    ap.add_argument("--frames-per-call", type=int, default=16)
    ap.add_argument("--steps", type=int, default=128, help="timed frames per case (a multiple of --frames-per-call)")
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--streams", default="4096,65536")
    ap.add_argument("--cases", default="0,1,2,3,4", help="which of the five cases, by index (a profiler run takes one at a time)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from rnnoise_amd import blob as rb
    from rnnoise_amd import capi

    blobs = [lzma.decompress(open(os.path.join(ROOT, "tests", "golden", f"{m}.blob.xz"), "rb").read()) for m in ("default", "little")]
    blobs += [rb.synth_model(seed=40 + i) for i in range(6)]
    models = [capi.Model(b) for b in blobs]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    F = a.frames_per_call

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    cases = [  # name, slots, map
        ("one model", 1, None),
        ("2 slots, all on slot 0", 2, lambda s: np.zeros_like(s)),
        ("2 models, per 64-stream group", 2, lambda s: (s // 64) % 2),
        ("2 models, interleaved", 2, lambda s: s % 2),
        ("8 models, interleaved", 8, lambda s: s % 8),
    ]
    cases = [cases[int(i)] for i in a.cases.split(",")]
    print(f"# tools/model_mix_bench.py --frames-per-call {F} --steps {a.steps} --warmup {a.warmup}  (device buffers, {torch.cuda.get_device_name(dev)})")
    print(f"{'streams':>8}  {'case':<32} {'ms/step':>8} {'vs one':>7} {'K2 ms':>7} {'vs one':>7}")
    res = []
    for n in (int(x) for x in a.streams.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        pcm = (torch.randn((F, n, 480), generator=g, device=dev) * 3000).round()
        out = torch.empty_like(pcm)
        vad = torch.empty((F, n), device=dev)
        gains = torch.empty((F, n, 32), device=dev)
        base = None
        for name, k, fmap in cases:
            b = capi.Batch(models[0], n)
            for i in range(1, k):
                b.add_model(models[i])
            if fmap is not None:
                b.set_stream_models(fmap(np.arange(n)).astype(np.uint8))
            fn = lambda: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream)  # noqa: E731
            timed(fn, max(1, a.warmup // F))
            calls = max(1, a.steps // F)
            ms = timed(fn, calls) / (calls * F)
            b.enable_timing(True)
            timed(fn, calls)
            k2 = b.kernel_ms()["network"]
            b.close()
            if base is None:
                base = (ms, k2)
            row = dict(streams=n, case=name, ms_per_step=round(ms, 4), k2_ms=round(k2, 4), step_vs_one=round(ms / base[0], 3),
                       k2_vs_one=round(k2 / base[1], 3))
            res.append(row)
            print(f"{n:>8}  {name:<32} {ms:>8.4f} {ms / base[0]:>7.3f} {k2:>7.4f} {k2 / base[1]:>7.3f}", flush=True)
        del pcm, out, vad, gains
    print(json.dumps(res))


if __name__ == "__main__":
    main()
