#!/usr/bin/env python3
"""Cost of the masked calls and of per-stream reset (include/rnnoise_amd.h), one JSON line on stdout.

  python tools/masked_bench.py [--frames-per-call F] [--steps K] [--warmup W]

For 65,536 and 4,096 streams: M frames/s and ms per step of the lock-step device call, and of the masked device call with an
all-present and with a half-present mask (frames/s counts stream-frames offered, present or not, so the three compare per step).
Then rnnoise_batch_reset_streams_device of 1 / 64 / 4,096 streams on a 65,536-stream batch whose layer-wise network is in use
(the state images of the listed tiles are re-quantised too).  Device buffers, HIP events on one torch stream; input PCM is noise
resident in HBM before timing starts.
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
    ap.add_argument("--steps", type=int, default=64, help="timed frames per configuration (a multiple of --frames-per-call)")
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--reset-reps", type=int, default=50)
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    F = a.frames_per_call
    res = {"frames_per_call": F}

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for n in (65536, 4096):
        g = torch.Generator(device=dev).manual_seed(n)
        pcm = (torch.randn((F, n, 480), generator=g, device=dev) * 3000).round()
        out = torch.empty_like(pcm)
        vad = torch.empty((F, n), device=dev)
        gains = torch.empty((F, n, 32), device=dev)
        half = (torch.rand((F, n), generator=g, device=dev) < 0.5).to(torch.uint8)
        ones = torch.ones((F, n), dtype=torch.uint8, device=dev)
        row = {}
        for name, mask in (("lockstep", None), ("masked_all", ones), ("masked_half", half)):
            b = capi.Batch(model, n)
            if mask is None:
                fn = lambda: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream)  # noqa: E731
            else:
                fn = lambda: b.process_masked_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(),  # noqa: E731
                                                     mask.data_ptr(), F, st.cuda_stream)
            timed(fn, max(1, a.warmup // F))
            calls = max(1, a.steps // F)
            ms = timed(fn, calls) / (calls * F)
            row[name] = {"ms_per_step": round(ms, 4), "M_frames_per_s": round(n / ms / 1e3, 2)}
            b.close()
        row["masked_all_vs_lockstep"] = round(row["masked_all"]["ms_per_step"] / row["lockstep"]["ms_per_step"], 3)
        res[f"streams_{n}"] = row
        del pcm, out, vad, gains

    n = 65536
    b = capi.Batch(model, n)
    pcm = torch.zeros((1, n, 480), device=dev)
    out, vad = torch.empty_like(pcm), torch.empty((1, n), device=dev)
    b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), 0, 1, st.cuda_stream)  # (the state images are now in use)
    reset = {}
    for k in (1, 64, 4096):
        idx = torch.randperm(n, device=dev)[:k].to(torch.int32)
        fn = lambda: b.reset_streams_device(idx.data_ptr(), k, st.cuda_stream)  # noqa: E731
        timed(fn, 5)
        reset[str(k)] = round(timed(fn, a.reset_reps) / a.reset_reps * 1e3, 1)
    res["reset_streams_us_at_65536"] = reset
    b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
