#!/usr/bin/env python3
"""Cost of low-rate PCM (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate), one JSON line on stdout.

  python tools/rate_bench.py [--frames-per-call F] [--steps K] [--warmup W] [--configs N:RATE,...]

Step time of the device-resident lock-step call at 48 kHz and at 16 kHz for 4,096 and 65,536 streams, and at 8 and 24 kHz for 65,536,
with the ratio to 48 kHz at the same size.  Device buffers, HIP events on one torch stream; input PCM is noise resident in HBM.
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
    ap.add_argument("--frames-per-call", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100, help="timed frames per configuration (a multiple of --frames-per-call)")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--configs", default="", help="only these, e.g. 65536:48000,65536:16000 (for a kernel-trace run)")
    a = ap.parse_args()
    plan = ((4096, (48000, 16000)), (65536, (48000, 24000, 16000, 8000)))
    if a.configs:
        pairs = [tuple(int(v) for v in c.split(":")) for c in a.configs.split(",")]
        plan = tuple((n, tuple(r for m, r in pairs if m == n)) for n in dict.fromkeys(m for m, _ in pairs))
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

    for n, rates in plan:
        row = {}
        for rate in rates:
            M = 480 * rate // 48000
            g = torch.Generator(device=dev).manual_seed(n + rate)
            pcm = (torch.randn((F, n, M), generator=g, device=dev) * 3000).round()
            out = torch.empty_like(pcm)
            vad = torch.empty((F, n), device=dev)
            gains = torch.empty((F, n, 32), device=dev)
            b = capi.Batch(model, n)
            b.set_pcm_rate(rate)
            fn = lambda: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream)  # noqa: E731
            timed(fn, max(1, a.warmup // F))
            calls = max(1, a.steps // F)
            ms = timed(fn, calls) / (calls * F)
            row[str(rate)] = {"ms_per_step": round(ms, 4), "M_frames_per_s": round(n / ms / 1e3, 2)}
            b.close()
            del pcm, out, vad, gains
        if "48000" in row:
            for rate in rates:
                if rate != 48000:
                    row[str(rate)]["vs_48000"] = round(row[str(rate)]["ms_per_step"] / row["48000"]["ms_per_step"], 3)
        res[f"streams_{n}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
