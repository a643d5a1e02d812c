#!/usr/bin/env python3
"""Cost of low-rate PCM (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate), one JSON line on stdout.

  python tools/rate_bench.py [--frames-per-call F] [--steps K] [--warmup W] [--configs N:RATE,...]
  python tools/rate_bench.py --mixed [--sizes 4096,65536] ...

Step time of the device-resident lock-step call at 48 kHz and at 16 kHz for 4,096 and 65,536 streams, and at 8 and 24 kHz for 65,536,
with the ratio to 48 kHz at the same size.  Device buffers, HIP events on one torch stream; input PCM is noise resident in HBM.
--mixed: a quarter of the streams at each of the four rates, two ways.  "mixed": ONE 48 kHz batch with a rate table
(rnnoise_batch_set_stream_rates), the rates interleaved stream by stream.  "four_batches": the same legs without a table -- four
uniform batches of a quarter of the streams each, their calls issued one after the other on one HIP stream; per-step time of the
four together, and of each alone.  (A library without the rate table reports "four_batches" only.)
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
    ap.add_argument("--mixed", action="store_true", help="one mixed-rate batch against four uniform batches of a quarter each")
    ap.add_argument("--sizes", default="4096,65536", help="--mixed: total streams of each configuration")
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

    def buffers(n, rate, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        pcm = (torch.randn((F, n, 480 * rate // 48000), generator=g, device=dev) * 3000).round()
        return pcm, torch.empty_like(pcm), torch.empty((F, n), device=dev), torch.empty((F, n, 32), device=dev)

    def call(b, bufs):
        pcm, out, vad, gains = bufs
        return lambda: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream)

    def per_step(fn):
        timed(fn, max(1, a.warmup // F))
        calls = max(1, a.steps // F)
        return round(timed(fn, calls) / (calls * F), 4)

    if a.mixed:
        res["mode"] = "mixed"
        for n in (int(v) for v in a.sizes.split(",")):
            row, q = {}, n // 4
            quarters = []
            for rate in capi.PCM_RATES:
                b = capi.Batch(model, q)
                b.set_pcm_rate(rate)
                quarters.append((b, call(b, buffers(q, rate, n + rate))))
            for rate, (b, fn) in zip(capi.PCM_RATES, quarters):
                row[f"quarter_{rate}"] = per_step(fn)
            row["four_batches"] = per_step(lambda: [fn() for _, fn in quarters])
            for b, _ in quarters:
                b.close()
            del quarters
            if hasattr(capi.Batch, "set_stream_rates"):
                b = capi.Batch(model, n)
                b.set_stream_rates([capi.PCM_RATES[s % 4] for s in range(n)])
                row["mixed"] = per_step(call(b, buffers(n, 48000, n)))
                row["mixed_vs_four"] = round(row["mixed"] / row["four_batches"], 3)
                b.close()
            res[f"streams_{n}"] = row
        print(json.dumps(res))
        return

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
