#!/usr/bin/env python3
"""Cost of per-stream G.711 (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats), one JSON line on stdout.

  python tools/format_bench.py [--frames-per-call F] [--steps K] [--warmup W] [--rounds R] [--sizes 4096,65536]

Step time of the device-resident lock-step int16 call, three workloads: "8k_N" a uniform 8 kHz batch of N streams (4,096 and 65,536),
"mixed_N" a 48 kHz batch whose rate table puts a quarter of the streams at each of 48 / 24 / 16 / 8 kHz, and "48k_N" a 48 kHz batch
with no rate table -- the one whose K0 the format table moves from the lane = stream form to one wave per stream.  Each is timed "linear" (no
format table: int16 rows, today's launches) and, where the library has the format table, "g711" (mu-law, A-law and linear streams
interleaved one by one, a third each) and "all_ulaw" (every stream companded).  --rounds: the whole set that many times over, every
round's figure listed, so that the spread is on the page.  Copied into a checkout of a commit without the table it reports "linear"
only: the baseline.  Device buffers, HIP events on one torch stream; the input is noise resident in HBM (as int16
for the linear rows; the same bytes are read as codes by the companded ones: every byte is a valid code).
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", default="4096,65536")
    a = ap.parse_args()
    import numpy as np
    import torch
    from rnnoise_amd import capi

    lib = capi.lib()
    has_table = hasattr(lib, "rnnoise_batch_set_stream_formats")
    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    F = a.frames_per_call
    res = {"frames_per_call": F, "format_table": has_table}

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def per_step(fn):
        timed(fn, max(1, a.warmup // F))
        calls = max(1, a.steps // F)
        return round(timed(fn, calls) / (calls * F), 4)

    def workload(n, kind):
        b = capi.Batch(model, n)
        if kind == "mixed":
            b.set_stream_rates([capi.PCM_RATES[s % 4] for s in range(n)])
        elif kind == "8k":
            b.set_pcm_rate(8000)
        g = torch.Generator(device=dev).manual_seed(n + len(kind))
        pcm = (torch.randn((F, n, b.frame), generator=g, device=dev) * 3000).round().to(torch.int16)
        out, vad, gains = torch.empty_like(pcm), torch.empty((F, n), device=dev), torch.empty((F, n, 32), device=dev)
        fn = lambda: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream, s16=True)  # noqa: E731
        return b, fn, (pcm, out, vad, gains)

    tables = {"linear": None}
    if has_table:
        tables["g711"] = lambda n: (np.arange(n) % 3).astype(np.uint8)
        tables["all_ulaw"] = lambda n: np.ones(n, np.uint8)
    for n in (int(v) for v in a.sizes.split(",")):
        for kind in ("8k", "mixed", "48k"):
            name = f"{kind}_{n}"
            b, fn, keep = workload(n, kind)
            row = {k: [] for k in tables}
            for _ in range(a.rounds):
                for k, t in tables.items():
                    if has_table:
                        b.set_stream_formats(None if t is None else t(n))
                    row[k].append(per_step(fn))
            res[name] = row
            b.close()
            del keep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
