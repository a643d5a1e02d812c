#!/usr/bin/env python3
"""What a caller-defined PCM layout buys (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout), one JSON line on stdout.

  python tools/layout_bench.py [--frames-per-call F] [--steps K] [--warmup W] [--rounds R] [--sizes 4096,65536]

A caller holds a device-resident [B, T] tensor (B streams, T = F frames of 480 samples each, float32 or int16) and wants the same
shape back.  Per size and sample type, ms per frame step of three ways to serve it:
  "permute"  the way without a layout: torch permute to frame-major [F][B][480] + the default call + permute back to [B, T];
  "streams"  one stream-contiguous call on the tensor as it lies, layout (480, F * 480);
  "default"  the plain default-layout call on a frame-major tensor, no transposes: "streams" against it is the price of strided rows
             in the kernels (above 2,048 streams K0 is the lane = stream form, whose lanes then read rows F * 480 samples apart).
--rounds: the whole set that many times over, every round's figure listed, so that the spread is on the page.  HIP events on one
torch stream; the input is noise resident in HBM.
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
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    F, M = a.frames_per_call, capi.FRAME
    res = {"frames_per_call": F}

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

    for n in (int(v) for v in a.sizes.split(",")):
        for s16 in (False, True):
            b = capi.Batch(model, n)
            g = torch.Generator(device=dev).manual_seed(n)
            bt = (torch.randn((n, F * M), generator=g, device=dev) * 3000).round()
            bt = bt.to(torch.int16) if s16 else bt
            fm = bt.view(n, F, M).permute(1, 0, 2).contiguous()  # the same frames, frame-major
            out_bt, out_fm = torch.empty_like(bt), torch.empty_like(fm)
            vad, gains = torch.empty((F, n), device=dev), torch.empty((F, n, 32), device=dev)

            def call(o, i):
                b.process_device(o.data_ptr(), i.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream, s16=s16)

            def permute():
                x = bt.view(n, F, M).permute(1, 0, 2).contiguous()
                call(out_fm, x)
                out_bt.view(n, F, M).copy_(out_fm.permute(1, 0, 2))

            ways = {"permute": ((0, 0), permute), "streams": ((M, F * M), lambda: call(out_bt, bt)),
                    "default": ((0, 0), lambda: call(out_fm, fm))}
            row = {k: [] for k in ways}
            for _ in range(a.rounds):
                for k, (lay, fn) in ways.items():
                    b.set_pcm_layout(*lay)
                    row[k].append(per_step(fn))
            res[f"{'s16' if s16 else 'f32'}_{n}"] = row
            b.close()
            del bt, fm, out_bt, out_fm, vad, gains
    print(json.dumps(res))


if __name__ == "__main__":
    main()
