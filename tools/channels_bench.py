#!/usr/bin/env python3
"""What interleaved channels cost and buy (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels), one JSON line on stdout.

  python tools/channels_bench.py [--frames-per-call F] [--steps K] [--warmup W] [--rounds R] [--sizes 65536,4096] [--channels 2]

A caller holds device-resident int16 PCM with C interleaved channels, frame-major: [F][B / C][480][C] (B streams in all), and wants
the same shape back.  Per size, ms per frame step of three ways to serve it:
  "planar"       the planar call on a [F][B][480] tensor, nothing around it: what the batch costs without the feature;
  "interleaved"  one call on the interleaved tensor as it lies, channel count C;
  "deinterleave" what callers do without the feature: a torch de-interleave to [F][B][480] + the planar call + an interleave back.
"interleaved" - "planar" is the price of strided rows in the kernels (above 2,048 streams it includes K0 running one wave per stream
where the planar call runs the lane = stream form: dispatch.h); what the feature has to beat is "deinterleave".
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
    ap.add_argument("--sizes", default="65536,4096")
    ap.add_argument("--channels", type=int, default=2)
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    F, M, C = a.frames_per_call, capi.FRAME, a.channels
    res = {"frames_per_call": F, "channels": C}

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
        b = capi.Batch(model, n)
        g = torch.Generator(device=dev).manual_seed(n)
        il = (torch.randn((F, n // C, M, C), generator=g, device=dev) * 3000).round().to(torch.int16)  # interleaved, as the caller holds it
        pl = il.permute(0, 1, 3, 2).contiguous().view(F, n, M)                                          # the same samples, planar
        out_il, out_pl = torch.empty_like(il), torch.empty_like(pl)
        vad, gains = torch.empty((F, n), device=dev), torch.empty((F, n, 32), device=dev)

        def call(o, i):
            b.process_device(o.data_ptr(), i.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, st.cuda_stream, s16=True)

        def deinterleave():
            x = il.permute(0, 1, 3, 2).contiguous()
            call(out_pl, x)
            out_il.copy_(out_pl.view(F, n // C, C, M).permute(0, 1, 3, 2))

        ways = {"planar": (1, lambda: call(out_pl, pl)), "interleaved": (C, lambda: call(out_il, il)), "deinterleave": (1, deinterleave)}
        row = {k: [] for k in ways}
        for _ in range(a.rounds):
            for k, (ch, fn) in ways.items():
                b.set_pcm_channels(ch)
                row[k].append(per_step(fn))
        res[f"s16_{n}"] = row
        b.close()
        del il, pl, out_il, out_pl, vad, gains
    print(json.dumps(res))


if __name__ == "__main__":
    main()
