#!/usr/bin/env python3
"""Cost of the record step of the eval-records call (include/rnnoise_amd.h: rnnoise_batch_eval_records_device), one
JSON line on stdout.

  python tools/eval_bench.py [--frames T] [--warmup W] [--rounds R] [--sizes N,...]

At 4,096 and 65,536 streams, over T-frame sequences of random records resident in HBM ([T][N][98]):
  eval_ms_per_frame        rnnoise_batch_eval_records_device, HIP events on one torch stream around the whole call, timing taps off
  network_ms_per_frame     the network's own time in the same call (kind 1 of rnnoise_batch_kernel_ms), from a run of its own with the
                           taps on
  record_step_ms           their difference: the record step's launch -- score step t, stage step t + 1 -- and the gaps around it
  features_ms_per_frame    rnnoise_batch_process_features_device on the same rows, timed the same way: the same launches with
                           nothing scored, so eval - features is what the scoring (the f64 terms) costs and features - network what
                           staging and the gaps between the launches cost
  process_network_ms       kind 1 of a one-frame rnnoise_batch_process_device call of a batch of the same size and path: the network as
                           the PCM calls run it, to hold against DESIGN.md 4.3
Each figure is the median of R rounds with the spread (max - min) of the rounds beside it; a round starts from a reset batch.
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
    ap.add_argument("--frames", type=int, default=40, help="frames per sequence: one eval call")
    ap.add_argument("--warmup", type=int, default=2, help="untimed calls per batch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536")
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    T = a.frames
    res = {"rounds": a.rounds, "frames": T, "rcp_profile": capi.rcp_profile()}

    def stat(v):
        return {"median": round(statistics.median(v), 5), "spread": round(max(v) - min(v), 5)}

    for n in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        rec = torch.randn((T, n, capi.REC), generator=g, device=dev)
        rec[:, :, 65:97] = torch.rand((T, n, 32), generator=g, device=dev) * 1.2 - 0.2   # targets, a sixth of them masked
        rec[:, :, 97] = (torch.rand((T, n), generator=g, device=dev) > 0.5).float()
        sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
        pcm = (torch.randn((1, n, 480), generator=g, device=dev) * 3000).round()
        out, vad, gains = torch.empty_like(pcm), torch.empty((1, n), device=dev), torch.empty((1, n, 32), device=dev)
        torch.cuda.synchronize()
        b = capi.Batch(model, n)

        def eval_call():
            b.eval_records_device(sums.data_ptr(), 0, 0, rec.data_ptr(), 0, T, stream=st.cuda_stream)

        for _ in range(a.warmup):
            eval_call()
        torch.cuda.synchronize()
        def feat_call():
            b.process_features_device(0, 0, rec.data_ptr(), T, frame_stride=n * capi.REC, row_stride=capi.REC, stream=st.cuda_stream)

        wall, net, feat = [], [], []
        for _ in range(a.rounds):
            b.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            eval_call()
            e1.record(st)
            e1.synchronize()
            wall.append(e0.elapsed_time(e1) / T)
            b.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            feat_call()
            e1.record(st)
            e1.synchronize()
            feat.append(e0.elapsed_time(e1) / T)
            b.reset()
            b.enable_timing(True)
            eval_call()
            torch.cuda.synchronize()
            k = b.kernel_ms()
            assert k["launches"] == T, k
            net.append(k["network"])
            b.enable_timing(False)
        b.close()
        p = capi.Batch(model, n)
        p.set_schedule(9)
        pnet = []
        for _ in range(a.warmup * 4):
            p.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), 1, st.cuda_stream)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            p.enable_timing(True)
            for _ in range(T):
                p.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), 1, st.cuda_stream)
            torch.cuda.synchronize()
            pnet.append(p.kernel_ms()["network"])
            p.enable_timing(False)
        p.close()
        res[f"streams_{n}"] = {"eval_ms_per_frame": stat(wall), "network_ms_per_frame": stat(net),
                               "record_step_ms": stat([w - k for w, k in zip(wall, net)]), "features_ms_per_frame": stat(feat),
                               "scoring_ms": stat([w - f for w, f in zip(wall, feat)]), "process_network_ms": stat(pnet),
                               "record_bytes_per_frame": n * (98 + 68 + 33) * 4}
        del rec, sums, pcm, out, vad, gains
    print(json.dumps(res))


if __name__ == "__main__":
    main()
