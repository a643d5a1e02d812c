#!/usr/bin/env python3
"""Cost of the score call (include/rnnoise_amd.h: rnnoise_batch_score_records_device), one JSON line on stdout.

  python tools/score_bench.py [--frames T] [--warmup W] [--rounds R] [--sizes N,...]

At 4,096 and 65,536 rows, over T-frame sequences of random records and random predictions resident in HBM ([T][N][98], [T][N][32],
[T][N]), HIP events on one torch stream around the call:
  score_ms_per_frame         one rnnoise_batch_score_records_device call over the T frames (one launch), divided by the frames scored
  score_bands_ms_per_frame   the same with band_sums
  per_frame_calls_ms         the same frames as T calls of one frame each (t0 = t): what a launch per frame costs, as the record step
                             of rnnoise_batch_eval_records pays it
  stream_layout_ms_per_frame one call on [N][T] buffers (frame stride 98 / 32 / 1): a wave's frames side by side in memory
To hold against the "scoring_ms" column of profiles/eval_bench.txt (eval - features of the record step: 0.0041 and 0.0489 ms).
Each figure is the median of R rounds with the spread (max - min) beside it.
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
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536")
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    b = capi.Batch(model, 1)   # (the batch names the device)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    T = a.frames
    first = 1                  # every step but step 0 is scored: T - 1 frames per call
    res = {"rounds": a.rounds, "frames": T, "frames_scored": T - 1}

    def stat(v):
        return {"median": round(statistics.median(v), 5), "spread": round(max(v) - min(v), 5)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / (T - 1)

    for n in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        rec = torch.randn((T, n, capi.REC), generator=g, device=dev)
        rec[:, :, 65:97] = torch.rand((T, n, 32), generator=g, device=dev) * 1.2 - 0.2
        rec[:, :, 97] = (torch.rand((T, n), generator=g, device=dev) > 0.5).float()
        gains, vad = torch.rand((T, n, 32), generator=g, device=dev), torch.rand((T, n), generator=g, device=dev)
        rec_s, gains_s, vad_s = rec.transpose(0, 1).contiguous(), gains.transpose(0, 1).contiguous(), vad.transpose(0, 1).contiguous()
        sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
        bands = torch.zeros((n, 32), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def one(bd=0):
            b.score_records_device(sums.data_ptr(), bd, gains.data_ptr(), vad.data_ptr(), rec.data_ptr(), n, 0, T, first=first,
                                   stream=st.cuda_stream)

        def per_frame():
            for t in range(T):
                b.score_records_device(sums.data_ptr(), 0, gains.data_ptr() + t * n * 32 * 4, vad.data_ptr() + t * n * 4, rec.data_ptr(),
                                       n, t, 1, first=first, stream=st.cuda_stream)

        def stream_layout():
            b.score_records_device(sums.data_ptr(), 0, gains_s.data_ptr(), vad_s.data_ptr(), rec_s.data_ptr(), n, 0, T,
                                   gain_strides=(32, T * 32), vad_strides=(1, T), rec_strides=(capi.REC, T * capi.REC), first=first,
                                   stream=st.cuda_stream)

        calls = {"score_ms_per_frame": one, "score_bands_ms_per_frame": lambda: one(bands.data_ptr()), "per_frame_calls_ms": per_frame,
                 "stream_layout_ms_per_frame": stream_layout}
        for fn in calls.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        got = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, fn in calls.items():
                got[k].append(timed(fn))
        res[f"rows_{n}"] = {k: stat(v) for k, v in got.items()}
        res[f"rows_{n}"]["bytes_per_frame"] = n * 66 * 4
        del rec, gains, vad, rec_s, gains_s, vad_s, sums, bands
    b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
