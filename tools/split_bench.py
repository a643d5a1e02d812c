#!/usr/bin/env python3
"""Cost of the split calls (include/rnnoise_amd.h: rnnoise_batch_analyze_device, rnnoise_batch_synthesize_device)
beside the full call of the same build, one JSON line on stdout.

  python tools/split_bench.py [--frames T] [--warmup W] [--rounds R] [--sizes N,...] [--text]

--text prints the same figures as the commented text of profiles/split_bench.txt, which is this tool's output:
  python tools/split_bench.py --text > profiles/split_bench.txt

At 4,096 and 65,536 streams, T frames per call of random loud PCM resident in HBM, HIP events on one torch stream around each call,
in ms per frame:
  process       rnnoise_batch_process_device with vad and gains out
  analyze       rnnoise_batch_analyze_device into [T][N][65] rows
  features      rnnoise_batch_process_features_device on those rows (the batch's own network between the halves)
  synthesize    rnnoise_batch_synthesize_device with the gains and vad that call wrote
  chain         the three as one timed sequence
  chain_minus_process   what the split costs: the two staging launches per frame, the features' second trip through HBM, and the
                        overlap of K1 with the network that the full call's three-stream schedule has and the chain has not
Each figure is the median of R rounds with the spread (max - min) of the rounds beside it.  Every round runs the five timings in the
same order on a batch that keeps its state: the kernels' time does not depend on the data.
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


HEADER = """\
# tools/split_bench.py --text on one MI355X (gfx950): {rounds} rounds, {frames} frames per call, random loud PCM resident in HBM.
# Milliseconds per frame, HIP events on one torch stream around each call; "median" over the rounds, "spread" = max - min of the
# rounds.  DESIGN.md 4.29 reads these numbers.
#   process_ms_per_frame      rnnoise_batch_process_device with vad and gains out
#   analyze_ms_per_frame      rnnoise_batch_analyze_device into [T][N][65] rows
#   features_ms_per_frame     rnnoise_batch_process_features_device on those rows
#   synthesize_ms_per_frame   rnnoise_batch_synthesize_device with what that call wrote
#   chain_ms_per_frame        the three as one timed sequence
#   chain_minus_process_ms    per round: chain - process
#   store_bytes               the pending store of the call's frames (rnnoise_amd_split_frame_bytes)"""


def render(res):
    """the result as the text of profiles/split_bench.txt"""
    out = [HEADER.format(**res)] + [f"{k}: {res[k]}" for k in ("rounds", "frames", "rcp_profile")]
    for key, row in res.items():
        if key.startswith("streams_"):
            out.append(key)
            out += [f"  {k:<25} {json.dumps(v)}" for k, v in row.items()]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8, help="frames per call")
    ap.add_argument("--warmup", type=int, default=2, help="untimed rounds per batch")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--text", action="store_true", help="the text of profiles/split_bench.txt instead of one JSON line")
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

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / T

    for n in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        pcm = (torch.randn((T, n, 480), generator=g, device=dev) * 3000).round()
        out = torch.empty_like(pcm)
        vad, gains = torch.empty((T, n), device=dev), torch.empty((T, n, 32), device=dev)
        feats = torch.empty((T, n, capi.FEATURES), device=dev)
        sil = torch.empty((T, n), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        b = capi.Batch(model, n)
        b.split_reserve(T)
        s = st.cuda_stream

        def process():
            b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), T, s)

        def analyze():
            b.analyze_device(feats.data_ptr(), sil.data_ptr(), pcm.data_ptr(), T, stream=s)

        def features():
            b.process_features_device(gains.data_ptr(), vad.data_ptr(), feats.data_ptr(), T, stream=s)

        def synthesize():
            b.synthesize_device(out.data_ptr(), gains.data_ptr(), vad.data_ptr(), T, stream=s)

        def chain():
            analyze(), features(), synthesize()

        t = {k: [] for k in ("process", "analyze", "features", "synthesize", "chain")}
        for r in range(a.warmup + a.rounds):
            row = {"process": timed(process), "analyze": timed(analyze), "features": timed(features), "synthesize": timed(synthesize),
                   "chain": timed(chain)}
            if r >= a.warmup:
                for k, v in row.items():
                    t[k].append(v)
        b.close()
        res[f"streams_{n}"] = {k + "_ms_per_frame": stat(v) for k, v in t.items()}
        res[f"streams_{n}"]["chain_minus_process_ms"] = stat([c - p for c, p in zip(t["chain"], t["process"])])
        res[f"streams_{n}"]["store_bytes"] = T * capi.split_frame_bytes(n)
        del pcm, out, vad, gains, feats, sil
    print(render(res) if a.text else json.dumps(res))


if __name__ == "__main__":
    main()
