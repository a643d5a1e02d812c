#!/usr/bin/env python3
"""Cost of the chunk calls' two staging steps (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks), one JSON line on stdout.

  python tools/chunk_bench.py --parent-lib PATH [--streams N,...] [--rounds R] [--steps K] [--warmup W]
  python tools/chunk_bench.py --side chunk|masked [--streams N,...] [--steps K] [--warmup W]      (one side, this process)

(a) "chunk": rnnoise_batch_process_device_chunks with every count equal to the frame (480 at 48 kHz, so F = 1 and every push
    completes exactly one frame), on this tree's library.
(b) "masked": rnnoise_batch_process_device_masked of one frame with every stream present, on the library at --parent-lib (the parent
    commit's build): the same kernels without the two staging steps.
With --parent-lib the two sides run in alternation, R rounds each, every run a fresh process (side (b) binds the few entry points it
needs by hand: the parent's library lacks the chunk calls this tree's binding declares); the median of the rounds' per-call times and
their min - max are reported per batch size, with the difference.  Device buffers, HIP events on one torch stream; the input is noise resident in HBM.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import lzma
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_side(a):
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    if a.side == "chunk":
        model = capi.Model(blob)
        res = {"side": a.side, "lib": capi.LIB_PATH}
    else:
        capi._share_hip_runtime_with_torch()
        L = C.CDLL(a.lib or capi.LIB_PATH)
        vp = C.c_void_p
        L.rnnoise_model_from_buffer.restype = vp
        L.rnnoise_model_from_buffer.argtypes = [C.c_char_p, C.c_int]
        L.rnnoise_batch_create.restype = vp
        L.rnnoise_batch_create.argtypes = [vp, C.c_int, C.c_int]
        L.rnnoise_batch_destroy.argtypes = [vp]
        L.rnnoise_batch_process_device_masked.argtypes = [vp] * 6 + [C.c_int, vp]
        model = L.rnnoise_model_from_buffer(blob, len(blob))
        res = {"side": a.side, "lib": a.lib or capi.LIB_PATH}
    for n in (int(v) for v in a.streams.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        b = capi.Batch(model, n) if a.side == "chunk" else L.rnnoise_batch_create(model, n, 0)
        assert b
        vad, gains = torch.empty((1, n), device=dev), torch.empty((1, n, 32), device=dev)
        if a.side == "chunk":
            pcm = (torch.randn((n, 480), generator=g, device=dev) * 3000).round()
            out = torch.empty_like(pcm)
            counts = torch.full((n,), 480, device=dev, dtype=torch.int32)
            frames = torch.empty((n,), device=dev, dtype=torch.int32)
            fn = lambda: b.process_chunks_device(out.data_ptr(), pcm.data_ptr(), counts.data_ptr(), 480, vad.data_ptr(), gains.data_ptr(),
                                                 frames.data_ptr(), h)
        else:
            pcm = (torch.randn((1, n, 480), generator=g, device=dev) * 3000).round()
            out = torch.empty_like(pcm)
            act = torch.ones((1, n), device=dev, dtype=torch.uint8)

            def fn():
                if L.rnnoise_batch_process_device_masked(b, out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), act.data_ptr(),
                                                         1, h):
                    raise RuntimeError("rnnoise_batch_process_device_masked failed")
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.steps):
            fn()
        e1.record(st)
        e1.synchronize()
        res[f"streams_{n}"] = round(e0.elapsed_time(e1) / a.steps, 5)
        if a.side == "chunk":
            b.close()
        else:
            L.rnnoise_batch_destroy(b)
        del pcm, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["chunk", "masked"])
    ap.add_argument("--lib", help="with --side masked: the library to load (default: this tree's)")
    ap.add_argument("--parent-lib", help="librnnoise_amd.so of the parent commit: side (b)")
    ap.add_argument("--streams", default="4096,65536")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="timed calls per round")
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.side:
        return one_side(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's librnnoise_amd.so (or --side for one side alone)")
    ms = {"chunk": {}, "masked": {}}
    for _ in range(a.rounds):
        for side in ("masked", "chunk"):
            lib = ["--lib", os.path.abspath(a.parent_lib)] if side == "masked" else []
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--streams", a.streams, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)] + lib, capture_output=True, text=True, check=True)
            row = json.loads(r.stdout.strip().splitlines()[-1])
            for k, v in row.items():
                if k.startswith("streams_"):
                    ms[side].setdefault(k, []).append(v)
    res = {"unit": "ms per call (median of the rounds; min, max)", "rounds": a.rounds, "steps": a.steps}
    for k in ms["chunk"]:
        c, m = ms["chunk"][k], ms["masked"][k]
        res[k] = {"chunk": [round(statistics.median(c), 4), min(c), max(c)], "parent_masked": [round(statistics.median(m), 4), min(m), max(m)],
                  "staging_ms": round(statistics.median(c) - statistics.median(m), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
