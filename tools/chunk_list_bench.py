#!/usr/bin/env python3
"""Cost of the chunk calls on a stream list (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks_list) against the only way
to push a part of a batch without them, and the split of that cost.  One JSON line on stdout.

  python tools/chunk_list_bench.py --parent-lib PATH [--streams N,...] [--rows R,...] [--rounds R] [--steps K] [--warmup W] [--order SIDES]
  python tools/chunk_list_bench.py --side list|frames|full [--lib PATH] ...                        (one side, this process)

Every configuration is a batch of N streams of which R push 480 samples per call (48 kHz: F = 1, every push completes one frame);
R = 0 on the command line stands for "all of them".
  "list"    rnnoise_batch_process_device_chunks_list on the R streams, this tree's library.
  "frames"  rnnoise_batch_process_device_list of one frame on the same R streams, this tree's library: the call in the middle of
            "list" without the two staging launches.
  "full"    rnnoise_batch_process_device_chunks on the whole batch with a count of 480 for the R streams and 0 elsewhere, on the
            library at --lib: the parent commit's way (bound by hand -- the parent's library lacks what this tree's binding declares).
With --parent-lib the sides run in alternation -- parent full, list, frames, this tree's full -- R rounds each, every run a fresh
process; per configuration the median of the rounds' per-call times and their min - max are reported.  Device buffers, HIP events
on one torch stream; the input is noise resident in HBM.
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
M = 480


def one_side(a):
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    lib = a.lib or capi.LIB_PATH
    if a.side == "full":
        capi._share_hip_runtime_with_torch()
        L = C.CDLL(lib)
        vp = C.c_void_p
        L.rnnoise_model_from_buffer.restype = vp
        L.rnnoise_model_from_buffer.argtypes = [C.c_char_p, C.c_int]
        L.rnnoise_batch_create.restype = vp
        L.rnnoise_batch_create.argtypes = [vp, C.c_int, C.c_int]
        L.rnnoise_batch_destroy.argtypes = [vp]
        L.rnnoise_batch_process_device_chunks.argtypes = [vp] * 4 + [C.c_int] + [vp] * 4
        model = L.rnnoise_model_from_buffer(blob, len(blob))
    else:
        model = capi.Model(blob)
    res = {"side": a.side, "lib": lib}
    for n in (int(v) for v in a.streams.split(",")):
        b = L.rnnoise_batch_create(model, n, 0) if a.side == "full" else capi.Batch(model, n)
        assert b
        for rows in (int(v) for v in a.rows.split(",")):
            R = n if rows == 0 or rows > n else rows
            g = torch.Generator(device=dev).manual_seed(n + R)
            # the R streams: spread over the batch, in shuffled order
            idx = (torch.randperm(n, generator=g, device=dev)[:R]).to(torch.int32).contiguous()
            if a.side == "full":
                pcm = (torch.randn((n, M), generator=g, device=dev) * 3000).round()
                out = torch.empty_like(pcm)
                counts = torch.zeros((n,), device=dev, dtype=torch.int32)
                counts[idx.long()] = M
                vad, gains = torch.empty((1, n), device=dev), torch.empty((1, n, 32), device=dev)
                frames = torch.empty((n,), device=dev, dtype=torch.int32)

                def fn():
                    if L.rnnoise_batch_process_device_chunks(b, out.data_ptr(), pcm.data_ptr(), counts.data_ptr(), M, vad.data_ptr(),
                                                             gains.data_ptr(), frames.data_ptr(), h):
                        raise RuntimeError("rnnoise_batch_process_device_chunks failed")
            else:
                pcm = (torch.randn((R, M), generator=g, device=dev) * 3000).round()
                out = torch.empty_like(pcm)
                counts = torch.full((R,), M, device=dev, dtype=torch.int32)
                vad, gains = torch.empty((1, R), device=dev), torch.empty((1, R, 32), device=dev)
                frames = torch.empty((R,), device=dev, dtype=torch.int32)
                if a.side == "list":
                    fn = lambda: b.process_chunks_list_device(out.data_ptr(), pcm.data_ptr(), counts.data_ptr(), M, idx.data_ptr(), R,
                                                              vad.data_ptr(), gains.data_ptr(), frames.data_ptr(), h)
                else:
                    fn = lambda: b.process_list_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), idx.data_ptr(), R, 0,
                                                       1, h)
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                fn()
            e1.record(st)
            e1.synchronize()
            res[f"streams_{n}_rows_{R}"] = round(e0.elapsed_time(e1) / a.steps, 5)
            del pcm, out
        if a.side == "full":
            L.rnnoise_batch_destroy(b)
        else:
            b.close()
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["list", "frames", "full"])
    ap.add_argument("--lib", help="with --side full: the library to load (default: this tree's)")
    ap.add_argument("--parent-lib", help="librnnoise_amd.so of the parent commit")
    ap.add_argument("--streams", default="4096,65536")
    ap.add_argument("--rows", default="64,1024,0", help="streams that push, per configuration; 0: the whole batch")
    ap.add_argument("--order", help="with --parent-lib: the sides to run and their order in a round, e.g. full,parent_full "
                                    "(default: parent_full,list,frames,full)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="timed calls per round")
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if a.side:
        return one_side(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent commit's librnnoise_amd.so (or --side for one side alone)")
    sides = [("parent_full", "full", ["--lib", os.path.abspath(a.parent_lib)]), ("list", "list", []), ("frames", "frames", []),
             ("full", "full", [])]
    if a.order:  # a subset of the sides, in the order given: whichever side runs first in a round has been seen to gain ~0.2 %
        sides = [next(v for v in sides if v[0] == name) for name in a.order.split(",")]
    ms = {name: {} for name, _, _ in sides}
    for _ in range(a.rounds):
        for name, side, extra in sides:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--streams", a.streams, "--rows", a.rows,
                                "--steps", str(a.steps), "--warmup", str(a.warmup)] + extra, capture_output=True, text=True)
            if r.returncode:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(f"side {name} ended with status {r.returncode}")  # (nothing more is started)
            row = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, json.dumps(row), file=sys.stderr, flush=True)
            for k, v in row.items():
                if k.startswith("streams_"):
                    ms[name].setdefault(k, []).append(v)
    res = {"unit": "ms per call (median of the rounds; min, max)", "rounds": a.rounds, "steps": a.steps}
    for k in next(iter(ms.values())):
        res[k] = {name: [round(statistics.median(v[k]), 4), min(v[k]), max(v[k])] for name, v in ms.items()}
        if "list" in ms and "frames" in ms:
            res[k]["staging_ms"] = round(statistics.median(ms["list"][k]) - statistics.median(ms["frames"][k]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
