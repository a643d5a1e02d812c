#!/usr/bin/env python3
"""Cost of the per-stream output tables (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates), and what they leave alone.

  python tools/out_tables_bench.py --parent-tree DIR [--rounds R] [--sizes 4096,65536]     parent and this tree alternated
  python tools/out_tables_bench.py --side [--tree DIR] [--sizes ...]                       one tree, this process, one JSON line

One side measures, on the package of the tree it is given (its own by default), per batch size:
  "mixed"       the device lock-step call of a 48 kHz batch with a rate table alone (a quarter of the streams at each of 48, 24, 16
                and 8 kHz), float, 20 frames per call: ms per step;
  "save","load" whole-batch rnnoise_batch_save_streams_device / load_streams_device on that batch: ms per call;
  "symmetric8k" 8 kHz mu-law legs the only way a tree without output tables has: a batch at 8 kHz, every stream mu-law, the int16 call,
                one frame per call -- K0 one wave per stream;
  "gateway"     48 kHz linear in, 8 kHz mu-law out: the out-rate and out-format tables alone, the int16 call, one frame per call --
                K0 lane = stream above 2,048 streams (a tree without the tables reports none).
The driver runs a fresh process per side and round, parent first then this tree, and both trees' `bench.py` lines (the default one
and --streams 4096 --frames-per-call 1, without the CPU baseline and the parity leg), and prints per figure the median of the rounds
with their min and max.  Device buffers, HIP events on one torch stream; the input is noise resident in HBM.
"""
from __future__ import annotations

import argparse
import json
import lzma
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one_side(a):
    tree = os.path.abspath(a.tree or ROOT)
    sys.path.insert(0, tree)
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    res = {"tree": tree, "lib": capi.LIB_PATH}

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def measure(fn, calls):
        timed(fn, max(1, calls // 4))
        return round(timed(fn, calls), 5)

    for n in (int(v) for v in a.sizes.split(",")):
        row = {}
        g = torch.Generator(device=dev).manual_seed(n)
        # the rate table alone, and the snapshots of that batch
        F = 20
        pcm = (torch.randn((F, n, 480), generator=g, device=dev) * 3000).round()
        out, vad, gains = torch.empty_like(pcm), torch.empty((F, n), device=dev), torch.empty((F, n, 32), device=dev)
        b = capi.Batch(model, n)
        b.set_stream_rates([capi.PCM_RATES[s % 4] for s in range(n)])
        row["mixed"] = round(measure(lambda: b.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), F, h),
                                     a.steps // F) / F, 5)
        snap = torch.empty((n, capi.SNAP_FLOATS), device=dev)
        row["save"] = measure(lambda: b.save_streams_device(snap.data_ptr(), 0, n, h), a.steps)
        row["load"] = measure(lambda: b.load_streams_device(snap.data_ptr(), 0, n, h), a.steps)
        b.close()
        del pcm, out, snap
        # 8 kHz mu-law legs: symmetric, and as the output side of 48 kHz linear legs
        vad, gains = torch.empty((1, n), device=dev), torch.empty((1, n, 32), device=dev)
        b = capi.Batch(model, n)
        b.set_pcm_rate(8000)
        b.set_stream_formats(["ulaw"] * n)
        code = torch.randint(0, 256, (1, n, 160), generator=g, device=dev, dtype=torch.uint8)  # (80 bytes at the front of a row count)
        cout = torch.empty_like(code)
        row["symmetric8k"] = measure(lambda: b.process_device(cout.data_ptr(), code.data_ptr(), vad.data_ptr(), gains.data_ptr(), 1, h,
                                                              s16=True), a.steps)
        b.close()
        if hasattr(capi.Batch, "set_stream_out_rates"):
            b = capi.Batch(model, n)
            b.set_stream_out_rates([8000] * n)
            b.set_stream_out_formats(["ulaw"] * n)
            pcm16 = (torch.randn((1, n, 480), generator=g, device=dev) * 3000).round().to(torch.int16)
            out16 = torch.empty_like(pcm16)
            row["gateway"] = measure(lambda: b.process_device(out16.data_ptr(), pcm16.data_ptr(), vad.data_ptr(), gains.data_ptr(), 1, h,
                                                              s16=True), a.steps)
            b.close()
            del pcm16, out16
        res[f"streams_{n}"] = row
        torch.cuda.empty_cache()
    print(json.dumps(res))


def bench_line(tree, extra, steps):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "10",
                        "--no-cpu-baseline", "--no-parity"] + extra, capture_output=True, text=True, check=True, cwd=tree)
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", action="store_true")
    ap.add_argument("--tree", help="with --side: the tree whose package and library are measured (default: this one)")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200, help="timed calls (frames, for the 20-frame call) per figure")
    ap.add_argument("--bench-steps", type=int, default=60)
    a = ap.parse_args()
    if a.side:
        return one_side(a)
    if not a.parent_tree or not os.path.isdir(a.parent_tree):
        ap.error("--parent-tree: a built checkout of the parent commit (or --side for one tree alone)")
    trees = {"parent": os.path.abspath(a.parent_tree), "change": ROOT}
    got = {}
    for _ in range(a.rounds):
        for name, tree in trees.items():
            env = {k: v for k, v in os.environ.items() if k not in ("RNNOISE_AMD_LIB", "PYTHONPATH")}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", "--tree", tree, "--sizes", a.sizes, "--steps", str(a.steps)],
                               capture_output=True, text=True, check=True, env=env, cwd=tree)
            row = json.loads(r.stdout.strip().splitlines()[-1])
            for size, figures in row.items():
                if size.startswith("streams_"):
                    for k, v in figures.items():
                        got.setdefault(f"{size}.{k}", {}).setdefault(name, []).append(v)
            got.setdefault("bench.default", {}).setdefault(name, []).append(bench_line(tree, [], a.bench_steps))
            got.setdefault("bench.4096x1", {}).setdefault(name, []).append(
                bench_line(tree, ["--streams", "4096", "--frames-per-call", "1"], a.bench_steps))
    res = {"unit": "ms per step or call: [median of the rounds, min, max]", "rounds": a.rounds, "steps": a.steps}
    for key, sides in got.items():
        res[key] = {name: [round(statistics.median(v), 5), min(v), max(v)] for name, v in sides.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
