#!/usr/bin/env python3
"""Cost of the stream snapshots (include/rnnoise_amd.h: rnnoise_batch_save_streams_device / load_streams_device), one JSON line on stdout.

  python tools/snapshot_bench.py [--batch N ...] [--list-rows R] [--reps K] [--warmup W] [--parent-streams P] [--nn-path 1|2]

For every batch size: whole-batch save and load, and at the first size a save and a load of --list-rows random rows, each timed
with HIP events on an otherwise idle stream (median of --reps after --warmup); beside them a device-to-device hipMemcpyAsync of the
snapshot array's byte count in the same process, the yardstick.  Bytes are algorithmic: a save reads and writes one record per row
(2 x 26,496 B); a load reads one and writes the stream's arrays (the whole pitch ring, the decimated ring, the rest of the state,
at 48 kHz no history: 33,576 B).  "parent_way": a loop of rnnoise_batch_export_state / import_state (one stream per call, each a device
drain) over --parent-streams streams of the first batch, wall clock, per stream.
"""
from __future__ import annotations

import argparse
import json
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--list-rows", type=int, default=256)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-streams", type=int, default=256)
    ap.add_argument("--nn-path", type=int, default=None, help="network path of the batches (2: the layer-wise network, whose listed "
                    "tiles a load re-quantises once a frame has run)")
    a = ap.parse_args()
    import torch
    from rnnoise_amd import capi

    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    rec = capi.SNAP_FLOATS * 4
    # what a load writes per stream: pitch ring 2880, decimated ring 1440, synthesis 480, scalars 4, lastg 32, conv1 130, conv2 256,
    # GRU 3 x 384, spectra 962 + 962 + 96 floats (the batches here run at 48 kHz: no history to write)
    load_writes = (2880 + 1440 + 480 + 4 + 32 + 130 + 256 + 3 * 384 + 962 + 962 + 96) * 4
    res = {"unit": "ms per call (median); GB/s = algorithmic bytes / time", "reps": a.reps}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def entry(ms, nbytes):
        return {"ms": round(ms, 4), "GB_per_s": round(nbytes / ms / 1e6, 1)}

    for bi, N in enumerate(a.batch):
        b = capi.Batch(model, N)
        if a.nn_path is not None:
            b.set_nn_path(a.nn_path)
        g = torch.Generator(device=dev).manual_seed(N)
        pcm = (torch.randn((2, N, 480), generator=g, device=dev) * 3000).round()
        out = torch.empty_like(pcm)
        b.process_device(out.data_ptr(), pcm.data_ptr(), 0, 0, 2, h)  # live state (and live state images on the layer-wise path)
        snap, copy = torch.empty((N, capi.SNAP_FLOATS), device=dev), torch.empty((N, capi.SNAP_FLOATS), device=dev)
        torch.cuda.synchronize()
        r = {}
        t_copy = timed(lambda: copy.copy_(snap))
        r["d2d_copy_of_the_snapshot_array"] = entry(t_copy, 2 * N * rec)
        t_save = timed(lambda: b.save_streams_device(snap.data_ptr(), 0, N, h))
        r["save_all"] = entry(t_save, 2 * N * rec)
        t_load = timed(lambda: b.load_streams_device(snap.data_ptr(), 0, N, h))
        r["load_all"] = entry(t_load, N * (rec + load_writes))
        copy_rate = 2 * N * rec / t_copy
        r["save_all_share_of_copy_rate"] = round(2 * N * rec / t_save / copy_rate, 3)
        r["load_all_share_of_copy_rate"] = round(N * (rec + load_writes) / t_load / copy_rate, 3)
        if bi == 0:
            n = min(a.list_rows, N)
            idx = torch.randperm(N, generator=g, device=dev)[:n].to(torch.int32)
            t_ls = timed(lambda: b.save_streams_device(snap.data_ptr(), idx.data_ptr(), n, h))
            t_ll = timed(lambda: b.load_streams_device(snap.data_ptr(), idx.data_ptr(), n, h))
            r[f"save_list_{n}"] = entry(t_ls, 2 * n * rec)
            r[f"load_list_{n}"] = entry(t_ll, n * (rec + load_writes))
            r[f"save_list_{n}_over_save_all"] = round(t_ls / t_save, 4)
            r[f"load_list_{n}_over_load_all"] = round(t_ll / t_load, 4)
            r["rows_over_batch"] = round(n / N, 4)
            # the parent's way: one stream per call, nothing else queued
            P = min(a.parent_streams, N)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            states = [b.export_state(s) for s in range(P)]
            t1 = time.perf_counter()
            for s in range(P):
                b.import_state(s, states[s])
            t2 = time.perf_counter()
            r["parent_way"] = {"streams": P, "export_state_us_per_stream": round((t1 - t0) / P * 1e6, 1),
                               "import_state_us_per_stream": round((t2 - t1) / P * 1e6, 1),
                               "save_all_us_per_stream": round(t_save * 1e3 / N, 4), "load_all_us_per_stream": round(t_load * 1e3 / N, 4),
                               f"save_list_{n}_us_per_stream": round(t_ls * 1e3 / n, 4),
                               f"load_list_{n}_us_per_stream": round(t_ll * 1e3 / n, 4)}
        res[f"batch_{N}"] = r
        del b, snap, copy, pcm, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
