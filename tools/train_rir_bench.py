#!/usr/bin/env python3
"""Cost of the RIR filtering of training sequences (include/rnnoise_amd.h: RNNoiseTrainRir), one JSON line on
stdout.

  python tools/train_rir_bench.py [--seqs N ...] [--frames T] [--reps K] [--warmup W] [--work-mb M ...] [--cpu-seqs C] [--rirs R]

For every batch size: rnnoise_batch_train_levels_device, rnnoise_batch_train_mix_device, rnnoise_batch_train_rir_device (every sequence
filtered, at each workspace size of --work-mb) and rnnoise_batch_train_features_device over one sequence of --frames frames per stream,
each timed on its own with HIP events on the call's stream (median of --reps after --warmup); rnnoise_batch_train_rir_load_device per
response.  Beside them the filter on this host's CPU: tests/csrc/rir_oracle.c, one thread, --cpu-seqs sequences (clean and noisy).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--work-mb", type=int, nargs="+", default=[1024, 8192])
    ap.add_argument("--cpu-seqs", type=int, default=2)
    ap.add_argument("--rirs", type=int, default=16)
    ap.add_argument("--corpus-samples", type=int, default=1 << 26)
    a = ap.parse_args()
    import numpy as np
    import torch

    import rir_oracle as ro
    from rnnoise_amd import capi, train_data

    T = a.frames
    rng = np.random.default_rng(5)
    corpora = [np.clip(np.rint(rng.standard_normal(a.corpus_samples + k) * s), -32768, 32767).astype(np.int16)
               for k, s in enumerate((5000, 2000, 3000))]
    lens = [len(c) for c in corpora]
    responses = [ro.response(12000 + 1000 * k, k) for k in range(a.rirs)]
    blocks = -(-T * 480 // ro.BLOCK)
    res = {"unit": "ms per call (median of reps)", "frames": T, "reps": a.reps, "rirs": a.rirs, "blocks_per_signal": blocks}

    # the CPU: one thread, the oracle's plain C
    spec = [ro.load(responses[0], 0), ro.load(responses[0], 1)]
    x = [ro.signal(T, k) for k in range(2 * a.cpu_seqs)]
    t0 = time.perf_counter()
    for k in range(a.cpu_seqs):
        ro.filter(x[2 * k], spec[1])
        ro.filter(x[2 * k + 1], spec[0])
    cpu = (time.perf_counter() - t0) * 1e3 / a.cpu_seqs
    res["cpu_one_thread_ms_per_sequence"] = round(cpu, 1)

    model = capi.Model(lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read()))
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    d_corp = [torch.from_numpy(c).to(dev) for c in corpora]
    ptrs = [c.data_ptr() for c in d_corp]

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
        return statistics.median(ms), ms

    for N in a.seqs:
        dr = train_data.draw(rng, N, lens, T)
        mix = dr.mix.copy()
        mix["clip"] = mix["quantize"] = 0
        rec = np.zeros(N, capi.RIR_DTYPE)
        rec["rir_id"] = np.arange(N) % a.rirs
        rec["clip"], rec["quantize"] = dr.mix["clip"], dr.mix["quantize"]
        b = capi.Batch(model, N)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        rows = np.zeros((a.rirs, capi.RIR_MAX), np.float32)
        for k, r in enumerate(responses):
            rows[k, :len(r)] = r
        d_rows, spectra = torch.from_numpy(rows).to(dev), new((a.rirs, 2, capi.RIR_FFT, 2))
        t_ld, _ = timed(lambda: b.train_rir_load_device(spectra.data_ptr(), d_rows.data_ptr(), [len(r) for r in responses], h))
        energy, rms = new((N, T)), new((N, 3))
        clean, noisy, target, nf, out = new((T, N, 480)), new((T, N, 480)), new((T, N)), new((N,), torch.int32), new((T, N, 98))
        d_lp, d_bl = torch.from_numpy(dr.lowpass).to(dev), torch.from_numpy(dr.band_lp).to(dev)
        t_lv, all_lv = timed(lambda: b.train_levels_device(energy.data_ptr(), rms.data_ptr(), ptrs, lens, mix, T, h))
        d_vad = torch.from_numpy(capi.train_vad(energy.cpu().numpy(), dr.start_pos)).to(dev)
        t_mx, all_mx = timed(lambda: b.train_mix_device(clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), nf.data_ptr(), ptrs, lens,
                                                        mix, rms.data_ptr(), d_vad.data_ptr(), T, h))
        units = 2 * blocks * N
        r = {"levels_ms": round(t_lv, 3), "mix_ms": round(t_mx, 3), "levels_runs": [round(v, 3) for v in all_lv],
             "mix_runs": [round(v, 3) for v in all_mx], "rir_load_ms_per_response": round(t_ld / a.rirs, 4), "rir_units": units}
        for mb in a.work_mb:
            work = new((mb << 20,), torch.uint8)
            t_rir, all_rir = timed(lambda: b.train_rir_device(clean.data_ptr(), noisy.data_ptr(), spectra.data_ptr(), a.rirs, rec,
                                                              work.data_ptr(), mb << 20, T, h))
            r[f"rir_ms_work_{mb}_mb"] = round(t_rir, 3)
            r[f"rir_runs_work_{mb}_mb"] = [round(v, 3) for v in all_rir]
            r[f"rir_us_per_unit_work_{mb}_mb"] = round(t_rir * 1e3 / units, 3)
            del work
            torch.cuda.empty_cache()
        t_tf, all_tf = timed(lambda: b.train_features_device(out.data_ptr(), clean.data_ptr(), noisy.data_ptr(), target.data_ptr(),
                                                             d_lp.data_ptr(), d_bl.data_ptr(), nf.data_ptr(), T, h))
        best = min(r[f"rir_ms_work_{mb}_mb"] for mb in a.work_mb)
        # per unit: the gather (0.25 MB), T and T2 written and read (4 x 0.5 MB), the spectrum (0.5 MB), the block stored (0.125 MB)
        r.update({"train_features_ms": round(t_tf, 3), "train_features_runs": [round(v, 3) for v in all_tf],
                  "rir_over_levels_mix_features": round(best / (t_lv + t_mx + t_tf), 3),
                  "rir_gb_moved": round(units * 2.875 * 2 ** 20 / 1e9, 1),
                  "rir_tb_per_s": round(units * 2.875 * 2 ** 20 / 1e12 / (best * 1e-3), 3),
                  "sequences_per_s_with_rir": round(N / (t_lv + t_mx + best + t_tf) * 1e3, 1),
                  "cpu_one_thread_rir_ms": round(cpu * N, 1), "cpu_over_gpu_rir": round(cpu * N / best, 1)})
        res[f"seqs_{N}"] = r
        b.close()
        del energy, rms, clean, noisy, target, nf, out, d_vad, spectra, d_rows
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
