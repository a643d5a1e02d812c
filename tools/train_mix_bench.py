#!/usr/bin/env python3
"""Cost of generating training sequences (include/rnnoise_amd.h: RNNoiseTrainMix), one JSON line on stdout.

  python tools/train_mix_bench.py [--seqs N ...] [--frames T] [--reps K] [--warmup W] [--cpu-seqs C] [--corpus-samples S] [--vad-device]

For every batch size: rnnoise_batch_train_levels_device, rnnoise_batch_train_mix_device and rnnoise_batch_train_features_device over one
sequence of --frames frames per stream, each timed on its own with HIP events on the call's stream (median of --reps after --warmup),
on draws of train_data.draw from three random corpora.  Beside them the same work on this host's CPU: tests/csrc/mix_oracle.c, one
thread, --cpu-seqs sequences (levels, Viterbi VAD and mix timed apart), and rnnoise_amd_train_vad, the host step of the GPU path.
--vad-device: also rnnoise_batch_train_levels_vad_device, the levels launch with the Viterbi VAD in it, beside
what it replaces -- the levels call, the energies to the host, rnnoise_amd_train_vad, the bytes back -- between the same two events.
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
    ap.add_argument("--cpu-seqs", type=int, default=4)
    ap.add_argument("--corpus-samples", type=int, default=1 << 26)
    ap.add_argument("--vad-device", action="store_true", help="also time the levels call with the VAD and the host path it replaces")
    a = ap.parse_args()
    import numpy as np
    import torch

    import mix_oracle as mo
    from rnnoise_amd import capi, train_data

    T = a.frames
    rng = np.random.default_rng(5)
    corpora = [np.clip(np.rint(rng.standard_normal(a.corpus_samples + k) * s), -32768, 32767).astype(np.int16)
               for k, s in enumerate((5000, 2000, 3000))]
    lens = [len(c) for c in corpora]
    res = {"unit": "ms per call (median of reps)", "frames": T, "reps": a.reps}

    # the CPU: one thread, the oracle's plain C
    d = train_data.draw(rng, a.cpu_seqs, lens, T)
    t = [time.perf_counter()]
    lv = [mo.levels(corpora, d.mix[i], T) for i in range(a.cpu_seqs)]
    t.append(time.perf_counter())
    vads = [mo.vad(lv[i][0], d.start_pos[i]) for i in range(a.cpu_seqs)]
    t.append(time.perf_counter())
    for i in range(a.cpu_seqs):
        mo.mix(corpora, d.mix[i], lv[i][1], vads[i], T)
    t.append(time.perf_counter())
    cpu = {k: (t[i + 1] - t[i]) * 1e3 / a.cpu_seqs for i, k in enumerate(("levels", "vad", "mix"))}
    res["cpu_one_thread_ms_per_sequence"] = {k: round(v, 3) for k, v in cpu.items()}

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
        b = capi.Batch(model, N)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        energy, rms = new((N, T)), new((N, 3))
        clean, noisy, target, nf, rec = new((T, N, 480)), new((T, N, 480)), new((T, N)), new((N,), torch.int32), new((T, N, 98))
        d_lp, d_bl = torch.from_numpy(dr.lowpass).to(dev), torch.from_numpy(dr.band_lp).to(dev)
        t_lv, all_lv = timed(lambda: b.train_levels_device(energy.data_ptr(), rms.data_ptr(), ptrs, lens, dr.mix, T, h))
        e = energy.cpu().numpy()
        t0 = time.perf_counter()
        vad = capi.train_vad(e, dr.start_pos)
        t_vad = (time.perf_counter() - t0) * 1e3
        d_vad = torch.from_numpy(vad).to(dev)
        t_mx, all_mx = timed(lambda: b.train_mix_device(clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), nf.data_ptr(), ptrs, lens,
                                                        dr.mix, rms.data_ptr(), d_vad.data_ptr(), T, h))
        t_tf, all_tf = timed(lambda: b.train_features_device(rec.data_ptr(), clean.data_ptr(), noisy.data_ptr(), target.data_ptr(),
                                                             d_lp.data_ptr(), d_bl.data_ptr(), nf.data_ptr(), T, h))
        extra = {}
        if a.vad_device:
            d_v = new((N, T), torch.uint8)
            t_lvv, all_lvv = timed(lambda: b.train_levels_vad_device(energy.data_ptr(), rms.data_ptr(), d_v.data_ptr(), ptrs, lens, dr.mix,
                                                                     dr.start_pos, T, h))
            assert (d_v.cpu().numpy() == vad).all()

            def host_path():
                b.train_levels_device(energy.data_ptr(), rms.data_ptr(), ptrs, lens, dr.mix, T, h)
                return torch.from_numpy(capi.train_vad(energy.cpu().numpy(), dr.start_pos)).to(dev)
            t_hp, all_hp = timed(host_path)
            extra = {"levels_vad_ms": round(t_lvv, 3), "levels_vad_runs": [round(v, 3) for v in all_lvv],
                     "levels_copy_host_vad_copy_ms": round(t_hp, 3), "levels_copy_host_vad_copy_runs": [round(v, 3) for v in all_hp],
                     "vad_epilogue_ms": round(t_lvv - t_lv, 3)}
            del d_v
        cpu_ms = (cpu["levels"] + cpu["mix"]) * N
        res[f"seqs_{N}"] = {
            "levels_ms": round(t_lv, 3), "mix_ms": round(t_mx, 3), "train_features_ms": round(t_tf, 3),
            "levels_runs": [round(v, 3) for v in all_lv], "mix_runs": [round(v, 3) for v in all_mx],
            "train_features_runs": [round(v, 3) for v in all_tf],
            "host_train_vad_ms_one_thread": round(t_vad, 3),
            "levels_plus_mix_over_train_features": round((t_lv + t_mx) / t_tf, 3),
            "sequences_per_s_levels_plus_mix": round(N / (t_lv + t_mx) * 1e3, 1),
            "sequences_per_s_all_three": round(N / (t_lv + t_mx + t_tf) * 1e3, 1),
            "cpu_one_thread_levels_plus_mix_ms": round(cpu_ms, 1),
            "cpu_over_gpu_levels_plus_mix": round(cpu_ms / (t_lv + t_mx), 1), **extra}
        b.close()
        del energy, rms, clean, noisy, target, nf, rec, d_vad
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
