#!/usr/bin/env python3
"""Cost of the STOI call (include/rnnoise_amd_stoi.h: rnnoise_amd_stoi_device).

  python tools/stoi_bench.py [--frames T] [--warmup W] [--rounds R] [--sizes N,...] [--out FILE]

At 128 and 1,024 rows of T = 2,000 frames, planes [T][N][480] of noise under a speech-like envelope resident in HBM (so that
silent-frame removal has frames to remove), HIP events on one torch stream around ONE call (five launches) with first = 2 and
delay = 960, with and without the noisy plane; scratch for all rows at once.  Beside it, on the same planes in the same job: one
rnnoise_amd_audio_score_device call with frame records, and rnnoise_batch_process_device denoising the noisy plane.  Per case: ms per
call -- the median of R rounds with min - max.  Writes the table to FILE (default profiles/stoi_bench.txt) and prints it.  Without a
GPU it fails: a number that was not measured is not reported.  Which stage dominates: run this file under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/stoi_bench.py --sizes 128 --rounds 3 --out /dev/null`, then
`python tools/stoi_kernel_times.py DIR` makes profiles/stoi_bench_kernels.txt of the trace.
"""
from __future__ import annotations

import argparse
import lzma
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="128,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_bench.txt"))
    a = ap.parse_args()
    import torch
    from rnnoise_amd import audio_score, capi, stoi

    if not torch.cuda.is_available():
        sys.exit("stoi_bench: no GPU: nothing measured")
    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    T, first, delay = a.frames, 2, 960
    lines = [f"STOI call: ms per call, median of {a.rounds} rounds (min - max); {T}-frame sequences [T][N][480], first {first}, delay {delay}, five launches",
             "stoi: with the noisy plane; stoi-out: without it (the out side alone); score: one rnnoise_amd_audio_score_device call with frame records; process: rnnoise_batch_process_device over the T frames; same planes, same job",
             "",
             f"{'rows':>6} {'what':<8} {'ms/call':>10} {'min':>10} {'max':>10} {'ms/row':>8} {'kept':>6} {'scratch MB':>10}"]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for n in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        t = torch.arange(T * 480, device=dev, dtype=torch.float32).view(T, 1, 480) / 48000.0
        phase = torch.rand((1, n, 1), generator=g, device=dev) * 6.2831853
        env = torch.clamp(torch.sin(6.2831853 * 3.0 * t + phase), min=0.0) ** 2 + 1e-4
        clean = torch.randn((T, n, 480), generator=g, device=dev) * env * 3000
        del env, t
        noisy = clean + torch.randn((T, n, 480), generator=g, device=dev) * 1000
        out = torch.empty_like(noisy)
        batch = capi.Batch(model, n)
        process = lambda: batch.process_device(out.data_ptr(), noisy.data_ptr(), 0, 0, T, st.cuda_stream)
        for _ in range(a.warmup):
            process()
        torch.cuda.synchronize()
        proc = [timed(process) for _ in range(a.rounds)]  # (out now holds a denoised plane)
        batch.close()
        fs, rs = audio_score.layout_frames(n)
        ptrs = [(p.data_ptr(), fs, rs) for p in (clean, noisy, out)]
        sums = torch.zeros((n, 8), dtype=torch.float64, device=dev)
        terms = torch.zeros((n, T, 8), dtype=torch.float64, device=dev)
        score = lambda: audio_score.score_device(sums.data_ptr(), *ptrs, n, 0, T, first, delay, terms.data_ptr(), T, 0, st.cuda_stream)
        for _ in range(a.warmup):
            score()
        torch.cuda.synchronize()
        sc = [timed(score) for _ in range(a.rounds)]
        del terms
        nbytes = stoi.workspace(n, T)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        res = torch.zeros((n, 8), dtype=torch.float64, device=dev)
        cases = [("stoi", ptrs[1]), ("stoi-out", None)]  # with the noisy plane, and the out side alone
        calls = [(lambda inp=inp: stoi.score_device(res.data_ptr(), scratch.data_ptr(), nbytes, ptrs[0], inp, ptrs[2], n, T, first, delay, 0,
                                                    st.cuda_stream)) for _, inp in cases]
        for fn in calls:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        got = [[] for _ in calls]
        for _ in range(a.rounds):  # (the cases alternate within a round)
            for k, fn in enumerate(calls):
                got[k].append(timed(fn))
        kept = float(res[:, 7].mean().item())
        for (name, _), v in zip(cases, got):
            ms = statistics.median(v)
            lines.append(f"{n:>6} {name:<8} {ms:>10.3f} {min(v):>10.3f} {max(v):>10.3f} {ms / n:>8.4f} {kept:>6.0f} {nbytes / 1e6:>10.1f}")
        for name, v in (("score", sc), ("process", proc)):
            lines.append(f"{n:>6} {name:<8} {statistics.median(v):>10.3f} {min(v):>10.3f} {max(v):>10.3f}")
        del clean, noisy, out, sums, scratch, res
        torch.cuda.empty_cache()
    model.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
