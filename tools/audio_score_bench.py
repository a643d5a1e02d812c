#!/usr/bin/env python3
"""Cost of the audio score call (include/rnnoise_amd_score.h: rnnoise_amd_audio_score_device).

  python tools/audio_score_bench.py [--frames T] [--warmup W] [--rounds R] [--sizes N,...] [--out FILE]

At 4,096 and 65,536 rows, over T-frame sequences of random PCM resident in HBM, HIP events on one torch stream around ONE call
(one launch) that scores frames 3 .. T - 1 (first = 3, so that a delay of 961 is allowed beside 960):
  layout   frames: [T][N][480], what the training mix leaves and process_device takes; streams: [N][T * 480]
  delay    960 (every granule one 16-byte load) against 961 (ref / in through four dword loads)
  records  without and with frame_terms
Per case: ms per scored frame -- the median of R rounds with min - max --, the achieved bytes per second (3 x 1,920 B per row and
scored frame over that time) and its share of the 6.29 TB/s a float4 copy reaches on this part; beside it the time per frame of
rnnoise_batch_process_device on the same planes in the same job, and the share of an evaluation pass (process + score) that the
scoring is.  Writes the table to FILE (default profiles/audio_score_bench.txt) and prints it.  Without a GPU it fails: a number that
was not measured is not reported.
"""
from __future__ import annotations

import argparse
import lzma
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BPS = 6.29e12  # measured float4 copy rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_score_bench.txt"))
    a = ap.parse_args()
    import torch
    from rnnoise_amd import audio_score, capi

    if not torch.cuda.is_available():
        sys.exit("audio_score_bench: no GPU: nothing measured")
    blob = lzma.decompress(open(os.path.join(ROOT, "tests", "golden", "default.blob.xz"), "rb").read())
    model = capi.Model(blob)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    T, first = a.frames, 3
    scored = T - first
    lines = [f"audio score call: ms per scored frame, median of {a.rounds} rounds (min - max); {T}-frame sequences, frames {first}..{T - 1} scored in one launch",
             f"bytes: 3 x 1,920 B per row and scored frame; HBM: share of {HBM_COPY_BPS / 1e12:.2f} TB/s (float4 copy); process: rnnoise_batch_process_device "
             "ms per frame, same planes, same job; share: score / (process + score)", "",
             f"{'rows':>6} {'layout':<8} {'delay':>5} {'records':<7} {'ms/frame':>9} {'min':>9} {'max':>9} {'TB/s':>7} {'HBM':>6} {'process':>9} {'share':>7}"]

    def timed(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) / per

    for n in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator(device=dev).manual_seed(n)
        clean = (torch.rand((T, n, 480), generator=g, device=dev) - .5) * 20000
        noisy = clean + (torch.rand((T, n, 480), generator=g, device=dev) - .5) * 4000
        out = torch.empty_like(noisy)
        batch = capi.Batch(model, n)
        process = lambda: batch.process_device(out.data_ptr(), noisy.data_ptr(), 0, 0, T, st.cuda_stream)
        for _ in range(a.warmup):
            process()
        torch.cuda.synchronize()
        proc = statistics.median(timed(process, T) for _ in range(a.rounds))  # (out now holds a denoised plane)
        batch.close()
        sums = torch.zeros((n, 8), dtype=torch.float64, device=dev)
        terms = torch.zeros((n, T, 8), dtype=torch.float64, device=dev)
        for layout in ("frames", "streams"):
            if layout == "frames":
                planes, (fs, rs) = (clean, noisy, out), audio_score.layout_frames(n)
            else:  # one plane at a time: the frame-major one goes as its stream-major copy arrives
                clean, noisy, out = (p.transpose(0, 1).contiguous() for p in (clean, noisy, out))
                planes, (fs, rs) = (clean, noisy, out), audio_score.layout_streams(T)
            ptrs = [(p.data_ptr(), fs, rs) for p in planes]
            cases = [(960, 0), (960, terms.data_ptr()), (961, 0)]
            calls = [(lambda d=d, ft=ft: audio_score.score_device(sums.data_ptr(), *ptrs, n, 0, T, first, d, ft, T, 0, st.cuda_stream)) for d, ft in cases]
            for fn in calls:
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            got = [[] for _ in calls]
            for _ in range(a.rounds):  # (the cases alternate within a round)
                for k, fn in enumerate(calls):
                    got[k].append(timed(fn, scored))
            for (d, ft), v in zip(cases, got):
                ms = statistics.median(v)
                bps = 3 * 1920 * n / (ms * 1e-3)
                lines.append(f"{n:>6} {layout:<8} {d:>5} {'yes' if ft else 'no':<7} {ms:>9.5f} {min(v):>9.5f} {max(v):>9.5f} {bps / 1e12:>7.3f} "
                             f"{100 * bps / HBM_COPY_BPS:>5.1f}% {proc:>9.5f} {100 * ms / (ms + proc):>6.2f}%")
        del clean, noisy, out, sums, terms, planes
        torch.cuda.empty_cache()
    model.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
