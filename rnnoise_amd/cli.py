"""Multi-stream file front end: N RAW s16 48 kHz mono files in, N denoised
files out, one GPU batch.

Per file the semantics are those of the reference's examples/rnnoise_demo.c:52-61: samples are
fed unscaled (+-32768 range), the first output frame is dropped, the float result is cast to
short by truncation, a trailing partial frame is ignored.  The samples cross PCIe as int16 both
ways (rnnoise_batch_process_s16: the two conversions of rnnoise_demo.c:56,58 run on the device).  Files of different lengths share the
batch; a stream whose file has ended is fed zeros and produces no more output.

  python -m rnnoise_amd.cli denoise --model weights_blob.bin --out-dir out  a.raw b.raw ...

--atten-limit-db, --vad-gate and --vad-hold apply the per-stream suppression controls of include/rnnoise_amd.h
(rnnoise_batch_set_stream_controls) to every file: a floor on the band gains, and a VAD gate with a hold time.
--rates 8000,48000,16000 gives every file its own sample rate (one per input, each at most --rate): one mixed-rate batch
(rnnoise_batch_set_stream_rates), every file read and written at its own rate.
--formats s16,ulaw,alaw gives every file its own sample format (one per input): a G.711 file is raw companded bytes, one per sample
(the .ul / .al convention), expanded and compressed on the device (rnnoise_batch_set_stream_formats); its output is written the same way.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import capi, g711

FRAME = capi.FRAME
SILENCE = {g711.ULAW: 0xFF, g711.ALAW: 0xD5}  # the code of sample 0 (A-law: of +8, its smallest magnitude)


def denoise_files(model_blob: bytes, inputs, out_dir: str, chunk_frames: int = 100, device: int = 0,
                  vad_csv: bool = False, rate: int = 48000, atten_limit_db=None, vad_gate: float = 0.0, vad_hold: int = 0, rates=None,
                  formats=None):
    """Streams the files through the batch chunk by chunk: at most `chunk_frames` frames of every file are in host memory
    at a time (two staging buffers, reused), whatever the file lengths.  rate: the files' sample rate (48000, 24000, 16000 or
    8000: 10 ms frames of 480 * rate // 48000 samples, resampled on the device).  atten_limit_db / vad_gate / vad_hold: the suppression
    controls of every file (capi.controls_table); all unset, the batch has no control table.  rates: one sample rate per file, none
    above `rate` (a mixed-rate batch: capi.Batch.set_stream_rates); a file's frames fill the front of its rows.  formats: one of
    "s16", "ulaw", "alaw" per file (capi.Batch.set_stream_formats): a companded file holds one byte per sample, which fill the front of
    its int16 rows as bytes, and is written back the same way."""
    os.makedirs(out_dir, exist_ok=True)
    FRAME = capi.FRAME * rate // 48000
    if rates is not None and len(rates) != len(inputs):
        raise ValueError(f"{len(rates)} rates for {len(inputs)} files")
    frame_of = [capi.FRAME * r // 48000 for r in rates] if rates is not None else [FRAME] * len(inputs)  # samples per 10 ms of each file
    if formats is not None and len(formats) != len(inputs):
        raise ValueError(f"{len(formats)} formats for {len(inputs)} files")
    width = [1 if g711.code(f) else 2 for f in formats] if formats is not None else [2] * len(inputs)  # bytes per sample of each file
    n_frames = [os.path.getsize(p) // w // fl for p, fl, w in zip(inputs, frame_of, width)]  # partial tail dropped (rnnoise_demo.c:55)
    N, T = len(inputs), max(n_frames + [0])
    model = capi.Model(model_blob)
    batch = capi.Batch(model, N, device=device)
    if rate != 48000:
        batch.set_pcm_rate(rate)
    if rates is not None:
        batch.set_stream_rates(rates)
    if formats is not None:
        batch.set_stream_formats(formats)
    if atten_limit_db is not None or vad_gate or vad_hold:
        batch.set_stream_controls(capi.controls_table(N, atten_limit_db, vad_gate, vad_hold))
    ins = [open(p, "rb") for p in inputs]
    outs = [open(os.path.join(out_dir, os.path.basename(p) + ".denoised.raw"), "wb") for p in inputs]
    vfs = [open(os.path.join(out_dir, os.path.basename(p) + ".vad.csv"), "w") for p in inputs] if vad_csv else None
    # every file's chunk is ONE contiguous run of the staging buffer, [N][chunk frames * FRAME], which the batch reads and writes where
    # it lies (capi.Batch.set_pcm_layout: frames FRAME apart, files a whole chunk apart) -- no interleaving into frame-major rows here.
    # `chunk` / `out` below are (frames, N, FRAME) VIEWS of those runs
    cf = min(chunk_frames, max(T, 1))
    batch.set_pcm_layout(FRAME, cf * FRAME)
    buf, obuf = batch.pcm_array(cf, np.int16), batch.pcm_array(cf, np.int16)
    rows8 = lambda a: a.view(np.uint8)  # the same rows as bytes (a companded file's view): (frames, N, 2 * FRAME)
    for t0 in range(0, T, chunk_frames):
        tn = min(chunk_frames, T - t0)
        chunk = buf[:tn]
        chunk[:] = 0  # a stream whose file has ended is fed silence and produces no more output
        for s in range(N):  # (silence of a companded stream is its law's zero code, not a zero byte: 0x00 is a full-scale sample)
            if width[s] == 1:
                rows8(chunk)[:, s, :frame_of[s]] = SILENCE[g711.code(formats[s])]
        for s, f in enumerate(ins):
            k = max(0, min(tn, n_frames[s] - t0))
            if k:
                if width[s] == 1:
                    rows8(chunk)[:k, s, :frame_of[s]] = np.frombuffer(f.read(k * frame_of[s]), dtype=np.uint8).reshape(k, frame_of[s])
                    continue
                x = np.frombuffer(f.read(k * frame_of[s] * 2), dtype=np.int16)
                chunk[:k, s, :frame_of[s]] = x.reshape(k, frame_of[s])
        out, vad, _ = batch.process_s16(chunk, want_gains=False, out=obuf[:tn])
        for s in range(N):
            k = max(0, min(tn, n_frames[s] - t0))
            first = 1 if t0 == 0 else 0  # the demo drops the first output frame (rnnoise_demo.c:59-60)
            if k > first and width[s] == 1:
                outs[s].write(rows8(out)[first:k, s, :frame_of[s]].tobytes())
            elif k > first:
                outs[s].write(out[first:k, s, :frame_of[s]].tobytes())  # (the demo's truncating (short) cast was done on the device)
            if vfs and k:
                vfs[s].write("".join(f"{v:.6f}\n" for v in vad[:k, s]))
    for f in ins + outs + (vfs or []):
        f.close()
    batch.close()
    model.close()
    return n_frames


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("denoise")
    p.add_argument("--model", required=True, help='"DNNw" weight blob (src/write_weights.c format)')
    p.add_argument("--out-dir", required=True)
    p.add_argument("--chunk-frames", type=int, default=100)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--vad-csv", action="store_true")
    p.add_argument("--rate", type=int, default=48000, choices=capi.PCM_RATES, help="sample rate of the RAW files")
    p.add_argument("--rates", type=lambda v: [int(x) for x in v.split(",")], default=None,
                   help="comma list, one sample rate per input file, each at most --rate: a mixed-rate batch")
    p.add_argument("--formats", type=lambda v: v.split(","), default=None,
                   help="comma list, one of s16 | ulaw | alaw per input file: G.711 files are raw bytes, one per sample")
    p.add_argument("--atten-limit-db", type=float, default=None,
                   help="attenuation limit in dB: no band is suppressed by more (a floor on the band gains); default none")
    p.add_argument("--vad-gate", type=float, default=0.0, help="VAD threshold in [0, 1] below which output is muted (0: no gate)")
    p.add_argument("--vad-hold", type=int, default=0, help="frames the VAD gate stays open after the last voice frame")
    p.add_argument("inputs", nargs="+")
    a = ap.parse_args(argv)
    n = denoise_files(open(a.model, "rb").read(), a.inputs, a.out_dir, a.chunk_frames, a.device, a.vad_csv, a.rate,
                      a.atten_limit_db, a.vad_gate, a.vad_hold, a.rates, a.formats)
    print(f"denoised {len(a.inputs)} streams, {sum(n)} frames")


if __name__ == "__main__":
    main(sys.argv[1:])
