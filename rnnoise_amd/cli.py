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
--out-rate HZ and --out-format s16|ulaw|alaw write every file at another rate or in another format than it was read in (at most
--rate): the legs leave the batch in that shape (rnnoise_batch_set_stream_out_rates, _out_formats), and a WAV output's header says so.
An input that starts with RIFF....WAVE is read as a WAV file (rnnoise_amd/wav.py: PCM16, A-law or mu-law, 1 to 8 channels, 8 to 48 kHz):
its rate, format and channel count come from its header, each channel is one stream, its samples cross the batch interleaved as they lie
in the file (rnnoise_batch_set_pcm_channels), and the output is <name>.denoised.wav with the input's header fields.
--link-channels gives the channels of every multichannel WAV file one suppression (rnnoise_batch_set_gain_link): per frame and band
the smallest gain of the file's non-silent channels, and one VAD for the gate, so that the stereo image stays put.  Mono inputs are
unaffected.

Training data (the reference's src/dump_features.c; rnnoise_amd/train_data.py): COUNT sequences of 98-float records from three RAW
s16 48 kHz mono corpora, each uploaded once, everything else on the device:

  python -m rnnoise_amd.cli dump-features --model weights_blob.bin speech.pcm noise.pcm fgnoise.pcm out.f32 COUNT
--rir-list FILE is the reference's -rir_list: FILE names one room impulse response per line (raw float32 at 48 kHz, of which the first
32768 samples count); half of the sequences are filtered with one of them before clipping and quantisation.

What a blob costs on such a file, in the reference trainer's loss (rnnoise_amd/evaluate.py; rnnoise_batch_eval_records): the network as
it ships over every whole sequence of the file, one JSON line with the trainer's three means per model:

  python -m rnnoise_amd.cli eval-records validation.f32 --model weights_blob.bin [--model other.bin ...]

From the trainer's checkpoint to the served blob (rnnoise_amd/export.py, float_net.py):

  python -m rnnoise_amd.cli export ckpt.pth out.blob [--densities R,Z,N] [--pack]
  python -m rnnoise_amd.cli eval-records validation.f32 --model out.blob --checkpoint ckpt.pth
  python -m rnnoise_amd.cli denoise --checkpoint ckpt.pth --out-dir out a.raw ...
  python -m rnnoise_amd.cli denoise --checkpoint ckpt.pth --float-net native --model a.blob --out-dir out a.raw ...
export writes the "DNNw" blob the reference's exporter and writer make of the checkpoint, byte for byte (--densities: block-sparsified
first, as the trainer does it; --pack: the GPU-native RNPK form).  eval-records --checkpoint scores the float checkpoint beside the
blobs with the same scoring code, and prints every blob's difference to it and the 32 per-band means of the gain loss of each.
denoise --checkpoint runs the float network between the split calls, as --torch-net runs a TorchScript file; without --model the DSP's
batch is built on the blob exported from that checkpoint.

What a blob, a checkpoint or a TorchScript net does to the AUDIO (rnnoise_amd/evaluate.py: evaluate_audio): COUNT
training sequences are generated on the device as dump-features generates them, denoised, and scored against their clean signals by
librnnoise_amd_score.so -- a table of SNR, SI-SDR and segmental SNR in dB per model, and every later model's difference to the first:

  python -m rnnoise_amd.cli eval-audio speech.pcm noise.pcm fgnoise.pcm --model a.blob [--model b.blob] [--checkpoint ckpt.pth]
         [--torch-net net.pt] --count N [--frames T] [--rir-list FILE] [--seed S] [--streams N] [--stoi]

Training (rnnoise_amd/train.py): the loop of the reference's torch/rnnoise/train_rnnoise.py with its options, the loss
and its gradient computed by librnnoise_amd_train.so in the doubles eval-records prints; one checkpoint per epoch under
OUT/checkpoints/, in the reference's format, and one line per epoch with the three means:

  python -m rnnoise_amd.cli train records.f32 OUT [--epochs N] [--batch-size B] [--sequence-length T] [--lr R] [--lr-decay D]
         [--gamma G] [--sparse] [--initial-checkpoint ckpt.pth] [--cond-size C] [--gru-size H] [--suffix S] [--seed S]
  python -m rnnoise_amd.cli train OUT --online speech.pcm noise.pcm fgnoise.pcm --sequences-per-epoch N [--rir-list FILE] [...]
--online trains on fresh sequences every epoch, generated on the device as dump-features generates them and never written to a file.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import capi, g711, wav

FRAME = capi.FRAME
SILENCE = {g711.ULAW: 0xFF, g711.ALAW: 0xD5}  # the code of sample 0 (A-law: of +8, its smallest magnitude)


def _describe(path, rate, fmt):
    """what the batch needs to know of one input: a WAV file's header gives rate, format and channel count; a RAW file is mono at
    the rate and in the format the caller names"""
    if wav.is_wav(path):
        info = wav.read_info(path)
        if fmt is not None and fmt != info.codec:
            raise ValueError(f"{path}: the header says {info.codec}, --formats says {fmt}")
        return dict(path=path, wav=info, channels=info.channels, rate=info.rate, codec=info.codec, width=info.width,
                    offset=info.data_offset, size=info.data_bytes)
    codec = fmt if fmt is not None else "s16"
    return dict(path=path, wav=None, channels=1, rate=rate, codec=codec, width=1 if g711.code(codec) else 2, offset=0,
                size=os.path.getsize(path))


def out_info(info: wav.WavInfo, out_rate=None, out_format=None) -> wav.WavInfo:
    """the header fields of the output of a WAV input under --out-rate / --out-format: the input's, with the rate and the format
    replaced where one is given"""
    return info._replace(rate=out_rate or info.rate, codec=out_format or info.codec)


def denoise_files(model_blob: bytes, inputs, out_dir: str, chunk_frames: int = 100, device: int = 0,
                  vad_csv: bool = False, rate: int = 48000, atten_limit_db=None, vad_gate: float = 0.0, vad_hold: int = 0, rates=None,
                  formats=None, link_channels: bool = False, out_rate=None, out_format=None, torch_net=None, max_store_gb: float = 4.0,
                  checkpoint=None, float_net: str = "torch"):
    """Streams the files through the batch chunk by chunk: at most `chunk_frames` frames of every file are in host memory
    at a time (two staging buffers, reused), whatever the file lengths.  rate: the files' sample rate (48000, 32000, 24000, 16000 or
    8000: 10 ms frames of 480 * rate // 48000 samples, resampled on the device).  atten_limit_db / vad_gate / vad_hold: the suppression
    controls of every file (capi.controls_table); all unset, the batch has no control table.  rates: one sample rate per file, none
    above `rate` (a mixed-rate batch: capi.Batch.set_stream_rates); a file's frames fill the front of its rows.  formats: one of
    "s16", "ulaw", "alaw" per file (capi.Batch.set_stream_formats): a companded file holds one byte per sample, which fill the front of
    its int16 rows as bytes, and is written back the same way.
    An input that starts with RIFF....WAVE is a WAV file (rnnoise_amd/wav.py): its header gives its rate, its format and its channel
    count, every channel is one stream, and its samples go through the batch interleaved as they lie in the file
    (capi.Batch.set_pcm_channels) into <name>.denoised.wav under the input's header fields.  The inputs are grouped by channel count,
    one batch per distinct count (a RAW file is mono).  link_channels: the channels of each multichannel file form one link group
    (capi.Batch.set_gain_link with the file's channel count).  out_rate / out_format: the rate (at most `rate`) and the format every
    output is written in where it is not the input's (capi.Batch.set_stream_out_rates, set_stream_out_formats); a frame then has
    480 * out_rate // 48000 samples on the way out.
    torch_net: a TorchScript file whose module maps features [N, T, 65] to (gains [N, T, 32], vad [N, T, 1]); it takes the place of
    the blob's network between the split calls (capi.Batch.analyze / synthesize), on the batch's device.  Each group of files then
    goes through ONE pair, whole -- a module's state need not survive a call -- and the call is refused (ValueError, before anything
    runs) where the pending frames would need more than max_store_gb GiB of device memory (capi.split_frame_bytes).
    checkpoint: a trainer checkpoint instead: rnnoise_amd.float_net's streaming module on the batch's device goes the same way (reset
    in front of every group of files); max_store_gb applies.  float_net: what runs that checkpoint's network -- "torch": the module;
    "native": rnnoise_amd.fnet.FloatNetRuntime on librnnoise_amd_fnet.so, any cond_size / gru_size the library takes.
    Returns the frames of every input."""
    os.makedirs(out_dir, exist_ok=True)
    if rates is not None and len(rates) != len(inputs):
        raise ValueError(f"{len(rates)} rates for {len(inputs)} files")
    if formats is not None and len(formats) != len(inputs):
        raise ValueError(f"{len(formats)} formats for {len(inputs)} files")
    files = [_describe(p, rates[i] if rates is not None else rate, formats[i] if formats is not None else None)
             for i, p in enumerate(inputs)]
    for d in files:
        if d["rate"] > rate:
            raise ValueError(f"{d['path']}: {d['rate']} Hz is above the batch's rate {rate} (--rate)")
        d["frame"] = capi.FRAME * d["rate"] // 48000  # samples per 10 ms and channel
        d["n_frames"] = d["size"] // (d["width"] * d["channels"]) // d["frame"]  # partial tail dropped (rnnoise_demo.c:55)
        # the way out: the input's rate and format unless --out-rate / --out-format say otherwise
        d["out_rate"], d["out_codec"] = out_rate or d["rate"], out_format or d["codec"]
        if d["out_rate"] > rate:
            raise ValueError(f"{d['path']}: output at {d['out_rate']} Hz is above the batch's rate {rate} (--rate)")
        d["out_frame"] = capi.FRAME * d["out_rate"] // 48000
        d["out_width"] = 1 if g711.code(d["out_codec"]) else 2
    groups = {}
    for d in files:
        groups.setdefault(d["channels"], []).append(d)
    net = None
    if torch_net is not None and checkpoint is not None:
        raise ValueError("--torch-net and --checkpoint both name the network")
    if float_net not in ("torch", "native"):
        raise ValueError(f'float_net: "torch" or "native", not {float_net!r}')
    if float_net == "native" and checkpoint is None:
        raise ValueError("--float-net native runs a --checkpoint")
    if torch_net is not None or checkpoint is not None:
        for channels, group in groups.items():
            frames, n = max([d["n_frames"] for d in group] + [0]), len(group) * channels
            need = frames * capi.split_frame_bytes(n)
            if need > max_store_gb * 2 ** 30:
                raise ValueError(f"--torch-net / --checkpoint: {frames} pending frames of {n} streams need {need / 2 ** 30:.2f} GiB of device memory, "
                                 f"above --max-store-gb {max_store_gb}")
        if checkpoint is not None and float_net == "native":
            from . import fnet
            net = fnet.FloatNetRuntime(checkpoint, device=device)
        elif checkpoint is not None:
            from . import float_net as float_net_module
            net = float_net_module.load_checkpoint(checkpoint, device=f"cuda:{device}")
        else:
            import torch
            net = torch.jit.load(torch_net, map_location=f"cuda:{device}").eval()
    model = capi.Model(model_blob)
    for channels, group in groups.items():
        _denoise_group(model, group, channels, out_dir, chunk_frames, device, vad_csv, rate, atten_limit_db, vad_gate, vad_hold,
                       rate_table=rates is not None, format_table=formats is not None, link=link_channels,
                       out_tables=out_rate is not None or out_format is not None, net=net)
    model.close()
    return [d["n_frames"] for d in files]


def _denoise_group(model, files, C, out_dir, chunk_frames, device, vad_csv, rate, atten_limit_db, vad_gate, vad_hold, rate_table,
                   format_table, link=False, out_tables=False, net=None):
    """the files of one channel count C through one batch of len(files) * C streams: file g's channel c is stream g * C + c"""
    FRAME = capi.FRAME * rate // 48000
    G, N = len(files), len(files) * C
    frame_of = [d["frame"] for d in files]
    width = [d["width"] for d in files]  # bytes per sample of each file
    n_frames = [d["n_frames"] for d in files]
    T = max(n_frames + [0])
    if net is not None:
        chunk_frames = max(T, 1)  # (the whole group in one analyze / synthesize pair)
        if hasattr(net, "reset"):
            net.reset()  # (a stateful net starts every group as a new sequence)
    batch = capi.Batch(model, N, device=device)
    if rate != 48000:
        batch.set_pcm_rate(rate)
    if rate_table or any(d["rate"] != rate for d in files):
        batch.set_stream_rates([d["rate"] for d in files for _ in range(C)])
    if format_table or any(w == 1 for w in width):
        batch.set_stream_formats([d["codec"] for d in files for _ in range(C)])
    if out_tables:  # (both, so that each side is described by its own pair of tables)
        batch.set_stream_out_rates([d["out_rate"] for d in files for _ in range(C)])
        batch.set_stream_out_formats([d["out_codec"] for d in files for _ in range(C)])
    out_frame_of, out_width = [d["out_frame"] for d in files], [d["out_width"] for d in files]
    if atten_limit_db is not None or vad_gate or vad_hold:
        batch.set_stream_controls(capi.controls_table(N, atten_limit_db, vad_gate, vad_hold))
    if C > 1:
        batch.set_pcm_channels(C)
        if link:
            batch.set_gain_link(C)
    ins = [open(d["path"], "rb") for d in files]
    outs = [open(os.path.join(out_dir, os.path.basename(d["path"]) + (".denoised.wav" if d["wav"] else ".denoised.raw")), "wb")
            for d in files]
    for d, f, o in zip(files, ins, outs):
        f.seek(d["offset"])
        if d["wav"]:  # (the first output frame is dropped, as for a RAW file: the length is known up front)
            oi = out_info(d["wav"], d["out_rate"], d["out_codec"])
            d["out_bytes"] = max(d["n_frames"] - 1, 0) * d["out_frame"] * oi.block
            o.write(wav.header(oi, d["out_bytes"]))
    vfs = [open(os.path.join(out_dir, os.path.basename(d["path"]) + ".vad.csv"), "w") for d in files] if vad_csv else None
    # every file's chunk is ONE contiguous run of the staging buffer, [G][chunk frames * FRAME * C], which the batch reads and writes
    # where it lies (capi.Batch.set_pcm_layout: frames FRAME * C apart, files a whole chunk apart) -- no interleaving into frame-major
    # rows here, and no de-interleaving of a file's channels: a frame's slot holds FRAME * C samples as they lie in the file
    # (capi.Batch.set_pcm_channels).  `chunk` / `out` below are (frames, G, FRAME * C) VIEWS of those runs
    cf = min(chunk_frames, max(T, 1))
    batch.set_pcm_layout(FRAME * C, cf * FRAME * C)
    buf, obuf = batch.pcm_array(cf, np.int16), batch.pcm_array(cf, np.int16)

    def slots(a):  # (frames, G, FRAME * C): a file's frame as one run, whatever the channel count
        v = a.reshape(a.shape[0], G, FRAME * C)
        assert np.shares_memory(v, a)
        return v
    rows8 = lambda a: a.view(np.uint8)  # the same rows as bytes (a companded file's view): (frames, G, 2 * FRAME * C)
    for t0 in range(0, T, chunk_frames):
        tn = min(chunk_frames, T - t0)
        chunk = slots(buf)[:tn]
        chunk[:] = 0  # a stream whose file has ended is fed silence and produces no more output
        for s in range(G):  # (silence of a companded stream is its law's zero code, not a zero byte: 0x00 is a full-scale sample)
            if width[s] == 1:
                rows8(chunk)[:, s, :frame_of[s] * C] = SILENCE[g711.code(files[s]["codec"])]
        for s, f in enumerate(ins):
            k = max(0, min(tn, n_frames[s] - t0))
            if k:
                if width[s] == 1:
                    rows8(chunk)[:k, s, :frame_of[s] * C] = np.frombuffer(f.read(k * frame_of[s] * C), dtype=np.uint8).reshape(k, frame_of[s] * C)
                    continue
                x = np.frombuffer(f.read(k * frame_of[s] * C * 2), dtype=np.int16)
                chunk[:k, s, :frame_of[s] * C] = x.reshape(k, frame_of[s] * C)
        if net is None:
            out, vad, _ = batch.process_s16(buf[:tn], want_gains=False, out=obuf[:tn])
        else:
            vad = _split_pair(batch, net, buf[:tn], obuf[:tn], device)
        out = slots(obuf)[:tn]
        for s in range(G):
            k = max(0, min(tn, n_frames[s] - t0))
            first = 1 if t0 == 0 else 0  # the demo drops the first output frame (rnnoise_demo.c:59-60)
            if k > first and out_width[s] == 1:
                outs[s].write(rows8(out)[first:k, s, :out_frame_of[s] * C].tobytes())
            elif k > first:
                outs[s].write(out[first:k, s, :out_frame_of[s] * C].tobytes())  # (the demo's truncating (short) cast was done on the device)
            if vfs and k:  # (one column per channel)
                vfs[s].write("".join(",".join(f"{v:.6f}" for v in row) + "\n" for row in vad[:k, s * C:(s + 1) * C]))
    for d, o in zip(files, outs):
        if d["wav"] and d["out_bytes"] & 1:
            o.write(b"\0")  # (the pad byte of an odd data chunk)
    for f in ins + outs + (vfs or []):
        f.close()
    batch.close()


def _split_pair(batch, net, pcm, out, device):
    """pcm through analyze -> net -> synthesize into out; returns the vad as (T, N): the net's, and 0 on a silent frame, where the
    net's rows are not read -- what the gate and a link saw, and what process_s16 reports there"""
    import torch
    feats, silence = batch.analyze(pcm, layout="stream", s16=True)
    with torch.no_grad():
        gains, vad = net(torch.from_numpy(feats).to(f"cuda:{device}"))
    gains, vad = gains.float().cpu().numpy(), vad.float().cpu().numpy()
    batch.synthesize(gains, vad, layout="stream", s16=True, out=out)
    return np.where(silence != 0, np.float32(0), vad.reshape(vad.shape[0], vad.shape[1]).T)


def dump_features(model_blob: bytes, speech: str, noise: str, fgnoise: str, out: str, count: int, seed=None, seq_frames: int = 2000,
                  streams: int = 64, device: int = 0, rir_list=None, rir_work_mb: int = 256, vad: str = "auto"):
    """COUNT training sequences of seq_frames frames into `out` (float32 records, sequence after sequence: the reference's file
    format): sequence i runs on stream i % streams of one batch in round i // streams.  Each corpus is read and uploaded once.  The
    draws come from numpy's default generator seeded with `seed` (train_data.draw, then train_data.draw_rir from the same generator
    when rir_list names a file of RIR file names).  vad: where the Viterbi VAD runs, "auto" | "device" | "host" (train_data.generate_rounds);
    the file is the same either way."""
    import torch

    from . import train_data
    dev = torch.device("cuda", device)
    corpora = [torch.from_numpy(np.fromfile(p, dtype=np.int16)).to(dev) for p in (speech, noise, fgnoise)]
    rng = np.random.default_rng(seed)
    draws = train_data.draw(rng, count, [c.numel() for c in corpora], seq_frames)
    model = capi.Model(model_blob)
    batch = capi.Batch(model, max(1, min(streams, count)), device=device)
    rirs = None
    if rir_list:
        with open(rir_list) as f:
            names = [line.rstrip("\n") for line in f if line.rstrip("\n")]
        responses = [np.fromfile(name, dtype=np.float32, count=capi.RIR_MAX) for name in names]
        with torch.cuda.device(dev):
            rirs = (train_data.rir_spectra(batch, responses, dev), train_data.draw_rir(rng, count, len(responses)))
    with torch.cuda.device(dev), open(out, "wb") as f:
        for rec in train_data.generate_rounds(batch, *corpora, draws, seq_frames, rirs, rir_work_mb << 20, vad):
            f.write(rec.tobytes())
    batch.close()
    model.close()
    return count * seq_frames


def train_arguments(ap, a) -> dict:
    """the keyword arguments of train.train_files from the parsed `train` command line; argparse errors where they do not fit"""
    if a.online is not None:
        if len(a.paths) != 1:
            ap.error("train --online: one path, the output folder")
        if a.sequences_per_epoch is None or a.sequences_per_epoch < a.batch_size:
            ap.error("train --online: --sequences-per-epoch, at least one batch")
        records, out = None, a.paths[0]
    else:
        if len(a.paths) != 2:
            ap.error("train: RECORDS OUT (or OUT with --online)")
        if a.sequences_per_epoch is not None or a.rir_list is not None:
            ap.error("train: --sequences-per-epoch and --rir-list belong to --online")
        records, out = a.paths
    if a.epochs < 1 or a.batch_size < 1 or a.sequence_length < 6 or not a.gamma > 0:
        ap.error("train: --epochs and --batch-size at least 1, --sequence-length at least 6, --gamma above 0")
    kw = dict(records=records, out=out, online=tuple(a.online) if a.online is not None else None,
              sequences_per_epoch=a.sequences_per_epoch, rir_list=a.rir_list, epochs=a.epochs, batch_size=a.batch_size,
              sequence_length=a.sequence_length, lr=a.lr, lr_decay=a.lr_decay, gamma=a.gamma, sparse=a.sparse,
              initial_checkpoint=a.initial_checkpoint, cond_size=a.cond_size, gru_size=a.gru_size, suffix=a.suffix, seed=a.seed,
              device=a.device)
    if a.gru != "torch":  # the default run's arguments are what they were before the switch existed
        kw["gru"] = a.gru
    return kw


AUDIO_COLUMNS = (("snr_in", "SNR in"), ("snr_out", "SNR out"), ("snr_gain", "gain"), ("si_sdr_in", "SI-SDR in"),
                 ("si_sdr_out", "SI-SDR out"), ("si_sdr_gain", "gain"), ("seg_snr_in", "segSNR in"), ("seg_snr_out", "segSNR out"))


STOI_COLUMNS = (("stoi_in", "STOI in"), ("stoi_out", "STOI out"), ("estoi_in", "ESTOI in"), ("estoi_out", "ESTOI out"))


def audio_table(names, results, stoi: bool = False) -> str:
    """the table of eval-audio: one row per model with the means over its sequences in dB (audio_score.summary's keys), the
    sequences scored and left out (zero clean energy); then, for every model after the first, a row of differences to the first.
    stoi: four more columns, the means of STOI and ESTOI (rnnoise_amd.stoi) of the noisy and of the denoised signal"""
    width = max([len("model")] + [len(n) + 2 for n in names])
    cell = lambda v: f"{v:>10.3f}"
    columns = AUDIO_COLUMNS + (STOI_COLUMNS if stoi else ())
    lines = [f"{'model':<{width}} {'seqs':>6} {'left out':>8} " + " ".join(f"{title:>10}" for _key, title in columns)]
    for n, r in zip(names, results):
        lines.append(f"{n:<{width}} {r['sequences']:>6d} {r['excluded']:>8d} " + " ".join(cell(r[k]) for k, _ in columns))
    for n, r in zip(names[1:], results[1:]):
        with np.errstate(invalid="ignore"):  # (inf - inf where both outputs are exact: nan)
            diff = [np.float64(r[k]) - np.float64(results[0][k]) for k, _ in columns]
        lines.append(f"{'d ' + n:<{width}} {'':>6} {'':>8} " + " ".join(cell(v) for v in diff))
    return "\n".join(lines)


def eval_audio_files(speech: str, noise: str, fgnoise: str, models, count: int, frames: int = 2000, checkpoint=None, torch_net=None,
                     rir_list=None, seed=None, streams: int = 64, device: int = 0, rir_work_mb: int = 256, stoi: bool = False,
                     float_net: str = "torch"):
    """eval-audio: `count` sequences of `frames` frames drawn as dump_features draws them (the same generator and seed give the
    same sequences), through every blob of `models` (paths) and the float networks named -> (names, evaluate.evaluate_audio's
    results).  Without a blob the DSP runs on the blob the checkpoint exports to.  stoi: every result also has the means of STOI and
    ESTOI (evaluate.evaluate_audio's stoi).  float_net: "torch" runs the checkpoint's network as the torch module, "native" as
    rnnoise_amd.fnet.FloatNetRuntime on librnnoise_amd_fnet.so."""
    import torch

    from . import evaluate, train_data
    dev = torch.device("cuda", device)
    corpora = [torch.from_numpy(np.fromfile(p, dtype=np.int16)).to(dev) for p in (speech, noise, fgnoise)]
    rng = np.random.default_rng(seed)
    draws = train_data.draw(rng, count, [c.numel() for c in corpora], frames)
    blobs = [open(m, "rb").read() for m in models]
    names, nets, net_blob = list(models), [], blobs[0] if blobs else None
    if float_net not in ("torch", "native"):
        raise ValueError(f'float_net: "torch" or "native", not {float_net!r}')
    if float_net == "native" and checkpoint is None:
        raise ValueError("--float-net native runs a --checkpoint")
    if checkpoint is not None:
        from . import export
        if float_net == "native":
            from . import fnet
            nets.append(fnet.FloatNetRuntime(checkpoint, device=device))
        else:
            from . import float_net as float_net_module
            nets.append(float_net_module.load_checkpoint(checkpoint, device=f"cuda:{device}"))
        names.append(checkpoint)
        if net_blob is None:
            net_blob = export.blob_from_state_dict(export.load_state_dict_file(checkpoint))
    if torch_net is not None:
        nets.append(torch.jit.load(torch_net, map_location=f"cuda:{device}").eval())
        names.append(torch_net)
    if net_blob is None:
        raise ValueError("eval-audio: --torch-net needs a --model or a --checkpoint for the DSP's batch")
    rirs = None
    if rir_list:
        with open(rir_list) as f:
            rir_names = [line.rstrip("\n") for line in f if line.rstrip("\n")]
        responses = [np.fromfile(name, dtype=np.float32, count=capi.RIR_MAX) for name in rir_names]
        model = capi.Model(net_blob)
        loader = capi.Batch(model, 1, device=device)
        with torch.cuda.device(dev):
            rirs = (train_data.rir_spectra(loader, responses, dev), train_data.draw_rir(rng, count, len(responses)))
        loader.close()
        model.close()
    res = evaluate.evaluate_audio(corpora, blobs, draws, frames, rirs=rirs, nets=nets, net_blob=net_blob, streams=streams,
                                  device=device, rir_work_bytes=rir_work_mb << 20, stoi=stoi)
    return names, res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("denoise")
    p.add_argument("--model", default=None, help='"DNNw" weight blob (src/write_weights.c format); optional beside --checkpoint')
    p.add_argument("--out-dir", required=True)
    p.add_argument("--chunk-frames", type=int, default=100)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--vad-csv", action="store_true")
    p.add_argument("--rate", type=int, default=48000, choices=capi.PCM_RATES_ALL, help="sample rate of the RAW files")
    p.add_argument("--rates", type=lambda v: [int(x) for x in v.split(",")], default=None,
                   help="comma list, one sample rate per input file, each at most --rate: a mixed-rate batch")
    p.add_argument("--formats", type=lambda v: v.split(","), default=None,
                   help="comma list, one of s16 | ulaw | alaw per input file: G.711 files are raw bytes, one per sample")
    p.add_argument("--out-rate", type=int, default=None, choices=capi.PCM_RATES_ALL,
                   help="sample rate every output is written at, at most --rate (default: each input's own)")
    p.add_argument("--out-format", default=None, choices=("s16", "ulaw", "alaw"),
                   help="sample format every output is written in (default: each input's own)")
    p.add_argument("--atten-limit-db", type=float, default=None,
                   help="attenuation limit in dB: no band is suppressed by more (a floor on the band gains); default none")
    p.add_argument("--vad-gate", type=float, default=0.0, help="VAD threshold in [0, 1] below which output is muted (0: no gate)")
    p.add_argument("--vad-hold", type=int, default=0, help="frames the VAD gate stays open after the last voice frame")
    p.add_argument("--link-channels", action="store_true",
                   help="one suppression for the channels of each multichannel WAV file: linked band gains and VAD gate")
    p.add_argument("--torch-net", default=None,
                   help="TorchScript module [N,T,65] -> ([N,T,32], [N,T,1]) that replaces the blob's network (split calls; one pair per file group)")
    p.add_argument("--checkpoint", default=None,
                   help="trainer checkpoint (.pth): its float network replaces the blob's network (split calls; one pair per file group)")
    p.add_argument("--max-store-gb", type=float, default=4.0,
                   help="--torch-net / --checkpoint: device memory the pending frames may take, in GiB")
    p.add_argument("--float-net", choices=("torch", "native"), default="torch",
                   help="what runs --checkpoint's network: the torch module (default), or native: this project's own kernels "
                        "(librnnoise_amd_fnet.so), any cond_size / gru_size the library takes")
    p.add_argument("inputs", nargs="+")
    p = sub.add_parser("dump-features")
    p.add_argument("--model", required=True, help='"DNNw" weight blob: a batch needs one (the extraction runs no network)')
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--seq-frames", type=int, default=2000, help="frames per sequence (the reference: 2000)")
    p.add_argument("--streams", type=int, default=64, help="sequences per round: the batch size")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--rir-list", default=None, help="file of RIR file names, one per line (raw float32): the reference's -rir_list")
    p.add_argument("--rir-work-mb", type=int, default=256, help="workspace of the RIR filter in MiB, at least 1")
    p.add_argument("--vad", default="auto", choices=("host", "device", "auto"),
                   help="where the Viterbi VAD runs: in the levels kernel, on the host, or on the device where this host's libm allows "
                        "(the default); the records are the same")
    p.add_argument("speech")
    p.add_argument("noise")
    p.add_argument("fgnoise")
    p.add_argument("out")
    p.add_argument("count", type=int)
    p = sub.add_parser("export")
    p.add_argument("--densities", type=lambda v: tuple(float(x) for x in v.split(",")), default=None,
                   help="R,Z,N: block-sparsify the GRU matrices first, to these densities of the reset, update and new gates")
    p.add_argument("--pack", action="store_true", help="write the GPU-native RNPK pack instead of the DNNw blob")
    p.add_argument("checkpoint", help="trainer checkpoint (.pth with 'state_dict', or a bare state dict)")
    p.add_argument("out")
    p = sub.add_parser("eval-records")
    p.add_argument("--model", default=None, action="append", help='"DNNw" weight blob; repeat to score several on the same records')
    p.add_argument("--checkpoint", default=None,
                   help="trainer checkpoint (.pth): scored in float beside the blobs, with their differences to it and per-band means")
    p.add_argument("--sequence-length", type=int, default=2000, help="records per sequence (the trainer: 2000)")
    p.add_argument("--gamma", type=float, default=0.25, help="perceptual exponent of the gain loss (the trainer: 0.25)")
    p.add_argument("--first", type=int, default=4, help="first step that is scored (the trainer: 4)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--max-streams", type=int, default=65536, help="sequences per slab: the batch size")
    p.add_argument("file", help="float32 records of 98 floats, sequence after sequence (dump-features' output)")
    p = sub.add_parser("eval-audio")
    p.add_argument("--model", default=None, action="append", help='"DNNw" weight blob; repeat to score several on the same sequences')
    p.add_argument("--checkpoint", default=None, help="trainer checkpoint (.pth): its float network between the split calls")
    p.add_argument("--torch-net", default=None, help="TorchScript module [N,T,65] -> ([N,T,32], [N,T,1]) between the split calls")
    p.add_argument("--float-net", choices=("torch", "native"), default="torch",
                   help="what runs --checkpoint's network: the torch module (default), or native: this project's own kernels "
                        "(librnnoise_amd_fnet.so), any cond_size / gru_size the library takes")
    p.add_argument("--count", type=int, required=True, help="sequences to generate and score")
    p.add_argument("--frames", type=int, default=2000, help="frames per sequence (the trainer: 2000)")
    p.add_argument("--rir-list", default=None, help="file of RIR file names, one per line (raw float32): the reference's -rir_list")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--streams", type=int, default=64, help="sequences per round: the batch size (the numbers do not depend on it)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--stoi", action="store_true",
                   help="also STOI and ESTOI of the noisy and of the denoised signal (librnnoise_amd_stoi.so): four more columns")
    p.add_argument("speech")
    p.add_argument("noise")
    p.add_argument("fgnoise")
    p = sub.add_parser("train")
    p.add_argument("--suffix", default="", help="model name suffix of the checkpoint files")
    p.add_argument("--cond-size", type=int, default=128)
    p.add_argument("--gru-size", type=int, default=384)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--epochs", type=int, default=200)
    p.add_argument("--sequence-length", type=int, default=2000)
    p.add_argument("--lr-decay", type=float, default=5e-5)
    p.add_argument("--initial-checkpoint", default=None)
    p.add_argument("--gamma", type=float, default=0.25, help="perceptual exponent of the gain loss")
    p.add_argument("--sparse", action="store_true", help="the GRU block sparsifier's schedule after every step")
    p.add_argument("--seed", type=int, default=None, help="of the shuffle, the initialisation and the online draws")
    p.add_argument("--online", nargs=3, metavar=("SPEECH", "NOISE", "FGNOISE"), default=None,
                   help="RAW s16 48 kHz corpora: train on sequences generated on the device instead of a record file")
    p.add_argument("--sequences-per-epoch", type=int, default=None, help="with --online: sequences generated per epoch")
    p.add_argument("--rir-list", default=None, help="with --online: file of RIR file names, one per line (raw float32)")
    p.add_argument("--gru", choices=("torch", "native", "stack"), default="torch",
                   help="what runs the three GRUs: torch's nn.GRU (default), or native: their recurrences, forward and backward, on "
                        "this project's own kernels (librnnoise_amd_gru.so: one launch per step, exact float32 matrix instructions), "
                        "or stack: the three layers as one diagonal launch per step, layers 2 and 3 one step behind each "
                        "(librnnoise_amd_gru_stack.so); the same parameters and checkpoints either way")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("paths", nargs="+", metavar="PATH", help="RECORDS OUT: a record file and the output folder; with --online: OUT")
    a = ap.parse_args(argv)
    if a.cmd == "train":
        kw = train_arguments(ap, a)
        from . import train
        train.train_files(**kw)
        return
    if a.cmd == "eval-audio":
        if not a.model and a.checkpoint is None and a.torch_net is None:
            ap.error("eval-audio: --model, --checkpoint or --torch-net")
        if a.count < 1 or a.frames < 3:
            ap.error("eval-audio: --count at least 1, --frames at least 3 (the first two output frames are not scored)")
        if a.float_net == "native" and a.checkpoint is None:
            ap.error("eval-audio: --float-net native needs a --checkpoint")
        if a.stoi and a.frames > 8192:
            ap.error("eval-audio: --stoi takes sequences of at most 8192 frames (RNNOISE_AMD_STOI_MAX_FRAMES)")
        names, res = eval_audio_files(a.speech, a.noise, a.fgnoise, a.model or [], a.count, a.frames, a.checkpoint, a.torch_net,
                                      a.rir_list, a.seed, a.streams, a.device,
                                      **(dict(stoi=True) if a.stoi else {}),  # (the default run's arguments are what they were before the flags)
                                      **(dict(float_net="native") if a.float_net == "native" else {}))
        print(f"eval-audio: {a.count} sequences of {a.frames} frames, seed {a.seed}, delay 960 samples, first scored frame 2")
        print(audio_table(names, res, a.stoi))
        return
    if a.cmd == "export":
        from . import export
        n = export.export_file(a.checkpoint, a.out, a.densities, a.pack)
        print(f"wrote {a.out}: {n} bytes ({'RNPK pack' if a.pack else 'DNNw blob'})")
        return
    if a.cmd == "eval-records" and (a.checkpoint is not None or not a.model):
        import json

        from . import evaluate
        if a.checkpoint is None:
            ap.error("eval-records: --model or --checkpoint")
        strip = lambda r: {k: v for k, v in r.items() if k != "per_sequence"}
        ck = evaluate.evaluate_checkpoint(a.file, a.checkpoint, a.sequence_length, a.gamma, a.first, a.device, a.max_streams)
        res = evaluate.evaluate_records(a.file, [open(m, "rb").read() for m in a.model or []], a.sequence_length, a.gamma,
                                        max(a.first, 4), a.device, a.max_streams, bands=True)
        delta = lambda r: dict(delta_to_checkpoint={k: r[k] - ck[k] for k in ("gain_loss", "vad_loss", "loss")},
                               band_delta_to_checkpoint=[x - y for x, y in zip(r["band_gain_loss"], ck["band_gain_loss"])])
        print(json.dumps(dict(file=a.file, sequence_length=a.sequence_length, gamma=a.gamma, first=max(a.first, 4),
                              checkpoint=dict(checkpoint=a.checkpoint, **strip(ck)),
                              models=[dict(model=m, **strip(r), **delta(r)) for m, r in zip(a.model or [], res)])))
        return
    if a.cmd == "eval-records":
        import json

        from . import evaluate
        res = evaluate.evaluate_records(a.file, [open(m, "rb").read() for m in a.model], a.sequence_length, a.gamma, a.first, a.device,
                                        a.max_streams)
        print(json.dumps(dict(file=a.file, sequence_length=a.sequence_length, gamma=a.gamma, first=a.first,
                              models=[dict(model=m, **{k: v for k, v in r.items() if k != "per_sequence"})
                                      for m, r in zip(a.model, res)])))
        return
    if a.cmd == "dump-features":
        n = dump_features(open(a.model, "rb").read(), a.speech, a.noise, a.fgnoise, a.out, a.count, a.seed, a.seq_frames, a.streams,
                          a.device, a.rir_list, a.rir_work_mb, a.vad)
        print(f"wrote {a.count} sequences, {n} records")
        return
    if a.model is None and a.checkpoint is None:
        ap.error("denoise: --model or --checkpoint")
    if a.float_net == "native" and a.checkpoint is None:
        ap.error("denoise: --float-net native needs a --checkpoint")
    if a.model is None:  # (the DSP's batch needs a blob: the one this checkpoint exports to)
        from . import export
        model_blob = export.blob_from_state_dict(export.load_state_dict_file(a.checkpoint))
    else:
        model_blob = open(a.model, "rb").read()
    n = denoise_files(model_blob, a.inputs, a.out_dir, a.chunk_frames, a.device, a.vad_csv, a.rate,
                      a.atten_limit_db, a.vad_gate, a.vad_hold, a.rates, a.formats, a.link_channels, a.out_rate, a.out_format,
                      a.torch_net, a.max_store_gb, a.checkpoint, **(dict(float_net="native") if a.float_net == "native" else {}))
    print(f"denoised {len(a.inputs)} streams, {sum(n)} frames")


if __name__ == "__main__":
    main(sys.argv[1:])
