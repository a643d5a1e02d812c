"""What a blob costs on a record file, in the reference trainer's own loss (include/rnnoise_amd.h: rnnoise_batch_eval_records;
DESIGN.md 4.28): the quantised, sparsified network as it ships, run over the 98-float records of dump_features -- the reference's
src/dump_features.c, or `python -m rnnoise_amd.cli dump-features` -- and scored as torch/rnnoise/train_rnnoise.py scores its float
checkpoint.  Nothing is trained here.

  python -m rnnoise_amd.cli eval-records validation.f32 --model weights_blob.bin [--model other.bin ...] [--checkpoint ckpt.pth]

evaluate_checkpoint scores the float checkpoint itself on the same file -- rnnoise_amd.float_net's forward_sequence in torch, its
outputs scored by rnnoise_batch_score_records_device, the scoring half of the record step -- so that the difference between a blob's
loss and its checkpoint's is what quantisation and sparsification cost, not what two pieces of loss code differ by.

evaluate_audio measures the AUDIO instead: the sequences the trainer would have seen are generated on the device
(train_data.mix_rounds), denoised where they lie -- by a blob's batch, or by a float network between the split calls -- and scored
against the clean signal by librnnoise_amd_score.so (rnnoise_amd/audio_score.py): SNR, SI-SDR and segmental SNR in dB, which see the
pitch filter, the gain smoothing and the overlap-add that the trainer's loss does not.

  python -m rnnoise_amd.cli eval-audio speech.pcm noise.pcm fgnoise.pcm --model weights_blob.bin [--checkpoint ckpt.pth] --count N
"""
from __future__ import annotations

import os

import numpy as np

from . import capi

REC = capi.REC


def map_records(path_or_array, sequence_length: int) -> np.ndarray:
    """the records as (sequences, sequence_length, 98) float32, truncated to whole sequences as the trainer's RNNoiseDataset does; a
    file is memory-mapped, an array is viewed"""
    if isinstance(path_or_array, np.ndarray):
        data = np.ascontiguousarray(path_or_array, np.float32).reshape(-1)
    else:
        floats = os.path.getsize(path_or_array) // 4  # (a partial float at the end is dropped with the partial sequence)
        data = np.memmap(path_or_array, dtype=np.float32, mode="r", shape=(floats,)) if floats else np.zeros(0, np.float32)
    n = data.shape[0] // sequence_length // REC
    return data[:n * sequence_length * REC].reshape(n, sequence_length, REC)


def _means(sums, bands=None):
    """the result dict of one model from its per-sequence sums (S, EVAL_SUMS) and, where asked for, band sums (S, 32)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        g = sums[:, 0] / (capi.NB_BANDS * sums[:, 2])
        v = sums[:, 1] / sums[:, 2]
        out = dict(sequences=sums.shape[0], **capi.eval_losses(sums), per_sequence=dict(gain_loss=g, vad_loss=v, loss=g + .001 * v))
        if bands is not None:  # band b's mean gain term over every scored frame: gain_loss is the mean of the 32
            frames = sums[:, 2].sum()
            out["band_gain_loss"] = [float(x) for x in (bands.sum(0) / frames if frames else np.full(capi.NB_BANDS, np.nan))]
    return out


def evaluate_records(path_or_array, models, sequence_length: int = 2000, gamma: float = .25, first: int = 4, device: int = 0,
                     max_streams: int = 65536, slab_bytes: int = 1 << 30, bands: bool = False, segment_bytes: int = 1 << 28):
    """Scores every model of `models` (blobs as bytes, or capi.Model objects) on the sequences of a record file or array.  The
    sequences go up in slabs of at most max_streams (and at most slab_bytes) as they lie in the file -- [sequence][frame][98] --, and
    each slab is walked with strides, one sequence per stream, by every model in turn; nothing is transposed.  Returns one dict per
    model: sequences, frames_scored, gain_loss, vad_loss, loss -- the trainer's three means over the whole file -- and per_sequence,
    a dict of (sequences,) float64 arrays gain_loss, vad_loss, loss with each sequence's own means (nan for a sequence with no scored
    frame).  bands: also band_gain_loss, the 32 per-band means of the gain term -- the walk then goes in segments of frames (at most
    segment_bytes of predictions each), eval_records' gains / vad outputs of a segment scored once more by
    rnnoise_batch_score_records_device for its band sums; the sums are those of one call either way."""
    import torch

    data = map_records(path_or_array, sequence_length)
    S, T = data.shape[0], sequence_length
    if S == 0:
        raise ValueError(f"no whole sequence of {sequence_length} records")
    handles = [m if isinstance(m, capi.Model) else capi.Model(m) for m in models]
    dev = torch.device("cuda", device)
    per_slab = max(1, min(max_streams, slab_bytes // (T * REC * 4), S))
    sums = [np.zeros((S, capi.EVAL_SUMS), np.float64) for _ in handles]
    band_sums = [np.zeros((S, capi.NB_BANDS), np.float64) for _ in handles] if bands else None
    batches = {}
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        for s0 in range(0, S, per_slab):
            n = min(per_slab, S - s0)
            d_rec = torch.from_numpy(np.array(data[s0:s0 + n])).to(dev)  # (a copy: the map is read-only)
            for k, m in enumerate(handles):
                if (k, n) not in batches:
                    batches[k, n] = capi.Batch(m, n, device=device)
                b = batches[k, n]
                b.reset()  # (synchronous: the upload above, on torch's stream, is done too)
                d_sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
                if not bands:
                    b.eval_records_device(d_sums.data_ptr(), 0, 0, d_rec.data_ptr(), 0, T, frame_stride=REC, row_stride=T * REC,
                                          gamma=gamma, first=first, stream=st.cuda_stream)
                else:
                    seg = max(1, min(T, segment_bytes // (n * (capi.NB_BANDS + 1) * 4)))
                    d_g = torch.empty((seg, n, capi.NB_BANDS), dtype=torch.float32, device=dev)
                    d_v = torch.empty((seg, n), dtype=torch.float32, device=dev)
                    d_again = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
                    d_bands = torch.zeros((n, capi.NB_BANDS), dtype=torch.float64, device=dev)
                    for t0 in range(0, T, seg):
                        k_frames = min(seg, T - t0)
                        b.eval_records_device(d_sums.data_ptr(), d_g.data_ptr(), d_v.data_ptr(), d_rec.data_ptr(), t0, k_frames,
                                              frame_stride=REC, row_stride=T * REC, gamma=gamma, first=first, stream=st.cuda_stream)
                        b.score_records_device(d_again.data_ptr(), d_bands.data_ptr(), d_g.data_ptr(), d_v.data_ptr(), d_rec.data_ptr(),
                                               n, t0, k_frames, rec_strides=(REC, T * REC), gamma=gamma, first=first,
                                               stream=st.cuda_stream)
                    band_sums[k][s0:s0 + n] = d_bands.cpu().numpy()
                sums[k][s0:s0 + n] = d_sums.cpu().numpy()  # (waits for the stream)
    for b in batches.values():
        b.close()
    out = [_means(sums[k], band_sums[k] if bands else None) for k in range(len(handles))]
    for m, h in zip(models, handles):
        if not isinstance(m, capi.Model):
            h.close()
    return out


def evaluate_checkpoint(path_or_array, checkpoint, sequence_length: int = 2000, gamma: float = .25, first: int = 4, device: int = 0,
                        max_streams: int = 65536, slab_bytes: int = 1 << 30, group_bytes: int = 1 << 30):
    """Scores a float checkpoint -- a path (float_net.load_checkpoint) or a module with forward_sequence -- on the sequences of a
    record file or array, as evaluate_records scores a blob: the slabs go up the same way, forward_sequence runs in torch on the
    feature columns of groups of sequences (a group's activations stay under group_bytes), and its [n][T - 4] outputs are scored
    where they lie by rnnoise_batch_score_records_device with t0 = 4 -- output k is step k + 4 -- against the records of the slab.
    `first` below 4 scores from step 4 all the same: the float network has no earlier output.  Returns evaluate_records' dict for
    one model, with band_gain_loss."""
    import torch

    from . import blob as blob_tools
    from . import float_net
    data = map_records(path_or_array, sequence_length)
    S, T = data.shape[0], sequence_length
    if S == 0:
        raise ValueError(f"no whole sequence of {sequence_length} records")
    if T <= float_net.LOOKAHEAD:
        raise ValueError(f"sequences of {T} records: the float network needs more than {float_net.LOOKAHEAD}")
    dev = torch.device("cuda", device)
    net = checkpoint if isinstance(checkpoint, torch.nn.Module) else float_net.load_checkpoint(checkpoint)
    net = net.to(dev).eval()
    model = capi.Model(blob_tools.synth_model())  # (a score call reads no model: the batch only names the device)
    batch = capi.Batch(model, 1, device=device)
    per_slab = max(1, min(max_streams, slab_bytes // (T * REC * 4), S))
    width = capi.FEATURES + 2 * net.cond_size + 10 * net.gru_size  # floats a frame of a sequence keeps alive in forward_sequence, roughly
    per_group = max(1, group_bytes // (T * width * 4))
    K = T - float_net.LOOKAHEAD
    sums, bands = np.zeros((S, capi.EVAL_SUMS), np.float64), np.zeros((S, capi.NB_BANDS), np.float64)
    with torch.cuda.device(dev), torch.no_grad():
        st = torch.cuda.current_stream(dev)
        for s0 in range(0, S, per_slab):
            n = min(per_slab, S - s0)
            d_rec = torch.from_numpy(np.array(data[s0:s0 + n])).to(dev)
            d_sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
            d_bands = torch.zeros((n, capi.NB_BANDS), dtype=torch.float64, device=dev)
            for g0 in range(0, n, per_group):
                m = min(per_group, n - g0)
                gains, vad = net.forward_sequence(d_rec[g0:g0 + m, :, :capi.FEATURES])
                gains, vad = gains.float().contiguous(), vad.float().contiguous()
                assert gains.shape == (m, K, capi.NB_BANDS) and vad.shape == (m, K, 1)
                batch.score_records_device(d_sums[g0:].data_ptr(), d_bands[g0:].data_ptr(), gains.data_ptr(), vad.data_ptr(),
                                           d_rec[g0:].data_ptr(), m, float_net.LOOKAHEAD, K, gain_strides=(capi.NB_BANDS, K * capi.NB_BANDS),
                                           vad_strides=(1, K), rec_strides=(REC, T * REC), gamma=gamma, first=first,
                                           stream=st.cuda_stream)
                st.synchronize()  # (the group's outputs are read by the launch: they stay until it is done)
            sums[s0:s0 + n], bands[s0:s0 + n] = d_sums.cpu().numpy(), d_bands.cpu().numpy()
    batch.close()
    model.close()
    return _means(sums, bands)


def evaluate_audio(corpora, models, draws, n_frames: int, rirs=None, nets=(), net_blob=None, streams: int = 64, device: int = 0,
                   vad: str = "auto", first: int = 2, delay: int = None, rir_work_bytes: int = 256 << 20, tap=None, stoi: bool = False):
    """Denoises the sequences of `draws` (train_data.draw) and scores the result against their clean signals, on the device.
    corpora: (speech, noise, fgnoise), 1-D int16 torch tensors on cuda:`device`.  models: blobs (bytes) or capi.Model objects, each
    run by a batch of `streams` streams; nets: torch modules mapping features (N, T, 65) to (gains (N, T, 32), vad (N, T, 1)) -- a
    float_net.FloatNet, a TorchScript file's module --, each run by RNNoiseOp.denoise_with on the DSP of net_blob (default: the
    first model's blob).  All of them see the same planes in one pass over the rounds of train_data.mix_rounds: per round and
    denoiser the state is reset (rnnoise_batch_reset; a net's reset()), the round's `noisy` plane is denoised, and
    rnnoise_amd_audio_score_device adds the round's sums with first frame `first` and delay `delay` (audio_score.DELAY) where the
    three planes lie.  Every sequence starts from the zero state, so its numbers depend neither on `streams` nor on its position.
    The first model's batch also runs the mixing calls: they touch no denoiser state (train_data.mix_rounds).
    tap: a function called as tap(first_sequence, k, clean, noisy, outs) after each round with the device tensors, outs one
    (n_frames, N, 480) plane per denoiser -- valid during the call.
    -> one dict per denoiser, models first: audio_score.summary's means (snr_in, snr_out, snr_gain, si_sdr_in, si_sdr_out,
    si_sdr_gain, seg_snr_in, seg_snr_out, sequences, excluded), sums (S, 8), frame_terms (S, n_frames, 8), active (S, n_frames) --
    vad_target moved to the output frames -- and per_sequence, audio_score.metrics' dict.
    stoi: every dict also has stoi_in, stoi_out, estoi_in, estoi_out -- the means of STOI and ESTOI over the sequences that have a
    segment (rnnoise_amd.stoi, include/rnnoise_amd_stoi.h; same planes, first and delay) --, stoi_results (S, 8) and stoi_per_sequence,
    stoi.metrics' dict.  The noisy side is computed with the first denoiser and reused for the others.  Without it
    librnnoise_amd_stoi.so is not loaded."""
    import torch

    from . import audio_score, train_data
    if stoi:
        from . import stoi as stoi_lib
        if n_frames > stoi_lib.MAX_FRAMES:  # (before anything is generated or denoised)
            raise ValueError(f"stoi: sequences of {n_frames} frames; the library takes at most {stoi_lib.MAX_FRAMES}")
    from .torch_op import RNNoiseOp
    delay = audio_score.DELAY if delay is None else delay
    if not models and not nets:
        raise ValueError("nothing to evaluate: no model and no net")
    S, T = len(draws.mix), n_frames
    N = max(1, min(streams, S))
    dev = torch.device("cuda", device)
    handles = [m if isinstance(m, capi.Model) else capi.Model(m) for m in models]
    ops = []
    if nets:
        dsp = net_blob if net_blob is not None else next((m for m in models if isinstance(m, (bytes, bytearray))), None)
        if dsp is None:
            raise ValueError("nets need net_blob, the blob of the DSP's batch")
        ops = [RNNoiseOp(dsp, N, device=device) for _ in nets]
    D = len(handles) + len(ops)
    sums = [np.zeros((S, audio_score.SLOTS), np.float64) for _ in range(D)]
    terms = [np.zeros((S, T, audio_score.SLOTS), np.float64) for _ in range(D)]
    stoi_res = [np.zeros((S, 8), np.float64) for _ in range(D)] if stoi else None
    active = np.zeros((S, T), np.float32)
    shift = (delay + audio_score.FRAME // 2) // audio_score.FRAME  # frames by which the output lags the input
    fs, rs = audio_score.layout_frames(N)
    with torch.cuda.device(dev):
        batches = [capi.Batch(m, N, device=device) for m in handles]
        gen = batches[0] if batches else ops[0].batch
        st = torch.cuda.current_stream(dev)
        outs = [torch.empty((T, N, audio_score.FRAME), dtype=torch.float32, device=dev) for _ in handles]
        d_sums = torch.empty((N, audio_score.SLOTS), dtype=torch.float64, device=dev)
        d_terms = torch.empty((N, T, audio_score.SLOTS), dtype=torch.float64, device=dev)
        s0 = 0
        for k, clean, noisy, vad_target in train_data.mix_rounds(gen, *corpora, draws, T, rirs, vad, rir_work_bytes):
            planes = []
            for b, out in zip(batches, outs):
                st.synchronize()  # (the reset below is not ordered with torch's stream: the round's planes are complete first)
                b.reset()
                b.process_device(out.data_ptr(), noisy.data_ptr(), 0, 0, T, st.cuda_stream)
                planes.append(out)
            for op, net in zip(ops, nets):
                st.synchronize()
                op.reset()
                if hasattr(net, "reset"):
                    net.reset()
                planes.append(op.denoise_with(net, noisy).contiguous())
            for i, out in enumerate(planes):
                d_sums.zero_()
                d_terms.zero_()
                audio_score.score_device(d_sums.data_ptr(), (clean.data_ptr(), fs, rs), (noisy.data_ptr(), fs, rs),
                                         (out.data_ptr(), out.stride(0), out.stride(1)), k, 0, T, first, delay,
                                         d_terms.data_ptr(), T, device, st.cuda_stream)
                sums[i][s0:s0 + k], terms[i][s0:s0 + k] = d_sums[:k].cpu().numpy(), d_terms[:k].cpu().numpy()  # (waits for the stream)
                if stoi:
                    r = stoi_lib.score(clean[:, :k], noisy[:, :k] if i == 0 else None, out[:, :k], T, first, delay, device)
                    if i > 0:
                        r[:, :4] = stoi_res[0][s0:s0 + k, :4]
                    stoi_res[i][s0:s0 + k] = r
            active[s0:s0 + k, shift:] = vad_target[:T - shift, :k].t().cpu().numpy() if shift < T else 0
            if tap is not None:
                tap(s0, k, clean, noisy, planes)
            s0 += k
        for b in batches:
            b.close()
        for op in ops:
            op.close()
    for m, h in zip(models, handles):
        if not isinstance(m, capi.Model):
            h.close()
    res = []
    for i in range(D):
        per = audio_score.metrics(sums[i], terms[i], active)
        res.append(dict(**audio_score.summary(per), sums=sums[i], frame_terms=terms[i], active=active, per_sequence=per))
        if stoi:
            m = stoi_lib.metrics(stoi_res[i])
            res[-1].update({k: m["summary"][k] for k in stoi_lib.METRIC_KEYS}, stoi_results=stoi_res[i], stoi_per_sequence=m)
    return res


eval_audio = evaluate_audio
