"""What a blob costs on a record file, in the reference trainer's own loss (include/rnnoise_amd.h: rnnoise_batch_eval_records;
DESIGN.md 4.28): the quantised, sparsified network as it ships, run over the 98-float records of dump_features -- the reference's
src/dump_features.c, or `python -m rnnoise_amd.cli dump-features` -- and scored as torch/rnnoise/train_rnnoise.py scores its float
checkpoint.  Nothing is trained here.

  python -m rnnoise_amd.cli eval-records validation.f32 --model weights_blob.bin [--model other.bin ...]
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


def evaluate_records(path_or_array, models, sequence_length: int = 2000, gamma: float = .25, first: int = 4, device: int = 0,
                     max_streams: int = 65536, slab_bytes: int = 1 << 30):
    """Scores every model of `models` (blobs as bytes, or capi.Model objects) on the sequences of a record file or array.  The
    sequences go up in slabs of at most max_streams (and at most slab_bytes) as they lie in the file -- [sequence][frame][98] --, and
    each slab is walked with strides, one sequence per stream, by every model in turn; nothing is transposed.  Returns one dict per
    model: sequences, frames_scored, gain_loss, vad_loss, loss -- the trainer's three means over the whole file -- and per_sequence,
    a dict of (sequences,) float64 arrays gain_loss, vad_loss, loss with each sequence's own means (nan for a sequence with no scored
    frame)."""
    import torch

    data = map_records(path_or_array, sequence_length)
    S, T = data.shape[0], sequence_length
    if S == 0:
        raise ValueError(f"no whole sequence of {sequence_length} records")
    handles = [m if isinstance(m, capi.Model) else capi.Model(m) for m in models]
    dev = torch.device("cuda", device)
    per_slab = max(1, min(max_streams, slab_bytes // (T * REC * 4), S))
    sums = [np.zeros((S, capi.EVAL_SUMS), np.float64) for _ in handles]
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
                b.eval_records_device(d_sums.data_ptr(), 0, 0, d_rec.data_ptr(), 0, T, frame_stride=REC, row_stride=T * REC,
                                      gamma=gamma, first=first, stream=st.cuda_stream)
                sums[k][s0:s0 + n] = d_sums.cpu().numpy()  # (waits for the stream)
    for b in batches.values():
        b.close()
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(len(handles)):
            g = sums[k][:, 0] / (capi.NB_BANDS * sums[k][:, 2])
            v = sums[k][:, 1] / sums[k][:, 2]
            out.append(dict(sequences=S, **capi.eval_losses(sums[k]), per_sequence=dict(gain_loss=g, vad_loss=v, loss=g + .001 * v)))
    for m, h in zip(models, handles):
        if not isinstance(m, capi.Model):
            h.close()
    return out
