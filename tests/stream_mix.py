"""One mixed block of streams for the at-size parity tests (plain helper module: tests/test_stream_mix_cpu.py checks what the block
covers, tests/test_gpu_at_size.py, tests/test_dropin_gpu.py run it).

`block()` is B = 389 streams x 30 frames of float PCM.  The at-size tests lay a batch out as copies of it (stream i takes block
stream i mod B); B is prime, so the copies land at shifting offsets modulo the 4 streams of an analysis workgroup, the 16 of a tile
and the 64 of a high-pass wave or a GRU group.  The block holds the pitch range from ~60 to ~767 (fuzz_pcm), the edge goldens, the
extreme signals, white noise around the silence threshold (E < 0.04, src/denoise.c:389), exact-zero frames at and across the call
boundaries of `CALLS`, one all-zero stream, streams of the synth recipe, and fuzz_pcm padding.  A fixed permutation then spreads
every category over the block, so that neighbouring streams -- the rows of one wave in the narrow phases of rn_analysis_kernel, of
one tile, of one layer-kernel group -- take different data-dependent lengths and branches in the same frame.

No NaN or Inf anywhere: the poisoned-stream test writes its own into copies of one stream.

`CASES` are the batches of the at-size test, as (streams, network path or None for the batch's default, calls).  On 256 CUs with
the default switches they reach every form of every stage that rn_plan (rnnoise_amd/csrc/dispatch.h) can choose;
test_stream_mix_cpu.py holds them to that.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import GOLD
from rnnoise_amd import synth
from test_gpu_parity import extreme_signals, fuzz_pcm

B = 389                                   # streams of the block: prime
T = 30                                    # frames
CALLS = (1, 8, 1, 1, 5, 1, 13)            # one-frame calls first, between pipelined calls and back to back; 13 frames wrap
                                          # the 6-slot pitch ring twice
STEP = 149                                # the permutation: block position p holds stream (p * STEP) % B of the layout below

CASES = [
    (251, 0, CALLS),       # the first 251 streams: rn_nn_one_kernel, rn_synthesis_few_kernel, rn_hp_one_kernel, rn_analysis_single_kernel
    (389, 0, CALLS),       # rn_nn_one_kernel, rn_synthesis_kernel
    (389, 1, CALLS),       # tile kernel: sixteen waves in one-frame calls, eight in pipelined ones
    (389, 2, CALLS),       # layer-wise network, rn_nn_gru_w8_kernel
    (1031, None, CALLS),   # default path 1: tile 16 / tile 8, one-wave high-pass, one-stream analysis
    (3001, None, CALLS),   # rn_hp_kernel, rn_analysis_kernel, tile 16 and tile 8
    (4096, None, CALLS),   # tile 16 at its last size (256 tiles on 256 CUs)
    (4099, 0, CALLS),      # rn_nn_vector_kernel at size, rn_analysis_kernel, rn_hp_kernel
    (10277, None, CALLS),  # layer-wise network with rn_nn_gru_w8_kernel
    (40037, None, CALLS),  # layer-wise network with rn_nn_gru_kernel (w4), ragged in every unit
]


def call_starts(calls=CALLS):
    """first frame of every call after the first"""
    return [int(x) for x in np.cumsum(calls)[:-1]]


# exact-zero frames [a, b) per stream of white noise (sigma 2: live wherever it is not zero).  A frame is silent when it and the one
# before it are zero (the analysis window spans both), so the runs are placed for the silent frames to start and end at the call
# boundaries 1, 9, 10, 11, 16, 17 of CALLS -- and, with single zero frames, for zero samples in frames that are not silent
_ZERO_RUNS = [
    [(0, 1), (9, 11)],
    [(1, 9)],
    [(8, 10), (16, 30)],
    [(9, 11), (15, 17)],
    [(10, 16)],
    [(15, 17)],
    [(16, 30)],
    [(0, 1), (8, 9), (16, 17)],
    [(0, 3), (9, 11), (15, 16)],
    [(5, 6), (10, 12), (16, 18)],
]


def _layout():
    """(streams (T, n, 480) float32, category label per stream) before the permutation"""
    parts, labels = [], []

    def add(pcm, label):
        pcm = np.asarray(pcm, np.float32)
        parts.append(pcm)
        labels.extend([label] * pcm.shape[1])

    add(fuzz_pcm(160, T, 1), "fuzz1")
    add(fuzz_pcm(160, T, 2), "fuzz2")
    g = np.load(os.path.join(GOLD, "edge_default.npz"))     # (its inputs: the same on every rcpps profile)
    add(np.stack([g[f"{k}_pcm"][:T] for k in ("loud", "dc", "impulses", "gaps")], axis=1), "edge")
    add(np.stack([x.reshape(T, 480) for x in extreme_signals(T)], axis=1), "extreme")
    rng = np.random.default_rng(389)
    add(np.stack([(s * rng.standard_normal(T * 480)).reshape(T, 480) for s in np.linspace(0.35, 0.6, 12)], axis=1), "threshold")
    gaps = np.stack([(2.0 * rng.standard_normal(T * 480)).reshape(T, 480) for _ in _ZERO_RUNS], axis=1)
    for s, runs in enumerate(_ZERO_RUNS):
        for a, b in runs:
            gaps[a:b, s] = 0
    add(gaps, "zero_runs")
    add(np.zeros((T, 1, 480)), "all_zero")
    add(synth.batch_pcm([0, 37, 79, 121, 159, 251, 302, 333], T), "synth")
    n = sum(p.shape[1] for p in parts)
    add(fuzz_pcm(B - n, T, 3), "fuzz3")
    return np.concatenate(parts, axis=1), labels


def block():
    """(T, B, 480) float32, and the category of every block position"""
    pcm, labels = _layout()
    assert pcm.shape == (T, B, 480) and np.isfinite(pcm).all()
    src = [(p * STEP) % B for p in range(B)]
    return np.ascontiguousarray(pcm[:, src]), [labels[s] for s in src]


def oracle_block(blob, pcm, streams=None, collect_state=True):
    """the oracle over the streams of a (T, n, 480) block (all of them, or the listed ones), several streams at a time: every stream
    has an Oracle of its own, and the oracle's C calls release the GIL.  Same keys as test_gpu_parity.oracle_run."""
    from oracle.binding import Oracle
    streams = list(range(pcm.shape[1])) if streams is None else list(streams)

    def one(s):
        o = Oracle(blob)
        r = o.run(pcm[:, s])
        if collect_state:
            r["state"] = o.get_state()
        return r

    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(workers) as pool:
        runs = list(pool.map(one, streams))
    keys = ("out", "vad", "gains", "features", "pitch", "silence") + (("state",) if collect_state else ())
    out = {k: np.stack([r[k] for r in runs], axis=1) for k in keys if k != "state"}
    if collect_state:
        out["state"] = np.stack([r["state"] for r in runs])
    return out
