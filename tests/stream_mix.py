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
the default switches they reach every form of every stage that rn_plan (rnnoise_amd/csrc/dispatch.h) can choose, in lock-step calls
and -- under the schedule below -- in per-stream frame phase and in stream-list calls; test_stream_mix_cpu.py holds them to that.

The presence schedule (`KINDS`, `presence()`, `LISTED`, `RESET`) runs the same block through the serving API: masked calls,
stream-list calls and lock-step calls on a batch in per-stream frame phase, and a per-stream reset between two calls.  It is defined
on block positions, so every copy of a position gets the same frames and one oracle run per position (`oracle_block` with
`presence` and `resets`) covers the whole batch.
"""
from __future__ import annotations

import functools
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


def call_frames(c, calls=CALLS):
    """the frames of call c"""
    first = ([0] + call_starts(calls))[c]
    return range(first, first + calls[c])


# ---- the presence schedule: what each call of CALLS is, and which block positions have which frames ----
# The first call puts the batch into per-stream frame phase (include/rnnoise_amd.h); every kind then runs as a one-frame call and as a
# pipelined one.  "lock": rnnoise_batch_process_device on the batch in per-stream phase (every stream present).
KINDS = ("masked", "list", "list", "lock", "lock", "masked", "masked")
RESET_BEFORE = 4                          # RESET's positions are reset (every copy: rnnoise_batch_reset_streams) before this call
OUT_OF_RANGE = (-1, None, 2 ** 31 - 1)    # list entries that name no stream (None: the batch's size), at the front, middle and end


def _rng(tag):
    return np.random.default_rng([B, T, tag])


def _pick(rng, share, avoid=()):
    keep = [int(p) for p in rng.permutation(B) if p not in avoid]
    return tuple(sorted(keep[:round(share * B)]))


# hand-made rows of presence() (positions below 251, so that the smallest case has them): absent from every masked and list frame
# ("never"), present in one of them ("once"), in every other one ("alternating"), and absent from only the first / only the last
# frame of the list call 1 and of the masked call 6
SPECIAL = dict(zip(("never", "once", "alternating", "first1", "last1", "first6", "last6"), (5, 12, 19, 26, 33, 40, 47)))
# LISTED[c]: the block positions listed in list call c, about 70 % (the hand-made rows that must show in call 1 and 2 always)
LISTED = {c: tuple(sorted(set(_pick(_rng(c), 0.7)) - {SPECIAL["never"]} | {SPECIAL[k] for k in ("once", "alternating", "first1", "last1")}))
          for c, kind in enumerate(KINDS) if kind == "list"}
# RESET: about 8 % of the block positions, every copy reset (rnnoise_batch_reset_streams) before call RESET_BEFORE
RESET = _pick(_rng(99), 0.08, avoid=set(SPECIAL.values()))


@functools.lru_cache(None)
def labels():
    """the category of every block position, and every position's index within its category"""
    _, lab = _layout()
    src = [(p * STEP) % B for p in range(B)]
    return [lab[s] for s in src], [s - lab.index(lab[s]) for s in src]


@functools.lru_cache(None)
def _presence():
    rng = _rng(6)
    lab, nth = labels()
    a = rng.random((T, B)) < rng.uniform(0.45, 0.95, B)
    a[0] = np.arange(B) % 3 != 0                              # the first call: both kinds among every three neighbours
    lock = [t for c, k in enumerate(KINDS) if k == "lock" for t in call_frames(c)]
    free = np.array([t for t in range(T) if t not in lock])   # the frames of masked and list calls
    # around the silent runs: a zero_runs stream misses the first zero frame of a run (the next frame's window then spans the last
    # present frame, which is live) or the first live frame after it (the next present frame's window spans the run's last zero frame)
    k = 0
    for p in range(B):
        if lab[p] == "zero_runs":
            for a0, b0 in _ZERO_RUNS[nth[p]]:
                t = a0 if k % 2 == 0 else b0
                if b0 - a0 >= 2 and t < T and t not in lock:
                    a[t, p] = False
                k += 1
    for name, p in SPECIAL.items():
        a[free, p] = False
        if name == "once":
            a[20, p] = True
        elif name == "alternating":
            a[free[::2], p] = True
        elif name != "never":
            fr = list(call_frames(int(name[-1])))
            a[fr, p] = True
            a[fr[0] if name.startswith("first") else fr[-1], p] = False
    for c, kind in enumerate(KINDS):
        fr = list(call_frames(c))
        if kind == "lock":
            a[fr] = True
        elif kind == "list":
            off = np.ones(B, bool)
            off[list(LISTED[c])] = False
            a[np.ix_(fr, np.flatnonzero(off))] = False
    return a.astype(np.uint8)


def presence():
    """(T, B) uint8: 1 where block position p has frame t under the schedule of KINDS.  Lock-step calls: every position.  A list call:
    the positions it does not list are absent from all of its frames, the listed ones follow the mask.  SPECIAL has the hand-made
    rows; zero_runs streams miss a frame at the edge of a silent run."""
    return _presence().copy()


def list_rows(n, c):
    """the stream list of list call c on a batch of n copies of the block (stream i takes position i mod B): every copy of the
    positions LISTED[c] in a fixed pseudo-random order, and the entries of OUT_OF_RANGE at the front, the middle and the end.  int32"""
    keep = np.zeros(B, bool)
    keep[list(LISTED[c])] = True
    rows = np.flatnonzero(keep[np.arange(n) % B])
    rows = _rng(100 + c).permutation(rows)
    bad = [n if e is None else e for e in OUT_OF_RANGE]
    mid = len(rows) // 2
    return np.concatenate([[bad[0]], rows[:mid], [bad[1]], rows[mid:], [bad[2]]]).astype(np.int32)


def call_plan(n, c):
    """what call c of KINDS hands a batch of n copies of the block (stream i takes position i mod B): "kind", "frames" (of the
    block), "rows" (the int32 stream list of a list call, else None: one row per stream), "src" (the block position each row reads;
    0 for an entry that names no stream), "present" ((frames, rows) bool: what the row is promised) and "active" (the (frames, rows)
    uint8 mask the call takes, None for a lock-step call; an out-of-range list entry is marked present there -- its row is absent
    all the same)"""
    frames = call_frames(c)
    pres = presence()[frames.start:frames.stop] != 0
    rows = active = None
    if KINDS[c] == "list":
        rows = list_rows(n, c)
        named = (rows >= 0) & (rows < n)
        src = np.where(named, rows, 0) % B
        present = pres[:, src] & named
        active = np.where(named, present, True).astype(np.uint8)
    else:
        src = np.arange(n) % B
        present = pres[:, src]
        if KINDS[c] == "masked":
            active = present.astype(np.uint8)
    present = np.ascontiguousarray(present)
    active = None if active is None else np.ascontiguousarray(active)     # (the calls take it frame by frame, row-major)
    return dict(kind=KINDS[c], frames=frames, rows=rows, src=src, present=present, active=active)


def call_input(blk, frames, src, present):
    """the input rows of a call of call_plan(): the block's frames for every row, NaN in every absent one (the header promises that
    absent rows are not read).  blk (T, B, 480), src and present as call_plan() gives them -- numpy arrays, or torch tensors on one
    device"""
    x = blk[frames.start:frames.stop][:, src]
    x[~present] = float("nan")
    return x


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


def oracle_block(blob, pcm, streams=None, collect_state=True, presence=None, resets=None):
    """the oracle over the streams of a (T, n, 480) block (all of them, or the listed ones), several streams at a time: every stream
    has an Oracle of its own, and the oracle's C calls release the GIL.  Same keys as test_gpu_parity.oracle_run.
    presence: (T, n) -- each stream's oracle runs on its present frames only; the absent frames hold what include/rnnoise_amd.h
    promises for them: out 0 (untouched), vad 0, 32 zero gains, silence 2, features and pitch 0 (undefined), and "present" (T, n)
    bool comes back too.  resets: streams that restart from a fresh Oracle at the first frame of call RESET_BEFORE of CALLS."""
    from oracle.binding import Oracle
    streams = list(range(pcm.shape[1])) if streams is None else list(streams)
    Tn = pcm.shape[0]
    present = None if presence is None else np.asarray(presence)[:Tn] != 0
    resets = set(resets or ())
    cut = call_frames(RESET_BEFORE)[0]

    def one(s):
        o = Oracle(blob)
        if present is None and s not in resets:
            r = o.run(pcm[:, s])
        else:
            have = np.ones(Tn, bool) if present is None else present[:, s]
            frames = np.flatnonzero(have)
            runs = []
            for seg in ((frames[frames < cut], frames[frames >= cut]) if s in resets else (frames,)):
                if runs:
                    o = Oracle(blob)
                runs.append(o.run(pcm[seg, s]))
            part = {k: np.concatenate([x[k] for x in runs]) for k in runs[0]}
            r = {k: np.zeros((Tn,) + v.shape[1:], v.dtype) for k, v in part.items()}
            r["silence"][:] = 2
            for k, v in part.items():
                r[k][frames] = v
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
    if present is not None:
        out["present"] = present[:, streams]
    return out
