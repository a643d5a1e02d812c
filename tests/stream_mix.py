"""One mixed block of streams for the at-size parity tests (plain helper module: tests/test_stream_mix_cpu.py checks what the block
and its dressings cover; tests/test_gpu_at_size.py runs it in lock-step calls, through masked and list calls, with poisoned streams
under linked gains, through the PCM front ends, through the chunk calls and through the feature calls; tests/test_dropin_gpu.py runs it
through the drop-in API).

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

The link dressing (`LINK_CASES`, `controls()`, `slots()`, `link_presence()`, `link_list_rows()`, `oracle_groups`) runs the block
under a link count K (include/rnnoise_amd.h: rnnoise_batch_set_gain_link) with a control record and a model slot on every position:
group j of a batch is streams K j .. K j + K - 1, at positions g0 .. g0 + K - 1 with g0 = (K j) mod B.  Rows are dressed by position,
groups by g0 -- a list call lists whole groups --, so one run of the link oracle per g0 covers every copy.

The PCM dressing (`DRESS_CASES`, `rate_codes()`, `formats()`, `laws()`, `dress_input()`, `dress_call_plan()`, `dress_expectation()`)
runs the block through the PCM front ends: a rate code (8 to 48 kHz) and a format (linear, mu-law, A-law) on every position, int16
and float calls, interleaved channels and caller strides.  Its expectation is a chain on the CPU alone, one run per position.

`block_pin_runs()`, `block_run()` and `block_digest()` are the runs of the block that tests/test_oracle.py compares between the oracle
and the compiled reference, and what tests/golden/block_pins.npz records of them.

The chunk dressing (`CHUNK_CASES`, `CHUNK_PUSHES`, `chunk_schedule()`, `chunk_push_plan()`, `chunk_expectation()`, `chunk_records()`)
runs the block through the chunk calls: every position's signal as one row at the batch rate (48, 32 or 16 kHz, float or int16),
handed over in full-size and list pushes of 0 .. max_count samples, with a reset while samples are pending and a move of the whole
batch with its FIFO records.  Its expectation is the closed form of include/rnnoise_amd.h -- y = 0^M ++ z -- over one CPU chain per
position; `chunk_pin_runs()` are the oracle inputs it adds, which tests/test_oracle.py compares with the compiled reference.

The feature dressing (`FEATURE_CASES`, `FEATURE_CALLS`, `feature_records()`, `feature_expectation()`, `feature_slots()`) runs the
block through the feature calls (include/rnnoise_amd.h: rnnoise_batch_process_features, rnnoise_batch_eval_records): every position's
65 features of the lock-step oracle run -- all zero on its silent frames, which a feature call must run the network on all the same --
as 98-float records with targets of every kind the trainer's loss treats differently, walked in the cuts of `CALLS`.  Its expectation
is the oracle's compute_rnn alone, one walk per position, and the float64 restatement of tests/eval_cases.py over it.
"""
from __future__ import annotations

import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import GOLD
from rnnoise_amd import g711, resample, synth
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
def _presence_mask():
    """(T, B) bool: the schedule before a list call's choice of positions -- the mask of the masked calls, all ones in lock-step calls"""
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
        if kind == "lock":
            a[list(call_frames(c))] = True
    return a


@functools.lru_cache(None)
def _presence():
    a = _presence_mask().copy()
    for c, kind in enumerate(KINDS):
        if kind == "list":
            off = np.ones(B, bool)
            off[list(LISTED[c])] = False
            a[np.ix_(list(call_frames(c)), np.flatnonzero(off))] = False
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


def oracle_block(blob, pcm, streams=None, collect_state=True, presence=None, resets=None, engine=None):
    """the oracle over the streams of a (T, n, 480) block (all of them, or the listed ones), several streams at a time: every stream
    has an Oracle of its own, and the oracle's C calls release the GIL.  Same keys as test_gpu_parity.oracle_run.
    presence: (T, n) -- each stream's oracle runs on its present frames only; the absent frames hold what include/rnnoise_amd.h
    promises for them: out 0 (untouched), vad 0, 32 zero gains, silence 2, features and pitch 0 (undefined), and "present" (T, n)
    bool comes back too.  resets: streams that restart from a fresh Oracle at the first frame of call RESET_BEFORE of CALLS.
    engine: the class that runs a stream, oracle.binding.Oracle by default; RefHarness (the compiled reference, where oracle/_ref is
    built) runs one stream after the other."""
    from oracle import binding
    Oracle = engine or binding.Oracle
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

    workers = max(1, min(16, len(os.sched_getaffinity(0)))) if Oracle is binding.Oracle else 1
    with ThreadPoolExecutor(workers) as pool:
        runs = list(pool.map(one, streams))
    keys = ("out", "vad", "gains", "features", "pitch", "silence") + (("state",) if collect_state else ())
    out = {k: np.stack([r[k] for r in runs], axis=1) for k in keys if k != "state"}
    if collect_state:
        out["state"] = np.stack([r["state"] for r in runs])
    if present is not None:
        out["present"] = present[:, streams]
    return out


# ---- the link dressing: the block under rnnoise_batch_set_gain_link, with controls, model slots and group-wise list calls ----
# With link count K, group j of a batch is streams K j .. K j + K - 1; its member k sits at block position (g0 + k) mod B with
# g0 = (K j) mod B.  B is prime, so a batch of more than B streams has groups at every g0 that K j reaches, the ones that wrap from
# position 388 to 0 among them, and one position is member 0 of one group and member 1 of another.  Whatever dresses a row is a function
# of its position, whatever dresses a group a function of its g0: one LinkGroup run per g0 (oracle_groups) covers every copy.
#
# LINK_CASES: (streams, network path or None for the batch's default, K), n % K == 0 and n % B != 0.  On 256 CUs with the default
# switches (test_stream_mix_cpu.py holds them to it):
LINK_CASES = [
    (252, 0, 2),        # rn_nn_one_kernel, rn_synthesis_few_kernel (list calls too: ~70 % of the rows), one-wave high-pass
    (390, 0, 3),        # rn_nn_one_kernel, rn_synthesis_kernel
    (390, 1, 2),        # tile 16 in one-frame calls, tile 8 in pipelined ones
    (390, 2, 3),        # layer-wise network, rn_nn_gru_w8_kernel; the tile kernels in its list calls
    (1032, 0, 8),       # rn_nn_vector_kernel (rn_nn_one_kernel in its list calls)
    (2568, None, 8),    # rn_hp_kernel, tile 16 / tile 8, rn_analysis_kernel in lock-step calls
    (16416, None, 2),   # layer-wise network, rn_nn_gru_kernel (w4): 257 groups of 64 on 256 CUs, the last one half full
]
LINK_KS = tuple(sorted({K for _, _, K in LINK_CASES}))


def link_g0(n, K):
    """g0 of every link group of a batch of n copies of the block, (n // K,) int"""
    assert n % K == 0
    return (K * np.arange(n // K)) % B


def link_groups(K, common=False):
    """the g0 that occur for link count K in some case of LINK_CASES (common: in every one of them), ascending"""
    sets = [{int(g) for g in link_g0(n, k)} for n, _, k in LINK_CASES if k == K]
    return sorted(set.intersection(*sets) if common else set.union(*sets))


def link_index(n, K):
    """(n,) int: where stream i of a batch of n copies finds its row in arrays indexed [g0, member] flattened to [g0 * K + member]"""
    i = np.arange(n)
    return (i // K * K) % B * K + i % K


# thr of controls(): the oracle's VAD on the block (default blob, no link) is below 0.05 in 2 % of the live row-frames, below 0.3 in
# 26 %, below 0.5 in 53 %, below 0.7 in 81 % and below 0.9 in 96 %, so every value below has rows on both sides of it in one group;
# 0.05 is a gate that nearly any live sibling opens for a silent row (the silent row's own VAD is 0)
_CTL_FLOOR = (0.0, 0.05, 0.1, 0.25, 0.5)
_CTL_THR = (0.0, 0.05, 0.3, 0.5, 0.7, 0.9)
_CTL_HOLD = (0, 0, 1, 2, 5)
RESET_HOLD = 20


@functools.lru_cache(None)
def _controls():
    rng = _rng(7)
    lab, _ = labels()
    on = rng.random(B) < 0.47
    quiet = [p for p in range(B) if lab[p] in ("zero_runs", "threshold", "all_zero")]
    on[quiet[::2]] = True                                  # silent rows with a gate of their own, and silent rows without one
    ctl = np.zeros((B, 3), np.float32)
    for p in np.flatnonzero(on):
        f, t, h = rng.choice(_CTL_FLOOR), rng.choice(_CTL_THR), rng.choice(_CTL_HOLD)
        if lab[p] in ("zero_runs", "threshold", "all_zero") and t == 0:
            t = _CTL_THR[1 + p % 3]
        if f == 0 and t == 0:
            f = _CTL_FLOOR[1 + p % 4]
        ctl[p] = f, t, h if t else 0
    for p in range(0, B - 1, 5):                           # neighbours that share thr and hold: they open and close together
        if ctl[p, 1] > 0 and on[p + 1]:
            ctl[p + 1, 1:] = ctl[p, 1:]
    # every other RESET position: a high threshold and a long hold.  Such a gate opens at the group's first loud frame and would stay
    # open for the rest of the run; the restart puts the counter back to 65536 ("no voice yet"), so the gate is closed again until the
    # next frame at thr -- a reset that forgot the counter shows in `out`
    for i, p in enumerate(RESET[::2]):
        ctl[p, 1:] = (0.7, 0.9)[i % 2], RESET_HOLD
    return ctl


def controls():
    """(B, 3) float32: the control record {floor, thr, hold} of every block position; about half keep the all-zero record"""
    return _controls().copy()


@functools.lru_cache(None)
def _slots():
    s = (_rng(8).random(B) < 1 / 3).astype(np.uint8)
    for p in range(2 * B):                                 # never a whole run of 8 (cyclic: groups wrap from 388 to 0)
        if all(s[(p + k) % B] for k in range(8)):
            s[(p + 7) % B] = 0
    return s


def slots():
    """(B,) uint8: the model slot of every block position -- slot 1 (tests/golden/little.blob.xz) on about a third, never on 8 in a row"""
    return _slots().copy()


def _members(K):
    return tuple(sorted({0, K // 2, K - 1})) if K > 2 else (0, 1, 1)


@functools.lru_cache(None)
def link_listed(K, c):
    """the g0 of the groups list call c lists under link count K: about 70 % of all g0, the groups of the hand-made rows that must
    show in a list call always.  A function of g0 (and K) alone"""
    must = {(SPECIAL[k] - m) % B for k in ("once", "alternating", "first1", "last1") for m in range(K)}
    return tuple(sorted(set(_pick(_rng(300 + c), 0.7)) | must))


@functools.lru_cache(None)
def link_replaced(K, c):
    """the three (g0, member, list entry) of list call c whose list entry names no stream: the first member of one group, a middle one
    of another and the last of a third (K = 8: members 0, 4, 7; K = 2: 0, 1, 1), groups that every case of K has and the call lists,
    away from the hand-made rows.  The stream is absent for that call in EVERY copy of the group -- its history must not depend on
    the copy --: one copy's entry is replaced (link_list_rows), the others are listed and masked out for the call (link_presence)"""
    near = {(p - m) % B for p in SPECIAL.values() for m in range(K)}
    fr = list(call_frames(c))
    there = _presence_mask()[fr]
    out, rng = [], _rng(400 + 10 * K + c)
    for m, e in zip(_members(K), OUT_OF_RANGE):            # a sibling is there in every frame of the call
        ok = [g for g in link_groups(K, common=True) if g in set(link_listed(K, c)) and g not in near and g not in {x[0] for x in out}
              and there[:, [(g + k) % B for k in range(K) if k != m]].any(1).all()]
        out.append((int(rng.choice(ok)), m, e))
    return tuple(out)


LONE_CALL = 6                                              # the masked call in which the hand-made groups have one row: a silent one, a voice


@functools.lru_cache(None)
def link_lone(K):
    """(g0, member) of a hand-made group that every case of K has and that holds the all-zero stream, or None without one (K = 2): from
    the second frame of the masked call LONE_CALL on every sibling is absent and the all-zero row present -- a present row and no
    participant, for K = 8 with the row in the second half of the group"""
    z = labels()[0].index("all_zero")
    at = [((z - m) % B, m) for m in range(K) if (z - m) % B in link_groups(K, common=True)]
    return at[-1] if at else None


@functools.lru_cache(None)
def link_solo(K):
    """(g0, member) of a second hand-made group that every case of K has, all of its rows fuzz_pcm voices (never silent): from the
    second frame of the masked call LONE_CALL on the member is present and every sibling absent -- exactly one participant, for
    K = 8 the sixth row (the second trip of the fold's loop, not its first word)"""
    lab = labels()[0]
    m = 2 * K // 3
    taken = {(p - k) % B for p in SPECIAL.values() for k in range(K)}
    if link_lone(K):
        taken |= {(link_lone(K)[0] + d) % B for d in range(-K + 1, K)}
    ok = [g for g in link_groups(K, common=True) if g not in taken and all(lab[(g + k) % B].startswith("fuzz") for k in range(K))]
    return ok[len(ok) // 2], m


@functools.lru_cache(None)
def _link_presence(K):
    base = _presence_mask()
    g0 = np.arange(B)
    a = np.stack([base[:, (g0 + k) % B] for k in range(K)], axis=-1)          # (T, B, K)
    for c, kind in enumerate(KINDS):
        if kind == "list":
            fr = list(call_frames(c))
            off = np.ones(B, bool)
            off[list(link_listed(K, c))] = False
            a[np.ix_(fr, np.flatnonzero(off))] = False
            for g, m, _ in link_replaced(K, c):
                a[fr, g, m] = False
    if link_lone(K):                                       # the hand-made group: the all-zero row there, every sibling absent
        g, m = link_lone(K)
        fr = list(call_frames(LONE_CALL))[1:]
        a[np.ix_(fr, [g], [k for k in range(K) if k != m])] = False
        a[fr, g, m] = True
    g, m = link_solo(K)                                    # the second one: one voice there, every sibling absent
    fr = list(call_frames(LONE_CALL))[1:]
    a[np.ix_(fr, [g], [k for k in range(K) if k != m])] = False
    a[fr, g, m] = True
    return a


def link_presence(K):
    """(T, B, K) bool, indexed [frame, g0, member]: the schedule of KINDS for linked runs.  Masked and lock-step calls: presence()'s
    mask of the member's position.  A list call lists whole groups (link_listed), so a group keeps its members in every call and a
    row's history is a function of (g0, member); the member whose entry link_replaced() takes is absent for that call.  Two
    hand-made groups (link_lone, link_solo) have one row on its own from the second frame of the masked call LONE_CALL on"""
    return _link_presence(K).copy()


def link_list_rows(n, K, c):
    """the stream list of list call c on a batch of n copies under link count K: every copy of the groups link_listed(K, c) in a fixed
    pseudo-random group order, members ascending, and OUT_OF_RANGE's three entries in place of one member each: of the first, a middle
    and the last copy of link_replaced()'s groups.  (rows int32, g0 of every row, member of every row)"""
    g0 = link_g0(n, K)
    keep = np.zeros(B, bool)
    keep[list(link_listed(K, c))] = True
    order = _rng(200 + c).permutation(np.flatnonzero(keep[g0]))
    rows = (K * order[:, None] + np.arange(K)).astype(np.int64)
    for x, (g, m, e) in enumerate(link_replaced(K, c)):
        copies = np.flatnonzero(g0[order] == g)
        at = copies[np.argsort(order[copies])][(0, len(copies) // 2, -1)[x]]
        rows[at, m] = n if e is None else e
    return rows.reshape(-1).astype(np.int32), np.repeat(g0[order], K), np.tile(np.arange(K), len(order))


def link_call_plan(n, K, c):
    """call_plan() for a linked run: what call c of KINDS hands a batch of n copies under link count K.  "kind", "frames", "rows" (a
    list call's int32 stream list, else None), "src" (the block position of every row), "gm" (its g0 * K + member: where
    oracle_groups' arrays, flattened over [g0, member], hold it), "present" and "active" as call_plan() has them"""
    frames = call_frames(c)
    pres = _link_presence(K)[frames.start:frames.stop].reshape(len(frames), B * K)
    rows = active = None
    if KINDS[c] == "list":
        rows, g0, mem = link_list_rows(n, K, c)
        named = (rows >= 0) & (rows < n)
        gm = g0 * K + mem
        present = pres[:, gm] & named
        active = np.where(named, present, True).astype(np.uint8)
    else:
        gm = link_index(n, K)
        g0, mem = gm // K, gm % K
        present = pres[:, gm]
        if KINDS[c] == "masked":
            active = present.astype(np.uint8)
    present = np.ascontiguousarray(present)
    active = None if active is None else np.ascontiguousarray(active)
    return dict(kind=KINDS[c], frames=frames, rows=rows, src=(g0 + mem) % B, gm=gm, present=present, active=active)


def link_state_streams(n, K):
    """one stream per (g0, member) of a batch of n copies under link count K, each pair from a different copy of its group:
    (streams, their g0 * K + member)"""
    g0 = link_g0(n, K)
    streams, gm = [], []
    for x, g in enumerate(sorted(set(g0.tolist()))):
        copies = np.flatnonzero(g0 == g)
        for k in range(K):
            streams.append(int(K * copies[(7 * (K * x + k)) % len(copies)] + k))
            gm.append(g * K + k)
    return np.array(streams), np.array(gm)


def oracle_groups(blobs, pcm, K, ctl, slots, presence=None, resets=None, groups=None, restart_counter=True):
    """the link oracle (tests/link_oracle.py: LinkGroup) over the groups of the block under link count K, one run per g0 (all of them,
    or `groups`), several at a time.  blobs: the model blob of every slot; ctl (B, 3) and slots (B,) by block position; presence
    (T, B, K) as link_presence() gives it, None: every row has every frame; resets: positions that restart as new streams -- state
    and gate counter (65536: include/rnnoise_amd.h, rnnoise_batch_reset_streams) -- at the first frame of call RESET_BEFORE
    (restart_counter=False: the state alone, what a reset that forgot the counter would do -- for the tests of the tests).
    Arrays indexed [frame, g0, member]: out, vad, gains, features, pitch, silence (each row's own raw values; an absent frame holds
    what the header promises: out 0 for untouched, vad 0, 32 zero gains, silence 2), present; [frame, g0]: n (participants), g_link,
    vad_link; [g0, member]: state, gate (the counter after the last frame); [g0]: ran.  Groups that were not run hold zeros"""
    import link_oracle
    Tn = pcm.shape[0]
    groups = list(range(B)) if groups is None else [int(g) for g in groups]
    pres = None if presence is None else np.asarray(presence)[:Tn] != 0
    resets = set(resets or ())
    cut = call_frames(RESET_BEFORE)[0]
    link_oracle.lib()

    def one(g0):
        pos = [(g0 + k) % B for k in range(K)]
        grp = link_oracle.LinkGroup([blobs[slots[p]] for p in pos], K, ctl[pos])
        frames = []
        for t in range(Tn):
            if t == cut:
                for k, p in enumerate(pos):
                    if p in resets:
                        grp.reset_row(k, counter=restart_counter)
            frames.append(grp.process(pcm[t, pos], None if pres is None else pres[t, g0]))
        r = {k: np.stack([np.asarray(f[k]) for f in frames]) for k in frames[0]}
        r["state"], r["gate"] = grp.state.copy(), grp.c.copy()
        return r

    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    first = one(groups[0])                                                     # (the library's tables are built by its first call)
    with ThreadPoolExecutor(workers) as pool:
        runs = [first] + list(pool.map(one, groups[1:]))
    out = {}
    for k, v in first.items():
        lead = (B,) if k in ("state", "gate") else (Tn, B)
        out[k] = np.zeros(lead + v.shape[len(lead) - 1:], v.dtype)
    out["silence"][:] = 2
    out["ran"] = np.zeros(B, bool)
    for g0, r in zip(groups, runs):
        out["ran"][g0] = True
        for k, v in r.items():
            if k in ("state", "gate"):
                out[k][g0] = v
            else:
                out[k][:, g0] = v
    out["present"] = out["present"] != 0
    return out


# ---- the PCM dressing: the block through the rate table, the format table, caller strides, interleaved channels, the int16 calls ----
# A rate code and a format on every block position; the batch stays at 48 kHz, so every row is 480 samples wide and a position at code
# L uses the first M = frame_samples(L) of them.  A position's low-rate input is resample.down of its 48 kHz block signal from zero
# history; the expectation is a chain on the CPU alone -- decode -> resample.up -> Oracle -> resample.down -> to_s16 -> encode --, one
# run per position and variant.  The variants: "float" (float calls: no cast, no codec; the format table is set and ignored), "s16"
# (int16 calls, linear rows) and "law" (int16 calls, the position's own law).  With C > 1 interleaved channels the rows of a group
# must all be linear or all companded (include/rnnoise_amd.h), so whether a row of an int16 call is companded is a property of its
# group -- of the position of the group's first row -- and the law a property of its own position: one position is a linear row in one
# copy and a companded one in another, which is why both variants are run for every position.
#
# DRESS_CASES: (streams, network path or None for the batch's default, "int16" | "float", channels C, layout), n % C == 0 and
# n % B != 0.  Layouts: "default"; "streams" (stream-contiguous [groups][frames of the call][M][C]); "padded" (row-major, 8 samples
# behind every group slot and 16 behind every frame).  On 256 CUs with the default switches (test_stream_mix_cpu.py holds them to it;
# K0 is rn_hp_one_kernel in every call: a rate table forces it):
DRESS_CASES = [
    (252, 0, "int16", 2, "default"),        # rn_nn_one_kernel, rn_synthesis_few_kernel, one-stream analysis
    (390, 0, "float", 1, "streams"),        # rn_synthesis_kernel
    (390, 1, "int16", 3, "padded"),         # tile 16 in one-frame calls, tile 8 in pipelined ones
    (390, 2, "int16", 1, "default"),        # layer-wise network, rn_nn_gru_w8_kernel
    (1032, 0, "float", 8, "default"),       # rn_nn_vector_kernel
    (2568, None, "int16", 2, "streams"),    # above K0's lane switch (the plain batch runs rn_hp_kernel there); rn_analysis_kernel in lock-step calls
    (10278, None, "int16", 1, "default"),   # layer-wise network at size, rn_nn_gru_w8_kernel
    (16416, None, "int16", 2, "default"),   # rn_nn_gru_kernel (w4): 257 groups of 64 on 256 CUs
]
DRESS_IDS = [f"n{n}-path{p}-{t}-c{C}-{lay}" for n, p, t, C, lay in DRESS_CASES]
RATE_CODES = (1, resample.RATE_32K, 2, 3, 6)
VARIANTS = ("float", "s16", "law")
JUNK_S16 = 7777                           # what the unused int16 samples of an input buffer hold (the float ones: NaN)


def rate_codes():
    """(B,) int: the rate code of every block position.  With p = 15 c + 5 a + j: RATE_CODES[(j + 2 c) mod 5] -- every five positions
    5 b .. 5 b + 4 hold all five rates, in an order that moves on with every fifteen"""
    p = np.arange(B)
    return np.array(RATE_CODES)[(p % 5 + 2 * (p // 15)) % 5]


def formats():
    """(B,) uint8: the format of every block position (g711.LINEAR, ULAW, ALAW).  With p = 15 c + 5 a + j: (j + a) mod 3 -- any three
    neighbours within five hold all three, and a rate meets each format once in its fifteen: every fifteen positions 15 c .. 15 c + 14
    hold all fifteen (rate, format) pairs, a third of the block each format.  (No formula in p mod 3 alone: the groups of a batch with
    three channels start at the multiples of 3.)"""
    p = np.arange(B)
    return ((p % 5 + p % 15 // 5) % 3).astype(np.uint8)


def laws():
    """(B,) uint8: the law a position's rows take where they are companded -- its own format, and for a linear position (whose row is
    companded where its group is) mu-law and A-law in turn"""
    f = formats()
    return np.where(f != 0, f, 1 + np.arange(B) % 2).astype(np.uint8)


def frame_lengths():
    """(B,) int: M of every block position, the samples (bytes, where companded) of its row it uses"""
    return np.array([resample.frame_samples(int(L)) for L in rate_codes()])


def dress_companded(n, C, s16=True):
    """(n,) bool: whether stream i of an int16 batch of n copies with C channels holds G.711 bytes: its group's first row sits on a
    position whose format is a law (C = 1: its own position).  Float calls: never"""
    lead = (np.arange(n) // C * C) % B
    return (formats()[lead] != 0) & bool(s16)


def dress_formats(n, C, s16=True):
    """(n,) uint8: the format table of a dressed batch.  Int16: the row's law where its group is companded, else linear.  Float: the
    position's format, which the float calls ignore"""
    p = np.arange(n) % B
    return np.where(dress_companded(n, C), laws()[p], 0).astype(np.uint8) if s16 else formats()[p]


def dress_strides(layout, C, k, R, M=480):
    """(frame_stride, row_stride) in samples of a call of k frames and R rows under `layout`, None for the default layout"""
    if layout == "default":
        return None
    if layout == "streams":
        return M * C, k * M * C
    assert layout == "padded"
    rs = M * C + 8
    return R // C * rs + 16, rs


@functools.lru_cache(None)
def _dress_list(n, C, c):
    if C == 1:
        rows = list_rows(n, c)
        return rows, np.where((rows >= 0) & (rows < n), rows, 0).astype(np.int64)
    keep = np.zeros(B, bool)
    keep[list(LISTED[c])] = True
    on = keep[np.arange(n) % B].reshape(-1, C)
    order = _rng(500 + c).permutation(np.flatnonzero(on.any(1)))
    streams = (C * order[:, None] + np.arange(C)).astype(np.int64)
    rows = streams.copy()
    # the entries that name no stream stand for rows that LISTED[c] leaves out: those streams miss the call in every copy anyway
    free = np.argwhere(~on[order])
    taken = set()
    for m, at, e in zip((0, C // 2, C - 1), (0, len(free) // 2, len(free) - 1), OUT_OF_RANGE):   # a first, a middle, a last member
        cand = np.array([i for i in np.flatnonzero(free[:, 1] == m) if int(free[i, 0]) not in taken])
        g = int(free[cand[np.argmin(np.abs(cand - at))], 0])
        taken.add(g)
        rows[g, m] = n if e is None else e
    return rows.reshape(-1).astype(np.int32), streams.reshape(-1)


def dress_list_rows(n, C, c):
    """the stream list of list call c on a dressed batch of n copies with C channels, and the stream every row stands for.  C = 1:
    list_rows().  C > 1: whole groups -- every group with a row on a position of LISTED[c], in a fixed pseudo-random group order,
    members ascending; the rows on other positions are listed and masked out (dress_call_plan), so presence() stays a function of the
    position -- and OUT_OF_RANGE's three entries in place of a first, a middle and a last member that is masked out anyway"""
    rows, streams = _dress_list(n, C, c)
    return rows.copy(), streams.copy()


def dress_call_plan(n, C, c, scheduled=True):
    """call_plan() for a dressed batch of n copies with C channels; scheduled=False: call c of the lock-step run (every row present).
    Also "stream": the stream of every row (for a list entry that names no stream: the one it stands for)"""
    frames = call_frames(c)
    if not scheduled:
        return dict(kind="lock", frames=frames, rows=None, src=np.arange(n) % B, stream=np.arange(n),
                    present=np.ones((len(frames), n), bool), active=None)
    if KINDS[c] != "list":
        return dict(call_plan(n, c), stream=np.arange(n))
    rows, streams = dress_list_rows(n, C, c)
    named = (rows >= 0) & (rows < n)
    src = streams % B
    present = (presence()[frames.start:frames.stop] != 0)[:, src] & named
    active = np.ascontiguousarray(np.where(named, present, True).astype(np.uint8))
    return dict(kind="list", frames=frames, rows=rows, src=src, stream=streams, present=np.ascontiguousarray(present), active=active)


@functools.lru_cache(None)
def _low_input():
    pcm, _ = block()
    sig = pcm.transpose(1, 0, 2).reshape(B, T * 480)
    x = np.zeros((T, B, 480), np.float32)
    codes = rate_codes()
    for L in RATE_CODES:
        pos = np.flatnonzero(codes == L)
        M = resample.frame_samples(L)
        y = sig[pos] if L == 1 else resample.down(sig[pos], L)
        x[:, pos, :M] = y.reshape(len(pos), T, M).transpose(1, 0, 2)
    return x


def _encode(x16, law):
    """g711.encode of (..., B, 480) int16 with the law of every position"""
    return np.where((law == g711.ULAW)[:, None], g711.ulaw_encode(x16), g711.alaw_encode(x16)).astype(np.uint8)


def _decode(b, law):
    return np.where((law == g711.ULAW)[:, None], g711.ulaw_decode(b), g711.alaw_decode(b)).astype(np.int16)


@functools.lru_cache(None)
def _dress_input(variant):
    x = _low_input()
    if variant == "float":
        return x
    x16 = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return x16 if variant == "s16" else _encode(x16, laws())


def dress_input(variant):
    """(T, B, 480): what the rows of every block position hold under `variant` -- "float": resample.down / down32 of the position's
    48 kHz block signal from zero history as float32 (the position's own signal at code 1); "s16": that rounded and clipped to int16;
    "law": g711.encode of the int16 samples with the position's law (laws()), uint8.  The first frame_lengths()[p] entries of a row
    count, the rest are zero"""
    return _dress_input(variant).copy()


def _resampled(x, codes, segments, up):
    """x (T, B, 480) through resample.up (rows of M samples -> 480) or resample.down (480 -> M) by position, whole signal by whole
    signal: `segments` are (T, B) masks, and the frames of a position that a segment marks are, concatenated, one signal from zero
    history (tests/test_resample_cpu.py: streaming equals the whole signal).  Frames in no segment come back zero; code 1 passes"""
    y = np.zeros((T, B, 480), np.float32)
    for L in RATE_CODES:
        pos = np.flatnonzero(codes == L)
        M = resample.frame_samples(L)
        w_in, w_out = (M, 480) if up else (480, M)
        for seg in segments:
            sel = seg[:, pos]
            if L == 1:
                y[:, pos] = np.where(sel[..., None], x[:, pos], y[:, pos])
                continue
            order = np.argsort(~sel, axis=0, kind="stable")                     # every position's marked frames first, in order
            packed = np.take_along_axis(x[:, pos, :w_in], order[..., None], axis=0)
            packed[np.arange(T)[:, None] >= sel.sum(0)[None]] = 0
            sig = packed.transpose(1, 0, 2).reshape(len(pos), T * w_in)
            res = (resample.up if up else resample.down)(sig, L).reshape(len(pos), T, w_out).transpose(1, 0, 2)
            back = np.zeros((T, len(pos), w_out), np.float32)
            np.put_along_axis(back, order[..., None], res, axis=0)
            y[:, pos, :w_out] = np.where(sel[..., None], back, y[:, pos, :w_out])
    return y


DRESS_MUTANTS = ("absent_advances", "reset_keeps_history", "encode_before_cast")


def dress_expectation(blob, variant, scheduled, mutant=None):
    """the CPU chain over every block position under `variant` (VARIANTS), lock-step or (scheduled) under presence() with RESET's
    restarts before call RESET_BEFORE: an absent frame advances neither the denoiser nor the resampler histories, a reset zeroes both.
    Keys as oracle_block, "out" (T, B, 480) in the variant's type (float32 | int16 | uint8 codes): the first frame_lengths()[p] entries
    of a present row, zeros elsewhere.  mutant (DRESS_MUTANTS) -- for the tests of the tests: a chain whose resampler histories advance
    over absent frames, one whose reset leaves them, one that encodes the rounded float output instead of the truncated int16"""
    assert variant in VARIANTS and mutant in (None,) + DRESS_MUTANTS
    codes, law = rate_codes(), laws()
    x = _dress_input(variant)
    x = (_decode(x, law) if variant == "law" else x).astype(np.float32)
    pres = presence() != 0 if scheduled else np.ones((T, B), bool)
    restart = np.zeros(B, bool)
    if scheduled and mutant != "reset_keeps_history":
        restart[list(RESET)] = True
    after = (np.arange(T) >= call_frames(RESET_BEFORE)[0])[:, None] & restart[None]
    run = np.ones((T, B), bool) if mutant == "absent_advances" else pres
    segments = (run & ~after, run & after)
    v = _resampled(x, codes, segments, up=True)
    r = oracle_block(blob, v, presence=pres, resets=RESET) if scheduled else oracle_block(blob, v)
    y = _resampled(r["out"], codes, segments, up=False)
    y[~pres] = 0
    if variant != "float":
        y16 = resample.to_s16(y)
        if variant == "law":
            y = _encode(np.clip(np.rint(y), -32768, 32767).astype(np.int16) if mutant == "encode_before_cast" else y16, law)
            y[~(pres[..., None] & (np.arange(480) < frame_lengths()[:, None])[None])] = 0
        else:
            y = y16
    r["out"], r["present"] = y, pres
    return r


# ---- the block through the compiled reference (tests/test_oracle.py; tests/golden/make_golden.py --block-pins) ----
PIN_KEYS = ("out_crc", "gains_crc", "features_crc", "vad", "pitch", "silence", "state_crc")


def block_pin_runs():
    """the runs of the block that tie the oracle to the reference, as (tag, blob name, block positions, scheduled): every position on
    the default model, and on the sparser one the first 40 of the positions that carry model slot 1 under the link dressing (slots());
    each in lock step and under presence() with RESET's restarts"""
    little = [int(p) for p in np.flatnonzero(slots() == 1)[:40]]
    return [(f"{name}_{'sched' if scheduled else 'lock'}", name, pos, scheduled)
            for name, pos in (("default", list(range(B))), ("little", little)) for scheduled in (False, True)]


def block_run(blob, positions, scheduled, engine=None):
    """oracle_block over `positions` of the block on `engine` (the oracle, or oracle.binding.RefHarness): lock-step, or each position's
    present frames with a fresh state at RESET's restart"""
    pcm, _ = block()
    if not scheduled:
        return oracle_block(blob, pcm, streams=positions, engine=engine)
    return oracle_block(blob, pcm, streams=positions, presence=presence(), resets=RESET, engine=engine)


def block_digest(r):
    """what tests/golden/block_pins.npz holds of a block_run(): CRC32 per (frame, position) of out, gains and features, vad as float32,
    pitch as int16, silence as int8, one CRC32 of the final state per position (PIN_KEYS)"""
    import zlib

    def crc(a):
        a = np.ascontiguousarray(a)
        flat = a.reshape(-1, a.shape[-1])
        return np.array([zlib.crc32(row.tobytes()) for row in flat], np.uint32).reshape(a.shape[:-1])

    return dict(out_crc=crc(r["out"]), gains_crc=crc(r["gains"]), features_crc=crc(r["features"]), vad=r["vad"].astype(np.float32),
                pitch=r["pitch"].astype(np.int16), silence=r["silence"].astype(np.int8), state_crc=crc(r["state"]))


# ---- the chunk dressing: the block through the chunk calls (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks[_list]) ----
# Position p's signal is one row of T M samples at the case's rate (M = 480 rate / 48000), handed over in the pushes of CHUNK_PUSHES:
# counts[q, p] new samples in push q, a function of the position, so one CPU chain per position covers every copy.  The expectation is
# cumulative sums and slices of the closed form the header promises -- y = 0^M ++ z --; nothing of rnnoise_amd/csrc/chunk_plan.h is
# ported here.
#
# CHUNK_CASES: (streams, network path or None for the batch's default, rate in Hz, "float" | "int16"), n % B != 0.  On 256 CUs with the
# default switches (test_stream_mix_cpu.py holds them to it; a low batch rate forces rn_hp_one_kernel at every size):
CHUNK_CASES = [
    (252, 0, 48000, "float"),       # rn_nn_one_kernel, rn_synthesis_few_kernel, rn_hp_one_kernel
    (390, 1, 48000, "int16"),       # tile 16 in F = 1 pushes, tile 8 in pipelined ones, rn_synthesis_kernel
    (390, 2, 16000, "int16"),       # layer-wise network, rn_nn_gru_w8_kernel; M = 160, rows packed 160 apart
    (1031, 0, 32000, "float"),      # rn_nn_vector_kernel behind the 2:3 resampler, M = 320
    (3001, None, 48000, "float"),   # rn_hp_kernel (lane = stream) in place, both tile kernels
    (4099, 0, 48000, "int16"),      # rn_nn_vector_kernel at size behind rn_hp_kernel
    (10277, None, 48000, "float"),  # layer-wise network, rn_nn_gru_w8_kernel just above the switch: partial tile, partial group
    (16421, None, 48000, "int16"),  # rn_nn_gru_kernel (w4): 257 groups of 64, ragged in every unit
]
CHUNK_IDS = [f"n{n}-path{p}-{hz}-{typ}" for n, p, hz, typ in CHUNK_CASES]
CHUNK_VARIANTS = tuple(sorted({(hz, typ) for _, _, hz, typ in CHUNK_CASES}))

# A push: max_count (a, b) = a M + b samples, so that one schedule serves every rate; its form; for a list push the share of the
# positions it lists; and its recipe: the count of position p is recipe[(p + shift) % len(recipe)], with
#   (a, b)  a M + b samples            "J"  jitter(p, M): a count of the position's own, 12 .. M - 13
#   "U"     unlisted (list pushes)     "T"  the tail: whatever brings the position to its total (_chunk_tail)
# The recipes are Latin: with the shifts 0, 1, 2 .. of the pushes that share a recipe every position takes every entry once -- the
# special counts 0, 1, M - 1, M, M + 1, 2 M and the push's max_count (M in the small pushes, 2 M in the big ones), in a full-size push
# and while listed -- and any four (five) neighbours hold all of a recipe's entries in every push.
# Where a rule of the schedule cannot hold as a sentence, it holds as far as it can (test_stream_mix_cpu.py asserts exactly this): a
# push with F = 1 has two values of k, not three; before the first push every FIFO is empty, so the fills mix from the second on; the
# position that no list push lists takes its special counts in full-size pushes only, the one in every other list push those of
# the list pushes it is in.
_SMALL = ((1, 0), (0, 0), (0, 1), (1, -1))                 # M = max_count (k = 1 = F), 0, 1, M - 1
_BIG = ((2, 0), (0, 0), (1, 1), (1, 0))                    # 2 M = max_count (k = 2 = F), 0, M + 1, M (k = 1)
_KINDS = {                                                 # kind: (max_count, form, recipe)
    "J": ((1, 0), "full", ((1, 0), "J", "J", "J")),        # the first push: a fill of its own on three positions in four
    "S": ((1, 0), "full", _SMALL),
    "s": ((1, 0), "list", _SMALL + ("U",)),
    "B": ((2, 0), "full", _BIG),
    "b": ((2, 0), "list", _BIG + ("U",)),
    "T7": ((7, 0), "full", ("T",)),                        # F = 7: the 6-slot pitch ring wraps inside one chunk call
    "t7": ((7, -1), "full", ("T",)),                       # ... with rows an odd number of samples apart
    "T4": ((4, 0), "full", ("T",)),
}
# full F = 1, list F = 1, full F = 2 and list F = 2 back to back, then alternating in form and schedule, then the tail
_ORDER = ("J", "S", "S", "s", "s", "B", "B", "b", "b", "S", "b", "S", "b", "s", "B", "s", "B", "s", "b", "T7", "t7", "T7", "T4")


def _pushes():
    seen, out = {}, []
    for kind in _ORDER:
        mc, form, recipe = _KINDS[kind]
        share = None if form == "full" else 1 - recipe.count("U") / len(recipe)
        out.append(dict(max_count=mc, form=form, share=share, recipe=recipe, shift=seen.get(kind, 0), tail=recipe == ("T",)))
        seen[kind] = seen.get(kind, 0) + 1
    return tuple(out)


CHUNK_PUSHES = _pushes()
CHUNK_RESET_BEFORE = 7                    # RESET's positions are reset (every copy) before this push ...
CHUNK_MOVE_BEFORE = 13                    # ... and the whole batch moves to a fresh one before this one
CHUNK_MUTANTS = ("no_delay", "reset_keeps_pending", "reset_keeps_history", "frames_late", "cast_before_down", "list_advances_unlisted")


def chunk_frame(hz):
    """M: the samples of a frame at a batch rate of hz"""
    return 480 * hz // 48000


def chunk_jitter(M):
    """(B,) int: a count of the position's own, 12 .. M - 13 (53 is coprime to M - 24 for M = 480, 320, 160)"""
    return 12 + (np.arange(B) * 53) % (M - 24)


_TAIL_IDLE_TOO = (3, 131, 259)


def _chunk_tail(M, cum, total, maxes, max_last):
    """the counts of the tail's pushes -- max_count maxes[t], and max_last in the last one --, which bring position p to total[p].
    Three kinds of position.  "Idle" ones -- p mod 4 = 1 without SPECIAL's "never", and _TAIL_IDLE_TOO: three more, one of them in the
    gap that "never" and the wrap from 388 to 0 leave -- keep max_last samples for the last push (k = F there), and the j-th of them
    pushes nothing in tail push t where (j + t) mod 3 = 0: k = 0 on one in any three of them.  Those with p mod 4 = 0 are done before
    the last push (k = 0 there), the others keep M - jitter for it (fill jitter, k = 1); both push max_count (k = F) in tail push t
    where (p + t) mod 4 = 0.  All of that wherever the rest still fits the other pushes; what is free takes whole frames first, so that
    the fills stay as mixed as they were"""
    jit = chunk_jitter(M)
    idle = [p for p in range(B) if (p % 4 == 1 and p != SPECIAL["never"]) or p in _TAIL_IDLE_TOO]
    assert len(idle) % 3 == 0                              # (cyclic: the copies wrap from 388 to 0)
    last = np.select([np.isin(np.arange(B), idle) | (np.arange(B) == SPECIAL["never"]), np.arange(B) % 4 == 0], [max_last, 0], M - jit)
    last = last + np.maximum(0, total - last - cum - sum(maxes))          # (a position that list pushes left behind: what does not fit)
    assert (last <= max_last).all()
    need = total - last - cum
    n_t = len(maxes)
    out = np.zeros((n_t + 1, B), np.int64)
    for p in range(B):
        if p in idle:
            want = ["zero" if (idle.index(p) + t) % 3 == 0 else None for t in range(n_t)]
        else:
            want = ["max" if (p + t) % 4 == 0 else None for t in range(n_t)]
        D = int(need[p])
        assert 0 <= D <= sum(maxes), (p, D)
        if D < sum(m for w, m in zip(want, maxes) if w == "max"):
            want = [None if w == "max" else w for w in want]
        fixed = sum(m for w, m in zip(want, maxes) if w == "max")
        if D - fixed > sum(m for w, m in zip(want, maxes) if w is None):
            want = [None if w == "zero" else w for w in want]
        rest = D - fixed
        free = [t for t in range(n_t) if want[t] is None]
        for i, t in enumerate(free):
            later = sum(maxes[u] for u in free[i + 1:])
            if i + 1 == len(free):
                n = rest
            else:
                n = min(maxes[t], rest, -(-rest // (len(free) - i) // M) * M)
                n = max(n, rest - later)
            assert 0 <= n <= maxes[t], (p, t, n)
            out[t, p] = n
            rest -= n
        for t in range(n_t):
            if want[t] == "max":
                out[t, p] = maxes[t]
    out[n_t] = last
    assert (out.sum(0) + cum == total).all()
    return out


@functools.lru_cache(None)
def chunk_schedule(M):
    """the schedule of CHUNK_PUSHES at frame length M, everything by block position: "counts" (Q, B) int32; "listed" (Q, B) bool (all
    true in a full-size push); "max_count", "F" (Q,); "cum" (Q + 1, B): samples pushed before push q; "base": the value of cum at the
    position's last restart before push q (0, or for RESET's positions from CHUNK_RESET_BEFORE on the samples pushed until then);
    "fill" = (cum - base) % M and "done" (frames completed) before push q, a restart before it included; "fill_after" (Q, B): the
    fill push q leaves; "k" (Q, B) = done[q + 1] - done[q]; "total" (B,)."""
    Q = len(CHUNK_PUSHES)
    jit = chunk_jitter(M)
    counts, listed = np.zeros((Q, B), np.int64), np.ones((Q, B), bool)
    maxc = np.array([a * M + b for a, b in (p["max_count"] for p in CHUNK_PUSHES)])
    reset = np.zeros(B, bool)
    reset[list(RESET)] = True
    nth_list = 0
    first_tail = min(q for q, p in enumerate(CHUNK_PUSHES) if p["tail"])
    assert all(p["tail"] for p in CHUNK_PUSHES[first_tail:]) and CHUNK_RESET_BEFORE < CHUNK_MOVE_BEFORE < first_tail
    for q, push in enumerate(CHUNK_PUSHES[:first_tail]):
        rec = push["recipe"]
        for p in range(B):
            e = rec[(p + push["shift"]) % len(rec)]
            if q == 0 and reset[p]:
                e = "J"                                    # a fill that no sum of special counts brings back to 0 before the reset
            if push["form"] == "list":
                if p == SPECIAL["never"] or (p == SPECIAL["alternating"] and nth_list % 2):
                    e = "U"
                elif p == SPECIAL["alternating"] and e == "U":
                    e = "J"
            if e == "U":
                listed[q, p] = False
            else:
                counts[q, p] = jit[p] if e == "J" else e[0] * M + e[1]
        nth_list += push["form"] == "list"
    cum = np.concatenate([np.zeros((1, B), np.int64), np.cumsum(counts, 0)])
    c_r = np.where(reset, cum[CHUNK_RESET_BEFORE], 0)
    total = c_r + (T * M - c_r) // M * M
    counts[first_tail:] = _chunk_tail(M, cum[first_tail], total, [int(m) for m in maxc[first_tail:-1]], int(maxc[-1]))
    assert (counts <= maxc[:, None]).all() and (counts >= 0).all() and not counts[~listed].any()
    cum = np.concatenate([np.zeros((1, B), np.int64), np.cumsum(counts, 0)])
    base = np.where((np.arange(Q + 1) >= CHUNK_RESET_BEFORE)[:, None], c_r[None], 0)
    fill = (cum - base) % M
    done = base // M + (cum - base) // M
    r = dict(counts=counts.astype(np.int32), listed=listed, max_count=maxc, F=(M - 1 + maxc) // M, cum=cum, base=base, fill=fill,
             fill_after=(cum[1:] - base[:-1]) % M, done=done, k=np.diff(done, axis=0), total=total)
    for v in r.values():
        v.setflags(write=False)
    return r


def chunk_counts(M):
    """(pushes, B) int32: the samples position p hands over in push q at frame length M"""
    return chunk_schedule(M)["counts"].copy()


def chunk_list_rows(n, q, M=480):
    """the stream list of list push q on a batch of n copies of the block: every copy of the positions the push lists in a fixed
    pseudo-random order, and the entries of OUT_OF_RANGE at the front, the middle and the end (as list_rows()).  int32"""
    assert CHUNK_PUSHES[q]["form"] == "list"
    keep = chunk_schedule(M)["listed"][q]                  # (the same positions at every M)
    rows = _rng(600 + q).permutation(np.flatnonzero(keep[np.arange(n) % B]))
    bad = [n if e is None else e for e in OUT_OF_RANGE]
    mid = len(rows) // 2
    return np.concatenate([[bad[0]], rows[:mid], [bad[1]], rows[mid:], [bad[2]]]).astype(np.int32)


def chunk_push_plan(n, q, M):
    """what push q hands a batch of n copies: "rows" (the int32 stream list of a list push, else None: one row per stream), "named"
    (the row's entry names a stream), "src" (the block position of every row; 0 for an entry that names no stream) and "counts"
    (int32 per row; the three rows whose entry names no stream carry max_count // 2, 1 and max_count of position 0's samples)"""
    s = chunk_schedule(M)
    if CHUNK_PUSHES[q]["form"] == "full":
        src = np.arange(n) % B
        return dict(rows=None, named=np.ones(n, bool), src=src, counts=s["counts"][q][src])
    rows = chunk_list_rows(n, q, M)
    named = (rows >= 0) & (rows < n)
    src = np.where(named, rows, 0) % B
    counts = np.where(named, s["counts"][q][src], 0).astype(np.int32)
    counts[~named] = int(s["max_count"][q]) // 2, 1, int(s["max_count"][q])
    return dict(rows=rows, named=named, src=src, counts=counts)


@functools.lru_cache(None)
def _chunk_signal(hz):
    pcm, _ = block()
    sig = np.ascontiguousarray(pcm.transpose(1, 0, 2).reshape(B, T * 480))
    L = resample.RATES[hz]
    return sig if L == 1 else np.ascontiguousarray(resample.down(sig, L), np.float32)


def chunk_signal(hz, typ):
    """(B, T M): position p's block signal as one row at the batch rate -- block()[:, p] itself at 48 kHz, resample.down of it from
    zero history below (as dress_input) --, float32, or for "int16" rounded and clipped (as dress_input("s16"))"""
    x = _chunk_signal(hz)
    return x.copy() if typ == "float" else np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _by_length(items, fn):
    """fn over the rows of `items` {key: 1-D array}, batched by length -> {key: result row}"""
    out = {}
    for n in sorted({len(v) for v in items.values()}):
        keys = [k for k, v in items.items() if len(v) == n]
        if n == 0:
            out.update({k: np.zeros(0, np.float32) for k in keys})
            continue
        res = fn(np.stack([items[k] for k in keys]))
        out.update({k: np.ascontiguousarray(res[i], np.float32) for i, k in enumerate(keys)})
    return out


def chunk_expectation(blob, hz, typ, lock=None, mutant=None):
    """The chunk calls' results on the CPU alone, by block position.  One chain per position over its whole frames -- resample.up ->
    Oracle -> resample.down -> (int16: resample.to_s16) -- gives z; the position's output, all pushes concatenated, is then

        y = 0^M ++ z                                 (a plain position)
        y = (0^M ++ z1)[:c] ++ 0^M ++ z2             (a position of RESET, restarted with c samples pushed, c = k1 M + f, 0 < f < M)

    A restart drops the f pending samples and the output FIFO.  Until then the position had been handed c samples: the M zeros and
    the first c - M = (k1 - 1) M + f samples of z1 (nothing of z1 while c < M), so the last M - f samples of z1's frame k1 - 1 were
    still in the FIFO and are lost.  z1 is the chain over x[0 : k1 M]; z2 a second chain from zero state and zero resampler history
    over the whole frames of x[c:], and the restarted FIFO's M zeros stand in front of it.
    Push q returns y[cum[q] : cum[q + 1]], completes k = (cum'[q + 1] // M) - (cum'[q] // M) frames with cum' counted from the
    restart, and leaves cum'[q + 1] % M pending (chunk_schedule: "cum", "base", "k", "fill"); its vad / gains rows are rows
    done[q] .. done[q] + k - 1 of "vad" / "gains" below.
    -> "x" (B, T M) the input in the call's type; "y" (B, (T + 1) M) in the call's type and "yf" the same before the cast (what the
    output FIFO holds); "vad" (B, T), "gains" (B, T, 32) by completed frame; "state" (B, STATE): the oracle's after the last frame;
    "move_state": after the frames completed before push CHUNK_MOVE_BEFORE.
    lock: oracle_block's lock-step run of the block -- at 48 kHz float the plain positions take their frames from it.
    mutant (CHUNK_MUTANTS) -- for the tests of the tests: a wrong expectation of that kind."""
    from oracle import binding
    assert mutant in (None,) + CHUNK_MUTANTS and typ in ("float", "int16")
    M, L = chunk_frame(hz), resample.RATES[hz]
    s = chunk_schedule(M)
    x = chunk_signal(hz, typ)
    xf = x.astype(np.float32)
    reset = np.zeros(B, bool)
    reset[list(RESET)] = True
    c_r = s["base"][-1]
    late = int(mutant == "frames_late")
    segs = {}                                              # (position, segment): the samples of its whole frames
    for p in range(B):
        if reset[p]:
            c = int(c_r[p])
            segs[p, 0] = xf[p, late:late + (c - late) // M * M]
            start = c - (c % M if mutant == "reset_keeps_pending" else 0) + late
            segs[p, 1] = xf[p, start:start + (int(s["total"][p]) - start) // M * M]
        else:
            segs[p, 0] = xf[p, late:late + (T * M - late) // M * M]
    keep_hist = mutant == "reset_keeps_history"

    def resampled(rows, fn):
        if L == 1:
            return dict(rows)
        if not keep_hist:
            return _by_length(rows, lambda a: fn(a, L))
        joined = {p: np.concatenate([rows[p, 0]] + ([rows[p, 1]] if reset[p] else [])) for p in range(B)}
        res = _by_length(joined, lambda a: fn(a, L))
        out = {}
        for p in range(B):
            cut = len(rows[p, 0]) * len(res[p]) // max(1, len(joined[p]))
            out[p, 0] = res[p][:cut]
            if reset[p]:
                out[p, 1] = res[p][cut:]
        return out

    v = resampled(segs, resample.up)
    use_lock = lock is not None and L == 1 and typ == "float" and mutant in (None, "no_delay")
    moved = s["done"][CHUNK_MOVE_BEFORE]                   # frames completed at the move, restarts included
    # list_advances_unlisted: every list push feeds a frame of zeros to the positions it does not list
    extra = {p: [int(s["done"][q, p]) for q, push in enumerate(CHUNK_PUSHES) if push["form"] == "list" and not s["listed"][q, p]]
             for p in range(B)} if mutant == "list_advances_unlisted" else {}

    def one(p):
        o = binding.Oracle(blob)
        runs, at, move_state = [], 0, None
        for seg in range(2 if reset[p] else 1):
            if seg:
                o = binding.Oracle(blob)
            fr = v[p, seg].reshape(-1, 480)
            if use_lock and not reset[p]:
                stop = int(moved[p])
                o.run(fr[:stop]) if stop else None
                return None, o.get_state()
            cuts = sorted({0, len(fr)} | ({int(moved[p]) - at} if at <= moved[p] <= at + len(fr) else set())
                          | {e - at for e in extra.get(p, ()) if at <= e < at + len(fr)})
            for a, b in zip(cuts[:-1], cuts[1:] if len(cuts) > 1 else []):
                if at + a == moved[p] and move_state is None:
                    move_state = o.get_state()
                for _ in range(extra.get(p, ()).count(at + a)):
                    o.run(np.zeros((1, 480), np.float32))
                runs.append(o.run(fr[a:b]))
            at += len(fr)
            if at == moved[p] and move_state is None:
                move_state = o.get_state()
        r = {k: np.concatenate([x_[k] for x_ in runs]) for k in ("out", "vad", "gains")} if runs else None
        return (r, o.get_state()), move_state

    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    with ThreadPoolExecutor(workers) as pool:
        res = list(pool.map(one, range(B)))
    vad, gains = np.zeros((B, T), np.float32), np.zeros((B, T, 32), np.float32)
    state = np.zeros((B, res[0][1].shape[0]), np.float32)
    move_state = np.zeros_like(state)
    outs = {}
    for p, (r, ms) in enumerate(res):
        move_state[p] = ms
        if r is None:                                      # a plain position at 48 kHz float: the lock-step run's frames
            outs[p, 0] = lock["out"][:, p].reshape(-1)
            vad[p], gains[p], state[p] = lock["vad"][:, p], lock["gains"][:, p], lock["state"][p]
            continue
        run, state[p] = r
        K = 0 if run is None else len(run["vad"])
        if K:
            vad[p, :K], gains[p, :K] = run["vad"], run["gains"]
        k1 = len(v[p, 0]) // 480
        out = np.zeros((0, 480), np.float32) if run is None else run["out"]
        outs[p, 0] = out[:k1].reshape(-1)
        if reset[p]:
            outs[p, 1] = out[k1:].reshape(-1)
    if mutant == "cast_before_down":
        outs = {k: resample.to_s16(a).astype(np.float32) for k, a in outs.items()}
    z = resampled(outs, resample.down)
    yf = np.zeros((B, (T + 1) * M), np.float32)
    lead = 0 if mutant == "no_delay" else M + late
    for p in range(B):
        a = np.concatenate([np.zeros(lead, np.float32), z[p, 0]])
        if reset[p]:
            c = int(c_r[p])
            a = np.concatenate([a, np.zeros(c, np.float32)])[:c]
            a = np.concatenate([a, np.zeros(lead, np.float32), z[p, 1]])
        n = min(len(a), yf.shape[1])
        yf[p, :n] = a[:n]
    y = yf if typ == "float" else resample.to_s16(yf)
    return dict(x=x, y=y, yf=yf, vad=vad, gains=gains, state=state, move_state=move_state)


def chunk_records(exp, M, q):
    """(B, 964) int32: the FIFO record of every position before push q (include/rnnoise_amd.h: rnnoise_batch_save_chunk_fifos) -- the
    pending samples x[cum - fill : cum], the output FIFO y[cum : cum + M - fill] before the cast, zeros up to 480 behind either, then
    fill, M, the magic word and a zero"""
    s = chunk_schedule(M)
    rec = np.zeros((B, 964), np.float32)
    xf = exp["x"].astype(np.float32)
    for p in range(B):
        c, f = int(s["cum"][q, p]), int(s["fill"][q, p])
        rec[p, :f] = xf[p, c - f:c]
        rec[p, 480:480 + M - f] = exp["yf"][p, c:c + M - f]
    rec = rec.view(np.int32)
    rec[:, 960], rec[:, 961], rec[:, 962] = s["fill"][q], M, 0x464B4301
    return rec


# ---- the chunk dressing's oracle inputs through the compiled reference (tests/test_oracle.py; make_golden.py --block-pins) ----
def chunk_pin_runs():
    """the signals the chunk expectation feeds the oracle that no run of block_pin_runs() holds, as (tag, rate, type): the block rounded
    to int16, and the two resampled ones -- resample.up of the 16 kHz int16 and of the 32 kHz float signal.  Every position, default
    model, lock step (the 48 kHz float signal is the block itself: "default_lock")"""
    return [(f"chunk_{hz}_{typ}", hz, typ) for hz, typ in CHUNK_VARIANTS if (hz, typ) != (48000, "float")]


def chunk_pin_input(hz, typ):
    """(T, B, 480) float32: the frames chunk_expectation's chain hands the oracle for the plain positions' whole signals"""
    x = chunk_signal(hz, typ).astype(np.float32)
    L = resample.RATES[hz]
    v = x if L == 1 else resample.up(x, L)
    return np.ascontiguousarray(np.asarray(v, np.float32).reshape(B, T, 480).transpose(1, 0, 2))


def chunk_pin_run(blob, hz, typ, engine=None):
    """oracle_block over chunk_pin_input() on `engine` (the oracle, or oracle.binding.RefHarness)"""
    return oracle_block(blob, chunk_pin_input(hz, typ), engine=engine)


CHUNK_PIN_KEYS = ("frame_crc", "state_crc")


def chunk_pin_digest(r):
    """what tests/golden/block_pins.npz holds of a chunk_pin_run(): one CRC32 per (frame, position) over out, gains, features, vad, pitch
    and silence together, and one of the final state per position (CHUNK_PIN_KEYS)"""
    import zlib
    Tn, n = r["vad"].shape
    parts = [np.ascontiguousarray(r[k][..., None] if r[k].ndim == 2 else r[k]) for k in ("out", "gains", "features", "vad", "pitch", "silence")]
    frame = np.array([[zlib.crc32(b"".join(a[t, s].tobytes() for a in parts)) for s in range(n)] for t in range(Tn)], np.uint32)
    return dict(frame_crc=frame, state_crc=np.array([zlib.crc32(np.ascontiguousarray(x).tobytes()) for x in r["state"]], np.uint32))


# ---- the feature dressing: the block through the feature calls (include/rnnoise_amd.h: rnnoise_batch_process_features[_device],
# rnnoise_batch_eval_records[_device]) ----
# A feature call plans a whole batch that runs nothing beside the network, unpipelined (rnnoise_amd/csrc/batch_eval.cpp), so the forms
# it can take are those of plan:n,1,cus,path,0,0,0 of tests/csrc/dispatch_test.cpp.  FEATURE_CASES: (streams, network path or None for
# the batch's default).  On 256 CUs with the default switches (test_stream_mix_cpu.py holds them to it):
FEATURE_CASES = [
    (251, 0),          # rn_nn_one_kernel
    (389, 1),          # tile 16 (rn_nn_mfma16_kernel)
    (389, 2),          # layer-wise network, rn_nn_gru_w8_kernel on seven groups, ragged tile and group
    (4096, None),      # tile 16 at its last size (256 tiles on 256 CUs)
    (4099, 0),         # rn_nn_vector_kernel at size
    (4099, 1),         # tile 8 (rn_nn_mfma_kernel): 257 tiles on 256 CUs, the only way a feature call reaches it
    (10277, None),     # layer-wise network by size, rn_nn_gru_w8_kernel; 10277 = 16 * 642 + 5 = 64 * 160 + 37
    (40037, None),     # layer-wise network, rn_nn_gru_kernel (w4), ragged in every unit
]
FEATURE_IDS = [f"n{n}-path{p}" for n, p in FEATURE_CASES]
FEATURE_CALLS = CALLS                     # eval calls of 1, 8, 1, 1, 5, 1 and 13 frames, each with the cumulative t0
FEATURE_LAYOUTS = ("frame", "stream", "pitch100")   # [T][n][98]; [n][T][98]; rows 100 floats apart, NaN in the pad: case i takes i mod 3
FEATURE_MUTANTS = ("silent_frames_skip", "lag0", "lag2")
# the kinds of target rows: the six of eval_cases.records()' edge streams, and what dump_features writes
TARGET_KINDS = ("minus_one", "negative", "zero", "tiny", "one", "mix", "ordinary")
REC = 98                                  # floats of a record: 65 features, 32 gain targets, 1 VAD target


def target_kinds():
    """(B,) int: the index into TARGET_KINDS of every block position -- that of stream (p * STEP) % B of a layout that deals the kinds
    out in turn, as block() permutes its streams.  STEP and STEP - B are no multiples of 7, so neighbouring positions (cyclic: the
    copies wrap from 388 to 0) never share a kind"""
    return (np.arange(B) * STEP) % B % len(TARGET_KINDS)


@functools.lru_cache(None)
def _feature_targets():
    import eval_cases as ec
    rng = _rng(11)
    kind = target_kinds()
    band, frame = np.arange(32), np.arange(T)
    g = np.empty((T, B, 32), np.float32)
    v = np.empty((T, B), np.float32)
    negative = -rng.uniform(0.05, 0.95, (T, B, 32)).astype(np.float32)
    ordinary = rng.uniform(0.02, 0.98, (T, B, 32)).astype(np.float32)
    limit = rng.integers(1, 33, B)                         # band_lp: -1 from this band upward (32: no band)
    ordinary[:, band[None, :] >= limit[:, None]] = -1.0
    vad = rng.uniform(0.0, 1.0, (T, B)).astype(np.float32)
    vad[rng.random((T, B)) < 0.2] = 1.0                    # (dump_features' VAD is a probability that often sits at its ends)
    vad[rng.random((T, B)) < 0.2] = 0.0
    mix = np.array([-1.0, -0.5, 0.0, 1e-20, 1.0, 0.3], np.float32)
    # the edge kinds' VAD targets: 0, 0.5 and 1 in turn, from a start of the position's own.  The weight 1 + 5 v of a record's gain terms
    # then changes from frame to frame where the targets themselves do not: a wrong lag between step and record shows in those sums too
    turn = np.array([0.0, 0.5, 1.0], np.float32)[(frame[:, None] + np.arange(B)[None, :]) % 3]
    rows = {
        "minus_one": (np.float32(-1.0), turn),
        "negative": (negative, turn),
        "zero": (np.float32(0.0), turn),
        "tiny": (np.where(band % 2, ec.TINY[0], ec.TINY[1]).astype(np.float32)[None, None, :], turn),
        "one": (np.float32(1.0), turn),
        "mix": (mix[(band[None, :] + frame[:, None]) % len(mix)][:, None, :], turn),
        "ordinary": (ordinary, vad),
    }
    for k, name in enumerate(TARGET_KINDS):
        gk, vk = rows[name]
        on = kind == k
        g[:, on] = np.broadcast_to(gk, g.shape)[:, on]
        v[:, on] = np.broadcast_to(vk, v.shape)[:, on]
    return g, v


def feature_records(want):
    """(T, B, 98) float32: the records of the feature dressing.  want: oracle_block's lock-step run of the block on the profile the test
    runs on -- its "features" are the records' 65 features, all exactly zero where the oracle found the frame silent.  The 32 gain
    targets and the VAD target are a function of position and frame alone (a seeded generator): by position (target_kinds()) -1 on
    every band, values in (-1, 0), exact 0, eval_cases.TINY, exact 1, a mix of them that moves on with the frame -- each under VAD
    targets 0, 0.5 and 1 in turn --, and ordinary rows: targets in (0, 1) below a band limit of the position's own and -1 from it
    upward (dump_features' band_lp), VAD targets in [0, 1].  No NaN, no Inf"""
    g, v = _feature_targets()
    feats = np.asarray(want["features"], np.float32)
    assert feats.shape == (T, B, 65)
    rec = np.ascontiguousarray(np.concatenate([feats, g, v[..., None]], axis=2), np.float32)
    assert rec.shape == (T, B, REC) and np.isfinite(rec).all()
    return rec


def feature_slots():
    """(B,) uint8: the model slot of every block position in the two-model run -- slots() of the link dressing"""
    return slots()


def feature_expectation(blob, rec, slot_blobs=None, mutant=None):
    """The feature calls' results on the CPU alone, by block position: one oracle.binding.Oracle per position walks compute_rnn over
    rec[t, p, :65] for every t -- every frame, the all-zero rows too: the calls have no silence decision -- several positions at a
    time.  slot_blobs: the blob of every model slot, position p then runs on slot_blobs[feature_slots()[p]], else every position on
    `blob`.  -> "gains" (T, B, 32), "vad" (T, B), "state" (B, STATE): the oracle's get_state() after the walk (nothing but the network
    state has moved), "sums" (B, 4) float64: eval_cases.expected_sums over the whole walk.
    mutant (FEATURE_MUTANTS) -- for the tests of the tests: "silent_frames_skip": a position's all-zero rows do not run the network
    and give zero gains and VAD, as rnnoise_batch_process has it for a silent frame; "lag0" / "lag2": step t scored against record t
    / t - 2."""
    import eval_cases as ec
    from oracle import binding
    assert mutant in (None,) + FEATURE_MUTANTS and rec.shape[1:] == (B, REC)
    Tn = rec.shape[0]
    where = feature_slots() if slot_blobs is not None else np.zeros(B, np.uint8)
    blobs = slot_blobs if slot_blobs is not None else (blob,)
    skip = mutant == "silent_frames_skip"

    def one(p):
        o = binding.Oracle(blobs[where[p]])
        g, v = np.zeros((Tn, 32), np.float32), np.zeros(Tn, np.float32)
        for t in range(Tn):
            if skip and not rec[t, p, :65].any():
                continue
            g[t], v[t] = o.compute_rnn(rec[t, p, :65])
        return g, v, o.get_state()

    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        res = list(pool.map(one, range(B)))
    gains, vad = np.stack([g for g, _, _ in res], 1), np.stack([v for _, v, _ in res], 1)
    lag = {"lag0": 0, "lag2": 2}.get(mutant, 1)
    return dict(gains=gains, vad=vad, state=np.stack([s for _, _, s in res]), sums=ec.expected_sums(rec, gains, vad, lag=lag))
