"""One mixed block of streams for the at-size parity tests (plain helper module: tests/test_stream_mix_cpu.py checks what the block
and its dressings cover; tests/test_gpu_at_size.py runs it in lock-step calls, through masked and list calls, with poisoned streams
under linked gains and through the PCM front ends; tests/test_dropin_gpu.py runs it through the drop-in API).

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
