"""A zoo of weight layouts that the blob loader accepts but no exporter writes (plain helper module for the weight-layout tests).

Every entry starts from `blob.synth_model(seed, density, boost=3)` and rewrites records through `read_blob` / `write_blob`.
The loader stages each int8 layer three times -- the block stream with its group / column tables (vector kernel), row-major
chunks (the one-stream kernel and the drop-in row kernels) and a zero-filled dense MFMA image with its row sums (tile
kernels, layer-wise GRU) -- and the entries aim at the places where those copies could come apart: empty and ragged
groups, unsorted and repeated columns, k-tiles that are full or empty, int8 extremes, a non-zero int8 diagonal beside the
float one, and subnormal / signed-zero float weights.

Unless an entry says otherwise it stays inside the exporter's numeric contract -- int8 values in [-127, 127], and every
same-sign input pair of a block sums to at most 129 in magnitude -- the contract under which the oracle's exact arithmetic
equals the reference's saturating `maddubs` (src/vec_avx.h:629-634).  `int8_extremes` uses -128 with a non-negative
partner: outside the exporter's range, inside the reference's exact range.  Two entries are refused by the loader
(`refusal`): `duplicates_overflow` (merged weights outside int8) and `pair_bound_broken` (a pair sum of 130).

No entry holds a NaN, an Inf, or parameters that push a pre-activation anywhere near 2^60 ("Residuals").
"""
from __future__ import annotations

import functools
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable

import numpy as np

from rnnoise_amd import blob as rb

NIN, NOUT = rb.GRU                       # every GRU matrix: 384 inputs, 1152 outputs (z | r | h)
NG, NB = NOUT // 8, NIN // 4             # 144 groups of 8 rows, 96 possible 4-column blocks per group
GRU_LAYERS = [f"gru{k}_{side}" for k in (1, 2, 3) for side in ("input", "recurrent")]
INT8_LAYERS = ["conv2"] + GRU_LAYERS
FLOAT_LAYERS = {"conv1": rb.CONV1, "dense_out": rb.DENSE, "vad_dense": rb.VAD}


# ---- block-sparse records as lists of groups -------------------------------------------------------------------------
def groups(rec, layer):
    """[[(col, int8 block (8 rows, 4 inputs)), ...] per 8-row group] of a block-sparse layer"""
    idx, w = rec[layer + "_weights_idx"], rec[layer + "_weights_int8"].reshape(-1, 8, 4)
    out, p, b = [], 0, 0
    for _ in range(NG):
        nb = int(idx[p])
        out.append([(int(c), w[b + i].copy()) for i, c in enumerate(idx[p + 1:p + 1 + nb])])
        p += nb + 1
        b += nb
    assert p == idx.size and b == w.shape[0]
    return out


def set_groups(rec, layer, gs):
    idx, w = [], []
    for g in gs:
        idx.append(len(g))
        for c, blk in g:
            idx.append(c)
            w.append(np.asarray(blk, np.int8).reshape(32))
    rec[layer + "_weights_idx"] = np.asarray(idx, np.int32)
    rec[layer + "_weights_int8"] = np.concatenate(w).astype(np.int8) if w else np.zeros(0, np.int8)


def matrix(rec, layer):
    """the int8 matrix [out][in] the reference computes with: every block added in (int64), repeated blocks summed"""
    if layer + "_weights_idx" not in rec:   # dense int8 (conv2): [out/8][in/4][8][4]
        nin, nout = rb.CONV2
        v = rec[layer + "_weights_int8"].astype(np.int64).reshape(nout // 8, nin // 4, 8, 4)
        return v.transpose(0, 2, 1, 3).reshape(nout, nin)
    m = np.zeros((NOUT, NIN), np.int64)
    for g, blocks in enumerate(groups(rec, layer)):
        for c, blk in blocks:
            m[8 * g:8 * g + 8, c:c + 4] += blk
    return m


def blocks_of(rec, layer):
    return rec[layer + "_weights_int8"].reshape(-1, 8, 4)


def pair_sums_ok(blk):
    """no same-sign input pair (c0, c1) / (c2, c3) of a block sums to 130 or more in magnitude (the reference stays exact)"""
    b = np.asarray(blk, np.int64).reshape(-1, 4)
    a, c = b[:, 0::2], b[:, 1::2]
    same = ((a > 0) & (c > 0)) | ((a < 0) & (c < 0))
    return not (same & (np.abs(a + c) >= 130)).any()


def _sample_blocks(rng, pool, n):
    return [pool[i].copy() for i in rng.integers(0, pool.shape[0], n)]


# ---- the entries -----------------------------------------------------------------------------------------------------
def _empty_groups(rec, rng):
    for layer in GRU_LAYERS:                        # first and last group of every GRU matrix
        gs = groups(rec, layer)
        gs[0], gs[-1] = [], []
        set_groups(rec, layer, gs)
    gs = groups(rec, "gru2_recurrent")              # every group of one gate: z of gru2's recurrent matrix
    for g in range(NIN // 8):
        gs[g] = []
    set_groups(rec, "gru2_recurrent", gs)


RAGGED_LENGTHS = [96, 0, 1, 2, 3, 4, 5, 6, 7, 0, 96, 9, 10, 11, 0, 13, 2, 6]


def _ragged_groups(rec, rng):
    """groups of 96 blocks beside empty ones and every length 1-7 (all residues mod 4): the row-major copy pads each group
    to whole chunks of four blocks, and the row kernels split a group's chunks into parts, some of which get none"""
    for li, layer in enumerate(GRU_LAYERS):
        pool = blocks_of(rec, layer).copy()
        gs = []
        for g in range(NG):
            n = RAGGED_LENGTHS[(g + 5 * li) % len(RAGGED_LENGTHS)]
            cols = np.sort(rng.choice(NB, n, replace=False)) * 4
            gs.append(list(zip(cols.tolist(), _sample_blocks(rng, pool, n))))
        set_groups(rec, layer, gs)


def _cols_descending(rec, rng):
    for layer in GRU_LAYERS:
        set_groups(rec, layer, [g[::-1] for g in groups(rec, layer)])


def _cols_shuffled(rec, rng):
    for layer in GRU_LAYERS:
        gs = groups(rec, layer)
        for g in gs:
            rng.shuffle(g)
        set_groups(rec, layer, gs)


def _duplicates(rec, rng):
    """a block listed 2-3 times in its group, the copies at scattered places (the reference sums them); merged weights fit
    int8.  From a dense model, so groups grow past 96 blocks and a layer past (384 / 4) x (1152 / 8) blocks."""
    for li, layer in enumerate(GRU_LAYERS):
        gs = groups(rec, layer)
        for k, g in enumerate(rng.choice(NG, 12, replace=False)):
            blocks = gs[g]
            if not blocks:
                continue
            j = int(rng.integers(len(blocks)))
            c, b = blocks[j]
            merged = b.astype(np.int64)
            extra = []
            for _ in range(1 + k % 2):              # 2x, 3x
                if k == 0 and np.abs(b).max() <= 63:
                    e = b.astype(np.int64)             # an exact copy
                else:
                    e = rng.integers(-40, 41, (8, 4))
                e[np.abs(merged + e) > 127] = 0
                merged = merged + e
                extra.append((c, e.astype(np.int8)))
            for e in extra:                          # next to the original (k even) or anywhere in the group
                pos = j + 1 if k % 2 == 0 else int(rng.integers(len(blocks) + 1))
                blocks.insert(pos, e)
        set_groups(rec, layer, gs)


def _duplicates_overflow(rec, rng):
    """one block listed twice whose copies sum to 200: no int8 MFMA image holds that (refused)"""
    gs = groups(rec, "gru1_input")
    c, b = gs[7][3]
    b[2, 0:2] = (100, 29)
    e = np.zeros((8, 4), np.int8)
    e[2, 0] = 100
    gs[7].insert(5, (c, e))
    set_groups(rec, "gru1_input", gs)


def _k_tiles(rec, rng):
    """groups whose blocks all lie in one 64-column k-tile of the MFMA image (whole tile or part of it), and matrices in which
    one k-tile is empty in every group (the middle tile of gru1's recurrent matrix, the last one of gru2's input matrix)"""
    pool = blocks_of(rec, "gru3_input").copy()
    gs = groups(rec, "gru3_input")
    for g in range(0, NG, 4):
        t = (g // 4) % (NIN // 64)
        cols = np.arange(16) if g % 8 == 0 else np.sort(rng.choice(16, 5, replace=False))
        gs[g] = [(64 * t + 4 * int(c), blk) for c, blk in zip(cols, _sample_blocks(rng, pool, len(cols)))]
    set_groups(rec, "gru3_input", gs)
    for layer, t in (("gru1_recurrent", 2), ("gru2_input", NIN // 64 - 1)):
        set_groups(rec, layer, [[(c, b) for c, b in g if c // 64 != t] for g in groups(rec, layer)])


EXTREME_ROWS = np.array([[127, 2, -127, -2],       # pair sums of exactly +-129
                         [-128, 5, 0, -128],        # -128 with a non-negative partner
                         [127, -127, -128, 127],
                         [64, 65, -65, -64],
                         [-127, -2, 127, 2],
                         [-128, 0, 1, -128]], np.int8)


def _int8_extremes(rec, rng):
    """+-127, same-sign pairs summing to exactly +-129, and -128 beside a non-negative partner (the exporter never writes -128;
    the reference's maddubs is still exact there: 254 * 128 < 2^15)"""
    for layer in ("conv2", "gru1_input", "gru2_recurrent", "gru3_input"):
        w = blocks_of(rec, layer).copy()
        for b in rng.choice(w.shape[0], 24, replace=False):
            rows = rng.choice(8, 3, replace=False)
            w[b, rows] = EXTREME_ROWS[rng.choice(len(EXTREME_ROWS), 3, replace=False)]
        rec[layer + "_weights_int8"] = w.reshape(-1)


def _recurrent_diagonal(rec, rng):
    """a non-zero int8 diagonal in every recurrent matrix beside the float `_weights_diag` (the exporter zeroes it); where no
    block covers a diagonal element one is inserted in column order"""
    for layer in ("gru1_recurrent", "gru2_recurrent", "gru3_recurrent"):
        gs = groups(rec, layer)
        for o in range(NOUT):
            i, g = o % NIN, o // 8
            c = 4 * (i // 4)
            cols = [cc for cc, _ in gs[g]]
            if c not in cols:
                pos = int(np.searchsorted(np.asarray(cols, np.int64), c)) if cols == sorted(cols) else len(cols)
                gs[g].insert(pos, (c, np.zeros((8, 4), np.int8)))
                cols.insert(pos, c)
            blk = gs[g][cols.index(c)][1]
            r, k = o % 8, i % 4
            v = int(rng.integers(1, 90)) * (1 if rng.integers(2) else -1)
            p = int(blk[r, k ^ 1])
            if p * v > 0 and abs(p + v) > 129:
                v = -v
            blk[r, k] = v
        set_groups(rec, layer, gs)


def _subnormals(rng, n):
    return (rng.uniform(1e-45, 1.1e-38, n) * rng.choice([-1, 1], n)).astype(np.float32)


def _float_specials(rec, rng):
    """subnormal and signed-zero float weights (conv1, dense_out, vad_dense, the recurrent diagonals) -- whole output columns
    of them with a zero bias, and scattered ones -- and int8 rows whose scale is +0 or -0"""
    for layer, (nin, nout) in FLOAT_LAYERS.items():
        fw = rec[layer + "_weights_float"].reshape(nin, nout).copy()
        bias = rec[layer + "_bias"].copy()
        m = rng.random(fw.shape)
        fw[m < 0.03] = _subnormals(rng, int((m < 0.03).sum()))
        fw[(m >= 0.03) & (m < 0.05)] = -0.0
        fw[(m >= 0.05) & (m < 0.06)] = 0.0
        if nout > 1:
            fw[:, 5] = _subnormals(rng, nin)
            bias[5] = 0.0
            fw[:, 6] = -0.0
            bias[6] = -0.0
        rec[layer + "_weights_float"] = fw.reshape(-1)
        rec[layer + "_bias"] = bias
    for layer in ("gru1_recurrent", "gru2_recurrent", "gru3_recurrent"):
        d = rec[layer + "_weights_diag"].copy()
        m = rng.random(d.size)
        d[m < 0.05] = _subnormals(rng, int((m < 0.05).sum()))
        d[(m >= 0.05) & (m < 0.08)] = -0.0
        rec[layer + "_weights_diag"] = d
    for layer, rows in (("conv2", (7, 200)), ("gru1_input", (10, 777)), ("gru2_recurrent", (500,))):
        s = rec[layer + "_scale"].copy()
        for k, r in enumerate(rows):
            s[r] = -0.0 if k % 2 else 0.0
        rec[layer + "_scale"] = s


def _pair_bound_broken(rec, rng):
    """one same-sign pair summing to 130: the reference's int16 pair products saturate there, exact arithmetic does not
    (refused)"""
    w = blocks_of(rec, "gru2_input").copy()
    w[100, 3, 0:2] = (65, 65)
    rec["gru2_input_weights_int8"] = w.reshape(-1)


@dataclass(frozen=True)
class Entry:
    name: str
    edit: Callable
    seed: int = 5
    density: float = 1 / 3
    refusal: str | None = None   # why the loader refuses it ("merged": repeated blocks leave int8, "pair": pair sum >= 130)


ENTRIES = [
    Entry("empty_groups", _empty_groups),
    Entry("ragged_groups", _ragged_groups, seed=6),
    Entry("cols_descending", _cols_descending, seed=7),
    Entry("cols_shuffled", _cols_shuffled, seed=8),
    Entry("duplicates", _duplicates, seed=9, density=1.0),
    Entry("duplicates_overflow", _duplicates_overflow, seed=10, refusal="merged"),
    Entry("k_tiles", _k_tiles, seed=11),
    Entry("int8_extremes", _int8_extremes, seed=12),
    Entry("recurrent_diagonal", _recurrent_diagonal, seed=13),
    Entry("float_specials", _float_specials, seed=14),
    Entry("pair_bound_broken", _pair_bound_broken, seed=15, refusal="pair"),
]
BY_NAME = {e.name: e for e in ENTRIES}
NAMES = [e.name for e in ENTRIES]
ACCEPTED = [e.name for e in ENTRIES if e.refusal is None]


@functools.lru_cache(maxsize=None)
def records(name) -> "OrderedDict[str, np.ndarray]":
    e = BY_NAME[name]
    rec = rb.read_blob(rb.synth_model(e.seed, e.density, boost=3))
    e.edit(rec, np.random.Generator(np.random.PCG64(1000 + e.seed)))
    return rec


@functools.lru_cache(maxsize=None)
def make(name) -> bytes:
    return rb.write_blob(records(name))


def weight_bytes(rec) -> int:
    """float layers 4 (nin nout + nout); int8 layers 32 per block + subias and scale, + 4 per index word and per
    diagonal element where present"""
    w = sum(4 * (nin * nout + nout) for nin, nout in FLOAT_LAYERS.values())
    for layer in INT8_LAYERS:
        nb = rec[layer + "_weights_int8"].size // 32
        nout = rec[layer + "_scale"].size
        w += 32 * nb + 8 * nout
        if layer + "_weights_idx" in rec:
            w += 4 * rec[layer + "_weights_idx"].size
        if layer + "_weights_diag" in rec:
            w += 4 * rec[layer + "_weights_diag"].size
    return w
