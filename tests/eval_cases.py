"""What the tests of the feature calls share (include/rnnoise_amd.h: rnnoise_batch_process_features, rnnoise_batch_eval_records;
plain helper module: tests/test_eval_records_cpu.py checks the restatement, tests/test_eval_records_gpu.py uses it).

  records()          (T = 12, D, 98): the 97 real streams of tests/train_cases.py (the oracle's records, cut to 12 frames) and six
                     synthetic edge streams -- real features, targets overwritten with -1, a value in (-1, 0), 0, tiny values, 1 and a
                     mix of them, VAD targets 0, 0.5 and 1
  oracle_outputs()   what oracle.binding's compute_rnn returns for every frame of every distinct stream, one oracle per stream
  loss_terms()       the trainer's terms (the reference's torch/rnnoise/train_rnnoise.py:149-155) restated with numpy in float64
  expected_sums()    ... summed per stream the way the eval-records calls define it: step t against record t - 1, from `first` on
"""
from __future__ import annotations

import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

T = 12
EDGE = 6            # synthetic streams behind the real ones
NB_BANDS, REC, SUMS = 32, 98, 4
TARGETS, VAD = slice(65, 97), 97
TINY = (1e-30, 1e-12)


@functools.lru_cache(None)
def records() -> np.ndarray:
    import train_cases as tc
    real = tc.oracle_records(tc.cases())[:T]
    edge = real[:, :EDGE].copy()
    band, frame = np.arange(NB_BANDS), np.arange(T)
    edge[:, 0, TARGETS], edge[:, 0, VAD] = -1.0, 0.0
    edge[:, 1, TARGETS], edge[:, 1, VAD] = -0.5, 0.5
    edge[:, 2, TARGETS], edge[:, 2, VAD] = 0.0, 1.0
    edge[:, 3, TARGETS], edge[:, 3, VAD] = np.where(band % 2, TINY[0], TINY[1]), 0.5
    edge[:, 4, TARGETS], edge[:, 4, VAD] = 1.0, 1.0
    mix = np.array([-1.0, -0.5, 0.0, 1e-20, 1.0, 0.3], np.float32)
    edge[:, 5, TARGETS] = mix[(band[None, :] + frame[:, None]) % len(mix)]
    edge[:, 5, VAD] = np.array([0.0, 0.5, 1.0], np.float32)[frame % 3]
    rec = np.ascontiguousarray(np.concatenate([real, edge], axis=1), np.float32)
    assert rec.shape == (T, tc.D + EDGE, REC) and np.isfinite(rec).all()
    rec.setflags(write=False)
    return rec


@functools.lru_cache(None)
def oracle_outputs(blob_name: str = "default"):
    """(gains (T, D, 32), vad (T, D)) of the blob on records(), read-only"""
    from conftest import load_blob
    from oracle.binding import Oracle
    blob, rec = load_blob(blob_name), records()

    def one(s):
        o = Oracle(blob)
        out = [o.compute_rnn(rec[t, s, :65]) for t in range(T)]
        return np.stack([g for g, _ in out]), np.array([v for _, v in out], np.float32)

    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        res = list(pool.map(one, range(rec.shape[1])))
    gains, vad = np.stack([g for g, _ in res], 1), np.stack([v for _, v in res], 1)
    gains.setflags(write=False), vad.setflags(write=False)
    return gains, vad


def loss_terms(g, v, p, q, gamma=0.25):
    """g (..., 32) gain targets, v (...) VAD targets, p (..., 32) predicted gains, q (...) predicted VAD -> (gain terms (..., 32), VAD
    term (...)) in float64"""
    g, v, p, q = (np.asarray(a, np.float64) for a in (g, v, p, q))
    tg = np.maximum(g, 0.0)
    tg = tg * np.tanh(8.0 * tg) ** 2
    e = p ** gamma - tg ** gamma
    gain = (1.0 + 5.0 * v[..., None]) * np.minimum(g + 1.0, 1.0) * e ** 2
    vad = np.abs(2.0 * v - 1.0) * (-v * np.log(.01 + q) - (1.0 - v) * np.log(1.01 - q))
    return gain, vad


def frames_scored(t0, n_frames, first=4):
    return max(0, t0 + n_frames - max(t0, first, 1))


def expected_sums(rec, gains, vad, t0=0, n_frames=None, first=4, gamma=0.25, lag=1):
    """rec (T, N, 98), gains (T, N, 32), vad (T, N): the outputs of steps 0 .. T - 1 -> (N, 4) float64: step t against record
    t - lag for t in [max(t0, first, 1), t0 + n_frames)"""
    n_frames = rec.shape[0] - t0 if n_frames is None else n_frames
    out = np.zeros((rec.shape[1], SUMS), np.float64)
    for t in range(max(t0, first, 1), t0 + n_frames):
        r = rec[t - lag]
        gt, vt = loss_terms(r[:, TARGETS], r[:, VAD], gains[t], vad[t], gamma)
        out[:, 0] += gt.sum(-1)
        out[:, 1] += vt
        out[:, 2] += 1
    return out


def rel_diff(got, want):
    """largest relative difference of two arrays of sums; equal values (two zeros included) differ by 0"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(d == 0, 0.0, d / np.abs(want))
    return float(np.max(r)) if r.size else 0.0
