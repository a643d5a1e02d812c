"""The feature calls without a GPU (include/rnnoise_amd.h: rnnoise_batch_process_features, rnnoise_batch_eval_records):

  a  rnnoise_amd_eval_records_check at its boundaries: gamma, first, t0, n_frames, and disjoint slots in both layouts
  b  the numpy restatement of the loss that tests/test_eval_records_gpu.py scores with (tests/eval_cases.py) against the same
     expression written with torch ops in float64 -- the trainer's arithmetic (the reference's torch/rnnoise/train_rnnoise.py:149-155)
  c  the Python and command-line surface
"""
import ctypes as C
import inspect
import subprocess
import sys

import numpy as np
import pytest

import eval_cases as ec
from conftest import ROOT
from rnnoise_amd import capi


# ---- a. the check ----
def ok(fs, rs, row, n, t0, T, gamma=None, first=None):
    return capi.eval_records_check(fs, rs, row, n, t0, T, gamma, first)


def test_check_config_boundaries():
    base = (0, 0, 98, 5, 0, 12)
    assert ok(*base) and ok(*base, 0.25, 4) and ok(*base, 1e-3, 0) and ok(*base, 3.0, 1000)
    for gamma in (0.0, -0.25, float("nan"), float("inf"), float("-inf")):
        assert not ok(*base, gamma, 4), gamma
    assert not ok(*base, 0.25, -1)
    # a zeroed struct and NULL are the defaults; gamma = 0 beside a first of its own is not
    L = capi.lib()
    zero = capi.EvalConfig(0.0, 0)
    assert L.rnnoise_amd_eval_records_check(C.byref(zero), 0, 0, 98, 5, 0, 12) == 1
    assert L.rnnoise_amd_eval_records_check(None, 0, 0, 98, 5, 0, 12) == 1
    assert L.rnnoise_amd_eval_records_check(C.byref(capi.EvalConfig(0.0, 1)), 0, 0, 98, 5, 0, 12) == 0
    assert L.rnnoise_amd_eval_records_check(C.byref(capi.EvalConfig(0.5, 0)), 0, 0, 98, 5, 0, 12) == 1
    assert C.sizeof(capi.EvalConfig) == 8 and capi.EVAL_SUMS == 4


def test_check_frames_and_streams():
    assert ok(0, 0, 98, 5, 0, 0) and ok(0, 0, 98, 5, 7, 0) and ok(0, 0, 98, 1, 0, 1)
    assert not ok(0, 0, 98, 5, -1, 12) and not ok(0, 0, 98, 5, 0, -1)
    assert not ok(0, 0, 98, 0, 0, 12) and not ok(0, 0, 98, -3, 0, 12)
    assert not ok(0, 0, 0, 5, 0, 12)
    assert ok(0, 0, 98, 5, 2 ** 31 - 13, 12) and not ok(0, 0, 98, 5, 2 ** 31 - 12, 12)   # t0 + n_frames stays an int


@pytest.mark.parametrize("row", [65, 98])
def test_check_layouts(row):
    n, T = 7, 12
    # [frame][n][row]: tight, and with padded rows and frames; nothing has to be a multiple of 4
    assert ok(n * row, row, row, n, 0, T) and ok(n * (row + 2) + 1, row + 2, row, n, 0, T) and ok(n * row, row, row, n, 5, 7)
    assert not ok(n * row, row - 1, row, n, 0, T)              # rows overlap
    assert not ok(n * row - 1, row, row, n, 0, T)              # frames overlap
    # [n][T][row]: a stream's frames together, streams T frames apart -- T counts from record 0, whatever t0
    assert ok(row, T * row, row, n, 0, T) and ok(row + 3, T * (row + 3), row, n, 0, T) and ok(row, T * row, row, n, 4, T - 4)
    assert not ok(row - 1, T * row, row, n, 0, T)              # frames overlap
    assert not ok(row, T * row - 1, row, n, 0, T)              # streams overlap
    assert not ok(row, (T - 1) * row, row, n, 1, T - 1)        # ... also when the call starts behind record 0
    # half a layout, negative strides
    assert not ok(0, row, row, n, 0, T) and not ok(n * row, 0, row, n, 0, T)
    assert not ok(-n * row, row, row, n, 0, T) and not ok(n * row, -row, row, n, 0, T)
    # records read as features where they lie: slots of 65 floats, 98 apart
    assert ok(n * 98, 98, 65, n, 0, T) and ok(98, T * 98, 65, n, 0, T)
    # a large file: 65,536 sequences of 2,000 records
    assert ok(98, 2000 * 98, row, 65536, 0, 2000)


def test_calls_refuse_null_arguments_without_a_gpu():
    L = capi.lib()
    assert L.rnnoise_batch_process_features_device(None, None, None, None, 0, 0, 1, None) == -1
    assert L.rnnoise_batch_process_features(None, None, None, None, 0, 0, 1) == -1
    assert L.rnnoise_batch_eval_records_device(None, None, None, None, None, 0, 0, 0, 1, None, None) == -1
    assert L.rnnoise_batch_eval_records(None, None, None, None, None, 0, 0, 0, 1, None) == -1


# ---- b. the restatement ----
def torch_terms(g, v, p, q, gamma):
    torch = pytest.importorskip("torch")
    g, v, p, q = (torch.from_numpy(np.asarray(a, np.float64)) for a in (g, v, p, q))
    v = v[..., None]
    q = q[..., None]
    target = torch.clamp(g, min=0)
    target = target * (torch.tanh(8 * target) ** 2)
    e = p ** gamma - target ** gamma
    gain = (1 + 5. * v) * torch.clamp(g + 1, max=1) * (e ** 2)
    vad = torch.abs(2 * v - 1) * (-v * torch.log(.01 + q) - (1 - v) * torch.log(1.01 - q))
    return gain.numpy(), vad[..., 0].numpy()


def edge_inputs():
    """every (target, VAD target, predicted gain, predicted VAD) combination of the edge values, as float32 like records and outputs"""
    g = np.array([-1.0, -0.75, -1e-3, 0.0, 1e-30, 1e-12, 1e-3, 0.05, 0.5, 0.999, 1.0], np.float32)
    v = np.array([0.0, 0.5, 1.0], np.float32)
    p = np.array([0.0, 1e-20, 1e-6, 0.3, 1 - 6e-8, 1.0], np.float32)
    G, V, P = np.meshgrid(g, v, p, indexing="ij")
    n = G.size
    pad = (-n) % 32
    flat = lambda a: np.concatenate([a.ravel(), a.ravel()[:pad]]).reshape(-1, 32)
    G, V, P = flat(G), flat(V)[:, 0], flat(P)
    return G, V, P, P[:, 0].copy()


@pytest.mark.parametrize("gamma", [0.25, 0.5, 1.0])
def test_numpy_restatement_is_the_trainers_arithmetic(gamma):
    G, V, P, Q = edge_inputs()
    want_g, want_v = torch_terms(G, V, P, Q, gamma)
    got_g, got_v = ec.loss_terms(G, V, P, Q, gamma)
    assert np.isfinite(want_g).all() and np.isfinite(want_v).all()
    # the same operations on the same doubles: libm against torch's vectorised pow / tanh / log, a few units in the last place of
    # p^gamma and tg^gamma (at most 1) and of the logs (at most 4.7) -- absolute, because the difference of two powers near 1 cancels
    assert np.abs(got_g - want_g).max() < 1e-14 and np.abs(got_v - want_v).max() < 1e-14
    # what the edges mean: a target of -1 masks its band, a target of 0 or below scores the prediction against 0, VAD 0.5 has no say
    assert (got_g[G == -1] == 0).all()
    assert np.allclose(got_g[(G <= 0) & (G > -1)], ((1 + 5 * V[:, None].astype(np.float64)) * (G.astype(np.float64) + 1) * P.astype(np.float64) ** (2 * gamma))[(G <= 0) & (G > -1)],
                       rtol=1e-12, atol=0)
    assert (got_v[V == 0.5] == 0).all() and (got_v[V != 0.5] != 0).all()


def test_expected_sums_alignment_and_counts():
    rng = np.random.default_rng(5)
    T, N = 9, 3
    rec = rng.random((T, N, 98)).astype(np.float32)
    gains, vad = rng.random((T, N, 32)).astype(np.float32), rng.random((T, N)).astype(np.float32)
    whole = ec.expected_sums(rec, gains, vad)
    assert (whole[:, 2] == 5).all() and (whole[:, 3] == 0).all()
    # step t against record t - 1, by hand for one stream and step
    one = ec.expected_sums(rec, gains, vad, t0=6, n_frames=1)
    g, v = ec.loss_terms(rec[5, 1, 65:97], rec[5, 1, 97], gains[6, 1], vad[6, 1])
    assert one[1, 0] == g.sum() and one[1, 1] == v and one[1, 2] == 1
    # segments add up to the whole (to rounding: the GPU tests ask the device for bit equality, not numpy)
    parts = ec.expected_sums(rec, gains, vad, 0, 5) + ec.expected_sums(rec, gains, vad, 5, 1) + ec.expected_sums(rec, gains, vad, 6, 3)
    assert ec.rel_diff(parts, whole) < 1e-14
    for t0, n, first, want in ((0, 12, 4, 8), (0, 3, 4, 0), (3, 4, 4, 3), (5, 7, 4, 7), (0, 12, 1, 11), (0, 12, 0, 11), (2, 0, 4, 0),
                               (0, 12, 12, 0), (0, 12, 20, 0), (0, 4, 4, 0), (0, 5, 4, 1), (4, 1, 4, 1)):
        assert ec.frames_scored(t0, n, first) == want, (t0, n, first)
    assert capi.eval_losses(whole)["frames_scored"] == 15
    l = capi.eval_losses(whole)
    assert l["gain_loss"] == whole[:, 0].sum() / (32 * 15) and l["vad_loss"] == whole[:, 1].sum() / 15
    assert l["loss"] == l["gain_loss"] + .001 * l["vad_loss"]


# ---- c. the surface ----
def test_python_and_cli_surface():
    from rnnoise_amd import evaluate
    assert {"rnnoise_amd_eval_records_check", "rnnoise_batch_process_features_device", "rnnoise_batch_process_features",
            "rnnoise_batch_eval_records_device", "rnnoise_batch_eval_records"} <= set(capi.EXPORTS)
    for name in ("process_features", "process_features_device", "eval_records", "eval_records_device"):
        assert callable(getattr(capi.Batch, name)), name
    sig = inspect.signature(evaluate.evaluate_records).parameters
    assert list(sig)[:7] == ["path_or_array", "models", "sequence_length", "gamma", "first", "device", "max_streams"]
    assert (sig["sequence_length"].default, sig["gamma"].default, sig["first"].default, sig["max_streams"].default) == (2000, .25, 4, 65536)
    h = subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "eval-records", "--help"], cwd=ROOT, capture_output=True, text=True).stdout
    for flag in ("--model", "--sequence-length", "--gamma", "--first"):
        assert flag in h, flag


def test_map_records_truncates_to_whole_sequences(tmp_path):
    from rnnoise_amd import evaluate
    data = np.arange(98 * 31, dtype=np.float32)
    p = tmp_path / "rec.f32"
    p.write_bytes(data.tobytes() + b"\1\2")      # a partial sequence and a partial float behind 2 whole sequences of 12... of 31 records
    m = evaluate.map_records(str(p), 12)
    assert m.shape == (2, 12, 98) and (m.reshape(-1) == data[:2 * 12 * 98]).all()
    assert evaluate.map_records(data, 31).shape == (1, 31, 98) and evaluate.map_records(data, 32).shape == (0, 32, 98)
