"""`python -m rnnoise_amd.cli eval-records` and rnnoise_amd.evaluate.evaluate_records on a small record file the test
writes: 3 sequences of 12 records and a partial fourth, which both ignore as the trainer's RNNoiseDataset does.  The command prints
the losses the function returns; the function's sums are those of the C call on the same sequences (tests/test_eval_records_gpu.py
holds that call to the oracle and to the float64 restatement)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_cases as ec
from conftest import ROOT, load_blob
from rnnoise_amd import capi, evaluate

pytestmark = pytest.mark.gpu
SEQ = (5, 40, 101)   # distinct streams of eval_cases.records(): two real ones and an edge stream


@pytest.fixture(scope="module")
def seqs():
    """(3, 12, 98): the file's whole sequences"""
    return np.ascontiguousarray(ec.records()[:, list(SEQ)].transpose(1, 0, 2))


def test_cli_prints_the_losses_evaluate_records_returns(tmp_path, seqs):
    path = tmp_path / "val.f32"
    path.write_bytes(seqs.tobytes() + ec.records()[:7, 9].tobytes())       # ... and 7 records of a fourth sequence
    blobs = []
    for name in ("default", "little"):
        p = tmp_path / f"{name}.blob"
        p.write_bytes(load_blob(name))
        blobs.append(str(p))
    res = evaluate.evaluate_records(str(path), [load_blob("default"), load_blob("little")], sequence_length=ec.T)
    assert [r["sequences"] for r in res] == [3, 3] and [r["frames_scored"] for r in res] == [3 * ec.frames_scored(0, ec.T)] * 2
    # the C call on the same sequences, one per stream, and the restatement over the oracle's outputs
    for r, name in zip(res, ("default", "little")):
        b = capi.Batch(capi.Model(load_blob(name)), 3)
        sums, _, _ = b.eval_records(seqs, layout="stream")
        b.close()
        want = capi.eval_losses(sums)
        assert {k: r[k] for k in want} == want, (name, r, want)
        g, v = ec.oracle_outputs(name)
        exp = capi.eval_losses(ec.expected_sums(ec.records()[:, list(SEQ)], g[:, list(SEQ)], v[:, list(SEQ)]))
        for k in ("gain_loss", "vad_loss", "loss"):
            assert abs(r[k] - exp[k]) <= 1e-10 * abs(exp[k]), (name, k, r[k], exp[k])
        per = r["per_sequence"]
        assert per["loss"].shape == (3,) and np.array_equal(per["gain_loss"], sums[:, 0] / (32 * sums[:, 2]))
        assert np.array_equal(per["loss"], per["gain_loss"] + .001 * per["vad_loss"])
    assert res[0]["loss"] != res[1]["loss"]
    # slabs of two sequences: the same sums, so the same losses
    slabbed = evaluate.evaluate_records(str(path), [load_blob("default")], sequence_length=ec.T, max_streams=2)[0]
    assert {k: slabbed[k] for k in ("gain_loss", "vad_loss", "loss", "frames_scored")} == {k: res[0][k] for k in ("gain_loss", "vad_loss", "loss", "frames_scored")}
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "eval-records", str(path), "--model", blobs[0], "--model", blobs[1],
                          "--sequence-length", str(ec.T)], check=True, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    j = json.loads(lines[0])
    assert j["sequence_length"] == ec.T and j["gamma"] == 0.25 and j["first"] == 4 and len(j["models"]) == 2
    for m, r, blob in zip(j["models"], res, blobs):
        assert m["model"] == blob and m["sequences"] == 3
        for k in ("frames_scored", "gain_loss", "vad_loss", "loss"):
            assert m[k] == r[k], (k, m[k], r[k])


def test_cli_first_and_gamma(tmp_path, seqs):
    path = tmp_path / "val.f32"
    path.write_bytes(seqs.tobytes())
    blob = tmp_path / "default.blob"
    blob.write_bytes(load_blob("default"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "eval-records", str(path), "--model", str(blob), "--sequence-length",
                          str(ec.T), "--gamma", "0.5", "--first", "6"], check=True, env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300).stdout
    m = json.loads(out.strip().splitlines()[-1])["models"][0]
    want = evaluate.evaluate_records(seqs, [load_blob("default")], sequence_length=ec.T, gamma=0.5, first=6)[0]
    assert m["frames_scored"] == 3 * ec.frames_scored(0, ec.T, 6) == want["frames_scored"]
    assert (m["gain_loss"], m["vad_loss"], m["loss"]) == (want["gain_loss"], want["vad_loss"], want["loss"])
