"""The mixed block of tests/stream_mix.py, without a GPU: what its streams reach on the oracle (pitch range, silence that flips from
frame to frame and at call boundaries), how well a batch laid out as copies of it mixes the streams of one analysis workgroup and
one 64-stream wave, and that its CASES reach every kernel form rn_plan can choose (rnnoise_amd/csrc/dispatch.h).  The GPU tests
that run the block (test_gpu_at_size.py: test_stream_mix_at_every_form) are only as good as what is checked here."""
import os
import subprocess

import numpy as np
import pytest

import stream_mix as sm
from conftest import ROOT, load_blob


@pytest.fixture(scope="module")
def mix():
    """(block, labels, oracle run of the block) on the goldens' profile"""
    from conftest import use_rcp_profile
    use_rcp_profile("intel")
    pcm, labels = sm.block()
    return pcm, labels, sm.oracle_block(load_blob("default"), pcm, collect_state=False)


def test_the_block_is_deterministic_and_every_category_is_there(mix):
    pcm, labels, _ = mix
    again, labels2 = sm.block()
    assert again.tobytes() == pcm.tobytes() and labels2 == labels
    assert pcm.shape == (sm.T, sm.B, 480) and pcm.dtype == np.float32
    counts = {c: labels.count(c) for c in set(labels)}
    assert counts["fuzz1"] == counts["fuzz2"] == 160 and counts["all_zero"] == 1
    assert counts["edge"] == 4 and counts["extreme"] >= 8 and counts["threshold"] >= 10 and counts["zero_runs"] >= 10
    assert counts["synth"] >= 4 and counts["fuzz3"] >= 1
    assert sum(counts.values()) == sm.B and all(sm.B % k for k in range(2, int(sm.B ** 0.5) + 1))   # B is prime


def test_the_block_reaches_the_pitch_range_and_the_silence_threshold(mix):
    _, labels, want = mix
    sil = want["silence"].astype(bool)
    live_pitch = want["pitch"][~sil]
    assert live_pitch.min() <= 62 and live_pitch.max() >= 760, (live_pitch.min(), live_pitch.max())
    assert len(np.unique(live_pitch)) >= 550
    # streams that go silent and live again, frame by frame (more than the first frame's silence of a quiet stream)
    turns = np.diff(sil.astype(np.int8), axis=0) != 0                 # turns[t - 1, s]: frame t differs from frame t - 1
    flipping = np.flatnonzero(turns.sum(0) >= 2)
    assert len(flipping) >= 4, [labels[s] for s in flipping]
    at_boundary = turns[np.array(sm.call_starts()) - 1]               # the first frame of a call against the last of the one before
    assert at_boundary[:, flipping].any(), "no stream turns silent or live at a call boundary"
    assert {labels[s] for s in flipping} >= {"zero_runs", "threshold"}
    assert sil.all(0).any(), "no stream is silent in every frame"
    # white noise around the threshold: some of it silent throughout, some live throughout (but for the first frame), some between
    thr = [s for s in range(sm.B) if labels[s] == "threshold"]
    assert sil[:, thr].all(0).any() and (~sil[1:, thr]).all(0).any() and (turns[:, thr].sum(0) >= 2).any()


def test_a_batch_of_copies_mixes_every_analysis_quad_and_wave(mix):
    """the 40,037-stream case's layout: stream i takes block stream i mod B"""
    _, labels, want = mix
    n = max(c[0] for c in sm.CASES)
    idx = np.arange(n) % sm.B
    sil = want["silence"].astype(bool)[:, idx[:n // 4 * 4]].reshape(sm.T, -1, 4)
    pitch = np.ma.masked_array(want["pitch"][:, idx[:n // 4 * 4]].reshape(sm.T, -1, 4), sil)
    spread = (pitch.max(-1) - pitch.min(-1)).filled(0)                  # live members only
    assert (spread >= 300).any(0).mean() >= 0.9
    assert (sil.any(-1) & (~sil).any(-1)).any(0).mean() >= 0.1
    for w in range(0, n, 64):
        kinds = {labels[s] for s in idx[w:w + 64]}
        assert len(kinds) >= 5, (w, kinds)


def _forms():
    """every form the harness can name, per stage: its name tables (one name per enumerator of dispatch.h), less "unknown" """
    import re
    src = open(os.path.join(ROOT, "tests", "csrc", "dispatch_test.cpp")).read()
    tables = dict(re.findall(r"static const char \*const (k\w+)\[\] = \{([^}]*)\}", src))
    assert set(tables) == {"kHp", "kK1", "kNn", "kGru", "kK3"}
    return {k: set(re.findall(r'"(\w+)"', v)) - {"unknown"} for k, v in tables.items()}


def test_the_cases_reach_every_kernel_form(tmp_path):
    """every CASES entry through the library's own dispatch rules (tests/csrc/dispatch_test.cpp), 256 CUs, default switches, the
    default schedule (one-frame calls unpipelined, longer ones pipelined): every form of every stage runs at least once"""
    exe = str(tmp_path / "dispatch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "dispatch_test.cpp"), "-o", exe],
                   check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}

    def run(cases):
        return subprocess.run([exe] + cases, capture_output=True, text=True, check=True, env=env).stdout.split("\n")[:len(cases)]

    forms = _forms()
    seen = {k: set() for k in forms}
    for n, path, calls in sm.CASES:
        if path is None:
            path = int(run([f"path:{n}"])[0])
            assert path == 1, n
        assert run([f"sched:{c},0" for c in calls]) == ["1 1" if c > 1 else "0 0" for c in calls]
        for line in run([f"plan:{n},1,256,{path},{int(c > 1)},0,0" for c in calls]):
            hp, k1, k2, gru, k3 = line.split()
            seen["kHp"].add(hp), seen["kK1"].add(k1), seen["kNn"].add(k2), seen["kK3"].add(k3)
            if k2 == "layers":
                seen["kGru"].add(gru)
    for kind, names in forms.items():
        assert seen[kind] == names, (kind, names - seen[kind])
