"""The mixed block of tests/stream_mix.py, without a GPU: what its streams reach on the oracle (pitch range, silence that flips from
frame to frame and at call boundaries), how well a batch laid out as copies of it mixes the streams of one analysis workgroup and
one 64-stream wave, and that its CASES reach every kernel form rn_plan can choose (rnnoise_amd/csrc/dispatch.h) -- in lock-step calls,
and under the presence schedule (stream_mix.KINDS, presence(), LISTED, RESET) in per-stream frame phase and in stream-list calls;
that the schedule mixes frame phases within every wave and tile, keeps the block's coverage on present frames, and gives a kernel
that ignores the mask or reads an absent row something to fail on.  The GPU tests that run the block (test_gpu_at_size.py:
test_stream_mix_at_every_form, test_stream_mix_masked_and_listed_at_every_form) are only as good as what is checked here."""
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


# ---- the presence schedule (stream_mix.KINDS, presence(), LISTED, RESET): what test_stream_mix_masked_and_listed_at_every_form runs ----
@pytest.fixture(scope="module")
def masked_mix(mix):
    """the oracle's run of the block on every position's present frames, with RESET's restarts"""
    pcm, labels, lock = mix
    return pcm, labels, lock, sm.oracle_block(load_blob("default"), pcm, collect_state=False, presence=sm.presence(), resets=sm.RESET)


def _lock_frames():
    return [t for c, k in enumerate(sm.KINDS) if k == "lock" for t in sm.call_frames(c)]


def test_the_presence_schedule_keeps_its_rules():
    a = sm.presence() != 0
    assert sm.presence().dtype == np.uint8 and a.shape == (sm.T, sm.B) and (sm.presence() == a).all()
    assert 0.4 <= a.mean() <= 0.9, a.mean()
    assert len(sm.KINDS) == len(sm.CALLS) and sm.KINDS[0] != "lock"           # the first call switches to per-stream phase
    for kind in ("masked", "list", "lock"):                                   # every kind as a one-frame and as a pipelined call
        assert {sm.CALLS[c] > 1 for c, k in enumerate(sm.KINDS) if k == kind} == {False, True}, kind
    lock = _lock_frames()
    free = [t for t in range(sm.T) if t not in lock]
    assert a[lock].all()
    for c, kind in enumerate(sm.KINDS):
        fr = list(sm.call_frames(c))
        if kind == "list":
            assert 0.65 <= len(sm.LISTED[c]) / sm.B <= 0.75
            off = np.setdiff1d(np.arange(sm.B), sm.LISTED[c])
            assert not a[np.ix_(fr, off)].any() and a[np.ix_(fr, sm.LISTED[c])].any() and not a[np.ix_(fr, sm.LISTED[c])].all()
        if sm.CALLS[c] > 1 and kind != "lock":                                # absent at only the first / only the last frame
            assert (~a[fr[0]] & a[fr[1:]].all(0)).any() and (~a[fr[-1]] & a[fr[:-1]].all(0)).any(), c
    sp = sm.SPECIAL
    assert not a[free, sp["never"]].any() and a[free, sp["once"]].sum() == 1
    assert (a[free, sp["alternating"]] == (np.arange(len(free)) % 2 == 0)).all()
    assert 0.06 <= len(sm.RESET) / sm.B <= 0.1 and not set(sm.RESET) & set(sp.values())
    labels = sm.labels()[0]
    assert all(labels[p] not in ("all_zero", "zero_runs") for p in sp.values()) and max(sp.values()) < min(n for n, _, _ in sm.CASES)
    # silent runs with a gap at their edge: a zero_runs stream absent at the first zero frame of a run or the first live one after it
    runs = [p for p in range(sm.B) if labels[p] == "zero_runs"]
    edges = [(p, t) for p in runs for a0, b0 in sm._ZERO_RUNS[sm.labels()[1][p]] if b0 - a0 >= 2 for t in (a0, b0) if t < sm.T and not a[t, p]]
    assert len({p for p, _ in edges}) >= 5, edges


@pytest.mark.parametrize("n", sorted({n for n, _, _ in sm.CASES}))
def test_every_case_lists_every_copy_once_and_three_entries_that_name_no_stream(n):
    for c, kind in enumerate(sm.KINDS):
        if kind != "list":
            continue
        rows = sm.list_rows(n, c)
        assert rows.dtype == np.int32
        bad = (rows < 0) | (rows >= n)
        assert bad.sum() == 3 and bad[0] and bad[-1] and bad[len(rows) // 2 - 1:len(rows) // 2 + 2].any()
        assert sorted(rows[bad].tolist()) == [-1, n, 2 ** 31 - 1]
        good = rows[~bad]
        assert len(set(good.tolist())) == len(good) and set(good.tolist()) == {s for s in range(n) if s % sm.B in sm.LISTED[c]}
        assert (np.diff(good) < 0).any()                                      # not in stream order
        plan = sm.call_plan(n, c)
        assert not plan["present"][:, bad].any() and plan["active"][:, bad].all()   # marked present in the mask, absent by range


def test_every_call_start_mixes_the_frame_phases():
    """each stream's frame phase at the start of a call -- its present frames so far mod RN_RING_SLOTS (6), which a reset leaves alone
    -- takes every residue over the block (as many as the frames before allow), and at least three in every 64-stream wave and every
    16-stream tile of every case's layout, partial ones included"""
    a = sm.presence().astype(int)
    for t in sm.call_starts():
        r = a[:t].sum(0) % 6
        assert len(set(r.tolist())) == min(6, t + 1), t
        for n, _, _ in sm.CASES:
            idx = np.arange(n) % sm.B
            for w in (64, 16):
                worst = min(len(set(r[idx[s:s + w]].tolist())) for s in range(0, n, w))
                assert worst >= min(3, t + 1), (t, n, w, worst)


def test_the_masked_block_keeps_its_coverage(masked_mix):
    """on present frames only, the oracle still reaches the pitch range, and silence still flips -- also across an absent frame"""
    _, labels, _, want = masked_mix
    have = want["present"]
    assert have.shape == (sm.T, sm.B) and (have == (sm.presence() != 0)).all()
    assert (want["silence"][~have] == 2).all() and not want["vad"][~have].any() and not want["gains"][~have].any()
    assert not want["out"][~have].any()
    live = have & (want["silence"] == 0)
    assert want["pitch"][live].min() <= 62 and want["pitch"][live].max() >= 760, (want["pitch"][live].min(), want["pitch"][live].max())
    flips, across = set(), set()
    for s in range(sm.B):
        t = np.flatnonzero(have[:, s])
        sil = want["silence"][t, s]
        turn = np.flatnonzero(sil[1:] != sil[:-1])
        if len(turn):
            flips.add(s)
        if (np.diff(t)[turn] > 1).any():
            across.add(s)
    assert len(flips) >= 4 and {labels[s] for s in flips} >= {"zero_runs", "threshold"}, [labels[s] for s in flips]
    assert across, "no stream turns silent or live across an absent frame"


def test_the_masked_expectation_has_teeth(masked_mix):
    """a kernel that ignores the mask must fail: for at least half of the block positions the expected pcm of a present frame differs
    from the lock-step run of the same input; and every absent row of every call's input is NaN, every present row finite"""
    pcm, _, lock, want = masked_mix
    have = want["present"]
    differ = [(want["out"][have[:, p], p] != lock["out"][have[:, p], p]).any() for p in range(sm.B)]
    assert np.mean(differ) >= 0.5, np.mean(differ)
    for n in (251, 389, 1031, 3001):
        for c in range(len(sm.KINDS)):
            plan = sm.call_plan(n, c)
            x = sm.call_input(pcm, plan["frames"], plan["src"], plan["present"])
            assert x.shape == (len(plan["frames"]), len(plan["src"]), 480)
            fin = np.isfinite(x)
            assert fin[plan["present"]].all() and not fin[~plan["present"]].any(), (n, c)
            if plan["kind"] != "lock":
                assert (~plan["present"]).any() and plan["active"].flags.c_contiguous, (n, c)


def _build(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", f"{name}.cpp"), "-o", exe],
                   check=True)
    return exe


def test_the_cases_reach_every_per_stream_and_list_form(tmp_path):
    """The forms the rules can choose in per-stream frame phase (masked calls, lock-step calls after them) and in list calls -- found by
    sweeping rn_plan over batch sizes, network paths and pipelining on 256 CUs with the default switches -- are all reached by CASES
    under KINDS on the default schedule: one-frame calls unpipelined, longer ones pipelined, a list call with as many rows as
    list_rows() gives it (tests/csrc/dispatch_test.cpp, tests/csrc/list_dispatch_test.cpp)"""
    plan_exe, list_exe = _build(tmp_path, "dispatch_test"), _build(tmp_path, "list_dispatch_test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}

    def run(exe, cases):
        lines = []
        for i in range(0, len(cases), 4000):
            part = cases[i:i + 4000]
            lines += subprocess.run([exe] + part, capture_output=True, text=True, check=True, env=env).stdout.split("\n")[:len(part)]
        return [tuple(l.split()) for l in lines]

    def forms(lines):
        seen = {k: set() for k in ("hp", "k1", "nn", "gru", "k3")}
        for hp, k1, nn, gru, k3 in lines:
            seen["hp"].add(hp), seen["k1"].add(k1), seen["nn"].add(nn), seen["k3"].add(k3)
            if nn == "layers":
                seen["gru"].add(gru)
        return seen

    sizes = sorted(set(range(1, 4200)) | {int(x) + d for x in np.geomspace(4096, 1 << 17, 400) for d in (-1, 0, 1)})
    grid = [(n, path, pipe) for n in sizes for path in (0, 1, 2) for pipe in (0, 1)]
    can_stream = forms(run(plan_exe, [f"plan:{n},1,256,{path},{pipe},1,0" for n, path, pipe in grid]))
    can_list = forms(run(list_exe, [f"list:{n},{n},256,{pipe},0,{path}" for n, path, pipe in grid]))
    # what the rules allow today (a new form shows up in the sweep on its own; this only says the sweep sees the regimes)
    assert can_stream["hp"] == {"rn_hp_one_kernel", "rn_hp_kernel"} and can_stream["k1"] == {"rn_analysis_single_kernel"}
    assert can_stream["nn"] == {"rn_nn_one_kernel", "rn_nn_vector_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel", "layers"}
    assert can_stream["gru"] == {"rn_nn_gru_kernel", "rn_nn_gru_w8_kernel"}
    assert can_list["hp"] == {"rn_hp_one_kernel"} and can_list["nn"] == {"rn_nn_one_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel"}
    assert can_stream["k3"] == can_list["k3"] == {"rn_synthesis_few_kernel", "rn_synthesis_kernel"}

    stream_cases, list_cases = [], []
    for n, path, calls in sm.CASES:
        assert calls == sm.CALLS
        if path is None:
            path = int(run(plan_exe, [f"path:{n}"])[0][0])
        assert run(plan_exe, [f"sched:{c},0" for c in calls]) == [("1", "1") if c > 1 else ("0", "0") for c in calls]
        for c, kind in enumerate(sm.KINDS):
            pipe = int(calls[c] > 1)
            if kind == "list":
                list_cases.append(f"list:{n},{len(sm.list_rows(n, c))},256,{pipe},0,{path}")
            else:
                stream_cases.append(f"plan:{n},1,256,{path},{pipe},1,0")
    seen_stream, seen_list = forms(run(plan_exe, stream_cases)), forms(run(list_exe, list_cases))
    for kind in can_stream:
        assert seen_stream[kind] == can_stream[kind], ("per-stream", kind, can_stream[kind] - seen_stream[kind])
        assert seen_list[kind] == can_list[kind], ("list", kind, can_list[kind] - seen_list[kind])
