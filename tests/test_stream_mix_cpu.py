"""The mixed block of tests/stream_mix.py, without a GPU: what its streams reach on the oracle (pitch range, silence that flips from
frame to frame and at call boundaries), how well a batch laid out as copies of it mixes the streams of one analysis workgroup and
one 64-stream wave, and that its CASES reach every kernel form rn_plan can choose (rnnoise_amd/csrc/dispatch.h) -- in lock-step calls,
and under the presence schedule (stream_mix.KINDS, presence(), LISTED, RESET) in per-stream frame phase and in stream-list calls;
that the schedule mixes frame phases within every wave and tile, keeps the block's coverage on present frames, and gives a kernel
that ignores the mask or reads an absent row something to fail on.  The GPU tests that run the block (test_gpu_at_size.py:
test_stream_mix_at_every_form, test_stream_mix_masked_and_listed_at_every_form) are only as good as what is checked here.  The same
for the link dressing (stream_mix.LINK_CASES and what follows it) on the link oracle alone: that its cases reach every kernel form,
that the linked gain differs from a participant's own almost everywhere, that the schedule produces every situation that decides who
participates (no participant beside a present row, one, a silent or an absent row beside one, only the second half of a group of
eight -- each for every K), and that a kernel that skips the fold, folds an absent row or gates on a row's own VAD, or a reset that
forgets the gate counter, has something to fail on
(test_stream_mix_linked_at_every_form, test_stream_mix_linked_masked_and_listed_at_every_form).  And for the PCM dressing
(stream_mix.DRESS_CASES and what follows it) on the CPU chain alone: that rates and formats mix in every neighbourhood, that groups
of channels stay pure and lists whole, that every call's strides fit, that the cases reach the kernel forms they are for with the
one-wave K0 everywhere, that the expectation reaches every G.711 segment, the zero codes and the denormals, and that a chain whose
histories advance on an absent frame, whose reset keeps them or which encodes before the truncating cast changes expected rows
(test_stream_mix_dressed_at_every_form, test_stream_mix_dressed_masked_and_listed_at_every_form).  And for the chunk dressing
(stream_mix.CHUNK_CASES and what follows it): that the schedule of pushes keeps its rules at every frame length -- both forms in both
schedules, every special count on every position, frames completed and FIFO fills mixed in every neighbourhood, a reset that drops
something, a move at every fill class, a tail that ends on whole frames --, that the cases reach every form a masked and a list call
can take, that six wrong expectations each change the samples some push returns, and that the closed form is the FIFO model of
tests/test_chunks_gpu.py on the oracle's frames (test_stream_mix_chunked_at_every_form).  And for the feature dressing
(stream_mix.FEATURE_CASES and what follows it): that the cases reach every form a feature call can take, that the records keep the
block's all-zero feature rows -- the silent frames -- at every call boundary and beside live rows in nearly every tile, with targets
of every kind on neighbouring positions, that the compute_rnn-only expectation is the pinned `process` run on every position that is
never silent, and that a call which skips the network on zero rows, or scores a step against the wrong record, has something to
fail on (test_stream_mix_feature_calls_at_every_form and the tests behind it)."""
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


def _forms_of(lines):
    """the forms of every stage in the output lines of dispatch_test / list_dispatch_test (the GRU form only where the network is layer-wise)"""
    seen = {k: set() for k in ("hp", "k1", "nn", "gru", "k3")}
    for hp, k1, nn, gru, k3 in lines:
        seen["hp"].add(hp), seen["k1"].add(k1), seen["nn"].add(nn), seen["k3"].add(k3)
        if nn == "layers":
            seen["gru"].add(gru)
    return seen


def _sweep_sizes():
    """the batch sizes of form_sweep: every one up to 4,199, and 400 steps from 4,096 to 131,072 with both neighbours of each"""
    return sorted(set(range(1, 4200)) | {int(x) + d for x in np.geomspace(4096, 1 << 17, 400) for d in (-1, 0, 1)})


@pytest.fixture(scope="module")
def form_sweep(tmp_path_factory):
    """The forms the rules can choose in per-stream frame phase (masked calls, lock-step calls after them) and in list calls -- found by
    sweeping rn_plan over batch sizes, network paths and pipelining on 256 CUs with the default switches (tests/csrc/dispatch_test.cpp,
    tests/csrc/list_dispatch_test.cpp) -- as (run, plan_exe, list_exe, can_stream, can_list); run(exe, cases) gives the output lines"""
    tmp = tmp_path_factory.mktemp("form_sweep")
    plan_exe, list_exe = _build(tmp, "dispatch_test"), _build(tmp, "list_dispatch_test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}

    def run(exe, cases):
        lines = []
        for i in range(0, len(cases), 4000):
            part = cases[i:i + 4000]
            lines += subprocess.run([exe] + part, capture_output=True, text=True, check=True, env=env).stdout.split("\n")[:len(part)]
        return [tuple(l.split()) for l in lines]

    grid = [(n, path, pipe) for n in _sweep_sizes() for path in (0, 1, 2) for pipe in (0, 1)]
    can_stream = _forms_of(run(plan_exe, [f"plan:{n},1,256,{path},{pipe},1,0" for n, path, pipe in grid]))
    can_list = _forms_of(run(list_exe, [f"list:{n},{n},256,{pipe},0,{path}" for n, path, pipe in grid]))
    # what the rules allow today (a new form shows up in the sweep on its own; this only says the sweep sees the regimes)
    assert can_stream["hp"] == {"rn_hp_one_kernel", "rn_hp_kernel"} and can_stream["k1"] == {"rn_analysis_single_kernel"}
    assert can_stream["nn"] == {"rn_nn_one_kernel", "rn_nn_vector_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel", "layers"}
    assert can_stream["gru"] == {"rn_nn_gru_kernel", "rn_nn_gru_w8_kernel"}
    assert can_list["hp"] == {"rn_hp_one_kernel"} and can_list["nn"] == {"rn_nn_one_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel"}
    assert can_stream["k3"] == can_list["k3"] == {"rn_synthesis_few_kernel", "rn_synthesis_kernel"}
    return run, plan_exe, list_exe, can_stream, can_list


def test_the_cases_reach_every_per_stream_and_list_form(form_sweep):
    """The forms the rules can choose in per-stream frame phase and in list calls (form_sweep) are all reached by CASES under KINDS on
    the default schedule: one-frame calls unpipelined, longer ones pipelined, a list call with as many rows as list_rows() gives it"""
    run, plan_exe, list_exe, can_stream, can_list = form_sweep
    forms = _forms_of

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


# ---- the link dressing (stream_mix.LINK_CASES, controls(), slots(), link_presence(), oracle_groups): what
# test_stream_mix_linked_at_every_form and test_stream_mix_linked_masked_and_listed_at_every_form run ----
_LINKED = {}


def _linked(K, scheduled):
    """the link oracle's run of the groups that occur for K, lock-step or under the linked presence schedule with RESET's restarts"""
    from conftest import use_rcp_profile
    use_rcp_profile("intel")
    if (K, scheduled) not in _LINKED:
        pcm, _ = sm.block()
        kw = dict(presence=sm.link_presence(K), resets=sm.RESET) if scheduled else {}
        _LINKED[K, scheduled] = sm.oracle_groups([load_blob("default"), load_blob("little")], pcm, K, sm.controls(), sm.slots(),
                                                 groups=sm.link_groups(K), **kw)
    return _LINKED[K, scheduled]


def _link_counts(r, K):
    """group-frames of a run of oracle_groups, by situation"""
    ran = r["ran"]
    pres, sil, n = r["present"][:, ran], r["silence"][:, ran], r["n"][:, ran]
    part = pres & (sil == 0)
    assert (part.sum(-1) == n).all()
    own = r["gains"][:, ran].view(np.uint32)
    bites = ((own != r["g_link"][:, ran].view(np.uint32)[:, :, None]).any(-1) & part).any(-1)
    silent = pres & (sil == 1)
    return dict(live=int((n > 0).sum()), bites=int((bites & (n > 0)).sum()),
                present_no_participant=int((pres.any(-1) & (n == 0)).sum()),
                one_participant=int((n == 1).sum()),
                silent_beside_participant=int((silent.any(-1) & (n > 0)).sum()),
                absent_beside_participant=int(((~pres).any(-1) & (n > 0)).sum()),
                only_members_4_to_7=int((part[..., 4:].any(-1) & ~part[..., :4].any(-1)).sum()) if K == 8 else 0,
                only_the_third_member=int((part[..., 2] & ~part[..., :2].any(-1)).sum()) if K == 3 else 0)


def test_the_link_dressing_keeps_its_rules():
    for n, _, K in sm.LINK_CASES:
        assert n % K == 0 and n % sm.B != 0, (n, K)
        g0 = sm.link_g0(n, K)
        gm = sm.link_index(n, K)
        assert ((gm // K + gm % K) % sm.B == np.arange(n) % sm.B).all() and (gm // K == np.repeat(g0, K)).all()
        streams, at = sm.link_state_streams(n, K)
        assert len(set(streams.tolist())) == len(streams) == K * len(set(g0.tolist())) and (gm[streams] == at).all()
        copies = n // K // len(set(g0.tolist()))
        assert copies == 1 or len(set((streams // K // len(set(g0.tolist()))).tolist())) >= min(copies, 5)   # from different copies
    assert any((np.diff(sm.link_g0(n, K)) < 0).any() for n, _, K in sm.LINK_CASES), "no case has a group that wraps from 388 to 0"
    ctl, slot = sm.controls(), sm.slots()
    assert ctl.shape == (sm.B, 3) and ctl.dtype == np.float32 and slot.shape == (sm.B,) and slot.dtype == np.uint8
    none = (ctl == 0).all(1)
    assert 0.4 <= none.mean() <= 0.6, none.mean()
    assert (ctl[:, 0] >= 0).all() and (ctl[:, 0] <= 1).all() and (ctl[:, 1] >= 0).all() and (ctl[:, 1] <= 1).all()
    assert (ctl[:, 2] == np.floor(ctl[:, 2])).all() and (ctl[:, 2] >= 0).all() and (ctl[:, 2] <= 65535).all()
    assert len({tuple(x) for x in ctl[~none]}) >= 20 and (ctl[~none, 0] > 0).any() and (ctl[~none, 2] > 0).any()
    gated = ctl[:, 1] > 0
    shared = gated[:-1] & gated[1:] & (ctl[:-1, 1:] == ctl[1:, 1:]).all(1)
    assert shared.sum() >= 10 and (gated[:-1] & gated[1:] & ~shared).sum() >= 10, shared.sum()
    assert 0.25 <= slot.mean() <= 0.4 and set(slot.tolist()) == {0, 1}
    assert not any(all(slot[(p + k) % sm.B] for k in range(8)) for p in range(sm.B)), "slot 1 on a whole run of 8"
    for K in sm.LINK_KS:
        both = [g for g in sm.link_groups(K) if len({int(slot[(g + k) % sm.B]) for k in range(K)}) == 2]
        assert len(both) >= 20, (K, len(both))


def test_the_linked_presence_schedule_keeps_its_rules():
    base = sm.presence() != 0
    lists = [c for c, k in enumerate(sm.KINDS) if k == "list"]
    free = [t for c, k in enumerate(sm.KINDS) if k != "list" for t in sm.call_frames(c)]
    for K in sm.LINK_KS:
        a = sm.link_presence(K)
        assert a.shape == (sm.T, sm.B, K) and a.dtype == bool
        lone, solo = sm.link_lone(K), sm.link_solo(K)
        made = [x for x in (lone, solo) if x]
        plain = ~np.isin(np.arange(sm.B), [g for g, _ in made])
        for k in range(K):                                                    # outside list calls: presence()'s mask of the position
            assert (a[free][:, plain, k] == base[free][:, (np.arange(sm.B) + k) % sm.B][:, plain]).all()
        assert (lone is None) == (K == 2)
        # the hand-made groups: one row on its own from the second frame of a masked call on -- the all-zero row, and a voice
        fr = list(sm.call_frames(sm.LONE_CALL))[1:]
        rest = [t for t in free if t not in fr]
        assert sm.KINDS[sm.LONE_CALL] == "masked" and len(fr) >= 10
        for g, m in made:
            assert a[fr, g, m].all() and a[fr, g].sum() == len(fr) and g in sm.link_groups(K, common=True) and (K < 8 or m >= 4)
            assert (a[rest, g] == np.stack([base[rest][:, (g + k) % sm.B] for k in range(K)], -1)).all()
        if lone:
            assert sm.labels()[0][(lone[0] + lone[1]) % sm.B] == "all_zero"
        assert all(sm.labels()[0][(solo[0] + k) % sm.B].startswith("fuzz") for k in range(K)) and solo[1] % 4 != 0
        assert lone is None or not {(lone[0] + k) % sm.B for k in range(K)} & {(solo[0] + k) % sm.B for k in range(K)}
        for c in lists:
            fr = list(sm.call_frames(c))
            on = sm.link_listed(K, c)
            assert 0.65 <= len(on) / sm.B <= 0.8, (K, c, len(on))
            off = np.setdiff1d(np.arange(sm.B), on)
            assert not a[np.ix_(fr, off)].any() and a[np.ix_(fr, on)].any()
            rep = sm.link_replaced(K, c)
            assert [m for _, m, _ in rep] == {2: [0, 1, 1], 3: [0, 1, 2], 8: [0, 4, 7]}[K] and [e for _, _, e in rep] == list(sm.OUT_OF_RANGE)
            assert len({g for g, _, _ in rep}) == 3 and {g for g, _, _ in rep} <= set(on) & set(sm.link_groups(K, common=True))
            for g, m, _ in rep:
                assert not a[fr, g, m].any() and a[fr, g].any(-1).all()         # absent for the call, beside siblings that are there
        sp = sm.SPECIAL                                                       # the hand-made rows keep their frames in every group
        for name in ("once", "alternating", "first1", "last1", "first6", "last6"):
            for m in range(K):
                assert (a[:, (sp[name] - m) % sm.B, m] == base[:, sp[name]]).all(), (K, name, m)
        for m in range(K):
            assert not a[[t for t in range(sm.T) if t not in _lock_frames()], (sp["never"] - m) % sm.B, m].any()


@pytest.mark.parametrize("n,path,K", sm.LINK_CASES, ids=[f"n{n}-path{p}-k{K}" for n, p, K in sm.LINK_CASES])
def test_every_linked_case_lists_whole_groups_and_three_entries_that_name_no_stream(n, path, K):
    g0_of = sm.link_g0(n, K)
    for c, kind in enumerate(sm.KINDS):
        if kind != "list":
            continue
        rows, g0, mem = sm.link_list_rows(n, K, c)
        assert rows.dtype == np.int32 and len(rows) % K == 0 and len(rows) <= n
        bad = (rows < 0) | (rows >= n)
        assert bad.sum() == 3 and sorted(rows[bad].tolist()) == [-1, n, 2 ** 31 - 1]
        assert (mem == np.tile(np.arange(K), len(rows) // K)).all() and (g0.reshape(-1, K) == g0[::K, None]).all()
        assert {(int(g0[i]), int(mem[i]), int(rows[i])) for i in np.flatnonzero(bad)} == {
            (g, m, n if e is None else e) for g, m, e in sm.link_replaced(K, c)}
        # whole groups, members ascending; every copy of every chosen group once (the replaced entries stand for their streams)
        first = np.where(bad, -1, rows).reshape(-1, K).max(1) // K * K
        whole = first[:, None] + np.arange(K)
        assert ((rows.reshape(-1, K) == whole) | bad.reshape(-1, K)).all()
        groups = first // K
        assert len(set(groups.tolist())) == len(groups) and (g0_of[groups] == g0[::K]).all()
        assert set(groups.tolist()) == {j for j in range(n // K) if g0_of[j] in sm.link_listed(K, c)}
        assert (np.diff(groups) < 0).any()                                    # not in stream order
        plan = sm.link_call_plan(n, K, c)
        assert not plan["present"][:, bad].any() and plan["active"][:, bad].all()
        assert ((plan["src"] == (g0 + mem) % sm.B)).all() and (plan["gm"] == g0 * K + mem).all()
        # the replaced stream's other copies are listed, and masked out for the call
        for g, m, _ in sm.link_replaced(K, c):
            same = (g0 == g) & (mem == m)
            assert same.sum() == (g0_of == g).sum() and not plan["present"][:, same].any() and not plan["active"][:, same & ~bad].any()


def test_the_linked_cases_reach_every_kernel_form(tmp_path):
    """every LINK_CASES entry through the library's dispatch rules on 256 CUs with the default switches: the forms its comment names,
    and together every form that CASES reaches in lock-step calls, in per-stream frame phase and in list calls"""
    plan_exe, list_exe = _build(tmp_path, "dispatch_test"), _build(tmp_path, "list_dispatch_test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}

    def run(exe, cases):
        return [tuple(l.split()) for l in subprocess.run([exe] + cases, capture_output=True, text=True, check=True,
                                                         env=env).stdout.split("\n")[:len(cases)]]

    def reach(cases, link):
        lock, stream, lists = [], [], []
        for n, path, third in cases:
            if path is None:
                path = int(run(plan_exe, [f"path:{n}"])[0][0])
            for c, kind in enumerate(sm.KINDS):
                pipe = int(sm.CALLS[c] > 1)
                lock.append((n, path, link and third, pipe, run(plan_exe, [f"plan:{n},1,256,{path},{pipe},0,0"])[0]))
                if kind == "list":
                    rows = len(sm.link_list_rows(n, third, c)[0]) if link else len(sm.list_rows(n, c))
                    lists.append((n, path, link and third, pipe, run(list_exe, [f"list:{n},{rows},256,{pipe},0,{path}"])[0]))
                else:
                    stream.append((n, path, link and third, pipe, run(plan_exe, [f"plan:{n},1,256,{path},{pipe},1,0"])[0]))
        return lock, stream, lists

    def forms(lines):
        seen = {k: set() for k in ("hp", "k1", "nn", "gru", "k3")}
        for *_, (hp, k1, nn, gru, k3) in lines:
            seen["hp"].add(hp), seen["k1"].add(k1), seen["nn"].add(nn), seen["k3"].add(k3)
            if nn == "layers":
                seen["gru"].add(gru)
        return seen

    got, want = reach(sm.LINK_CASES, True), reach(sm.CASES, False)
    for what, g, w in zip(("lock-step", "per-stream", "list"), got, want):
        assert forms(g) == forms(w), (what, forms(g), forms(w))
    lock, stream, _ = got

    def at(lines, n, path, K, pipe=None):
        return [f for n_, p_, k_, pipe_, f in lines if (n_, p_, k_) == (n, path, K) and pipe in (None, pipe_)]

    for f in at(lock, 252, 0, 2):
        assert (f[0], f[2], f[4]) == ("rn_hp_one_kernel", "rn_nn_one_kernel", "rn_synthesis_few_kernel"), f
    for f in at(lock, 390, 0, 3):
        assert (f[2], f[4]) == ("rn_nn_one_kernel", "rn_synthesis_kernel"), f
    assert {f[2] for f in at(lock, 390, 1, 2, 0)} == {"rn_nn_mfma16_kernel"} and {f[2] for f in at(lock, 390, 1, 2, 1)} == {"rn_nn_mfma_kernel"}
    assert {f[2:4] for f in at(lock, 390, 2, 3)} == {("layers", "rn_nn_gru_w8_kernel")}
    assert {f[2] for f in at(lock, 1032, 0, 8)} == {"rn_nn_vector_kernel"}
    for lines, k1 in ((lock, "rn_analysis_kernel"), (stream, "rn_analysis_single_kernel")):
        assert {(f[0], f[1]) for f in at(lines, 2568, 1, 8)} == {("rn_hp_kernel", k1)}
        assert {f[2] for f in at(lines, 2568, 1, 8)} == {"rn_nn_mfma16_kernel", "rn_nn_mfma_kernel"}
        assert {f[2:4] for f in at(lines, 16416, 1, 2)} == {("layers", "rn_nn_gru_kernel")}
    assert (16416 + 63) // 64 == 257 and 16416 % 64 == 32


def test_the_link_bites_in_lock_step():
    """per K over the groups that occur: the linked gain differs from some participant's own in at least 90 % of the live
    group-frames of the lock-step run"""
    msg = {}
    for K in sm.LINK_KS:
        c = _link_counts(_linked(K, False), K)
        msg[K] = c
        assert c["bites"] >= 0.9 * c["live"], msg
    print("lock-step", msg)


def test_the_linked_schedule_covers_who_participates():
    """the schedule runs: the share of live group-frames in which the link bites (K = 2: at least 40 %, K = 8: at least 90 %), and
    for every K at least 10 group-frames of every situation that decides who participates"""
    counts = {K: _link_counts(_linked(K, True), K) for K in sm.LINK_KS}
    assert counts[2]["bites"] >= 0.4 * counts[2]["live"], counts
    assert counts[8]["bites"] >= 0.9 * counts[8]["live"], counts
    for what in ("present_no_participant", "one_participant", "silent_beside_participant", "absent_beside_participant"):
        for K in sm.LINK_KS:
            assert counts[K][what] >= 10, (K, what, counts)
    assert counts[8]["only_members_4_to_7"] >= 10 and counts[3]["only_the_third_member"] >= 10, counts
    print("schedule", counts)


def _gate_walk(r, ctl_of, resets_of):
    """every row's gate counter frame by frame under a VAD (T, B, K) -- include/rnnoise_amd.h's rule, restarted at RESET's restart --
    as (closed (T, B, K), the counter after the last frame)"""
    def walk(vad):
        thr, hold = ctl_of[..., 1], ctl_of[..., 2]
        c = np.full(thr.shape, 65536, np.int64)
        closed = np.zeros(vad.shape, bool)
        for t in range(vad.shape[0]):
            if t == sm.call_frames(sm.RESET_BEFORE)[0]:
                c[resets_of] = 65536
            voice = (thr == 0) | (vad[t] >= thr)
            c = np.where(r["present"][t], np.where(voice, 0, np.minimum(c + 1, 65536)), c)
            closed[t] = r["present"][t] & (thr > 0) & (c > hold)
        return closed, c
    return walk


def test_the_linked_expectation_has_teeth(mix):
    """a kernel that skips the fold, folds the wrong rows or gates on a row's own VAD must fail"""
    pcm, _, lock = mix
    ctl, msg = sm.controls(), {}
    for K in sm.LINK_KS:
        r = _linked(K, False)
        ran = np.flatnonzero(r["ran"])
        pos = (ran[:, None] + np.arange(K)) % sm.B
        live = r["silence"][:, ran] == 0
        differ = (r["out"][:, ran].view(np.uint32) != lock["out"][:, pos].view(np.uint32)).any(-1)
        msg[K] = dict(out_differs=int((differ & live).sum()), live=int(live.sum()))
        assert (differ & live).sum() >= 0.9 * live.sum(), msg
        # the gate under vad_link against the gate each row's own VAD would give, over both runs
        ctl_of = ctl[(np.arange(sm.B)[:, None] + np.arange(K)) % sm.B]
        for scheduled in (False, True):
            r = _linked(K, scheduled)
            resets_of = np.isin((np.arange(sm.B)[:, None] + np.arange(K)) % sm.B, sm.RESET) & scheduled
            walk = _gate_walk(r, ctl_of, resets_of)
            linked, c_end = walk(np.broadcast_to(r["vad_link"][:, :, None], r["vad"].shape))
            alone, _ = walk(r["vad"])
            assert (c_end[r["ran"]] == r["gate"][r["ran"]]).all(), (K, scheduled)   # (the walk is the oracle's counter)
            apart = (linked != alone) & r["ran"][None, :, None]
            voice = ((r["vad_link"][:, :, None] >= ctl_of[..., 1]) != (r["vad"] >= ctl_of[..., 1])) & (ctl_of[..., 1] > 0) & r["present"]
            voice &= r["ran"][None, :, None]
            msg[K][f"gate_apart_{'schedule' if scheduled else 'lock'}"] = int(apart.sum())
            msg[K][f"voice_apart_{'schedule' if scheduled else 'lock'}"] = int(voice.sum())
            msg[K][f"silent_gate_apart_{'schedule' if scheduled else 'lock'}"] = int((apart & (r["silence"] == 1)).sum())
            assert apart.sum() >= 20 and voice.sum() >= 20 and (apart & (r["silence"] == 1)).any(), msg
        # an absent sibling: the present rows' expectation differs from the one with that sibling present
        r, a = _linked(K, True), sm.link_presence(K)
        t0 = [t for c, k in enumerate(sm.KINDS) if k == "masked" for t in sm.call_frames(c) if t > 0]
        found = tried = 0
        for g in np.flatnonzero(r["ran"]):
            t = next((t for t in t0 if (~a[t, g]).any() and r["n"][t, g] > 0), None)
            if t is None:
                continue
            a2 = a.copy()
            a2[t, g] = True
            r2 = sm.oracle_groups([load_blob("default"), load_blob("little")], pcm, K, ctl, sm.slots(), presence=a2, resets=sm.RESET,
                                  groups=[g])
            k = int(np.flatnonzero(a[t, g] & (r["silence"][t, g] == 0))[0])
            tried += 1
            found += int((r2["out"][t, g, k].view(np.uint32) != r["out"][t, g, k].view(np.uint32)).any())
            if tried == 6:
                break
        msg[K]["absent_sibling_changes_out"] = found
        assert found >= 1, msg
    print("teeth", msg)


# ---- the PCM dressing (stream_mix.DRESS_CASES, rate_codes(), formats(), dress_call_plan(), dress_expectation): what
# test_stream_mix_dressed_at_every_form and test_stream_mix_dressed_masked_and_listed_at_every_form run ----
_DRESSED = {}


def _dressed(variant, scheduled, mutant=None):
    """the CPU chain's run of the block under `variant`, lock-step or under the presence schedule, on the goldens' profile"""
    from conftest import use_rcp_profile
    use_rcp_profile("intel")
    if (variant, scheduled, mutant) not in _DRESSED:
        _DRESSED[variant, scheduled, mutant] = sm.dress_expectation(load_blob("default"), variant, scheduled, mutant)
    return _DRESSED[variant, scheduled, mutant]


def _valid(r):
    """(T, B, 480) bool: the entries of the expectation's `out` that a present row owns"""
    return r["present"][..., None] & (np.arange(480) < sm.frame_lengths()[:, None])[None]


def test_the_pcm_dressing_keeps_its_rules(tmp_path):
    from rnnoise_amd import g711, resample
    codes, fmt, law = sm.rate_codes(), sm.formats(), sm.laws()
    assert codes.shape == fmt.shape == law.shape == (sm.B,) and set(codes.tolist()) == {1, resample.RATE_32K, 2, 3, 6}
    assert set(fmt.tolist()) == {g711.LINEAR, g711.ULAW, g711.ALAW} and set(law.tolist()) == {g711.ULAW, g711.ALAW}
    assert (law[fmt != 0] == fmt[fmt != 0]).all() and len(set(law[fmt == 0].tolist())) == 2
    pair = [(int(c), int(f)) for c, f in zip(codes, fmt)]
    for p in range(sm.B):                                                     # cyclic: the copies of a batch wrap from 388 to 0
        near = [pair[(p + d) % sm.B] for d in range(64)]
        assert len({c for c, _ in near[:16]}) == 5 and len({f for _, f in near[:16]}) == 3, p
        assert len(set(near)) == 15, p
    lab, nth = sm.labels()
    for cat in ("zero_runs", "threshold", "extreme"):
        assert {int(codes[p]) for p in range(sm.B) if lab[p] == cat} == set(sm.RATE_CODES), cat
    exe = _build(tmp_path, "channels_dispatch_test")
    fit, side_by_side = [], 0
    for n, path, typ, C, lay in sm.DRESS_CASES:
        s16 = typ == "int16"
        assert n % C == 0 and n % sm.B != 0 and typ in ("int16", "float") and 1 <= C <= 8, (n, C)
        pos = np.arange(n) % sm.B
        comp, table = sm.dress_companded(n, C, s16), sm.dress_formats(n, C, s16)
        groups = comp.reshape(-1, C)
        assert (groups == groups[:, :1]).all(), "a group with linear and companded rows"
        if s16:
            assert (table == np.where(comp, law[pos], 0)).all() and (groups[:, 0] == (fmt[pos[::C]] != 0)).all()
            assert {int(x) for x in table} == {0, 1, 2}
            if C > 1:
                side_by_side += int((groups[:-1, 0] != groups[1:, 0]).sum())
                both = (table.reshape(-1, C) == g711.ULAW).any(1) & (table.reshape(-1, C) == g711.ALAW).any(1)
                assert both.sum() >= 10, "no group holds both laws"
                # one position as a linear row in one copy and as a companded one in another
                assert n < 2 * sm.B or any(len(set(comp[p::sm.B].tolist())) == 2 for p in range(sm.B))
        else:
            assert not comp.any() and (table == fmt[pos]).all() and table.any()     # a table that the float calls must ignore
        for scheduled in (False, True):
            for c in range(len(sm.CALLS)):
                plan = sm.dress_call_plan(n, C, c, scheduled)
                k, R = len(plan["frames"]), len(plan["src"])
                assert R % C == 0 and plan["present"].shape == (k, R) and len(plan["stream"]) == R
                assert (plan["stream"] % sm.B == plan["src"]).all()
                st = sm.dress_strides(lay, C, k, R)
                if st is not None:
                    assert st[0] % 4 == 0 and st[1] % 4 == 0 and min(st) > 0
                    fit.append(f"fit:{st[0]},{st[1]},480,{C},{R},{k}")
                if scheduled and plan["kind"] == "list" and s16:              # a list's groups are groups of the batch: still pure
                    rows_comp = comp[plan["stream"]].reshape(-1, C)
                    assert (rows_comp == rows_comp[:, :1]).all()
    assert side_by_side >= 100
    got = subprocess.run([exe] + fit, capture_output=True, text=True, check=True).stdout.split()
    laid = sum(lay != "default" for *_, lay in sm.DRESS_CASES)
    assert laid >= 3 and len(fit) == laid * 2 * len(sm.CALLS) and got == ["1"] * len(fit)


@pytest.mark.parametrize("n,path,typ,C,lay", sm.DRESS_CASES, ids=sm.DRESS_IDS)
def test_every_dressed_case_lists_whole_groups(n, path, typ, C, lay):
    pres = sm.presence() != 0
    for c, kind in enumerate(sm.KINDS):
        plan = sm.dress_call_plan(n, C, c)
        fr = plan["frames"]
        if kind != "list":
            assert (plan["stream"] == np.arange(n)).all() and (plan["present"] == pres[fr.start:fr.stop][:, np.arange(n) % sm.B]).all()
            continue
        rows, streams = sm.dress_list_rows(n, C, c)
        assert rows.dtype == np.int32 and len(rows) % C == 0 and len(rows) <= n + 3 and (plan["rows"] == rows).all()
        bad = (rows < 0) | (rows >= n)
        assert bad.sum() == 3 and sorted(rows[bad].tolist()) == [-1, n, 2 ** 31 - 1]
        assert (rows[~bad] == streams[~bad]).all() and len(set(streams[~bad].tolist())) == (~bad).sum()
        listed = np.isin(np.arange(n) % sm.B, sm.LISTED[c])
        # every copy of every listed position is in the list, so that a position's frames do not depend on the copy
        assert set(np.flatnonzero(listed).tolist()) <= set(rows[~bad].tolist())
        assert (plan["present"] == (pres[fr.start:fr.stop][:, streams % sm.B] & ~bad)).all()
        assert not plan["present"][:, bad].any() and plan["active"][:, bad].all() and (plan["active"][:, ~bad] == plan["present"][:, ~bad]).all()
        assert (np.diff(streams[::C]) < 0).any()                              # not in stream order
        if C > 1:
            assert (streams.reshape(-1, C) == streams[::C, None] + np.arange(C)).all() and (streams[::C] % C == 0).all()
            assert set((streams[::C] // C).tolist()) == set(np.flatnonzero(listed.reshape(-1, C).any(1)).tolist())
            assert not listed[streams[bad]].any()                             # the replaced entries: rows that miss the call in every copy
            assert sorted((np.flatnonzero(bad) % C).tolist()) == sorted([0, C // 2, C - 1])
            assert plan["present"].reshape(len(fr), -1, C)[:, bad.reshape(-1, C).any(1)].any(), "no replaced entry beside a present sibling"
            masked = ~bad & ~listed[streams]
            assert masked.sum() >= 10 and not plan["active"][:, masked].any()  # listed with their group, masked out


def test_the_dressed_cases_reach_every_kernel_form(tmp_path):
    """every DRESS_CASES entry through the library's dispatch rules on 256 CUs with the default switches, shaped as a call of a batch
    with a rate table (and, in the int16 calls, a format table): K0 is the one-wave form in every call, the other stages take the
    forms the comments of DRESS_CASES name, and together every form that CASES reaches"""
    exe = _build(tmp_path, "formats_dispatch_test")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}

    def run(cases):
        out = subprocess.run([exe] + cases, capture_output=True, text=True, check=True, env=env).stdout.split("\n")[:len(cases)]
        return [tuple(l.split()) for l in out]

    plan_exe = _build(tmp_path, "dispatch_test")
    lock, stream, lists = {}, {}, {}
    for case in sm.DRESS_CASES:
        n, path, typ, C, _ = case
        comp = int(typ == "int16")
        if path is None:
            path = int(subprocess.run([plan_exe, f"path:{n}"], capture_output=True, text=True, check=True, env=env).stdout)
            assert path == 1
        for c, kind in enumerate(sm.KINDS):
            pipe = int(sm.CALLS[c] > 1)
            lock.setdefault(case, []).append((pipe,) + run([f"fmt:{n},1,256,{path},{pipe},0,1,0,{comp}"])[0])
            if kind == "list":
                R = len(sm.dress_list_rows(n, C, c)[0])
                lists.setdefault(case, []).append((pipe,) + run([f"fmt:{R},0,256,{path},{pipe},1,1,1,{comp}"])[0])
            else:
                stream.setdefault(case, []).append((pipe,) + run([f"fmt:{n},1,256,{path},{pipe},1,1,0,{comp}"])[0])
    every = [f for d in (lock, stream, lists) for v in d.values() for f in v]
    assert {f[1] for f in every} == {"rn_hp_one_kernel"}
    by_n = {(c[0], c[1]): c for c in sm.DRESS_CASES}
    for f in lock[by_n[252, 0]]:
        assert (f[2], f[3], f[5]) == ("rn_analysis_single_kernel", "rn_nn_one_kernel", "rn_synthesis_few_kernel"), f
    assert {(f[3], f[5]) for f in lock[by_n[390, 0]]} == {("rn_nn_one_kernel", "rn_synthesis_kernel")}
    assert {(f[0], f[3]) for f in lock[by_n[390, 1]]} == {(0, "rn_nn_mfma16_kernel"), (1, "rn_nn_mfma_kernel")}
    assert {f[3:5] for f in lock[by_n[390, 2]]} == {("layers", "rn_nn_gru_w8_kernel")}
    assert {f[3] for f in lock[by_n[1032, 0]]} == {"rn_nn_vector_kernel"}
    assert {f[2] for f in lock[by_n[2568, None]]} == {"rn_analysis_kernel"}
    assert {f[2] for f in stream[by_n[2568, None]]} == {"rn_analysis_single_kernel"}
    assert run(["fmt:2568,1,256,1,0,0,0,0,0"])[0][0] == "rn_hp_kernel"       # what the plain batch runs there
    for d in (lock, stream):
        assert {f[3:5] for f in d[by_n[10278, None]]} == {("layers", "rn_nn_gru_w8_kernel")}
        assert {f[3:5] for f in d[by_n[16416, None]]} == {("layers", "rn_nn_gru_kernel")}
    assert (16416 + 63) // 64 == 257
    forms = _forms()
    seen = {"kK1": {f[2] for f in every}, "kNn": {f[3] for f in every}, "kGru": {f[4] for f in every if f[3] == "layers"},
            "kK3": {f[5] for f in every}}
    for kind, names in seen.items():
        assert names == forms[kind], (kind, forms[kind] - names)


def test_the_dressed_expectation_has_teeth():
    """on the CPU chain alone: both laws reach every segment with both signs in the expected output, zero frames come out as the laws'
    zero codes, the denormal stream is still denormal at its low rate, the float and the int16 chain differ, and the schedule shows"""
    from rnnoise_amd import g711
    lab, nth = sm.labels()
    law, codes, M = sm.laws(), sm.rate_codes(), sm.frame_lengths()
    msg = {}
    for scheduled in (False, True):
        r = _dressed("law", scheduled)
        ok = _valid(r)
        assert r["out"].dtype == np.uint8 and not r["out"][~ok].any()
        for name, code, zero in (("ulaw", g711.ULAW, 0xFF), ("alaw", g711.ALAW, 0xD5)):
            at = ok & (law == code)[None, :, None]
            seg, neg = g711.segment(r["out"][at], code)
            msg[name, scheduled] = len(set(zip(seg.tolist(), neg.tolist())))
            assert msg[name, scheduled] == 16, msg
            # frames whose output is exact zero: all of the row's bytes are the law's code of zero
            quiet = [(t, p) for p in np.flatnonzero(law == code) for t in range(sm.T)
                     if r["present"][t, p] and lab[p] in ("all_zero", "zero_runs") and (r["out"][t, p, :M[p]] == zero).all()]
            msg[name + "_zero_frames", scheduled] = len(quiet)
            assert len(quiet) >= 3, msg
    zero = sm.labels()[0].index("all_zero")
    assert (sm.dress_input("law")[:, zero, :M[zero]] == (0xFF if law[zero] == g711.ULAW else 0xD5)).all()
    assert (_dressed("law", False)["out"][:, zero, :M[zero]] == (0xFF if law[zero] == g711.ULAW else 0xD5)).all()
    # the denormal stream (extreme_signals' fifth, sigma 1e-38): a low rate; its low-rate input is nonzero nearly everywhere, below the
    # smallest normal in most samples (a sample beyond one sigma is a normal number) and nowhere above a few sigma; so is what comes out
    den = next(p for p in range(sm.B) if lab[p] == "extreme" and nth[p] == 4)
    tiny = np.finfo(np.float32).tiny
    for what, x in (("in", sm.dress_input("float")[:, den, :M[den]]), ("out", _dressed("float", False)["out"][:, den, :M[den]])):
        msg["denormal " + what] = (int(codes[den]), float((x != 0).mean()), float((np.abs(x) < tiny).mean()), float(np.abs(x).max()))
        assert codes[den] != 1 and (x != 0).mean() >= 0.9 and ((x != 0) & (np.abs(x) < tiny)).mean() >= 0.5 and np.abs(x).max() < 1e-37, msg
    # +-3e6: the float rows keep it, the int16 rows clip it
    loud = next(p for p in range(sm.B) if lab[p] == "extreme" and nth[p] == 1)
    assert np.abs(sm.dress_input("float")[:, loud]).max() > 1e6 and np.abs(sm.dress_input("s16")[:, loud].astype(int)).max() >= 32767
    # the three variants are three runs: vad differs between them for most positions
    f, s, c = (_dressed(v, True) for v in sm.VARIANTS)
    assert ((f["vad"] != s["vad"]).any(0)).mean() >= 0.5 and ((s["vad"] != c["vad"]).any(0)).mean() >= 0.5
    # a kernel that ignores the mask: the expectation under the schedule differs from the lock-step one on present frames
    for v in sm.VARIANTS:
        a, b = _dressed(v, True), _dressed(v, False)
        differ = [(a["out"][a["present"][:, p], p] != b["out"][a["present"][:, p], p]).any() for p in range(sm.B)]
        assert np.mean(differ) >= 0.5, (v, np.mean(differ))
    print("dressed teeth", msg)


@pytest.mark.parametrize("mutant", sm.DRESS_MUTANTS)
def test_the_dressed_expectation_catches_a_wrong_chain(mutant):
    """a chain whose resampler history advances on an absent frame, one whose reset keeps the history, one that encodes before the
    truncating cast: each changes expected rows"""
    variant = "law" if mutant == "encode_before_cast" else "s16"
    good, bad = _dressed(variant, True), _dressed(variant, True, mutant)
    rows = (good["out"] != bad["out"]).any(-1)                                # (T, B)
    codes = sm.rate_codes()
    assert not rows[~good["present"]].any()
    if mutant == "encode_before_cast":
        assert rows.any(0).sum() >= 100, rows.any(0).sum()
        for k in ("vad", "gains", "state"):
            assert (good[k].view(np.uint32) == bad[k].view(np.uint32)).all(), k
        return
    assert not rows[:, codes == 1].any()                                      # (no resampler, no history)
    low = np.flatnonzero(codes != 1)
    if mutant == "reset_keeps_history":
        cut = sm.call_frames(sm.RESET_BEFORE)[0]
        hit = [p for p in sm.RESET if codes[p] != 1]
        assert not rows[:cut].any() and not rows[:, [p for p in low if p not in sm.RESET]].any()
        assert len(hit) >= 10 and rows[cut:, hit].any(0).sum() >= len(hit) - 3, (len(hit), rows[cut:, hit].any(0).sum())
        assert {int(codes[p]) for p in hit if rows[:, p].any()} == set(sm.RATE_CODES) - {1}
    else:
        gaps = ~good["present"][:, low].all(0)
        assert rows[:, low][:, gaps].any(0).mean() >= 0.9
        assert {int(codes[p]) for p in low if rows[:, p].any()} == set(sm.RATE_CODES) - {1}


def test_a_reset_that_forgets_the_gate_counter_shows_in_the_expectation():
    """rnnoise_batch_reset_streams puts the gate counter back to 65536 (include/rnnoise_amd.h): every other RESET position carries a
    gate with a high threshold and a long hold, which the group's first loud frame opens for the rest of the run unless the restart
    closes it again.  Against a run of the oracle whose reset leaves the counter: for every K, `out` differs in at least 10
    row-frames (as many as the issue asks of every situation) of at least 3 restarted rows, and so do final counters"""
    pcm, _ = sm.block()
    ctl, msg = sm.controls(), {}
    gated = [p for p in sm.RESET if ctl[p, 1] > 0 and ctl[p, 2] == sm.RESET_HOLD]
    assert len(gated) >= len(sm.RESET) // 2 >= 10 and len(set(sm.RESET) - set(gated)) >= 10
    cut = sm.call_frames(sm.RESET_BEFORE)[0]
    for K in sm.LINK_KS:
        r = _linked(K, True)
        groups = [g for g in sm.link_groups(K) if any((g + k) % sm.B in gated for k in range(K))]
        r2 = sm.oracle_groups([load_blob("default"), load_blob("little")], pcm, K, ctl, sm.slots(), presence=sm.link_presence(K),
                              resets=sm.RESET, groups=groups, restart_counter=False)
        differ = (r2["out"][:, groups].view(np.uint32) != r["out"][:, groups].view(np.uint32)).any(-1)      # (T, groups, K)
        assert not differ[:cut].any()
        for name in ("vad", "gains", "silence"):                               # (the gate is in out and the synthesis tail alone)
            assert (r2[name][:, groups] == r[name][:, groups]).all(), name
        rows = differ.any(0)
        at = np.array([[(g + k) % sm.B in gated for k in range(K)] for g in groups])
        assert not (rows & ~at).any(), "a row without a restarted gate changed"
        msg[K] = dict(out_row_frames=int(differ.sum()), rows=int(rows.sum()), of_rows=int(at.sum()),
                      final_counters=int((r2["gate"][groups] != r["gate"][groups]).sum()))
        assert differ.sum() >= 10 and rows.sum() >= 3 and msg[K]["final_counters"] >= 1, msg
    print("counter restart", msg)


# ---- the chunk dressing (stream_mix.CHUNK_CASES, CHUNK_PUSHES, chunk_schedule(), chunk_expectation): what
# test_stream_mix_chunked_at_every_form runs ----
_CHUNK_MS = (480, 320, 160)
_CHUNKED = {}


def _chunked(hz, typ, mutant=None):
    """the CPU chain's chunk expectation of the block, on the goldens' profile"""
    from conftest import use_rcp_profile
    use_rcp_profile("intel")
    if (hz, typ, mutant) not in _CHUNKED:
        _CHUNKED[hz, typ, mutant] = sm.chunk_expectation(load_blob("default"), hz, typ, mutant=mutant)
    return _CHUNKED[hz, typ, mutant]


def _windows(a, w):
    """the sets of values that any w neighbouring positions hold (cyclic: the copies of a batch wrap from 388 to 0)"""
    return [set(a[np.arange(i, i + w) % sm.B].tolist()) for i in range(sm.B)]


@pytest.mark.parametrize("M", _CHUNK_MS)
def test_the_chunk_schedule_keeps_its_rules(M):
    assert {sm.chunk_frame(hz) for _, _, hz, _ in sm.CHUNK_CASES} == set(_CHUNK_MS)
    s, P = sm.chunk_schedule(M), sm.CHUNK_PUSHES
    Q = len(P)
    counts, listed, F, cum, fill, k = s["counts"], s["listed"], s["F"], s["cum"], s["fill"], s["k"]
    assert counts.shape == (Q, sm.B) and counts.dtype == np.int32 and (sm.chunk_counts(M) == counts).all()
    assert (s["max_count"] == [a * M + b for a, b in (p["max_count"] for p in P)]).all() and (F == (M - 1 + s["max_count"]) // M).all()
    assert (counts >= 0).all() and (counts <= s["max_count"][:, None]).all()
    # both schedules in both forms, back to back and alternating; one push wraps the 6-slot pitch ring
    kind = [(p["form"], bool(f > 1)) for p, f in zip(P, F)]
    for form in ("full", "list"):
        for piped in (False, True):
            at = [q for q in range(Q) if kind[q] == (form, piped)]
            assert any(b - a == 1 for a, b in zip(at, at[1:])), ("back to back", form, piped)
            assert any(q + 1 < Q and kind[q + 1] == (other, not piped) for q in at for other in ("full", "list") if other != form), (form, piped)
    assert (s["max_count"][F == 1] <= M).all() and (s["max_count"][F > 1] > M).all() and F.max() >= 7
    assert any(b % 2 for (_, b), f in zip((p["max_count"] for p in P), F) if f > 1)          # rows an odd number of samples apart
    # every position is pushed every special count in a full-size push and while listed (the position in no list push and the one in
    # every other list push: in the full-size pushes)
    never, alt = sm.SPECIAL["never"], sm.SPECIAL["alternating"]
    full = np.array([p["form"] == "full" for p in P])
    for p in range(sm.B):
        for form_rows, where in ((full, np.ones(Q, bool)), (~full, listed[:, p])):
            if not form_rows[0] and p in (never, alt):
                continue
            got = set(counts[form_rows & where, p].tolist())
            assert {0, 1, M - 1, M, M + 1, 2 * M} <= got, (p, form_rows[0], sorted(got))
            assert (counts[form_rows & where, p] == s["max_count"][form_rows & where]).any(), (p, "max_count")
    # unlisted positions push nothing; the hand-made rows carry over
    assert listed[full].all() and not counts[~listed].any()
    lists = np.flatnonzero(~full)
    assert not listed[lists, never].any() and (listed[lists, alt] == (np.arange(len(lists)) % 2 == 0)).all()
    for q in lists:
        assert abs(listed[q].mean() - P[q]["share"]) < 0.01 and P[q]["share"] == 0.8
        assert (~listed[q]).sum() >= 70                                       # (what "a list push that advances unlisted positions" bites on)
    # some push completes a frame exactly (on nearly every position), some leaves M - 1 pending
    moved = counts > 0
    assert ((s["fill_after"] == 0) & moved & (fill[:-1] != 0)).any(0).mean() >= 0.9 and ((s["fill_after"] == M - 1) & moved).any(0).sum() >= 20
    # in every push any 16 neighbours hold 3 different k (2 where F = 1: there are no more), k = 0 and k = F among them; before every
    # push but the first (every FIFO is empty then) any 64 neighbours hold 16 different fills
    assert (k >= 0).all() and (k <= F[:, None]).all() and (k == (fill[:-1] + counts) // M).all()
    for q in range(Q):
        for w in _windows(k[q], 16):
            assert len(w) >= min(3, F[q] + 1) and 0 in w and F[q] in w, (q, w)
        if q:
            assert min(len(w) for w in _windows(fill[q], 64)) >= 16, q
    assert not fill[0].any()
    # the reset drops something on every position of RESET; the move finds every fill class
    pend = cum[sm.CHUNK_RESET_BEFORE, list(sm.RESET)] % M
    assert (pend != 0).all() and len(set(pend.tolist())) >= 10 and (s["base"][-1, list(sm.RESET)] == cum[sm.CHUNK_RESET_BEFORE, list(sm.RESET)]).all()
    assert 0 < sm.CHUNK_RESET_BEFORE < sm.CHUNK_MOVE_BEFORE < min(q for q in range(Q) if P[q]["tail"])
    at = fill[sm.CHUNK_MOVE_BEFORE]
    assert (at == 0).any() and (at == 1).any() and (at == M - 1).any() and ((at > 1) & (at < M - 1)).sum() >= 100
    assert s["done"][sm.CHUNK_MOVE_BEFORE].min() >= 1 and len(set(s["done"][sm.CHUNK_MOVE_BEFORE].tolist())) >= 4
    # the tail tops every position up to whole frames: T M samples for the plain ones
    plain = np.setdiff1d(np.arange(sm.B), sm.RESET)
    assert (cum[-1] == s["total"]).all() and (s["total"][plain] == sm.T * M).all() and not fill[-1].any()
    assert ((s["total"] - s["base"][-1]) % M == 0).all() and (s["total"] > (sm.T - 2) * M).all()


@pytest.mark.parametrize("n,path,hz,typ", sm.CHUNK_CASES, ids=sm.CHUNK_IDS)
def test_every_chunk_case_lists_every_copy_once_and_three_entries_that_name_no_stream(n, path, hz, typ):
    M = sm.chunk_frame(hz)
    s = sm.chunk_schedule(M)
    assert n % sm.B != 0 and n <= 16421 and typ in ("float", "int16")
    for q, push in enumerate(sm.CHUNK_PUSHES):
        plan = sm.chunk_push_plan(n, q, M)
        if push["form"] == "full":
            assert plan["rows"] is None and (plan["src"] == np.arange(n) % sm.B).all() and (plan["counts"] == s["counts"][q][plan["src"]]).all()
            continue
        rows = sm.chunk_list_rows(n, q, M)
        assert rows.dtype == np.int32 and (rows == plan["rows"]).all() and len(rows) <= n
        bad = (rows < 0) | (rows >= n)
        assert bad.sum() == 3 and bad[0] and bad[-1] and bad[len(rows) // 2 - 1:len(rows) // 2 + 2].any()
        assert sorted(rows[bad].tolist()) == [-1, n, 2 ** 31 - 1] and (plan["named"] == ~bad).all()
        good = rows[~bad]
        assert len(set(good.tolist())) == len(good) and set(good.tolist()) == {i for i in range(n) if s["listed"][q][i % sm.B]}
        assert len(rows) == 3 + sum(int(s["listed"][q][i % sm.B]) for i in range(n))
        assert (np.diff(good) < 0).any()                                      # not in stream order
        assert (plan["counts"][~bad] == s["counts"][q][good % sm.B]).all()
        assert plan["counts"][bad].tolist() == [s["max_count"][q] // 2, 1, s["max_count"][q]]   # samples and a count of their own


def test_the_chunk_cases_reach_every_kernel_form(form_sweep):
    """every full-size push of every CHUNK_CASES entry through dispatch_test as the masked call it makes, every list push through
    list_dispatch_test with the push's row count: the forms the comments of CHUNK_CASES name, and together every form of form_sweep
    but rn_analysis_kernel, which per-stream frame phase cannot take"""
    run, plan_exe, list_exe, can_stream, can_list = form_sweep
    full, lists = {}, {}
    for case in sm.CHUNK_CASES:
        n, path, hz, typ = case
        M = sm.chunk_frame(hz)
        F = sm.chunk_schedule(M)["F"]
        if path is None:
            path = int(run(plan_exe, [f"path:{n}"])[0][0])
            assert path == 1, n
        pipes = [int(x[0]) for x in run(plan_exe, [f"sched:{f},0" for f in F])]
        assert pipes == [int(f > 1) for f in F]
        for q, push in enumerate(sm.CHUNK_PUSHES):
            if push["form"] == "full":
                full.setdefault(case, []).append((pipes[q],) + run(plan_exe, [f"plan:{n},1,256,{path},{pipes[q]},1,{int(hz != 48000)}"])[0])
            else:
                R = len(sm.chunk_list_rows(n, q, M))
                lists.setdefault(case, []).append((pipes[q],) + run(list_exe, [f"list:{n},{R},256,{pipes[q]},{int(hz != 48000)},{path}"])[0])
    seen_full = _forms_of([f[1:] for v in full.values() for f in v])
    seen_list = _forms_of([f[1:] for v in lists.values() for f in v])
    for kind in can_stream:
        assert seen_full[kind] == can_stream[kind], ("full-size", kind, can_stream[kind] - seen_full[kind])
        assert seen_list[kind] == can_list[kind], ("list", kind, can_list[kind] - seen_list[kind])
    assert "rn_analysis_kernel" not in can_stream["k1"]
    by = {(c[0], c[1]): c for c in sm.CHUNK_CASES}
    for f in full[by[252, 0]]:
        assert (f[1], f[3], f[5]) == ("rn_hp_one_kernel", "rn_nn_one_kernel", "rn_synthesis_few_kernel"), f
    assert {(f[0], f[3], f[5]) for f in full[by[390, 1]]} == {(0, "rn_nn_mfma16_kernel", "rn_synthesis_kernel"), (1, "rn_nn_mfma_kernel", "rn_synthesis_kernel")}
    assert {f[3:5] for f in full[by[390, 2]]} == {("layers", "rn_nn_gru_w8_kernel")} and by[390, 2][2] == 16000
    assert {(f[1], f[3]) for f in full[by[1031, 0]]} == {("rn_hp_one_kernel", "rn_nn_vector_kernel")} and by[1031, 0][2] == 32000
    assert {(f[0], f[1], f[3]) for f in full[by[3001, None]]} == {(0, "rn_hp_kernel", "rn_nn_mfma16_kernel"), (1, "rn_hp_kernel", "rn_nn_mfma_kernel")}
    assert {(f[1], f[3]) for f in full[by[4099, 0]]} == {("rn_hp_kernel", "rn_nn_vector_kernel")}
    assert {(f[1],) + f[3:5] for f in full[by[10277, None]]} == {("rn_hp_kernel", "layers", "rn_nn_gru_w8_kernel")}
    assert {(f[1],) + f[3:5] for f in full[by[16421, None]]} == {("rn_hp_kernel", "layers", "rn_nn_gru_kernel")}
    assert (16421 + 63) // 64 == 257 and 16421 % 64 and 16421 % 16 and 10277 % 16 and 10277 % 64
    # a low batch rate: the one-wave K0 at every size, so the lane = stream form is met at 48 kHz only
    assert {f[1] for c, v in full.items() if c[2] != 48000 for f in v} == {"rn_hp_one_kernel"}
    assert {f[3] for v in lists.values() for f in v} == {"rn_nn_one_kernel", "rn_nn_mfma16_kernel", "rn_nn_mfma_kernel"}


def _first_difference(good, bad, M):
    """where two chunk expectations part: (positions whose returned samples differ, the first (push, position) in push order)"""
    s = sm.chunk_schedule(M)
    total = s["cum"][-1]
    ne = (good["y"] != bad["y"]) & (np.arange(good["y"].shape[1])[None] < total[:, None])
    pos = np.flatnonzero(ne.any(1))
    if not len(pos):
        return pos, None
    first = np.array([np.flatnonzero(ne[p])[0] for p in pos])
    push = np.array([np.searchsorted(s["cum"][:, p], t, side="right") - 1 for p, t in zip(pos, first)])
    i = int(np.argmin(push))
    return pos, (int(push[i]), int(pos[i]))


# (variant the mutant is run on, the rule of the schedule that makes it differ)
_CHUNK_TEETH = {
    "no_delay": ((48000, "float"), "the tail tops every position up to T M samples, so all of z but its last frame is returned: z and "
                                   "0^M ++ z differ wherever a live signal is not periodic in M"),
    "reset_keeps_pending": ((48000, "int16"), "before push CHUNK_RESET_BEFORE every RESET position holds pending samples (fill != 0), so "
                                              "frames cut with them start `fill` samples early"),
    "reset_keeps_history": ((16000, "int16"), "RESET's positions are reset after completed frames of live signal, at a batch rate that "
                                              "has resampler histories to zero"),
    "frames_late": ((32000, "float"), "every position completes frames in many pushes; frames cut at x[1 + j M] differ from those at x[j M]"),
    "cast_before_down": ((16000, "int16"), "an int16 case runs at a low batch rate (CHUNK_CASES), where the down-resampler stands between "
                                           "the denoiser's float output and the cast"),
    "list_advances_unlisted": ((48000, "float"), "every list push leaves a fifth of the positions unlisted (and SPECIAL's never-listed one "
                                                 "always): advancing them changes every frame they complete later"),
}


@pytest.mark.parametrize("mutant", sm.CHUNK_MUTANTS)
def test_the_chunk_expectation_catches_a_wrong_one(mutant):
    """six wrong expectations, each of which must differ from the true one in the samples some push returns to some position"""
    (hz, typ), rule = _CHUNK_TEETH[mutant]
    M = sm.chunk_frame(hz)
    s = sm.chunk_schedule(M)
    good, bad = _chunked(hz, typ), _chunked(hz, typ, mutant)
    pos, first = _first_difference(good, bad, M)
    assert first is not None, f"{mutant}: the expectation does not change ({rule})"
    print(f"{mutant} ({hz} Hz {typ}): caught on {len(pos)} of {sm.B} positions, first in push {first[0]} at position {first[1]} -- {rule}")
    lab = sm.labels()[0]
    live = np.array([lab[p] not in ("all_zero",) for p in range(sm.B)])
    if mutant in ("reset_keeps_pending", "reset_keeps_history"):
        assert set(pos.tolist()) <= set(sm.RESET) and first[0] >= sm.CHUNK_RESET_BEFORE and len(pos) >= len(sm.RESET) - 3, (len(pos), first)
    elif mutant == "list_advances_unlisted":
        unlisted = np.flatnonzero((~s["listed"]).any(0))
        assert set(pos.tolist()) <= set(unlisted.tolist()) and len(pos) >= 0.9 * len(unlisted), (len(pos), len(unlisted))
        assert sm.SPECIAL["never"] in pos and first[0] <= min(q for q, p in enumerate(sm.CHUNK_PUSHES) if p["form"] == "list") + 3
    else:
        assert len(pos) >= 0.9 * live.sum(), len(pos)


def test_the_chunk_expectation_is_the_fifo_model_on_the_oracles_frames():
    """on 7 positions -- the never-listed one, the one in every other list push, two of RESET, the block's first and last -- the closed
    form equals the numpy deques of tests/test_chunks_gpu.py (Fifos) driven push by push with the oracle's frames: samples returned,
    frames completed, fills, vad and gains"""
    from conftest import assert_bits_equal
    from oracle.binding import Oracle
    from test_chunks_gpu import Fifos                                         # (lazily: its module carries the gpu mark)
    hz, typ, M = 48000, "float", 480
    s, exp = sm.chunk_schedule(M), _chunked(hz, typ)
    pos = [sm.SPECIAL["never"], sm.SPECIAL["alternating"], sm.RESET[0], sm.RESET[-1], 0, 1, sm.B - 1]
    blob = load_blob("default")
    fifos, oracles = Fifos(len(pos), M), [Oracle(blob) for _ in pos]
    done = np.zeros(len(pos), int)
    for q in range(len(sm.CHUNK_PUSHES)):
        if q == sm.CHUNK_RESET_BEFORE:
            hit = [i for i, p in enumerate(pos) if p in sm.RESET]
            fifos.restart(hit)
            for i in hit:
                oracles[i] = Oracle(blob)
        counts, mc, F = s["counts"][q][pos], int(s["max_count"][q]), int(s["F"][q])
        rows = np.full((len(pos), mc), np.nan, np.float32)
        for i, p in enumerate(pos):
            rows[i, :counts[i]] = exp["x"][p, s["cum"][q, p]:s["cum"][q + 1, p]]
        frames, mask, k = fifos.push(rows, counts, F)
        ref = np.zeros_like(frames)
        for i, p in enumerate(pos):
            if k[i]:
                r = oracles[i].run(frames[:k[i], i])
                ref[:k[i], i] = r["out"]
                assert_bits_equal(exp["vad"][p, done[i]:done[i] + k[i]], r["vad"], f"push {q} position {p}: vad")
                assert_bits_equal(exp["gains"][p, done[i]:done[i] + k[i]], r["gains"], f"push {q} position {p}: gains")
            assert done[i] == s["done"][q, p]
            done[i] += k[i]
        want = fifos.pop(ref, k, counts)
        assert (k == s["k"][q][pos]).all() and (fifos.fill() == s["fill_after"][q][pos]).all(), q
        for i, p in enumerate(pos):
            assert_bits_equal(exp["y"][p, s["cum"][q, p]:s["cum"][q + 1, p]], want[i], f"push {q} position {p}: the samples returned")
        if q + 1 == sm.CHUNK_MOVE_BEFORE:                                     # the FIFO records at the move are the deques' contents
            rec = sm.chunk_records(exp, M, q + 1)
            for i, p in enumerate(pos):
                f = int(s["fill"][q + 1, p])
                assert_bits_equal(rec[p, :f].view(np.float32), fifos.inq[i], f"position {p}: pending samples at the move")
                assert_bits_equal(rec[p, 480:480 + M - f].view(np.float32), fifos.outq[i], f"position {p}: output FIFO at the move")
                assert not rec[p, f:480].any() and not rec[p, 480 + M - f:960].any() and rec[p, 960:].tolist() == [f, M, 0x464B4301, 0]
                assert_bits_equal(exp["move_state"][p], oracles[i].get_state(), f"position {p}: state at the move")
    for i, p in enumerate(pos):
        assert_bits_equal(exp["state"][p], oracles[i].get_state(), f"position {p}: final state")
        assert done[i] == s["done"][-1, p]


def test_the_int16_and_low_rate_chunk_expectations_are_their_chains():
    """what the 48 kHz float model above does not reach: the int16 expectation is the float chain on the rounded input followed by the
    truncating cast, and a low-rate one the same chain between resample.up and resample.down, restarted with the reset"""
    from rnnoise_amd import resample
    from oracle.binding import Oracle
    blob = load_blob("default")
    for hz, typ in sm.CHUNK_VARIANTS:
        M, L = sm.chunk_frame(hz), resample.RATES[hz]
        s, exp = sm.chunk_schedule(M), _chunked(hz, typ)
        assert exp["x"].dtype == (np.float32 if typ == "float" else np.int16) and exp["y"].dtype == exp["x"].dtype
        assert (exp["y"] == (exp["yf"] if typ == "float" else resample.to_s16(exp["yf"]))).all()
        assert not exp["yf"][:, :M].any()
        for p in (2, sm.RESET[3]):
            x = exp["x"][p].astype(np.float32)
            c = int(s["base"][-1, p])
            parts = []
            for a, b in (((0, c // M * M), (c, int(s["total"][p]))) if c else ((0, sm.T * M),)):
                o = Oracle(blob)
                v = x[a:b] if L == 1 else resample.up(x[a:b], L)
                out = o.run(v.reshape(-1, 480))["out"].reshape(-1)
                parts.append(out if L == 1 else resample.down(out, L))
            want = np.concatenate([np.zeros(M, np.float32), parts[0]])
            if c:
                want = np.concatenate([want[:c], np.zeros(M, np.float32), parts[1]])
            n = int(s["total"][p])
            assert (exp["yf"][p, :n].view(np.uint32) == want[:n].view(np.uint32)).all(), (hz, typ, p)
            assert (exp["state"][p].view(np.uint32) == o.get_state().view(np.uint32)).all(), (hz, typ, p)


# ---- the feature dressing (stream_mix.FEATURE_CASES, feature_records(), feature_expectation()): what
# test_stream_mix_feature_calls_at_every_form and the two tests behind it run ----
@pytest.fixture(scope="module")
def feature_mix(mix):
    """(records, the compute_rnn-only expectation, the oracle's lock-step run of the block) on the goldens' profile"""
    _, _, want = mix
    rec = sm.feature_records(want)
    return rec, sm.feature_expectation(load_blob("default"), rec), want


def _feature_forms(lines):
    """the (network form, GRU form where the network is layer-wise) of dispatch_test's output lines"""
    return {(nn, gru if nn == "layers" else None) for _, _, nn, gru, _ in lines}


def test_the_feature_cases_reach_every_form_a_feature_call_can_take(form_sweep):
    """A feature call plans a whole batch, unpipelined, in lock step, at 48 kHz (rnnoise_amd/csrc/batch_eval.cpp: eval_device): the
    forms of plan:n,1,256,path,0,0,0 over form_sweep's sizes and the three paths are exactly those FEATURE_CASES produce, and every
    case runs the form its comment names"""
    run, plan_exe, _, _, _ = form_sweep
    can = _feature_forms(run(plan_exe, [f"plan:{n},1,256,{path},0,0,0" for n in _sweep_sizes() for path in (0, 1, 2)]))
    got = {}
    for n, path in sm.FEATURE_CASES:
        p = int(run(plan_exe, [f"path:{n}"])[0][0]) if path is None else path
        assert path is not None or p == 1, n
        got[n, path], = _feature_forms(run(plan_exe, [f"plan:{n},1,256,{p},0,0,0"]))
    assert set(got.values()) == can, (can - set(got.values()), set(got.values()) - can)
    assert got == {(251, 0): ("rn_nn_one_kernel", None), (389, 1): ("rn_nn_mfma16_kernel", None), (389, 2): ("layers", "rn_nn_gru_w8_kernel"),
                   (4096, None): ("rn_nn_mfma16_kernel", None), (4099, 0): ("rn_nn_vector_kernel", None),
                   (4099, 1): ("rn_nn_mfma_kernel", None), (10277, None): ("layers", "rn_nn_gru_w8_kernel"),
                   (40037, None): ("layers", "rn_nn_gru_kernel")}
    assert len(sm.FEATURE_IDS) == len(set(sm.FEATURE_IDS)) == len(sm.FEATURE_CASES) and sm.FEATURE_CALLS == sm.CALLS
    # the units the comments speak of: 257 tiles on 256 CUs, seven groups, ragged tiles and groups, more groups than CUs
    assert (4099 + 15) // 16 == 257 and 4096 // 16 == 256 and (389 + 63) // 64 == 7 and (40037 + 63) // 64 > 256 >= (10277 + 63) // 64
    assert all(n % 16 and n % 64 for n in (389, 4099, 10277, 40037))
    # the eight-wave tile kernel is met on path 1 between 4,097 and 10,239 streams only, the layer-wise network by size from 10,240 on
    edges = [x[2] for x in run(plan_exe, [f"plan:{n},1,256,1,0,0,0" for n in (4096, 4097, 10239, 10240)])]
    assert edges == ["rn_nn_mfma16_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma_kernel", "layers"], edges


def _target_kind(row):
    """the kind (stream_mix.TARGET_KINDS) of a record's 32 gain targets, told from the values alone"""
    import eval_cases as ec
    g = row[65:97]
    if (g == -1).all():
        return "minus_one"
    if ((g > -1) & (g < 0)).all():
        return "negative"
    if (g == 0).all():
        return "zero"
    if (g == 1).all():
        return "one"
    if set(g.tolist()) == {float(np.float32(x)) for x in ec.TINY}:
        return "tiny"
    if set(g.tolist()) == {float(np.float32(x)) for x in (-1.0, -0.5, 0.0, 1e-20, 1.0, 0.3)}:
        return "mix"
    limit = int((g != -1).sum())
    assert limit >= 1 and ((g[:limit] > 0) & (g[:limit] < 1)).all() and (g[limit:] == -1).all(), g
    return "ordinary"


def test_the_feature_records_keep_their_coverage(feature_mix):
    """Recomputed here (goldens' profile; the silence decision does not depend on the profile): 304 stream-frames of 29 positions have
    65 features that are all exactly zero, 7 positions throughout and 22 partly; every call of FEATURE_CALLS has between 9 and 20 such
    positions in its first and in its last frame; 241 of the 256 whole tiles of a 4,099-stream batch hold such a row beside a live one"""
    rec, _, want = feature_mix
    assert rec.shape == (sm.T, sm.B, sm.REC) and rec.dtype == np.float32 and np.isfinite(rec).all()
    assert (rec[..., :65].view(np.uint32) == want["features"].view(np.uint32)).all()
    assert sm.feature_records(want).tobytes() == rec.tobytes()
    zero = ~rec[..., :65].any(-1)
    assert (zero == (want["silence"] != 0)).all(), "the zero-feature rows are not the oracle's silent frames"
    some, always = zero.any(0), zero.all(0)
    assert (int(zero.sum()), int(some.sum()), int(always.sum()), int((some & ~always).sum())) == (304, 29, 7, 22)
    for c in range(len(sm.FEATURE_CALLS)):
        fr = sm.call_frames(c, sm.FEATURE_CALLS)
        for t in (fr[0], fr[-1]):
            assert 9 <= zero[t].sum() <= 20, (c, t, int(zero[t].sum()))
    idx = np.arange(4099) % sm.B
    z = zero[:, idx[:4096]].reshape(sm.T, 256, 16)
    mixed = (z.any(-1) & ~z.all(-1)).any(0)
    assert mixed.sum() >= 200, int(mixed.sum())
    # the targets: a function of position and frame, every kind there, no two neighbours (cyclic: the copies wrap) alike
    kinds = [[_target_kind(rec[t, p]) for p in range(sm.B)] for t in range(sm.T)]
    assert all(k == kinds[0] for k in kinds), "a position changes its kind of targets from frame to frame"
    kinds = kinds[0]
    assert kinds == [sm.TARGET_KINDS[k] for k in sm.target_kinds()]
    assert all(kinds.count(k) >= sm.B // 8 for k in sm.TARGET_KINDS), {k: kinds.count(k) for k in sm.TARGET_KINDS}
    assert all(kinds[p] != kinds[(p + 1) % sm.B] for p in range(sm.B))
    vad = {k: rec[:, [p for p in range(sm.B) if kinds[p] == k], 97] for k in sm.TARGET_KINDS}
    for k in sm.TARGET_KINDS[:-1]:                                            # 0, 0.5 and 1 in turn on every edge position
        assert all(set(row.tolist()) == {0.0, 0.5, 1.0} and (row[1:] != row[:-1]).all() for row in vad[k].T), k
    v = vad["ordinary"]
    assert ((v >= 0) & (v <= 1)).all() and (v == 0).any() and (v == 1).any() and ((v > 0) & (v < 1)).mean() > 0.5
    limits = {int((rec[0, p, 65:97] != -1).sum()) for p in range(sm.B) if kinds[p] == "ordinary"}
    assert len(limits) >= 16 and 32 in limits and min(limits) <= 4, sorted(limits)
    assert (rec[:, [p for p in range(sm.B) if kinds[p] == "mix"], 65:97][:-1] != rec[:, [p for p in range(sm.B) if kinds[p] == "mix"], 65:97][1:]).any()
    # the zero-feature rows meet most kinds of target
    assert len({kinds[p] for p in np.flatnonzero(some)}) >= 5, {kinds[p] for p in np.flatnonzero(some)}


def test_the_feature_expectation_is_anchored_to_the_pinned_oracle_run(feature_mix):
    """tests/test_oracle.py compares the block's `process` run with the compiled reference; here compute_rnn alone is held to that run:
    on every position that is never silent (360 of them) the compute_rnn walk over the run's features gives the run's gains and VAD
    bit for bit -- and on the others up to their first silent frame"""
    rec, exp, want = feature_mix
    zero = ~rec[..., :65].any(-1)
    never = np.flatnonzero(~zero.any(0))
    assert len(never) == 360
    assert (exp["gains"][:, never].view(np.uint32) == want["gains"][:, never].view(np.uint32)).all()
    assert (exp["vad"][:, never].view(np.uint32) == want["vad"][:, never].view(np.uint32)).all()
    for p in np.flatnonzero(zero.any(0) & ~zero[0]):
        t = int(np.flatnonzero(zero[:, p])[0])
        assert (exp["gains"][:t, p].view(np.uint32) == want["gains"][:t, p].view(np.uint32)).all(), p
    # the walk ran the network on every all-zero row: a sigmoid's output, where `process` leaves 32 zero gains
    assert exp["gains"][zero].all() and not want["gains"][zero].any()
    # the sums, written out once more for one position of every kind: step t against record t - 1, from step 4 on
    import eval_cases as ec
    for k in range(len(sm.TARGET_KINDS)):
        p = int(never[sm.target_kinds()[never] == k][0])
        terms = [ec.loss_terms(rec[t - 1, p, 65:97], rec[t - 1, p, 97], exp["gains"][t, p], exp["vad"][t, p]) for t in range(4, sm.T)]
        by_hand = [sum(float(g.sum()) for g, _ in terms), sum(float(v) for _, v in terms), sm.T - 4, 0]
        assert np.allclose(exp["sums"][p], by_hand, rtol=1e-12, atol=0), (p, exp["sums"][p], by_hand)
    assert exp["state"].shape[0] == sm.B and exp["sums"].shape == (sm.B, 4) and np.isfinite(exp["sums"]).all()
    assert (exp["sums"][:, 0] > 0).sum() > 300 and (exp["sums"][:, 1] > 0).sum() > 150       # (the sums are about something)


def test_the_feature_expectation_has_teeth(feature_mix):
    """a feature call that skipped the network on all-zero rows, as rnnoise_batch_process does on a silent frame, would give other
    gains on the live frames of at least 15 of the 22 partly silent positions (measured: 20; the other two are silent only at their
    end); a lag of 0 or 2 between a step and its record moves the gain sums of more than half of the positions that have one"""
    import eval_cases as ec
    rec, exp, _ = feature_mix
    blob = load_blob("default")
    zero = ~rec[..., :65].any(-1)
    partly = np.flatnonzero(zero.any(0) & ~zero.all(0))
    skip = sm.feature_expectation(blob, rec, mutant="silent_frames_skip")
    moved = [p for p in partly if (skip["gains"][~zero[:, p], p] != exp["gains"][~zero[:, p], p]).any()]
    print(f"silent_frames_skip: caught on {len(moved)} of {len(partly)} partly silent positions")
    assert len(moved) >= 15, (len(moved), len(partly))
    never = ~zero.any(0)
    assert (skip["gains"][:, never] == exp["gains"][:, never]).all() and not skip["gains"][zero].any()
    scored = np.flatnonzero(exp["sums"][:, 0] > 0)
    for mutant in ("lag0", "lag2"):
        off = sm.feature_expectation(blob, rec, mutant=mutant)
        assert (off["gains"] == exp["gains"]).all() and (off["sums"][:, 2] == exp["sums"][:, 2]).all()
        moved = [p for p in scored if ec.rel_diff(off["sums"][p, 0], exp["sums"][p, 0]) > 1e-6]
        print(f"{mutant}: the gain sums of {len(moved)} of {len(scored)} positions move")
        assert len(moved) > len(scored) / 2, (mutant, len(moved), len(scored))
