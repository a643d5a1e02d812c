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
(test_stream_mix_linked_at_every_form, test_stream_mix_linked_masked_and_listed_at_every_form)."""
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
