"""The front of the layer-wise network (rn_nn_front_kernel: conv1, conv2) serves 64 streams -- four 16-stream tiles -- per workgroup.

What can go wrong there and nowhere else: the last workgroup owning one to three tiles, its last tile one to fifteen rows; the four
tiles of a group sharing every weight fragment (a mix-up between them shows only when they hold different streams); silent streams
and rows of another model slot inside a group that otherwise runs.  Every case forces the layer-wise network at a small size
(set_nn_path(2)) and compares bit for bit with the oracle, the state also with the 16-stream tile kernel (set_nn_path(1))."""
import numpy as np
import pytest

from conftest import assert_bits_equal, load_blob
from oracle.binding import Oracle
from rnnoise_amd import capi, synth

pytestmark = [pytest.mark.gpu, pytest.mark.rcp("host")]

OFF_CONV1, OFF_CONV2, OFF_GRU, OFF_GRU_END = 2724, 2854, 3110, 4262  # include/rn_layout.h: RN_OFF_CONV1, _CONV2, _GRU1, _DELAYED_X
STATE_FIELDS = (("conv1_state", OFF_CONV1, OFF_CONV2), ("conv2_state", OFF_CONV2, OFF_GRU), ("gru_state", OFF_GRU, OFF_GRU_END))
T_EDGE, CALLS_EDGE = 6, (4, 1, 1)
NAMES = ("out", "vad", "gains")


def test_the_state_offsets_are_the_layout_headers():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "rn_layout.h")).read()
    env = {}
    for name, expr in re.findall(r"^#define (RN_\w+) (\([^/\n]*\)|\d+)\s", text, re.M):
        try:
            env[name] = eval(expr, {}, env)
        except Exception:
            pass
    assert (env["RN_OFF_CONV1"], env["RN_OFF_CONV2"], env["RN_OFF_GRU1"], env["RN_OFF_DELAYED_X"]) == (OFF_CONV1, OFF_CONV2, OFF_GRU, OFF_GRU_END)


def run_calls(b, pcm, calls, after=None):
    parts, t = [], 0
    for i, c in enumerate(calls):
        parts.append(b.process(pcm[t:t + c]))
        t += c
        if after:
            after(i)
    assert t == pcm.shape[0]
    return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


class OracleRuns:
    """the oracle's answer per (blob, stream, PCM), computed once and shared by the cases: outputs, and the state after every
    prefix of the calls"""

    def __init__(self):
        self.memo = {}

    def get(self, key, blob, pcm, calls):
        if key not in self.memo:
            o, outs, states, t = Oracle(blob), [], [], 0
            for c in calls:
                outs.append(o.run(pcm[t:t + c]))
                states.append(o.get_state())
                t += c
            self.memo[key] = ({k: np.concatenate([w[k] for w in outs]) for k in NAMES + ("silence",)}, states)
        return self.memo[key]


@pytest.fixture(scope="module")
def oracle_runs():
    return OracleRuns()


@pytest.fixture(scope="module")
def blobs():
    return [load_blob("default"), load_blob("little")]


@pytest.fixture(scope="module")
def models(blobs):
    return [capi.Model(b) for b in blobs]


@pytest.fixture(scope="module")
def edge_pcm():
    return synth.batch_pcm(range(129), T_EDGE)  # stream s has the same PCM at every batch size: one oracle run per stream


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 113, 129])
def test_edges_of_the_group(models, blobs, oracle_runs, edge_pcm, n):
    """partial tile, partial group and both; four frames in one call (frames 3 and later run on shifted conv histories), then two
    one-frame calls"""
    pcm = np.ascontiguousarray(edge_pcm[:, :n])
    assert n < 32 or not np.array_equal(pcm[:, 0], pcm[:, 16])  # (the tiles of a group are no look-alikes)
    layers, tiles = capi.Batch(models[0], n), capi.Batch(models[0], n)
    layers.set_nn_path(2)
    tiles.set_nn_path(1)
    got, ref = run_calls(layers, pcm, CALLS_EDGE), run_calls(tiles, pcm, CALLS_EDGE)
    for s in range(n):
        want, states = oracle_runs.get(("edge", s), blobs[0], pcm[:, s], CALLS_EDGE)
        for name, a in zip(NAMES, got):
            assert_bits_equal(a[:, s], want[name], f"{n} streams, stream {s} {name} against the oracle")
        mine, theirs = layers.export_state(s), tiles.export_state(s)
        for f, lo, hi in STATE_FIELDS:
            assert_bits_equal(mine[lo:hi], theirs[lo:hi], f"{n} streams, stream {s} {f} against the tile kernel")
        assert_bits_equal(mine, theirs, f"{n} streams, stream {s} state against the tile kernel")
        assert_bits_equal(mine, states[-1], f"{n} streams, stream {s} state against the oracle")
    for name, a, r in zip(NAMES, got, ref):
        assert_bits_equal(a, r, f"{n} streams, {name} against the tile kernel")
    layers.close()
    tiles.close()


def test_silence_inside_a_group(models, blobs, oracle_runs, edge_pcm):
    """streams 3, 16, 47 and 64 of 65 are fed zeros in frames 2-3, signal otherwise: outputs and the conv state after every call are
    the oracle's.  Two zero frames behind signal are not silent frames yet: the input high-pass rings for several frames, so the
    oracle's silence flag stays 0 and its conv state moves through them (the next test feeds zeros until the flag is raised)"""
    n, quiet, calls = 65, (3, 16, 47, 64), (2, 2, 2)
    pcm = np.ascontiguousarray(edge_pcm[:, :n])
    pcm[2:4, list(quiet)] = 0
    b = capi.Batch(models[0], n)
    b.set_nn_path(2)
    seen = []
    got = run_calls(b, pcm, calls, after=lambda i: seen.append([b.export_state(s) for s in range(n)]))
    for s in range(n):
        key = ("quiet", s) if s in quiet else ("edge-222", s)
        want, states = oracle_runs.get(key, blobs[0], pcm[:, s], calls)
        for name, a in zip(NAMES, got):
            assert_bits_equal(a[:, s], want[name], f"stream {s} {name}")
        for i in range(len(calls)):
            for f, lo, hi in STATE_FIELDS:
                assert_bits_equal(seen[i][s][lo:hi], states[i][lo:hi], f"stream {s} {f} after call {i}")
    b.close()


def test_silent_frames_inside_a_group(models, blobs, oracle_runs):
    """the same four streams fed zeros in frames 2-11 of 13: the oracle flags their frames 9-11 silent (asserted), which are the
    second call here, so their conv and GRU state is frozen across that call while every neighbour's moves; the last frame is
    live again and runs on the kept state"""
    n, quiet, calls = 65, (3, 16, 47, 64), (9, 3, 1)
    pcm = synth.batch_pcm(range(n), sum(calls))
    pcm[2:12, list(quiet)] = 0
    b = capi.Batch(models[0], n)
    b.set_nn_path(2)
    seen = []
    got = run_calls(b, pcm, calls, after=lambda i: seen.append([b.export_state(s) for s in range(n)]))
    for s in range(n):
        want, states = oracle_runs.get(("long-quiet" if s in quiet else "long", s), blobs[0], pcm[:, s], calls)
        assert want["silence"][9:12].all() if s in quiet else not want["silence"].any(), f"stream {s}: the oracle's silence flags"
        for name, a in zip(NAMES, got):
            assert_bits_equal(a[:, s], want[name], f"stream {s} {name}")
        for i in range(len(calls)):
            for f, lo, hi in STATE_FIELDS:
                assert_bits_equal(seen[i][s][lo:hi], states[i][lo:hi], f"stream {s} {f} after call {i}")
        if s in quiet:
            assert_bits_equal(seen[1][s][OFF_CONV1:OFF_GRU_END], seen[0][s][OFF_CONV1:OFF_GRU_END], f"stream {s}: network state across its silent frames")
            assert seen[0][s][OFF_CONV1:OFF_GRU].any()
        else:
            assert not np.array_equal(seen[1][s][OFF_CONV1:OFF_GRU], seen[0][s][OFF_CONV1:OFF_GRU])
    b.close()


MAPS = {
    "alternating": lambda s: s & 1,
    "by-tile": lambda s: (s // 16) & 1,
    "slot-1-absent-from-the-last-group": lambda s: np.where(s < 64, s & 1, 0),
}


@pytest.mark.parametrize("kind", list(MAPS))
def test_two_model_slots_inside_a_group(models, blobs, oracle_runs, kind):
    n, calls = 80, (3, 1)
    pcm = synth.batch_pcm(range(n), sum(calls))
    slots = np.ascontiguousarray(MAPS[kind](np.arange(n)), np.uint8)
    assert set(slots[:64].tolist()) == {0, 1} and (kind != "slot-1-absent-from-the-last-group" or not slots[64:].any())
    b = capi.Batch(models[0], n)
    assert b.add_model(models[1]) == 1
    b.set_stream_models(slots)
    b.set_nn_path(2)
    got = run_calls(b, pcm, calls)
    for s in range(n):
        want, states = oracle_runs.get(("slot", int(slots[s]), s), blobs[slots[s]], pcm[:, s], calls)
        for name, a in zip(NAMES, got):
            assert_bits_equal(a[:, s], want[name], f"{kind}: stream {s} (slot {slots[s]}) {name}")
        assert_bits_equal(b.export_state(s), states[-1], f"{kind}: stream {s} (slot {slots[s]}) state")
    b.close()
