"""CPU checks of linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link): declared, exported by the product libraries and
the instrumented one, bound by ctypes, the torch op and the CLI, NULL batches refused without a GPU; the setter's rule and the
sibling-stream helper of the synthesis kernel compiled for the host; the fold rules on hand-made values; and the link oracle
(tests/csrc/link_oracle.c) against the existing oracles, bit for bit, where a link changes nothing.  (The setter on a live batch --
its refusals, its return value, what leaves the count alone -- needs a device: tests/test_gain_link_gpu.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

from abi_contract import declared_once, exported
from conftest import ROOT, assert_bits_equal, load_blob
from ctl_oracle import CtlOracle
from link_oracle import C_NONE, LinkGroup, fold
from rnnoise_amd import capi, synth

NEW = ["rnnoise_batch_set_gain_link", "rnnoise_batch_gain_link"]


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_libraries_export_them(so):
    exported(so, NEW)


def test_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_set_gain_link.argtypes) == 2 and len(L.rnnoise_batch_gain_link.argtypes) == 1
    assert callable(capi.Batch.set_gain_link) and isinstance(capi.Batch.gain_link, property)
    import inspect

    from rnnoise_amd import cli, torch_op
    assert callable(torch_op.RNNoiseOp.set_gain_link)
    assert "link" in inspect.signature(torch_op.RNNoiseOp.process_channels).parameters
    assert "link_channels" in inspect.signature(cli.denoise_files).parameters


def test_null_batch_returns_minus_one():
    L = capi.lib()
    for k in (1, 2, 8, 0, -1, 9):
        assert L.rnnoise_batch_set_gain_link(None, k) == -1
    assert L.rnnoise_batch_gain_link(None) == -1


def test_no_new_kernel_and_the_field_is_k3s_alone():
    """a mode of the two synthesis kernels, not a kernel; RnGroupDev::link is written in one place, the step, on K3's copy"""
    csrc = os.path.join(ROOT, "rnnoise_amd", "csrc")
    assert not any("link" in k for f in os.listdir(csrc) if f.endswith(".hip")
                   for k in re.findall(r"__global__[^(]*?(\w+)\s*\(", open(os.path.join(csrc, f)).read()))
    host = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".cpp")}
    writers = [f for f, text in host.items() for _ in re.findall(r"[.>]link\s*=[^=]", text)]
    assert sorted(writers) == ["batch_step.cpp", "batch_tables.cpp"], writers  # (g.link of the step; b->link of the setter)
    assert "g.link = link > 1 ? link : 0;" in host["batch_step.cpp"]
    for f, text in host.items():
        assert "b->g.link" not in text, f


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("link_dispatch") / "link_dispatch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "link_dispatch_test.cpp"), "-o", exe],
                   check=True)
    return lambda cases: subprocess.run([exe] + list(cases), capture_output=True, text=True, check=True).stdout.splitlines()


def test_setter_rule(prog):
    """1 .. RNNOISE_AMD_MAX_CHANNELS, and a divisor of the batch's streams: 0, 9 and a non-divisor are refused"""
    cases = {(1, 12): 1, (2, 12): 1, (3, 12): 1, (8, 16): 1, (8, 264): 1, (3, 264): 1, (1, 7): 1, (0, 12): 0, (-1, 12): 0, (9, 18): 0,
             (5, 12): 0, (8, 12): 0, (2, 7): 0}
    assert [int(x) for x in prog([f"ok:{k},{n}" for k, n in cases])] == list(cases.values())
    src = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "batch_tables.cpp")).read()
    assert re.search(r"rnnoise_batch_set_gain_link\(RNNoiseBatch \*b, int k\) \{\s*if \(!b \|\| !rn_pcm_channels_ok\(k, b->n\)\) return -1;", src)


def test_sibling_stream_helper(prog):
    """member j of row's group: row k * (row / k) + j, through the list with its range check in a list call"""
    for k in (2, 3, 8):
        rows = range(0, 3 * k)
        got = prog([f"sib:{r},{k},{j}" for r in rows for j in range(k)])
        assert [int(x) for x in got] == [r // k * k + j for r in rows for j in range(k)]
    lst = [11, 3, 7, 0, 12, -1, 5, 9, 2]  # over 12 streams: entry 12 and entry -1 name no stream
    for k in (3, 9 // 3):
        got = prog([f"lsib:12,{r},{k},{j}," + ",".join(map(str, lst)) for r in range(9) for j in range(k)])
        want = [lst[r // k * k + j] for r in range(9) for j in range(k)]
        assert [int(x) for x in got] == [w if 0 <= w < 12 else -1 for w in want]


# ---- the fold rules on hand-made values ----
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_fold_rules():
    nan = np.float32(np.nan)
    a, b, c = (np.full(32, v, np.float32) for v in (0.5, 0.25, 0.75))
    a[3], b[3], c[3] = 0.1, 0.9, 0.05
    g, v = fold([a, b, c], [0.2, 0.9, 0.4])
    assert_bits_equal(g, np.minimum(np.minimum(a, b), c), "min of three")
    assert v == np.float32(0.9)
    g1, v1 = fold([a], [0.3])  # one participant: its own values
    assert_bits_equal(g1, a, "one participant")
    assert v1 == np.float32(0.3)
    # row order: the fold keeps the FIRST of equal values -- -0.0 and +0.0 compare equal, so the first one's sign stays
    z0, z1 = np.full(32, -0.0, np.float32), np.full(32, 0.0, np.float32)
    assert (_bits(fold([z0, z1], [0, 0])[0]) == 0x80000000).all() and (_bits(fold([z1, z0], [0, 0])[0]) == 0).all()
    assert _bits(fold([z0, z1], [-0.0, 0.0])[1]) == 0x80000000 and _bits(fold([z0, z1], [0.0, -0.0])[1]) == 0
    # a NaN first value stays; a NaN later never replaces
    n = a.copy()
    n[5] = nan
    g, v = fold([n, b], [nan, 0.5])
    assert np.isnan(g[5]) and np.isnan(v)
    assert_bits_equal(np.delete(g, 5), np.delete(np.minimum(a, b), 5), "the other bands")
    g, v = fold([b, n, c], [0.5, nan, 0.1])
    assert g[5] == min(b[5], c[5]) and v == np.float32(0.5)
    # no participant: vad_link 0
    g, v = fold(np.zeros((0, 32), np.float32), [])
    assert _bits(v) == 0


# ---- the link oracle against the existing ones ----
T = 8


@pytest.fixture(scope="module")
def blob():
    return load_blob("default")


def _pcm(streams, lead_silence=0):
    return synth.batch_pcm(streams, T, lead_silence=lead_silence)  # (T, n, 480)


CTL = (0.1, 0.5, 2)


def _ctl_run(blob, pcm, ctl):
    o = CtlOracle(blob)
    r = o.run(pcm, ctl)
    return r, o


@pytest.mark.parametrize("ctl", [None, CTL], ids=["plain", "controls"])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_identical_rows_equal_unlinked_runs(blob, K, ctl):
    """a group of K identical signals: every fold returns the row's own values"""
    pcm = _pcm([5], lead_silence=2)
    want, o = _ctl_run(blob, pcm[:, 0], ctl if ctl else (0, 0, 0))
    grp = LinkGroup(blob, K, None if ctl is None else [ctl] * K)
    got = grp.run(np.repeat(pcm, K, axis=1))
    for k in range(K):
        for name in ("out", "vad", "gains"):
            assert_bits_equal(got[name][:, k], want[name], f"row {k} {name}")
        assert_bits_equal(grp.state[k], o.state, f"row {k} state")
        assert grp.c[k] == o.c
    assert (got["n"][2:] == K).all() and (got["n"][:2] == 0).all()


@pytest.mark.parametrize("other", ["absent", "silent"])
def test_lone_row_equals_the_plain_oracle(blob, other):
    """a group whose other rows are absent, or all-zero (silent): the remaining row is the plain oracle's"""
    K = 3
    pcm = _pcm([9, 33, 71])
    o = CtlOracle(blob)
    want = o.run(pcm[:, 1])  # (no controls: rno_process_frame)
    grp = LinkGroup(blob, K)
    x = pcm.copy()
    active = None
    if other == "silent":
        x[:, 0] = 0
        x[:, 2] = 0
    else:
        active = np.zeros((T, K), np.uint8)
        active[:, 1] = 1
    got = grp.run(x, active)
    for name in ("out", "vad", "gains"):
        assert_bits_equal(got[name][:, 1], want[name], name)
    assert_bits_equal(grp.state[1], o.state, "state")
    assert (got["n"] == 1).all()
    if other == "absent":
        assert not grp.state[0].any() and not grp.state[2].any() and (grp.c[[0, 2]] == C_NONE).all()
        assert not got["out"][:, [0, 2]].any()


@pytest.mark.parametrize("ctl", [(0, 0, 0), CTL, (0.3, 0.9, 0)])
def test_k1_equals_the_ctl_oracle(blob, ctl):
    pcm = _pcm([17], lead_silence=1)
    want, o = _ctl_run(blob, pcm[:, 0], ctl)
    grp = LinkGroup(blob, 1, [ctl])
    got = grp.run(pcm)
    for name in ("out", "vad", "gains"):
        assert_bits_equal(got[name][:, 0], want[name], name)
    assert_bits_equal(grp.state[0], o.state, "state")
    assert grp.c[0] == o.c


def test_link_changes_something_and_only_what_it_should(blob):
    """two different signals: the linked run differs from the unlinked one in `out`, the fold is what numpy's rule gives on the rows'
    own raw gains, and a silent row takes the group's VAD into its gate without participating"""
    pcm = _pcm([3, 130])
    pcm[:3, 1] = 0  # row 1 starts silent (after a signal the high-pass rings on above the silence threshold for many frames)
    ctl = [(0, 0.5, 0), (0, 0.5, 0)]
    grp = LinkGroup(blob, 2, ctl)
    got = grp.run(pcm)
    quiet = np.nonzero(got["silence"][:, 1] == 1)[0]
    assert list(quiet) == [0, 1, 2] and (got["n"][quiet] == 1).all() and (got["silence"][:, 0] == 0).all()
    assert not got["vad"][quiet, 1].any()
    for t in range(T):
        p = [k for k in range(2) if got["silence"][t, k] == 0]
        g, v = fold(got["gains"][t, p], got["vad"][t, p])
        assert_bits_equal(got["g_link"][t], g, f"frame {t} g_link")
        assert_bits_equal(got["vad_link"][t], v, f"frame {t} vad_link")
    solo = [CtlOracle(blob).run(pcm[:, k], ctl[k]) for k in range(2)]
    assert any(not np.array_equal(_bits(got["out"][:, k]), _bits(solo[k]["out"])) for k in range(2))
