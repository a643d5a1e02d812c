"""CPU checks of the per-stream suppression controls (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls): the oracle of the
controls (tests/csrc/ctl_oracle.c) against the plain oracle -- all zeros is the plain oracle bit for bit, a closed gate outputs the
previous synthesis tail and leaves a zero one, a floor changes no state word but synthesis_mem --, and the product surface: declared
once, exported by both product libraries, bound by ctypes, argument errors refused without a GPU, the dB helper."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from abi_contract import declared_once, exported
from conftest import ROOT, assert_bits_equal, golden, load_blob
from ctl_oracle import C_NONE, CtlOracle
from oracle.binding import Oracle
from rnnoise_amd import capi

NEW = ["rnnoise_batch_set_stream_controls", "rnnoise_batch_set_stream_controls_device", "rnnoise_batch_stream_controls"]
HEADER = os.path.join(ROOT, "include", "rnnoise_amd.h")
SYN0, SYN1 = 480, 960  # synthesis_mem in the portable state (include/rn_layout.h: RN_OFF_SYNTHESIS)


@pytest.fixture(scope="module")
def blob():
    return load_blob("default")


def streams():
    """the committed golden inputs (speech-like, silent gaps, clicks) and a NaN-poisoned stream"""
    d, e = golden("detail_default.npz"), golden("edge_default.npz")
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    out = {"s3": f(d["s3_pcm"]), "s77": f(d["s77_pcm"][:60]), "gaps": f(e["gaps_pcm"]), "impulses": f(e["impulses_pcm"])}
    bad = out["s3"][:40].copy()
    bad[12, 100] = np.nan
    out["nan"] = bad
    return out


def run_both(blob, pcm, ctl):
    """frame by frame: the plain oracle and the ctl oracle side by side, with the states after every frame"""
    a, b = CtlOracle(blob), CtlOracle(blob)
    rows = []
    for t in range(pcm.shape[0]):
        pre = b.state.copy()
        ra = a.process(pcm[t])
        rb = b.process(pcm[t], ctl)
        rows.append((ra, rb, a.state.copy(), b.state.copy(), pre, b.c))
    return rows


@pytest.mark.parametrize("name", ["s3", "s77", "gaps", "impulses", "nan"])
def test_all_zero_controls_are_the_plain_oracle(blob, name):
    pcm = streams()[name]
    for t, (ra, rb, sa, sb, _, _) in enumerate(run_both(blob, pcm, (0, 0, 0))):
        for what, x, y in zip(("out", "vad", "gains"), ra, rb):
            assert_bits_equal(y, x, f"{name} frame {t} {what}")
        assert_bits_equal(sb, sa, f"{name} frame {t} state")


def test_ctl_library_is_the_oracle(blob):
    """the ctl oracle's library is oracle/rn_oracle.c compiled once more: its plain frame equals liboracle.so's"""
    pcm = streams()["s3"][:30]
    want = Oracle(blob).run(pcm)
    got = CtlOracle(blob).run(pcm)
    for k in ("out", "vad", "gains"):
        assert_bits_equal(got[k], want[k], k)


@pytest.mark.parametrize("name", ["s3", "gaps", "nan"])
def test_closed_gate_outputs_the_synthesis_tail(blob, name):
    """thr = 1, hold = 0 and no voice frame yet: the gate is closed on every frame whose vad is below 1"""
    pcm = streams()[name]
    closed = 0
    for t, (ra, rb, sa, sb, pre, c) in enumerate(run_both(blob, pcm, (0, 1.0, 0))):
        assert_bits_equal(rb[1], ra[1], f"frame {t} vad")  # (the controls change neither vad nor gains)
        assert_bits_equal(rb[2], ra[2], f"frame {t} gains")
        if c == 0:
            continue
        closed += 1
        assert_bits_equal(rb[0], pre[SYN0:SYN1] + np.float32(0), f"frame {t}: out is the previous synthesis tail")
        assert_bits_equal(sb[SYN0:SYN1], np.zeros(480, np.float32), f"frame {t}: synthesis_mem")
        rest = np.r_[0:SYN0, SYN1:sb.size]
        assert_bits_equal(sb[rest], sa[rest], f"frame {t}: every other state word")
    assert closed >= pcm.shape[0] - 2


@pytest.mark.parametrize("floor_db", [6, 20, 40])
def test_floor_changes_only_synthesis_mem(blob, floor_db):
    pcm = streams()["s3"]
    fl = float(capi.floor_of_limit_db(floor_db))
    differs = 0
    for t, (ra, rb, sa, sb, _, _) in enumerate(run_both(blob, pcm, (fl, 0, 0))):
        assert_bits_equal(rb[1], ra[1], f"frame {t} vad")
        assert_bits_equal(rb[2], ra[2], f"frame {t} gains")
        rest = np.r_[0:SYN0, SYN1:sb.size]
        assert_bits_equal(sb[rest], sa[rest], f"frame {t}: state outside synthesis_mem")
        differs += not np.array_equal(ra[0], rb[0])
    assert differs > 0, "a floor that changes no output"


def test_gate_counter_and_hold(blob):
    """the counter follows the returned vad (the frame's own vad counts before the gate is decided), and the gate closes exactly when
    c > hold; a gated frame outputs the previous synthesis tail"""
    pcm = np.concatenate([streams()["gaps"], streams()["s3"][:40]])
    thr, hold = 0.6, 3
    o = CtlOracle(blob)
    c, seen_open, seen_closed = C_NONE, 0, 0
    for t in range(pcm.shape[0]):
        pre = o.state.copy()
        out, vad, _ = o.process(pcm[t], (0, thr, hold))
        c = 0 if vad >= thr else min(c + 1, C_NONE)
        assert o.c == c, f"frame {t}"
        if c > hold:
            seen_closed += 1
            assert_bits_equal(out, pre[SYN0:SYN1] + np.float32(0), f"frame {t}: gated")
        else:
            seen_open += 1
    assert seen_open and seen_closed


def test_nan_controls_read_as_zero(blob):
    """the oracle takes an entry as the kernel does: NaN as 0, clamped into range, hold truncated"""
    pcm = streams()["s3"][:30]
    a, b = CtlOracle(blob), CtlOracle(blob)
    for t in range(pcm.shape[0]):
        ra = a.process(pcm[t], (0, 0.5, 2))
        rb = b.process(pcm[t], (float("nan"), 0.5, 2.9))
        for x, y in zip(ra, rb):
            assert_bits_equal(y, x, f"frame {t}")
    a, b = CtlOracle(blob), CtlOracle(blob)
    for t in range(pcm.shape[0]):
        assert_bits_equal(b.process(pcm[t], (-3, float("nan"), -1))[0], a.process(pcm[t], (0, 0, 0))[0], f"frame {t}")


# ---- surface ----
def test_prototypes_declared_once_each_with_export():
    src = declared_once(NEW)
    assert re.search(r"^#define RNNOISE_AMD_CTL_FLOATS 3$", src, re.M)
    assert capi.CTL_FLOATS == 3
    # the drop-in header has no controls
    assert "stream_controls" not in open(os.path.join(ROOT, "include", "rnnoise.h")).read()


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_the_product_libraries_export_them(so):
    exported(so, NEW)


def test_ctypes_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_set_stream_controls.argtypes) == 2
    assert len(L.rnnoise_batch_set_stream_controls_device.argtypes) == 3
    assert len(L.rnnoise_batch_stream_controls.argtypes) == 2
    for m in ("set_stream_controls", "set_stream_controls_device", "stream_controls"):
        assert callable(getattr(capi.Batch, m)), m


def test_null_arguments_fail_without_a_gpu():
    L = capi.lib()
    t = (C.c_float * 6)(0, 0, 0, 0.5, 0.5, 3)
    assert L.rnnoise_batch_set_stream_controls(None, t) == -1
    assert L.rnnoise_batch_set_stream_controls(None, None) == -1
    assert L.rnnoise_batch_set_stream_controls_device(None, None, None) == -1
    assert L.rnnoise_batch_stream_controls(None, t) == -1
    assert L.rnnoise_batch_stream_controls(None, None) == -1


def test_db_helper():
    for db in (0.0, 3.0, 6.0, 20.0, 40.0, 96.0):
        f = capi.floor_of_limit_db(db)
        assert f.dtype == np.float32 and f == np.float32(10 ** (-db / 20))
        assert abs(float(capi.limit_db_of_floor(f)) - db) < 1e-4
    assert capi.floor_of_limit_db(np.inf) == 0 and capi.limit_db_of_floor(0.0) == np.inf
    assert capi.floor_of_limit_db(20.0) == np.float32(0.1)
    t = capi.controls_table(4, limit_db=[0, 6, 20, np.inf], vad_threshold=0.5, hold_frames=[0, 1, 2, 3])
    assert t.dtype == np.float32 and t.shape == (4, 3)
    assert_bits_equal(t[:, 0], capi.floor_of_limit_db([0, 6, 20, np.inf]))
    assert (t[:, 1] == np.float32(0.5)).all() and (t[:, 2] == [0, 1, 2, 3]).all()
    assert not capi.controls_table(3).any()


def test_torch_op_and_cli_take_the_controls():
    import inspect
    try:
        from rnnoise_amd import torch_op
    except ImportError:  # (torch is optional for the C API; the op needs it)
        torch_op = None
    if torch_op is not None:
        sig = inspect.signature(torch_op.RNNoiseOp.set_stream_controls).parameters
        assert {"limit_db", "vad_threshold", "hold_frames"} <= set(sig)
        assert callable(torch_op.RNNoiseOp.clear_stream_controls)
    h = subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "denoise", "--help"], cwd=ROOT, capture_output=True, text=True).stdout
    for flag in ("--atten-limit-db", "--vad-gate", "--vad-hold"):
        assert flag in h, flag
