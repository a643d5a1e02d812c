"""CPU checks of the stream snapshots (include/rnnoise_amd.h: rnnoise_batch_save_streams / load_streams and their device forms):
declared, exported by both product libraries and the instrumented one, bound by ctypes, capi.Batch and the torch op; the record's
layout constants (include/rn_layout.h: RN_SNAP_*) against their rules and against the Python mirror; bad arguments refused without
a GPU; and the two state kernels still the only ones in their source file, with no scalar store in it."""
import ctypes as C
import os
import re

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_save_streams_device", "rnnoise_batch_load_streams_device", "rnnoise_batch_save_streams",
       "rnnoise_batch_load_streams"]


def test_prototypes_declared_once_each_with_export():
    src = declared_once(NEW)
    assert re.search(r"#define\s+RNNOISE_AMD_SNAP_FLOATS\s+RN_SNAP_FLOATS\b", src)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_the_product_libraries_and_the_instrumented_one_export_them(so):
    exported(so, NEW)


def test_ctypes_capi_and_torch_bindings():
    L = capi.lib()
    for n in NEW:
        assert getattr(L, n).argtypes, n
    assert len(L.rnnoise_batch_save_streams_device.argtypes) == 5
    assert len(L.rnnoise_batch_load_streams_device.argtypes) == 5
    assert len(L.rnnoise_batch_save_streams.argtypes) == 4
    assert len(L.rnnoise_batch_load_streams.argtypes) == 4
    for m in ("save_streams", "load_streams", "save_streams_device", "load_streams_device"):
        assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.save_streams) and callable(torch_op.RNNoiseOp.load_streams)


def header_constants():
    """the #defines of include/rn_layout.h, evaluated (they are integer expressions over each other)"""
    src = open(os.path.join(ROOT, "include", "rn_layout.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    vals = {}
    for name, expr in re.findall(r"^#define\s+(RN_\w+)\s+(.+?)\s*$", src, flags=re.M):
        if "(" in name:
            continue
        try:
            vals[name] = int(eval(expr, {"__builtins__": {}}, dict(vals)))
        except Exception:
            pass
    return vals


def test_layout_constants():
    h = header_constants()
    assert h["RN_STATE_FLOATS"] == 6282 == capi.STATE_FLOATS
    # the prefix is the portable state; the header follows it; the history starts on a 16-byte boundary; rows are 16-byte multiples
    assert h["RN_SNAP_OFF_MAGIC"] == h["RN_STATE_FLOATS"]
    assert h["RN_SNAP_FLOATS"] % 4 == 0
    assert h["RN_SNAP_OFF_HIST"] % 4 == 0
    assert h["RN_SNAP_HIST_FLOATS"] == 336
    assert h["RN_SNAP_FLOATS"] == h["RN_SNAP_OFF_HIST"] + h["RN_SNAP_HIST_FLOATS"]
    head = [h[k] for k in ("RN_SNAP_OFF_MAGIC", "RN_SNAP_OFF_L", "RN_SNAP_OFF_GATE", "RN_SNAP_OFF_RESERVED")]
    assert head == sorted(set(head)) and head[0] >= h["RN_STATE_FLOATS"] and h["RN_SNAP_OFF_RESERVED"] < h["RN_SNAP_OFF_HIST"]
    assert h["RN_SNAP_MAGIC"] != 0 and h["RN_SNAP_GATE_NONE"] == 65536
    # the history length is the kernels' (rn_dev.h: RN_RS_HIST = 48 + 47 * 6 + 6)
    dev = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "rn_dev.h")).read()
    assert re.search(r"#define RN_RS_HIST \(RN_RS_DOWN0 \+ RN_RS_DOWN_HIST\(6\) \+ 6\)", dev) and 48 + 47 * 6 + 6 == 336
    # the Python mirror
    for py, c in (("SNAP_OFF_MAGIC", "RN_SNAP_OFF_MAGIC"), ("SNAP_OFF_L", "RN_SNAP_OFF_L"), ("SNAP_OFF_GATE", "RN_SNAP_OFF_GATE"),
                  ("SNAP_OFF_RESERVED", "RN_SNAP_OFF_RESERVED"), ("SNAP_OFF_HIST", "RN_SNAP_OFF_HIST"),
                  ("SNAP_HIST_FLOATS", "RN_SNAP_HIST_FLOATS"), ("SNAP_FLOATS", "RN_SNAP_FLOATS"), ("SNAP_MAGIC", "RN_SNAP_MAGIC"),
                  ("SNAP_GATE_NONE", "RN_SNAP_GATE_NONE")):
        assert getattr(capi, py) == h[c], (py, c)


def test_bad_arguments_return_minus_one_without_a_gpu():
    L = capi.lib()
    buf = (C.c_float * capi.SNAP_FLOATS)()
    idx = (C.c_int * 1)(0)
    for n in (1, 0, -1):  # a NULL batch, whatever the count
        assert L.rnnoise_batch_save_streams(None, buf, idx, n) == -1
        assert L.rnnoise_batch_load_streams(None, buf, idx, n) == -1
        assert L.rnnoise_batch_save_streams_device(None, None, None, n, None) == -1
        assert L.rnnoise_batch_load_streams_device(None, None, None, n, None) == -1
    # (a batch needs a GPU; what the calls do with a real one on n < 0 and NULL buffers is in tests/test_snapshot_gpu.py)


def test_the_state_kernels_keep_their_names_and_hold_no_scalar_store():
    src = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "state_kernels.hip")).read()
    kernels = re.findall(r"__global__\s+void(?:\s+__launch_bounds__\(\d+\))?\s+(\w+)\s*\(", src)
    assert sorted(kernels) == ["rn_release_store_kernel", "rn_state_gather_kernel", "rn_state_scatter_kernel"], kernels
    assert "getenv" not in src and "RN_LAB_ENV" not in src
    assert not re.search(r"\basm\b", src)  # plain C++ only: every store is a vector store the compiler chose
