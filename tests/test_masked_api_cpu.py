"""CPU checks of the masked-call / per-stream reset API (include/rnnoise_amd.h): declared, exported by both product libraries,
bound by ctypes and by the torch custom op, and argument errors refused without touching a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_process_device_masked", "rnnoise_batch_process_device_masked_s16", "rnnoise_batch_process_masked",
       "rnnoise_batch_process_masked_s16", "rnnoise_batch_reset_streams", "rnnoise_batch_reset_streams_device"]


def test_prototypes_declared_once_each_with_export():
    src = open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    for n in NEW:
        assert len(re.findall(rf"RNNOISE_EXPORT\s+int\s+{n}\s*\(", src)) == 1, n
        assert n in capi.EXPORTS, n


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_both_product_libraries_export_them(so):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "rnnoise_amd", so)], capture_output=True, text=True).stdout
    for n in NEW:
        assert re.search(rf"\bT {n}\b", nm), (so, n)


def test_ctypes_bindings():
    L = capi.lib()
    for n in NEW:
        assert getattr(L, n).argtypes, n
    assert len(L.rnnoise_batch_process_device_masked.argtypes) == 8
    assert len(L.rnnoise_batch_process_masked_s16.argtypes) == 7
    assert len(L.rnnoise_batch_reset_streams_device.argtypes) == 4
    for m in ("process_masked", "process_masked_s16", "process_masked_device", "reset_streams", "reset_streams_device"):
        assert callable(getattr(capi.Batch, m)), m


def test_bad_arguments_fail_without_a_gpu():
    L = capi.lib()
    buf = (C.c_float * 480)()
    sbuf = (C.c_short * 480)()
    act = (C.c_ubyte * 1)(1)
    idx = (C.c_int * 2)(0, 1 << 20)
    # no batch
    assert L.rnnoise_batch_process_masked(None, buf, buf, None, None, act, 1) == -1
    assert L.rnnoise_batch_process_masked_s16(None, sbuf, sbuf, None, None, act, 1) == -1
    assert L.rnnoise_batch_process_device_masked(None, None, None, None, None, None, 1, None) == -1
    assert L.rnnoise_batch_process_device_masked_s16(None, None, None, None, None, None, 1, None) == -1
    assert L.rnnoise_batch_reset_streams(None, idx, 1) == -1
    assert L.rnnoise_batch_reset_streams_device(None, None, 1, None) == -1
    # negative counts, out-of-range indices (refused before the batch is looked at: no batch needed to see -1)
    assert L.rnnoise_batch_process_masked(None, buf, buf, None, None, act, -1) == -1
    assert L.rnnoise_batch_reset_streams(None, idx, -1) == -1
    assert L.rnnoise_batch_reset_streams(None, idx, 2) == -1
    assert L.rnnoise_batch_reset_streams_device(None, None, -3, None) == -1


def test_torch_op_schema_and_fake():
    torch = pytest.importorskip("torch")
    from rnnoise_amd import torch_op
    torch_op.register_torch_op()
    op = torch.ops.rnnoise_amd.process_masked
    assert "Tensor active" in str(op.default._schema) and "Tensor(a!) state" in str(op.default._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pcm = torch.empty(3, 5, 480)
        act = torch.empty(3, 5, dtype=torch.uint8)
        st = torch.zeros(1, dtype=torch.int64)
        out, vad, gains = op(pcm, act, st, 0)
        assert out.shape == (3, 5, 480) and vad.shape == (3, 5) and gains.shape == (3, 5, 32)
    for m in ("process_masked", "reset_streams"):
        assert callable(getattr(torch_op.RNNoiseOp, m)), m
