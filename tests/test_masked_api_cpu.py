"""CPU checks of the masked-call / per-stream reset API (include/rnnoise_amd.h): declared, exported by both product libraries,
bound by ctypes and by the torch custom op, and argument errors refused without touching a GPU."""
import ctypes as C

import pytest

from abi_contract import declared_once, exported
from rnnoise_amd import capi

NEW = ["rnnoise_batch_process_device_masked", "rnnoise_batch_process_device_masked_s16", "rnnoise_batch_process_masked",
       "rnnoise_batch_process_masked_s16", "rnnoise_batch_reset_streams", "rnnoise_batch_reset_streams_device"]


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_both_product_libraries_export_them(so):
    exported(so, NEW)


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


# the registered ops as a caller's traces and exported graphs name them: name -> schema
SCHEMAS = {
    "process": "(Tensor pcm, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)",
    "process_masked": "(Tensor pcm, Tensor active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)",
    "process_list": "(Tensor pcm, Tensor idx, Tensor? active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)",
    "process_streams": "(Tensor pcm, Tensor? active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)",
    "process_channels": "(Tensor pcm, Tensor? active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)",
    "process_chunks": "(Tensor pcm, Tensor counts, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor, Tensor)",
    "process_chunks_list": "(Tensor pcm, Tensor counts, Tensor idx, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor, Tensor)",
    "analyze": "(Tensor pcm, Tensor(a!) state, int handle) -> (Tensor, Tensor)",
    "synthesize": "(Tensor gains, Tensor vad, Tensor like, Tensor(a!) state, int handle) -> Tensor",
}


def test_torch_op_schemas_are_pinned():
    torch = pytest.importorskip("torch")
    from rnnoise_amd import torch_op
    torch_op.register_torch_op()
    for name, schema in SCHEMAS.items():
        assert str(getattr(torch.ops.rnnoise_amd, name).default._schema) == f"rnnoise_amd::{name}{schema}", name
