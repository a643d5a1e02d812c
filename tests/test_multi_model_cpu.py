"""CPU checks of per-stream model selection (include/rnnoise_amd.h: rnnoise_batch_add_model and the stream-model map): declared once,
exported, bound by ctypes, the capi and torch wrappers present, and argument errors refused without touching a GPU."""
import ctypes as C
import os
import re

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_add_model", "rnnoise_batch_set_stream_models", "rnnoise_batch_set_stream_models_device",
       "rnnoise_batch_stream_models"]
HEADER = os.path.join(ROOT, "include", "rnnoise_amd.h")


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


def test_max_models_is_eight():
    src = open(HEADER).read()
    assert re.search(r"^#define RNNOISE_AMD_MAX_MODELS 8$", src, re.M)
    assert capi.MAX_MODELS == 8


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_the_product_libraries_export_them(so):
    # (both: the two product libraries export the same declared set -- tests/test_capi_cpu.py holds them to it)
    exported(so, NEW)


def test_ctypes_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_add_model.argtypes) == 2
    assert len(L.rnnoise_batch_set_stream_models.argtypes) == 2
    assert len(L.rnnoise_batch_set_stream_models_device.argtypes) == 3
    assert len(L.rnnoise_batch_stream_models.argtypes) == 2
    for m in ("add_model", "set_stream_models", "set_stream_models_device", "stream_models"):
        assert callable(getattr(capi.Batch, m)), m


def test_null_arguments_fail_without_a_gpu():
    L = capi.lib()
    slots = (C.c_ubyte * 4)(0, 1, 0, 1)
    assert L.rnnoise_batch_add_model(None, None) == -1
    assert L.rnnoise_batch_set_stream_models(None, slots) == -1
    assert L.rnnoise_batch_set_stream_models(None, None) == -1
    assert L.rnnoise_batch_set_stream_models_device(None, None, None) == -1
    assert L.rnnoise_batch_stream_models(None, slots) == -1
    assert L.rnnoise_batch_stream_models(None, None) == -1


def test_torch_op_takes_extra_models():
    pytest.importorskip("torch")
    import inspect
    from rnnoise_amd import torch_op
    assert "extra_models" in inspect.signature(torch_op.RNNoiseOp.__init__).parameters
    assert callable(torch_op.RNNoiseOp.set_stream_models)
