"""CPU checks of the mixed-rate batches (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates, its device form and the read-back):
declared, exported by both product libraries and the instrumented one, bound by ctypes, capi.Batch and the torch op; bad arguments
refused without a GPU; the Hz -> divisor conversion of capi.Batch.set_stream_rates and what it refuses; and the plan of a batch with
a rate table (rnnoise_amd/csrc/dispatch.h: rn_shape_low_rate)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_set_stream_rates", "rnnoise_batch_set_stream_rates_device", "rnnoise_batch_stream_rates"]


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_the_product_libraries_and_the_instrumented_one_export_them(so):
    exported(so, NEW)


def test_ctypes_capi_and_torch_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_set_stream_rates.argtypes) == 2
    assert len(L.rnnoise_batch_set_stream_rates_device.argtypes) == 3
    assert len(L.rnnoise_batch_stream_rates.argtypes) == 2
    for m in ("set_stream_rates", "set_stream_rates_device", "stream_rates"):
        assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.set_stream_rates)


def test_bad_arguments_return_minus_one_without_a_gpu():
    L = capi.lib()
    buf = (C.c_ubyte * 4)(1, 2, 3, 6)
    assert L.rnnoise_batch_set_stream_rates(None, buf) == -1
    assert L.rnnoise_batch_set_stream_rates(None, None) == -1
    assert L.rnnoise_batch_set_stream_rates_device(None, None, None) == -1
    assert L.rnnoise_batch_set_stream_rates_device(None, C.cast(buf, C.c_void_p), None) == -1
    assert L.rnnoise_batch_stream_rates(None, buf) == -1
    assert L.rnnoise_batch_stream_rates(None, None) == -1
    assert list(buf) == [1, 2, 3, 6]
    # (a batch needs a GPU: a NULL buffer on a real batch, and entries a batch refuses, are in tests/test_stream_rates_gpu.py)


class _FakeLib:
    """the C entry point as a recorder: capi.Batch.set_stream_rates must validate and convert before it gets here"""

    def __init__(self):
        self.calls = []

    def rnnoise_batch_set_stream_rates(self, h, p):
        self.calls.append(None if p is None else [p[i] for i in range(4)])
        return 0

    def rnnoise_batch_pcm_rate(self, h):
        return self.rate


def _fake_batch(rate, n=4):
    b = capi.Batch.__new__(capi.Batch)
    b._L, b.h, b.n = _FakeLib(), 1, n
    b._L.rate = rate
    return b


def test_capi_converts_hz_to_divisors_and_refuses_what_the_batch_cannot_take():
    b = _fake_batch(48000)
    b.set_stream_rates([48000, 24000, 16000, 8000])
    assert b._L.calls == [[1, 2, 3, 6]]
    b.set_stream_rates(None)
    assert b._L.calls[-1] is None
    for bad in ([48000, 44100, 16000, 8000], [48000, 0, 16000, 8000], [48000, 12000, 16000, 8000]):
        with pytest.raises(ValueError):
            b.set_stream_rates(bad)
    assert len(b._L.calls) == 2
    low = _fake_batch(16000)
    low.set_stream_rates(np.array([16000, 8000, 8000, 16000]))
    assert low._L.calls == [[3, 6, 6, 3]]
    for bad in ([48000, 16000, 16000, 16000], [16000, 24000, 8000, 8000]):  # a rate above the batch's: the frame would not fit the row
        with pytest.raises(ValueError):
            low.set_stream_rates(bad)
    assert len(low._L.calls) == 1
    b.h = None  # (nothing to destroy)
    low.h = None


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rates_dispatch") / "rates_dispatch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "rates_dispatch_test.cpp"), "-o", exe],
                   check=True)

    def run(n, rate, table, pipelined=False, **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
        env.update({f"RNNOISE_AMD_{k}": str(v) for k, v in knobs.items()})
        r = subprocess.run([exe, f"rates:{n},{rate},{int(table)},{int(pipelined)}"], capture_output=True, text=True, check=True, env=env)
        return tuple(r.stdout.split())
    return run


def test_a_rate_table_plans_like_a_low_rate_batch(prog):
    for pipelined in (False, True):
        # without a table a 48 kHz batch of this size runs the lane = stream K0; with one, one wave per stream at every size
        assert prog(65536, 48000, False, pipelined)[0] == "rn_hp_kernel"
        assert prog(65536, 48000, True, pipelined)[0] == "rn_hp_one_kernel"
        assert prog(65536, 48000, True, pipelined, HP_ONE_MAX=0)[0] == "rn_hp_one_kernel"
        # ... and everything else as the uniform low-rate batch of that size: K1 four streams per workgroup, the layer-wise network
        assert prog(65536, 48000, True, pipelined) == prog(65536, 16000, False, pipelined)
        assert prog(65536, 48000, True, pipelined)[1:3] == ("rn_analysis_kernel", "layers")
        assert prog(65536, 16000, True, pipelined) == prog(65536, 16000, False, pipelined)
    for n in (1, 2049, 4096):
        assert prog(n, 48000, True)[0] == "rn_hp_one_kernel"
        assert prog(n, 48000, True)[1:] == prog(n, 48000, False)[1:]
