"""CPU checks of the per-stream PCM formats (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats, its device form and the
read-back): declared, exported by both product libraries and the instrumented one and by nothing outside the rnnoise_ namespace, bound
by ctypes, capi.Batch, the torch op and the CLI; bad arguments refused without a GPU; the names capi.Batch.set_stream_formats takes;
and the plan of an int16 call of a batch with a format table (rnnoise_amd/csrc/dispatch.h: RnStepShape::companded) -- K0 one wave per
stream at every size, nothing else moved, and the member's default the plan of every boundary tests/test_dispatch_cpu.py walks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_set_stream_formats", "rnnoise_batch_set_stream_formats_device", "rnnoise_batch_stream_formats"]


def test_prototypes_and_codes_declared_once_each():
    src = declared_once(NEW)
    for name, v in (("LINEAR", 0), ("ULAW", 1), ("ALAW", 2)):
        assert len(re.findall(rf"#define\s+RNNOISE_AMD_PCM_{name}\s+{v}\b", src)) == 1, name
    from rnnoise_amd import g711
    assert (g711.LINEAR, g711.ULAW, g711.ALAW) == (0, 1, 2)
    dev = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "g711.h")).read()
    for name, v in (("LINEAR", 0), ("ULAW", 1), ("ALAW", 2)):
        assert re.search(rf"#define\s+RN_PCM_{name}\s+{v}\b", dev), name


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_the_product_libraries_and_the_instrumented_one_export_them(so):
    exported(so, NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_nothing_of_the_feature_leaves_the_rnnoise_namespace(so):
    """the drop-in library's dynamic symbols outside rnnoise_*: none, so none named after the codec or the table either"""
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "rnnoise_amd", so)], capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in nm.splitlines() if ln.strip()]
    assert names and all(n.startswith("rnnoise_") for n in names), [n for n in names if not n.startswith("rnnoise_")][:5]
    assert not [n for n in names if re.search(r"g711|ulaw|alaw|pcm_fmt", n)]


def test_ctypes_capi_torch_and_cli_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_set_stream_formats.argtypes) == 2
    assert len(L.rnnoise_batch_set_stream_formats_device.argtypes) == 3
    assert len(L.rnnoise_batch_stream_formats.argtypes) == 2
    for m in ("set_stream_formats", "set_stream_formats_device", "stream_formats"):
        assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import cli, torch_op
    assert callable(torch_op.RNNoiseOp.set_stream_formats)
    import inspect
    assert "formats" in inspect.signature(cli.denoise_files).parameters


def test_bad_arguments_return_minus_one_without_a_gpu():
    L = capi.lib()
    buf = (C.c_ubyte * 4)(0, 1, 2, 1)
    assert L.rnnoise_batch_set_stream_formats(None, buf) == -1
    assert L.rnnoise_batch_set_stream_formats(None, None) == -1
    assert L.rnnoise_batch_set_stream_formats_device(None, None, None) == -1
    assert L.rnnoise_batch_set_stream_formats_device(None, C.cast(buf, C.c_void_p), None) == -1
    assert L.rnnoise_batch_stream_formats(None, buf) == -1
    assert L.rnnoise_batch_stream_formats(None, None) == -1
    assert list(buf) == [0, 1, 2, 1]
    # (a batch needs a GPU: a NULL buffer on a real batch, and an entry a batch refuses, are in tests/test_stream_formats_gpu.py)


class _FakeLib:
    """the C entry point as a recorder: capi.Batch.set_stream_formats must convert and validate before it gets here"""

    def __init__(self):
        self.calls = []

    def rnnoise_batch_set_stream_formats(self, h, p):
        self.calls.append(None if p is None else [p[i] for i in range(4)])
        return 0


def test_capi_converts_names_to_codes_and_refuses_unknown_ones():
    b = capi.Batch.__new__(capi.Batch)
    b._L, b.h, b.n = _FakeLib(), 1, 4
    b.set_stream_formats(["s16", "ulaw", "alaw", "ulaw"])
    assert b._L.calls == [[0, 1, 2, 1]]
    b.set_stream_formats(np.array([2, 0, 1, 2]))
    assert b._L.calls[-1] == [2, 0, 1, 2]
    b.set_stream_formats(None)
    assert b._L.calls[-1] is None
    for bad in (["s16", "mulaw", "alaw", "s16"], [0, 1, 2, 3], ["s16", "g722", "s16", "s16"]):
        with pytest.raises(ValueError):
            b.set_stream_formats(bad)
    assert len(b._L.calls) == 3
    b.h = None  # (nothing to destroy)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("formats_dispatch") / "formats_dispatch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "formats_dispatch_test.cpp"), "-o", exe],
                   check=True)

    def run(cases, **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
        env.update({f"RNNOISE_AMD_{k}": str(v) for k, v in knobs.items()})
        r = subprocess.run([exe] + [f"fmt:{','.join(str(int(v)) for v in c)}" for c in cases], capture_output=True, text=True, check=True, env=env)
        return [tuple(ln.split()) for ln in r.stdout.splitlines()]
    return run


# the sizes tests/test_dispatch_cpu.py pins a boundary at, both sides of each
SIZES = [1, 15, 16, 17, 99, 100, 101, 255, 256, 257, 511, 512, 513, 1600, 1601, 2047, 2048, 2049, 2559, 2560, 2561, 4096, 4097, 6400, 6401,
         8192, 10239, 10240, 12288, 16384, 16385, 40037, 65536]


def _shapes():
    for n in SIZES:
        for whole in (1, 0):
            for cus in (256, 100):
                for path in (0, 1, 2):
                    for pipelined in (0, 1):
                        for per_stream, low_rate, listed in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)):
                            yield (n, whole, cus, path, pipelined, per_stream, low_rate, listed)


@pytest.mark.parametrize("knobs", [{}, {"HP_ONE_MAX": 0}, {"HP_ONE_MAX": 100}, {"K1_SPW": 4, "TILE_WAVES": 8, "NN_LAYERS_MIN": 100, "NN_ONE_MAX": 0}])
def test_a_format_table_forces_k0_one_wave_per_stream_and_moves_nothing_else(prog, knobs):
    shapes = list(_shapes())
    off = prog([s + (0,) for s in shapes], **knobs)
    on = prog([s + (1,) for s in shapes], **knobs)
    dflt = prog([s + (-1,) for s in shapes], **knobs)
    assert len(off) == len(on) == len(dflt) == len(shapes)
    assert dflt == off  # the default member: the plan of a shape built by code that has never heard of it
    for s, a, b in zip(shapes, off, on):
        assert b[0] == "rn_hp_one_kernel", s
        assert b[1:] == a[1:], s
    # ... and the forced form is a change where a table-less batch takes the lane = stream kernel
    moved = [s for s, a in zip(shapes, off) if a[0] == "rn_hp_kernel"]
    assert moved and all(not s[6] and not s[7] for s in moved)
    if not knobs:
        assert {s[0] for s in moved} == {n for n in SIZES if n > 2048}


def test_the_default_member_gives_the_plans_test_dispatch_pins(prog):
    d = lambda n, whole=1, cus=256, path=0, pipelined=0, per_stream=0, low_rate=0: prog([(n, whole, cus, path, pipelined, per_stream, low_rate, 0, -1)])[0]
    assert d(2048)[0] == "rn_hp_one_kernel" and d(2049)[0] == "rn_hp_kernel"
    assert d(65536, low_rate=1)[0] == "rn_hp_one_kernel"
    assert d(2559)[1] == "rn_analysis_single_kernel" and d(2560)[1] == "rn_analysis_kernel"
    assert d(512)[2] == "rn_nn_one_kernel" and d(513)[2] == "rn_nn_vector_kernel"
    assert d(10239, path=1, pipelined=1)[2] == "rn_nn_mfma_kernel" and d(10240, path=1, pipelined=1)[2] == "layers"
    assert d(4096, path=1)[2] == "rn_nn_mfma16_kernel" and d(4097, path=1)[2] == "rn_nn_mfma_kernel"
    assert d(16384, path=2)[3] == "rn_nn_gru_w8_kernel" and d(16385, path=2)[3] == "rn_nn_gru_kernel"
    assert d(256)[4] == "rn_synthesis_few_kernel" and d(257)[4] == "rn_synthesis_kernel"
    assert d(1, whole=0) == ("rn_hp_one_kernel", "rn_analysis_single_kernel", "rn_nn_one_kernel", "rn_nn_gru_w8_kernel", "rn_synthesis_few_kernel")
