"""CPU checks of the per-stream output tables (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates, _out_formats, their device
forms and read-backs): declared once, exported by the product libraries and the instrumented one, bound by ctypes, capi.Batch and the
torch op; bad arguments refused without a GPU; the record word of include/rn_layout.h; the Hz -> code conversion of capi.Batch; the
plan of a batch with output tables (rnnoise_amd/csrc/dispatch.h: RnStepShape::split) under the sanitizers; and the header `cli
denoise --out-rate 8000 --out-format ulaw` writes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi, cli, wav

NEW = ["rnnoise_batch_set_stream_out_rates", "rnnoise_batch_set_stream_out_rates_device", "rnnoise_batch_stream_out_rates",
       "rnnoise_batch_set_stream_out_formats", "rnnoise_batch_set_stream_out_formats_device", "rnnoise_batch_stream_out_formats"]


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_the_product_libraries_and_the_instrumented_one_export_them(so):
    exported(so, NEW)


def test_ctypes_capi_and_torch_bindings():
    L = capi.lib()
    for kind in ("rates", "formats"):
        assert len(getattr(L, f"rnnoise_batch_set_stream_out_{kind}").argtypes) == 2
        assert len(getattr(L, f"rnnoise_batch_set_stream_out_{kind}_device").argtypes) == 3
        assert len(getattr(L, f"rnnoise_batch_stream_out_{kind}").argtypes) == 2
        for m in (f"set_stream_out_{kind}", f"set_stream_out_{kind}_device", f"stream_out_{kind}"):
            assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.set_stream_out_rates) and callable(torch_op.RNNoiseOp.set_stream_out_formats)


def test_bad_arguments_return_minus_one_without_a_gpu():
    L = capi.lib()
    buf = (C.c_ubyte * 4)(1, 2, 3, 6)
    for kind in ("rates", "formats"):
        setter, dev, getter = (getattr(L, f"rnnoise_batch_{n}") for n in (f"set_stream_out_{kind}", f"set_stream_out_{kind}_device", f"stream_out_{kind}"))
        assert setter(None, buf) == -1 and setter(None, None) == -1
        assert dev(None, None, None) == -1 and dev(None, C.cast(buf, C.c_void_p), None) == -1
        assert getter(None, buf) == -1 and getter(None, None) == -1
    assert list(buf) == [1, 2, 3, 6]
    # (a batch needs a GPU: a NULL buffer on a real batch, and entries a batch refuses, are in tests/test_out_tables_gpu.py)


def _define(src, name):
    m = re.search(rf"#define\s+{name}\s+(.+?)\s*(/\*|$)", src, re.M)
    assert m, name
    return m.group(1).strip()


def test_the_header_constants_match():
    layout = open(os.path.join(ROOT, "include", "rn_layout.h")).read()
    api = open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    # the output code is the first of the three reserved words; the record keeps its size
    assert _define(layout, "RN_SNAP_OFF_OUT_L") == "RN_SNAP_OFF_RESERVED"
    assert _define(layout, "RN_SNAP_OFF_RESERVED") == "(RN_SNAP_OFF_MAGIC + 3)"
    assert _define(layout, "RN_SNAP_OFF_HIST") == "(RN_SNAP_OFF_MAGIC + 6)"
    assert capi.SNAP_OFF_OUT_L == capi.SNAP_OFF_RESERVED == capi.SNAP_OFF_MAGIC + 3 and capi.SNAP_FLOATS == 6624
    # the codes of the out tables are the codes of the rate and format tables
    assert int(_define(api, "RNNOISE_AMD_RATE_32K")) == capi.RATE_32K == 32
    from rnnoise_amd import g711
    assert [int(_define(api, f"RNNOISE_AMD_PCM_{n}")) for n in ("LINEAR", "ULAW", "ALAW")] == [g711.LINEAR, g711.ULAW, g711.ALAW] == [0, 1, 2]
    # the down half of a history starts where the kernels and the setters cut it
    dev = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "rn_dev.h")).read()
    assert int(_define(dev, "RN_RS_DOWN0")) == 48 and int(_define(layout, "RN_SNAP_HIST_FLOATS")) == capi.SNAP_HIST_FLOATS == 336


class _FakeLib:
    """the C entry points as recorders: capi.Batch must validate and convert before it gets here"""

    def __init__(self):
        self.calls = []

    def rnnoise_batch_set_stream_out_rates(self, h, p):
        self.calls.append(("rates", None if p is None else [p[i] for i in range(4)]))
        return 0

    def rnnoise_batch_set_stream_out_formats(self, h, p):
        self.calls.append(("formats", None if p is None else [p[i] for i in range(4)]))
        return 0

    def rnnoise_batch_pcm_rate(self, h):
        return self.rate


def _fake_batch(rate, n=4):
    b = capi.Batch.__new__(capi.Batch)
    b._L, b.h, b.n = _FakeLib(), 1, n
    b._L.rate = rate
    return b


def test_capi_converts_hz_and_names_and_refuses_what_the_batch_cannot_take():
    b = _fake_batch(48000)
    b.set_stream_out_rates([48000, 32000, 16000, 8000])
    assert b._L.calls == [("rates", [1, 32, 3, 6])]
    b.set_stream_out_rates(None)
    assert b._L.calls[-1] == ("rates", None)
    for bad in ([48000, 44100, 16000, 8000], [48000, 0, 16000, 8000], [48000, 12000, 16000, 8000]):
        with pytest.raises(ValueError):
            b.set_stream_out_rates(bad)
    b.set_stream_out_formats(["s16", "ulaw", "alaw", "s16"])
    assert b._L.calls[-1] == ("formats", [0, 1, 2, 0])
    b.set_stream_out_formats(np.array([2, 1, 0, 0]))
    assert b._L.calls[-1] == ("formats", [2, 1, 0, 0])
    b.set_stream_out_formats(None)
    assert b._L.calls[-1] == ("formats", None)
    for bad in (["s16", "mulaw", "alaw", "s16"], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            b.set_stream_out_formats(bad)
    assert len(b._L.calls) == 5
    low = _fake_batch(16000)
    low.set_stream_out_rates(np.array([16000, 8000, 8000, 16000]))
    assert low._L.calls == [("rates", [3, 6, 6, 3])]
    for bad in ([48000, 16000, 16000, 16000], [16000, 32000, 8000, 8000]):  # above the batch's rate: the frame would not fit the row
        with pytest.raises(ValueError):
            low.set_stream_out_rates(bad)
    assert len(low._L.calls) == 1
    b.h = None  # (nothing to destroy)
    low.h = None


def test_the_plan_of_a_batch_with_output_tables_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "out_tables_dispatch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "out_tables_dispatch_test.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) shapes, (\d+) out-only plans with the lane high-pass, 0 failures\n", r.stdout)
    assert m and int(m.group(1)) > 50000 and int(m.group(2)) > 1000, r.stdout


def test_the_header_cli_denoise_writes_for_out_rate_8000_and_out_format_ulaw(tmp_path):
    src = wav.WavInfo(48000, 2, "s16", False, 44, 0)
    info = cli.out_info(src, 8000, "ulaw")
    assert (info.rate, info.channels, info.codec, info.block) == (8000, 2, "ulaw", 2)
    assert cli.out_info(src, None, None) == src and cli.out_info(src, 16000, None).codec == "s16" and cli.out_info(src, None, "alaw").rate == 48000
    frames, data = 5, 5 * 80 * info.block
    path = tmp_path / "o.wav"
    path.write_bytes(wav.header(info, data) + bytes(data))
    back = wav.read_info(str(path))
    assert (back.rate, back.channels, back.codec, back.data_bytes) == (8000, 2, "ulaw", frames * 80 * 2)
    h = path.read_bytes()
    assert h[20:22] == (7).to_bytes(2, "little") and h[24:28] == (8000).to_bytes(4, "little")  # wFormatTag mu-law; samples per second
    # the command line takes the two options and keeps their values in range
    with pytest.raises(SystemExit):
        cli.main(["denoise", "--model", "m", "--out-dir", "o", "--out-rate", "44100", "x.raw"])
    with pytest.raises(SystemExit):
        cli.main(["denoise", "--model", "m", "--out-dir", "o", "--out-format", "g722", "x.raw"])
