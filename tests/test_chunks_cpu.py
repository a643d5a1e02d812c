"""CPU checks of the chunk calls (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks and its siblings): the push rule of
rnnoise_amd/csrc/chunk_plan.h at every fill and count; the two staging bodies of rnnoise_amd/csrc/chunk_fifo.h as a stand-alone host
program under AddressSanitizer and UBSan, lane after lane between the barriers, against two deques per stream; and the C ABI --
declared, exported, bound, and refusing bad arguments without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_amd_chunk_frames", "rnnoise_batch_process_device_chunks", "rnnoise_batch_process_device_chunks_s16",
       "rnnoise_batch_process_chunks", "rnnoise_batch_process_chunks_s16", "rnnoise_batch_chunk_fill"]
FRAMES = (80, 160, 240, 320, 480)


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "csrc", f"{name}.cpp"),
                    "-o", exe], check=True)
    return exe


def test_the_push_rule_at_every_fill_and_count(tmp_path):
    """for M in 80, 160, 240, 320, 480, every r in [0, M) and every n in [0, 2M + 1]: k and the new fill as counting gives them,
    out_fill = M - in_fill, at least n samples to pop, k within rnnoise_amd_chunk_frames(M, n) (tests/csrc/chunk_plan_test.cpp)"""
    exe = _build(tmp_path, "chunk_plan_test")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == sum(M * (2 * M + 2) for M in FRAMES)


@pytest.fixture(scope="module")
def fifo_exe(tmp_path_factory):
    # a program with its own main, linked against the sanitizers' runtimes the ordinary way: nothing is preloaded
    return _build(tmp_path_factory.mktemp("chunk_fifo"), "chunk_fifo_test", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("M,max_count", [(480, 1024), (480, 441), (480, 128), (320, 1023), (240, 441), (160, 441), (80, 128), (80, 1)])
@pytest.mark.parametrize("s16,alias", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_the_staging_bodies_against_two_deques(fifo_exe, lanes, M, max_count, s16, alias):
    """3 streams, 40 pushes, counts from a fixed seed (zero, everything, up to a frame boundary and one sample either side of it among
    them): staged frames, mask, frames[], both tails, the fill, the popped output and the samples behind the count -- float and
    int16, `in` aliasing `out`, odd row lengths (441, 1023)"""
    r = subprocess.run([fifo_exe, str(lanes), str(M), str(max_count), str(s16), str(alias)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    ok, pushes, frames = r.stdout.split()
    assert ok == "ok" and int(pushes) == 40
    if max_count >= 128:
        assert int(frames) >= 3  # (the run did complete frames)


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_both_product_libraries_export_them(so):
    exported(so, NEW)


def test_chunk_frames():
    L = capi.lib()
    assert [L.rnnoise_amd_chunk_frames(480, n) for n in (0, 1, 480, 481, 1024)] == [0, 1, 1, 2, 3]
    for M in FRAMES:  # a FIFO of M - 1 samples and max_count more
        for n in (0, 1, M - 1, M, M + 1, 2 * M, 2 * M + 1, 65536):
            assert L.rnnoise_amd_chunk_frames(M, n) == (M - 1 + n) // M == capi.chunk_frames(M, n)
    assert L.rnnoise_amd_chunk_frames(480, 2**31 - 1) == (479 + 2**31 - 1) // 480  # (no 32-bit overflow on the way)
    for M, n in ((0, 10), (-480, 10), (480, -1), (0, 0)):
        assert L.rnnoise_amd_chunk_frames(M, n) == -1
        with pytest.raises(ValueError):
            capi.chunk_frames(M, n)


def test_a_null_batch_returns_minus_one_without_a_gpu():
    L = capi.lib()
    f = (C.c_float * 8)()
    s = (C.c_short * 8)()
    n = (C.c_int * 2)(1, 1)
    for max_count in (4, 0, -1):
        assert L.rnnoise_batch_process_chunks(None, f, f, n, max_count, None, None, None) == -1
        assert L.rnnoise_batch_process_chunks_s16(None, s, s, n, max_count, None, None, None) == -1
        assert L.rnnoise_batch_process_device_chunks(None, None, None, None, max_count, None, None, None, None) == -1
        assert L.rnnoise_batch_process_device_chunks_s16(None, None, None, None, max_count, None, None, None, None) == -1
    assert L.rnnoise_batch_chunk_fill(None, n) == -1


def test_ctypes_capi_and_torch_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_process_chunks.argtypes) == 8 and len(L.rnnoise_batch_process_chunks_s16.argtypes) == 8
    assert len(L.rnnoise_batch_process_device_chunks.argtypes) == 9 and len(L.rnnoise_batch_process_device_chunks_s16.argtypes) == 9
    for m in ("process_chunks", "process_chunks_s16", "process_chunks_device", "chunk_fill"):
        assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.process_chunks)


def test_the_chunk_code_is_a_record_kind_of_the_two_state_kernels():
    """no kernel of its own: the bodies live in a header that names no __global__ function, and the state kernels call them"""
    csrc = os.path.join(ROOT, "rnnoise_amd", "csrc")
    for h in ("chunk_plan.h", "chunk_fifo.h"):
        text = open(os.path.join(csrc, h)).read()
        assert "__global__" not in text and "hip_runtime" not in text, h
    src = open(os.path.join(csrc, "state_kernels.hip")).read()
    for body in ("rn_chunk_scatter_frames", "rn_chunk_scatter_tail", "rn_chunk_gather_pop", "rn_chunk_gather_keep", "rn_chunk_restart"):
        assert body in src, body
    dev = open(os.path.join(csrc, "rn_dev.h")).read()
    assert re.search(r"enum RnRecKind \{ RN_REC_STATE, RN_REC_SNAP, RN_REC_CHUNK \}", dev)
