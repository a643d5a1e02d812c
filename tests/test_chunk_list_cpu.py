"""CPU checks of the chunk calls on a stream list and of the FIFO records (include/rnnoise_amd.h:
rnnoise_batch_process_device_chunks_list, rnnoise_batch_save_chunk_fifos and their siblings): the list and record bodies of
rnnoise_amd/csrc/chunk_fifo.h as a stand-alone host program under AddressSanitizer and UBSan, lane after lane between the barriers,
against two deques per stream (tests/csrc/chunk_list_test.cpp); and the C ABI -- declared, exported, bound, and refusing a NULL batch
without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

CALLS = ["rnnoise_batch_process_device_chunks_list", "rnnoise_batch_process_device_chunks_list_s16",
         "rnnoise_batch_process_chunks_list", "rnnoise_batch_process_chunks_list_s16"]
RECORDS = ["rnnoise_batch_save_chunk_fifos_device", "rnnoise_batch_load_chunk_fifos_device", "rnnoise_batch_save_chunk_fifos",
           "rnnoise_batch_load_chunk_fifos"]
NEW = CALLS + RECORDS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    # a program with its own main, linked against the sanitizers' runtimes the ordinary way: nothing is preloaded
    out = str(tmp_path_factory.mktemp("chunk_list") / "chunk_list_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "csrc", "chunk_list_test.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("M,max_count", [(480, 1024), (480, 441), (160, 441), (80, 1)])
@pytest.mark.parametrize("s16,alias", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("mode", ["list", "mixed"])
def test_the_list_bodies_against_two_deques(exe, mode, lanes, M, max_count, s16, alias):
    """7 streams, 40 calls, lists of 0 to 5 rows in shuffled order, some naming an entry outside the batch: staged frames, mask and
    frames[] by row, both tails and the fill by stream, the popped output, the bytes of `out` behind each count and every byte of an
    absent row, and after every call the records of the unlisted streams byte for byte -- float and int16, `in` aliasing `out`.
    mixed: every third call goes through the full-size bodies on the same FIFOs"""
    r = subprocess.run([exe, mode, str(lanes), str(M), str(max_count), str(s16), str(alias)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    ok, calls, frames, absent = r.stdout.split()
    assert ok == "ok" and int(calls) == 40 and int(absent) >= 3
    if max_count >= 441:
        assert int(frames) >= 30  # (the run did complete frames)


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("M", [480, 320, 160, 80])
def test_the_record_bodies(exe, lanes, M):
    """save -> load into another stream index gives back the FIFOs and the fill, NaN payloads included; a saved record is zero outside
    its valid ranges and two saves are equal bytes; save leaves the batch alone and marks an entry outside it with magic 0; a batch
    without FIFOs saves restarted records; load refuses and touches nothing on another magic word, another M, r = -1 and r = M"""
    r = subprocess.run([exe, "records", str(lanes), str(M)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.split() == ["ok"]


def test_prototypes_declared_once_each_with_export():
    src = declared_once(NEW)
    assert re.search(r"#define\s+RNNOISE_AMD_CHUNK_REC_FLOATS\s+964\b", src)
    magic = re.search(r"#define\s+RNNOISE_AMD_CHUNK_MAGIC\s+(0x[0-9a-fA-F]+)", src)
    assert magic and int(magic.group(1), 16) == capi.CHUNK_MAGIC != capi.SNAP_MAGIC
    assert capi.CHUNK_REC_FLOATS == 964 and capi.CHUNK_OFF_FILL == 960 and capi.CHUNK_OFF_M == 961 and capi.CHUNK_OFF_MAGIC == 962


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_both_product_libraries_export_them(so):
    exported(so, NEW)


def test_a_null_batch_returns_minus_one_without_a_gpu():
    L = capi.lib()
    f = (C.c_float * 8)()
    s = (C.c_short * 8)()
    n = (C.c_int * 2)(1, 1)
    idx = (C.c_int * 2)(0, 1)
    for max_count in (4, 0, -1):
        for rows in (2, 0, -1):
            assert L.rnnoise_batch_process_chunks_list(None, f, f, n, max_count, idx, rows, None, None, None) == -1
            assert L.rnnoise_batch_process_chunks_list_s16(None, s, s, n, max_count, idx, rows, None, None, None) == -1
            assert L.rnnoise_batch_process_chunks_list(None, f, f, n, max_count, None, rows, None, None, None) == -1
            assert L.rnnoise_batch_process_device_chunks_list(None, None, None, None, max_count, None, rows, None, None, None, None) == -1
            assert L.rnnoise_batch_process_device_chunks_list_s16(None, None, None, None, max_count, None, rows, None, None, None, None) == -1
    rec = (C.c_float * (2 * capi.CHUNK_REC_FLOATS))()
    for rows in (2, 0, -1):
        assert L.rnnoise_batch_save_chunk_fifos(None, rec, idx, rows) == -1
        assert L.rnnoise_batch_load_chunk_fifos(None, rec, idx, rows) == -1
        assert L.rnnoise_batch_save_chunk_fifos_device(None, None, None, rows, None) == -1
        assert L.rnnoise_batch_load_chunk_fifos_device(None, None, None, rows, None) == -1


def test_ctypes_capi_and_torch_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_process_chunks_list.argtypes) == 10 and len(L.rnnoise_batch_process_chunks_list_s16.argtypes) == 10
    assert len(L.rnnoise_batch_process_device_chunks_list.argtypes) == 11
    assert len(L.rnnoise_batch_process_device_chunks_list_s16.argtypes) == 11
    assert len(L.rnnoise_batch_save_chunk_fifos.argtypes) == 4 and len(L.rnnoise_batch_load_chunk_fifos.argtypes) == 4
    assert len(L.rnnoise_batch_save_chunk_fifos_device.argtypes) == 5 and len(L.rnnoise_batch_load_chunk_fifos_device.argtypes) == 5
    for m in ("process_chunks_list", "process_chunks_list_s16", "process_chunks_list_device", "save_chunk_fifos", "load_chunk_fifos",
              "save_chunk_fifos_device", "load_chunk_fifos_device"):
        assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import torch_op
    for m in ("process_chunks_list", "save_chunk_fifos", "load_chunk_fifos"):
        assert callable(getattr(torch_op.RNNoiseOp, m)), m


def test_the_new_work_is_further_cases_of_the_chunk_launch():
    """no kernel and no record kind of its own: the list and record bodies live in the header that names no __global__ function,
    the two state kernels call them, and RnChunkDev's first fields -- what a state launch reads -- are where they were"""
    csrc = os.path.join(ROOT, "rnnoise_amd", "csrc")
    for h in ("chunk_plan.h", "chunk_fifo.h"):
        text = open(os.path.join(csrc, h)).read()
        assert "__global__" not in text and "hip_runtime" not in text and not re.search(r"\basm\b", text), h
    src = open(os.path.join(csrc, "state_kernels.hip")).read()
    for body in ("rn_chunk_list_scatter_frames", "rn_chunk_list_scatter_tail", "rn_chunk_list_gather_pop", "rn_chunk_list_gather_keep",
                 "rn_chunk_rec_save", "rn_chunk_rec_load"):
        assert body in src, body
    assert len(re.findall(r"__global__", src)) == 3  # gather, scatter, the release store
    plan = open(os.path.join(csrc, "chunk_plan.h")).read()
    fields = re.search(r"struct RnChunkDev \{(.*?)\n\};", plan, re.S).group(1)
    names = re.findall(r"(\w+);", fields)
    assert names[:2] == ["fifo", "M"] and names[-4:] == ["list", "S", "op", "rec"], names
