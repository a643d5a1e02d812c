"""The Viterbi VAD of training-data generation as device code (rnnoise_batch_train_levels_vad_device), as far
as a machine without a GPU can hold it:

  a  the restated pow and log (rnnoise_amd/csrc/pow_glibc.h) against the running libm, bit for bit, over the VAD's whole domains:
     every float w of [.1f, .9f] and NaN for pow, every finite float energy for log(1e-15 + E), every float from +0 to +Inf for log
  b  tools/extract_glibc_pow_tables.py reproduces the committed data header from this machine's libm
  c  the kernel's own source as host C++ under the address and undefined-behaviour sanitizers (tests/csrc/hip_emul/vad_main.cpp):
     byte-equal to rnnoise_amd_train_vad and tests/csrc/mix_oracle.c at 1 / 2 / 7 / 300 / 2000 frames and 1 / 65 / 130 sequences, and
     to the reference's own viterbi_vad at 2000 frames
  d  the refusals that need no device, the self-check's test hook, the exports, the vad= argument
"""
import ctypes as C
import ctypes.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from rnnoise_amd import capi, train_data
from train_support import T_REF, reference_dump_features, run_kernel_emul

SRC = os.path.join(ROOT, "tests", "csrc", "vad_libm_sweep.c")
_bits = lambda v: int(np.float32(v).view(np.uint32))


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vad_sweep") / "vad_libm_sweep")
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp", "-o", exe, SRC, "-lm"], check=True)

    def run(*args):
        env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
        n, bad, first = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True, env=env).stdout.split()
        return int(n), int(bad), first
    return run


# ---- a. the restated functions against the running libm: zero differences, nothing else ----
def test_pow_half_is_the_hosts_for_every_clamped_float_and_nan(sweep):
    n, bad, first = sweep("pow")
    assert n == _bits(.9) - _bits(.1) + 2   # every float of [.1f, .9f], and NaN
    assert bad == 0, f"{bad} of {n} differ, the last at w = {first}"


def test_log_is_the_hosts_for_every_float_energy(sweep):
    n, bad, first = sweep("loge", 1)
    assert n >= 0x7f800000                  # every finite float >= 0
    assert bad == 0, f"{bad} of {n} differ, the last at E = {first}"


def test_log_is_the_hosts_for_every_float_from_zero_to_inf(sweep):
    n, bad, first = sweep("logf", 1)
    assert n >= 0x7f800001                  # subnormals, zero and Inf among them
    assert bad == 0, f"{bad} of {n} differ, the last at f = {first}"


def test_log_specials_are_the_hosts(sweep):
    n, bad, first = sweep("spec")
    assert n == 11 and bad == 0, first


# ---- b. the generated data header ----
def test_data_header_is_what_the_extraction_tool_reads_out_of_this_libm():
    path = ctypes.util.find_library("m")
    cands = [p for p in ("/lib/x86_64-linux-gnu/libm.so.6", "/usr/lib/x86_64-linux-gnu/libm.so.6", "/lib64/libm.so.6") if os.path.exists(p)]
    assert cands, f"no libm.so.6 found ({path})"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_glibc_pow_tables.py"), cands[0]], check=True,
                         capture_output=True, text=True).stdout
    have = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "pow_glibc_data.h")).read()
    assert out == have
    assert have.count("\n  0x1.") + have.count("\n  0x0.") >= 128 and have.count("ull,") == 256


# ---- c. the kernel source on the host ----
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vad_emul")
    dump = str(tmp / "vad_2000.bin")
    old = os.environ.get("VAD_EMUL_DUMP")
    os.environ["VAD_EMUL_DUMP"] = dump   # (the stand-alone program's own switch: run_kernel_emul passes the environment on)
    try:
        r = run_kernel_emul(tmp, "train_mix", "vad_main.cpp", "mix_oracle.c", [os.path.join(ROOT, "include")])
    finally:
        if old is None:
            del os.environ["VAD_EMUL_DUMP"]
        else:
            os.environ["VAD_EMUL_DUMP"] = old
    return r, dump


def test_kernel_source_on_the_host_stays_inside_its_rows_and_gives_the_host_calls_bytes(emul):
    r, _ = emul
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all equal" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("n=")]
    assert len(lines) == 15 and all(" 0 mismatching blocks" in ln for ln in lines), r.stdout
    for T in (1, 2, 7, 300, 2000):
        assert any(f" T={T} " in ln for ln in lines), T
    for n in (1, 65, 130):
        assert any(ln.startswith(f"n={n} ") for ln in lines), n
    assert sum("null_start=1" in ln for ln in lines) == 2
    # the decoded tracks are not trivial: frames of both kinds at 300 frames and 130 sequences
    active, total = [int(x) for x in [ln for ln in lines if ln.startswith("n=130 T=300 ")][0].split(", ")[1].split(" active frames of ")]
    assert 0 < active < total


def test_kernel_source_on_the_host_is_the_references_viterbi_vad_at_2000_frames(emul, tmp_path_factory):
    r, dump = emul
    assert r.returncode == 0 and os.path.exists(dump)
    ref = reference_dump_features(tmp_path_factory.mktemp("ref_dump_vad"))
    if isinstance(ref, str):
        pytest.skip(ref)
    raw = open(dump, "rb").read()
    n, T = np.frombuffer(raw, np.int32, 2)
    assert (n, T) == (65, T_REF)
    energy = np.frombuffer(raw, np.float32, n * T, 8).reshape(n, T)
    start = np.frombuffer(raw, np.int32, n, 8 + 4 * n * T)
    vad = np.frombuffer(raw, np.uint8, n * T, 8 + 4 * n * T + 4 * n).reshape(n, T)
    assert (energy[1] == 0).all() and (energy[0] > 0).any()              # the silent row and a live one are there
    assert len(np.unique(energy[3])) == 1 and (energy[2] > 0).sum() == 1  # one repeated value; one loud frame
    assert {0, 479, 480}.issubset(set(start.tolist())) and (start > 480 * T).any()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    for s in range(n):
        want = np.zeros(T, np.int32)
        ref.refm_viterbi_vad(np.ascontiguousarray(energy[s]).ctypes.data_as(fp), want.ctypes.data_as(ip))
        want[:min(start[s] // 480, T)] = 0                               # RNN_CLEAR(vad, start_pos / 480)
        assert (vad[s] == want).all(), (s, int(start[s]))


# ---- d. refusals, the self-check and its hook, the surface ----
def test_the_new_calls_are_exported_and_mirrored():
    assert {"rnnoise_amd_train_vad_device_available", "rnnoise_batch_train_levels_vad_device"} <= set(capi.EXPORTS)
    assert hasattr(capi.Batch, "train_levels_vad_device")
    L = capi.lib()
    assert L.rnnoise_amd_train_vad_device_available() in (0, 1)
    assert capi.train_vad_device_available() == bool(L.rnnoise_amd_train_vad_device_available())


def test_this_hosts_libm_passes_the_self_check():
    """(sweeps a: this machine's libm is the restated one, so the library's own short sweep has to say so too)"""
    assert capi.lib().rnnoise_amd_train_vad_device_available() == 1


def test_null_arguments_are_refused():
    L = capi.lib()
    t = np.zeros(1, capi.MIX_DTYPE)
    p = C.c_void_p(16)
    assert L.rnnoise_batch_train_levels_vad_device(None, p, p, p, p, p, p, 4800, 4800, 4800, t.ctypes.data, None, 2, None) == -1


def test_forced_self_check_failure_makes_the_device_form_unavailable():
    with capi.instrumented() as L:
        assert L.rnnoise_amd_train_vad_device_available() == 1
        L.rnnoise_amd_debug_train_vad_selfcheck(0)
        try:
            assert L.rnnoise_amd_train_vad_device_available() == 0 and not capi.train_vad_device_available()
            t = np.zeros(1, capi.MIX_DTYPE)
            p = C.c_void_p(16)
            assert L.rnnoise_batch_train_levels_vad_device(None, p, p, p, p, p, p, 4800, 4800, 4800, t.ctypes.data, None, 2, None) == -1
        finally:
            L.rnnoise_amd_debug_train_vad_selfcheck(-1)
        assert L.rnnoise_amd_train_vad_device_available() == 1
    assert not hasattr(capi.lib(), "rnnoise_amd_debug_train_vad_selfcheck")   # the hook is not in the product


def test_generate_refuses_an_unknown_vad_argument():
    with pytest.raises(ValueError, match="vad="):
        next(train_data.generate_rounds(None, None, None, None, None, 1, vad="gpu"))
