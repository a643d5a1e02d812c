"""What the tests of the training units (rnnoise_amd/csrc/train_mix.hip, train_rir.hip) and the test oracles share.  TEST
INFRASTRUCTURE, plain helpers:

  c_library                 a C file compiled once per process into a temporary shared object, loaded with ctypes (the oracles)
  reference_dump_features   the reference's own src/dump_features.c with -DTRAINING=1 behind tests/csrc/ref_dump_harness.c
  run_kernel_emul           a unit's kernels on the host: tests/csrc/hip_emul under the address and undefined-behaviour sanitizers
  guarded, guards_intact    device buffers between guard words (the GPU tests)"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
INCLUDE = os.path.join(ROOT, "include")
REF = os.environ.get("RNNOISE_REFERENCE", "/root/reference")
GEN = os.path.join(ROOT, "oracle", "_ref", "gen_default")
T_REF, NFFT_REF = 2000, 65536   # the reference's SEQUENCE_LENGTH and RIR_FFT_SIZE
GUARD = 64
_libs = {}


def c_library(src, includes=(), flags=(), extra=(), where=None):
    """`src` (and the sources `extra`) as a shared object built with gcc -O2 -ffp-contract=off, once per process, in the directory
    `where` or a temporary one of its own: the CDLL"""
    key = (src, tuple(includes), tuple(flags), tuple(extra))
    if key not in _libs:
        name = os.path.splitext(os.path.basename(src))[0]
        so = os.path.join(str(where) if where else tempfile.mkdtemp(prefix=name), f"lib{name}.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", *flags, *[f"-I{i}" for i in includes], "-o", so, src, *extra,
                        "-lm"], check=True)
        _libs[key] = C.CDLL(so)
    return _libs[key]


def reference_dump_features(where):
    """the reference's functions of both training stages (tests/csrc/ref_dump_harness.c: refm_*, refr_*), with the flags of its pinned
    build (oracle/Makefile: REF_CFLAGS), compiled into the directory `where` once per process; a string saying why not where that
    cannot be done"""
    if not os.path.isdir(os.path.join(REF, "src")):
        return "the reference's sources are not here"
    if not os.path.exists(os.path.join(GEN, "rnnoise_data.h")):
        return "oracle/_ref/gen_default not built (python -c 'import __graft_entry__ as g; g.build()')"
    L = c_library(os.path.join(CSRC, "ref_dump_harness.c"), (GEN, f"{REF}/include", f"{REF}/src", REF),
                  ("-DDISABLE_DEBUG_FLOAT", "-DRNN_ENABLE_X86_RTCD", "-DCPU_INFO_BY_ASM", "-DRNNOISE_BUILD", "-DTRAINING=1",
                   f"-DREF_DUMP_FEATURES_C=\"{REF}/src/dump_features.c\"", "-w"),
                  [os.path.join(REF, "src", f) for f in ("denoise.c", "kiss_fft.c", "pitch.c", "celt_lpc.c", "rnnoise_tables.c")], where)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.refm_biquad.argtypes = [fp, fp, fp, fp, fp, C.c_int]
    L.refm_weighted_rms.argtypes = [fp]
    L.refm_weighted_rms.restype = C.c_float
    L.refm_viterbi_vad.argtypes = [fp, ip]
    L.refm_clear_vad.argtypes = [fp, ip]
    L.refr_tables.argtypes = [fp, ip, ip]
    L.refr_load_rir.argtypes = [C.c_char_p, C.c_int, fp]
    L.refr_filter.argtypes = [fp, fp]
    assert L.refm_sequence_frames() == L.refr_sequence_frames() == T_REF and L.refr_fft_size() == NFFT_REF
    return L


def run_kernel_emul(tmp_path, unit, main_cpp, oracle_c, oracle_includes=()):
    """rnnoise_amd/csrc/<unit>.hip and train_common.h as plain C++ beside tests/csrc/hip_emul/shim.h, linked with the program
    `main_cpp` of that directory and the oracle tests/csrc/<oracle_c>: a stand-alone program under the address and
    undefined-behaviour sanitizers, run once -- the CompletedProcess"""
    emul, csrc = os.path.join(CSRC, "hip_emul"), os.path.join(ROOT, "rnnoise_amd", "csrc")
    for f in ("shim.h", main_cpp):
        shutil.copy(os.path.join(emul, f), tmp_path / f)
    shutil.copy(os.path.join(csrc, "train_common.h"), tmp_path / "train_common.h")
    shutil.copy(os.path.join(csrc, unit + ".hip"), tmp_path / (unit + ".cpp"))
    obj = str(tmp_path / "oracle.o")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", *[f"-I{i}" for i in oracle_includes], "-c", os.path.join(CSRC, oracle_c), "-o", obj],
                   check=True)
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-w", "-I", str(tmp_path), "-I", INCLUDE, str(tmp_path / (unit + ".cpp")), str(tmp_path / main_cpp), obj, "-o",
                    str(tmp_path / "emul"), "-lpthread", "-lm"], check=True)
    return subprocess.run([str(tmp_path / "emul")], capture_output=True, text=True)


def guarded(shape, dtype=None, fill=None):
    """a buffer of `shape` on cuda:0 between GUARD guard words on both sides: (whole, view, fill)"""
    import torch
    dtype = dtype or torch.float32
    if fill is None:
        fill = {torch.float32: -7.5e33, torch.int32: -77777777, torch.uint8: 0xA5}[dtype]
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return buf, buf[GUARD:GUARD + n].view(*shape), fill


def guards_intact(buf, fill, what):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == h.dtype.type(fill)).all() and (h[-GUARD:] == h.dtype.type(fill)).all(), f"{what}: a guard word was written"
