"""CPU checks of the caller-defined PCM layout (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout): declared, exported by the product
libraries and the instrumented one, bound by ctypes and the torch op, NULL batches refused without a GPU; the setter's rule and the
overlap rule of the process calls (rnnoise_amd/csrc/dispatch.h) at their edges; and the kernel forms of a step, which a layout
cannot move."""
import ctypes as C
import os
import re
import subprocess

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_set_pcm_layout", "rnnoise_batch_pcm_layout", "rnnoise_amd_pcm_layout_fits"]


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_libraries_export_them(so):
    names = exported(so, NEW)
    if so != "librnnoise_amd_instr.so":  # the product exports the C API and nothing else: no helper of the layout leaks out
        assert names and all(x.startswith("rnnoise_") for x in names), [x for x in names if not x.startswith("rnnoise_")][:5]
        assert not [x for x in names if "layout" in x and x not in NEW]


def test_ctypes_and_torch_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_set_pcm_layout.argtypes) == 3
    assert len(L.rnnoise_batch_pcm_layout.argtypes) == 3
    assert len(L.rnnoise_amd_pcm_layout_fits.argtypes) == 5
    for m in ("set_pcm_layout", "pcm_array"):
        assert callable(getattr(capi.Batch, m)), m
    assert isinstance(capi.Batch.pcm_layout, property)
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.process_streams)


def test_null_batch_returns_minus_one():
    L = capi.lib()
    f, r = C.c_long(7), C.c_long(7)
    for fs, rs in ((0, 0), (480, 4800), (4, 4), (-4, 8)):
        assert L.rnnoise_batch_set_pcm_layout(None, fs, rs) == -1
    assert L.rnnoise_batch_pcm_layout(None, C.byref(f), C.byref(r)) == -1
    assert (f.value, r.value) == (7, 7)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("layout_dispatch")
    exes = {}
    for name in ("layout_dispatch_test", "dispatch_test"):
        exes[name] = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", name + ".cpp"), "-o",
                        exes[name]], check=True)

    def run(cases, exe="layout_dispatch_test", **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
        env.update({f"RNNOISE_AMD_{k}": str(v) for k, v in knobs.items()})
        return subprocess.run([exes[exe]] + list(cases), capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    return run


def test_setter_rule(prog):
    cases = {(0, 0): 1, (480, 480 * 70): 1, (4, 4): 1, (480 * 70 + 8, 488): 1, (2 ** 40, 2 ** 31 - 4): 1, (80, 2 ** 31): 0,
             (0, 480): 0, (480, 0): 0, (-480, 480): 0, (480, -4): 0, (482, 4800): 0, (480, 4802): 0, (481, 481): 0, (3, 3): 0, (1, 4): 0}
    got = prog([f"ok:{f},{r}" for f, r in cases])
    assert [int(x) for x in got] == list(cases.values()), list(zip(cases, got))


FITS = [
    # (frame_stride, row_stride, M, n_rows, n_frames) -> fits
    # stream-contiguous: frame_stride >= M and row_stride >= n_frames * frame_stride
    ((480, 6 * 480, 480, 70, 6), 1), ((480, 6 * 480 - 4, 480, 70, 6), 0), ((476, 6 * 480, 480, 70, 6), 0), ((484, 6 * 484, 480, 70, 6), 1),
    ((484, 6 * 484 - 4, 480, 70, 6), 0), ((480, 6 * 480, 480, 70, 7), 0), ((480, 6 * 480, 480, 70, 1), 1), ((160, 5 * 160, 160, 2564, 5), 1),
    ((160, 5 * 160 - 4, 160, 2564, 5), 0), ((80, 80, 80, 1, 1), 1), ((80, 20 * 80, 80, 65536, 20), 1),
    # row-major: row_stride >= M and frame_stride >= n_rows * row_stride
    ((70 * 488, 488, 480, 70, 6), 1), ((70 * 488 - 4, 488, 480, 70, 6), 0), ((70 * 480, 480, 480, 70, 6), 1), ((70 * 476, 476, 480, 70, 6), 0),
    ((70 * 488, 488, 480, 71, 6), 0), ((70 * 488, 488, 480, 71, 1), 0),  # (one row too many, however few the frames)
    ((65536 * 480, 480, 480, 65536, 20), 1), ((65536 * 480 - 4, 480, 480, 65536, 20), 0),
    # neither: interleaved slots
    ((480, 480, 480, 2, 2), 0), ((960, 480, 480, 2, 2), 1), ((480, 960, 480, 2, 2), 1), ((484, 480, 480, 2, 2), 0),
    # nothing to place fits; no layout (or a bad one) does not
    ((480, 480, 480, 0, 5), 1), ((480, 480, 480, 5, 0), 1), ((0, 0, 480, 70, 6), 0), ((-480, 4800, 480, 2, 2), 0),
]


def test_overlap_rule(prog):
    got = prog([f"fits:{','.join(map(str, c))}" for c, _ in FITS])
    assert [int(x) for x in got] == [w for _, w in FITS], [(c, g) for (c, w), g in zip(FITS, got) if int(g) != w]


def test_overlap_rule_exported():
    """the same rule through the library (rnnoise_amd_pcm_layout_fits: strides the setter refuses never fit)"""
    L = capi.lib()
    for c, w in FITS:
        assert L.rnnoise_amd_pcm_layout_fits(*c) == w, c
    assert L.rnnoise_amd_pcm_layout_fits(482, 6 * 482, 480, 70, 6) == 0  # (not a multiple of 4)
    assert L.rnnoise_amd_pcm_layout_fits(484, 6 * 484 + 2, 480, 70, 6) == 0


@pytest.mark.parametrize("n", [70, 2048, 2564, 65536])
def test_layout_moves_no_plan(prog, n):
    for pipelined in (0, 1):
        plain = prog([f"plan:{n},256,{pipelined},0,0"])[0]
        for fs, rs in ((480, 20 * 480), (n * 488, 488), (484, 8 * 484)):
            assert prog([f"plan:{n},256,{pipelined},{fs},{rs}"])[0] == plain, (n, fs, rs)
        # ... and it is the plan of the seven-value shape every other dispatch test uses: whole batch, default path, lock-step, 48 kHz
        for knobs in ({}, {"HP_ONE_MAX": 0}):
            path = prog([f"plan:{n},256,{pipelined},0,0"], **knobs)[0]
            assert path == _reference_plan(prog, n, pipelined, **knobs), (n, knobs)


def _reference_plan(prog, n, pipelined, **knobs):
    nn_path = 1 if n > 512 and n >= 16 else 0  # (dispatch.h: rn_default_nn_path at the default switches)
    return prog([f"plan:{n},1,256,{nn_path},{pipelined},0,0"], exe="dispatch_test", **knobs)[0]


def test_kernel_argument_block_keeps_its_size():
    """RnGroupDev::pcm_pitch sits in what was padding behind rs_pitch: every kernel's argument block is as long as before"""
    src = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "rn_dev.h")).read()
    assert re.search(r"int rs_pitch;\n(\s*//[^\n]*\n)+\s*int pcm_pitch;", src)
