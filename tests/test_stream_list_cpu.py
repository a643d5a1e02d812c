"""CPU checks of the stream-list calls (include/rnnoise_amd.h: rnnoise_batch_process_*list*): declared, exported by both product
libraries, bound by ctypes and the torch op, NULL batches refused without a GPU -- and the kernel forms of a list step
(rnnoise_amd/csrc/dispatch.h: RnStepShape::listed) pinned at the batch sizes of every regime, with the plans of every other step
unchanged."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_process_device_list", "rnnoise_batch_process_device_list_s16", "rnnoise_batch_process_list",
       "rnnoise_batch_process_list_s16"]


def test_prototypes_declared_once_each_with_export():
    declared_once(NEW)


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_both_product_libraries_export_them(so):
    exported(so, NEW)


def test_ctypes_and_torch_bindings():
    L = capi.lib()
    for n in NEW:
        assert getattr(L, n).argtypes, n
    assert len(L.rnnoise_batch_process_device_list.argtypes) == 10
    assert len(L.rnnoise_batch_process_device_list_s16.argtypes) == 10
    assert len(L.rnnoise_batch_process_list.argtypes) == 9
    assert len(L.rnnoise_batch_process_list_s16.argtypes) == 9
    for m in ("process_list", "process_list_s16", "process_list_device"):
        assert callable(getattr(capi.Batch, m)), m
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.process_list)


def test_null_batch_and_bad_counts_return_minus_one():
    L = capi.lib()
    buf, sbuf = (C.c_float * 480)(), (C.c_short * 480)()
    idx = (C.c_int * 1)(0)
    for n_rows in (1, 0, -1):
        assert L.rnnoise_batch_process_list(None, buf, buf, None, None, idx, n_rows, None, 1) == -1
        assert L.rnnoise_batch_process_list_s16(None, sbuf, sbuf, None, None, idx, n_rows, None, 1) == -1
        assert L.rnnoise_batch_process_device_list(None, None, None, None, None, None, n_rows, None, 1, None) == -1
        assert L.rnnoise_batch_process_device_list_s16(None, None, None, None, None, None, n_rows, None, 1, None) == -1


# ---- the forms of a list step ----
@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("list_dispatch")
    exes = {}
    for name in ("list_dispatch_test", "dispatch_test"):
        exes[name] = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", name + ".cpp"), "-o",
                        exes[name]], check=True)

    def run(cases, exe="list_dispatch_test", **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
        env.update({f"RNNOISE_AMD_{k}": str(v) for k, v in knobs.items()})
        return subprocess.run([exes[exe]] + list(cases), capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    return run


def list_plan(prog, batch, rows, pipelined=False, low_rate=False, cus=256, **knobs):
    return tuple(prog([f"list:{batch},{rows},{cus},{int(pipelined)},{int(low_rate)}"], **knobs)[0].split())


ROWS = {300: (1, 37, 256, 257, 300), 4096: (1, 256, 257, 1000, 4096), 20480: (1, 3000, 4096, 4097, 20480),
        65536: (1, 512, 4096, 8192, 16384, 65536)}


@pytest.mark.parametrize("batch", sorted(ROWS))
def test_list_step_forms(prog, batch):
    for rows, pipelined, low_rate in itertools.product(ROWS[batch], (False, True), (False, True)):
        hp, k1, nn, _, k3 = list_plan(prog, batch, rows, pipelined, low_rate)
        assert hp == "rn_hp_one_kernel", (batch, rows)  # one wave per listed stream: the form with the resampling prologue
        assert k1 == "rn_analysis_single_kernel", (batch, rows)
        assert nn != "layers" and nn != "rn_nn_vector_kernel", (batch, rows)
        if batch == 300:  # a batch on network path 0: the per-stream network kernel at every number of rows
            assert nn == "rn_nn_one_kernel", (batch, rows)
        else:  # paths 1 and 2: the tile kernel over the tiles of the listed rows, its form by their number
            tiles = (rows + 15) // 16
            assert nn == ("rn_nn_mfma16_kernel" if not pipelined and tiles <= 256 else "rn_nn_mfma_kernel"), (batch, rows, pipelined)
        assert k3 == ("rn_synthesis_few_kernel" if rows <= 256 else "rn_synthesis_kernel"), (batch, rows)


def test_list_step_never_layer_wise_even_when_forced(prog):
    for batch, rows, nn in ((20480, 3000, "rn_nn_mfma16_kernel"), (20480, 20480, "rn_nn_mfma_kernel"), (65536, 65536, "rn_nn_mfma_kernel")):
        assert list_plan(prog, batch, rows, NN_LAYERS_MIN=16)[2] == nn, (batch, rows)
    # the switches that pick among tile forms and K0 / K1 forms still apply where they are forms a list step has
    assert list_plan(prog, 65536, 512, TILE_WAVES=8)[2] == "rn_nn_mfma_kernel"
    assert list_plan(prog, 65536, 8192, pipelined=True, TILE_WAVES=16)[2] == "rn_nn_mfma16_kernel"
    assert list_plan(prog, 65536, 8192, HP_ONE_MAX=0, K1_SPW=4)[:2] == ("rn_hp_one_kernel", "rn_analysis_single_kernel")


def test_plans_of_other_steps_unchanged(prog):
    """the library's rules for a step that is no list call, through a shape that leaves `listed` at its default, give the same forms
    as the seven-value shape of tests/csrc/dispatch_test.cpp everywhere on a grid over every field"""
    cases = [f"plan:{n},{w},{c},{p},{pl},{ps},{lr}" for n, w, c, p, pl, ps, lr in itertools.product(
        (1, 256, 257, 300, 512, 513, 2048, 2049, 2559, 2560, 4096, 4097, 10239, 10240, 20480, 65536), (0, 1), (80, 256), (0, 1, 2),
        (0, 1), (0, 1), (0, 1))]
    for knobs in ({}, {"NN_LAYERS_MIN": 4096, "TILE_WAVES": 8, "K1_SPW": 1}):
        assert prog(cases, **knobs) == prog(cases, exe="dispatch_test", **knobs)
