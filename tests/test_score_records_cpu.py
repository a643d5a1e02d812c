"""The score calls without a GPU (include/rnnoise_amd.h: rnnoise_batch_score_records[_device], rnnoise_amd_score_records_check;
DESIGN 4.30): the symbols declared, exported and bound; the check at its boundaries; NULL refusals."""
import ctypes as C
import os
import re

from conftest import ROOT
from rnnoise_amd import capi

NAMES = ("rnnoise_amd_score_records_check", "rnnoise_batch_score_records_device", "rnnoise_batch_score_records")


def ok(n, t0, T, rec=(0, 0), gains=(0, 0), vad=(0, 0), gamma=None, first=None):
    return capi.score_records_check(n, t0, T, rec, gains, vad, gamma, first)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(r"RNNOISE_EXPORT int " + name + r"\(", header), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert len(L.rnnoise_amd_score_records_check.argtypes) == 10
    assert len(L.rnnoise_batch_score_records_device.argtypes) == 17 and len(L.rnnoise_batch_score_records.argtypes) == 16
    for name in ("score_records", "score_records_device"):
        assert callable(getattr(capi.Batch, name)), name
    # the fourth step mode sits beside the other three, in the kernel the other three run in
    dev = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "rn_dev.h")).read()
    assert re.search(r"RN_STEP_EVAL = 1, RN_STEP_EXPORT = 2, RN_STEP_IMPORT = 3, RN_STEP_SCORE = 4", dev)
    src = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "dsp_kernels.hip")).read()
    assert "score_rows_body(tr.score)" in src and src.count("eval_frame_terms(") == 3  # one definition, two users: shared, not restated


def test_check_config_boundaries():
    assert ok(5, 0, 12) and ok(5, 0, 12, gamma=0.25, first=4) and ok(5, 0, 12, gamma=1e-3, first=0) and ok(5, 0, 12, gamma=3.0, first=1000)
    for gamma in (0.0, -0.25, float("nan"), float("inf")):
        assert not ok(5, 0, 12, gamma=gamma, first=4), gamma
    assert not ok(5, 0, 12, gamma=0.25, first=-1)
    L = capi.lib()
    z = (0,) * 6
    assert L.rnnoise_amd_score_records_check(C.byref(capi.EvalConfig(0.0, 0)), *z, 5, 0, 12) == 1
    assert L.rnnoise_amd_score_records_check(C.byref(capi.EvalConfig(0.0, 1)), *z, 5, 0, 12) == 0
    assert L.rnnoise_amd_score_records_check(None, *z, 5, 0, 12) == 1


def test_check_rows_and_frames():
    assert ok(1, 0, 1) and ok(5, 0, 0) and ok(5, 7, 0) and ok(65536, 4, 1996)
    assert not ok(0, 0, 12) and not ok(-3, 0, 12) and not ok(5, -1, 12) and not ok(5, 0, -1)
    assert ok(5, 2 ** 31 - 13, 12) and not ok(5, 2 ** 31 - 12, 12)   # t0 + n_frames stays an int


def test_check_layouts_of_each_buffer():
    n, t0, k = 7, 4, 8
    T = t0 + k
    # records: n x (t0 + n_frames) slots of 98 from record 0, in both layouts, padded or not; no multiple of anything
    assert ok(n, t0, k, rec=(n * 98, 98)) and ok(n, t0, k, rec=(n * 101 + 1, 101)) and ok(n, t0, k, rec=(98, T * 98))
    assert not ok(n, t0, k, rec=(n * 98, 97)) and not ok(n, t0, k, rec=(n * 98 - 1, 98))
    assert not ok(n, t0, k, rec=(97, T * 98)) and not ok(n, t0, k, rec=(98, T * 98 - 1))
    assert not ok(n, t0, k, rec=(98, k * 98))                       # the rows are T records long, whatever t0
    # gains: n x n_frames slots of 32 from the call's first step
    assert ok(n, t0, k, gains=(n * 32, 32)) and ok(n, t0, k, gains=(32, k * 32)) and ok(n, t0, k, gains=(40, k * 40 + 3))
    assert not ok(n, t0, k, gains=(n * 32, 31)) and not ok(n, t0, k, gains=(n * 32 - 1, 32))
    assert not ok(n, t0, k, gains=(31, k * 32)) and not ok(n, t0, k, gains=(32, k * 32 - 1))
    # vad: slots of one float
    assert ok(n, t0, k, vad=(n, 1)) and ok(n, t0, k, vad=(1, k)) and ok(n, t0, k, vad=(3, 3 * k))
    assert not ok(n, t0, k, vad=(n - 1, 1)) and not ok(n, t0, k, vad=(1, k - 1))
    # half a layout, negative strides: in any of the three
    for which in ("rec", "gains", "vad"):
        for pair in ((0, 200), (2000, 0), (-2000, 200), (2000, -200)):
            assert not ok(n, t0, k, **{which: pair}), (which, pair)
    # the trainer's shapes: 65,536 sequences of 2,000 records, the float network's [n][T - 4] outputs
    assert ok(65536, 4, 1996, rec=(98, 2000 * 98), gains=(32, 1996 * 32), vad=(1, 1996))


def test_calls_refuse_null_arguments_without_a_gpu():
    L = capi.lib()
    p = C.c_void_p(256)
    assert L.rnnoise_batch_score_records_device(None, p, None, p, 0, 0, p, 0, 0, p, 0, 0, 1, 0, 1, None, None) == -1
    assert L.rnnoise_batch_score_records(None, None, None, None, 0, 0, None, 0, 0, None, 0, 0, 1, 0, 1, None) == -1
