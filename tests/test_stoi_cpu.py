"""CPU checks of the STOI library (include/rnnoise_amd_stoi.h, rnnoise_amd/csrc/stoi/, rnnoise_amd/stoi.py): the numpy restatement of
its definition (tests/stoi_ref.py) on its own; the committed tables against their design; what the library declares, exports and
refuses; that it shares nothing with the other libraries; its host-only half as a program under the address and undefined-behaviour
sanitizers; metrics() on hand-made results; and the eval-audio command's new flag.  (The kernels: tests/test_stoi_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stoi_ref as R
from rnnoise_amd import cli
from rnnoise_amd import stoi as S
from rnnoise_amd import stoi_tables as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
HEADER = os.path.join(ROOT, "include", "rnnoise_amd_stoi.h")
T = 120


@pytest.fixture(scope="module")
def graded():
    """one signal, itself and its three degraded versions scored by the reference"""
    clean = R.make_signal(0, T)
    ref10 = R.resample(clean)
    rows = {snr: R.score_row(clean, clean if snr is None else R.degrade(clean, snr, 100), ref10=ref10) for snr in (None, 20, 5, -5)}
    return clean, ref10, rows


# ---- the reference on its own ----
def test_identical_signals_score_one(graded):
    g = graded[2][None]
    assert g["segments"] == g["K"] - 30 > 5 and g["margin"] > 1e-6
    assert abs(g["stoi"] / g["segments"] - 1) < 1e-12 and abs(g["estoi"] / g["segments"] - 1) < 1e-12


def test_both_measures_fall_with_the_noise(graded):
    rows = graded[2]
    for key in ("stoi", "estoi"):
        v = [rows[snr][key] / rows[snr]["segments"] for snr in (None, 20, 5, -5)]
        assert v[0] > v[1] > v[2] > v[3] > 0, (key, v)
    assert rows[5]["K"] == rows[None]["K"]  # the kept frames are the clean signal's


def test_stoi_does_not_depend_on_the_level_of_the_degraded_signal(graded):
    clean, ref10, rows = graded
    quiet = 0.25 * R.degrade(clean, 5, 100).astype(np.float64)
    g = R.score_row(clean, quiet, ref10=ref10)
    assert abs(g["stoi"] - rows[5]["stoi"]) / g["segments"] < 1e-9


def test_the_other_orders_give_the_same_numbers(graded):
    clean, ref10, rows = graded
    g = R.score_row(clean, R.degrade(clean, 5, 100), "dft", True, ref10=ref10)
    assert g["segments"] == rows[5]["segments"]
    assert abs(g["stoi"] - rows[5]["stoi"]) < 1e-12 and abs(g["estoi"] - rows[5]["estoi"]) < 1e-12


def test_short_and_silent_rows():
    g = R.score_row(*[R.make_signal(1, 45)] * 2)
    assert 0 < g["K"] < 31 and g["segments"] == 0 and g["stoi"] == 0.0 and g["estoi"] == 0.0
    z = np.zeros(T * 480, np.float32)
    g = R.score_row(z, R.make_signal(1, T))
    assert g["K"] == R.n_frames_10k(100 * T) == 92 and g["segments"] == 62 and g["stoi"] == 0.0 and g["estoi"] == 0.0 and abs(g["margin"] - 40.0) < 1e-9


def test_band_bins():
    assert TB.band_edges() == list(TB.BANDS) == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55),
                                                (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
    src = open(os.path.join(PKG, "csrc", "stoi", "stoi.hip")).read()
    lo = [int(v) for v in re.search(r"rn_stoi_band_lo\[RN_STOI_BANDS \+ 1\] = \{([^}]*)\}", src)[1].split(",")]
    assert lo == [a for a, _ in TB.BANDS] + [TB.BANDS[-1][1]]


def test_committed_tables_against_their_design():
    made = TB.design()
    for name in "HWCS":
        got, want = TB.TABLES[name], made[name]
        assert got.shape == want.shape and np.all(np.abs(got - want) <= np.spacing(np.abs(want))), name
    assert TB.H.size == 2305 and abs(TB.H.sum() - 1) < 1e-15 and np.array_equal(TB.H, TB.H[::-1])
    # the filter: flat where the bands are, down where the 10 kHz grid folds
    n = 1 << 20
    db = 20 * np.log10(np.abs(np.fft.rfft(TB.H, n)) + 1e-300)
    f = np.arange(n // 2 + 1) * (240000.0 / n)
    assert np.abs(db[f <= 4300]).max() < 0.0008
    assert -86.5 < db[np.argmin(np.abs(f - 5000))] < -86.0
    assert db[f >= 5000].max() <= -74.7
    text = open(os.path.join(PKG, "csrc", "stoi", "stoi_tables.h")).read()
    assert text == TB.header_text(), "stoi_tables.h is not what `python -m rnnoise_amd.stoi_tables --header` emits"
    assert TB.table_text(TB.TABLES).split() == TB._TABLE.split()


def test_resampled_length_and_a_tone():
    for frames in (1, 3, T):
        assert R.resample(np.zeros(480 * frames)).size == 100 * frames
    n = np.arange(480 * 40)
    y = R.resample(np.sin(2 * np.pi * 1000.0 * n / 48000.0))
    m = np.arange(y.size)
    mid = slice(300, y.size - 300)
    assert np.abs(y - np.sin(2 * np.pi * 1000.0 * m / 10000.0))[mid].max() < 2e-4  # zero phase, unit gain


# ---- the surface ----
def _declarations():
    src = open(HEADER).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return [(" ".join(ret.split()), name, " ".join(params.split()))
            for ret, name, params in re.findall(r"RNNOISE_EXPORT\s+([\w\s\*]+?)\b(rnnoise_\w+)\s*\(([^()]*)\)\s*;", src)]


def test_prototype_table_matches_the_header():
    decl = _declarations()
    assert [d[1] for d in decl] == list(S.PROTOTYPES) == S.EXPORTS and len(decl) == 4
    for ret, name, params in decl:
        restype, argtypes = S.PROTOTYPES[name]
        assert {"int": C.c_int, "long long": C.c_longlong}[ret] is restype, name
        assert len(argtypes) == params.count(",") + 1, (name, params)
    src = open(HEADER).read()
    for macro, value in (("FRAME", S.FRAME), ("SLOTS", S.SLOTS), ("MAX_ROWS", S.MAX_ROWS), ("MAX_FRAMES", S.MAX_FRAMES)):
        assert int(re.search(rf"#define RNNOISE_AMD_STOI_{macro} (\d+)", src)[1]) == value
    body = lambda name: re.sub(r"/\*.*?\*/", "", re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", src, re.S)[1], flags=re.S)
    fields = lambda text: [f.strip().lstrip("*") for d in text.split(";") if d.strip()
                           for f in d.replace("const float", "").replace("RNNoiseStoiPlane", "").replace("long", "").replace("int", "").split(",")]
    assert fields(body("RNNoiseStoiPlane")) == [n for n, _ in S.Plane._fields_]
    assert fields(body("RNNoiseStoi")) == [n.rstrip("_") for n, _ in S.Call._fields_]
    assert C.sizeof(S.Plane) == 24 and C.sizeof(S.Call) == 3 * 24 + 4 * 4


def test_library_exports_the_header_and_nothing_else():
    nm = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert syms == set(S.EXPORTS), sorted(syms ^ set(S.EXPORTS))
    assert all(hasattr(S.lib(), n) for n in S.EXPORTS)


def test_its_own_kernels_and_nothing_shared():
    strings = lambda p: subprocess.run(["strings", "-a", p], capture_output=True, text=True, check=True).stdout
    own = strings(S.LIB_PATH)
    assert set(re.findall(r"\b(rn_\w+)\.kd\b", own)) == set(S.KERNELS) and len(S.KERNELS) == 5
    assert not re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", own)  # no environment variable
    for name in ("librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so", "librnnoise_amd_score.so", "librnnoise_amd_train.so",
                 "librnnoise_amd_gru.so", "librnnoise_amd_gru_stack.so"):
        assert "rn_stoi" not in strings(os.path.join(PKG, name)) and "rnnoise_amd_stoi" not in strings(os.path.join(PKG, name)), name
    assert "librnnoise" not in subprocess.run(["ldd", S.LIB_PATH], capture_output=True, text=True).stdout
    for header in ("rnnoise_amd.h", "rnnoise_amd_score.h", "rnnoise_amd_train.h", "rnnoise_amd_gru.h", "rnnoise_amd_gru_stack.h"):
        assert "stoi" not in open(os.path.join(ROOT, "include", header)).read().lower(), header
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    for var in ("SRCS", "ISRCS", "HDRS", "FLAGS", "SIDE_FLAGS"):
        assert "stoi" not in re.search(rf"^{var}\s*:?=\s*(.*)$", mk, re.M)[1], var
    assert "-ffp-contract=off" in re.search(r"^SIDE_FLAGS\s*:?=\s*(.*)$", mk, re.M)[1]
    assert re.search(r"^\$\(eval \$\(call SIDE_LIB,stoi,stoi\.hip,rnnoise_amd_stoi\.h,side_host\.h .*\)\)$", mk, re.M)
    assert "build_stoi" in re.search(r"^clean:\n\t(.*)$", mk, re.M)[1] and "librnnoise_amd_stoi.so" in re.search(r"^all:(.*)$", mk, re.M)[1]
    # its objects are not among the product's, which tests/test_kernel_budgets_cpu.py lists
    assert os.path.exists(os.path.join(PKG, "csrc", "build_stoi", "stoi.o")) and not os.path.exists(os.path.join(PKG, "csrc", "build", "stoi.o"))
    ignored = open(os.path.join(ROOT, ".gitignore")).read()
    assert "rnnoise_amd/csrc/build_stoi/" in ignored


# ---- the host-only calls ----
def _call(**kw):
    buf = np.zeros(16 + 3 * 480 * 10, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    d = dict(ref=(base, 1440, 480), inp=(base, 1440, 480), out=(base, 1440, 480), n_rows=3, n_frames=10, first=2, delay=960)
    d.update(kw)
    return S.make_call(**d), buf


def test_check_accepts_and_refuses():
    ok, keep = _call()
    assert S.check(ok)
    base = ok.ref.p
    L = S.lib()
    assert L.rnnoise_amd_stoi_check(None) == -1
    bad = dict(
        null_ref=dict(ref=(0, 1440, 480)), null_out=dict(out=(0, 1440, 480)),
        unaligned_out=dict(out=(base + 4, 1440, 480)), unaligned_in=dict(inp=(base + 8, 1440, 480)),
        frame_stride_mod4=dict(ref=(base, 1442, 480)), row_stride_mod4=dict(inp=(base, 1440, 481)), stride_small=dict(out=(base, 476, 480)),
        stride_zero=dict(out=(base, 0, 0)), stride_negative=dict(ref=(base, -1440, 480)),
        first_before_delay=dict(first=1), first_before_delay_by_one=dict(first=2, delay=961), first_beyond_frames=dict(first=11, delay=0),
        negative_rows=dict(n_rows=-1), no_rows=dict(n_rows=0), negative_frames=dict(n_frames=-1), negative_first=dict(first=-1, delay=0),
        negative_delay=dict(delay=-1), rows_beyond=dict(n_rows=S.MAX_ROWS + 1), frames_beyond=dict(n_frames=S.MAX_FRAMES + 1),
        extent_overflow=dict(out=(base, 2 ** 62, 480)),
    )
    big = 1 << 40
    for name, kw in bad.items():
        call, _ = _call(**kw)
        assert not S.check(call), name
        # ... and the calls themselves refuse before they touch a device or a pointer
        assert L.rnnoise_amd_stoi_device(0, C.c_void_p(16), C.c_void_p(16), big, C.byref(call), None) == -1, name
        assert L.rnnoise_amd_stoi(0, C.cast(C.c_void_p(16), S._dp), C.byref(call)) == -1, name
    for kw in (dict(), dict(inp=None), dict(inp=(0, -5, 3)), dict(first=3, delay=963), dict(first=0, delay=0), dict(n_frames=0, first=0, delay=0),
               dict(first=10), dict(n_rows=S.MAX_ROWS, n_frames=S.MAX_FRAMES), dict(ref=(base, 480, 4800), n_rows=1)):
        assert S.check(_call(**kw)[0]), kw
    # a NULL results, and a NULL, misaligned or short scratch, are the device call's own refusals
    need = S.workspace(3, 10)
    for res, scratch, nbytes in ((None, 16, need), (16, None, need), (16, 20, need), (16, 16, need - 1), (16, 16, -1)):
        assert L.rnnoise_amd_stoi_device(0, res, scratch, nbytes, C.byref(ok), None) == -1, (res, scratch, nbytes)
    assert L.rnnoise_amd_stoi(0, None, C.byref(ok)) == -1
    del keep


def test_workspace_formula():
    for rows, frames in ((1, 0), (1, 2), (1, 3), (3, 10), (65, 120), (190, 2000), (S.MAX_ROWS, S.MAX_FRAMES)):
        assert S.workspace(rows, frames) == S.workspace_formula(rows, frames) > 0, (rows, frames)
    assert S.workspace_formula(1, 2000) == 8 * (3 * 200000 + 50 * 1561) + 4 * 1562 + 8  # 5.4 MB a row
    for rows, frames in ((0, 10), (-1, 10), (1, -1), (S.MAX_ROWS + 1, 10), (1, S.MAX_FRAMES + 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert S.lib().rnnoise_amd_stoi_workspace(rows, frames) == -1
        with pytest.raises(ValueError):
            S.workspace(rows, frames)


def test_host_half_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stoi_check_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "stoi_check_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- metrics ----
def test_metrics_on_hand_made_results():
    res = np.array([[9.0, 4.5, 10, 40, 9.5, 6.0, 10, 40],
                    [0.0, 0.0, 0, 12, 0.0, 0.0, 0, 12],       # fewer than 31 kept frames: no segment
                    [0.0, 0.0, 0, 0, 18.0, 15.0, 20, 50]])   # scored without a noisy plane
    m = S.metrics(res)
    assert m["stoi_in"][0] == 0.9 and m["estoi_in"][0] == 0.45 and m["stoi_out"][0] == 0.95 and m["estoi_out"][0] == 0.6
    assert all(np.isnan(m[k][1]) for k in S.METRIC_KEYS) and np.isnan(m["stoi_in"][2]) and m["stoi_out"][2] == 0.9
    s = m["summary"]
    assert s["sequences"] == 2 and s["excluded"] == 1 and m["kept"].tolist() == [True, False, True]
    assert s["stoi_out"] == pytest.approx(0.925) and s["estoi_out"] == pytest.approx(0.675) and s["stoi_in"] == 0.9 and s["estoi_in"] == 0.45
    none = S.metrics(res[1:2])["summary"]
    assert none["sequences"] == 0 and none["excluded"] == 1 and np.isnan(none["stoi_out"])


# ---- the command line ----
def test_eval_audio_stoi_flag(monkeypatch, capsys):
    row = dict(sequences=2, excluded=0, snr_in=1.0, snr_out=2.0, snr_gain=1.0, si_sdr_in=1.0, si_sdr_out=2.0, si_sdr_gain=1.0, seg_snr_in=1.5,
               seg_snr_out=4.25)
    with_stoi = [dict(row, stoi_in=0.75, stoi_out=0.875, estoi_in=0.5, estoi_out=0.625), dict(row, stoi_in=0.75, stoi_out=0.9375, estoi_in=0.5, estoi_out=0.75)]
    seen = {}

    def fake(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return ["a.blob", "ckpt.pth"], with_stoi if kw.get("stoi") else [row, row]
    monkeypatch.setattr(cli, "eval_audio_files", fake)
    argv = ["eval-audio", "s.pcm", "n.pcm", "f.pcm", "--model", "a.blob", "--checkpoint", "ckpt.pth", "--count", "9", "--frames", "30", "--seed", "4",
            "--streams", "4"]
    cli.main(argv)
    plain = capsys.readouterr().out
    # the default call passes what it passed before the flag existed, and prints the table it printed
    assert seen["args"] == ("s.pcm", "n.pcm", "f.pcm", ["a.blob"], 9, 30, "ckpt.pth", None, None, 4, 4, 0) and seen["kw"] == {}
    assert "STOI" not in plain and plain.splitlines()[1:] == cli.audio_table(["a.blob", "ckpt.pth"], [row, row]).splitlines()
    cli.main(argv + ["--stoi"])
    assert seen["args"] == ("s.pcm", "n.pcm", "f.pcm", ["a.blob"], 9, 30, "ckpt.pth", None, None, 4, 4, 0) and seen["kw"] == dict(stoi=True)
    head, a, b, d = capsys.readouterr().out.splitlines()[1:]
    assert head.split()[-8:] == ["STOI", "in", "STOI", "out", "ESTOI", "in", "ESTOI", "out"] and "segSNR out" in head
    assert [float(v) for v in a.split()[-4:]] == [0.75, 0.875, 0.5, 0.625] and [float(v) for v in b.split()[-4:]] == [0.75, 0.938, 0.5, 0.75]
    assert [float(v) for v in d.split()[-4:]] == [0.0, 0.062, 0.0, 0.125] and float(a.split()[-5]) == 4.25
    # without the flag the first lines of the two tables agree column for column
    assert head.startswith(plain.splitlines()[1]) and a.startswith(plain.splitlines()[2])


def test_evaluate_audio_takes_the_flag():
    """off by default, in cli.eval_audio_files and in evaluate.evaluate_audio (tests/test_stoi_gpu.py runs it)"""
    import inspect

    from rnnoise_amd import evaluate
    assert evaluate.eval_audio is evaluate.evaluate_audio
    assert inspect.signature(evaluate.evaluate_audio).parameters["stoi"].default is False
    assert inspect.signature(cli.eval_audio_files).parameters["stoi"].default is False


def test_eval_audio_files_reaches_evaluate_audio(monkeypatch, tmp_path):
    """cli.main -> cli.eval_audio_files -> evaluate.evaluate_audio(stoi=True), the corpora kept on the host: the flag arrives, and
    without it the evaluation is told stoi=False"""
    import torch

    from rnnoise_amd import evaluate

    class HostCorpus:
        def __init__(self, a):
            self.a = a

        def to(self, _device):
            return self

        def numel(self):
            return self.a.size
    names = []
    for k, n in enumerate((480 * 40, 480 * 35, 480 * 33)):
        names.append(str(tmp_path / f"c{k}.pcm"))
        np.zeros(n, np.int16).tofile(names[-1])
    blob = tmp_path / "a.blob"
    blob.write_bytes(b"DNNw")
    row = dict(sequences=2, excluded=0, snr_in=1.0, snr_out=2.0, snr_gain=1.0, si_sdr_in=1.0, si_sdr_out=2.0, si_sdr_gain=1.0, seg_snr_in=1.5,
               seg_snr_out=4.25, stoi_in=0.75, stoi_out=0.875, estoi_in=0.5, estoi_out=0.625)
    seen = []

    def fake(corpora, models, draws, n_frames, **kw):
        seen.append((len(corpora), models, len(draws.mix), n_frames, kw["stoi"]))
        return [row]
    monkeypatch.setattr(torch, "from_numpy", HostCorpus)
    monkeypatch.setattr(evaluate, "evaluate_audio", fake)
    argv = ["eval-audio", *names, "--model", str(blob), "--count", "2", "--frames", "30", "--seed", "4"]
    cli.main(argv + ["--stoi"])
    cli.main(argv)
    assert seen == [(3, [b"DNNw"], 2, 30, True), (3, [b"DNNw"], 2, 30, False)]


def test_stoi_refuses_long_sequences_before_any_work():
    from rnnoise_amd import evaluate
    with pytest.raises(ValueError, match="at most 8192"):
        evaluate.evaluate_audio([], [b"DNNw"], None, S.MAX_FRAMES + 1, stoi=True)
    with pytest.raises(SystemExit):
        cli.main(["eval-audio", "s", "n", "f", "--model", "a", "--count", "1", "--frames", str(S.MAX_FRAMES + 1), "--stoi"])
