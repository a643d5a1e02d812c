"""CPU checks of the float-network runtime library (include/rnnoise_amd_fnet.h, rnnoise_amd/csrc/fnet/, rnnoise_amd/fnet.py): what it
declares, exports and refuses; that it shares only the two headers with the other libraries and changed none of them; its byte and
launch formulas; its host-only half as a program under the address and undefined-behaviour sanitizers; what FloatNetRuntime refuses;
the --float-net flag of the command line; and that the C example compiles and links.  (The kernels: tests/test_fnet_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fnet_cases as fc
from gru_cases import _declarations
from rnnoise_amd import cli
from rnnoise_amd import fnet as N

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
HEADER = os.path.join(ROOT, "include", "rnnoise_amd_fnet.h")


# ---- the surface ----
def test_prototype_table_matches_the_header():
    decl = _declarations(HEADER)
    assert [d[1] for d in decl] == list(N.PROTOTYPES) == N.EXPORTS and len(decl) == 10
    for ret, name, params in decl:
        restype, argtypes = N.PROTOTYPES[name]
        assert {"int": C.c_int, "long long": C.c_longlong, "void": None, "RNNoiseFnet *": C.c_void_p}[ret] is restype, name
        assert len(argtypes) == params.count(",") + 1, (name, params)
    src = open(HEADER).read()
    for macro, value in (("FEATURES", N.FEATURES), ("BANDS", N.BANDS), ("LOOKAHEAD", N.LOOKAHEAD), ("MIN_COND", N.MIN_COND), ("MAX_COND", N.MAX_COND),
                         ("MIN_GRU", N.MIN_GRU), ("MAX_GRU", N.MAX_GRU), ("MAX_ROWS", N.MAX_ROWS), ("MAX_FRAMES", N.MAX_FRAMES)):
        assert int(re.search(rf"#define RNNOISE_AMD_FNET_{macro} (\d+)", src)[1]) == value
    body = lambda name: re.sub(r"/\*.*?\*/", "", re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", src, re.S)[1], flags=re.S)
    names = lambda text: [re.sub(r"\[\d+\]", "", f.strip().lstrip("*")) for d in text.split(";") if d.strip()
                          for f in re.sub(r"\b(const float|long|int)\b", "", d).split(",")]
    assert names(body("RNNoiseFnetRows")) == [n for n, _ in N.Rows._fields_]
    assert names(body("RNNoiseFnetWeights")) == [n for n, _ in N.Weights._fields_]
    assert C.sizeof(N.Rows) == 16 and C.sizeof(N.Weights) == 8 + 20 * 8
    assert "rnnoise_amd.h" not in re.findall(r'#include\s+"([^"]+)"', src)  # a struct of its own, not the product's header
    for word in ("OUT OF SCOPE", "saving and loading", "masks", "int8", "backward"):
        assert word in src, word


def test_library_exports_the_header_and_nothing_else():
    nm = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert syms == set(N.EXPORTS), sorted(syms ^ set(N.EXPORTS))
    assert all(hasattr(N.lib(), n) for n in N.EXPORTS)


def test_its_own_kernels_and_nothing_shared():
    from rnnoise_amd import gru_native, gru_stack, stoi, train_loss
    strings = lambda p: subprocess.run(["strings", "-a", p], capture_output=True, text=True, check=True).stdout
    kernels = lambda p: set(re.findall(r"\b(rn_\w+)\.kd\b", strings(p)))
    own = strings(N.LIB_PATH)
    assert kernels(N.LIB_PATH) == set(N.KERNELS) and len(N.KERNELS) == 6
    assert not re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", own) and "getenv" not in own  # no environment variable
    # no other library's object changed its kernel list
    for module in (gru_native, gru_stack, stoi, train_loss):
        assert kernels(module.LIB_PATH) == set(module.KERNELS), module.__name__
    assert len(kernels(os.path.join(PKG, "librnnoise_amd_score.so"))) == 1
    for name in ("librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so", "librnnoise_amd_score.so", "librnnoise_amd_train.so",
                 "librnnoise_amd_gru.so", "librnnoise_amd_gru_stack.so", "librnnoise_amd_stoi.so"):
        other = strings(os.path.join(PKG, name))
        assert "rn_fnet" not in other and "rnnoise_amd_fnet" not in other, name
    assert "librnnoise" not in subprocess.run(["ldd", N.LIB_PATH], capture_output=True, text=True).stdout
    for header in ("rnnoise_amd.h", "rnnoise.h", "rnnoise_amd_score.h", "rnnoise_amd_train.h", "rnnoise_amd_gru.h", "rnnoise_amd_gru_stack.h",
                   "rnnoise_amd_stoi.h"):
        assert "fnet" not in open(os.path.join(ROOT, "include", header)).read().lower(), header
    # the unit's quoted includes: its public header, the cell, and its plan (which brings the shared host checks)
    unit = open(os.path.join(PKG, "csrc", "fnet", "fnet.hip")).read()
    assert sorted(re.findall(r'^\s*#\s*include\s+"([^"]+)"', unit, re.M)) == ["../gru_cell.h", "fnet_plan.h", "rnnoise_amd_fnet.h"]
    plan = open(os.path.join(PKG, "csrc", "fnet", "fnet_plan.h")).read()
    assert sorted(re.findall(r'^\s*#\s*include\s+"([^"]+)"', plan, re.M)) == ["../side_host.h", "rnnoise_amd_fnet.h"]
    for word in ("__global__", "hip/", "getenv", 'extern "C"'):
        assert word not in plan, word
    assert "getenv" not in unit and "atomic" not in unit.lower() and "hipGraph" not in unit


def test_makefile_and_ignore_rules():
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    for var in ("SRCS", "ISRCS", "HDRS", "FLAGS", "SIDE_FLAGS"):
        assert "fnet" not in re.search(rf"^{var}\s*:?=\s*(.*)$", mk, re.M)[1], var
    assert "-ffp-contract=off" in re.search(r"^SIDE_FLAGS\s*:?=\s*(.*)$", mk, re.M)[1]
    rule = re.search(r"^\$\(eval \$\(call SIDE_LIB,fnet,fnet\.hip,rnnoise_amd_fnet\.h,(.*)\)\)$", mk, re.M)
    assert rule and sorted(rule[1].split()) == ["fnet/fnet_plan.h", "gru_cell.h", "side_host.h"]
    clean, all_ = re.search(r"^clean:\n\t(.*)$", mk, re.M)[1], re.search(r"^all:(.*)$", mk, re.M)[1]
    assert "build_fnet" in clean and "../librnnoise_amd_fnet.so" in clean and "../librnnoise_amd_fnet.so" in all_
    assert re.search(r"^build .*\bbuild_fnet\b.*:$", mk, re.M)
    assert os.path.exists(os.path.join(PKG, "csrc", "build_fnet", "fnet.o")) and not os.path.exists(os.path.join(PKG, "csrc", "build", "fnet.o"))
    assert "rnnoise_amd/csrc/build_fnet/" in open(os.path.join(ROOT, ".gitignore")).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert re.search(r"for module in \(.*\bfnet\b.*\):", entry)


# ---- the host-only calls ----
def _weights(cond=32, gru=48):
    return N.weights(fc.net(cond, gru).state_dict())


def test_check_accepts_and_refuses():
    w, keep = _weights()
    L = N.lib()
    assert N.check(w, 1, 1) and N.check(w, N.MAX_ROWS, N.MAX_FRAMES) and N.check(w, 67, 16)
    assert L.rnnoise_amd_fnet_check(None, 1, 1) == -1
    for n_rows, max_frames in ((0, 1), (-1, 1), (N.MAX_ROWS + 1, 1), (1, 0), (1, -1), (1, N.MAX_FRAMES + 1)):
        assert not N.check(w, n_rows, max_frames), (n_rows, max_frames)
        assert not L.rnnoise_amd_fnet_create(0, C.byref(w), n_rows, max_frames)  # ... and create refuses before it touches a device
    # every dimension limit and its neighbours (the tensors are not dereferenced: the pointers of the small net do)
    dims = lambda c, h: N.Weights.from_buffer_copy(bytes(C.c_int(c)) + bytes(C.c_int(h)) + bytes(w)[8:])
    for c in (16, 32, 1008, 1024):
        assert N.check(dims(c, 384), 1, 1), c
    for c in (0, -16, 8, 15, 17, 24, 1025, 1040):
        assert not N.check(dims(c, 384), 1, 1), c
    for h in (16, 32, 48, 4080, 4096):
        assert N.check(dims(128, h), 1, 1), h
    for h in (0, -16, 8, 15, 17, 40, 4097, 4112):
        assert not N.check(dims(128, h), 1, 1), h
        assert not L.rnnoise_amd_fnet_create(0, C.byref(dims(128, h)), 1, 1)
    # NULL and misaligned tensors, one at a time
    raw = bytearray(bytes(w))
    for k in range(20):
        for value in (0, keep["conv1.bias"].ctypes.data + 2):
            b = bytearray(raw)
            b[8 + 8 * k: 16 + 8 * k] = value.to_bytes(8, "little")
            assert not N.check(N.Weights.from_buffer_copy(bytes(b)), 1, 1), (k, value)
    del keep


def test_rows_check_and_process_refusals():
    ok = [((0, 0), 65), (None, 65), (None, 1), ((7 * 65, 65), 65), ((65, 3 * 65), 65), ((7 * 67 + 5, 67), 65), ((3, 9), 1), ((32, 96), 32)]
    for rows, w in ok:
        assert N.rows_check(rows, w, 7, 3), (rows, w)
    bad = [((65, 64), 65), ((64, 7 * 65), 65), ((7 * 65 - 1, 65), 65), ((65, 3 * 65 - 1), 65), ((0, 65), 65), ((65, 0), 65), ((-65, 65), 65),
           ((65, -65), 65), ((2 ** 62, 65), 65), ((32, 16), 32), ((1, 2), 1)]
    for rows, w in bad:
        assert not N.rows_check(rows, w, 7, 3), (rows, w)
    assert not N.rows_check(None, 0, 7, 3) and not N.rows_check(None, 65, 0, 3) and not N.rows_check(None, 65, 7, -1) and N.rows_check(None, 65, 7, 0)
    L = N.lib()
    # a NULL runtime is refused by every call that takes one, before anything else is looked at
    p = C.c_void_p(16)
    assert L.rnnoise_amd_fnet_process_device(None, p, None, p, None, p, None, 1, None) == -1
    assert L.rnnoise_amd_fnet_process(None, p, None, p, None, p, None, 1) == -1
    assert L.rnnoise_amd_fnet_reset(None, None) == -1 and L.rnnoise_amd_fnet_reset_rows_device(None, p, 1, None) == -1
    assert L.rnnoise_amd_fnet_reset_rows(None, None, 0) == -1
    L.rnnoise_amd_fnet_destroy(None)


def test_bytes_formula():
    for cond, gru, rows, frames in ((16, 16, 1, 1), (32, 48, 67, 16), (128, 384, 16384, 10), (128, 256, 4096, 1), (1024, 4096, N.MAX_ROWS, N.MAX_FRAMES)):
        assert N.nbytes(cond, gru, rows, frames) == N.bytes_formula(cond, gru, rows, frames) > 0, (cond, gru, rows, frames)
    # the default size, one row, one frame, term by term
    assert N.bytes_formula(128, 384, 1, 1) == 4 * (196 * 128 + 128 + 3 * 128 * 384 + 384 + 18 * 384 * 384 + 18 * 384 + 192 * 384 + 48) + 4 * (65 * 5 + 1152) + 8 \
        + 4 * (3 * 128 + 4 * 384 + 12 * 384 + 1)
    for cond, gru, rows, frames in ((0, 384, 1, 1), (24, 384, 1, 1), (128, 8, 1, 1), (128, 4112, 1, 1), (128, 384, 0, 1), (128, 384, N.MAX_ROWS + 1, 1),
                                    (128, 384, 1, 0), (128, 384, 1, N.MAX_FRAMES + 1)):
        assert N.lib().rnnoise_amd_fnet_bytes(cond, gru, rows, frames) == -1
        with pytest.raises(ValueError):
            N.nbytes(cond, gru, rows, frames)


def test_launch_formula_of_the_module():
    assert N.launches_formula(35, 16, 0) == 3 * 4 + 14 + 18 + 5 and N.launches_formula(3, 16, 0) == 4 and N.launches_formula(3, 16, 2) == 7
    assert N.launches_formula(0, 4, 0) == 0 and N.launches_formula(1, 1, 100) == 7


def test_host_half_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fnet_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "fnet_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.fullmatch(r"fnet_plan_main: \d+ checks\n", r.stdout)


# ---- the module ----
def test_weights_reads_the_dimensions_off_the_tensors(tmp_path):
    w, keep = _weights(32, 48)
    assert (w.cond_size, w.gru_size) == (32, 48) and set(keep) == set(N.TENSORS) and len(N.TENSORS) == 20
    assert w.gru_weight_hh[2] == keep["gru3.weight_hh_l0"].ctypes.data and w.vad_dense_bias == keep["vad_dense.bias"].ctypes.data
    sd = dict(fc.net(32, 48).state_dict())
    path = tmp_path / "ck.pth"
    torch.save({"model_args": (), "model_kwargs": {}, "state_dict": sd}, path)
    for source in (fc.net(32, 48), sd, str(path)):
        rt = N.FloatNetRuntime(source, max_frames=4)
        assert (rt.cond_size, rt.gru_size, rt.max_frames) == (32, 48, 4)
    del sd["gru2.bias_hh_l0"]
    with pytest.raises(ValueError, match="lacks"):
        N.weights(sd)
    sd = dict(fc.net(32, 48).state_dict())
    sd["dense_out.weight"] = sd["dense_out.weight"][:, :-1]
    with pytest.raises(ValueError, match="dense_out.weight"):
        N.weights(sd)
    with pytest.raises(ValueError, match="max_frames"):
        N.FloatNetRuntime(fc.net(32, 48), max_frames=0)
    with pytest.raises(ValueError, match="on the device"):
        N.FloatNetRuntime(fc.net(32, 48), device="cpu")


def test_runtime_refuses_cpu_tensors_and_other_dtypes():
    rt = N.FloatNetRuntime(fc.net(16, 16))
    x = torch.zeros((2, 3, 65))
    for bad in (x, x.double(), x.numpy()):
        with pytest.raises(ValueError, match="no fallback"):
            rt(bad)
    assert rt._h is None  # nothing was created
    rt.reset(), rt.reset_rows([0]), rt.close()  # before the first call there is nothing to reset


# ---- the command line ----
def test_cli_float_net_flag(monkeypatch, capsys):
    seen = {}

    def fake_audio(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        row = dict(sequences=2, excluded=0, snr_in=1.0, snr_out=2.0, snr_gain=1.0, si_sdr_in=1.0, si_sdr_out=2.0, si_sdr_gain=1.0, seg_snr_in=1.5,
                   seg_snr_out=4.25, stoi_in=0.75, stoi_out=0.875, estoi_in=0.5, estoi_out=0.625)
        return ["ckpt.pth"], [row]

    def fake_denoise(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        return [7]
    monkeypatch.setattr(cli, "eval_audio_files", fake_audio)
    monkeypatch.setattr(cli, "denoise_files", fake_denoise)
    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the command line loaded the library"))
    audio = ["eval-audio", "s.pcm", "n.pcm", "f.pcm", "--checkpoint", "ckpt.pth", "--count", "9", "--frames", "30", "--seed", "4", "--streams", "4"]
    cli.main(audio)
    plain = capsys.readouterr().out
    # the default call passes what it passed before the flag existed, and prints what it printed
    assert seen["args"] == ("s.pcm", "n.pcm", "f.pcm", [], 9, 30, "ckpt.pth", None, None, 4, 4, 0) and seen["kw"] == {}
    cli.main(audio + ["--float-net", "torch"])
    assert seen["kw"] == {} and capsys.readouterr().out == plain
    cli.main(audio + ["--float-net", "native"])
    assert seen["args"] == ("s.pcm", "n.pcm", "f.pcm", [], 9, 30, "ckpt.pth", None, None, 4, 4, 0) and seen["kw"] == dict(float_net="native")
    assert capsys.readouterr().out == plain
    cli.main(audio + ["--float-net", "native", "--stoi"])
    assert seen["kw"] == dict(stoi=True, float_net="native")
    capsys.readouterr()
    den = ["denoise", "--checkpoint", "ckpt.pth", "--model", os.devnull, "--out-dir", "out", "a.raw"]
    want = (b"", ["a.raw"], "out", 100, 0, False, 48000, None, 0.0, 0, None, None, False, None, None, None, 4.0, "ckpt.pth")
    cli.main(den)
    assert seen["args"] == want and seen["kw"] == {}
    plain = capsys.readouterr().out
    cli.main(den + ["--float-net", "native"])
    assert seen["args"] == want and seen["kw"] == dict(float_net="native") and capsys.readouterr().out == plain == "denoised 1 streams, 7 frames\n"
    # native without a checkpoint is an argument error, and so is another word
    for argv in (["denoise", "--model", os.devnull, "--out-dir", "out", "a.raw", "--float-net", "native"],
                 ["eval-audio", "s", "n", "f", "--model", "a.blob", "--count", "1", "--float-net", "native"],
                 den + ["--float-net", "fast"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    capsys.readouterr()


def test_the_functions_take_the_flag_and_default_to_torch(monkeypatch, tmp_path):
    import inspect

    from rnnoise_amd import float_net
    assert inspect.signature(cli.eval_audio_files).parameters["float_net"].default == "torch"
    assert inspect.signature(cli.denoise_files).parameters["float_net"].default == "torch"
    with pytest.raises(ValueError, match="checkpoint"):
        cli.denoise_files(b"", [], str(tmp_path), float_net="native")
    with pytest.raises(ValueError, match="float_net"):
        cli.denoise_files(b"", [], str(tmp_path), checkpoint="ckpt.pth", float_net="fast")
    # the default path loads the torch module, the native one a FloatNetRuntime: neither reaches a device here
    made = []
    monkeypatch.setattr(float_net, "load_checkpoint", lambda path, device=None: made.append(("torch", path, device)) or "net")
    monkeypatch.setattr(N, "FloatNetRuntime", lambda path, device=None: made.append(("native", path, device)) or "net")
    monkeypatch.setattr(cli.capi, "Model", lambda blob: pytest.fail("no file, no model") if False else type("M", (), {"close": lambda self: None})())
    cli.denoise_files(b"", [], str(tmp_path), checkpoint="ckpt.pth")
    cli.denoise_files(b"", [], str(tmp_path), checkpoint="ckpt.pth", float_net="native", device=3)
    assert made == [("torch", "ckpt.pth", "cuda:0"), ("native", "ckpt.pth", 3)]


# ---- the C example ----
def test_the_c_example_compiles_and_links(tmp_path):
    exe = fc.build_c_example(str(tmp_path))
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tools", "fnet_serve.c")).read()
    assert sorted(re.findall(r'#include\s+"([^"]+)"', src)) == ["rnnoise_amd.h", "rnnoise_amd_fnet.h"] and len(src.splitlines()) <= 110
    for call in ("rnnoise_batch_analyze_device", "rnnoise_amd_fnet_process_device", "rnnoise_batch_synthesize_device"):
        assert call in src
    # INTEGRATION.md shows this file
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "tools/fnet_serve.c" in doc and "rnnoise_amd_fnet_process_device(net, d_gains, NULL, d_vad, NULL, d_feat, NULL, T, stream)" in doc
