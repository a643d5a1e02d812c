"""CPU checks of the audio score library (include/rnnoise_amd_score.h, rnnoise_amd/csrc/score/audio_score.hip, rnnoise_amd/audio_score.py):
what it declares, exports and refuses; that the product libraries know nothing of it; metrics() on hand-made sums; the numpy
restatement of the ORDER (tests/audio_score_ref.py) against plain sums; the kernel's own body on the host under the address and
undefined-behaviour sanitizers, lane after lane, bit for bit against the restatement; the delay constant against the oracle; and the
eval-audio command's arguments and table.  (The kernel itself: tests/test_audio_score_gpu.py.)"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import audio_score_ref as R
from conftest import assert_bits_equal
from rnnoise_amd import audio_score as A
from rnnoise_amd import capi, cli, synth

planes = R.planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
HEADER = os.path.join(ROOT, "include", "rnnoise_amd_score.h")


def _declarations():
    src = open(HEADER).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return [(" ".join(ret.split()), name, " ".join(params.split()))
            for ret, name, params in re.findall(r"RNNOISE_EXPORT\s+([\w\s\*]+?)\b(rnnoise_\w+)\s*\(([^()]*)\)\s*;", src)]


# ---- the surface ----
def test_prototype_table_matches_the_header():
    decl = _declarations()
    assert [d[1] for d in decl] == list(A.PROTOTYPES) == A.EXPORTS and len(decl) == 3
    for ret, name, params in decl:
        restype, argtypes = A.PROTOTYPES[name]
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == params.count(",") + 1, (name, params)
    src = open(HEADER).read()
    for macro, value in (("RNNOISE_AMD_SCORE_FRAME", A.FRAME), ("RNNOISE_AMD_SCORE_SLOTS", A.SLOTS), ("RNNOISE_AMD_SCORE_DELAY", A.DELAY)):
        assert int(re.search(rf"#define {macro} (\d+)", src)[1]) == value == {"FRAME": R.FRAME, "SLOTS": R.SLOTS, "DELAY": R.DELAY}[macro[18:]]
    # the structures: field for field
    fields = lambda body: [f.strip().lstrip("*") for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip()
                           for f in decl.replace("const float", "").replace("RNNoiseAudioPlane", "").replace("long", "").replace("int", "").split(",")]
    body = lambda name: re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", src, re.S)[1]
    assert fields(body("RNNoiseAudioPlane")) == [n for n, _ in A.Plane._fields_]
    assert fields(body("RNNoiseAudioScore")) == [n.rstrip("_") for n, _ in A.Call._fields_]
    assert C.sizeof(A.Plane) == 24 and C.sizeof(A.Call) == 3 * 24 + 6 * 4


def test_library_exports_the_header_and_nothing_else():
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert syms == set(A.EXPORTS), sorted(syms ^ set(A.EXPORTS))
    L = A.lib()
    assert all(hasattr(L, n) for n in A.EXPORTS)


def test_one_kernel_of_its_own_and_nothing_in_the_product():
    strings = lambda p: subprocess.run(["strings", "-a", p], capture_output=True, text=True, check=True).stdout
    own = strings(A.LIB_PATH)
    assert set(re.findall(r"\b(rn_\w+)\.kd\b", own)) == {"rn_audio_score_kernel"}
    assert not re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", own)  # no environment variable
    for name in ("librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"):
        text = strings(os.path.join(PKG, name))
        assert "audio_score" not in text, name
    ldd = subprocess.run(["ldd", A.LIB_PATH], capture_output=True, text=True).stdout
    assert "librnnoise" not in ldd
    # nothing of it in the product's headers, prototype table or source lists
    assert "audio_score" not in open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    assert not [n for n in capi.PROTOTYPES if "audio" in n]
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    for var in ("SRCS", "ISRCS", "HDRS", "FLAGS"):
        assert "score" not in re.search(rf"^{var}\s*:=\s*(.*)$", mk, re.M)[1], var


# ---- the argument check ----
def _call(**kw):
    buf = np.zeros(16 + 3 * 480 * 10, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    d = dict(ref=(base, 480 * 3, 480), inp=(base, 480 * 3, 480), out=(base, 480 * 3, 480), n_rows=3, t0=0, n_frames=10, first=2, delay=960,
             terms_frames=10)
    d.update(kw)
    return A.make_call(**d), buf


def test_check_accepts_and_refuses():
    ok, keep = _call()
    assert A.check(ok)
    base = ok.ref.p
    assert A.lib().rnnoise_amd_audio_score_check(None) == -1
    bad = dict(
        null_ref=dict(ref=(0, 1440, 480)), null_in=dict(inp=(0, 1440, 480)), null_out=dict(out=(0, 1440, 480)),
        unaligned=dict(out=(base + 4, 1440, 480)),
        frame_stride_mod4=dict(ref=(base, 1442, 480)), row_stride_mod4=dict(inp=(base, 1440, 481)), stride_small=dict(out=(base, 476, 480)),
        stride_zero=dict(out=(base, 0, 0)), stride_negative=dict(ref=(base, -1440, 480)),
        first_before_delay=dict(first=1), first_before_delay_by_one=dict(first=2, delay=961),
        negative_rows=dict(n_rows=-1), no_rows=dict(n_rows=0), negative_t0=dict(t0=-1), negative_frames=dict(n_frames=-1),
        negative_first=dict(first=-1, delay=0), negative_delay=dict(delay=-1),
        frames_overflow=dict(t0=2 ** 31 - 5, n_frames=10), extent_overflow=dict(out=(base, 2 ** 62, 480)),
    )
    for name, kw in bad.items():
        call, _ = _call(**kw)
        assert not A.check(call), name
        # ... and the calls themselves refuse before they touch a device or a pointer
        assert A.lib().rnnoise_amd_audio_score_device(0, C.c_void_p(16), None, C.byref(call), None) == -1, name
        assert A.lib().rnnoise_amd_audio_score(0, C.cast(C.c_void_p(16), A._dp), None, C.byref(call)) == -1, name
    for kw in (dict(first=2, delay=960), dict(first=3, delay=963), dict(first=0, delay=0), dict(n_frames=0), dict(t0=2 ** 31 - 11, n_frames=10),
               dict(ref=(base, 480, 4800), n_rows=1)):
        assert A.check(_call(**kw)[0]), kw
    # a NULL sums, and frame records shorter than the call, are the calls' own refusals
    assert A.lib().rnnoise_amd_audio_score_device(0, None, None, C.byref(ok), None) == -1
    short, _ = _call(terms_frames=9)
    assert A.check(short) and A.lib().rnnoise_amd_audio_score_device(0, C.c_void_p(16), C.c_void_p(16), C.byref(short), None) == -1
    del keep


# ---- metrics ----
def test_metrics_on_hand_made_sums():
    #           r.r   x.x   y.y   x.r   y.r  (x-r)^2 (y-r)^2  n
    sums = np.array([[100., 200., 100., 100., 100., 100., 0., 960.],      # out == ref: no error energy
                     [0., 50., 10., 0., 0., 50., 10., 960.],               # silent clean signal: left out
                     [400., 500., 404., 400., 400., 100., 4., 960.],
                     [100., 100., 25., 100., 50., 0., 25., 960.]])          # in == ref; out = ref / 2
    m = A.metrics(sums)
    assert m["kept"].tolist() == [True, False, True, True] and m["excluded"] == 1 and m["sequences"] == 3
    assert m["snr_in"][0] == 0.0 and np.isposinf(m["snr_out"][0]) and np.isposinf(m["snr_gain"][0])
    assert np.isposinf(m["si_sdr_out"][0]) and m["si_sdr_in"][0] == pytest.approx(0.0)  # target 100, distortion 200 - 100
    assert m["snr_in"][1] == pytest.approx(10 * np.log10(4)) and m["snr_out"][1] == pytest.approx(20.0)
    assert m["si_sdr_in"][1] == pytest.approx(10 * np.log10(400 / 100)) and m["si_sdr_out"][1] == pytest.approx(10 * np.log10(400 / 4))
    assert m["si_sdr_gain"][1] == pytest.approx(m["si_sdr_out"][1] - m["si_sdr_in"][1])
    # scale invariance: out = ref / 2 has SNR 10 log10(100 / 25) but no distortion
    assert np.isposinf(m["snr_in"][2]) and m["snr_out"][2] == pytest.approx(10 * np.log10(4)) and np.isposinf(m["si_sdr_out"][2])
    s = A.summary(m)
    assert s["sequences"] == 3 and s["excluded"] == 1 and np.isposinf(s["snr_out"]) and "seg_snr_out" not in s


def test_segmental_snr_clamps_masks_and_skips():
    T = 6
    ft = np.zeros((2, T, 8))
    # sequence 0: frame 0 unscored (all zero); 1: +50 dB -> 35; 2: -30 dB -> -10; 3: 20 dB; 4: silent clean frame, skipped; 5: no error -> 35
    for t, (e0, e6) in {1: (1e5, 1.0), 2: (1.0, 1e3), 3: (100.0, 1.0), 4: (0.0, 5.0), 5: (7.0, 0.0)}.items():
        ft[0, t] = [e0, 0, 0, 0, 0, 2 * e6, e6, 480]
    ft[1, 3] = [100.0, 0, 0, 0, 0, 1.0, 10.0, 480]
    sums = ft.sum(1)
    m = A.metrics(sums, ft)
    assert m["seg_frames"].tolist() == [4, 1]
    assert m["seg_snr_out"][0] == pytest.approx((35 - 10 + 20 + 35) / 4) and m["seg_snr_out"][1] == pytest.approx(10.0)
    assert m["seg_snr_in"][0] == pytest.approx((35 - 10 + (20 - 10 * np.log10(2)) + 35) / 4)
    active = np.zeros((2, T))
    active[0, [2, 3, 4]] = 1
    m = A.metrics(sums, ft, active)
    assert m["seg_frames"].tolist() == [2, 0] and m["seg_snr_out"][0] == pytest.approx(5.0) and np.isnan(m["seg_snr_out"][1])
    s = A.summary(m)
    assert s["seg_snr_out"] == pytest.approx(5.0)  # (the sequence without a frame is left out of this mean)


# ---- the restatement ----
def test_restatement_against_plain_sums():
    """a wrong term or a wrong index shows here; the order does not (that is the kernel tests' business)"""
    rng = np.random.default_rng(5)
    for layout, D, first in (("frames", 960, 2), ("streams", 963, 3), ("frames", 1, 1), ("streams", 0, 0)):
        n_rows, T = 3, 6
        ref, inp, out = planes(rng, n_rows, T, layout, special=False)
        sums = np.zeros((n_rows, 8))
        ft = np.full((n_rows, T, 8), -1.0)
        R.score(ref, inp, out, n_rows, 0, T, first, D, sums, ft)
        r, x, y = (R.sequences(*p, n_rows, T) for p in (ref, inp, out))
        n = np.arange(first * 480, T * 480)
        want = R.terms(r[:, n - D], x[:, n - D], y[:, n]).sum(1)
        assert np.all(np.abs(sums - want) <= 1e-12 * np.abs(want)), (layout, D)
        assert np.all(ft[:, :first] == -1.0) and np.all(ft[:, first:, 7] == 480)
        per_frame = R.terms(r[:, n - D], x[:, n - D], y[:, n]).reshape(n_rows, T - first, 480, 8).sum(2)
        assert np.all(np.abs(ft[:, first:] - per_frame) <= 1e-12 * np.abs(per_frame))


# ---- the kernel body on the host, under the sanitizers ----
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("audio_score_emul") / "audio_score_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "csrc"),
                    "-I", os.path.join(PKG, "csrc", "score"), os.path.join(ROOT, "tests", "csrc", "audio_score_main.cpp"), "-o", exe], check=True)
    return exe


def run_emul(exe, tmp, ref, inp, out, n_rows, T, D, first, cuts, sums, ft):
    job, res = str(tmp / "job.bin"), str(tmp / "out.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("16q", n_rows, T, D, first, len(cuts), ref[1], ref[2], ref[0].size, inp[1], inp[2], inp[0].size,
                            out[1], out[2], out[0].size, 1 if ft is not None else 0, 0))
        f.write(np.asarray(cuts, np.int64).tobytes())
        for p in (ref, inp, out):
            f.write(p[0].tobytes())
        f.write(sums.tobytes())
        if ft is not None:
            f.write(ft.tobytes())
    r = subprocess.run([exe, job, res], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(res, np.float64)
    return raw[:sums.size].reshape(sums.shape), (raw[sums.size:].reshape(ft.shape) if ft is not None else None)


@pytest.mark.parametrize("layout", ["frames", "streams"])
@pytest.mark.parametrize("n_rows", [1, 3])
def test_kernel_body_on_the_host_under_sanitizers(emul, tmp_path, n_rows, layout):
    T = 5
    rng = np.random.default_rng(100 * n_rows + len(layout))
    ref, inp, out = planes(rng, n_rows, T, layout)
    for D in (0, 1, 479, 480, 960, 963):
        first = -(-D // 480)
        sums0 = rng.uniform(-1e6, 1e6, (n_rows, 8))
        want, want_ft = sums0.copy(), np.full((n_rows, T, 8), -7.0)
        R.score(ref, inp, out, n_rows, 0, T, first, D, want, want_ft)
        for cuts in ([(0, 5)], [(0, 1), (1, 4)]):
            got, got_ft = run_emul(emul, tmp_path, ref, inp, out, n_rows, T, D, first, cuts, sums0.copy(), np.full((n_rows, T, 8), -7.0))
            assert_bits_equal(got.view(np.uint64), want.view(np.uint64), f"sums, D={D}, cuts={cuts}")
            assert_bits_equal(got_ft.view(np.uint64), want_ft.view(np.uint64), f"frame records, D={D}, cuts={cuts}")
        if n_rows >= 2:  # the NaN stays in its row
            assert np.isnan(want[n_rows - 1]).any() and not np.isnan(want[:n_rows - 1]).any()
    got, _ = run_emul(emul, tmp_path, ref, inp, out, n_rows, T, 960, 2, [(0, 5)], np.zeros((n_rows, 8)), None)  # no frame records
    assert_bits_equal(got.view(np.uint64), R.score(ref, inp, out, n_rows, 0, T, 2, 960, np.zeros((n_rows, 8))).view(np.uint64), "without records")


# ---- the delay ----
def test_the_denoiser_delays_by_960_samples(blob_default):
    """the constant of the header: the oracle's output correlates best with its input 960 samples earlier"""
    from oracle.binding import Oracle
    streams, T = [3, 77, 130], 40
    pcm = synth.batch_pcm(streams, T)
    for i, s in enumerate(streams):
        x = pcm[:, i].astype(np.float64).reshape(-1)
        y = Oracle(blob_default).run(pcm[:, i])["out"].astype(np.float64).reshape(-1)
        n = x.size - 1500
        corr = np.array([np.dot(y[lag:lag + n], x[:n]) / np.sqrt(np.dot(y[lag:lag + n], y[lag:lag + n]) * np.dot(x[:n], x[:n]))
                         for lag in range(1500)])
        assert int(np.argmax(corr)) == A.DELAY == 960, (s, int(np.argmax(corr)))


# ---- the command line ----
def test_eval_audio_arguments_and_table(monkeypatch, capsys):
    sums = np.array([[400., 500., 404., 400., 400., 100., 4., 960.], [0., 5., 1., 0., 0., 5., 1., 960.], [100., 300., 150., 100., 100., 200., 50., 960.]])
    better = sums.copy()
    better[:, 6] /= 10
    canned = [dict(A.summary(A.metrics(s)), seg_snr_in=1.5, seg_snr_out=v) for s, v in ((sums, 4.25), (better, 6.5))]
    seen = {}

    def fake(*args):
        seen["args"] = args
        return ["a.blob", "ckpt.pth"], canned
    monkeypatch.setattr(cli, "eval_audio_files", fake)
    cli.main(["eval-audio", "s.pcm", "n.pcm", "f.pcm", "--model", "a.blob", "--checkpoint", "ckpt.pth", "--count", "9", "--frames", "30",
              "--seed", "4", "--streams", "4", "--rir-list", "rirs.txt"])
    assert seen["args"] == ("s.pcm", "n.pcm", "f.pcm", ["a.blob"], 9, 30, "ckpt.pth", None, "rirs.txt", 4, 4, 0)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("eval-audio: 9 sequences of 30 frames")
    head, a, b, d = lines[1:]
    assert head.split()[:4] == ["model", "seqs", "left", "out"] and "SI-SDR out" in head and "segSNR out" in head
    assert a.split()[:3] == ["a.blob", "2", "1"] and b.split()[:3] == ["ckpt.pth", "2", "1"] and d.split()[:2] == ["d", "ckpt.pth"]
    va, vb, vd = ([float(v) for v in ln.split()[-8:]] for ln in (a, b, d))
    assert va[0] == pytest.approx((10 * np.log10(4) + 10 * np.log10(.5)) / 2, abs=1e-3) and va[1] == pytest.approx((20 + 10 * np.log10(2)) / 2, abs=1e-3)
    assert vb[1] == pytest.approx(va[1] + 10, abs=2e-3) and vd[1] == pytest.approx(10.0, abs=2e-3) and vd[0] == 0.0
    assert va[7] == 4.25 and vb[7] == 6.5 and vd[7] == 2.25
    for argv in (["eval-audio", "s", "n", "f", "--count", "3"], ["eval-audio", "s", "n", "f", "--model", "a"],
                 ["eval-audio", "s", "n", "f", "--model", "a", "--count", "0"], ["eval-audio", "s", "n", "--model", "a", "--count", "1"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    # the other commands parse as before
    with pytest.raises(SystemExit):
        cli.main(["eval-records"])
