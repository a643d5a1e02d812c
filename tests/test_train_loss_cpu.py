"""CPU checks of the train library (include/rnnoise_amd_train.h, rnnoise_amd/csrc/train/train_loss.hip, rnnoise_amd/train_loss.py):
what it declares, exports and refuses; that the product libraries know nothing of it; and the two kernel bodies on the host under the
address and undefined-behaviour sanitizers, lane after lane, against the float64 torch reference (tests/train_loss_ref.py).  (The
kernels themselves: tests/test_train_loss_gpu.py.)

The gain gradient's bound is |got - ref| <= ulp32(ref) + K 2^-52 S (train_loss_ref.gain_scale: S multiplies the difference of the two
powers, which cancels).  Measured K, the largest (|got - ref| - ulp32(ref)) / (2^-52 S), against the float64 reference: the host
program (glibc pow / tanh) 0.990 on the case set and 0.000 on 10^5 random cases (every one within one ulp32 of the reference); the
device (MI355X, the device library's pow / tanh) 0.987 and 0.000.  The largest excess sits in the case set's p = float32(tg) cases,
where the two powers cancel to their last bits.  Asserted: 4 x the larger, K = 3.96 (the cap is 64)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import train_loss_ref as R
from conftest import assert_bits_equal
from rnnoise_amd import capi
from rnnoise_amd import train_loss as TL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
HEADER = os.path.join(ROOT, "include", "rnnoise_amd_train.h")


def _declarations():
    src = open(HEADER).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return [(" ".join(ret.split()), name, " ".join(params.split()))
            for ret, name, params in re.findall(r"RNNOISE_EXPORT\s+([\w\s\*]+?)\b(rnnoise_\w+)\s*\(([^()]*)\)\s*;", src)]


# ---- the surface ----
def test_prototype_table_matches_the_header():
    decl = _declarations()
    assert [d[1] for d in decl] == list(TL.PROTOTYPES) == TL.EXPORTS and len(decl) == 3
    for ret, name, params in decl:
        restype, argtypes = TL.PROTOTYPES[name]
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == params.count(",") + 1, (name, params)
    src = open(HEADER).read()
    for macro, value in (("RECORD", TL.RECORD), ("BANDS", TL.BANDS), ("SUMS", TL.SUMS), ("FRAME_BLOCK", TL.FRAME_BLOCK)):
        assert int(re.search(rf"#define RNNOISE_AMD_TRAIN_{macro} (\d+)", src)[1]) == value, macro
    assert (TL.RECORD, TL.BANDS, TL.SUMS) == (capi.REC, capi.NB_BANDS, capi.EVAL_SUMS) == (R.REC, R.BANDS, 4)
    # the structure: field for field, type for type
    body = re.search(r"typedef struct RNNoiseTrainLoss \{(.*?)\} RNNoiseTrainLoss;", src, re.S)[1]
    fields = []
    for decl_ in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        if decl_.strip():
            kind = re.match(r"\s*(const float|float|long|int|double)\b", decl_)[1]
            for f in decl_.strip()[len(kind):].split(","):
                f = f.strip()
                ctype = C.c_void_p if f.startswith("*") else {"long": C.c_long, "int": C.c_int, "double": C.c_double}[kind]
                fields.append((f.lstrip("*"), ctype))
    assert fields == list(TL.Call._fields_)
    assert C.sizeof(TL.Call) == 3 * 24 + 16 + 16 + 24


def test_library_exports_the_header_and_nothing_else():
    nm = subprocess.run(["nm", "-D", "--defined-only", TL.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert syms == set(TL.EXPORTS), sorted(syms ^ set(TL.EXPORTS))
    L = TL.lib()
    assert all(hasattr(L, n) for n in TL.EXPORTS)


def test_two_kernels_of_its_own_and_nothing_in_the_product():
    strings = lambda p: subprocess.run(["strings", "-a", p], capture_output=True, text=True, check=True).stdout
    own = strings(TL.LIB_PATH)
    assert set(re.findall(r"\b(rn_\w+)\.kd\b", own)) == set(TL.KERNELS) == {"rn_train_loss_kernel", "rn_train_loss_sums_kernel"}
    assert not re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", own)  # no environment variable
    for name in ("librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so", "librnnoise_amd_score.so"):
        text = strings(os.path.join(PKG, name))
        assert "train_loss" not in text, name
    ldd = subprocess.run(["ldd", TL.LIB_PATH], capture_output=True, text=True).stdout
    assert "librnnoise" not in ldd
    # nothing of it in the product's headers, prototype table or source lists; the shared header is among the product's
    assert "train_loss" not in open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    assert not [n for n in capi.PROTOTYPES if "train_loss" in n]
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    for var in ("SRCS", "ISRCS", "FLAGS"):
        assert "train_loss" not in re.search(rf"^{var}\s*:=\s*(.*)$", mk, re.M)[1], var
    assert "eval_terms.h" in re.search(r"^HDRS\s*:=\s*(.*)$", mk, re.M)[1].split()
    # one text for the terms: neither unit keeps a copy of its own
    for unit in ("dsp_kernels.hip", os.path.join("train", "train_loss.hip")):
        text = open(os.path.join(PKG, "csrc", unit)).read()
        assert "eval_terms.h" in text and "struct EvalTerms" not in text, unit


# ---- the argument check ----
def _call(**kw):
    """a call that is accepted: 3 rows, steps 4 .. 13 of [frame][row] buffers at made-up addresses (nothing is dereferenced)"""
    d = dict(records=(4096, 3 * 98, 98), gains=(8192, 3 * 32, 32), vad=(12288, 3, 1), n_rows=3, t0=4, n_frames=10, first=4, gamma=.25,
             w_gain=1e-3, w_vad=1e-5, grad_gains=16384, grad_vad=20480)
    d.update(kw)
    return TL.make_call(**d)


REFUSED = dict(
    null_records=dict(records=(0, 294, 98)), null_gains=dict(gains=(0, 96, 32)), null_vad=dict(vad=(0, 3, 1)),
    no_rows=dict(n_rows=0), negative_rows=dict(n_rows=-1), negative_t0=dict(t0=-1), negative_frames=dict(n_frames=-1),
    negative_first=dict(first=-1), frames_overflow=dict(t0=2 ** 31 - 5, n_frames=10),
    gamma_zero=dict(gamma=0.0), gamma_negative=dict(gamma=-.25), gamma_inf=dict(gamma=float("inf")), gamma_nan=dict(gamma=float("nan")),
    w_gain_inf=dict(w_gain=float("inf")), w_gain_nan=dict(w_gain=float("nan")), w_vad_inf=dict(w_vad=float("-inf")),
    w_vad_nan=dict(w_vad=float("nan")),
    grad_gains_alone=dict(grad_vad=0), grad_vad_alone=dict(grad_gains=0),
    rec_rows_overlap=dict(records=(4096, 294, 97)), rec_frames_overlap=dict(records=(4096, 293, 98)),
    gain_rows_overlap=dict(gains=(8192, 96, 31)), gain_frames_overlap=dict(gains=(8192, 95, 32)),
    gain_row_major_short=dict(gains=(8192, 32, 32 * 9)),  # [row][step] with rows of 9 steps for a call of 10
    vad_overlap=dict(vad=(12288, 2, 1)), vad_same_slot=dict(vad=(12288, 1, 1)),
    stride_zero=dict(gains=(8192, 0, 0)), stride_negative=dict(records=(4096, -294, 98)), extent_overflow=dict(records=(4096, 2 ** 62, 98)),
)
ACCEPTED = (dict(), dict(grad_gains=0, grad_vad=0), dict(n_frames=0), dict(t0=0, first=0), dict(t0=2 ** 31 - 11, n_frames=10, records=(4096, 98, 2 ** 40),
            gains=(8192, 32, 320), vad=(12288, 1, 10)), dict(gains=(8192, 32, 320), vad=(12288, 1, 10), records=(4096, 98, 98 * 13)),
            dict(gains=(8192, 40, 10 * 40 + 7)), dict(w_gain=0.0, w_vad=-1.0), dict(gamma=1.0), dict(n_rows=1, vad=(12288, 1, 1)),
            dict(first=1000))


def test_check_accepts_and_refuses():
    assert TL.lib().rnnoise_amd_train_loss_check(None) == -1
    for kw in ACCEPTED:
        assert TL.check(_call(**kw)), kw
    for name, kw in REFUSED.items():
        assert not TL.check(_call(**kw)), name


def test_calls_refuse_before_they_touch_a_pointer():
    """every pointer of these calls is a made-up address: a call that looked at one would not come back"""
    L = TL.lib()
    for name, kw in REFUSED.items():
        call = _call(**kw)
        assert L.rnnoise_amd_train_loss_device(0, C.c_void_p(64), C.c_void_p(128), C.byref(call), None) == -1, name
        assert L.rnnoise_amd_train_loss(0, C.cast(C.c_void_p(64), TL._dp), None, C.byref(call)) == -1, name
    ok = _call()
    assert L.rnnoise_amd_train_loss_device(0, None, C.c_void_p(128), C.byref(ok), None) == -1  # no sums
    assert L.rnnoise_amd_train_loss_device(0, C.c_void_p(64), None, C.byref(ok), None) == -1   # no workspace in the device form
    assert L.rnnoise_amd_train_loss(0, None, None, C.byref(ok)) == -1
    assert L.rnnoise_amd_train_loss_device(0, None, None, None, None) == -1 and L.rnnoise_amd_train_loss(0, None, None, None) == -1
    with pytest.raises(ValueError):
        TL.loss_device(64, 128, _call(gamma=0.0))


# ---- the kernel bodies on the host, under the sanitizers ----
@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_loss_emul") / "train_loss_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "csrc"), "-I", os.path.join(PKG, "csrc", "train"),
                    os.path.join(ROOT, "tests", "csrc", "train_loss_main.cpp"), "-o", exe], check=True)
    return exe


def run_emul(exe, tmp, rec, gains, vad, t_base, first, cuts, sums, gamma=.25, w_gain=0.0, w_vad=0.0, grads=True):
    """rec, gains, vad: (steps, rows, width) views (train_loss_ref.lay_out); gains / vad hold steps t_base ..; cuts: (t0, n_frames)
    -> sums, grad_gains, grad_vad as views of the layout of gains / vad over what the program wrote (gaps included)"""
    n_rows = gains.shape[1]

    def flat(view):  # the floats from the view's first to the end of its last slot
        fs, rs = R.strides_of(view)
        n = (view.shape[0] - 1) * fs + (view.shape[1] - 1) * rs + view.shape[2]
        return np.lib.stride_tricks.as_strided(view, (n,), (view.itemsize,))
    vad3 = vad.reshape(vad.shape[0], n_rows, 1) if vad.ndim == 2 else vad
    bufs = [flat(rec), flat(gains), flat(vad3)]
    job, res = str(tmp / "job.bin"), str(tmp / "out.bin")
    with open(job, "wb") as f:
        f.write(struct.pack("16q", n_rows, t_base, first, len(cuts), *R.strides_of(rec), bufs[0].size, *R.strides_of(gains), bufs[1].size,
                            *R.strides_of(vad3), bufs[2].size, 1 if grads else 0, 0, 0))
        f.write(struct.pack("3d", gamma, w_gain, w_vad))
        f.write(np.asarray(cuts, np.int64).tobytes())
        for b in bufs:
            f.write(b.tobytes())
        f.write(sums.tobytes())
    r = subprocess.run([exe, job, res], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(res, "rb").read()
    got = np.frombuffer(raw[:sums.nbytes], np.float64).reshape(sums.shape)
    if not grads:
        assert len(raw) == sums.nbytes
        return got, None, None
    fl = np.frombuffer(raw[sums.nbytes:], np.float32)
    assert fl.size == bufs[1].size + bufs[2].size
    as_view = lambda flat_, like: np.lib.stride_tricks.as_strided(flat_, like.shape, like.strides)
    return got, as_view(fl[:bufs[1].size], gains), as_view(fl[bufs[1].size:], vad3)[..., 0]


FB = TL.FRAME_BLOCK
W_GAIN, W_VAD = R.W_GAIN, R.W_VAD


check_against_reference = R.check_against_reference


@pytest.mark.parametrize("layout", ["frames", "rows", "padded"])
def test_kernel_bodies_on_the_host_under_sanitizers(emul, tmp_path, layout):
    n_rows, T = 3, 2 * FB + 3 + 4
    rec, gains, vad, _ = R.case_buffers(n_rows, T)
    gains, vad = gains[4:], vad[4:]  # the predictions of steps 4 ..: what the float network gives
    rec_l, gains_l, vad_l = R.lay_out(rec, layout), R.lay_out(gains, layout), R.lay_out(vad[..., None], layout)
    sums0 = np.random.default_rng(3).uniform(-1e3, 1e3, (n_rows, 4))
    sums0[:, 3] = 0
    n = T - 4
    whole = run_emul(emul, tmp_path, rec_l, gains_l, vad_l, 4, 4, [(4, n)], sums0.copy(), w_gain=W_GAIN, w_vad=W_VAD)
    zero = run_emul(emul, tmp_path, rec_l, gains_l, vad_l, 4, 4, [(4, n)], np.zeros((n_rows, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    check_against_reference(rec, gains, vad, 4, 4, zero[0], zero[1], zero[2], R.GRAD_K, layout)
    # uneven cuts: the bits of one call, sums and gradients; sums only: the same sums, no gradient buffer at all
    cut = run_emul(emul, tmp_path, rec_l, gains_l, vad_l, 4, 4, [(4, 1), (5, FB), (5 + FB, 0), (5 + FB, n - FB - 1)], sums0.copy(),
                   w_gain=W_GAIN, w_vad=W_VAD)
    assert_bits_equal(cut[0].view(np.uint64), whole[0].view(np.uint64), "sums of uneven cuts")
    assert_bits_equal(np.ascontiguousarray(cut[1]).view(np.uint32), np.ascontiguousarray(whole[1]).view(np.uint32), "gain gradients of uneven cuts")
    assert_bits_equal(np.ascontiguousarray(cut[2]).view(np.uint32), np.ascontiguousarray(whole[2]).view(np.uint32), "vad gradients of uneven cuts")
    only, _, _ = run_emul(emul, tmp_path, rec_l, gains_l, vad_l, 4, 4, [(4, n)], sums0.copy(), grads=False)
    assert_bits_equal(only.view(np.uint64), whole[0].view(np.uint64), "sums without gradients")


def test_unscored_steps_and_a_later_start_on_the_host(emul, tmp_path):
    n_rows, T = 2, 12
    rec, gains, vad, _ = R.case_buffers(n_rows, T)
    # t0 = 0, first = 4: four unscored steps that must be zeros; t0 = 7: reads record 6
    a = run_emul(emul, tmp_path, rec, gains, vad[..., None], 0, 4, [(0, T)], np.zeros((n_rows, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    check_against_reference(rec, gains, vad, 0, 4, *a, R.GRAD_K, "t0 = 0")
    assert np.all(a[1][:4] == 0) and np.all(a[2][:4] == 0) and np.all(a[0][:, 2] == T - 4)
    b = run_emul(emul, tmp_path, rec, gains[7:], vad[7:, :, None], 7, 4, [(7, T - 7)], np.zeros((n_rows, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    check_against_reference(rec, gains[7:], vad[7:], 7, 4, *b, R.GRAD_K, "t0 = 7")
    assert_bits_equal(np.ascontiguousarray(b[1]).view(np.uint32), np.ascontiguousarray(a[1][7:]).view(np.uint32), "the same steps from t0 = 7")
    # first = 0 scores from step 1 (step 0 has no record); a call wholly below `first` scores nothing and zeroes its gradients
    c = run_emul(emul, tmp_path, rec, gains, vad[..., None], 0, 0, [(0, T)], np.zeros((n_rows, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    assert np.all(c[0][:, 2] == T - 1) and np.all(c[1][0] == 0) and np.all(c[2][0] == 0)
    d = run_emul(emul, tmp_path, rec, gains, vad[..., None], 0, 9, [(0, 5)], np.ones((n_rows, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    assert np.all(d[0] == 1) and np.all(d[1][:5] == 0) and np.all(d[1][5:] == -7) and np.all(d[2][:5] == 0) and np.all(d[2][5:] == -7)


def test_the_case_set_is_covered_and_k_is_within_the_asserted_bound(emul, tmp_path):
    """the whole cross product of the value lists, then 10^5 random cases: the measured K of the host program (printed; the
    docstring of this module records it beside the device's) under the asserted one"""
    n_rows, T = 67, 2 * FB + 3 + 1
    rec, gains, vad, cover = R.case_buffers(n_rows, T)
    assert len(cover) == len(R.COMBOS) * len(R.FRAME_KINDS) == 420
    got = run_emul(emul, tmp_path, rec, gains[1:], vad[1:, :, None], 1, 1, [(1, T - 1)], np.zeros((n_rows, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    k_set = check_against_reference(rec, gains[1:], vad[1:], 1, 1, *got, R.GRAD_K, "case set")
    rng = np.random.default_rng(11)
    rec, gains, vad = R.random_buffers(rng, 25, 126)  # 25 x 125 scored steps x 32 bands = 10^5
    got = run_emul(emul, tmp_path, rec, gains[1:], vad[1:, :, None], 1, 1, [(1, 125)], np.zeros((25, 4)), w_gain=W_GAIN, w_vad=W_VAD)
    want, rg, rv = R.reference(rec, gains[1:], vad[1:], 1, 1, .25, W_GAIN, W_VAD)
    S = R.gain_scale(rec, gains[1:], 1, 1, .25, W_GAIN)
    k_rand = R.measured_k(got[1], rg, S)
    print(f"measured K on the host: case set {k_set:.3f}, random {k_rand:.3f}; asserted {R.GRAD_K}")
    assert np.all(np.abs(got[1].astype(np.float64) - rg) <= R.ulp32(rg) + R.GRAD_K * 2.0 ** -52 * S)
    assert np.all(np.abs(got[2].astype(np.float64) - rv) <= R.vad_bound(rec, vad[1:], 1, 1, W_VAD, rv))
    assert np.all(np.abs(got[0][:, :2] - want[:, :2]) <= 1e-12 * np.abs(want[:, :2]))
    assert max(k_set, k_rand) <= R.GRAD_K <= 64
