"""The training-mix calls without a GPU (include/rnnoise_amd.h: RNNoiseTrainMix; the reference's src/dump_features.c:408-465).

  a  tests/csrc/mix_oracle.c -- what the GPU tests compare against -- equals the reference's own rnn_biquad, weighted_rms, clear_vad
     and viterbi_vad (tests/csrc/ref_dump_harness.c, compiled where the reference's sources are) on 2000-frame sequences
  b  rnnoise_amd_train_vad: the reference at 2000 frames, the oracle at other lengths, the start_pos rule
  c  rnnoise_amd_train_mix_check, the struct's layout, NULL arguments
  d  train_data.draw: ranges, branch frequencies, the band_lp carry-over
  e  the kernels' own source run on the host under the address sanitizer (tests/csrc/hip_emul), against the oracle
(the kernels of train_mix.hip by name, without scratch or spills: tests/test_product_surface_cpu.py, tests/test_kernel_budgets_cpu.py)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mix_oracle as mo
from conftest import ROOT, assert_bits_equal
from rnnoise_amd import capi, train_data
from train_support import T_REF, reference_dump_features, run_kernel_emul

N_REF = T_REF * 480
B_HP, A_HP = (-2, 1), (-1.99599, 0.99600)
# one coefficient pair per branch of rand_filt (dump_features.c:159-178): none, a complex pair, two real roots
FILTERS = {"zero": (0.0, 0.0), "complex": (-2 * .55 * np.cos(.9), .55 * .55), "real": (-.62 + .31, -.62 * .31)}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the reference's functions (tests/csrc/ref_dump_harness.c: train_support.reference_dump_features)"""
    L = reference_dump_features(tmp_path_factory.mktemp("ref_dump"))
    if isinstance(L, str):
        pytest.skip(L)
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def ref_biquad(L, x, b, a):
    x = np.ascontiguousarray(x, np.float32)
    y, mem = np.empty_like(x), np.zeros(2, np.float32)
    b, a = np.asarray(b, np.float32), np.asarray(a, np.float32)
    L.refm_biquad(_fp(y), _fp(mem), _fp(x), _fp(b), _fp(a), len(x))
    return y


@pytest.fixture(scope="module")
def signal():
    """a 2000-frame int16 sequence as floats: noise under a slow envelope, with full-scale stretches and silences"""
    rng = np.random.default_rng(20)
    env = np.repeat(rng.choice([0.0, 30.0, 900.0, 9000.0, 40000.0], T_REF // 20), 20 * 480)
    x = np.clip(np.rint(rng.standard_normal(N_REF) * env), -32768, 32767).astype(np.int16).astype(np.float32)
    x.setflags(write=False)
    return x


# ---- a. the oracle against the reference ----
@pytest.mark.parametrize("branch", list(FILTERS))
def test_oracle_biquad_chain_is_the_references(ref, signal, branch):
    """the high-pass, then a filter of each rand_filt branch as numerator and as denominator, then the weighting filter's level"""
    c = FILTERS[branch]
    hp_o, hp_r = mo.biquad(signal, B_HP, A_HP), ref_biquad(ref, signal, B_HP, A_HP)
    assert_bits_equal(hp_o, hp_r, "high-pass")
    for b, a in ((c, FILTERS["zero"]), (FILTERS["zero"], c), (c, FILTERS["complex"])):
        y_o, y_r = mo.biquad(hp_o, b, a), ref_biquad(ref, hp_r, b, a)
        assert np.isfinite(y_r).all() and np.abs(y_r).max() > 1000
        assert_bits_equal(y_o, y_r, f"{branch}: b={b} a={a}")
        want = np.float32(ref.refm_weighted_rms(_fp(np.array(y_r))))
        assert_bits_equal(np.array([mo.weighted_rms(y_o)]), np.array([want]), f"{branch}: weighted_rms")


def _tracks():
    """VAD tracks of 2000 frames: one that starts silent and takes every action of clear_vad -- zero, fade in, keep, fade out, zero
    again, a fade in on the last but one frame --, one that starts active, one that is active to the end, one all silent"""
    a = np.zeros(T_REF, np.int32)
    a[5:9] = 1
    a[40:41] = 1
    a[42:60] = 1          # (a one-frame gap is kept: fading out takes two silent frames)
    a[T_REF - 1] = 1
    b = a.copy()
    b[0:3] = 1
    c = np.ones(T_REF, np.int32)
    c[100:300] = 0
    return {"silent start": a, "active start": b, "active end": c, "all silent": np.zeros(T_REF, np.int32)}


def clear_vad_actions(vad):
    """the action clear_vad takes on every frame (0 keep, 1 zero, 2 fade in, 3 fade out), from its definition"""
    act, on = [], vad[0]
    for i in range(len(vad)):
        if not on:
            if i < len(vad) - 1 and vad[i + 1]:
                act.append(2)
                on = 1
            else:
                act.append(1)
        elif i >= 1 and vad[i] == 0 and vad[i - 1] == 0:
            act.append(3)
            on = 0
        else:
            act.append(0)
    return np.array(act)


@pytest.mark.parametrize("name", list(_tracks()))
def test_oracle_clear_vad_is_the_references(ref, signal, name):
    vad = _tracks()[name]
    if name == "silent start":
        assert set(clear_vad_actions(vad)) == {0, 1, 2, 3}
    if name == "active start":
        assert clear_vad_actions(vad)[0] == 0
    x = signal + np.float32(0.25)
    want = x.copy()
    ref.refm_clear_vad(_fp(want), _ip(vad.copy()))
    assert_bits_equal(mo.clear_vad(x, vad), want, name)


def _energies(T):
    rng = np.random.default_rng(21)
    loud = (rng.random(T) * 1e10 + 1e8).astype(np.float32)
    quiet = (rng.random(T) * 40).astype(np.float32)
    alt = np.where((np.arange(T) // 3) % 2 == 0, 0, 3e9).astype(np.float32)
    speech = (np.repeat(rng.choice([0.0, 2e4, 5e9, 8e10], -(-T // 25)), 25)[:T] * rng.random(T)).astype(np.float32)
    return {"loud": loud, "quiet": quiet, "zero": np.zeros(T, np.float32), "alternating": alt, "speech": speech}


@pytest.mark.parametrize("name", list(_energies(4)))
def test_oracle_and_library_viterbi_are_the_references(ref, name):
    E = _energies(T_REF)[name]
    want = np.zeros(T_REF, np.int32)
    ref.refm_viterbi_vad(_fp(E), _ip(want))
    if name == "speech":  # (the track has both states and changes between them)
        assert 0 < want.sum() < T_REF and (np.diff(want) != 0).sum() > 10
    assert (mo.viterbi(E) == want).all(), name
    assert (capi.train_vad(E[None])[0] == want).all(), name


# ---- b. rnnoise_amd_train_vad ----
@pytest.mark.parametrize("T", [1, 2, 7, 300])
def test_train_vad_is_the_oracle_at_other_lengths(T):
    names = list(_energies(T))
    E = np.stack([_energies(T)[n] for n in names] * 4)
    start = np.repeat([0, 479, 480, 480 * T + 5000], len(names)).astype(np.int32)
    got = capi.train_vad(E, start)
    assert got.shape == (len(E), T) and got.dtype == np.uint8
    for s in range(len(E)):
        assert (got[s] == mo.vad(E[s], start[s])).all(), (names[s % len(names)], start[s])
        plain = mo.viterbi(E[s])
        lead = min(start[s] // 480, T)
        assert (got[s, :lead] == 0).all() and (got[s, lead:] == plain[lead:]).all()
    assert (capi.train_vad(E) == capi.train_vad(E, np.zeros(len(E), np.int32))).all()   # start_pos NULL: nothing cleared
    assert got[np.arange(len(E)) // len(names) == 0].any()


def test_train_vad_refuses_null_and_empty():
    L = capi.lib()
    E, v = np.zeros(4, np.float32), np.zeros(4, np.uint8)
    vp = v.ctypes.data_as(C.POINTER(C.c_ubyte))
    assert L.rnnoise_amd_train_vad(None, 1, 4, None, vp) == -1
    assert L.rnnoise_amd_train_vad(_fp(E), 1, 4, None, None) == -1
    assert L.rnnoise_amd_train_vad(_fp(E), 0, 4, None, vp) == -1
    assert L.rnnoise_amd_train_vad(_fp(E), 1, 0, None, vp) == -1
    assert L.rnnoise_amd_train_vad(_fp(E), 1, 4, None, vp) == 0


# ---- c. the check, the struct, NULL ----
def _table(n, lens, T):
    t = np.zeros(n, capi.MIX_DTYPE)
    t["speech_gain"], t["noise_gain"], t["fgnoise_gain"] = .1, .02, .03
    t["a_sig"] = FILTERS["complex"]
    return t


def test_check_accepts_the_boundaries_and_refuses_beyond():
    lens, T = (480 * 9 + 1, 480 * 7, 480 * 8 + 3), 7
    ok = lambda t: capi.train_mix_check(t, lens, T)
    t = _table(3, lens, T)
    assert ok(t)
    t["speech_pos"], t["noise_pos"], t["fgnoise_pos"] = [0, 480 * 2 + 1, 7], 0, [480 + 3, 0, 1]
    assert ok(t)
    for k, name in enumerate(("speech_pos", "noise_pos", "fgnoise_pos")):
        for bad in (lens[k] - 480 * T + 1, -1, 2 ** 40):
            u = t.copy()
            u[name][2] = bad
            assert not ok(u), (name, bad)
    for name in ("speech_gain", "noise_gain", "fgnoise_gain"):
        u = t.copy()
        u[name][1] = np.nan
        assert not ok(u), name
    for name in ("a_sig", "b_sig", "a_noise", "b_noise", "a_fgnoise", "b_fgnoise"):
        for v in (np.inf, -np.inf, np.nan):
            u = t.copy()
            u[name][0, 1] = v
            assert not ok(u), (name, v)
    for name in ("clip", "quantize"):
        for v, good in ((1, True), (2, False), (-1, False)):
            u = t.copy()
            u[name][1] = v
            assert ok(u) == good, (name, v)
    assert not capi.train_mix_check(t, lens, 8)          # the noise corpus holds 7 frames
    assert not capi.train_mix_check(t, lens, 0)
    L = capi.lib()
    assert L.rnnoise_amd_train_mix_check(None, 3, *lens, T) == 0
    assert L.rnnoise_amd_train_mix_check(t.ctypes.data, 0, *lens, T) == 0


def test_struct_layout_is_the_headers(tmp_path):
    names = [f[0] for f in capi.TrainMix._fields_]
    prog = tmp_path / "probe.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnnoise_amd.h"\nint main(void) {\n'
                    '  printf("%zu\\n", sizeof(RNNoiseTrainMix));\n'
                    + "".join(f'  printf("%zu\\n", offsetof(RNNoiseTrainMix, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(capi.TrainMix) == capi.MIX_DTYPE.itemsize
    assert out[1:] == [getattr(capi.TrainMix, n).offset for n in names] == [capi.MIX_DTYPE.fields[n][1] for n in names]


def test_null_batch_calls_fail():
    L = capi.lib()
    assert {"rnnoise_amd_train_mix_check", "rnnoise_batch_train_levels_device", "rnnoise_amd_train_vad",
            "rnnoise_batch_train_mix_device"} <= set(capi.EXPORTS)
    t = _table(1, (4800,) * 3, 2)
    p = 4096  # (never dereferenced: the batch is checked first)
    assert L.rnnoise_batch_train_levels_device(None, p, p, p, p, p, 4800, 4800, 4800, t.ctypes.data, 2, None) == -1
    assert L.rnnoise_batch_train_mix_device(None, p, p, p, p, p, p, p, 4800, 4800, 4800, t.ctypes.data, p, p, 2, None) == -1


# ---- d. draw() ----
class Recording:
    """a Generator that keeps the matrix of uniform numbers draw() asks for, or hands out a prepared one"""

    def __init__(self, seed=None, forced=None):
        self.rng, self.u = np.random.default_rng(seed), forced

    def random(self, size):
        if self.u is None:
            self.u = self.rng.random(size)
        assert self.u.shape == tuple(size)
        return self.u


def test_draw_ranges_and_frequencies():
    n, T, lens = 20000, 2000, (480 * 2000 + 1, 480 * 2000 * 3 + 17, 10 ** 9)
    r = Recording(7)
    d = train_data.draw(r, n, lens, T)
    m, u = d.mix, r.u
    assert m.dtype == capi.MIX_DTYPE and capi.train_mix_check(m, lens, T)
    assert m["speech_pos"].min() >= 0 and m["speech_pos"].max() == 1          # a corpus one sample longer than a sequence
    assert (m["fgnoise_pos"] % 2 == 1).any() and m["fgnoise_pos"].max() > 9 * 10 ** 8
    assert (d.start_pos >= 0).all() and (d.start_pos <= 480 * T).all()
    sg = m["speech_gain"].astype(np.float64)
    assert (sg >= 10 ** (-45 / 20) * (1 - 1e-6)).all() and (sg <= 10 ** (10 / 20) * (1 + 1e-6)).all()
    quiet = u[:, train_data.U_QUIET] < 1 / 12
    for name in ("noise_gain", "fgnoise_gain"):
        ratio = m[name].astype(np.float64) / sg
        on = ratio != 0
        lo, hi = 10 ** (-30 / 20) * (1 - 1e-5), 10 ** (25 / 20) * (1 + 1e-5)
        assert ((ratio[on & ~quiet] >= lo) & (ratio[on & ~quiet] <= hi)).all()
        assert ((ratio[on & quiet] >= .03 * lo) & (ratio[on & quiet] <= .03 * hi)).all()
    assert (d.lowpass >= 60).all() and (d.lowpass <= 3006).all() and (d.lowpass > 1500).any()
    assert (d.band_lp >= 18).all() and (d.band_lp <= 32).all()  # (eband[18] = 68 is the first edge above the lowest lowpass, 60)
    filt = np.stack([m[k] for k in ("a_sig", "b_sig", "a_noise", "b_noise", "a_fgnoise", "b_fgnoise")], 1)   # (n, 6, 2)
    assert (np.abs(filt[..., 0]) <= 1.4 + 1e-6).all() and (filt[..., 1] <= .49 + 1e-6).all() and (filt[..., 1] >= -.49 - 1e-6).all()
    zero = (filt == 0).all(-1)
    assert (filt[~zero][:, 1] < 0).any() and (filt[~zero][:, 1] > 0).any()

    def near(count, total, p, what):
        sd = np.sqrt(total * p * (1 - p))
        assert abs(count - total * p) <= 5 * sd, (what, count, total * p, sd)
    near(zero.sum(), zero.size, 2 / 3, "zero filters")
    near((m["noise_gain"] == 0).sum(), n, 1 / 8, "noise_gain == 0")
    near((m["fgnoise_gain"] == 0).sum(), n, 7 / 8, "fgnoise_gain == 0")
    near(quiet.sum(), n, 1 / 12, "both noise gains * 0.03")
    near((m["clip"] == 1).sum(), n, 1 / 4, "clip")
    near((m["quantize"] == 1).sum(), n, 1 / 2, "quantize")
    near((d.start_pos == 0).sum(), n, 3 / 4, "start_pos == 0")
    assert set(np.unique(m["clip"])) == set(np.unique(m["quantize"])) == {0, 1}


def test_draw_band_lp_keeps_the_previous_sequences_value_when_no_band_is_above_lowpass():
    u = np.full((4, train_data.N_UNIFORM), .5)
    # lowpass = 60.125 * 50 ** u: 60 -> band 18 (the first edge above 60 is 68); 60.125 * 50 = 3006 is above every edge looked at
    u[:, train_data.U_LOWPASS] = [1.0 - 1e-12, 0.0, 1.0 - 1e-12, np.log(199.5 / 60.125) / np.log(50)]
    d = train_data.draw(Recording(forced=u), 4, (10 ** 6,) * 3, 20)
    assert list(d.lowpass) == [3006, 60, 3006, 199]
    assert list(d.band_lp) == [32, 18, 18, 28]          # 32 at the start; the third sequence keeps the second's 18
    assert train_data.band_lp_of(316, 5) == 31 and train_data.band_lp_of(317, 5) == 5
    d2 = train_data.draw(Recording(forced=u), 4, (10 ** 6,) * 3, 20, band_lp=7)
    assert list(d2.band_lp) == [7, 18, 18, 28]


# ---- e. the kernels' loops on the host ----
def test_kernel_source_on_the_host_stays_inside_its_buffers_and_gives_the_oracles_bits(tmp_path):
    """train_mix.hip compiled as plain C++ against a stand-in for shim.h (192 host threads per workgroup), a stand-alone program under
    the address and undefined-behaviour sanitizers: corpora and outputs of exact size, rows at even and odd addresses, a row that
    ends with its corpus, 1 / 65 / 70 sequences, 1 to 40 frames"""
    r = run_kernel_emul(tmp_path, "train_mix", "mix_main.cpp", "mix_oracle.c", [os.path.join(ROOT, "include")])
    assert r.returncode == 0 and r.stdout.strip().endswith("all equal"), r.stdout[-2000:] + r.stderr[-4000:]
