"""rnnoise_batch_train_levels_vad_device on the GPU (rnnoise_amd/csrc/train_mix.hip, include/rn_train_vad.h):
the Viterbi VAD as the epilogue of rn_train_levels, byte for byte rnnoise_amd_train_vad on the energies the same launch wrote.

  a  1 / 65 / 130 sequences of 7 frames, and 1, 2 and 300 frames: the row set of tests/csrc/hip_emul/vad_main.cpp (speech with silent
     stretches, digital silence, one loud frame, one repeated value, loud and zero frames in turn, a climbing level, quiet noise) at
     odd and even corpus positions, every start_pos case and none; energies and levels identical to the levels call; guard words
  b  chained into mix and feature extraction on a stream of the caller's without a host synchronisation, against TrainOracle; on
     a batch in per-stream frame phase with tables set
  c  the restated pow and log on the device against this host's libm: pow over its whole domain, log over 10^7 arguments
  d  the forced self-check failure refuses and touches nothing
  e  train_data.generate(vad="device") == generate(vad="host") == the oracles, with and without RIRs; the command line"""
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest

import mix_oracle as mo
from conftest import ROOT, assert_bits_equal, load_blob
from rnnoise_amd import capi, train_data
from train_support import guarded, guards_intact

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
KINDS = 7


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


def speech_row(kind, T, rng):
    """one sequence of T frames, int16: the kinds of tests/csrc/hip_emul/vad_main.cpp"""
    n = 480 * T
    r = rng.integers(-20000, 20001, n)
    f = np.arange(n) // 480
    if kind == 0:
        x = r * ((np.arange(n) // 700) % 3 != 0)
    elif kind == 1:
        x = np.zeros(n)
    elif kind == 2:
        x = r * (f == T // 2)
    elif kind == 3:
        x = ((np.arange(n) % 480) * 37) % 2001 - 1000
    elif kind == 4:
        x = r * ((f // 3) % 2 == 1)
    elif kind == 5:
        x = np.trunc(r * (f + 1.0) / T)
    else:
        x = np.trunc(r / 2000)
    return x.astype(np.int16)


def make_rows(n, T, seed):
    """(corpora, table, start_pos): sequence s is a row of kind s % 7 at an even (s even) or odd position of the speech corpus"""
    rng = np.random.default_rng(seed)
    span, stride = 480 * T, 480 * T + 2
    speech = np.zeros(stride * n, np.int16)
    t = np.zeros(n, capi.MIX_DTYPE)
    for s in range(n):
        at = s * stride + (s & 1)
        speech[at:at + span] = speech_row(s % KINDS, T, rng)
        t["speech_pos"][s] = at
    noise = rng.integers(-1000, 1001, span + 778).astype(np.int16)
    fg = rng.integers(-1000, 1001, span + 1).astype(np.int16)
    t["noise_pos"] = (np.arange(n) * 39 + 1) % (len(noise) - span + 1)
    t["fgnoise_pos"] = np.arange(n) & 1
    t["speech_gain"], t["noise_gain"], t["fgnoise_gain"] = 1.0, .5, np.where(np.arange(n) % 3, 0, .8)
    t["a_sig"] = (-0.6838, 0.3025)
    starts = np.array([0, 479, 480, 480 * (T // 2) + 7, 480 * T + 900, 961, 480 * T], np.int32)
    start = starts[(np.arange(n) // KINDS + np.arange(n)) % 7]
    return [speech, noise, fg], t, start


def levels_vad(b, d, table, T, start, stream=0, sync=torch.cuda.synchronize):
    """the new call and the existing levels call into guarded buffers -> (energy, rms, vad) of the new call, everything else checked"""
    n = len(table)
    bufs = {k: guarded(shape, dt) for k, shape, dt in (("energy", (n, T), torch.float32), ("rms", (n, 3), torch.float32),
                                                       ("vad", (n, T), torch.uint8), ("energy0", (n, T), torch.float32),
                                                       ("rms0", (n, 3), torch.float32))}
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    sync()
    b.train_levels_vad_device(p["energy"], p["rms"], p["vad"], d.ptrs, d.lens, table, start, T, stream)
    b.train_levels_device(p["energy0"], p["rms0"], d.ptrs, d.lens, table, T, stream)
    sync()
    for k, (buf, _, fill) in bufs.items():
        guards_intact(buf, fill, k)
    r = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    assert_bits_equal(r["energy"], r["energy0"], "energies of the call with the VAD and of the levels call")
    assert_bits_equal(r["rms"], r["rms0"], "levels of the call with the VAD and of the levels call")
    return r["energy"], r["rms"], r["vad"]


# ---- a. the rows, the sizes around the wave, the short and the long sequences ----
@pytest.mark.parametrize("n,T", [(1, 7), (65, 7), (130, 7), (65, 1), (65, 2), (14, 300)])
def test_vad_bytes_are_the_host_calls_on_the_same_energies(model, n, T):
    from test_train_mix_gpu import Device
    corpora, table, start = make_rows(n, T, 100 + n + T)
    assert capi.train_mix_check(table, [len(c) for c in corpora], T)
    d = Device(corpora)
    b = capi.Batch(model, n)
    energy, rms, vad = levels_vad(b, d, table, T, start)
    _, _, vad_null = levels_vad(b, d, table, T, None)
    b.close()
    d.corpora_unchanged()
    assert (vad == capi.train_vad(energy, start)).all()
    assert (vad_null == capi.train_vad(energy)).all()
    assert vad.max() <= 1
    if n >= KINDS:
        assert (energy[1] == 0).all() and (energy[5] != 0).all()                  # digital silence: log(0), NaN through the limits
        assert len(np.unique(energy[3])) == 1                                      # one repeated value
        if T > 2:
            assert (energy[2] != 0).sum() == 1 and (energy[4] == 0).any() and (energy[4] != 0).any()
            assert 0 < vad_null.sum() < vad_null.size
        assert (table["speech_pos"] % 2 == 0).any() and (table["speech_pos"] % 2 == 1).any()
        for s in range(n):
            assert (vad[s, :min(start[s] // 480, T)] == 0).all()
            assert (vad[s, min(start[s] // 480, T):] == vad_null[s, min(start[s] // 480, T):]).all()


def test_the_oracles_tracks_at_seven_frames(model):
    """the table of tests/test_train_mix_gpu.py, which tests/csrc/mix_oracle.c decodes: the same tracks from the device"""
    from test_train_mix_gpu import Device, make_corpora, make_table
    T, n = 7, 65
    corpora = make_corpora(T, 31)
    table = make_table(n, T, corpora, 32)
    start = ((np.arange(n) % 4 == 2) * (np.arange(n) * 53 % (480 * T + 900))).astype(np.int32)
    want = mo.batch(corpora, table, T, start)
    d = Device(corpora)
    b = capi.Batch(model, n)
    energy, rms, vad = levels_vad(b, d, table, T, start)
    b.close()
    assert_bits_equal(energy, want["energy"], "energy")
    assert_bits_equal(rms, want["rms"], "rms")
    assert (vad == want["vad"]).all()


# ---- b. chained, on a caller's stream, without a host synchronisation; a batch in per-stream frame phase ----
def _chain(model, features, prepare=None):
    from oracle.binding import TrainOracle
    from test_train_mix_gpu import Device, make_corpora, make_table
    n, T = 5, 12
    corpora = make_corpora(T, 61)
    table = make_table(n, T, corpora, 62)
    start = np.array([0, 500, 0, 2000, 0], np.int32)
    lowpass, band_lp = np.array([481, 100, 300, 481, 60], np.int32), np.array([32, 20, 28, 31, 18], np.int32)
    w = mo.batch(corpora, table, T, start)
    d = Device(corpora)
    dev = d.dev
    st = torch.cuda.Stream(device=dev)
    b = capi.Batch(model, n)
    if prepare:
        prepare(b, n)
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    energy, rms, vad = new(n, T), new(n, 3), new(n, T, dtype=torch.uint8)
    clean, noisy, target, nf, rec = new(T, n, 480), new(T, n, 480), new(T, n), new(n, dtype=torch.int32), new(T, n, 98)
    d_lp, d_bl = torch.from_numpy(lowpass).to(dev), torch.from_numpy(band_lp).to(dev)
    torch.cuda.synchronize()
    b.train_levels_vad_device(energy.data_ptr(), rms.data_ptr(), vad.data_ptr(), d.ptrs, d.lens, table, start, T, st.cuda_stream)
    b.train_mix_device(clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), nf.data_ptr(), d.ptrs, d.lens, table, rms.data_ptr(),
                       vad.data_ptr(), T, st.cuda_stream)
    if features:
        b.train_features_device(rec.data_ptr(), clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), d_lp.data_ptr(), d_bl.data_ptr(),
                                nf.data_ptr(), T, st.cuda_stream)
    st.synchronize()
    b.close()
    assert 0 < w["vad"].sum() < w["vad"].size
    assert (vad.cpu().numpy() == w["vad"]).all()
    for name, got in (("clean", clean), ("noisy", noisy), ("vad_target", target), ("noise_free", nf)):
        assert_bits_equal(got.cpu().numpy(), w[name], f"levels+VAD -> mix on one stream: {name}")
    if features:
        oracles = [TrainOracle() for _ in range(n)]
        ref = np.stack([np.stack([oracles[s].frame(w["clean"][f, s], w["noisy"][f, s], int(lowpass[s]), int(band_lp[s]),
                                                   float(w["vad_target"][f, s]), int(w["noise_free"][s])) for s in range(n)])
                        for f in range(T)])
        assert_bits_equal(rec.cpu().numpy(), ref, "levels+VAD -> mix -> features on one stream")


def test_chain_into_mix_and_features_on_a_callers_stream(model):
    _chain(model, True)


def test_chain_into_mix_on_a_batch_in_per_stream_phase_with_tables_set(model):
    def prepare(b, n):
        b.set_pcm_rate(48000)
        b.set_stream_rates(np.where(np.arange(n) % 2, 16000, 48000))
        b.set_stream_formats(["ulaw" if s % 3 == 0 else "s16" for s in range(n)])
        b.set_stream_controls(capi.controls_table(n, 12.0, .4, 3))
        active = np.ones((2, n), np.uint8)
        active[0, ::2] = 0
        b.process_masked(np.zeros((2, n, 480), np.float32), active)   # from here on: per-stream frame phase
    _chain(model, False, prepare)   # (the feature extraction refuses a batch in per-stream frame phase: the training-mix calls do not)


# ---- c. the restated functions on the device against this host's libm ----
def _device_sweep(mode, first, stride, n):
    bad, where = C.c_ulonglong(7), C.c_uint(0)
    with capi.instrumented() as L:
        assert L.rnnoise_amd_debug_train_vad_libm(0, mode, first, stride, n, C.byref(bad), C.byref(where)) == 0
    return bad.value, where.value


def test_device_pow_is_the_hosts_over_its_whole_domain():
    lo, hi = (int(np.float32(v).view(np.uint32)) for v in (.1, .9))
    assert _device_sweep(1, lo, 1, hi - lo + 1) == (0, 0)
    assert _device_sweep(1, 0x7fc00000, 1, 1) == (0, 0)        # NaN in, NaN out
    assert _device_sweep(1, 0x3f000000, 1, 1) == (0, 0)        # w = .5: pow(1, .5), the tiny-product path


@pytest.mark.parametrize("mode", [2, 3])
def test_device_log_is_the_hosts_on_ten_million_arguments(mode):
    stride = 0x7f800000 // 10_000_000
    last = 0x7f7fffff if mode == 2 else 0x7f800000
    assert _device_sweep(mode, 0, stride, last // stride + 1) == (0, 0)
    assert _device_sweep(mode, 0, 1, 4096) == (0, 0)            # zero (log(0) for mode 3) and the smallest subnormals
    assert _device_sweep(mode, last - 4095, 1, 4096) == (0, 0)  # up to the largest finite float, and Inf for mode 3


# ---- d. a host whose libm fails the self-check ----
def test_forced_self_check_failure_refuses_and_touches_nothing():
    from test_train_mix_gpu import Device
    n, T = 3, 7
    corpora, table, start = make_rows(n, T, 5)
    with capi.instrumented() as L:
        model = capi.Model(load_blob("default"))
        b = capi.Batch(model, n)
        d = Device(corpora)
        bufs = [guarded((n, T)), guarded((n, 3)), guarded((n, T), torch.uint8)]
        p = [v[1].data_ptr() for v in bufs]
        call = lambda vad=p[2]: L.rnnoise_batch_train_levels_vad_device(b.h, p[0], p[1], vad, *d.ptrs, *d.lens, table.ctypes.data,
                                                                        start.ctypes.data_as(C.POINTER(C.c_int)), T, None)
        L.rnnoise_amd_debug_train_vad_selfcheck(0)
        try:
            assert call() == -1
            with pytest.raises(RuntimeError):
                b.train_levels_vad_device(p[0], p[1], p[2], d.ptrs, d.lens, table, start, T)
        finally:
            L.rnnoise_amd_debug_train_vad_selfcheck(-1)
        assert call(None) == -1                                  # a NULL d_vad
        bad = table.copy()
        bad["noise_pos"][1] = d.lens[1] - 480 * T + 1
        assert L.rnnoise_batch_train_levels_vad_device(b.h, p[0], p[1], p[2], *d.ptrs, *d.lens, bad.ctypes.data, None, T, None) == -1
        torch.cuda.synchronize()
        for buf, view, fill in bufs:
            assert (buf.cpu().numpy() == buf.cpu().numpy().dtype.type(fill)).all()
        assert call() == 0                                       # and with the self-check's own answer it runs
        torch.cuda.synchronize()
        assert (bufs[2][1].cpu().numpy() == capi.train_vad(bufs[0][1].cpu().numpy(), start)).all()
        b.close()
        model.close()


# ---- e. generate and the command line ----
def test_generate_on_the_device_is_generate_on_the_host_and_the_oracles(model):
    corpora, want = _oracle_records()
    dev = torch.device("cuda", 0)
    d_corpora = [torch.from_numpy(c).to(dev) for c in corpora]
    rng = np.random.default_rng(1234)
    draws = train_data.draw(rng, 7, [len(c) for c in corpora], 9)
    assert (draws.start_pos > 0).any()
    b = capi.Batch(model, 3)
    got = {}
    for vad in ("host", "device", "auto"):
        b.reset()
        got[vad] = train_data.generate(b, *d_corpora, draws, 9, vad=vad)
    assert_bits_equal(got["host"], want, 'generate(vad="host"): the bytes of the chain with the host call')
    assert got["device"].tobytes() == got["host"].tobytes() == got["auto"].tobytes()
    # ... and with room impulse responses between mix and features
    h = [(np.random.default_rng(3).standard_normal(k) * np.exp(-np.arange(k) / 300.0)).astype(np.float32) for k in (900, 4000)]
    rec = train_data.draw_rir(rng, 7, len(h))
    rec["rir_id"][:2] = (0, -1)
    b.reset()
    spectra = train_data.rir_spectra(b, h, dev)
    for vad in ("host", "device"):
        b.reset()
        got[vad] = train_data.generate(b, *d_corpora, draws, 9, rirs=(spectra, rec), rir_work_bytes=64 << 20, vad=vad)
    b.close()
    assert got["device"].tobytes() == got["host"].tobytes() and got["host"].tobytes() != got["auto"].tobytes()


def _oracle_records():
    """the records of tests/test_train_mix_gpu.py's `generated`: 7 sequences of 9 frames on 3 streams through the two oracles"""
    from oracle.binding import TrainOracle
    from test_train_mix_gpu import make_corpora
    T, count, N = 9, 7, 3
    corpora = make_corpora(40, 71)
    draws = train_data.draw(np.random.default_rng(1234), count, [len(c) for c in corpora], T)
    w = mo.batch(corpora, draws.mix, T, draws.start_pos)
    oracles = [TrainOracle() for _ in range(N)]
    rec = np.empty((count, T, 98), np.float32)
    for i in range(count):
        for f in range(T):
            rec[i, f] = oracles[i % N].frame(w["clean"][f, i], w["noisy"][f, i], int(draws.lowpass[i]), int(draws.band_lp[i]),
                                             float(w["vad_target"][f, i]), int(w["noise_free"][i]))
    return corpora, rec


def test_cli_writes_the_same_file_with_the_vad_on_the_device_and_on_the_host(tmp_path):
    from test_train_mix_gpu import make_corpora
    names = []
    for k, c in enumerate(make_corpora(40, 71)):
        names.append(str(tmp_path / f"c{k}.pcm"))
        c.tofile(names[-1])
    blob = tmp_path / "model.blob"
    blob.write_bytes(load_blob("default"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    files = {}
    for vad in ("device", "host"):
        out = tmp_path / f"out_{vad}.f32"
        subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "dump-features", "--model", str(blob), *names, str(out), "7", "--seed", "1234",
                        "--seq-frames", "9", "--streams", "3", "--vad", vad], check=True, env=env, cwd=ROOT)
        files[vad] = out.read_bytes()
    assert len(files["host"]) == 7 * 9 * 98 * 4 and files["device"] == files["host"]
