"""The training-mix calls on the GPU (include/rnnoise_amd.h: RNNoiseTrainMix; rnnoise_amd/csrc/train_mix.hip) against
tests/csrc/mix_oracle.c, bit for bit -- which tests/test_train_mix_cpu.py holds to the reference's own functions.

  a  7 frames, 1 / 65 / 130 sequences: every filter branch, absent noises, clipping at and beyond +-32767, quantisation of halves,
     odd and even rows, overlapping rows, a row that ends with its corpus; guard words around every output, the corpora unchanged
  b  300 frames: the recurrences over 144,000 samples
  c  hand-made VAD tracks: every action of clear_vad on neighbouring lanes
  d  mix -> rnnoise_batch_train_features_device on one stream without a host synchronisation, two sequences per stream, against
     oracle.binding.TrainOracle; then reset and process against the Oracle
  e  a stream of the caller's; a batch in per-stream frame phase with rate, format and control tables
  f  train_data.generate and `cli dump-features` against the same draws through the two oracles, in file order"""
import os
import subprocess
import sys

import numpy as np
import pytest

import mix_oracle as mo
from conftest import ROOT, assert_bits_equal, load_blob
from rnnoise_amd import capi, train_data
from train_support import GUARD, guarded, guards_intact

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
FILTERS = [(0.0, 0.0), (-2 * .55 * np.cos(.9), .55 * .55), (-.62 + .31, -.62 * .31), (-2 * .69 * np.cos(.1), .69 * .69)]
SPECIAL = (32767, -32767, -32768, 12345, -12345, 32767, -32768, 777)   # noise samples planted for (a): see special_rows


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


def make_corpora(T, seed):
    """three int16 corpora a little longer than a sequence of T frames, of odd and even lengths: loud speech with silences, two
    noises.  The speech holds zeros and the noise the values of SPECIAL at fixed places (special_rows)."""
    rng = np.random.default_rng(seed)
    span = 480 * T
    lens = (span + 2001, span + 778, span + 1)
    env = np.repeat(rng.choice([0.0, 200.0, 6000.0, 20000.0], lens[0] // 240 + 1), 240)[:lens[0]]
    speech = np.clip(np.rint(rng.standard_normal(lens[0]) * env), -32768, 32767).astype(np.int16)
    noise = np.clip(np.rint(rng.standard_normal(lens[1]) * 3000), -32768, 32767).astype(np.int16)
    fg = np.clip(np.rint(rng.standard_normal(lens[2]) * 9000 * (rng.random(lens[2]) < .05)), -32768, 32767).astype(np.int16)
    speech[10:2000:97] = 0
    for k in range(64):
        noise[5 + 12 * k] = SPECIAL[k % len(SPECIAL)]
    return [speech, noise, fg]


def make_table(n, T, corpora, seed):
    """n sequences whose parameters cycle through the filter branches, the absent noises, the flags and odd / even positions; the
    last one ends with each corpus' last sample"""
    rng = np.random.default_rng(seed)
    lens = [len(c) for c in corpora]
    t = np.zeros(n, capi.MIX_DTYPE)
    s = np.arange(n)
    for k, name in enumerate(("speech_pos", "noise_pos", "fgnoise_pos")):
        t[name] = (s * (37 + 2 * k) + k) % (lens[k] - 480 * T + 1)
        t[name][-1] = lens[k] - 480 * T
    t["speech_gain"] = np.array([.3, 1.0, 3.1], np.float32)[s % 3]
    t["noise_gain"] = np.where(s % 5 == 1, 0, np.array([.5, 4.0], np.float32)[(s // 3) % 2])
    t["fgnoise_gain"] = np.where(s % 5 == 2, 0, .8)
    both = s % 5 == 3
    t["noise_gain"][both] = t["fgnoise_gain"][both] = 0
    for k, name in enumerate(("a_sig", "b_sig", "a_noise", "b_noise", "a_fgnoise", "b_fgnoise")):
        t[name] = np.array(FILTERS, np.float32)[(s + k + s // 4) % 4]
    t["clip"], t["quantize"] = s % 2, (s // 2) % 2
    return t


def special_rows(t, rows, corpora, T):
    """Rows of t rewritten so that the first sample of the noisy signal is exactly noise[noise_pos] * g for a chosen g: the speech row
    starts with a zero sample, the foreground gain is 0, and the first output of a biquad chain is its input.  g = 1 on 32767, -32767
    and -32768 (clip: at the bound, and beyond it), g = 1/2 on odd samples (quantize: a half, of either sign).  The noise gain that
    normalises to g exactly is searched among the floats around g / k, k = 3000.f / (1 + rms); not every row has one, so several
    planted samples are tried.  Returns {row: expected first noisy sample before clip and quantise}."""
    f32 = np.float32
    speech, noise, _ = corpora
    zeros = [z for z in range(10, 2000, 97) if z <= len(speech) - 480 * T]
    want, k0 = {}, 0
    for row, value in zip(rows, SPECIAL[:5]):
        g = f32(.5) if value in (12345, -12345) else f32(1)
        for k in range(k0, 64):
            pos = 5 + 12 * k
            if noise[pos] != value:
                continue
            r = t[row:row + 1].copy()
            r["speech_pos"], r["noise_pos"], r["fgnoise_gain"] = zeros[row % len(zeros)], pos, 0
            r["clip"], r["quantize"] = g == 1, g != 1
            _, rms = mo.levels(corpora, r[0], T)
            kk = f32(3000) / (f32(1) + rms[1])
            cand = f32(g / kk)
            for _ in range(4):
                cand = np.nextafter(cand, f32(0))
            found = None
            for _ in range(9):
                if f32(cand * kk) == g:
                    found = cand
                    break
                cand = np.nextafter(cand, f32(np.inf))
            if found is not None:
                r["noise_gain"] = found
                t[row] = r[0]
                want[row] = float(value) * float(g)
                k0 = k + 1
                break
        assert row in want, f"no exact noise gain found for sample {value}"
    return want


class Device:
    """the corpora on the device, and output buffers with guard words on both sides (train_support.guarded)"""

    def __init__(self, corpora):
        self.dev = torch.device("cuda", 0)
        self.host = corpora
        # (each corpus between guard samples of its own, so that a row that ends with its corpus ends inside the tensor)
        self.padded = [torch.from_numpy(np.concatenate([np.full(GUARD, 0x5A5A, np.int16), c, np.full(GUARD, 0x5A5A, np.int16)])).to(self.dev)
                       for c in corpora]
        self.ptrs = [p.data_ptr() + 2 * GUARD for p in self.padded]
        self.lens = [len(c) for c in corpora]

    def out(self, shape, dtype=torch.float32):
        return guarded(shape, dtype)

    def corpora_unchanged(self):
        for p, c in zip(self.padded, self.host):
            h = p.cpu().numpy()
            assert (h[GUARD:-GUARD] == c).all() and (h[:GUARD] == 0x5A5A).all() and (h[-GUARD:] == 0x5A5A).all()


def run_gpu(b, d, table, T, start_pos=None, vad_tracks=None, stream=0, sync=torch.cuda.synchronize):
    """levels -> train_vad on the host (or the given tracks) -> mix on batch b: the dict of mix_oracle.batch, guards checked"""
    n = len(table)
    bufs = {k: d.out(shape, dt) for k, shape, dt in (("energy", (n, T), torch.float32), ("rms", (n, 3), torch.float32),
                                                     ("clean", (T, n, 480), torch.float32), ("noisy", (T, n, 480), torch.float32),
                                                     ("vad_target", (T, n), torch.float32), ("noise_free", (n,), torch.int32))}
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    sync()
    b.train_levels_device(p["energy"], p["rms"], d.ptrs, d.lens, table, T, stream)
    sync()
    energy = bufs["energy"][1].cpu().numpy()
    vad = capi.train_vad(energy, start_pos) if vad_tracks is None else np.ascontiguousarray(vad_tracks, np.uint8)
    vbuf, vview, vfill = d.out((n, T), torch.uint8)
    vview.copy_(torch.from_numpy(vad))
    sync()
    b.train_mix_device(p["clean"], p["noisy"], p["vad_target"], p["noise_free"], d.ptrs, d.lens, table, p["rms"], vview.data_ptr(), T,
                       stream)
    sync()
    for k, (buf, _, fill) in bufs.items():
        guards_intact(buf, fill, k)
    guards_intact(vbuf, vfill, "vad")
    assert (vview.cpu().numpy() == vad).all()
    r = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    r["vad"] = vad
    return r


def compare(got, want, what):
    for k in ("energy", "rms", "vad", "clean", "noisy", "vad_target", "noise_free"):
        assert_bits_equal(got[k], want[k], f"{what}: {k}")


# ---- a. sizes around the wave, every parameter branch ----
@pytest.fixture(scope="module")
def seven():
    """corpora, the 130-sequence table, its special rows and the oracle's results, shared and never written"""
    T = 7
    corpora = make_corpora(T, 31)
    table = make_table(130, T, corpora, 32)
    special = special_rows(table, (60, 61, 62, 63, 64), corpora, T)
    assert capi.train_mix_check(table, [len(c) for c in corpora], T)
    start = (np.arange(130) % 4 == 2) * (np.arange(130) * 53 % (480 * T + 900))
    want = mo.batch(corpora, table, T, start.astype(np.int32))
    for a in want.values():
        a.setflags(write=False)
    return corpora, table, special, start.astype(np.int32), want


def test_the_table_of_the_seven_frame_cases_covers_what_it_is_there_for(seven):
    corpora, table, special, start, want = seven
    T = 7
    raw = table.copy()
    raw["clip"] = raw["quantize"] = 0
    plain = mo.batch(corpora, raw, T, start)["noisy"]            # the noisy signal before clip and quantise
    assert [plain[0, r, 0] for r in sorted(special)] == [32767.0, -32767.0, -32768.0, 6172.5, -6172.5]
    clip = table["clip"] == 1
    assert (np.abs(plain[:, clip]) > 32767).sum() > 100 and (plain[:, clip] > 32767).any() and (plain[:, clip] < -32767).any()
    assert np.abs(want["noisy"][:, clip]).max() == 32767 and np.abs(want["noisy"][:, ~clip]).max() > 32767
    q = table["quantize"] == 1
    assert (want["noisy"][:, q] == np.floor(want["noisy"][:, q])).all() and (plain[:, q] != np.floor(plain[:, q])).any()
    assert want["noisy"][0, 63, 0] == 6173.0 and want["noisy"][0, 64, 0] == -6172.0
    for name, n_len in (("speech_pos", 0), ("noise_pos", 1), ("fgnoise_pos", 2)):
        assert (table[name] % 2 == 0).any() and (table[name] % 2 == 1).any()
        assert table[name][-1] + 480 * T == len(corpora[n_len])
    assert len(corpora[0]) < 2 * 480 * T                                   # every two rows overlap
    nf = (table["noise_gain"] == 0) & (table["fgnoise_gain"] == 0)
    assert (want["noise_free"] == nf).all() and 0 < nf.sum() < 130
    assert ((table["noise_gain"] == 0) & ~nf).any() and ((table["fgnoise_gain"] == 0) & ~nf).any()
    for name in ("a_sig", "b_sig", "a_noise", "b_noise", "a_fgnoise", "b_fgnoise"):
        assert len({tuple(v) for v in table[name][:65]}) == 4
    assert 0 < want["vad"].sum() < want["vad"].size and (want["vad"][start >= 480, 0] == 0).all()


@pytest.mark.parametrize("n", [1, 65, 130])
def test_seven_frames(model, seven, n):
    corpora, table, special, start, want = seven
    d = Device(corpora)
    b = capi.Batch(model, n)
    got = run_gpu(b, d, table[:n], 7, start[:n])
    b.close()
    d.corpora_unchanged()
    sub = {k: (v[:n] if k in ("energy", "rms", "vad", "noise_free") else v[:, :n]) for k, v in want.items()}
    compare(got, sub, f"{n} sequences")


# ---- b. long recurrences ----
def test_three_hundred_frames(model):
    T = 300
    corpora = make_corpora(T, 41)
    table = make_table(4, T, corpora, 42)
    table["noise_gain"], table["fgnoise_gain"] = [.5, 4.0, .5, .02], [.8, 0, .8, .8]
    start = np.array([0, 7000, 0, 480 * 40 + 3], np.int32)
    want = mo.batch(corpora, table, T, start)
    assert 0 < want["vad"].sum() < want["vad"].size
    d = Device(corpora)
    b = capi.Batch(model, 4)
    got = run_gpu(b, d, table, T, start)
    b.close()
    d.corpora_unchanged()
    compare(got, want, "300 frames")


# ---- c. the actions of clear_vad ----
def test_vad_actions_on_neighbouring_lanes(model):
    from test_train_mix_cpu import clear_vad_actions
    T, n = 12, 6
    tracks = np.array([[0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1],     # zero, fade in, keep (a one-frame gap), fade out, zero, fade in at the end
                       [1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1],     # starts active: keep, fade out, zero, fade in, keep
                       [0] * 12,                                 # all zero
                       [1] * 12,                                 # all kept
                       [0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0],     # fades back to back
                       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]], np.uint8)  # a fade in on the last frame's predecessor only
    acts = [set(clear_vad_actions(t)) for t in tracks]
    assert acts[0] == {0, 1, 2, 3} and acts[2] == {1} and acts[3] == {0} and clear_vad_actions(tracks[1])[0] == 0
    corpora = make_corpora(T, 51)
    table = make_table(n, T, corpora, 52)
    want = mo.batch(corpora, table, T, vad_tracks=tracks)
    assert (want["clean"][2:4, 2] == 0).all() and (want["clean"][:, 3] != 0).any()
    assert_bits_equal(want["vad_target"], tracks.T.astype(np.float32), "the VAD target is the track")
    d = Device(corpora)
    b = capi.Batch(model, n)
    got = run_gpu(b, d, table, T, vad_tracks=tracks)
    b.close()
    compare(got, want, "hand-made VAD tracks")


# ---- d. the chain into the feature extraction ----
def test_chain_into_train_features_and_no_state_left_behind(model):
    from oracle.binding import Oracle, TrainOracle
    n, T = 5, 12
    corpora = make_corpora(T, 61)
    lens = [len(c) for c in corpora]
    tables = [make_table(n, T, corpora, 62), make_table(n, T, corpora, 63)[::-1].copy()]
    tables[1]["speech_pos"] += 1
    tables[1]["speech_pos"][0] = 5
    starts = [np.array([0, 500, 0, 2000, 0], np.int32), np.zeros(n, np.int32)]
    lowpass, band_lp = np.array([481, 100, 300, 481, 60], np.int32), np.array([32, 20, 28, 31, 18], np.int32)
    want = [mo.batch(corpora, t, T, s) for t, s in zip(tables, starts)]
    oracles = [TrainOracle() for _ in range(n)]
    ref = np.stack([np.stack([np.stack([oracles[s].frame(w["clean"][f, s], w["noisy"][f, s], int(lowpass[s]), int(band_lp[s]),
                                                         float(w["vad_target"][f, s]), int(w["noise_free"][s])) for s in range(n)])
                              for f in range(T)]) for w in want])                                  # (2, T, n, 98)
    d = Device(corpora)
    dev = d.dev
    st = torch.cuda.Stream(device=dev)
    b = capi.Batch(model, n)
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    energy, rms = [new(n, T), new(n, T)], [new(n, 3), new(n, 3)]
    clean, noisy, target, nf, rec = new(T, n, 480), new(T, n, 480), new(T, n), new(n, dtype=torch.int32), new(2, T, n, 98)
    d_lp, d_bl = torch.from_numpy(lowpass).to(dev), torch.from_numpy(band_lp).to(dev)
    torch.cuda.synchronize()
    vads = []
    for k in range(2):  # the levels and the Viterbi VAD of both sequences first: they carry no state
        b.train_levels_device(energy[k].data_ptr(), rms[k].data_ptr(), d.ptrs, d.lens, tables[k], T, st.cuda_stream)
        st.synchronize()
        v = capi.train_vad(energy[k].cpu().numpy(), starts[k])
        assert (v == want[k]["vad"]).all()
        vads.append(torch.from_numpy(v).to(dev))
    torch.cuda.synchronize()
    for k in range(2):  # mix, features, mix, features: one stream, no host synchronisation in between
        b.train_mix_device(clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), nf.data_ptr(), d.ptrs, lens, tables[k], rms[k].data_ptr(),
                           vads[k].data_ptr(), T, st.cuda_stream)
        b.train_features_device(rec[k].data_ptr(), clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), d_lp.data_ptr(), d_bl.data_ptr(),
                                nf.data_ptr(), T, st.cuda_stream)
    st.synchronize()
    got = rec.cpu().numpy()
    for k in range(2):
        for s in range(n):
            assert_bits_equal(got[k, :, s], ref[k, :, s], f"sequence {k} of stream {s}")
    # the analysis state carried from the first sequence into the second: fresh oracles give other records
    fresh = TrainOracle().frame(want[1]["clean"][0, 0], want[1]["noisy"][0, 0], 481, 32, float(want[1]["vad_target"][0, 0]), 0)
    assert (fresh.view(np.uint32) != ref[1, 0, 0].view(np.uint32)).any()
    # reset, process: the mix calls left nothing behind
    from rnnoise_amd import synth
    pcm = synth.batch_pcm([3, 77, 130, 8, 9], 6, lead_silence=1)
    b.reset()
    out, vad, gains = b.process(pcm)
    b.close()
    blob = load_blob("default")
    for i in range(n):
        w = Oracle(blob).run(pcm[:, i])
        for name, g, r in (("pcm", out[:, i], w["out"]), ("vad", vad[:, i], w["vad"]), ("gains", gains[:, i], w["gains"])):
            assert_bits_equal(g, r, f"process after the chain and a reset: {name} of stream {i}")


# ---- e. streams and batch modes ----
def test_on_a_stream_of_the_callers(model, seven):
    corpora, table, special, start, want = seven
    n = 65
    d = Device(corpora)
    st = torch.cuda.Stream(device=d.dev)
    b = capi.Batch(model, n)
    got = run_gpu(b, d, table[:n], 7, start[:n], stream=st.cuda_stream, sync=st.synchronize)
    b.close()
    compare(got, {k: (v[:n] if k in ("energy", "rms", "vad", "noise_free") else v[:, :n]) for k, v in want.items()}, "caller's stream")


def test_per_stream_phase_batch_with_tables_gives_the_same_bits(model, seven):
    corpora, table, special, start, want = seven
    n = 65
    b = capi.Batch(model, n)
    b.set_pcm_rate(48000)
    b.set_stream_rates(np.where(np.arange(n) % 2, 16000, 48000))
    b.set_stream_formats(["ulaw" if s % 3 == 0 else "s16" for s in range(n)])
    b.set_stream_controls(capi.controls_table(n, 12.0, .4, 3))
    active = np.ones((2, n), np.uint8)
    active[0, ::2] = 0
    b.process_masked(np.zeros((2, n, 480), np.float32), active)              # from here on: per-stream frame phase
    with pytest.raises(RuntimeError):
        z = np.zeros((1, n, 480), np.float32)
        b.train_features(z, z, np.zeros((1, n), np.float32), np.full(n, 481), np.full(n, 32), np.zeros(n))
    d = Device(corpora)
    got = run_gpu(b, d, table[:n], 7, start[:n])
    b.close()
    compare(got, {k: (v[:n] if k in ("energy", "rms", "vad", "noise_free") else v[:, :n]) for k, v in want.items()},
            "per-stream frame phase, tables set")


def test_refusals_touch_nothing(model, seven):
    corpora, table, special, start, want = seven
    n, T = 3, 7
    d = Device(corpora)
    b = capi.Batch(model, n)
    bufs = [d.out((T * n * 480,)) for _ in range(4)]
    p = [v[1].data_ptr() for v in bufs]
    assert all(q % 16 == 0 for q in p)
    L = capi.lib()
    bad = table[:n].copy()
    bad["noise_pos"][1] = d.lens[1] - 480 * T + 1
    t = table[:n].copy()
    calls = [
        lambda: L.rnnoise_batch_train_levels_device(b.h, p[0], p[1], *d.ptrs, *d.lens, bad.ctypes.data, T, None),
        lambda: L.rnnoise_batch_train_levels_device(b.h, p[0], p[1], *d.ptrs, *d.lens, t.ctypes.data, 0, None),
        lambda: L.rnnoise_batch_train_levels_device(b.h, p[0], None, *d.ptrs, *d.lens, t.ctypes.data, T, None),
        lambda: L.rnnoise_batch_train_mix_device(b.h, p[0], p[1], p[2], p[3], *d.ptrs, *d.lens, bad.ctypes.data, p[2], p[3], T, None),
        lambda: L.rnnoise_batch_train_mix_device(b.h, p[0], p[1], p[2], p[3], *d.ptrs, *d.lens, t.ctypes.data, p[2], None, T, None),
        lambda: L.rnnoise_batch_train_mix_device(b.h, p[0], p[1], p[2], p[3], *d.ptrs, *d.lens, t.ctypes.data, p[2], p[3], -1, None),
        # d_clean / d_noisy are stored 16 bytes at a time: a pointer that is not 16-byte aligned is refused
        lambda: L.rnnoise_batch_train_mix_device(b.h, p[0] + 4, p[1], p[2], p[3], *d.ptrs, *d.lens, t.ctypes.data, p[2], p[3], T, None),
        lambda: L.rnnoise_batch_train_mix_device(b.h, p[0], p[1] + 8, p[2], p[3], *d.ptrs, *d.lens, t.ctypes.data, p[2], p[3], T, None),
    ]
    for i, c in enumerate(calls):
        assert c() == -1, i
    torch.cuda.synchronize()
    b.close()
    for buf, view, fill in bufs:
        assert (buf.cpu().numpy() == np.float32(fill)).all()


# ---- f. generate and the command line ----
@pytest.fixture(scope="module")
def generated():
    """7 sequences of 9 frames on 3 streams through the two oracles, in file order: (corpora, draws, records (7, 9, 98))"""
    from oracle.binding import TrainOracle
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


def test_generate_is_the_oracles_in_file_order(model, generated):
    corpora, want = generated
    dev = torch.device("cuda", 0)
    draws = train_data.draw(np.random.default_rng(1234), 7, [len(c) for c in corpora], 9)
    b = capi.Batch(model, 3)
    got = train_data.generate(b, *[torch.from_numpy(c).to(dev) for c in corpora], draws, 9)
    b.close()
    assert got.shape == (7, 9, 98)
    assert_bits_equal(got, want, "generate")


def test_cli_dump_features_writes_those_bytes(generated, tmp_path):
    corpora, want = generated
    names = []
    for k, c in enumerate(corpora):
        names.append(str(tmp_path / f"c{k}.pcm"))
        c.tofile(names[-1])
    blob = tmp_path / "model.blob"
    blob.write_bytes(load_blob("default"))
    out = tmp_path / "out.f32"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "dump-features", "--model", str(blob), *names, str(out), "7", "--seed", "1234",
                    "--seq-frames", "9", "--streams", "3"], check=True, env=env, cwd=ROOT)
    assert out.read_bytes() == want.tobytes()
