"""The RIR calls on the GPU (include/rnnoise_amd.h: RNNoiseTrainRir; rnnoise_amd/csrc/train_rir.hip) against tests/csrc/rir_oracle.c,
bit for bit -- which tests/test_train_rir_cpu.py holds to the reference's own load_rir and rir_filter_sequence.

  a  the loader: every response length at which load_rir changes, the denormal one, rows filled with NaN behind their length
  b  the filter: 7 / 69 / 137 / 300 frames (a partial block; one block and a bit; block borders inside frames; five blocks) on 1 / 3 /
     65 sequences, rir_id mixed among -1, repeated and distinct ids, all four clip / quantise combinations on filtered and unfiltered
     sequences, samples at and beyond +-32767; a one-unit workspace and one that holds everything; guard words around every buffer
  c  an unfiltered sequence is what the mix call alone gives with the same flags; a caller's stream; the refusals
  d  mix -> rir -> train_features on one stream, two sequences per stream, against TrainOracle fed with the oracle's frames
  e  train_data.generate with and without RIRs, `cli dump-features --rir-list`
  f  one 2000-frame sequence against the reference's own output (tests/golden/train_rir_reference.npz)"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mix_oracle as mo
import rir_oracle as ro
from conftest import GOLD, ROOT, assert_bits_equal, load_blob
from rnnoise_amd import capi, train_data
from train_support import guarded, guards_intact

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
PLANTED = (32767.0, -32767.0, 32768.0, -32769.0, 6172.5, -6172.5, 32767.5, -.5)
UNIT = 2 * ro.NFFT * 8


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


@pytest.fixture(scope="module")
def rirs():
    """the responses of rir_oracle.responses() and the oracle's spectra (10, 2, 65536, 2), shared and never written"""
    h = ro.responses()
    spec = ro.spectra(h)
    spec.setflags(write=False)
    return h, spec


def upload(a):
    buf, view, fill = guarded(a.shape)
    view.copy_(torch.from_numpy(np.array(a, np.float32)))
    return buf, view, fill


# ---- a. the loader ----
def test_load_device_is_the_oracles(model, rirs):
    h, want = rirs
    rows = np.full((len(h), ro.RIR_MAX), np.nan, np.float32)     # (behind a response's length: never read as a sample that counts)
    for i, r in enumerate(h):
        rows[i, :len(r)] = r
    d_rows, d_spec = upload(rows), guarded(want.shape)
    b = capi.Batch(model, 2)
    b.train_rir_load_device(d_spec[1].data_ptr(), d_rows[1].data_ptr(), [len(r) for r in h])
    torch.cuda.synchronize()
    got = d_spec[1].cpu().numpy()
    for i in range(len(h)):
        for early in (0, 1):
            assert_bits_equal(got[i, early], want[i, early], f"response {i} ({len(h[i])} samples), early {early}")
    denormal = got[len(h) - 1, 0]
    assert ((denormal != 0) & (np.abs(denormal) < np.finfo(np.float32).tiny)).sum() > 1000   # (kept, not flushed)
    guards_intact(d_spec[0], d_spec[2], "spectra")
    guards_intact(d_rows[0], d_rows[2], "responses")
    assert_bits_equal(d_rows[1].cpu().numpy(), rows, "the responses are only read")
    # one response on a stream of the caller's, into the middle of a larger table
    st = torch.cuda.Stream()
    d_one = guarded((3, 2, ro.NFFT, 2))
    b.train_rir_load_device(d_one[1][1].data_ptr(), d_rows[1][3].data_ptr(), [len(h[3])], st.cuda_stream)
    st.synchronize()
    b.close()
    one = d_one[1].cpu().numpy()
    assert_bits_equal(one[1], want[3], "one response")
    assert (one[0] == np.float32(d_one[2])).all() and (one[2] == np.float32(d_one[2])).all()


# ---- b. the filter ----
def make_case(T, n, seed):
    """clean and noisy frames (T, n, 480) and a table: ids cycle with period 3 through none / a repeated response / one of its own,
    flags with period 4 through the four combinations; the noisy signals reach beyond +-32767, and every sequence starts with PLANTED"""
    clean = np.stack([ro.signal(T, [seed, s], 2500.0).reshape(T, 480) for s in range(n)], 1)
    noisy = clean + np.stack([ro.signal(T, [seed, s, 1], 14000.0).reshape(T, 480) for s in range(n)], 1)
    noisy[0, :, :len(PLANTED)] = PLANTED
    s = np.arange(n)
    t = np.zeros(n, capi.RIR_DTYPE)
    t["rir_id"] = np.where(s % 3 == 0, -1, np.where(s % 3 == 1, 6, s % 10)) if n > 1 else [7]
    t["clip"], t["quantize"] = s % 2, (s // 2) % 2
    return np.ascontiguousarray(clean, np.float32), np.ascontiguousarray(noisy, np.float32), t


def run_rir(b, d_spec, clean, noisy, table, units, stream=0, sync=torch.cuda.synchronize):
    """rnnoise_batch_train_rir_device on copies of the frames, in a workspace of `units` units: clean, noisy; guards checked"""
    T, n = clean.shape[:2]
    d_clean, d_noisy = upload(clean), upload(noisy)
    work = guarded((units * UNIT // 4,), fill=3.25e-33)
    sync()
    torch.cuda.synchronize()
    b.train_rir_device(d_clean[1].data_ptr(), d_noisy[1].data_ptr(), d_spec[1].data_ptr(), d_spec[1].shape[0], table, work[1].data_ptr(),
                       units * UNIT, T, stream)
    sync()
    for name, (buf, _, fill) in (("clean", d_clean), ("noisy", d_noisy), ("spectra", d_spec), ("workspace", work)):
        guards_intact(buf, fill, name)
    return d_clean[1].cpu().numpy(), d_noisy[1].cpu().numpy()


def units_of(table, T):
    return 2 * -(-T * 480 // ro.BLOCK) * int((table["rir_id"] >= 0).sum())


def test_the_cases_cover_what_they_are_there_for(rirs):
    h, spec = rirs
    clean, noisy, t = make_case(7, 65, 3)
    f = t["rir_id"] >= 0
    for filtered in (True, False):
        assert {(int(c), int(q)) for c, q in zip(t["clip"][f == filtered], t["quantize"][f == filtered])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ids = t["rir_id"][f]
    assert (ids == 6).sum() > 10 and len(set(ids)) >= 7 and len(h) - 1 in ids            # repeated, distinct, the denormal one
    wc, wn = ro.batch(clean, noisy, spec, t)
    raw = t.copy()
    raw["clip"] = raw["quantize"] = 0
    plain = ro.batch(clean, noisy, spec, raw)[1]
    clip = t["clip"] == 1
    assert (plain[:, clip & f] > 32767).any() and (plain[:, clip & f] < -32767).any() and (plain[:, clip & ~f] > 32767).any()
    assert np.abs(wn[:, clip]).max() == 32767 and np.abs(wn[:, ~clip]).max() > 32767
    q = t["quantize"] == 1
    assert (wn[:, q] == np.floor(wn[:, q])).all() and (plain[:, q & f] != np.floor(plain[:, q & f])).any()
    assert list(wn[0, 9, :8]) == [32767, -32767, 32767, -32767, 6172.5, -6172.5, 32767, -.5]          # clip only, unfiltered
    assert list(wn[0, 6, :8]) == [32767, -32767, 32768, -32769, 6173, -6172, 32768, 0]                # quantise only, unfiltered
    assert (wc[:, ~f] == clean[:, ~f]).all() and (wc[:, f] != clean[:, f]).any()
    assert 69 * 480 == ro.BLOCK + 352 and 137 * 480 == 2 * ro.BLOCK + 224 and ro.BLOCK % 480 == 128


@pytest.mark.parametrize("T,n", [(7, 1), (7, 65), (69, 3), (137, 3), (137, 65), (300, 1), (300, 3)])
def test_filter_is_the_oracles(model, rirs, T, n):
    h, spec = rirs
    clean, noisy, t = make_case(T, n, 100 * T + n)
    wc, wn = ro.batch(clean, noisy, spec, t)
    d_spec = upload(spec)
    b = capi.Batch(model, n)
    gc, gn = run_rir(b, d_spec, clean, noisy, t, max(1, units_of(t, T)))           # everything in one slab
    assert_bits_equal(gc, wc, f"{T} frames, {n} sequences: clean")
    assert_bits_equal(gn, wn, f"{T} frames, {n} sequences: noisy")
    if n <= 3:                                                                     # one unit per slab; and a slab that ends inside a block
        for units in (1, 3):
            sc, sn = run_rir(b, d_spec, clean, noisy, t, units)
            assert_bits_equal(sc, wc, f"{T} frames, {n} sequences, {units}-unit workspace: clean")
            assert_bits_equal(sn, wn, f"{T} frames, {n} sequences, {units}-unit workspace: noisy")
    b.close()
    assert_bits_equal(d_spec[1].cpu().numpy(), spec, "the spectra are only read")


def test_small_workspace_on_many_sequences(model, rirs):
    """65 sequences of 69 frames in slabs of 7 units: slabs that start and end anywhere inside a block's list of sequences"""
    h, spec = rirs
    clean, noisy, t = make_case(69, 65, 5)
    wc, wn = ro.batch(clean, noisy, spec, t)
    b = capi.Batch(model, 65)
    gc, gn = run_rir(b, upload(spec), clean, noisy, t, 7)
    b.close()
    assert_bits_equal(gc, wc, "clean")
    assert_bits_equal(gn, wn, "noisy")


# ---- c. beside the mix call; streams; refusals ----
def test_an_unfiltered_sequence_is_what_the_mix_call_alone_gives(model, rirs):
    from test_train_mix_gpu import Device, make_corpora, make_table, run_gpu
    T, n = 7, 6
    corpora = make_corpora(T, 31)
    table = make_table(n, T, corpora, 32)
    table["noise_gain"] *= 40                                                      # (loud: the clip has work to do)
    assert {(int(c), int(q)) for c, q in zip(table["clip"], table["quantize"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    d = Device(corpora)
    b = capi.Batch(model, n)
    want = run_gpu(b, d, table, T)
    raw = table.copy()
    raw["clip"] = raw["quantize"] = 0
    plain = run_gpu(b, d, raw, T)
    assert (np.abs(plain["noisy"]) > 32767).any() and (plain["noisy"] != want["noisy"]).any()
    rec = np.zeros(n, capi.RIR_DTYPE)
    rec["rir_id"], rec["clip"], rec["quantize"] = -1, table["clip"], table["quantize"]
    gc, gn = run_rir(b, upload(rirs[1][:1]), plain["clean"], plain["noisy"], rec, 1)
    b.close()
    assert_bits_equal(gn, want["noisy"], "noisy")
    assert_bits_equal(gc, want["clean"], "clean")


def test_on_a_stream_of_the_callers(model, rirs):
    h, spec = rirs
    clean, noisy, t = make_case(69, 3, 8)
    wc, wn = ro.batch(clean, noisy, spec, t)
    st = torch.cuda.Stream()
    b = capi.Batch(model, 3)
    gc, gn = run_rir(b, upload(spec), clean, noisy, t, 2, stream=st.cuda_stream, sync=st.synchronize)
    b.close()
    assert_bits_equal(gc, wc, "clean")
    assert_bits_equal(gn, wn, "noisy")


def test_refusals_touch_nothing(model, rirs):
    import ctypes as C
    h, spec = rirs
    T, n, R = 7, 3, 2
    clean, noisy, t = make_case(T, n, 9)
    t["rir_id"] = [1, -1, 0]
    d_clean, d_noisy, d_spec, work = upload(clean), upload(noisy), upload(spec[:R]), guarded((UNIT // 4,))
    d_rows = upload(np.ones((R, ro.RIR_MAX), np.float32))
    pc, pn, ps, pw, pr = (v[1].data_ptr() for v in (d_clean, d_noisy, d_spec, work, d_rows))
    assert all(q % 16 == 0 for q in (pc, pn, ps, pw, pr))
    b = capi.Batch(model, n)
    L = capi.lib()

    def bad(**kw):
        u = t.copy()
        for k, (row, v) in kw.items():
            u[k][row] = v
        return u
    lens = lambda *v: np.array(v, np.int32).ctypes.data_as(C.POINTER(C.c_int))
    f = lambda clean=pc, noisy=pn, spec=ps, n_rirs=R, table=t, wk=pw, wb=UNIT, frames=T: \
        L.rnnoise_batch_train_rir_device(b.h, clean, noisy, spec, n_rirs, table.ctypes.data if table is not None else None, wk, wb, frames, None)
    calls = [lambda: f(clean=None), lambda: f(noisy=None), lambda: f(spec=None), lambda: f(table=None), lambda: f(wk=None),
             lambda: f(frames=0), lambda: f(frames=-1),
             lambda: f(table=bad(rir_id=(0, R))), lambda: f(table=bad(rir_id=(1, -2))), lambda: f(n_rirs=1),
             lambda: f(table=bad(clip=(1, 2))), lambda: f(table=bad(quantize=(2, -1))),
             lambda: f(wb=UNIT - 1), lambda: f(wb=0),
             lambda: f(clean=pc + 4), lambda: f(noisy=pn + 8), lambda: f(spec=ps + 8), lambda: f(wk=pw + 4),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, None, pr, lens(5, 5), R, None),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, ps, None, lens(5, 5), R, None),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, ps, pr, None, R, None),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, ps, pr, lens(5, 5), 0, None),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, ps, pr, lens(5, 0), R, None),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, ps, pr, lens(32769, 5), R, None),
             lambda: L.rnnoise_batch_train_rir_load_device(b.h, ps + 8, pr, lens(5, 5), R, None)]
    for i, c in enumerate(calls):
        assert c() == -1, i
    torch.cuda.synchronize()
    assert f() == 0                                                                 # (the arguments the refusals vary are good ones)
    torch.cuda.synchronize()
    b.close()


def test_refused_calls_leave_the_buffers_alone(model, rirs):
    T, n = 7, 2
    clean, noisy, t = make_case(T, n, 10)
    t["rir_id"] = [0, 5]                                                            # (there is one response only)
    d_clean, d_noisy, d_spec, work = upload(clean), upload(noisy), upload(rirs[1][:1]), guarded((UNIT // 4,))
    b = capi.Batch(model, n)
    with pytest.raises(RuntimeError):
        b.train_rir_device(d_clean[1].data_ptr(), d_noisy[1].data_ptr(), d_spec[1].data_ptr(), 1, t, work[1].data_ptr(), UNIT, T)
    torch.cuda.synchronize()
    b.close()
    assert_bits_equal(d_clean[1].cpu().numpy(), clean, "clean")
    assert_bits_equal(d_noisy[1].cpu().numpy(), noisy, "noisy")
    assert (work[0].cpu().numpy() == np.float32(work[2])).all()


# ---- d. the chain ----
def test_chain_mix_rir_train_features(model, rirs):
    """two sequences per stream of 70 frames (two blocks), one stream of the caller's, no host synchronisation between the calls"""
    from oracle.binding import TrainOracle
    from test_train_mix_gpu import Device, make_corpora, make_table
    h, spec = rirs
    n, T = 3, 70
    corpora = make_corpora(T, 61)
    tables = [make_table(n, T, corpora, 62), make_table(n, T, corpora, 63)[::-1].copy()]
    recs = np.zeros((2, n), capi.RIR_DTYPE)
    recs["rir_id"] = [[4, -1, 7], [-1, 9, 9]]
    for k in range(2):
        recs[k]["clip"], recs[k]["quantize"] = tables[k]["clip"], tables[k]["quantize"]
        tables[k]["clip"] = tables[k]["quantize"] = 0
    lowpass, band_lp = np.array([481, 100, 300], np.int32), np.array([32, 20, 28], np.int32)
    want = [mo.batch(corpora, t, T) for t in tables]
    oracles = [TrainOracle() for _ in range(n)]
    ref = []
    for k, w in enumerate(want):
        wc, wn = ro.batch(w["clean"], w["noisy"], spec, recs[k])
        assert (wn != w["noisy"]).any()
        ref.append(np.stack([np.stack([oracles[s].frame(wc[f, s], wn[f, s], int(lowpass[s]), int(band_lp[s]), float(w["vad_target"][f, s]),
                                                        int(w["noise_free"][s])) for s in range(n)]) for f in range(T)]))
    d = Device(corpora)
    dev = d.dev
    st = torch.cuda.Stream(device=dev)
    b = capi.Batch(model, n)
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    energy, rms = [new(n, T), new(n, T)], [new(n, 3), new(n, 3)]
    clean, noisy, target, nf, rec = new(T, n, 480), new(T, n, 480), new(T, n), new(n, dtype=torch.int32), new(2, T, n, 98)
    d_lp, d_bl, d_spec, work = torch.from_numpy(lowpass).to(dev), torch.from_numpy(band_lp).to(dev), upload(spec), new(2 * UNIT // 4)
    vads = []
    torch.cuda.synchronize()
    for k in range(2):
        b.train_levels_device(energy[k].data_ptr(), rms[k].data_ptr(), d.ptrs, d.lens, tables[k], T, st.cuda_stream)
        st.synchronize()
        vads.append(torch.from_numpy(capi.train_vad(energy[k].cpu().numpy())).to(dev))
    torch.cuda.synchronize()
    for k in range(2):
        b.train_mix_device(clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), nf.data_ptr(), d.ptrs, d.lens, tables[k], rms[k].data_ptr(),
                           vads[k].data_ptr(), T, st.cuda_stream)
        b.train_rir_device(clean.data_ptr(), noisy.data_ptr(), d_spec[1].data_ptr(), len(spec), recs[k], work.data_ptr(), 2 * UNIT, T,
                           st.cuda_stream)
        b.train_features_device(rec[k].data_ptr(), clean.data_ptr(), noisy.data_ptr(), target.data_ptr(), d_lp.data_ptr(), d_bl.data_ptr(),
                                nf.data_ptr(), T, st.cuda_stream)
    st.synchronize()
    b.close()
    got = rec.cpu().numpy()
    for k in range(2):
        for s in range(n):
            assert_bits_equal(got[k, :, s], ref[k][:, s], f"sequence {k} of stream {s}")


# ---- e. generate and the command line ----
GEN_T, GEN_COUNT, GEN_N, GEN_SEED = 70, 5, 2, 4321


@pytest.fixture(scope="module")
def generated(rirs):
    """5 sequences of 70 frames on 2 streams through the oracles, in file order, with three responses: corpora, the responses, the
    records without RIRs and with them"""
    from oracle.binding import TrainOracle
    from test_train_mix_gpu import make_corpora
    h = [rirs[0][k] for k in (3, 7, 8)]
    spec = rirs[1][[3, 7, 8]]
    corpora = make_corpora(GEN_T + 30, 71)
    rng = np.random.default_rng(GEN_SEED)
    draws = train_data.draw(rng, GEN_COUNT, [len(c) for c in corpora], GEN_T)
    rec = train_data.draw_rir(rng, GEN_COUNT, len(h))
    assert (rec["rir_id"] >= 0).any() and (rec["rir_id"] < 0).any()
    rec["clip"], rec["quantize"] = draws.mix["clip"], draws.mix["quantize"]
    raw = draws.mix.copy()
    raw["clip"] = raw["quantize"] = 0
    out = []
    for table, apply in ((draws.mix, False), (raw, True)):
        w = mo.batch(corpora, table, GEN_T, draws.start_pos)
        clean, noisy = ro.batch(w["clean"], w["noisy"], spec, rec) if apply else (w["clean"], w["noisy"])
        oracles = [TrainOracle() for _ in range(GEN_N)]
        r = np.empty((GEN_COUNT, GEN_T, 98), np.float32)
        for i in range(GEN_COUNT):
            for f in range(GEN_T):
                r[i, f] = oracles[i % GEN_N].frame(clean[f, i], noisy[f, i], int(draws.lowpass[i]), int(draws.band_lp[i]),
                                                   float(w["vad_target"][f, i]), int(w["noise_free"][i]))
        out.append(r)
    assert (out[0] != out[1]).any()
    return corpora, h, out[0], out[1]


def test_generate_without_and_with_rirs(model, generated):
    corpora, h, plain, reverberant = generated
    dev = torch.device("cuda", 0)
    d_corpora = [torch.from_numpy(c).to(dev) for c in corpora]
    rng = np.random.default_rng(GEN_SEED)
    draws = train_data.draw(rng, GEN_COUNT, [len(c) for c in corpora], GEN_T)
    rec = train_data.draw_rir(rng, GEN_COUNT, len(h))
    b = capi.Batch(model, GEN_N)
    a = train_data.generate(b, *d_corpora, draws, GEN_T)
    b.reset()
    c = train_data.generate(b, *d_corpora, draws, GEN_T, rirs=None)
    assert a.tobytes() == c.tobytes()
    assert_bits_equal(a, plain, "generate without RIRs")
    b.reset()
    spectra = train_data.rir_spectra(b, h, dev)
    for work in (UNIT, 64 << 20):
        got = train_data.generate(b, *d_corpora, draws, GEN_T, rirs=(spectra, rec), rir_work_bytes=work)
        b.reset()
        assert_bits_equal(got, reverberant, f"generate with RIRs, workspace {work}")
    b.close()


def test_cli_dump_features_with_a_rir_list_writes_those_bytes(generated, tmp_path):
    corpora, h, plain, reverberant = generated
    names = []
    for k, c in enumerate(corpora):
        names.append(str(tmp_path / f"c{k}.pcm"))
        c.tofile(names[-1])
    listing = tmp_path / "rirs.txt"
    with open(listing, "w") as f:
        for k, r in enumerate(h):
            r.tofile(tmp_path / f"rir{k}.f32")
            f.write(str(tmp_path / f"rir{k}.f32") + "\n")
    blob = tmp_path / "model.blob"
    blob.write_bytes(load_blob("default"))
    out = tmp_path / "out.f32"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "dump-features", "--model", str(blob), *names, str(out), str(GEN_COUNT), "--seed",
                    str(GEN_SEED), "--seq-frames", str(GEN_T), "--streams", str(GEN_N), "--rir-list", str(listing), "--rir-work-mb", "3"],
                   check=True, env=env, cwd=ROOT)
    assert out.read_bytes() == reverberant.tobytes()


# ---- f. 2000 frames against the reference's own output ----
@pytest.fixture(scope="module")
def two_thousand(model):
    """the recipe of tests/golden/train_rir_reference.npz through the loader and the filter: (inputs, clean, noisy) as the GPU gives them"""
    from test_train_rir_cpu import reference_recipe
    h, clean, noisy = reference_recipe()
    b = capi.Batch(model, 1)
    spectra = train_data.rir_spectra(b, [h], torch.device("cuda", 0))
    rec = np.zeros(1, capi.RIR_DTYPE)
    gc, gn = run_rir(b, upload(spectra.cpu().numpy()), clean.reshape(2000, 1, 480), noisy.reshape(2000, 1, 480), rec, 16)
    b.close()
    return (h, clean, noisy), gc.reshape(-1), gn.reshape(-1)


def test_two_thousand_frames_are_the_oracles(two_thousand):
    (h, clean, noisy), gc, gn = two_thousand
    assert_bits_equal(gc, ro.filter(clean, ro.load(h, 1)), "clean")
    assert_bits_equal(gn, ro.filter(noisy, ro.load(h, 0)), "noisy")


def test_two_thousand_frames_are_the_references(two_thousand):
    g = np.load(os.path.join(GOLD, "train_rir_reference.npz"))
    if hashlib.sha256(ro.twiddles().tobytes()).hexdigest() != str(g["twiddles_sha256"]):
        pytest.skip("this host's libm gives other twiddles than the one the fixture was recorded on")
    _, gc, gn = two_thousand
    assert_bits_equal(gc[g["at"]], g["clean_at"], "clean")
    assert_bits_equal(gn[g["at"]], g["noisy_at"], "noisy")
    assert hashlib.sha256(gc.tobytes()).hexdigest() == str(g["clean_sha256"])
    assert hashlib.sha256(gn.tobytes()).hexdigest() == str(g["noisy_sha256"])
