"""The feature calls on the GPU (include/rnnoise_amd.h: rnnoise_batch_process_features[_device], rnnoise_batch_eval_records[_device];
DESIGN 4.28): the network alone on the records of tests/eval_cases.py -- the 97 real streams of tests/train_cases.py cut to 12 frames
and six synthetic edge streams -- against oracle.binding's compute_rnn, one oracle per distinct stream, and the sums against the
float64 restatement of the trainer's loss over those outputs.

  a  predictions bit for bit at 1, 17, 65 streams on every network path and at 513 on path 0; the sums the same doubles in all of them
  b  the sums the same doubles across cuts of the frames into calls and across the three layouts
  c  the sums against the restatement, relative difference at most 1e-10 (any float32 step would show at 1e-8); frames scored exact
  d  `first`, gamma and the one-frame lag between a step and its record
  e  sums are added to; NULL outputs change nothing else
  f  two blobs in one batch through the model map
  g  NaN / Inf features in some streams reach no other stream
  h  reset, and what an eval call leaves behind for rnnoise_batch_process
  i  the device form on a stream of the caller's, on records extracted in place by rnnoise_batch_train_features_device
  j  argument errors return -1 and launch nothing

Batch stream i takes distinct stream i mod D.  The oracle runs once per distinct stream and blob (eval_cases.oracle_outputs).

The forms of a holds stop at 513 streams.  The at-size forms -- the eight-wave tile kernel, the layer-wise network chosen by size, the
four-wave rn_nn_gru_kernel, the vector kernel at size, ragged last tiles and groups of grids with more units than CUs -- run in
tests/test_gpu_at_size.py (test_stream_mix_feature_calls_at_every_form and the three tests behind it) on the mixed block of
tests/stream_mix.py, whose silent frames are rows of 65 exact zeros that a feature call must run the network on all the same."""
import ctypes as C

import numpy as np
import pytest

import eval_cases as ec
from conftest import assert_bits_equal, load_blob, use_rcp_profile
from rnnoise_amd import capi

pytestmark = pytest.mark.gpu
T = ec.T
FORMS = [(1, 0), (17, 0), (65, 0), (1, 1), (17, 1), (65, 1), (1, 2), (17, 2), (65, 2), (513, 0)]


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


@pytest.fixture(scope="module")
def rec():
    return ec.records()


@pytest.fixture(scope="module")
def want():
    use_rcp_profile("intel")
    return ec.oracle_outputs("default")


@pytest.fixture(scope="module")
def canon(model, rec):
    """(D, 4) the sums of every distinct stream from one call of one batch on the default path: what every other run must give, bit
    for bit.  (A module fixture is set up ahead of the per-test profile fixture of conftest.py: it names the suite's profile itself)"""
    use_rcp_profile("intel")
    b = capi.Batch(model, rec.shape[1])
    sums, _, _ = b.eval_records(rec)
    b.close()
    sums.setflags(write=False)
    return sums


def src(n, D):
    return np.arange(n) % D


def same_doubles(a, b, what):
    assert_bits_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64), what)


def check_outputs(vad, gains, want, idx, what, skip=()):
    wg, wv = want
    for s in range(len(idx)):
        if s not in skip:
            assert_bits_equal(gains[:, s], wg[:gains.shape[0], idx[s]], f"{what}: gains of stream {s}")
            assert_bits_equal(vad[:, s], wv[:vad.shape[0], idx[s]], f"{what}: vad of stream {s}")


def batch(model, n, path=None):
    b = capi.Batch(model, n)
    if path is not None:
        assert b.set_nn_path(path) >= 0
    return b


# ---- a. every network form ----
@pytest.mark.parametrize("n,path", FORMS)
def test_predictions_and_sums_at_every_network_form(model, rec, want, canon, n, path):
    """1: the one-stream kernel / one ragged tile; 17: a ragged second tile; 65: a ragged 64-stream group of the layer-wise network;
    513: the vector kernel.  process_features reads the features out of the records where they lie (98 floats apart); after a reset
    eval_records gives the same predictions again (path 2: the layer images are rebuilt) and the sums of every other form"""
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    b = batch(model, n, path)
    vad, gains = b.process_features(r)
    check_outputs(vad, gains, want, idx, f"process_features, {n} streams, path {path}")
    tight = np.ascontiguousarray(r[:, :, :65])
    b.reset()
    vad2, gains2 = b.process_features(tight)
    assert_bits_equal(vad2, vad, "features 65 apart against features 98 apart: vad")
    assert_bits_equal(gains2, gains, "features 65 apart against features 98 apart: gains")
    b.reset()
    sums, vad3, gains3 = b.eval_records(r)
    b.close()
    check_outputs(vad3, gains3, want, idx, f"eval_records, {n} streams, path {path}")
    same_doubles(sums, canon[idx], f"sums, {n} streams, path {path}")


# ---- b. cuts and layouts ----
@pytest.mark.parametrize("cuts", [(12,), (1,) * 12, (5, 1, 6)])
@pytest.mark.parametrize("n,path", [(17, 1), (65, 2)])
def test_sums_do_not_depend_on_the_cut(model, rec, want, canon, n, path, cuts):
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    b = batch(model, n, path)
    sums = np.zeros((n, capi.EVAL_SUMS))
    t, vads, gs = 0, [], []
    for k in cuts:
        _, v, g = b.eval_records(r, t0=t, n_frames=k, sums=sums)
        vads.append(v), gs.append(g)
        t += k
    b.close()
    assert t == T
    check_outputs(np.concatenate(vads), np.concatenate(gs), want, idx, f"cuts {cuts}")
    same_doubles(sums, canon[idx], f"sums over the cuts {cuts}, {n} streams, path {path}")


@pytest.mark.parametrize("layout", ["frame", "stream", "pitch100"])
def test_sums_do_not_depend_on_the_layout(model, rec, want, canon, layout):
    """[T][N][98], [N][T][98] (the file's order: one sequence after the other) and rows 100 floats apart, the pad full of NaN; the
    stream-contiguous layout also in two calls, the second of which starts behind record 0"""
    n = 70
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    if layout == "stream":
        r = np.ascontiguousarray(r.transpose(1, 0, 2))
    elif layout == "pitch100":
        r = np.concatenate([r, np.full((T, n, 2), np.nan, np.float32)], axis=2)
    lay = "stream" if layout == "stream" else "frame"
    b = batch(model, n, 1)
    sums, vad, gains = b.eval_records(r, layout=lay)
    check_outputs(vad, gains, want, idx, layout)
    same_doubles(sums, canon[idx], f"sums, layout {layout}")
    b.reset()
    sums2 = np.zeros_like(sums)
    b.eval_records(r, 0, 7, sums2, layout=lay)
    b.eval_records(r, 7, 5, sums2, layout=lay)
    b.close()
    same_doubles(sums2, canon[idx], f"sums in two calls, layout {layout}")


# ---- c. against the float64 restatement ----
def test_sums_against_the_float64_restatement(rec, want, canon, capsys):
    """Double arithmetic on the device differs from numpy's by a few units in the 16th digit per term; a float32 step anywhere (a
    float pow, a float accumulator) would show at 1e-8 or worse.  1e-10 separates the two by orders of magnitude.
    Measured on MI355X: largest relative difference over the 103 streams 4.0e-16 (gain sums) and 1.8e-16 (VAD sums)."""
    exp = ec.expected_sums(rec, *want)
    worst = [max(ec.rel_diff(canon[s, k], exp[s, k]) for s in range(rec.shape[1])) for k in (0, 1)]
    with capsys.disabled():
        print(f"\n[eval-records] largest relative difference of a stream's sums against the float64 restatement: "
              f"gain {worst[0]:.3e}, vad {worst[1]:.3e} ({rec.shape[1]} streams, {ec.frames_scored(0, T)} scored frames)")
    assert (canon[:, 2] == ec.frames_scored(0, T)).all() and (canon[:, 3] == 0).all()
    assert np.isfinite(canon).all() and (exp[:97, 0] > 0).sum() > 60 and (exp[:, 1] > 0).sum() > 40   # (the sums are about something)
    for s in range(rec.shape[1]):
        for k, name in ((0, "gain"), (1, "vad")):
            assert ec.rel_diff(canon[s, k], exp[s, k]) <= 1e-10, (s, name, canon[s, k], exp[s, k])
    # the edge streams: every target -1 masks every band; VAD target 0.5 has no say
    D = rec.shape[1] - ec.EDGE
    assert canon[D + 0, 0] == 0 and canon[D + 1, 1] == 0 and canon[D + 3, 1] == 0 and canon[D + 4, 0] > 0


@pytest.mark.parametrize("t0,n_frames,first", [(0, 12, 4), (0, 3, 4), (0, 4, 4), (0, 5, 4), (3, 4, 4), (5, 7, 4), (0, 12, 1), (0, 12, 0),
                                               (2, 0, 4), (0, 12, 11), (0, 12, 12), (0, 12, 20)])
def test_frames_scored(model, rec, t0, n_frames, first):
    n = 17
    r = np.ascontiguousarray(rec[:, src(n, rec.shape[1])])
    b = batch(model, n)
    sums, _, _ = b.eval_records(r, t0, n_frames, first=first, gamma=0.25)
    b.close()
    assert (sums[:, 2] == max(0, t0 + n_frames - max(t0, first, 1))).all(), sums[:, 2]
    if first >= 1:
        assert (sums[:, 2] == max(0, t0 + n_frames - max(t0, first))).all()


# ---- d. first, gamma, and the lag ----
def test_first_gamma_and_the_one_frame_lag(model, rec, want, canon):
    n = 103
    assert n == rec.shape[1]
    exp = ec.expected_sums(rec, *want)
    # the records shifted by one against the steps: other sums.  Without this a wrong lag would pass everything above
    for lag in (0, 2):
        off = ec.expected_sums(rec, *want, lag=lag)
        moved = [s for s in range(97) if exp[s, 0] > 0 and ec.rel_diff(off[s, 0], exp[s, 0]) > 1e-6]
        assert len(moved) > 50, (lag, len(moved))
        assert sum(ec.rel_diff(canon[s, 0], off[s, 0]) > 1e-6 for s in moved) == len(moved)
    b = batch(model, n)
    for first, gamma in ((6, None), (None, 0.5), (1, 1.0)):
        b.reset()
        sums, _, _ = b.eval_records(rec, first=first, gamma=gamma)
        e = ec.expected_sums(rec, *want, first=4 if first is None else first, gamma=0.25 if gamma is None else gamma)
        assert (sums[:, 2] == e[:, 2]).all()
        for s in range(n):
            assert ec.rel_diff(sums[s, :2], e[s, :2]) <= 1e-10, (first, gamma, s, sums[s], e[s])
        assert (sums[:, 0] != canon[:, 0]).sum() > 60
    b.close()


# ---- e. accumulation, NULL outputs ----
def test_sums_are_added_to_and_null_outputs_change_nothing(model, rec, want, canon):
    n = 65
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    rng = np.random.default_rng(3)
    pre = rng.standard_normal((n, capi.EVAL_SUMS)) * 100
    b = batch(model, n, 2)
    sums, vad, gains = b.eval_records(r, sums=pre.copy())
    # one addition per scored frame onto the prefill is another rounding than prefill + total: what comes back is the chain
    chain = pre.copy()
    per_frame = np.zeros((T + 1, n, capi.EVAL_SUMS))
    b2 = batch(model, n, 2)
    for t in range(T):
        b2.eval_records(r, t, 1, per_frame[t + 1])
    b2.close()
    for t in range(T):
        chain += per_frame[t + 1]
    same_doubles(sums, chain, "a pre-filled sums array")
    assert np.allclose(sums, pre + canon[idx], rtol=1e-12, atol=1e-9)
    assert (sums[:, 3] == pre[:, 3]).all()
    for wg, wv in ((False, True), (True, False), (False, False)):
        b.reset()
        s2, v2, g2 = b.eval_records(r, want_gains=wg, want_vad=wv)
        same_doubles(s2, canon[idx], f"sums with gains {wg}, vad {wv}")
        assert (g2 is None) == (not wg) and (v2 is None) == (not wv)
        if wg:
            assert_bits_equal(g2, gains, "gains without vad")
        if wv:
            assert_bits_equal(v2, vad, "vad without gains")
    b.reset()
    v3, g3 = b.process_features(r, want_gains=False)
    assert g3 is None
    assert_bits_equal(v3, vad, "process_features without gains")
    b.close()


# ---- f. two blobs in one batch ----
def test_two_blobs_through_the_model_map(model, rec, want, canon):
    """streams 0 .. 34 and 35 .. 69 carry the same 35 records; the map puts the halves on the default and the little blob, interleaved
    across the tiles.  Each half equals a one-model batch, and the little blob its own oracle"""
    h, D = 35, rec.shape[1]
    idx = (np.arange(h) * 3) % D
    r = np.ascontiguousarray(rec[:, np.concatenate([idx, idx])])
    little = capi.Model(load_blob("little"))
    lw = ec.oracle_outputs("little")
    for path in (0, 1, 2):
        b = batch(model, 2 * h, path)
        assert b.add_model(little) == 1
        slot = np.zeros(2 * h, np.uint8)
        slot[h:] = 1
        j = np.arange(2 * h)
        perm = (j % 2) * h + j // 2                                   # position j holds row perm[j]: the slots alternate
        b.set_stream_models(slot[perm])
        sums, vad, gains = b.eval_records(np.ascontiguousarray(r[:, perm]))
        b.close()
        inv = np.argsort(perm)
        sums, vad, gains = sums[inv], vad[:, inv], gains[:, inv]
        check_outputs(vad[:, :h], gains[:, :h], want, idx, f"default half, path {path}")
        check_outputs(vad[:, h:], gains[:, h:], lw, idx, f"little half, path {path}")
        same_doubles(sums[:h], canon[idx], f"default half, path {path}")
        one = batch(little, h, path)
        s1, v1, g1 = one.eval_records(np.ascontiguousarray(rec[:, idx]))
        one.close()
        same_doubles(sums[h:], s1, f"little half against a one-model batch, path {path}")
        assert_bits_equal(gains[:, h:], g1, "little half: gains")
        assert_bits_equal(vad[:, h:], v1, "little half: vad")
        exp = ec.expected_sums(rec[:, idx], lw[0][:, idx], lw[1][:, idx])
        assert max(ec.rel_diff(s1[s, :2], exp[s, :2]) for s in range(h)) <= 1e-10
        assert (s1[:, 0] != canon[idx, 0]).sum() > 20


# ---- g. isolation ----
@pytest.mark.parametrize("n,path", [(70, 0), (70, 1), (70, 2), (513, 0)])
def test_poisoned_streams_stay_alone(model, rec, want, canon, n, path):
    bad = (3, 16, 64, n - 1)
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx]).copy()
    for s in bad:
        r[2, s, 5] = np.nan
        r[3, s, 40] = np.inf
        r[4:, s, 0:65:7] = -np.inf
        r[6, s, 70] = np.nan                                  # a target, too
    b = batch(model, n, path)
    sums, vad, gains = b.eval_records(r)
    b.close()
    check_outputs(vad, gains, want, idx, "beside poisoned streams", skip=bad)
    keep = np.array([s for s in range(n) if s not in bad])
    same_doubles(sums[keep], canon[idx[keep]], "sums beside poisoned streams")


# ---- h. reset ----
def test_reset_and_what_an_eval_call_leaves_behind(model, rec, canon):
    from rnnoise_amd import synth
    n = 70
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    pcm = synth.batch_pcm(list(range(n)), 6, lead_silence=1)
    for path in (0, 2):
        fresh = batch(model, n, path)
        out0, vad0, gains0 = fresh.process(pcm)
        fresh.close()
        b = batch(model, n, path)
        s1, v1, g1 = b.eval_records(r)
        b.reset()
        s2, v2, g2 = b.eval_records(r)
        same_doubles(s2, s1, "the same call after a reset")
        same_doubles(s1, canon[idx], "sums")
        assert_bits_equal(g2, g1, "gains after a reset")
        assert_bits_equal(v2, v1, "vad after a reset")
        # without a reset the sequence goes on: other predictions
        _, v3, _ = b.eval_records(r)
        assert (v3 != v1).any()
        b.reset()
        out, vad, gains = b.process(pcm)
        b.close()
        for name, got, ref in (("pcm", out, out0), ("vad", vad, vad0), ("gains", gains, gains0)):
            assert_bits_equal(got, ref, f"process after an eval call and a reset, path {path}: {name}")


def test_reset_streams_restarts_single_sequences(model, rec, canon):
    n = 70
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    b = batch(model, n, 2)
    b.eval_records(r, 0, 5)
    some = [0, 15, 16, 64, 69]
    b.reset_streams(some)
    sums, _, _ = b.eval_records(r)
    b.close()
    same_doubles(sums[some], canon[idx[some]], "restarted streams")
    rest = [s for s in range(n) if s not in some]
    assert (sums[rest, 0] != canon[idx[rest], 0]).sum() > 40


# ---- i. the device form ----
def test_device_form_on_records_extracted_in_place(model, rec, want, canon):
    """rnnoise_batch_train_features_device writes the records, rnnoise_batch_eval_records_device scores them where they lie, both on one
    non-default stream of the caller's with no host step between; then process_features_device on the same records"""
    torch = pytest.importorskip("torch")
    import train_cases as tc
    n = 130
    c = tc.cycled(n, slice(0, T))
    dev = torch.device("cuda", 0)
    ins = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c.args()]
    d_rec = torch.full((T + 1, n, 98), float("nan"), dtype=torch.float32, device=dev)
    d_sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
    d_gains = torch.full((T + 1, n, 32), -7.0, dtype=torch.float32, device=dev)
    d_vad = torch.full((T + 1, n), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    b = batch(model, n, 1)
    b.train_features_device(d_rec.data_ptr(), *[t.data_ptr() for t in ins], T, stream=st.cuda_stream)
    b.eval_records_device(d_sums.data_ptr(), d_gains.data_ptr(), d_vad.data_ptr(), d_rec.data_ptr(), 0, 5, stream=st.cuda_stream)
    b.eval_records_device(d_sums.data_ptr(), d_gains.data_ptr() + 5 * n * 32 * 4, d_vad.data_ptr() + 5 * n * 4, d_rec.data_ptr(), 5, T - 5,
                          frame_stride=n * 98, row_stride=98, stream=st.cuda_stream)
    st.synchronize()
    idx = src(n, tc.D)
    got = d_rec.cpu().numpy()
    assert_bits_equal(got[:T], rec[:, idx], "the records extracted on the device")
    assert np.isnan(got[T]).all()
    gains, vad = d_gains.cpu().numpy(), d_vad.cpu().numpy()
    assert (gains[T] == -7).all() and (vad[T] == -7).all(), "the call wrote behind its last frame"
    check_outputs(vad[:T], gains[:T], want, idx, "device form")
    same_doubles(d_sums.cpu().numpy(), canon[idx], "device form: sums")
    # the network alone, stream-contiguous: the transposed records, one sequence after the other
    d_seq = d_rec[:T].transpose(0, 1).contiguous()
    torch.cuda.synchronize()
    b.reset()
    d_gains.fill_(-7.0)
    torch.cuda.synchronize()
    b.process_features_device(d_gains.data_ptr(), 0, d_seq.data_ptr(), T, frame_stride=98, row_stride=T * 98, stream=st.cuda_stream)
    st.synchronize()
    b.close()
    g2 = d_gains.cpu().numpy()
    assert_bits_equal(g2[:T], gains[:T], "process_features_device on [N][T][98]")
    assert (g2[T] == -7).all()


# ---- j. argument errors ----
def test_argument_errors_return_minus_one_and_launch_nothing(model, rec, canon):
    n = 17
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    L = capi.lib()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    b = batch(model, n)
    sums = np.full((n, capi.EVAL_SUMS), 5.0)
    gains = np.full((T, n, 32), -7.0, np.float32)
    call = lambda fs, rs, t0, k, cfg, recs=r, s=sums: L.rnnoise_batch_eval_records(
        b.h, s.ctypes.data_as(dp) if s is not None else None, gains.ctypes.data_as(fp), None,
        recs.ctypes.data_as(fp) if recs is not None else None, fs, rs, t0, k, C.byref(cfg) if cfg is not None else None)
    bad = [(0, 0, 0, T, capi.EvalConfig(0.0, 4)), (0, 0, 0, T, capi.EvalConfig(-1.0, 4)), (0, 0, 0, T, capi.EvalConfig(float("nan"), 4)),
           (0, 0, 0, T, capi.EvalConfig(float("inf"), 4)), (0, 0, 0, T, capi.EvalConfig(0.25, -1)), (0, 0, -1, T, None), (0, 0, 0, -1, None),
           (n * 98, 97, 0, T, None), (n * 98 - 1, 98, 0, T, None), (98, T * 98 - 1, 0, T, None), (0, 98, 0, T, None), (-98, 98, 0, T, None)]
    for args in bad:
        assert call(*args) == -1, args[:4]
    assert call(0, 0, 0, T, None, recs=None) == -1 and call(0, 0, 0, T, None, s=None) == -1
    assert L.rnnoise_batch_process_features(b.h, gains.ctypes.data_as(fp), None, r.ctypes.data_as(fp), n * 98, 64, T) == -1
    assert L.rnnoise_batch_process_features(b.h, gains.ctypes.data_as(fp), None, None, 0, 0, T) == -1
    assert L.rnnoise_batch_eval_records_device(b.h, None, None, None, C.c_void_p(256), 0, 0, 0, T, None, None) == -1
    assert (sums == 5.0).all() and (gains == -7.0).all()
    # nothing ran: the batch is still at the start of its sequences
    assert call(0, 0, 0, 0, None) == 0 and (sums == 5.0).all()
    got, _, _ = b.eval_records(r)
    b.close()
    same_doubles(got, canon[idx], "after the refused calls")
