"""The score calls on the GPU (include/rnnoise_amd.h: rnnoise_batch_score_records[_device]): the scoring of the record
step with the network taken out, one launch per call, on the records of tests/eval_cases.py (T = 12).

  a  identity: eval_records returns gains / vad; score_records of those outputs on zeroed sums gives THE SAME DOUBLES -- at 1, 17, 65
     and 513 rows (ragged against a wave, a workgroup round and a launch), on the three record layouts, in the cuts (12,), 12 x (1,)
     and (5, 1, 6), with prediction rows packed and strided
  b  arbitrary predictions -- 0, 1, above 1, negative, NaN, q = 0 and 1 -- and targets -1 and above 1 against the float64 restatement
     of eval_cases.loss_terms, relative difference at most 1e-10 (the bound eval_records is held to: double arithmetic differs in the
     16th digit, any float32 step shows at 1e-8); band_sums per band against the same restatement, and bitwise whatever the cut
  c  sums prefilled (the call adds), band_sums NULL, first / gamma / t0 > 0 reading record t0 - 1, sentinels behind every output, NaN
     behind every input row, more rows than the batch has streams, the device form on a stream of the caller's
  d  no state: pending split frames and a later synthesize as on a twin batch; save_streams bits before and after
  e  argument errors return -1 and launch nothing

Row i takes distinct stream i mod D.  The batch of every score call has 3 streams: it names the device and nothing else."""
import ctypes as C

import numpy as np
import pytest

import eval_cases as ec
from conftest import assert_bits_equal, load_blob, use_rcp_profile
from rnnoise_amd import capi, synth

pytestmark = pytest.mark.gpu
T = ec.T
NB = ec.NB_BANDS


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


@pytest.fixture(scope="module")
def rec():
    return ec.records()


@pytest.fixture(scope="module")
def ran(model, rec):
    """(sums (D, 4), vad (T, D), gains (T, D, 32)) of one eval_records call over every distinct stream: the doubles every score call
    on these predictions must give, and the predictions themselves"""
    use_rcp_profile("intel")
    b = capi.Batch(model, rec.shape[1])
    sums, vad, gains = b.eval_records(rec)
    b.close()
    for a in (sums, vad, gains):
        a.setflags(write=False)
    assert np.isfinite(sums).all() and (sums[:, 2] == ec.frames_scored(0, T)).all()
    return sums, vad, gains


@pytest.fixture(scope="module")
def scorer(model):
    b = capi.Batch(model, 3)
    yield b
    b.close()


def src(n, D):
    return np.arange(n) % D


def same_doubles(a, b, what):
    assert_bits_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64), what)


def band_restatement(rec, gains, vad, t0=0, n_frames=None, first=4, gamma=0.25):
    """(N, 32) float64: band b's gain terms of eval_cases.loss_terms added in frame order"""
    n_frames = rec.shape[0] - t0 if n_frames is None else n_frames
    out = np.zeros((rec.shape[1], NB), np.float64)
    with np.errstate(invalid="ignore"):
        for t in range(max(t0, first, 1), t0 + n_frames):
            r = rec[t - 1]
            gt, _ = ec.loss_terms(r[:, ec.TARGETS], r[:, ec.VAD], gains[t], vad[t], gamma)
            out += gt
    return out


# ---- a. identity ----
@pytest.mark.parametrize("n", [1, 17, 65, 513])
def test_scoring_the_outputs_of_eval_records_gives_its_doubles(scorer, rec, ran, n):
    """also: n_rows is not tied to the batch (3 streams), and the band sums of a row add up to its gain sum within rounding"""
    canon, vad, gains = ran
    idx = src(n, rec.shape[1])
    sums, bands = scorer.score_records(np.ascontiguousarray(rec[:, idx]), gains[:, idx], vad[:, idx])
    same_doubles(sums, canon[idx], f"sums of {n} rows")
    assert ec.rel_diff(bands.sum(1), canon[idx, 0]) <= 1e-12
    same_doubles(bands, bands[:len(set(idx))][idx % len(set(idx))], "rows of one stream: one set of band sums")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("layout", ["frame", "stream", "pitch100"])
def test_identity_on_every_layout(scorer, rec, ran, layout, strided):
    """records [T][N][98], [N][T][98] and rows 100 floats apart; prediction rows packed (32 and 1 floats) or strided (40 and 3 floats,
    stream-contiguous beside stream-contiguous records); every pad is NaN, so a read beside a row poisons a sum"""
    canon, vad, gains = ran
    n = 70
    idx = src(n, rec.shape[1])
    r, g, v = np.ascontiguousarray(rec[:, idx]), np.ascontiguousarray(gains[:, idx]), np.ascontiguousarray(vad[:, idx])[..., None]
    if strided:
        g = np.concatenate([g, np.full((T, n, 8), np.nan, np.float32)], axis=2)
        v = np.concatenate([v, np.full((T, n, 2), np.nan, np.float32)], axis=2)
    if layout == "pitch100":
        r = np.concatenate([r, np.full((T, n, 2), np.nan, np.float32)], axis=2)
    r = r.copy()
    r[:, :, :65] = np.nan  # the features of a record are not read
    lay = "stream" if layout == "stream" else "frame"
    if lay == "stream":
        r, g, v = (np.ascontiguousarray(a.transpose(1, 0, 2)) for a in (r, g, v))
    sums, bands = scorer.score_records(r, g, v, layout=lay)
    same_doubles(sums, canon[idx], f"sums, layout {layout}, strided {strided}")
    assert np.isfinite(bands).all()


@pytest.mark.parametrize("cuts", [(12,), (1,) * 12, (5, 1, 6)])
def test_identity_in_every_cut(scorer, rec, ran, cuts):
    canon, vad, gains = ran
    n = 65
    idx = src(n, rec.shape[1])
    r = np.ascontiguousarray(rec[:, idx])
    whole_s, whole_b = scorer.score_records(r, gains[:, idx], vad[:, idx])
    sums, bands = np.zeros((n, capi.EVAL_SUMS)), np.zeros((n, NB))
    t = 0
    for k in cuts:
        scorer.score_records(r, gains[t:t + k, idx], vad[t:t + k, idx], t0=t, sums=sums, band_sums=bands)
        t += k
    assert t == T
    same_doubles(sums, canon[idx], f"sums over the cuts {cuts}")
    same_doubles(bands, whole_b, f"band sums over the cuts {cuts}")
    same_doubles(whole_s, canon[idx], "one call")


# ---- b. arbitrary predictions against the float64 restatement ----
@pytest.fixture(scope="module")
def arbitrary(rec):
    """records with targets above 1 and -1 beside the real ones, predictions with every special value; row s, band b, frame t"""
    rng = np.random.Generator(np.random.PCG64(20))
    n = rec.shape[1]
    r = rec.copy()
    r[:, 1::7, 65 + 3] = 1.5
    r[:, 2::7, 65 + 9] = -1.0
    r[:, 3::11, 65:97] = 2.0
    p = rng.uniform(0, 1, (T, n, NB)).astype(np.float32)
    q = rng.uniform(0, 1, (T, n)).astype(np.float32)
    p[:, 0::5, 0], p[:, 1::5, 1], p[:, 2::5, 2] = 0.0, 1.0, 1.75
    q[:, 0::4], q[:, 1::4] = 0.0, 1.0
    bad = np.zeros(n, bool)
    bad[[5, 40]] = True           # NaN and a negative prediction: the row's gain sum is NaN, as in numpy; no other row's is
    p[6, 5, 7], p[8, 40, 30] = np.nan, -0.5
    return r, p, q, bad


def test_arbitrary_predictions_against_the_float64_restatement(scorer, arbitrary, capsys):
    """Bound 1e-10, as for eval_records (tests/test_eval_records_gpu.py).  Measured on MI355X, largest relative difference over the
    103 rows: 4.8e-16 (gain sums), 0 (VAD sums), 1.2e-14 (band sums: a band's eight terms, some of them cancelling powers near 1)."""
    r, p, q, bad = arbitrary
    with np.errstate(invalid="ignore"):
        exp = ec.expected_sums(r, p, q)
    expb = band_restatement(r, p, q)
    sums, bands = scorer.score_records(r, p, q)
    assert np.isnan(exp[bad, 0]).all() and np.isfinite(exp[~bad]).all()
    assert np.isnan(sums[bad, 0]).all() and np.isfinite(sums[~bad]).all() and np.isfinite(sums[:, 1:]).all()
    assert (np.isnan(bands) == np.isnan(expb)).all() and np.isnan(bands).sum() == 2
    ok = ~np.isnan(expb)
    worst = (ec.rel_diff(sums[~bad, 0], exp[~bad, 0]), ec.rel_diff(sums[:, 1], exp[:, 1]), ec.rel_diff(bands[ok], expb[ok]))
    with capsys.disabled():
        print(f"\n[score-records] largest relative difference against the float64 restatement: gain sums {worst[0]:.3e}, vad sums "
              f"{worst[1]:.3e}, band sums {worst[2]:.3e} ({r.shape[1]} rows, {ec.frames_scored(0, T)} scored frames)")
    assert (sums[:, 2] == ec.frames_scored(0, T)).all() and (sums[:, 3] == 0).all()
    assert (exp[~bad, 0] > 0).sum() > 60 and (exp[:, 1] > 0).sum() > 40
    for s in range(r.shape[1]):
        if not bad[s]:
            assert ec.rel_diff(sums[s, 0], exp[s, 0]) <= 1e-10, (s, sums[s, 0], exp[s, 0])
        assert ec.rel_diff(sums[s, 1], exp[s, 1]) <= 1e-10, (s, sums[s, 1], exp[s, 1])
        for b in range(NB):
            if ok[s, b]:
                assert ec.rel_diff(bands[s, b], expb[s, b]) <= 1e-10, (s, b, bands[s, b], expb[s, b])


@pytest.mark.parametrize("cuts", [(1,) * 12, (5, 1, 6)])
def test_band_sums_of_arbitrary_predictions_do_not_depend_on_the_cut(scorer, arbitrary, cuts):
    r, p, q, _ = arbitrary
    n = r.shape[1]
    whole_s, whole_b = scorer.score_records(r, p, q)
    sums, bands = np.zeros((n, capi.EVAL_SUMS)), np.zeros((n, NB))
    t = 0
    for k in cuts:
        scorer.score_records(r, p[t:t + k], q[t:t + k], t0=t, sums=sums, band_sums=bands)
        t += k
    same_doubles(sums, whole_s, f"sums over the cuts {cuts}")
    same_doubles(bands, whole_b, f"band sums over the cuts {cuts}")


# ---- c. further properties ----
def test_sums_are_added_to_and_band_sums_may_be_null(scorer, arbitrary):
    r, p, q, bad = arbitrary
    zero_s, zero_b = scorer.score_records(r, p, q)
    pre_s = np.tile(np.array([3.0, -2.0, 5.0, 7.0]), (r.shape[1], 1))
    pre_b = np.full((r.shape[1], NB), 0.5)
    s2, b2 = scorer.score_records(r, p, q, sums=pre_s.copy(), band_sums=pre_b.copy())
    s3, b3 = scorer.score_records(r, p, q, sums=pre_s.copy(), want_bands=False)
    assert b3 is None
    same_doubles(s3, s2, "band_sums NULL: the same sums")
    # (the additions start from the prefilled double, so the totals differ from prefill + sums-from-zero by roundings of the total)
    close = lambda got, pre, add: (np.abs(got - (pre + add)) <= 1e-13 * (np.abs(pre) + np.abs(add))).all()
    ok = ~bad
    assert (s2[:, 2] == 5.0 + zero_s[:, 2]).all() and (s2[:, 3] == 7.0).all()
    assert close(s2[ok, 0], 3.0, zero_s[ok, 0]) and close(s2[:, 1], -2.0, zero_s[:, 1])
    fin = np.isfinite(zero_b)
    assert close(b2[fin], 0.5, zero_b[fin]) and (np.isfinite(b2) == fin).all()
    assert (zero_s[ok, 0] > 1e-3).sum() > 60 and (s2[ok, 0] != 3.0).sum() > 60


@pytest.mark.parametrize("t0,n_frames,first,gamma", [(0, 12, 6, None), (0, 12, None, 0.5), (0, 12, 1, 1.0), (0, 12, 0, 0.25), (3, 4, 4, None),
                                                     (5, 7, 4, None), (7, 5, 2, 0.5), (0, 3, 4, None), (0, 4, 4, None), (2, 0, 4, None),
                                                     (0, 12, 12, 0.25), (0, 12, 20, 0.25)])
def test_first_gamma_and_t0(scorer, arbitrary, t0, n_frames, first, gamma):
    """a call with t0 > 0 reads record t0 - 1 and the predictions from its own base on"""
    r, p, q, bad = arbitrary
    kw = dict(first=4 if first is None else first, gamma=0.25 if gamma is None else gamma)
    with np.errstate(invalid="ignore"):
        exp = ec.expected_sums(r, p, q, t0=t0, n_frames=n_frames, **kw)
    expb = band_restatement(r, p, q, t0=t0, n_frames=n_frames, **kw)
    sums, bands = scorer.score_records(r, p[t0:t0 + n_frames], q[t0:t0 + n_frames], t0=t0, first=first, gamma=gamma)
    assert (sums[:, 2] == exp[:, 2]).all() and (sums[:, 2] == ec.frames_scored(t0, n_frames, kw["first"])).all()
    ok = np.isfinite(exp[:, 0])
    assert (np.isfinite(sums[:, 0]) == ok).all()
    assert ec.rel_diff(sums[ok, 0], exp[ok, 0]) <= 1e-10 and ec.rel_diff(sums[:, 1], exp[:, 1]) <= 1e-10
    okb = np.isfinite(expb)
    assert (np.isfinite(bands) == okb).all() and ec.rel_diff(bands[okb], expb[okb]) <= 1e-10


def test_sentinels_behind_every_output_and_the_device_form(model, scorer, rec, ran):
    """the raw calls on buffers one row longer than the call's: the extra rows keep their words; the device form on a stream of the
    caller's, rows beyond the batch's 3 streams, gives the doubles of the host form"""
    import torch
    canon, vad, gains = ran
    n = 70
    idx = src(n, rec.shape[1])
    r, g, v = np.ascontiguousarray(rec[:, idx]), np.ascontiguousarray(gains[:, idx]), np.ascontiguousarray(vad[:, idx])
    sums, bands = np.zeros((n + 1, capi.EVAL_SUMS)), np.zeros((n + 1, NB))
    sums[n], bands[n] = -77.0, -78.0
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    assert scorer._L.rnnoise_batch_score_records(scorer.h, sums.ctypes.data_as(dp), bands.ctypes.data_as(dp), g.ctypes.data_as(fp), 0, 0,
                                                 v.ctypes.data_as(fp), 0, 0, r.ctypes.data_as(fp), 0, 0, n, 0, T, None) == 0
    same_doubles(sums[:n], canon[idx], "raw host call")
    assert (sums[n] == -77.0).all() and (bands[n] == -78.0).all()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_r, d_g, d_v = (torch.from_numpy(a).to(dev) for a in (r, g, v))
        d_s = torch.zeros((n + 1, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
        d_b = torch.zeros((n + 1, NB), dtype=torch.float64, device=dev)
        d_s[n], d_b[n] = -77.0, -78.0
        scorer.score_records_device(d_s.data_ptr(), d_b.data_ptr(), d_g.data_ptr(), d_v.data_ptr(), d_r.data_ptr(), n, 0, T,
                                    stream=st.cuda_stream)
        # a second call on the same stream in two segments, stream-contiguous predictions of its own
        d_s2 = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
        d_gs, d_vs = d_g.transpose(0, 1).contiguous(), d_v.transpose(0, 1).contiguous()
        for t0, k in ((0, 7), (7, 5)):
            scorer.score_records_device(d_s2.data_ptr(), 0, d_gs.data_ptr() + t0 * NB * 4, d_vs.data_ptr() + t0 * 4, d_r.data_ptr(), n,
                                        t0, k, gain_strides=(NB, T * NB), vad_strides=(1, T), stream=st.cuda_stream)
    st.synchronize()
    hs, hb = d_s.cpu().numpy(), d_b.cpu().numpy()
    same_doubles(hs[:n], canon[idx], "device form")
    same_doubles(hb[:n], bands[:n], "device form: band sums")
    assert (hs[n] == -77.0).all() and (hb[n] == -78.0).all()
    same_doubles(d_s2.cpu().numpy(), canon[idx], "device form in two segments, stream-contiguous predictions")


# ---- d. no state ----
def test_a_score_call_reads_and_writes_no_state(model, rec, ran):
    """on a batch with pending split frames: split_pending and a later synthesize as on a twin that scored nothing; on a batch that
    has run frames: the bits of save_streams before and after"""
    canon, vad, gains = ran
    streams, F = [3, 77, 130], 4
    pcm = synth.batch_pcm(streams, F, lead_silence=1)
    a, twin = capi.Batch(model, 3), capi.Batch(model, 3)
    fa, sa = a.analyze(pcm)
    ft, stw = twin.analyze(pcm)
    assert_bits_equal(fa, ft, "features of the twins")
    sums, _ = a.score_records(rec, gains, vad)
    same_doubles(sums, canon, "scored while split frames are pending")
    assert a.split_pending == F and twin.split_pending == F
    g = np.ascontiguousarray(gains[:F, :3])
    v = np.ascontiguousarray(vad[:F, :3])
    assert_bits_equal(a.synthesize(g, v), twin.synthesize(g, v), "synthesize after a score call")
    assert a.split_pending == 0
    twin.close()
    a.reset()
    a.process(pcm)
    before = a.save_streams()
    a.score_records(rec, gains, vad)
    assert_bits_equal(a.save_streams().view(np.uint32), before.view(np.uint32), "save_streams around a score call")
    a.close()


# ---- e. argument errors ----
def test_argument_errors_return_minus_one(scorer, rec, ran):
    canon, vad, gains = ran
    n = 5
    r, g, v = np.ascontiguousarray(rec[:, :n]), np.ascontiguousarray(gains[:, :n]), np.ascontiguousarray(vad[:, :n])
    sums = np.full((n, capi.EVAL_SUMS), 9.0)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    S, G, V, R = sums.ctypes.data_as(dp), g.ctypes.data_as(fp), v.ctypes.data_as(fp), r.ctypes.data_as(fp)
    L = scorer._L
    call = lambda b=scorer.h, s=S, gg=G, vv=V, rr=R, gs=(0, 0), vs=(0, 0), rs=(0, 0), rows=n, t0=0, k=T, cfg=None: \
        L.rnnoise_batch_score_records(b, s, None, gg, gs[0], gs[1], vv, vs[0], vs[1], rr, rs[0], rs[1], rows, t0, k, cfg)
    assert call(b=None) == -1 and call(s=None) == -1 and call(gg=None) == -1 and call(vv=None) == -1 and call(rr=None) == -1
    assert call(rows=0) == -1 and call(t0=-1) == -1 and call(k=-1) == -1
    assert call(gs=(NB, 0)) == -1 and call(gs=(n * NB - 1, NB)) == -1 and call(vs=(n - 1, 1)) == -1 and call(rs=(97, n * 98)) == -1
    bad = capi.EvalConfig(0.0, 3)
    assert call(cfg=C.byref(bad)) == -1
    assert (sums == 9.0).all()
    assert call() == 0 and (sums[:, 2] == 9.0 + ec.frames_scored(0, T)).all()
    null = C.c_void_p(256)
    assert L.rnnoise_batch_score_records_device(scorer.h, None, None, null, 0, 0, null, 0, 0, null, 0, 0, n, 0, T, None, None) == -1
    assert L.rnnoise_batch_score_records_device(scorer.h, null, None, null, 0, 0, null, 0, 0, None, 0, 0, n, 0, T, None, None) == -1
    assert L.rnnoise_batch_score_records_device(scorer.h, null, None, null, 1, 1, null, 0, 0, null, 0, 0, n, 0, T, None, None) == -1
