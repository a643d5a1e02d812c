"""The split calls on the GPU (include/rnnoise_amd.h: rnnoise_batch_analyze, rnnoise_batch_synthesize):

  1  identity: analyze -> process_features of the same batch -> synthesize gives the bits of process -- out, vad, gains, the snapshot
     of every stream and a plain 3-frame process call afterwards -- against a twin batch at size and against the oracle on the
     distinct streams, at 3, 257 and 2,563 streams (every K0 / K1 / K3 form, a ragged quad, a ragged wave), in pairs of 1, 5, 1 and 8
     frames, float and int16
  2  a foreign network: the DSP on a `default` batch, the network on a second batch holding `little`, against Oracle(little)
  3  arbitrary gains against tests/csrc/split_oracle.c: the float model's gains of tests/golden/torch_float_default.npz, seeded random
     rows, a NaN row, leading silence with garbage in the caller's rows, a controls table with thr > 0 on those frames
  4  layouts: [T][N], [N][T] and padded rows for features, gains and vad through the device forms, sentinels behind every row untouched
  5  two dressed batches against their twins
  6  the protocol: pending counts, every refusal with the state unchanged, a reset dropping pending frames, the store grown by a call,
     the per-stream-phase refusal

The identity needs streams without silent frames (the full call skips the network on a silent frame, process_features does not):
asserted where it is used."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLD, assert_bits_equal, load_blob
from oracle.binding import Oracle
from rnnoise_amd import capi, synth

pytestmark = pytest.mark.gpu
IDS = [3, 77, 130]
PAIRS = [1, 5, 1, 8]
T = sum(PAIRS)
TAIL = 3


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


@pytest.fixture(scope="module")
def pcm3():
    p = synth.batch_pcm(IDS, T + TAIL)
    p.setflags(write=False)
    return p


def oracle_runs(blob_name, pcm):
    blob = load_blob(blob_name)
    runs = []
    for i in range(pcm.shape[1]):
        o = Oracle(blob)
        r = o.run(np.ascontiguousarray(pcm[:, i], np.float32))
        r["state"] = o.get_state()
        assert not r["silence"].any(), f"stream {i} has a silent frame: the identity does not hold on it"
        runs.append(r)
    return runs


@pytest.fixture(scope="module")
def want3(pcm3):
    from conftest import use_rcp_profile
    use_rcp_profile("intel")
    return oracle_runs("default", pcm3)


def cuts(pairs):
    t0 = 0
    for p in pairs:
        yield t0, t0 + p
        t0 += p


def chain(b, pcm, pairs, net=None, s16=False):
    """analyze -> process_features (of `net`, or of b itself) -> synthesize over pcm cut into `pairs` -> out, vad, gains, features"""
    net = b if net is None else net
    outs, vads, gs, fs = [], [], [], []
    for t0, t1 in cuts(pairs):
        assert b.split_pending == 0
        feats, sil = b.analyze(pcm[t0:t1], s16=s16)
        assert b.split_pending == t1 - t0 and not sil.any()
        vad, gains = net.process_features(feats)
        outs.append(b.synthesize(gains, vad, s16=s16))
        vads.append(vad), gs.append(gains), fs.append(feats)
    assert b.split_pending == 0
    return np.concatenate(outs), np.concatenate(vads), np.concatenate(gs), np.concatenate(fs)


def canon_nan(a):
    """a float array with every NaN as one bit pattern: an invalid operation gives the default NaN of the machine that ran it -- sign
    bit set on x86 SSE, clear on the GPU --, so where NaNs are expected the comparison is: NaN at the same places, the same bits
    everywhere else"""
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a


def to_s16(x):
    """the float -> short conversion of the int16 calls for values in range: truncation"""
    assert np.abs(x).max() < 32767
    return x.astype(np.int32).astype(np.int16)


# ---- 1. identity ----
@pytest.mark.parametrize("s16", [False, True], ids=["float", "int16"])
@pytest.mark.parametrize("n", [3, 257, 2563])
def test_identity_with_the_batchs_own_network(model, pcm3, want3, n, s16):
    idx = np.arange(n) % len(IDS)
    pcm = np.ascontiguousarray(pcm3[:, idx])
    if s16:
        pcm = pcm.astype(np.int16)  # (synth's samples are whole numbers: the oracle's float input is the same signal)
        assert np.array_equal(pcm[:, :3].astype(np.float32), pcm3)
    twin, b = capi.Batch(model, n), capi.Batch(model, n)
    proc = twin.process_s16 if s16 else twin.process
    t_out, t_vad, t_gains = proc(pcm[:T])
    out, vad, gains, feats = chain(b, pcm[:T], PAIRS, s16=s16)
    assert_bits_equal(out, t_out, "out against the twin")
    assert_bits_equal(vad, t_vad, "vad against the twin")
    assert_bits_equal(gains, t_gains, "gains against the twin")
    assert_bits_equal(b.save_streams(), twin.save_streams(), "the snapshot of every stream against the twin")
    # a plain call afterwards continues bit for bit
    proc_b = b.process_s16 if s16 else b.process
    for got, ref, what in zip(proc_b(pcm[T:]), proc(pcm[T:]), ("out", "vad", "gains")):
        assert_bits_equal(got, ref, f"the 3-frame process call afterwards: {what}")
    # ... and the oracle on the distinct streams: first and last copies (the ragged quad / wave ends)
    for s in sorted({0, 1, 2, n - 3, n - 2, n - 1}):
        w = want3[idx[s]]
        assert_bits_equal(out[:, s], to_s16(w["out"][:T]) if s16 else w["out"][:T], f"stream {s}: out against the oracle")
        assert_bits_equal(vad[:, s], w["vad"][:T], f"stream {s}: vad against the oracle")
        assert_bits_equal(gains[:, s], w["gains"][:T], f"stream {s}: gains against the oracle")
        assert_bits_equal(feats[:, s], w["features"][:T], f"stream {s}: the exported features against the oracle")
    for s in (0, n - 1):
        st = b.export_state(s)
        # (analysis_mem is not stored in a batch: export rebuilds it from the pitch ring, as it does after process)
        assert_bits_equal(st, twin.export_state(s), f"stream {s}: exported state against the twin")
        assert_bits_equal(st, want3[idx[s]]["state"], f"stream {s}: exported state against the oracle after {T + TAIL} frames")
    b.close(), twin.close()


# ---- 2. a foreign network ----
def test_foreign_network_on_a_second_batch(model, pcm3):
    n = 19
    idx = np.arange(n) % len(IDS)
    pcm = np.ascontiguousarray(pcm3[:, idx])
    want = oracle_runs("little", pcm3)
    little = capi.Model(load_blob("little"))
    dsp, net = capi.Batch(model, n), capi.Batch(little, n)
    out, vad, gains, _ = chain(dsp, pcm[:T], PAIRS, net=net)
    for s in range(n):
        w = want[idx[s]]
        assert_bits_equal(out[:, s], w["out"][:T], f"stream {s}: out against Oracle(little)")
        assert_bits_equal(gains[:, s], w["gains"][:T], f"stream {s}: gains against Oracle(little)")
    # the state: the DSP half from the DSP batch, the network half from the network batch
    out2, vad2, gains2, _ = chain(dsp, pcm[T:], [TAIL], net=net)
    nn = slice(2724, 4262)  # include/rn_layout.h: RN_OFF_CONV1 .. RN_OFF_DELAYED_X
    for s in (0, 7, n - 1):
        w = want[idx[s]]
        assert_bits_equal(out2[:, s], w["out"][T:], f"stream {s}: the next pair")
        st = dsp.export_state(s)
        st[nn] = net.export_state(s)[nn]
        assert_bits_equal(st, w["state"], f"stream {s}: DSP state of one batch + network state of the other against Oracle(little)")
    dsp.close(), net.close()


# ---- 3. arbitrary gains against the split oracle ----
def test_arbitrary_gains_against_the_split_oracle(model):
    from split_oracle import SplitStream
    g = np.load(GOLD + "/torch_float_default.npz")
    sid, Tn, lead = int(g["stream"]), 24, 3
    ids = [sid, sid, 5, 9, 130]
    n = len(ids)
    pcm = synth.batch_pcm(ids, Tn)
    pcm[:, 1:] = synth.batch_pcm(ids[1:], Tn, lead_silence=lead)
    rng = np.random.default_rng(20)
    gains = rng.random((Tn, n, 32), dtype=np.float32)
    vad = rng.random((Tn, n), dtype=np.float32)
    gains[4:, 0], vad[4:, 0] = g["gains"][:Tn - 4], g["vad"][:Tn - 4]    # the float model's own, from its first valid frame on
    gains[10, 2], vad[11, 2] = np.nan, np.nan                              # a NaN row, a NaN vad
    gains[12, 3, 5] = np.nan
    gains[:lead, 1:], vad[:lead, 1:] = np.nan, 9.0                         # garbage on the silent frames: must not be read
    ctl = np.zeros((n, 3), np.float32)
    ctl[1] = (0.0, 0.5, 1)                                                 # a gate that the silent frames (vad 0) must close
    ctl[3] = (0.2, 0.4, 0)
    ctl[4] = (0.1, 0.0, 0)
    b = capi.Batch(model, n)
    b.set_stream_controls(ctl)
    outs, sils = [], []
    for t0, t1 in cuts([2, 1, 9, 12]):
        feats, sil = b.analyze(pcm[t0:t1])
        outs.append(b.synthesize(gains[t0:t1], vad[t0:t1]))
        sils.append(sil)
    out, sil = np.concatenate(outs), np.concatenate(sils)
    assert sil[:lead, 1:].all() and not sil[lead:].any() and not sil[:, 0].any()
    for s in range(n):
        o = SplitStream(ctl[s])
        _, osil = o.analyze(pcm[:, s])
        assert_bits_equal(sil[:, s], osil, f"stream {s}: silence words")
        w_out = o.synthesize(gains[:, s], vad[:, s])
        st = b.export_state(s)
        keep = np.ones(len(st), bool)
        keep[2724:4262] = False
        if s in (2, 3):  # the streams that were handed NaNs
            assert np.isnan(w_out).any() and not np.isnan(w_out[:10]).any()
            assert_bits_equal(canon_nan(out[:, s]), canon_nan(w_out), f"stream {s}: out against the split oracle, NaNs as one pattern")
            assert_bits_equal(canon_nan(st[keep]), canon_nan(o.state[keep]), f"stream {s}: DSP state, NaNs as one pattern")
            continue
        assert_bits_equal(out[:, s], w_out, f"stream {s}: out against the split oracle")
        assert_bits_equal(st[keep], o.state[keep], f"stream {s}: DSP state against the split oracle")
        assert not st[~keep].any(), f"stream {s}: the split calls touched the network state"
    b.close()


# ---- 4. layouts, through the device forms ----
SENT = 12345.0


@pytest.mark.parametrize("layout", ["frame", "stream", "padded"])
def test_layouts_and_sentinels(model, pcm3, layout):
    torch = pytest.importorskip("torch")
    n, Tn = 6, 5
    idx = np.arange(n) % len(IDS)
    pcm = np.ascontiguousarray(pcm3[:Tn, idx])
    twin = capi.Batch(model, n)
    w_out, w_vad, w_gains = twin.process(pcm)
    w_feats = np.stack([Oracle(load_blob("default")).run(pcm3[:Tn, i])["features"] for i in range(len(IDS))], 1)[:, idx]

    def rows(width):
        """a sentinel-filled flat device buffer, the strides of the layout for rows of `width` floats, and the (T, n, width) view"""
        pad = 0 if layout != "padded" else 3
        w = width + pad
        if layout == "stream":
            fs, rs, size = w, Tn * w, n * Tn * w
        else:
            fs, rs, size = n * w + pad, w, Tn * (n * w + pad)
        flat = torch.full((size + 8,), SENT, dtype=torch.float32, device="cuda")
        return flat, (fs, rs)

    def view(flat, strides, width):
        a = flat.cpu().numpy()
        fs, rs = strides
        v = np.lib.stride_tricks.as_strided(a, (Tn, n, width), (fs * 4, rs * 4, 4))
        mask = np.zeros(a.shape, bool)
        np.lib.stride_tricks.as_strided(mask, (Tn, n, width), (fs, rs, 1))[...] = True
        return v.copy(), a[~mask]

    b = capi.Batch(model, n)
    st = torch.cuda.Stream()
    d_in = torch.from_numpy(pcm).cuda()
    feat, f_rows = rows(65)
    gbuf, g_rows = rows(32)
    vbuf, v_rows = rows(1)
    d_sil = torch.full((Tn, n), 7, dtype=torch.int32, device="cuda")
    d_out = torch.empty_like(d_in)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        b.analyze_device(feat.data_ptr(), d_sil.data_ptr(), d_in.data_ptr(), Tn, feat_rows=f_rows, stream=st.cuda_stream)
    st.synchronize()
    assert b.split_pending == Tn
    got_f, rest = view(feat, f_rows, 65)
    assert_bits_equal(got_f, w_feats, f"{layout}: features")
    assert (rest == SENT).all(), f"{layout}: analyze wrote outside the feature rows"
    assert not d_sil.cpu().numpy().any()
    # the twin's gains and vad into the layout's rows, between sentinels
    fs, rs = g_rows
    ga = gbuf.cpu().numpy()
    np.lib.stride_tricks.as_strided(ga, (Tn, n, 32), (fs * 4, rs * 4, 4))[...] = w_gains
    fs, rs = v_rows
    va = vbuf.cpu().numpy()
    np.lib.stride_tricks.as_strided(va, (Tn, n, 1), (fs * 4, rs * 4, 4))[...] = w_vad[..., None]
    gbuf.copy_(torch.from_numpy(ga)), vbuf.copy_(torch.from_numpy(va))
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        b.synthesize_device(d_out.data_ptr(), gbuf.data_ptr(), vbuf.data_ptr(), Tn, gain_rows=g_rows, vad_rows=v_rows, stream=st.cuda_stream)
    st.synchronize()
    assert b.split_pending == 0
    assert_bits_equal(d_out.cpu().numpy(), w_out, f"{layout}: out")
    assert_bits_equal(gbuf.cpu().numpy(), ga, f"{layout}: synthesize wrote to the gain rows")
    assert_bits_equal(vbuf.cpu().numpy(), va, f"{layout}: synthesize wrote to the vad rows")
    # the host forms in the trainer's batch-first layout
    if layout == "stream":
        b.reset()
        feats, sil = b.analyze(pcm, layout="stream")
        assert feats.shape == (n, Tn, 65)
        assert_bits_equal(feats.transpose(1, 0, 2), w_feats, "host analyze, batch-first")
        out = b.synthesize(np.ascontiguousarray(w_gains.transpose(1, 0, 2)), np.ascontiguousarray(w_vad.T), layout="stream")
        assert_bits_equal(out, w_out, "host synthesize, batch-first")
    b.close(), twin.close()


# ---- 5. dressed batches against their twins ----
def noise_s16(shape, seed):
    return np.random.default_rng(seed).integers(-6000, 6000, shape, dtype=np.int16)


def test_dressed_int16_rate_format_out_tables_controls(model):
    n, Tn = 12, 7
    rates = np.array([48000, 16000, 8000, 24000, 32000, 48000] * 2)
    fmts = ["s16", "ulaw", "alaw", "s16", "ulaw", "s16"] * 2
    out_rates = np.array([8000, 48000, 16000, 24000, 8000, 32000] * 2)
    out_fmts = ["ulaw", "s16", "s16", "alaw", "alaw", "s16"] * 2
    ctl = capi.controls_table(n, limit_db=20, vad_threshold=0.3, hold_frames=1)

    def dressed():
        b = capi.Batch(model, n)
        b.set_stream_rates(rates), b.set_stream_formats(fmts), b.set_stream_out_rates(out_rates), b.set_stream_out_formats(out_fmts)
        b.set_stream_controls(ctl)
        return b

    pcm = noise_s16((Tn, n, 480), 5)
    twin, b = dressed(), dressed()
    fill = np.full_like(pcm, 77)
    w_out, w_vad, w_gains = twin.process_s16(pcm, out=fill.copy())
    outs = []
    for t0, t1 in cuts([1, 4, 2]):
        feats, sil = b.analyze(pcm[t0:t1], s16=True)
        assert not sil.any()
        vad, gains = b.process_features(feats)
        assert_bits_equal(vad, w_vad[t0:t1], "vad")
        outs.append(b.synthesize(gains, vad, s16=True, out=fill[t0:t1].copy()))
    assert_bits_equal(np.concatenate(outs), w_out, "out: rate, format and out tables, controls")
    assert_bits_equal(b.save_streams(), twin.save_streams(), "snapshots")
    b.close(), twin.close()


def test_dressed_channels_link_layout(model):
    n, Tn, ch = 12, 6, 2

    def dressed():
        b = capi.Batch(model, n)
        b.set_pcm_channels(ch), b.set_gain_link(2)
        b.set_pcm_layout(6 * 964 + 8, 964)
        return b

    twin, b = dressed(), dressed()
    pcm = twin.pcm_array(Tn, np.float32, fill=3.0)
    pcm[...] = np.random.default_rng(8).integers(-6000, 6000, pcm.shape).astype(np.float32)
    w_out, w_vad, w_gains = twin.process(pcm, out=twin.pcm_array(Tn))
    assert w_out.shape == pcm.shape
    feats, sil = b.analyze(pcm)
    assert not sil.any()
    vad, gains = b.process_features(feats)
    out = b.synthesize(gains, vad)
    assert_bits_equal(vad, w_vad, "vad"), assert_bits_equal(gains, w_gains, "gains")
    assert_bits_equal(out, w_out, "out: channels 2, link 2, a PCM layout")
    assert_bits_equal(out.base, w_out.base, "the whole buffers, padding included")
    assert_bits_equal(b.save_streams(), twin.save_streams(), "snapshots")
    b.close(), twin.close()


# ---- 6. the protocol ----
def test_protocol_pending_refusals_reset_growth(model, pcm3):
    n = 3
    pcm = np.ascontiguousarray(pcm3)
    L = capi.lib()
    twin, b = capi.Batch(model, n), capi.Batch(model, n)
    w_out, w_vad, w_gains = twin.process(pcm[:9])
    fp = C.POINTER(C.c_float)
    assert b.split_pending == 0
    b.split_reserve(2)
    f1, _ = b.analyze(pcm[:2])
    assert b.split_pending == 2
    # every refusal, with frames pending: nothing is launched and nothing changes (shown below: the pair still gives the twin's bits)
    buf = np.zeros((2, n, 480), np.float32)
    s16 = np.zeros((2, n, 480), np.int16)
    act = np.ones((2, n), np.uint8)
    lst = np.arange(n, dtype=np.int32)
    state = np.zeros(capi.STATE_FLOATS, np.float32)
    for call in (lambda: b.process(buf), lambda: b.process_s16(s16), lambda: b.analyze(buf), lambda: b.process_masked(buf, act),
                 lambda: b.process_list(buf, lst), lambda: b.process_chunks(np.zeros((n, 100), np.float32), np.full(n, 100)),
                 lambda: b.split_reserve(8), lambda: b.set_pcm_rate(16000), lambda: b.set_nn_path(0), lambda: b.set_schedule(9),
                 lambda: b.set_stream_controls(capi.controls_table(n, 10)), lambda: b.set_gain_link(3), lambda: b.set_pcm_channels(3),
                 lambda: b.set_pcm_layout(2000, 480), lambda: b.set_stream_rates(np.full(n, 48000)),
                 lambda: b.set_stream_formats(["s16"] * n), lambda: b.set_stream_out_rates(np.full(n, 48000)),
                 lambda: b.set_stream_out_formats(["s16"] * n), lambda: b.export_state(0), lambda: b.import_state(0, state),
                 lambda: b.save_streams(), lambda: b.reset_streams([0]),
                 lambda: b.synthesize(np.zeros((1, n, 32), np.float32), np.zeros((1, n), np.float32)),
                 lambda: b.synthesize(np.zeros((3, n, 32), np.float32), np.zeros((3, n), np.float32))):
        with pytest.raises((RuntimeError, ValueError)):
            call()
        assert b.split_pending == 2
    # overlapping rows, NULL buffers
    g2, v2 = np.zeros((2, n, 32), np.float32), np.zeros((2, n), np.float32)
    bad = capi.Rows(n * 32, 31)
    assert L.rnnoise_batch_synthesize(b.h, buf.ctypes.data_as(fp), g2.ctypes.data_as(fp), C.byref(bad), v2.ctypes.data_as(fp), None, 2) == -1
    assert L.rnnoise_batch_synthesize(b.h, None, g2.ctypes.data_as(fp), None, v2.ctypes.data_as(fp), None, 2) == -1
    assert L.rnnoise_batch_synthesize(b.h, buf.ctypes.data_as(fp), None, None, v2.ctypes.data_as(fp), None, 2) == -1
    assert L.rnnoise_batch_synthesize(b.h, buf.ctypes.data_as(fp), g2.ctypes.data_as(fp), None, None, None, 2) == -1
    assert b.split_pending == 2
    # the getters and the feature calls work
    assert b.pcm_rate == 48000 and b.gain_link == 1 and (b.stream_controls() == 0).all()
    vad, gains = b.process_features(f1)
    out = b.synthesize(gains, vad)
    assert b.split_pending == 0
    assert_bits_equal(out, w_out[:2], "the pair after the refused calls")
    # a call that needs more than the reserved store grows it (7 frames after room for 2)
    f2, _ = b.analyze(pcm[2:9])
    assert b.split_pending == 7
    vad, gains = b.process_features(f2)
    assert_bits_equal(b.synthesize(gains, vad), w_out[2:9], "a 7-frame pair after a reserve of 2")
    assert_bits_equal(b.save_streams(), twin.save_streams(), "snapshots")
    # analyze refuses bad rows and NULL, with nothing pending afterwards
    feats = np.zeros((2, n, 65), np.float32)
    bad = capi.Rows(n * 65, 64)
    assert L.rnnoise_batch_analyze(b.h, feats.ctypes.data_as(fp), C.byref(bad), None, buf.ctypes.data_as(fp), 2) == -1
    assert L.rnnoise_batch_analyze(b.h, None, None, None, buf.ctypes.data_as(fp), 2) == -1
    assert L.rnnoise_batch_analyze(b.h, feats.ctypes.data_as(fp), None, None, None, 2) == -1
    assert b.split_pending == 0
    assert_bits_equal(b.save_streams(), twin.save_streams(), "snapshots after the refused analyze calls")
    # a reset drops pending frames; the batch then starts over like a new one
    b.analyze(pcm[:3])
    assert b.split_pending == 3
    b.reset(), twin.reset()
    assert b.split_pending == 0
    for got, ref, what in zip(b.process(pcm[:4]), twin.process(pcm[:4]), ("out", "vad", "gains")):
        assert_bits_equal(got, ref, f"process after a reset with frames pending: {what}")
    # per-stream frame phase (after a masked call): both calls are refused
    b.process_masked(pcm[:1], np.ones((1, n), np.uint8))
    with pytest.raises(RuntimeError):
        b.analyze(pcm[:1])
    assert L.rnnoise_batch_synthesize(b.h, buf.ctypes.data_as(fp), g2.ctypes.data_as(fp), None, v2.ctypes.data_as(fp), None, 0) == -1
    assert b.split_pending == 0
    b.close(), twin.close()


def test_protocol_the_remaining_refusals(model, pcm3):
    """With frames pending: the training calls -- each shown first to succeed with the same arguments on a batch with nothing
    pending, so that the -1 is the refusal and not an argument --, load / save of streams and FIFO records, the model calls, the
    stream-ordered setters, and the device forms of the PCM, masked, list and chunk calls, on real device buffers.  Afterwards the pair
    still gives the twin's bits and snapshot."""
    torch = pytest.importorskip("torch")
    n, Tn = 3, 2
    pcm = np.ascontiguousarray(pcm3)
    dev = torch.device("cuda", 0)
    twin, b, free = capi.Batch(model, n), capi.Batch(model, n), capi.Batch(model, n)
    w_out, w_vad, w_gains = twin.process(pcm[:Tn])
    snap0 = b.save_streams()
    fifo0 = b.save_chunk_fifos()
    feats, _ = b.analyze(pcm[:Tn])
    assert b.split_pending == Tn

    def z(shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=dev)

    # ---- the training calls ----
    rng = np.random.default_rng(3)
    corpora = [torch.from_numpy(rng.integers(-3000, 3000, 480 * Tn + 64, dtype=np.int16)).to(dev) for _ in range(3)]
    cptr, clen = [c.data_ptr() for c in corpora], [int(c.numel()) for c in corpora]
    mix = np.zeros(n, capi.MIX_DTYPE)
    mix["speech_gain"], mix["noise_gain"] = 1.0, 0.5
    assert capi.train_mix_check(mix, clen, Tn)
    energy, rms, vad8 = z((n, Tn)), z((n, 3)), z((n, Tn), torch.uint8)
    clean, noisy, vtarget, nfree = z((Tn, n, 480)), z((Tn, n, 480)), z((Tn, n)), z((n,), torch.int32)
    rec, lp, bl = z((Tn, n, 98)), torch.full((n,), 481, dtype=torch.int32, device=dev), torch.full((n,), 32, dtype=torch.int32, device=dev)
    d_rir, spectra = z((1, capi.RIR_MAX)), z((1, 2, capi.RIR_FFT, 2))
    d_rir[0, 0] = 1.0
    rir = np.zeros(n, capi.RIR_DTYPE)
    wb = capi.train_rir_work_bytes(1)
    work = z((wb,), torch.uint8)
    host = np.zeros((Tn, n, 480), np.float32)
    train = {
        "train_features": lambda x: x.train_features(host, host, np.zeros((Tn, n), np.float32), np.full(n, 481), np.full(n, 32), np.zeros(n)),
        "train_features_device": lambda x: x.train_features_device(rec.data_ptr(), clean.data_ptr(), noisy.data_ptr(), vtarget.data_ptr(),
                                                                   lp.data_ptr(), bl.data_ptr(), nfree.data_ptr(), Tn),
        "train_levels_device": lambda x: x.train_levels_device(energy.data_ptr(), rms.data_ptr(), cptr, clen, mix, Tn),
        "train_mix_device": lambda x: x.train_mix_device(clean.data_ptr(), noisy.data_ptr(), vtarget.data_ptr(), nfree.data_ptr(), cptr, clen,
                                                         mix, rms.data_ptr(), vad8.data_ptr(), Tn),
        "train_rir_load_device": lambda x: x.train_rir_load_device(spectra.data_ptr(), d_rir.data_ptr(), [5]),
        "train_rir_device": lambda x: x.train_rir_device(clean.data_ptr(), noisy.data_ptr(), spectra.data_ptr(), 1, rir, work.data_ptr(), wb, Tn),
    }
    if capi.train_vad_device_available():
        train["train_levels_vad_device"] = lambda x: x.train_levels_vad_device(energy.data_ptr(), rms.data_ptr(), vad8.data_ptr(), cptr, clen,
                                                                               mix, None, Tn)
    for name, call in train.items():
        call(free)                      # the arguments are good: a batch with nothing pending takes them
        torch.cuda.synchronize()
        with pytest.raises((RuntimeError, ValueError)):
            call(b)
        assert b.split_pending == Tn, name
    # ---- state, models, stream-ordered setters, device forms of the PCM calls ----
    little = capi.Model(load_blob("little"))
    d_pcm, d_out, d_pcm16, d_out16 = z((Tn, n, 480)), z((Tn, n, 480)), z((Tn, n, 480), torch.int16), z((Tn, n, 480), torch.int16)
    d_vad, d_gains, d_act = z((Tn, n)), z((Tn, n, 32)), torch.ones((Tn, n), dtype=torch.uint8, device=dev)
    d_list, d_counts, d_frames = torch.arange(n, dtype=torch.int32, device=dev), torch.full((n,), 100, dtype=torch.int32, device=dev), z((n,), torch.int32)
    d_bytes, d_ctl = z((n,), torch.uint8), z((n, 3))
    d_snap, d_fifo = z((n, capi.SNAP_FLOATS)), z((n, capi.CHUNK_REC_FLOATS))
    chunk = np.zeros((n, 100), np.float32)
    P = lambda t: t.data_ptr()  # noqa: E731
    others = {
        "load_streams": lambda: b.load_streams(snap0),
        "save_chunk_fifos": lambda: b.save_chunk_fifos(),
        "load_chunk_fifos": lambda: b.load_chunk_fifos(fifo0),
        "save_streams_device": lambda: b.save_streams_device(P(d_snap), P(d_list), n),
        "load_streams_device": lambda: b.load_streams_device(P(d_snap), P(d_list), n),
        "save_chunk_fifos_device": lambda: b.save_chunk_fifos_device(P(d_fifo), P(d_list), n),
        "load_chunk_fifos_device": lambda: b.load_chunk_fifos_device(P(d_fifo), P(d_list), n),
        "reset_streams_device": lambda: b.reset_streams_device(P(d_list), n),
        "add_model": lambda: b.add_model(little),
        "set_stream_models": lambda: b.set_stream_models(np.zeros(n, np.uint8)),
        "set_stream_models_device": lambda: b.set_stream_models_device(P(d_bytes)),
        "set_stream_controls_device": lambda: b.set_stream_controls_device(P(d_ctl)),
        "set_stream_rates_device": lambda: b.set_stream_rates_device(P(d_bytes)),
        "set_stream_formats_device": lambda: b.set_stream_formats_device(P(d_bytes)),
        "set_stream_out_rates_device": lambda: b.set_stream_out_rates_device(P(d_bytes)),
        "set_stream_out_formats_device": lambda: b.set_stream_out_formats_device(P(d_bytes)),
        "process_device": lambda: b.process_device(P(d_out), P(d_pcm), P(d_vad), P(d_gains), Tn),
        "process_device_s16": lambda: b.process_device(P(d_out16), P(d_pcm16), P(d_vad), P(d_gains), Tn, s16=True),
        "process_masked_device": lambda: b.process_masked_device(P(d_out), P(d_pcm), P(d_vad), P(d_gains), P(d_act), Tn),
        "process_list_device": lambda: b.process_list_device(P(d_out), P(d_pcm), P(d_vad), P(d_gains), P(d_list), n, 0, Tn),
        "process_list_device, empty": lambda: b.process_list_device(P(d_out), P(d_pcm), 0, 0, 0, 0, 0, Tn),
        "process_chunks_device": lambda: b.process_chunks_device(P(d_out), P(d_pcm), P(d_counts), 100, P(d_vad), P(d_gains), P(d_frames)),
        "process_chunks_list": lambda: b.process_chunks_list(chunk, np.full(n, 100), np.arange(n)),
        "process_chunks_list, empty": lambda: b.process_chunks_list(chunk[:0], np.zeros(0, np.int32), np.zeros(0, np.int32)),
        "process_chunks_list_device": lambda: b.process_chunks_list_device(P(d_out), P(d_pcm), P(d_counts), 100, P(d_list), n, P(d_vad),
                                                                           P(d_gains), P(d_frames)),
        "analyze_device": lambda: b.analyze_device(P(z((Tn, n, 65))), 0, P(d_pcm), Tn),
    }
    for name, call in others.items():
        with pytest.raises((RuntimeError, ValueError)):
            call()
        assert b.split_pending == Tn, name
    # nothing was launched and nothing changed: the pair gives the twin's bits, and the batch the twin's snapshot
    vad, gains = b.process_features(feats)
    assert_bits_equal(b.synthesize(gains, vad), w_out, "the pair after the refused calls")
    assert_bits_equal(gains, w_gains, "gains")
    assert_bits_equal(b.save_streams(), twin.save_streams(), "snapshots after the refused calls")
    assert_bits_equal(b.save_chunk_fifos(), twin.save_chunk_fifos(), "FIFO records after the refused calls")
    assert b.stream_models().max() == 0
    b.close(), twin.close(), free.close()


def test_process_makes_its_own_output_under_channels_and_a_layout(model):
    """Batch.process with interleaved channels and a PCM layout and no `out`: the fresh output spans the rows of the call (it was
    sized by its channel groups, half of them at two channels, and the library wrote past its end)"""
    n, Tn, ch = 12, 3, 2
    b, twin = capi.Batch(model, n), capi.Batch(model, n)
    for x in (b, twin):
        x.set_pcm_channels(ch)
        x.set_pcm_layout(6 * 964 + 8, 964)
    pcm = twin.pcm_array(Tn, np.float32)
    pcm[...] = np.random.default_rng(11).integers(-6000, 6000, pcm.shape).astype(np.float32)
    w_out, w_vad, _ = twin.process(pcm, out=twin.pcm_array(Tn))
    out, vad, _ = b.process(pcm)
    assert out.shape == pcm.shape == w_out.shape and out.base.size == w_out.base.size
    assert_bits_equal(out, w_out, "out"), assert_bits_equal(vad, w_vad, "vad")
    pcm16 = b.pcm_array(Tn, np.int16)
    pcm16[...] = pcm
    out16, _, _ = b.process_s16(pcm16)
    assert out16.shape == pcm.shape and out16.base.size == w_out.base.size
    b.close(), twin.close()
