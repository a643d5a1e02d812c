"""Interleaved channels on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels).  The oracle of every test is the planar
call, which the rest of the suite pins to the reference: twin batches of one configuration get the same samples, batch A planar in
the default [frames][rows][M] layout, batch B with a channel count (and maybe a layout) over buffers pre-filled with a canary.  B's
samples of out -- gathered from the positions the header documents --, its vad, its gains and the snapshots of every stream after the
last call must equal A's bit for bit, and every byte of B's `out` that no present row owns -- padding, the positions of a low-rate
or companded row it does not use, the samples of an absent channel -- must still hold the canary.  The unused parts of `in` hold
NaN / junk: a kernel that read them would not reproduce A.

Everything is addressed in BYTES here, so that float, int16 and companded rows go through one index function."""
import os

import numpy as np
import pytest

from conftest import assert_bits_equal
from rnnoise_amd import capi, g711, synth, wav

pytestmark = [pytest.mark.gpu, pytest.mark.rcp("host")]
PAD = 48  # bytes behind the last slot of every buffer: nothing may land there either
CANARY, JUNK_F32 = 0xA5, np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
DISTINCT = 12


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


@pytest.fixture(scope="module")
def base():
    """(4, DISTINCT, 480) float32 of integer samples: the synth streams, shared by every test and never written"""
    b = synth.batch_pcm(range(DISTINCT), 4)
    b.setflags(write=False)
    return b


def samples(base, n, T, dtype, M=480):
    """(T, n, M) of `dtype`: stream s takes base stream s mod DISTINCT, scaled so that copies differ"""
    s = np.arange(n)
    x = base[:T, s % DISTINCT, :M] * (1.0 - 0.125 * ((s // DISTINCT) % 5))[None, :, None].astype(np.float32)
    return np.ascontiguousarray(np.trunc(x).astype(dtype))


class Run:
    """the device buffers of T frames x rows rows of M samples of `dtype`, planar (C = 1, no layout) or interleaved C at a time under
    layout `lay` ((frame_stride, row_stride) in samples; None: the default).  used[r] / comp[r]: the samples row r uses per frame, and
    whether it holds them as bytes (a companded stream of an int16 call).  `in` holds pcm's used samples and junk elsewhere, `out` the
    canary everywhere (alias: `out` is `in`)."""

    def __init__(self, torch, pcm, C=1, lay=None, alias=False, used=None, comp=None):
        self.torch, self.alias, self.C = torch, alias, C
        self.T, self.rows, self.M = pcm.shape
        self.it = pcm.dtype.itemsize
        self.dt = pcm.dtype
        self.fs, self.rs = lay if lay is not None else (self.rows * self.M, self.M * C)
        self.used = [self.M] * self.rows if used is None else list(used)
        self.comp = [False] * self.rows if comp is None else list(comp)
        G = self.rows // C
        self.nbytes = ((self.T - 1) * self.fs + (G - 1) * self.rs + self.M * C) * self.it + PAD
        junk = np.full(self.nbytes // self.it, JUNK_F32 if self.dt == np.float32 else 7777, self.dt).view(np.uint8)
        self.h_in = np.concatenate([junk, np.full(self.nbytes - junk.size, 0x5A, np.uint8)])
        src = np.ascontiguousarray(pcm).view(np.uint8).reshape(self.T, self.rows, self.M * self.it)
        for f in range(self.T):
            for r in range(self.rows):
                n = self.used[r] * (1 if self.comp[r] else self.it)
                self.h_in[self.at(f, r)] = src[f, r, :n]  # (a companded row's codes: the low bytes of its samples, any byte is a code)
        dev = torch.device("cuda", 0)
        self.d_in = torch.from_numpy(self.h_in).to(dev)
        self.d_out = self.d_in if alias else torch.full((self.nbytes,), CANARY, dtype=torch.uint8, device=dev)
        self.d_vad = torch.full((self.T, self.rows), -7.0, device=dev)
        self.d_g = torch.full((self.T, self.rows, 32), -7.0, device=dev)

    def at(self, f, r):
        """byte indices of the samples row r uses in frame f: sample i of channel c of group g at f * fs + g * rs + i * C + c, a
        companded row's byte i at byte i * C + c of its group slot"""
        g, c = divmod(r, self.C)
        e = 1 if self.comp[r] else self.it
        first = (f * self.fs + g * self.rs) * self.it + c * e
        return (first + np.arange(self.used[r])[:, None] * (self.C * e) + np.arange(e)[None, :]).reshape(-1)

    def call(self, b, f0, k, active=None, streams=None):
        """frames [f0, f0 + k) as one device call of b: lock-step, masked (active) or list (streams[, active]); returns rc"""
        torch, dev = self.torch, self.d_in.device
        s16 = self.dt == np.int16
        po, pi = self.d_out.data_ptr() + f0 * self.fs * self.it, self.d_in.data_ptr() + f0 * self.fs * self.it
        pv, pg = self.d_vad.data_ptr() + f0 * self.rows * 4, self.d_g.data_ptr() + f0 * self.rows * 128
        d_act = torch.from_numpy(np.ascontiguousarray(active, np.uint8)).to(dev) if active is not None else None
        L, h = b._L, b.h
        torch.cuda.synchronize()
        if streams is not None:
            d_list = torch.from_numpy(np.ascontiguousarray(streams, np.int32)).to(dev)
            fn = L.rnnoise_batch_process_device_list_s16 if s16 else L.rnnoise_batch_process_device_list
            rc = fn(h, po, pi, pv, pg, d_list.data_ptr(), len(streams), d_act.data_ptr() if d_act is not None else None, k, None)
        elif active is not None:
            fn = L.rnnoise_batch_process_device_masked_s16 if s16 else L.rnnoise_batch_process_device_masked
            rc = fn(h, po, pi, pv, pg, d_act.data_ptr(), k, None)
        else:
            fn = L.rnnoise_batch_process_device_s16 if s16 else L.rnnoise_batch_process_device
            rc = fn(h, po, pi, pv, pg, k, None)
        torch.cuda.synchronize()
        return rc

    def result(self, what, present=None):
        """([T][rows] lists of the bytes each present row wrote, vad, gains) after checking that every byte of `out` outside the used
        samples of the present rows holds what it held before the call, and that `in` was not written"""
        flat = self.d_out.cpu().numpy()
        before = self.h_in if self.alias else np.full(self.nbytes, CANARY, np.uint8)
        owned = np.zeros(self.nbytes, bool)
        got = [[None] * self.rows for _ in range(self.T)]
        for f in range(self.T):
            for r in range(self.rows):
                if present is None or present[f][r]:
                    idx = self.at(f, r)
                    assert not owned[idx].any(), "test bug: two rows own one byte"
                    owned[idx] = True
                    got[f][r] = flat[idx].copy()
        bad = (flat != before) & ~owned
        assert not bad.any(), f"{what}: {int(bad.sum())} bytes outside the present rows' samples were written (first at byte {int(np.argmax(bad))})"
        if not self.alias:
            assert np.array_equal(self.d_in.cpu().numpy(), self.h_in), f"{what}: `in` was written"
        return got, self.d_vad.cpu().numpy(), self.d_g.cpu().numpy()


def compare(ra, rb, A, B, what, present=None):
    (oa, va, ga), (ob, vb, gb) = ra.result(what + " [planar]", present), rb.result(what, present)
    for f in range(ra.T):
        for r in range(ra.rows):
            if oa[f][r] is not None:
                assert np.array_equal(oa[f][r], ob[f][r]), f"{what}: out of frame {f}, row {r} differs in {int((oa[f][r] != ob[f][r]).sum())} bytes"
    assert_bits_equal(va, vb, what + ": vad")
    assert_bits_equal(ga, gb, what + ": gains")
    assert_bits_equal(A.save_streams(), B.save_streams(), what + ": snapshots of every stream")


def twins(model, n, C, lay=None, setup=None):
    A, B = capi.Batch(model, n), capi.Batch(model, n)
    for b in (A, B):
        if setup:
            setup(b)
    assert B.pcm_channels == 1 and B.set_pcm_channels(C) == 1 and B.pcm_channels == C and A.pcm_channels == 1
    if lay is not None:
        B.set_pcm_layout(*lay)
    return A, B


def run_twins(torch, model, pcm, C, calls, what, lay=None, alias=False, setup=None, used=None, comp=None):
    A, B = twins(model, pcm.shape[1], C, lay, setup)
    ra, rb = Run(torch, pcm, used=used, comp=comp), Run(torch, pcm, C, lay, alias, used=used, comp=comp)
    f0 = 0
    for k in calls:
        assert ra.call(A, f0, k) == 0 and rb.call(B, f0, k) == 0, what
        f0 += k
    compare(ra, rb, A, B, what)
    return A, B


# ---- 1. the default layout: each frame [rows / C][M][C] ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("C", [2, 3])
def test_default_layout(torch, model, base, dtype, C):
    run_twins(torch, model, samples(base, 12, 4, dtype), C, (1, 3), f"C = {C}, {np.dtype(dtype).name}, calls of 1 + 3 frames")


# ---- 2. with a layout: a [G][T][C] tensor, and row and frame padding; in aliasing out ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("shape", ["GTC", "padded", "GTC-aliased", "padded-aliased"])
def test_with_a_layout(torch, model, base, dtype, shape):
    C, T, M, n = 2, 4, 480, 12
    lay = (M * C, T * M * C) if shape.startswith("GTC") else ((n // C) * (M * C + 8) + 16, M * C + 8)
    assert capi.pcm_channels_fit(*lay, M, C, n, T)
    run_twins(torch, model, samples(base, n, T, dtype), C, (1, 3), f"{shape}, {np.dtype(dtype).name}", lay=lay, alias=shape.endswith("aliased"))


def test_channels_and_layout_in_either_order(torch, model, base):
    pcm = samples(base, 12, 2, np.int16)
    lay = (960, 2 * 960)
    A, B = capi.Batch(model, 12), capi.Batch(model, 12)
    B.set_pcm_layout(*lay)
    assert B.set_pcm_channels(2) == 1 and B.pcm_layout == lay
    assert B.set_pcm_rate(48000) == 48000 and B.pcm_layout == (0, 0) and B.pcm_channels == 2  # the rate call drops the layout only
    B.set_pcm_layout(*lay)
    B.reset()
    B.set_stream_controls(None)
    assert B.pcm_channels == 2  # configuration, not state
    ra, rb = Run(torch, pcm), Run(torch, pcm, 2, lay)
    assert ra.call(A, 0, 2) == 0 and rb.call(B, 0, 2) == 0
    compare(ra, rb, A, B, "layout set before the channel count")


# ---- 3. mixed groups at a 48 kHz batch: 48, 8 and 16 kHz channels in one slot, mu-law and A-law channels in one slot ----
def test_mixed_rates_and_formats_in_a_group(torch, model, base):
    """Channel 0 at 48 kHz, channel 1 at 8 kHz, channel 2 at 16 kHz in every group; the even groups linear, the odd groups companded
    with both laws side by side.  The issue asked for ONE group of a 48 kHz linear, an 8 kHz mu-law and a 16 kHz A-law channel.  That
    case cannot exist under the addressing it specifies: a linear channel 0 holds int16 sample 0 in bytes 0-1 of the slot and the
    companded channel 1 holds its byte 0 at byte 0 * C + 1 = 1 -- two rows own one byte (this harness found it: "two rows own one
    byte").  Channels of one group must share a sample width (include/rnnoise_amd.h); everything else the case asked for is here."""
    n, C, T = 12, 3, 4
    rates = [48000, 8000, 16000] * (n // C)
    fmts = ["s16", "s16", "s16", "alaw", "ulaw", "alaw", "s16", "s16", "s16", "ulaw", "ulaw", "alaw"]

    def setup(b):
        b.set_stream_rates(rates)
        b.set_stream_formats(fmts)
    used = [480 * r // 48000 for r in rates]
    comp = [f != "s16" for f in fmts]
    # (Run.result: the positions i * C + c with i >= 480 / L_s, and the high bytes a companded row never fills, keep the canary)
    A, B = run_twins(torch, model, samples(base, n, T, np.int16), C, (1, 3), "mixed group", setup=setup, used=used, comp=comp)
    assert B.pcm_channels == 3


# ---- 4. a masked call in which exactly one channel of a group is absent in some frame ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_masked_call_with_an_absent_channel(torch, model, base, dtype):
    n, C, T = 12, 2, 4
    act = np.ones((T, n), np.uint8)
    act[1, 3] = 0                 # group 1: channel 1 absent, channel 0 present
    act[2, 4] = 0                 # group 2: channel 0 absent
    act[2, 10] = act[2, 11] = 0   # a whole group absent
    act[3, 0] = 0
    pcm = samples(base, n, T, dtype)
    A, B = twins(model, n, C)
    ra, rb = Run(torch, pcm), Run(torch, pcm, C)
    assert ra.call(A, 0, 1, act[:1]) == 0 and rb.call(B, 0, 1, act[:1]) == 0
    assert ra.call(A, 1, 3, act[1:]) == 0 and rb.call(B, 1, 3, act[1:]) == 0
    compare(ra, rb, A, B, f"masked, {np.dtype(dtype).name}", present=act)  # (absent rows keep the canary: Run.result)


# ---- 5. a list call: 6 rows over 12 streams, the channels of a group non-adjacent streams ----
@pytest.mark.parametrize("masked", [False, True])
def test_list_call(torch, model, base, masked):
    n, C, T = 12, 2, 3
    streams = [7, 2, 11, 0, 4, 9]
    pcm = samples(base, n, T, np.int16)[:, streams]
    act = np.ones((T, len(streams)), np.uint8)
    if masked:
        act[1, 2] = 0  # row 2 = channel 0 of the list's group 1
        act[2, 5] = 0
    A, B = twins(model, n, C)
    ra, rb = Run(torch, pcm), Run(torch, pcm, C)
    # rows that fill no whole group: -1, nothing launched, nothing changed
    before = B.save_streams()
    assert rb.call(B, 0, 1, streams=streams[:5]) == -1
    assert_bits_equal(before, B.save_streams(), "a refused list call changed state")
    assert (rb.d_out.cpu().numpy() == CANARY).all() and (rb.d_vad.cpu().numpy() == -7.0).all()
    for f0, k in ((0, 1), (1, 2)):
        a = act[f0:f0 + k] if masked else None
        assert ra.call(A, f0, k, a, streams) == 0 and rb.call(B, f0, k, a, streams) == 0
    compare(ra, rb, A, B, f"list call, masked = {masked}", present=act)


# ---- 6. the host forms (staged path) ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("laid", [False, True])
def test_host_forms(model, base, dtype, laid):
    n, C, T, M = 12, 3, 3, 480
    pcm = samples(base, n, T, dtype)
    A, B = capi.Batch(model, n), capi.Batch(model, n)
    B.set_pcm_channels(C)
    if laid:
        B.set_pcm_layout(M * C + 8, T * (M * C + 8) + 4)
    fn = (lambda b, *a, **k: b.process(*a, **k)) if dtype == np.float32 else (lambda b, *a, **k: b.process_s16(*a, **k))
    oa, va, ga = fn(A, pcm)
    fill = np.array([0xFFC12345], np.uint32).view(np.float32)[0] if dtype == np.float32 else np.int16(-32768)
    x, out = B.pcm_array(T, dtype, fill=fill), B.pcm_array(T, dtype, fill=fill)
    assert x.shape == (T, n // C, M, C)
    x[...] = pcm.reshape(T, n // C, C, M).transpose(0, 1, 3, 2)
    ob, vb, gb = fn(B, x, out=out)
    assert ob is out
    assert np.array_equal(ob.transpose(0, 1, 3, 2).reshape(T, n, M).view(np.uint8 if dtype == np.int16 else np.uint32),
                          oa.view(np.uint8 if dtype == np.int16 else np.uint32))
    assert_bits_equal(va, vb, "vad")
    assert_bits_equal(ga, gb, "gains")
    assert_bits_equal(A.save_streams(), B.save_streams(), "snapshots")
    if laid:  # nothing but the slots was written on the host
        flat, mask = out.base, np.ones(out.base.size, bool)
        np.lib.stride_tricks.as_strided(mask, out.shape, tuple(s // flat.itemsize for s in out.strides))[...] = False
        assert mask.any() and (flat[mask].view(np.uint32 if dtype == np.float32 else np.uint16) == np.array([fill]).view(
            np.uint32 if dtype == np.float32 else np.uint16)[0]).all()


# ---- 7. above the K0 and K1 form switches (dispatch.h: 2,048 and 2,560 streams), the network's default path there ----
@pytest.mark.parametrize("n", [2304, 2816])
def test_above_the_form_switches(torch, model, base, n):
    run_twins(torch, model, samples(base, n, 2, np.int16), 2, (2,), f"{n} streams")


# ---- 8. back to one channel ----
def test_channel_count_of_one_drops_the_feature(torch, model, base):
    n, T = 12, 3
    pcm = samples(base, n, T, np.float32)
    A, B = twins(model, n, 2)
    ra, rb = Run(torch, pcm), Run(torch, pcm, 2)
    assert ra.call(A, 0, 2) == 0 and rb.call(B, 0, 2) == 0
    assert B.set_pcm_channels(1) == 2 and B.pcm_channels == 1
    rp = Run(torch, pcm)  # planar buffers for B's last frame
    assert ra.call(A, 2, 1) == 0 and rp.call(B, 2, 1) == 0
    (oa, va, ga), (op, vp, gp) = ra.result("A"), rp.result("B planar", present=[[f == 2] * n for f in range(T)])
    for r in range(n):
        assert np.array_equal(oa[2][r], op[2][r]), r
    assert_bits_equal(va[2], vp[2], "vad")
    assert_bits_equal(ga[2], gp[2], "gains")
    assert_bits_equal(A.save_streams(), B.save_streams(), "snapshots")
    # the refusals of the setter, with a batch: nothing changes
    for bad in (0, -1, 9, 5, 8):
        assert B._L.rnnoise_batch_set_pcm_channels(B.h, bad) == -1 and B.pcm_channels == 1
    with pytest.raises(ValueError):
        B.set_pcm_channels(5)
    # training-feature extraction refuses a channel count
    B.set_pcm_channels(2)
    z = torch.zeros(n * 480, device="cuda")
    zi = torch.zeros(n, dtype=torch.int32, device="cuda")
    rec = torch.zeros(n * 98, device="cuda")
    args = (rec.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), zi.data_ptr(), zi.data_ptr(), zi.data_ptr(), 1, None)
    fresh = capi.Batch(model, n)
    assert fresh._L.rnnoise_batch_train_features_device(fresh.h, *args) == 0
    assert B._L.rnnoise_batch_train_features_device(B.h, *args) == -1


# ---- 9. the torch op ----
@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_torch_op_process_channels(torch, blob_default, base, dtype):
    from rnnoise_amd.torch_op import RNNoiseOp
    G, C, T, M = 6, 2, 3, 480
    planar = samples(base, G * C, T, np.dtype(dtype))                       # (T, 12, 480)
    streams = torch.from_numpy(np.ascontiguousarray(planar.transpose(1, 0, 2)).reshape(G * C, T * M)).cuda()
    inter = streams.reshape(G, C, T * M).permute(0, 2, 1).contiguous()      # (6, 3 * 480, 2)
    a, b = RNNoiseOp(blob_default, G * C), RNNoiseOp(blob_default, G * C)
    oa, va, ga = a.process_streams(streams)
    ob, vb, gb = b.process_channels(inter)
    assert ob.shape == inter.shape and ob.dtype == inter.dtype and vb.shape == (T, G * C) and gb.shape == (T, G * C, 32)
    assert torch.equal(ob.permute(0, 2, 1).reshape(G * C, T * M), oa)
    assert_bits_equal(va.cpu().numpy(), vb.cpu().numpy(), "vad")
    assert_bits_equal(ga.cpu().numpy(), gb.cpu().numpy(), "gains")
    assert b.batch.pcm_channels == 2 and b.batch.pcm_layout == (M * C, T * M * C)
    act = torch.ones((T, G * C), dtype=torch.uint8, device="cuda")
    act[1, 5] = 0
    om, _, _ = b.process_channels(inter, act)
    assert (om[2, M:2 * M, 1] == 0).all() and bool((om[2, M:2 * M, 0] != 0).any())  # stream 5 = group 2, channel 1: absent in frame 1


# ---- 10. the CLI: WAV files in, the same samples as their de-interleaved channels as RAW files ----
def test_cli_wav(tmp_path, blob_default, base):
    from rnnoise_amd import cli
    T = 4
    st = samples(base, 2, T, np.int16).transpose(1, 0, 2).reshape(2, T * 480)               # two 48 kHz channels
    mono8 = g711.encode(samples(base, 3, T, np.int16, 80)[:, 2].reshape(-1), "ulaw")        # 8 kHz mu-law codes
    rawx = samples(base, 4, T, np.int16)[:, 3].reshape(-1)
    d = tmp_path / "in"
    d.mkdir()
    wav.write(str(d / "st.wav"), wav.WavInfo(48000, 2, "s16", False, 0, 0), st.T)
    wav.write(str(d / "m.wav"), wav.WavInfo(8000, 1, "ulaw", False, 0, 0), mono8.reshape(-1, 1))
    rawx.tofile(str(d / "x.raw"))
    st[0].tofile(str(d / "l.raw")), st[1].tofile(str(d / "r.raw")), mono8.tofile(str(d / "m.ul"))
    (tmp_path / "w.blob").write_bytes(blob_default)
    cli.main(["denoise", "--model", str(tmp_path / "w.blob"), "--out-dir", str(tmp_path / "a"), "--chunk-frames", "3",
              str(d / "st.wav"), str(d / "m.wav"), str(d / "x.raw")])
    cli.main(["denoise", "--model", str(tmp_path / "w.blob"), "--out-dir", str(tmp_path / "b"), "--chunk-frames", "3",
              "--rates", "48000,48000,8000,48000", "--formats", "s16,s16,ulaw,s16",
              str(d / "l.raw"), str(d / "r.raw"), str(d / "m.ul"), str(d / "x.raw")])
    rd = lambda p, dt: np.fromfile(str(p), dt)
    info, y = wav.read(str(tmp_path / "a" / "st.wav.denoised.wav"))
    assert (info.rate, info.channels, info.codec, info.extensible) == (48000, 2, "s16", False) and y.shape == ((T - 1) * 480, 2)
    assert np.array_equal(y[:, 0], rd(tmp_path / "b" / "l.raw.denoised.raw", np.int16)) and y.any()
    assert np.array_equal(y[:, 1], rd(tmp_path / "b" / "r.raw.denoised.raw", np.int16))
    info, y = wav.read(str(tmp_path / "a" / "m.wav.denoised.wav"))
    assert (info.rate, info.channels, info.codec) == (8000, 1, "ulaw") and y.shape == ((T - 1) * 80, 1)
    assert np.array_equal(y[:, 0], rd(tmp_path / "b" / "m.ul.denoised.raw", np.uint8))
    assert np.array_equal(rd(tmp_path / "a" / "x.raw.denoised.raw", np.int16), rd(tmp_path / "b" / "x.raw.denoised.raw", np.int16))
    assert os.path.getsize(tmp_path / "a" / "x.raw.denoised.raw") == (T - 1) * 960
