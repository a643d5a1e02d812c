"""Caller-defined PCM strides on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout).  The oracle of every test is the
default layout, which the rest of the suite pins to the reference: twin batches of one model get the same frames, batch A in the
default [frames][rows][M] layout, batch B through a layout over buffers pre-filled with a sentinel.  B's strided samples of out, its
vad, gains and the snapshots of every stream after the last call must equal A's bit for bit, and every word of B's buffers outside
the frame slots must still hold what it held before the call.  (The tail of a slot behind a low-rate or companded stream's samples
is compared with A's, which starts from the same sentinel.)  The unread parts of `in` hold NaN / junk: a kernel that read them would
not reproduce A.

Buffers span the whole run and the calls walk through them frame by frame -- the way a [B, T] tensor is consumed."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from rnnoise_amd import capi, g711, synth

pytestmark = [pytest.mark.gpu, pytest.mark.rcp("host")]
PAD = 24  # words behind the last slot of every buffer: nothing may land there either
SENT = {np.dtype(np.float32): np.array([0xFFC12345], np.uint32).view(np.float32)[0], np.dtype(np.int16): np.int16(-32768)}
JUNK = {np.dtype(np.float32): np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0], np.dtype(np.int16): np.int16(7777)}
DISTINCT = 97


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


@pytest.fixture(scope="module")
def base():
    """(6, DISTINCT, 480) float32 of integer samples: the synth streams, shared by every test and never written"""
    b = synth.batch_pcm(range(DISTINCT), 6)
    b.setflags(write=False)
    return b


def frames_of(base, n, T, dtype, M=480):
    """(T, n, M) of `dtype`: stream s takes base stream s mod DISTINCT, scaled so that neighbouring copies differ"""
    s = np.arange(n)
    x = base[:T, s % DISTINCT, :M] * (1.0 - 0.25 * ((s // DISTINCT) % 3))[None, :, None].astype(np.float32)
    return np.ascontiguousarray(np.trunc(x).astype(dtype))


def strided(flat, fs, rs, T, rows, M):
    it = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat, (T, rows, M), (fs * it, rs * it, it))


class Buf:
    """the device buffers of one run of T frames x rows: PCM in layout `lay` ((frame_stride, row_stride), None: the default), `in`
    holding pcm in its slots and junk elsewhere, `out` the sentinel everywhere (alias: `out` is `in`)"""

    def __init__(self, torch, pcm, lay=None, alias=False):
        self.torch, self.alias = torch, alias
        self.T, self.rows, self.M = pcm.shape
        self.fs, self.rs = lay if lay is not None else (self.rows * self.M, self.M)
        self.dt = pcm.dtype
        n = (self.T - 1) * self.fs + (self.rows - 1) * self.rs + self.M + PAD
        self.h_in = np.full(n, JUNK[self.dt], self.dt)
        strided(self.h_in, self.fs, self.rs, *pcm.shape)[...] = pcm
        self.slots = np.zeros(n, bool)
        strided(self.slots, self.fs, self.rs, *pcm.shape)[...] = True
        dev = torch.device("cuda", 0)
        self.d_in = torch.from_numpy(self.h_in).to(dev)
        self.d_out = self.d_in if alias else torch.from_numpy(np.full(n, SENT[self.dt], self.dt)).to(dev)
        self.d_vad = torch.full((self.T, self.rows), -7.0, device=dev)
        self.d_g = torch.full((self.T, self.rows, 32), -7.0, device=dev)

    def call(self, b, f0, k, active=None, streams=None):
        """frames [f0, f0 + k) of the run as one device call of b: lock-step, masked (active) or list (streams[, active]); returns rc"""
        torch, it = self.torch, self.h_in.itemsize
        dev = self.d_in.device
        s16 = self.dt == np.int16
        po, pi = self.d_out.data_ptr() + f0 * self.fs * it, self.d_in.data_ptr() + f0 * self.fs * it
        pv, pg = self.d_vad.data_ptr() + f0 * self.rows * 4, self.d_g.data_ptr() + f0 * self.rows * 128
        d_act = torch.from_numpy(np.ascontiguousarray(active, np.uint8)).to(dev) if active is not None else None
        L, h = b._L, b.h
        torch.cuda.synchronize()
        if streams is not None:
            d_list = torch.from_numpy(np.ascontiguousarray(streams, np.int32)).to(dev)
            fn = L.rnnoise_batch_process_device_list_s16 if s16 else L.rnnoise_batch_process_device_list
            rc = fn(h, po, pi, pv, pg, d_list.data_ptr(), self.rows, d_act.data_ptr() if d_act is not None else None, k, None)
        elif active is not None:
            fn = L.rnnoise_batch_process_device_masked_s16 if s16 else L.rnnoise_batch_process_device_masked
            rc = fn(h, po, pi, pv, pg, d_act.data_ptr(), k, None)
        else:
            fn = L.rnnoise_batch_process_device_s16 if s16 else L.rnnoise_batch_process_device
            rc = fn(h, po, pi, pv, pg, k, None)
        torch.cuda.synchronize()
        return rc

    def result(self, what):
        """(out (T, rows, M), vad, gains) as numpy, after checking that nothing outside the frame slots was written"""
        flat = self.d_out.cpu().numpy()
        before = self.h_in if self.alias else np.full(flat.size, SENT[self.dt], self.dt)
        outside = ~self.slots
        assert np.array_equal(raw(flat)[outside], raw(before)[outside]), \
            f"{what}: {int((raw(flat)[outside] != raw(before)[outside]).sum())} words outside the frame slots of `out` were written"
        if not self.alias:
            assert np.array_equal(raw(self.d_in.cpu().numpy()), raw(self.h_in)), f"{what}: `in` was written"
        return strided(flat, self.fs, self.rs, self.T, self.rows, self.M).copy(), self.d_vad.cpu().numpy(), self.d_g.cpu().numpy()


def twins(model, n, lay, setup=None, schedule=None):
    A, B = capi.Batch(model, n), capi.Batch(model, n)
    for b in (A, B):
        if setup:
            setup(b)
        if schedule is not None:
            b.set_schedule(schedule)
    B.set_pcm_layout(*lay)
    assert B.pcm_layout == tuple(lay) and A.pcm_layout == (0, 0)
    return A, B


def run_twins(torch, A, B, pcm, lay, calls, what, alias=False):
    """the same lock-step calls on A (default layout) and B (layout `lay`); everything compared"""
    ba, bb = Buf(torch, pcm), Buf(torch, pcm, lay, alias=alias)
    f0 = 0
    for k in calls:
        assert ba.call(A, f0, k) == 0 and bb.call(B, f0, k) == 0, what
        f0 += k
    compare(ba, bb, A, B, what)


def compare(ba, bb, A, B, what):
    (oa, va, ga), (ob, vb, gb) = ba.result(what + " [default layout]"), bb.result(what)
    assert np.array_equal(raw(oa), raw(ob)), f"{what}: out differs in {int((raw(oa) != raw(ob)).sum())} samples"
    assert_bits_equal(va, vb, what + ": vad")
    assert_bits_equal(ga, gb, what + ": gains")
    assert_bits_equal(A.save_streams(), B.save_streams(), what + ": snapshots of every stream")
    return oa, va, ga


# ---- 1. 70 streams: the wave-per-stream K0, rn_synthesis_few_kernel and the one-stream forms ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("shape", ["stream-contiguous", "row-major-padded", "stream-contiguous-aliased"])
def test_small_batch(torch, model, base, dtype, shape):
    n, T, M = 70, 6, 480
    lay = (n * (M + 8), M + 8) if shape == "row-major-padded" else (M, T * M)
    A, B = twins(model, n, lay)
    pcm = frames_of(base, n, T, dtype)
    run_twins(torch, A, B, pcm, lay, (1, 5), f"70 streams {shape} {np.dtype(dtype).name}", alias=shape.endswith("aliased"))
    A.close(), B.close()


# ---- 2. 2,564 streams: the smallest batch on the lane = stream K0 and the at-size K1 / K3, ragged in every unit ----
@pytest.mark.parametrize("schedule", [0, 9])
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_lane_form(torch, model, base, dtype, schedule):
    n, T, M = 2564, 5, 480
    lay = (M, T * M)
    A, B = twins(model, n, lay, schedule=schedule)
    pcm = frames_of(base, n, T, dtype)
    run_twins(torch, A, B, pcm, lay, (1, 4), f"2564 streams schedule {schedule} {np.dtype(dtype).name}")
    A.close(), B.close()


# ---- 3. rate and format tables under a layout ----
def test_rates_and_formats_48k(torch, model, base):
    n, T, M = 70, 6, 480
    s = np.arange(n)
    Ls = np.array([1, 2, 3, 6])[s % 4]
    fmts = ((s + s // 4) % 3).astype(np.uint8)

    def setup(b):
        b.set_stream_rates(48000 // Ls)
        b.set_stream_formats(fmts)
    lay = (M, T * M)
    A, B = twins(model, n, lay, setup)
    x = frames_of(base, n, T, np.int16)
    pcm = np.full_like(x, JUNK[x.dtype])
    p8 = pcm.view(np.uint8)
    for i in range(n):
        m = M // int(Ls[i])
        if fmts[i]:
            p8[:, i, :m] = g711.encode(x[:, i, :m], int(fmts[i]))  # (bytes at the front of the slot; junk int16 behind them)
        else:
            pcm[:, i, :m] = x[:, i, :m]
    run_twins(torch, A, B, pcm, lay, (1, 5), "48 kHz batch, four rates and three formats interleaved")
    A.close(), B.close()


def test_rates_16k(torch, model, base):
    n, T, M = 70, 6, 160
    Ls = np.array([3, 6])[np.arange(n) % 2]

    def setup(b):
        b.set_pcm_rate(16000)
        b.set_stream_rates(48000 // Ls)
    lay = (M, T * M)
    A, B = twins(model, n, lay, setup)
    assert B.frame == M
    x = frames_of(base, n, T, np.float32, M)
    pcm = np.full_like(x, JUNK[x.dtype])
    for i in range(n):
        m = 480 // int(Ls[i])
        pcm[:, i, :m] = x[:, i, :m]
    run_twins(torch, A, B, pcm, lay, (1, 5), "16 kHz batch with a 16 / 8 kHz rate table")
    A.close(), B.close()


# ---- 4. masked and list calls ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_masked_and_list(torch, model, base, dtype):
    n, T, M = 130, 6, 480
    rng = np.random.Generator(np.random.PCG64(130))
    lay = (M, 3 * M)
    A, B = twins(model, n, lay)
    pcm = frames_of(base, n, T, dtype)
    act = (rng.random((3, n)) < 0.6).astype(np.uint8)
    act[:, 5] = 0
    ba, bb = Buf(torch, pcm[:3]), Buf(torch, pcm[:3], lay)
    assert ba.call(A, 0, 3, active=act) == 0 and bb.call(B, 0, 3, active=act) == 0
    oa, _, _ = compare(ba, bb, A, B, "masked call")
    assert (raw(oa)[act == 0] == raw(np.array([SENT[pcm.dtype]]))[0]).all(), "an absent frame's out slot was written"
    rows = rng.permutation(n)[:37].astype(np.int32)
    lact = (rng.random((3, 37)) < 0.7).astype(np.uint8)
    lact[1, 4] = 0
    lp = np.ascontiguousarray(pcm[3:6][:, rows])
    ba, bb = Buf(torch, lp), Buf(torch, lp, lay)
    assert ba.call(A, 0, 3, active=lact, streams=rows) == 0 and bb.call(B, 0, 3, active=lact, streams=rows) == 0
    oa, _, _ = compare(ba, bb, A, B, "list call of 37 shuffled rows")
    assert (raw(oa)[lact == 0] == raw(np.array([SENT[pcm.dtype]]))[0]).all(), "an absent row's out slot was written"
    assert (raw(oa)[lact != 0] != raw(np.array([SENT[pcm.dtype]]))[0]).any()
    A.close(), B.close()


# ---- 5. host forms on pageable arrays viewed with the layout's strides, against the device form ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("shape", ["stream-contiguous", "row-major-padded"])
def test_host_forms(torch, model, base, dtype, shape):
    n, T, M = 70, 4, 480
    lay = (n * (M + 8), M + 8) if shape == "row-major-padded" else (M, T * M)
    A, B = twins(model, n, lay)
    pcm = frames_of(base, n, T + 2, dtype)
    ba = Buf(torch, pcm)
    assert ba.call(A, 0, T) == 0
    act = (np.random.Generator(np.random.PCG64(5)).random((2, n)) < 0.5).astype(np.uint8)
    assert ba.call(A, T, 2, active=act) == 0
    oa, va, ga = ba.result("device form")
    x, out = B.pcm_array(T, dtype, fill=JUNK[np.dtype(dtype)]), B.pcm_array(T, dtype, fill=SENT[np.dtype(dtype)])
    x[...] = pcm[:T]
    keep = x.base.copy()
    o, v, g = (B.process_s16 if dtype == np.int16 else B.process)(x, out=out)
    assert o is out and np.array_equal(raw(x.base), raw(keep))
    assert np.array_equal(raw(np.ascontiguousarray(o)), raw(oa[:T]))
    assert_bits_equal(v, va[:T], "vad")
    assert_bits_equal(g, ga[:T], "gains")
    slots = np.zeros(out.base.size, bool)
    strided(slots, *lay, T, n, M)[...] = True
    assert (raw(out.base)[~slots] == raw(np.array([SENT[np.dtype(dtype)]]))[0]).all(), "the host call wrote outside the frame slots"
    # the masked host form; absent slots keep the sentinel
    x2, out2 = B.pcm_array(2, dtype, fill=JUNK[np.dtype(dtype)]), B.pcm_array(2, dtype, fill=SENT[np.dtype(dtype)])
    x2[...] = pcm[T:]
    o2, v2, g2 = (B.process_masked_s16 if dtype == np.int16 else B.process_masked)(x2, act, out=out2)
    assert np.array_equal(raw(np.ascontiguousarray(o2)), raw(oa[T:]))
    assert_bits_equal(v2, va[T:], "masked vad")
    assert_bits_equal(g2, ga[T:], "masked gains")
    assert_bits_equal(A.save_streams(), B.save_streams(), "snapshots")
    with pytest.raises(ValueError):  # an array that does not lie in the layout is refused, not copied
        B.process(np.zeros((T, n, M), np.float32))
    A.close(), B.close()


# ---- 6. rejections, and what drops the layout ----
def test_rejections(torch, model, base):
    n, T, M = 70, 3, 480
    A, B = capi.Batch(model, n), capi.Batch(model, n)
    for bad in ((0, 480), (480, 0), (-480, 480), (482, 4820), (480, 4802)):
        with pytest.raises(ValueError):
            B.set_pcm_layout(*bad)
        assert B.pcm_layout == (0, 0)
    pcm = frames_of(base, n, 2 * T, np.float32)
    lay = (M, T * M)
    B.set_pcm_layout(*lay)
    run = lambda b, buf, f0, k: buf.call(b, f0, k)
    ba, bb = Buf(torch, pcm[:T]), Buf(torch, pcm[:T], lay)
    assert run(A, ba, 0, T) == 0 and run(B, bb, 0, T) == 0
    compare(ba, bb, A, B, "first call")
    # overlapping: one frame more than the rows have room for, and rows closer than a frame -- -1, nothing launched or changed
    snap = B.save_streams()
    big = Buf(torch, frames_of(base, n, T + 1, np.float32), (M, (T + 1) * M))
    assert big.call(B, 0, T + 1) == -1
    B.set_pcm_layout(M - 4, T * M)
    assert bb.call(B, 0, 1) == -1
    B.set_pcm_layout(2 * M, M)  # (row-major needs frame_stride >= 70 rows)
    assert bb.call(B, 0, 2) == -1
    assert big.call(B, 0, 1, active=np.ones((1, n), np.uint8)) == -1
    assert_bits_equal(B.save_streams(), snap, "a refused call changed a stream")
    assert (raw(big.d_out.cpu().numpy()) == raw(np.array([SENT[np.dtype(np.float32)]]))[0]).all()
    # configuration, not state: reset_streams, import / load and reset leave it alone; set_pcm_rate drops it
    B.set_pcm_layout(*lay)
    B.reset_streams([3])
    A.reset_streams([3])
    B.load_streams(B.save_streams())
    assert B.pcm_layout == lay
    # extraction is refused under a layout and works again without one
    dev = torch.device("cuda", 0)
    z = lambda *s, dt=torch.float32: torch.zeros(s, device=dev, dtype=dt)
    rec, cl, nz, vd = z(1, n, 98), z(1, n, 480), z(1, n, 480), z(1, n)
    lp, bl, nf = torch.full((n,), 481, device=dev, dtype=torch.int32), torch.full((n,), 32, device=dev, dtype=torch.int32), z(n, dt=torch.int32)
    targs = [t.data_ptr() for t in (rec, cl, nz, vd, lp, bl, nf)] + [1, None]
    C, D = capi.Batch(model, n), capi.Batch(model, n)
    C.set_pcm_layout(*lay)
    torch.cuda.synchronize()
    assert C._L.rnnoise_batch_train_features_device(C.h, *targs) == -1
    C.set_pcm_layout(0, 0)
    assert C._L.rnnoise_batch_train_features_device(C.h, *targs) == 0
    assert D._L.rnnoise_batch_train_features_device(D.h, *targs) == 0
    torch.cuda.synchronize()
    assert_bits_equal(C.save_streams(), D.save_streams(), "the refused extraction call left a trace")
    C.close(), D.close()
    assert B.set_pcm_rate(48000) == 48000 and B.pcm_layout == (0, 0)
    B.set_pcm_layout(*lay)
    assert B.set_pcm_rate(16000) == 48000 and B.pcm_layout == (0, 0) and B.set_pcm_rate(48000) == 16000
    # ... and after (0, 0) the batch goes on bit for bit as its twin
    ba, bb = Buf(torch, pcm[T:]), Buf(torch, pcm[T:])
    assert run(A, ba, 0, T) == 0 and run(B, bb, 0, T) == 0
    compare(ba, bb, A, B, "after the layout was dropped")
    A.close(), B.close()


# ---- 7. the torch op's stream-contiguous entry point against its frame-major one ----
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_torch_process_streams(torch, blob_default, base, dtype):
    from rnnoise_amd.torch_op import RNNoiseOp
    n, T, M = 70, 3, 480
    dev = torch.device("cuda", 0)
    a, b = RNNoiseOp(blob_default, n), RNNoiseOp(blob_default, n)
    pcm = frames_of(base, n, 2 * T, dtype)
    act = (np.random.Generator(np.random.PCG64(9)).random((T, n)) < 0.6).astype(np.uint8)

    def frame_major(x, active=None):
        if dtype == np.float32:
            xt = torch.from_numpy(x).to(dev)
            return a(xt) if active is None else a.process_masked(xt, torch.from_numpy(active).to(dev))
        buf = Buf(torch, x)  # (the op's frame-major calls are float: the batch's int16 device call stands in)
        buf.d_out.zero_()
        assert buf.call(a.batch, 0, x.shape[0], active=active) == 0
        return buf.d_out[:x.size].reshape(x.shape), buf.d_vad, buf.d_g

    for part, active in ((pcm[:T], None), (pcm[T:], act)):
        bt = torch.from_numpy(np.ascontiguousarray(part.transpose(1, 0, 2)).reshape(n, T * M)).to(dev)  # [B, T * M]
        keep = bt.clone()
        o, v, g = b.process_streams(bt, None if active is None else torch.from_numpy(active).to(dev))
        wo, wv, wg = frame_major(part, active)
        assert o.shape == bt.shape and o.dtype == bt.dtype and o.is_contiguous() and torch.equal(bt, keep)
        got = o.cpu().numpy().reshape(n, T, M).transpose(1, 0, 2)
        assert np.array_equal(raw(got), raw(wo.cpu().numpy())), "out"
        assert_bits_equal(v.cpu().numpy(), wv.cpu().numpy(), "vad")
        assert_bits_equal(g.cpu().numpy(), wg.cpu().numpy(), "gains")
    assert int(b.state.item()) == 2 * T
    assert_bits_equal(a.batch.save_streams(), b.batch.save_streams(), "snapshots")
    # ... and the frame-major entry point of the same op still takes frame-major tensors afterwards
    if dtype == np.float32:
        more = torch.from_numpy(pcm[:1]).to(dev)
        assert torch.equal(a(more)[0].view(torch.int32), b(more)[0].view(torch.int32))
    a.close(), b.close()
