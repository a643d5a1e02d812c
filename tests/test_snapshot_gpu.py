"""Stream snapshots on the GPU (include/rnnoise_amd.h: rnnoise_batch_save_streams / load_streams and their device forms).  Every
comparison is bit-exact: a snapshot's prefix is export_state (and the oracle's state); a stream that is saved from one batch and
loaded into another -- of another size, at another frame phase, lock-step or per-stream -- continues exactly like the same stream left
running where it was, and like the oracle, with float and int16 PCM, at 48, 16 and 8 kHz (the resampler history), behind a VAD gate
(the counter) and on two model slots; nobody else moves; a record of another rate loads like import_state; whole batches round-trip
at sizes that reach the tile and the layer-wise network kernels (the re-quantisation of the listed tiles); the device forms are
ordered on their stream between pipelined calls; entries and records that name nothing touch nothing.

Inputs are the mixed block of tests/stream_mix.py: neighbouring rows sit in different pitch regimes and silence states."""
import ctypes as C
import functools

import numpy as np
import pytest

import stream_mix
from conftest import assert_bits_equal, load_blob
from oracle.binding import Oracle
from rnnoise_amd import capi
from test_masked_gpu import s16_of
from test_stream_controls_gpu import Ref

pytestmark = pytest.mark.gpu

S, SNAP = capi.STATE_FLOATS, capi.SNAP_FLOATS
HIST = slice(capi.SNAP_OFF_HIST, capi.SNAP_FLOATS)


@pytest.fixture(scope="module")
def blob():
    return load_blob("default")


@pytest.fixture(scope="module")
def blob2():
    return load_blob("little")


@pytest.fixture(scope="module")
def model(blob):
    return capi.Model(blob)


@functools.lru_cache(None)
def block():
    return stream_mix.block()[0]  # (T, B, 480)


def inputs(pos, L=1, s16=False, frames=slice(None)):
    """the block's frames for the block positions `pos` as PCM at 48000 / L (every L-th sample), float or int16: (T, n, 480 / L)"""
    x = block()[frames][:, np.asarray(pos) % stream_mix.B]
    if L > 1:
        x = x[..., ::L]
    return np.ascontiguousarray(s16_of(x) if s16 else x)


def run(b, x, s16=False, active=None):
    if active is not None:
        return (b.process_masked_s16 if s16 else b.process_masked)(x, active)
    return (b.process_s16 if s16 else b.process)(x)


def header(snap):
    return np.ascontiguousarray(snap[..., capi.SNAP_OFF_MAGIC:capi.SNAP_OFF_HIST]).view(np.int32)


def presence(pos, frames):
    """the block's presence schedule for these positions, with every stream present at least once"""
    a = stream_mix.presence()[frames][:, np.asarray(pos) % stream_mix.B].copy()
    a[0, a.sum(0) == 0] = 1
    return np.ascontiguousarray(a)


# ---- 1. the prefix of a snapshot is export_state ----
@pytest.mark.parametrize("mode", ["lock", "per_stream"])
def test_prefix_is_export_state_and_the_oracles_state(model, blob, mode):
    n, k = 45, 9
    pos = np.arange(n) * 3
    x = inputs(pos, frames=slice(0, k))
    b = capi.Batch(model, n)
    act = None
    if mode == "per_stream":
        act = presence(pos, slice(0, k))
        assert len(set((act.sum(0) % 6).tolist())) >= 4, "the streams must sit at unequal frame phases"
    run(b, x, active=act)
    snap = b.save_streams()
    assert snap.shape == (n, SNAP) and snap.dtype == np.float32
    for s in range(n):
        assert_bits_equal(snap[s, :S], b.export_state(s), f"{mode}: prefix of stream {s}")
    for s in range(6):
        o = Oracle(blob)
        for t in range(k):
            if act is None or act[t, s]:
                o.process(x[t, s])
        assert_bits_equal(snap[s, :S], o.get_state(), f"{mode}: prefix of stream {s} against the oracle")
    h = header(snap)
    assert (h[:, 0] == capi.SNAP_MAGIC).all() and (h[:, 1] == 1).all() and (h[:, 2] == capi.SNAP_GATE_NONE).all() and not h[:, 3:].any()
    assert not snap[:, HIST].view(np.uint32).any(), "48 kHz: the history reads zero"
    # a list, in any order and with repeats, gives the same records by row
    idx = np.concatenate([np.random.default_rng(1).permutation(n)[:20], [7, 7]])
    assert_bits_equal(b.save_streams(idx), snap[idx], f"{mode}: listed rows")
    assert_bits_equal(b.save_streams(), snap, f"{mode}: a save changes nothing")


# ---- 2. and 3. a moved leg continues as if it had not moved; nobody else moves ----
N_A, N_B, T1, T2, N_MOVED = 67, 45, 11, 9, 20
POS_A = np.arange(N_A) * 7
POS_B = 150 + np.arange(N_B) * 5
GRID = [(thr, hold) for thr in (0.5, 0.6, 0.3, 0.9) for hold in (4, 2, 1, 7)]


def gate_counters(vad, thr):
    """the ctl oracle's counter rule over a (T, n) VAD trace (rn_dev.h: RnGroupDev::ctl)"""
    c = np.full(vad.shape[1], 65536)
    for t in range(vad.shape[0]):
        c = np.where(vad[t] >= np.float32(thr), 0, np.minimum(c + 1, 65536))
    return c


MOVE_CASES = [("f32-48k", 48000, False, None), ("s16-48k", 48000, True, None), ("f32-16k", 16000, False, None),
              ("s16-16k", 16000, True, None), ("f32-8k", 8000, False, None), ("s16-8k", 8000, True, None),
              ("gate-48k", 48000, False, "ctl"), ("gate-16k", 16000, False, "ctl"), ("slots-48k", 48000, False, "slots")]


@pytest.mark.parametrize("b_mode", ["lock", "per_stream"])
@pytest.mark.parametrize("name,rate,s16,extra", MOVE_CASES, ids=[c[0] for c in MOVE_CASES])
def test_a_moved_leg_continues_as_if_it_had_not_moved(blob, blob2, name, rate, s16, extra, b_mode):
    L = 48000 // rate
    rng = np.random.default_rng([rate, int(s16), len(name)])
    xa = inputs(POS_A, L, s16, slice(0, T1 + T2))
    blobs = [blob, blob2]
    slot_a = np.arange(N_A) % 2 if extra == "slots" else np.zeros(N_A, int)
    ctl_a = None
    moved = rng.permutation(N_A)[:N_MOVED]
    if extra == "ctl":
        # thr / hold from the oracle's VAD (the controls change neither VAD nor gains): at the frame of the move some moved stream
        # must be inside its hold (0 < c <= hold) and some behind it (c > hold) -- asserted on the oracle's own counters below
        vad = np.empty((T1, N_A), np.float32)
        for s in range(N_A):
            r = Ref(blob, None, L)
            vad[:, s] = [r.frame(xa[t, s])[1] for t in range(T1)]
        for thr, hold in GRID:
            c = gate_counters(vad, thr)
            inside, behind = np.flatnonzero((c > 0) & (c <= hold)), np.flatnonzero(c > hold)
            if len(inside) >= 2 and len(behind) >= 2:
                break
        else:
            raise AssertionError("no thr / hold of the grid puts streams on both sides of the hold")
        rest = [s for s in rng.permutation(N_A) if s not in set(inside[:2]) | set(behind[:2])]
        moved = np.concatenate([inside[:2], behind[:2], rest[:N_MOVED - 4]])[rng.permutation(N_MOVED)]
        ctl_a = np.zeros((N_A, 3), np.float32)
        ctl_a[:, 0] = np.where(np.arange(N_A) % 3 == 0, 0.1, 0.0)
        ctl_a[:, 1], ctl_a[:, 2] = thr, hold
        watch = list(inside[:2]) + list(behind[:2])
    else:
        watch = list(moved[:4])
    dest = rng.permutation(N_B)[:N_MOVED]
    assert (dest != moved).any()
    refs = {s: Ref(blobs[slot_a[s]], None if ctl_a is None else ctl_a[s], L) for s in watch}
    want = {s: [r.frame(xa[t, s]) for t in range(T1 + T2)] for s, r in refs.items()}
    if extra == "ctl":
        # (the oracle's counters at the move, before anything runs on the GPU)
        cs = {}
        for s in watch:
            r = Ref(blob, ctl_a[s], L)
            for t in range(T1):
                r.frame(xa[t, s])
            cs[s] = r.o.c
        assert sum(0 < c <= hold for c in cs.values()) >= 1 and sum(c > hold for c in cs.values()) >= 1, cs

    def make(n, slots, ctl):
        b = capi.Batch(capi.Model(blob), n)
        if rate != 48000:
            b.set_pcm_rate(rate)
        if extra == "slots":
            assert b.add_model(capi.Model(blob2)) == 1
            b.set_stream_models(slots)
        if ctl is not None:
            b.set_stream_controls(ctl)
        return b

    # A runs the first part; B, of another size, has run another number of frames on other signals
    a = make(N_A, slot_a, ctl_a)
    slot_b = (np.arange(N_B) + 1) % 2 if extra == "slots" else np.zeros(N_B, int)
    ctl_b = None
    if ctl_a is not None:
        ctl_b = np.zeros((N_B, 3), np.float32)
        ctl_b[:, 1], ctl_b[:, 2] = 0.4, 3
    b = make(N_B, slot_b, ctl_b)
    run(a, xa[:T1], s16)
    kb = 4 if b_mode == "lock" else 7
    act_b = presence(POS_B, slice(0, kb)) if b_mode == "per_stream" else None
    if act_b is not None:
        assert len(set((act_b[:, dest].sum(0) % 6).tolist())) >= 3, "the destinations must sit at unequal frame phases"
    run(b, inputs(POS_B, L, s16, slice(0, kb)), s16, act_b)

    # the move: save on A, set slot and controls on B, load
    a_before = a.save_streams()
    snap = a.save_streams(moved)
    assert_bits_equal(a.save_streams(), a_before, f"{name}: the source is unchanged by a save")
    assert_bits_equal(snap, a_before[moved], f"{name}: listed rows")
    h = header(snap)
    assert (h[:, 0] == capi.SNAP_MAGIC).all() and (h[:, 1] == L).all()
    if L > 1:
        assert snap[:, HIST].any(axis=1).sum() >= N_MOVED // 2, "the saved histories must not be zero: the case would prove nothing"
    if extra == "ctl":
        for i, s in enumerate(moved):
            if s in cs:
                assert h[i, 2] == cs[s], (s, h[i, 2], cs[s])
    else:
        assert (h[:, 2] == capi.SNAP_GATE_NONE).all()
    if extra == "slots":
        slot_b[dest] = slot_a[moved]
        b.set_stream_models(slot_b)
    if ctl_b is not None:
        ctl_b[dest] = ctl_a[moved]
        b.set_stream_controls(ctl_b)
        # (a new table over an old one keeps the counters)
    b_before = b.save_streams()
    b.load_streams(snap, dest)
    b_after = b.save_streams()
    others = np.setdiff1d(np.arange(N_B), dest)
    assert_bits_equal(b_after[others], b_before[others], f"{name}: streams of the destination that were not listed")
    assert_bits_equal(b_after[dest][:, S:], snap[:, S:], f"{name}: header and history of the loaded streams")
    assert_bits_equal(b_after[dest][:, :S], snap[:, :S], f"{name}: portable state of the loaded streams")

    # both batches continue: the moved streams get the same frames in both
    xb = inputs(POS_B, L, s16, slice(kb, kb + T2))
    xb[:, dest] = xa[T1:, moved]
    got_a = run(a, xa[T1:], s16)
    got_b = run(b, xb, s16)
    for k, what in enumerate(("out", "vad", "gains")):
        assert_bits_equal(got_b[k][:, dest], got_a[k][:, moved], f"{name}, B {b_mode}: {what} of the moved streams after the move")
    for i, s in enumerate(moved):
        assert_bits_equal(b.export_state(int(dest[i])), a.export_state(int(s)), f"{name}: final state of stream {s} -> {dest[i]}")
    end_a, end_b = a.save_streams(moved), b.save_streams(dest)
    assert_bits_equal(end_b, end_a, f"{name}: final snapshots of the moved streams")
    # ... and the oracle
    for s, r in refs.items():
        i = int(np.flatnonzero(moved == s)[0])
        for t in range(T2):
            o, v, g = want[s][T1 + t]
            if s16:
                from rnnoise_amd import resample
                o = resample.to_s16(o) if L > 1 else s16_of(o)
            tag = f"{name}, B {b_mode}: stream {s} -> {dest[i]} frame {T1 + t} against the oracle:"
            assert_bits_equal(got_b[0][t, dest[i]], o, tag + " out")
            assert_bits_equal(got_b[1][t, dest[i]], v, tag + " vad")
            assert_bits_equal(got_b[2][t, dest[i]], g, tag + " gains")
        assert_bits_equal(end_b[i, :S], r.o.state, f"{name}: final state of stream {s} against the oracle")
        if extra == "ctl":
            assert header(end_b)[i, 2] == r.o.c, (s, header(end_b)[i, 2], r.o.c)


# ---- 4. a record of another rate loads like import_state of its prefix ----
@pytest.mark.parametrize("dst_rate", [48000, 8000])
def test_rate_mismatch_is_import_state(model, dst_rate):
    a = capi.Batch(model, 12)
    a.set_pcm_rate(16000)
    run(a, inputs(np.arange(12) * 11, 3, frames=slice(0, 6)))
    snap = a.save_streams([3, 5])
    assert snap[:, HIST].any() and (header(snap)[:, 1] == 3).all()
    Ld = 48000 // dst_rate
    pos = 40 + np.arange(9) * 13
    pair = []
    for how in ("load", "import"):
        b = capi.Batch(model, 9)
        if dst_rate != 48000:
            b.set_pcm_rate(dst_rate)
        run(b, inputs(pos, Ld, frames=slice(0, 4)))
        if how == "load":
            b.load_streams(snap, [1, 2])
        else:
            b.import_state(1, snap[0, :S])
            b.import_state(2, snap[1, :S])
        pair.append((b.save_streams(), run(b, inputs(pos, Ld, frames=slice(4, 9)))))
    assert_bits_equal(pair[0][0], pair[1][0], "snapshots after load_streams / import_state")
    assert not pair[0][0][1:3, HIST].view(np.uint32).any(), "a record of another rate zeroes the history"
    for k, what in enumerate(("out", "vad", "gains")):
        assert_bits_equal(pair[0][1][k], pair[1][1][k], what)


# ---- 5. whole batches at size: save all, reset, load all; and a partial list through the tiles of the layer-wise network ----
def device_snap(b, n_rows, idx=None, load=None):
    """the device forms through torch buffers, on torch's current stream: save -> the snapshots (a CUDA tensor); load=<tensor>"""
    import torch
    d_idx = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    if load is None:
        snap = torch.empty((n_rows, SNAP), device="cuda", dtype=torch.float32)
        b.save_streams_device(snap.data_ptr(), 0 if d_idx is None else d_idx.data_ptr(), n_rows, st)
        torch.cuda.synchronize()
        return snap
    b.load_streams_device(load.data_ptr(), 0 if d_idx is None else d_idx.data_ptr(), n_rows, st)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,host_form", [(4096, True), (10277, False), (65536, False)])
def test_whole_batch_round_trip_and_partial_list_at_size(model, n, host_form):
    pytest.importorskip("torch")
    Ta, Tb = (5, 2) if n < 65536 else (3, 1)
    x = inputs(np.arange(n), frames=slice(0, Ta + 2 * Tb + 1))
    b, twin = capi.Batch(model, n), capi.Batch(model, n)
    run(b, x[:Ta])
    run(twin, x[:Ta])
    snap = b.save_streams() if host_form else device_snap(b, n)
    b.reset()
    if host_form:
        b.load_streams(snap)
    else:
        device_snap(b, n, load=snap)
    t = Ta
    got, want = run(b, x[t:t + Tb]), run(twin, x[t:t + Tb])
    for k, what in enumerate(("out", "vad", "gains")):
        assert_bits_equal(got[k], want[k], f"{n} streams: {what} after save all / reset / load all")
    t += Tb
    del snap
    # a partial list that cuts through 16-stream tiles: those streams are saved, everybody takes one more frame, the saved ones are
    # loaded back (while the layer-wise network's state images are live from 10,240 streams up) and take that frame again
    idx = np.flatnonzero((np.arange(n) % 37 < 9) | (np.arange(n) % 1000 == 999)).astype(np.int32)
    idx = np.random.default_rng(n).permutation(idx)
    part = b.save_streams(idx) if host_form else device_snap(b, len(idx), idx)
    got1, want1 = run(b, x[t:t + 1]), run(twin, x[t:t + 1])
    for k, what in enumerate(("out", "vad", "gains")):
        assert_bits_equal(got1[k], want1[k], f"{n} streams: {what} of the frame after the partial save")
    if host_form:
        b.load_streams(part, idx)
    else:
        device_snap(b, len(idx), idx, load=part)
    x2 = x[t + 1:t + 2].copy()
    x2[:, idx] = x[t:t + 1, idx]
    got2, want2 = run(b, x2), run(twin, x[t + 1:t + 2])
    rest = np.setdiff1d(np.arange(n), idx)
    for k, what in enumerate(("out", "vad", "gains")):
        assert_bits_equal(got2[k][:, idx], want1[k][:, idx], f"{n} streams: {what} of the rolled-back streams")
        assert_bits_equal(got2[k][:, rest], want2[k][:, rest], f"{n} streams: {what} of the streams beside them")


# ---- 6. ordering on one stream between pipelined calls ----
def test_device_forms_are_ordered_on_their_stream(model):
    torch = pytest.importorskip("torch")
    n, calls = 600, (5, 3, 3)
    x = inputs(np.arange(n), frames=slice(0, sum(calls)))
    src = np.arange(0, 200, dtype=np.int32)[::-1].copy()
    dst = (300 + np.arange(200, dtype=np.int32) * 3 // 2).astype(np.int32)  # other streams of the same batch
    assert len(set(dst.tolist())) == 200 and not set(dst.tolist()) & set(src.tolist())
    res = []
    for sync in (False, True):
        b = capi.Batch(model, n)
        st = torch.cuda.Stream()
        h = st.cuda_stream
        with torch.cuda.stream(st):
            d_in = torch.from_numpy(x).cuda()
            d_out, d_vad = torch.zeros_like(d_in), torch.zeros((sum(calls), n), device="cuda")
            d_gains = torch.zeros((sum(calls), n, capi.NB_BANDS), device="cuda")
            d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
            d_snap = torch.zeros((200, SNAP), device="cuda")
        torch.cuda.synchronize()

        def proc(t, c):
            b.process_device(d_out[t].data_ptr(), d_in[t].data_ptr(), d_vad[t].data_ptr(), d_gains[t].data_ptr(), c, h)
            if sync:
                torch.cuda.synchronize()

        proc(0, calls[0])
        b.save_streams_device(d_snap.data_ptr(), d_src.data_ptr(), 200, h)
        if sync:
            torch.cuda.synchronize()
        proc(calls[0], calls[1])
        b.load_streams_device(d_snap.data_ptr(), d_dst.data_ptr(), 200, h)
        if sync:
            torch.cuda.synchronize()
        proc(calls[0] + calls[1], calls[2])
        torch.cuda.synchronize()
        res.append((d_out.cpu().numpy(), d_vad.cpu().numpy(), d_gains.cpu().numpy(), d_snap.cpu().numpy(), b.save_streams()))
    for k, what in enumerate(("out", "vad", "gains", "the saved records", "the final snapshot")):
        assert_bits_equal(res[0][k], res[1][k], f"queued without a synchronise against synchronised after every call: {what}")
    # (and the load did something: the destinations continue from the sources' state of the first call)
    assert (header(res[0][3])[:, 0] == capi.SNAP_MAGIC).all()


def test_torch_op_forms(blob):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n = 40
    op = RNNoiseOp(blob, n)
    x = torch.from_numpy(inputs(np.arange(n), frames=slice(0, 4))).cuda()
    op(x)
    whole = op.save_streams()
    assert tuple(whole.shape) == (n, SNAP) and whole.is_cuda
    torch.cuda.synchronize()
    assert_bits_equal(whole.cpu().numpy(), op.batch.save_streams(), "torch save against the host form")
    part = op.save_streams([5, 9])
    op.load_streams(part, torch.tensor([20, 21]))
    torch.cuda.synchronize()
    after = op.batch.save_streams()
    assert_bits_equal(after[[20, 21]], whole.cpu().numpy()[[5, 9]], "torch load")
    op.close()


# ---- 7. entries and records that name nothing ----
def test_bad_entries_device_forms(model):
    torch = pytest.importorskip("torch")
    n = 24
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    run(a, inputs(np.arange(n), frames=slice(0, 5)))
    run(b, inputs(100 + np.arange(n), frames=slice(0, 3)))
    good = a.save_streams([3, 5, 7])
    lst = np.array([-1, 3, n, 5, 2 ** 31 - 1, 7], np.int32)
    d_lst = torch.from_numpy(lst).cuda()
    d_snap = torch.full((len(lst), SNAP), 7.0, device="cuda")
    a.save_streams_device(d_snap.data_ptr(), d_lst.data_ptr(), len(lst), 0)
    torch.cuda.synchronize()
    snap = d_snap.cpu().numpy()
    assert (header(snap)[[0, 2, 4], 0] == 0).all(), "an entry out of range leaves an empty record"
    assert_bits_equal(snap[[1, 3, 5]], good, "the rows beside them")
    # load: out-of-range entries and a record with a zeroed magic word are skipped
    before = b.save_streams()
    snap[5, capi.SNAP_OFF_MAGIC] = 0
    snap[[0, 2, 4]] = snap[1]  # (valid records on the rows whose entries name nothing)
    d_snap.copy_(torch.from_numpy(snap))
    dst = np.array([-5, 10, n + 1, 12, -2 ** 31, 14], np.int32)
    d_dst = torch.from_numpy(dst).cuda()
    b.load_streams_device(d_snap.data_ptr(), d_dst.data_ptr(), len(dst), 0)
    torch.cuda.synchronize()
    after = b.save_streams()
    same = np.setdiff1d(np.arange(n), [10, 12])
    assert_bits_equal(after[same], before[same], "streams beside the two loaded ones (14: its record has no magic word)")
    assert_bits_equal(after[[10, 12]], good[:2], "the two loaded streams")
    L = capi.lib()
    # refusals of the device forms: nothing is launched
    assert L.rnnoise_batch_save_streams_device(a.h, d_snap.data_ptr() + 4, d_lst.data_ptr(), 2, None) == -1  # not 16-byte aligned
    assert L.rnnoise_batch_save_streams_device(a.h, None, d_lst.data_ptr(), 2, None) == -1
    assert L.rnnoise_batch_save_streams_device(a.h, d_snap.data_ptr(), None, 2, None) == -1  # no list, and not the whole batch
    assert L.rnnoise_batch_load_streams_device(a.h, d_snap.data_ptr(), d_lst.data_ptr(), -1, None) == -1
    assert L.rnnoise_batch_load_streams_device(a.h, d_snap.data_ptr(), d_lst.data_ptr(), n + 1, None) == -1
    assert L.rnnoise_batch_save_streams_device(a.h, None, None, 0, None) == 0
    assert L.rnnoise_batch_load_streams_device(a.h, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert_bits_equal(b.save_streams(), after, "refused calls change nothing")


def test_bad_entries_host_forms(model):
    n = 24
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    run(a, inputs(np.arange(n), frames=slice(0, 5)))
    run(b, inputs(100 + np.arange(n), frames=slice(0, 3)))
    good = a.save_streams([3, 5, 7])
    before = b.save_streams()
    L = capi.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)

    def load(snap, lst, count=None):
        snap = np.ascontiguousarray(snap, np.float32)
        lst = np.ascontiguousarray(lst, np.int32)
        return L.rnnoise_batch_load_streams(b.h, snap.ctypes.data_as(fp), lst.ctypes.data_as(ip), len(lst) if count is None else count)

    def save(lst, count=None):
        out = np.zeros((max(len(lst), 1), SNAP), np.float32)
        lst = np.ascontiguousarray(lst, np.int32)
        return L.rnnoise_batch_save_streams(b.h, out.ctypes.data_as(fp), lst.ctypes.data_as(ip), len(lst) if count is None else count)

    assert load(good, [1, n, 2]) == -1 and load(good, [1, -1, 2]) == -1, "an entry out of range"
    assert load(good, [1, 2, 1]) == -1, "a duplicate entry"
    bad = good.copy()
    bad[1, capi.SNAP_OFF_MAGIC] = 0
    assert load(bad, [1, 2, 3]) == -1, "a record without the magic word"
    bad = good.copy()
    bad[2, 17] += 1.0
    assert load(bad, [1, 2, 3]) == -1, "analysis_mem differs from the tail of pitch_buf"
    assert load(good, [1, 2, 3], count=-1) == -1 and load(good, [1, 2, 3], count=0) == 0
    assert L.rnnoise_batch_load_streams(b.h, None, None, 1) == -1
    assert L.rnnoise_batch_load_streams(b.h, good.ctypes.data_as(fp), None, 3) == -1, "no list, and not the whole batch"
    assert save([0, n]) == -1 and save([-1]) == -1 and save([0], count=-1) == -1 and save([0], count=0) == 0
    assert save([4, 4]) == 0, "duplicates in a save are harmless"
    assert L.rnnoise_batch_save_streams(b.h, None, None, n) == -1
    with pytest.raises(ValueError):
        b.load_streams(good, [1, 2, 2])
    with pytest.raises(ValueError):
        b.save_streams([n])
    assert_bits_equal(b.save_streams(), before, "refused calls change nothing")
    assert load(good, [1, 2, 3]) == 0
    after = b.save_streams()
    assert_bits_equal(after[[1, 2, 3]], good, "the accepted load")
    assert_bits_equal(after[[0] + list(range(4, n))], before[[0] + list(range(4, n))], "and nobody else")
