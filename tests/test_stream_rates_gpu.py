"""Mixed-rate batches on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates): a PCM rate per stream, 8 to 48 kHz in one
batch.  Every stream must give, bit for bit in out, vad, gains and exported state, what it gives in a uniform batch at its own rate
-- the chain resample.Up -> Oracle.process per frame -> resample.Down, or the plain oracle at 48 kHz -- whatever its neighbours run
at; the part of its `in` row behind its frame is not read and the part of its `out` row behind it is not written.  All comparisons
are on bits."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal
from ctl_oracle import CtlOracle
from oracle.binding import Oracle
from rnnoise_amd import capi, resample
from test_gpu_parity import fuzz_pcm
from test_resample_gpu import Chain, low_pcm, tiled

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)
SENTINEL16 = np.int16(-32768)
JUNK = 7777.0  # what the unread part of an `in` row holds
LS = np.array([1, 2, 3, 6])
CALLS = [1, 4, 1, 3]
DISTINCT = 37


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


def divisors(n):
    """the divisor of every stream: all four rates inside every 16-stream tile and 64-stream group, and in most quads"""
    s = np.arange(n)
    return LS[(s + s // 5) % 4]


class Signals:
    """per divisor, DISTINCT fuzz signals at that rate; stream s at divisor L carries signal s % DISTINCT of that rate"""

    def __init__(self, T, seed, Ls=(1, 2, 3, 6)):
        self.base = {int(L): (low_pcm(DISTINCT, T, int(L), seed + int(L)) if L > 1 else fuzz_pcm(DISTINCT, T, seed + 1)) for L in Ls}

    def rows(self, Ls, sl, Lb=1, s16=False):
        """(frames, n, 480 / Lb): every stream's frames at the front of its rows, junk behind them"""
        n, k = len(Ls), sl.stop - sl.start
        pcm = np.full((k, n, 480 // Lb), JUNK, np.float32)
        for L in np.unique(Ls):
            idx = np.nonzero(Ls == L)[0]
            pcm[:, idx, :480 // L] = self.base[int(L)][sl][:, idx % DISTINCT]
        return np.clip(np.round(pcm), -32768, 32767).astype(np.int16) if s16 else pcm

    def uniform(self, L, n, sl):
        return tiled(self.base[int(L)][sl], n)


class Plain:
    """a 48 kHz stream: the oracle alone, with the interface of test_resample_gpu.Chain"""
    L = 1

    def __init__(self, blob):
        self.o = Oracle(blob)

    def frame(self, x):
        ro, rv, rec = self.o.process(x)
        return np.asarray(ro, np.float32), np.float32(rv), np.frombuffer(rec.gains, np.float32)


def chain(blob, L, o=None):
    """the reference of one stream at divisor L; o: a DenoiseState to carry into it (its filters then start from zero)"""
    c = Chain(blob, int(L)) if L > 1 else Plain(blob)
    if o is not None:
        c.o = o
    return c


def check(chains, Ls, pcm, out, vad, gains, what, active=None, s16=False, rows=None):
    """chains: {stream: reference}, advanced over the call's frames; rows: {stream: row of the call's buffers} (default: its own)"""
    sent = SENTINEL16 if s16 else SENTINEL
    for t in range(pcm.shape[0]):
        for s, c in chains.items():
            i = s if rows is None else rows[s]
            M, tag = 480 // int(Ls[s]), f"{what} stream {s} (L={Ls[s]}) frame {t}"
            assert_bits_equal(out[t, i, M:], np.full(out.shape[2] - M, sent, out.dtype), tag + ": row behind the stream's frame")
            if active is not None and not active[t, i]:
                assert_bits_equal(out[t, i, :M], np.full(M, sent, out.dtype), tag + ": absent row")
                assert vad[t, i] == 0 and not gains[t, i].any(), tag
                continue
            y, v, g = c.frame(pcm[t, i, :M].astype(np.float32))
            assert_bits_equal(out[t, i, :M], resample.to_s16(y) if s16 else y, tag + " out")
            assert_bits_equal(vad[t, i], v, tag + " vad")
            assert_bits_equal(gains[t, i], g, tag + " gains")


def check_states(b, chains, what):
    for s, c in chains.items():
        assert_bits_equal(b.export_state(s), c.o.get_state(), f"{what}: state of stream {s}")


def run_masked(b, pcm, act=None, s16=False):
    """a host call with `out` pre-filled with the sentinel (the masked host form takes an `out`; active None = everything present)"""
    out = np.full(pcm.shape, SENTINEL16 if s16 else SENTINEL, pcm.dtype)
    return (b.process_masked_s16 if s16 else b.process_masked)(pcm, act, out=out) if act is not None else host_call(b, pcm, out, s16)


def host_call(b, pcm, out, s16=False):
    """rnnoise_batch_process[_s16] into a pre-filled `out`"""
    T, n = pcm.shape[:2]
    vad, gains = np.empty((T, n), np.float32), np.empty((T, n, 32), np.float32)
    b.process_into(out.ctypes.data, pcm.ctypes.data, vad.ctypes.data, gains.ctypes.data, T, s16=s16)
    return out, vad, gains


def picked(Ls, n, extra=()):
    """checked streams: 0, n - 1 and at least two of every rate"""
    rows = {0, n - 1, *extra}
    for L in np.unique(Ls):
        idx = np.nonzero(Ls == L)[0]
        rows.update((int(idx[0]), int(idx[len(idx) // 2]), int(idx[-1])))
    return sorted(rows)


# ---- 1. the mixed batch is the chains, at sizes that reach every dispatch form of the other kernels ----
@pytest.mark.parametrize("n", [37, 600, 2100, 4096, 10277])
def test_mixed_batch_follows_the_chains(model, blob_default, n):
    T = sum(CALLS)
    Ls, sig = divisors(n), Signals(T, seed=n)
    b = capi.Batch(model, n)
    b.set_stream_rates(48000 // Ls)
    assert_bits_equal(b.stream_rates(), (48000 // Ls).astype(np.int32), "stream_rates")
    assert b.pcm_rate == 48000 and b.frame == 480
    chains = {s: chain(blob_default, Ls[s]) for s in picked(Ls, n)}
    t0 = 0
    for k in CALLS:
        pcm = sig.rows(Ls, slice(t0, t0 + k))
        out, vad, gains = run_masked(b, pcm)
        check(chains, Ls, pcm, out, vad, gains, f"n={n} call at {t0}")
        t0 += k
    check_states(b, chains, f"n={n}")
    b.close()


# ---- 2. every stream of the mixed batch against its twin in the uniform batch of its rate ----
@pytest.mark.parametrize("n", [4096, 10277])
def test_every_stream_equals_its_twin_in_a_uniform_batch(model, n):
    T = 9
    Ls, sig = divisors(n), Signals(T, seed=3 * n)
    mixed = capi.Batch(model, n)
    mixed.set_stream_rates(48000 // Ls)
    uni = {}
    for L in LS:
        uni[int(L)] = capi.Batch(model, n)
        if L > 1:
            uni[int(L)].set_pcm_rate(48000 // int(L))
    for sl in (slice(0, 4), slice(4, 5), slice(5, 9)):
        pcm = sig.rows(Ls, sl)
        out, vad, gains = run_masked(mixed, pcm)
        for L in LS:
            idx, M = np.nonzero(Ls == L)[0], 480 // int(L)
            o, v, g = uni[int(L)].process(sig.uniform(L, n, sl))
            assert_bits_equal(out[:, idx, :M], o[:, idx], f"n={n} L={L} frames {sl}: out of every stream")
            assert_bits_equal(vad[:, idx], v[:, idx], f"n={n} L={L} frames {sl}: vad")
            assert_bits_equal(gains[:, idx], g[:, idx], f"n={n} L={L} frames {sl}: gains")
            assert (out[:, idx, M:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"n={n} L={L}: rows behind the frames"
    for b in (mixed, *uni.values()):
        b.close()


# ---- 3. a 16 kHz batch takes 16 and 8 kHz streams ----
def test_a_16k_batch_with_16_and_8k_streams_and_its_refusals(model, blob_default):
    n, T = 300, 6
    Ls = np.where((np.arange(n) + np.arange(n) // 5) % 2, 6, 3)
    sig = Signals(T, seed=16, Ls=(3, 6))
    b = capi.Batch(model, n)
    b.set_pcm_rate(16000)
    b.set_stream_rates(48000 // Ls)
    assert b.frame == 160
    chains = {s: chain(blob_default, Ls[s]) for s in picked(Ls, n)}
    pcm = sig.rows(Ls, slice(0, 3), Lb=3)
    assert pcm.shape == (3, n, 160)
    check(chains, Ls, pcm, *run_masked(b, pcm), "16k batch")
    # 48 and 24 kHz do not fit a 160-sample row: refused by the C call with nothing changed, and by capi before it gets there
    for bad in (1, 2, 0, 4, 5, 7, 255):
        t = Ls.astype(np.uint8)
        t[7] = bad
        assert capi.lib().rnnoise_batch_set_stream_rates(b.h, t.ctypes.data_as(C.POINTER(C.c_ubyte))) == -1, bad
    with pytest.raises(ValueError):
        b.set_stream_rates(np.where(np.arange(n) == 4, 48000, 16000))
    assert_bits_equal(b.stream_rates(), (48000 // Ls).astype(np.int32), "table after the refusals")
    pcm = sig.rows(Ls, slice(3, T), Lb=3)
    check(chains, Ls, pcm, *run_masked(b, pcm), "16k batch after the refusals")
    check_states(b, chains, "16k batch")
    # NULL buffers on a real batch
    assert capi.lib().rnnoise_batch_set_stream_rates_device(b.h, None, None) == -1
    assert capi.lib().rnnoise_batch_stream_rates(b.h, None) == -1
    b.close()


# ---- 4. the call forms ----
def device_buffers(torch, pcm, s16):
    dev = torch.device("cuda", 0)
    T, n = pcm.shape[:2]
    d_in = torch.from_numpy(pcm).to(dev)
    d_out = torch.full_like(d_in, int(SENTINEL16) if s16 else float(SENTINEL))
    return d_in, d_out, torch.empty((T, n), device=dev), torch.empty((T, n, 32), device=dev)


@pytest.mark.parametrize("n", [64, 4096])
def test_s16_host_and_device_forms(model, blob_default, n):
    torch = pytest.importorskip("torch")
    T = 5
    Ls, sig = divisors(n), Signals(T, seed=7)
    pcm = sig.rows(Ls, slice(0, T), s16=True)
    host, dev_b = capi.Batch(model, n), capi.Batch(model, n)
    for b in (host, dev_b):
        b.set_stream_rates(48000 // Ls)
    chains = {s: chain(blob_default, Ls[s]) for s in picked(Ls, n)}
    out, vad, gains = run_masked(host, pcm, s16=True)
    check(chains, Ls, pcm, out, vad, gains, f"s16 host n={n}", s16=True)
    d_in, d_out, d_vad, d_g = device_buffers(torch, pcm, True)
    torch.cuda.synchronize()
    dev_b.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), 2, 0, s16=True)
    f = n * 480
    dev_b.process_device(d_out.data_ptr() + 2 * f * 2, d_in.data_ptr() + 2 * f * 2, d_vad.data_ptr() + 2 * n * 4,
                         d_g.data_ptr() + 2 * n * 32 * 4, T - 2, 0, s16=True)
    torch.cuda.synchronize()
    assert_bits_equal(d_out.cpu().numpy(), out, "s16 device form = host form")
    assert_bits_equal(d_vad.cpu().numpy(), vad, "s16 device vad")
    assert_bits_equal(d_g.cpu().numpy(), gains, "s16 device gains")
    for b in (host, dev_b):
        b.close()


def test_float_device_form_matches_host_form(model):
    torch = pytest.importorskip("torch")
    n, T = 3000, 6
    Ls, sig = divisors(n), Signals(T, seed=11)
    pcm = sig.rows(Ls, slice(0, T))
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    for x in (a, b):
        x.set_stream_rates(48000 // Ls)
    want = run_masked(a, pcm)
    d_in, d_out, d_vad, d_g = device_buffers(torch, pcm, False)
    torch.cuda.synchronize()
    b.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), T, 0)
    torch.cuda.synchronize()
    for name, got, w in zip(("out", "vad", "gains"), (d_out, d_vad, d_g), want):
        assert_bits_equal(got.cpu().numpy(), w, f"float device form {name}")
    a.close()
    b.close()


def masks(n, T, seed):
    rng = np.random.default_rng(seed)
    act = (rng.random((T, n)) < 0.6).astype(np.uint8)
    act[:, 0] = 0
    act[:, 1] = np.arange(T) % 2
    act[:, 2] = 1
    return act


@pytest.mark.parametrize("n", [160, 4096])
def test_masked_host_calls_leave_history_and_state_alone(model, blob_default, n):
    T = 9
    Ls, sig, act = divisors(n), Signals(T, seed=5), masks(n, T, n)
    b = capi.Batch(model, n)
    b.set_stream_rates(48000 // Ls)
    chains = {s: chain(blob_default, Ls[s]) for s in picked(Ls, n, extra=(1, 2, 3))}
    for sl in (slice(0, 4), slice(4, 5), slice(5, T)):
        pcm = sig.rows(Ls, sl)
        check(chains, Ls, pcm, *run_masked(b, pcm, act[sl]), f"masked n={n}", active=act[sl])
    check_states(b, chains, f"masked n={n}")
    b.close()


def test_masked_device_s16(model, blob_default):
    torch = pytest.importorskip("torch")
    n, T = 3000, 7
    Ls, sig, act = divisors(n), Signals(T, seed=n), masks(n, T, n + 1)
    pcm = sig.rows(Ls, slice(0, T), s16=True)
    b = capi.Batch(model, n)
    b.set_stream_rates(48000 // Ls)
    chains = {s: chain(blob_default, Ls[s]) for s in picked(Ls, n, extra=(1, 2))}
    d_in, d_out, d_vad, d_g = device_buffers(torch, pcm, True)
    d_act = torch.from_numpy(act).to(d_in.device)
    torch.cuda.synchronize()
    b.process_masked_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), d_act.data_ptr(), T, 0, s16=True)
    torch.cuda.synchronize()
    check(chains, Ls, pcm, d_out.cpu().numpy(), d_vad.cpu().numpy(), d_g.cpu().numpy(), "masked device s16", active=act, s16=True)
    b.close()


@pytest.mark.parametrize("s16", [False, True])
def test_list_calls_in_scrambled_order_leave_unlisted_streams_alone(model, blob_default, s16):
    n, R, T = 600, 150, 9
    Ls, sig = divisors(n), Signals(T, seed=21)
    a, twin = capi.Batch(model, n), capi.Batch(model, n)
    for b in (a, twin):
        b.set_stream_rates(48000 // Ls)
    rng = np.random.default_rng(2)
    streams = rng.permutation(n)[:R].astype(np.int32)
    streams[:3] = [n - 1, 0, 17]
    streams[3:] = rng.permutation(np.setdiff1d(np.arange(n), streams[:3]))[:R - 3]
    row_of = {int(s): i for i, s in enumerate(streams)}
    listed = sorted({n - 1, 0, 17, *(int(s) for s in streams[3:15])})
    assert set(int(L) for L in Ls[listed]) == {1, 2, 3, 6}
    chains = {s: chain(blob_default, Ls[s]) for s in listed}
    pcm = sig.rows(Ls, slice(0, 3), s16=s16)
    got = run_masked(a, pcm, s16=s16)
    run_masked(twin, pcm, s16=s16)
    check(chains, Ls, pcm, *got, "before the list call", s16=s16)
    # the list call: rows in scrambled order, with a mask on top; the twin does not take these frames
    act = (rng.random((3, R)) < 0.7).astype(np.uint8)
    act[:, 0] = 1
    act[:, 1] = [1, 0, 1]
    rows = np.ascontiguousarray(sig.rows(Ls, slice(3, 6), s16=s16)[:, streams])
    out = np.full(rows.shape, SENTINEL16 if s16 else SENTINEL, rows.dtype)
    out, vad, gains = (a.process_list_s16 if s16 else a.process_list)(rows, streams, act, out=out)
    check(chains, Ls, rows, out, vad, gains, "list call", active=act, s16=s16, rows=row_of)
    # the next frames of every UNLISTED stream: as in the twin, which never saw the list call
    pcm = sig.rows(Ls, slice(6, T), s16=s16)
    got, want = run_masked(a, pcm, s16=s16), run_masked(twin, pcm, s16=s16)
    unlisted = np.setdiff1d(np.arange(n), streams)
    assert set(int(L) for L in Ls[unlisted]) == {1, 2, 3, 6}
    for name, g, w in zip(("out", "vad", "gains"), got, want):
        assert_bits_equal(g[:, unlisted], w[:, unlisted], f"unlisted streams after the list call: {name}")
    check(chains, Ls, pcm, *got, "listed streams after the list call", s16=s16)
    check_states(a, chains, "list call")
    a.close()
    twin.close()


# ---- 5. table changes ----
def test_table_changes_restart_only_the_changed_streams(model, blob_default):
    n, T = 300, 12
    Ls, sig = divisors(n), Signals(T, seed=33)
    b = capi.Batch(model, n)
    b.set_stream_rates(48000 // Ls)
    rows = picked(Ls, n, extra=(4, 5, 6, 7, 8))
    chains = {s: chain(blob_default, Ls[s]) for s in rows}
    pcm = sig.rows(Ls, slice(0, 3))
    check(chains, Ls, pcm, *run_masked(b, pcm), "first table")
    # a few streams change their divisor: their filters restart from zero with the DenoiseState carried; all others continue
    new = Ls.copy()
    for s, L in ((0, 6), (4, 2), (5, 1), (6, 3), (n - 1, int(LS[(np.nonzero(LS == Ls[n - 1])[0][0] + 1) % 4]))):
        assert new[s] != L
        new[s] = L
        chains[s] = chain(blob_default, L, o=chains[s].o)
    b.set_stream_rates(48000 // new)
    assert_bits_equal(b.stream_rates(), (48000 // new).astype(np.int32), "second table")
    pcm = sig.rows(new, slice(3, 6))
    check(chains, new, pcm, *run_masked(b, pcm), "second table")
    # no table: the streams already at the batch's rate continue, the others restart their filters there
    b.set_stream_rates(None)
    assert (b.stream_rates() == 48000).all()
    for s in rows:
        if new[s] != 1:
            chains[s] = chain(blob_default, 1, o=chains[s].o)
    ones = np.ones(n, np.int64)
    pcm = sig.rows(ones, slice(6, 9))
    check(chains, ones, pcm, *run_masked(b, pcm), "table dropped")
    check_states(b, chains, "table dropped")
    # rnnoise_batch_set_pcm_rate drops the table, at the same rate and at another one
    b.set_stream_rates(48000 // Ls)
    assert b.set_pcm_rate(48000) == 48000 and (b.stream_rates() == 48000).all()
    for s in rows:
        chains[s] = chain(blob_default, 1, o=chains[s].o)
    pcm = sig.rows(ones, slice(9, 10))
    check(chains, ones, pcm, *run_masked(b, pcm), "set_pcm_rate(48000) dropped the table")
    b.set_stream_rates(48000 // Ls)
    assert b.set_pcm_rate(16000) == 48000 and (b.stream_rates() == 16000).all() and b.frame == 160
    threes = np.full(n, 3)
    for s in rows:
        chains[s] = chain(blob_default, 3, o=chains[s].o)
    pcm = sig.rows(threes, slice(10, T), Lb=3)
    check(chains, threes, pcm, *run_masked(b, pcm), "set_pcm_rate(16000) dropped the table")
    check_states(b, chains, "end")
    b.close()


# ---- 6. the device setter ----
def test_device_setter_is_ordered_on_its_stream_and_reads_bad_entries_as_the_batch_rate(model, blob_default):
    torch = pytest.importorskip("torch")
    n, T = 600, 8
    Ls, sig = divisors(n), Signals(T, seed=44)
    bad = {12: 0, 40: 4, 64: 7, 100: 255, 101: 9}  # entries that name no rate: the batch's own (48 kHz)
    Ls[list(bad)] = 1
    new = Ls.copy()
    changed = np.array([3, 17, 18, 250, n - 1], np.int32)
    for s in changed:
        new[s] = int(LS[(np.nonzero(LS == Ls[s])[0][0] + 1 + s % 3) % 4])
    assert (new[changed] != Ls[changed]).all()
    dev = torch.device("cuda", 0)
    host, devb = capi.Batch(model, n), capi.Batch(model, n)
    host.set_stream_rates(48000 // Ls)
    t0 = Ls.astype(np.uint8)
    for s, v in bad.items():
        t0[s] = v
    d_t0, d_t1 = torch.from_numpy(t0).to(dev), torch.from_numpy(new.astype(np.uint8)).to(dev)
    d_changed = torch.from_numpy(changed).to(dev)
    pcm0, pcm1 = sig.rows(Ls, slice(0, 4)), sig.rows(new, slice(4, T))
    in0, out0, vad0, g0 = device_buffers(torch, pcm0, False)
    in1, out1, vad1, g1 = device_buffers(torch, pcm1, False)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    h = st.cuda_stream
    # the first table of the batch from device memory, frames, the second table, the reset of its changed streams, frames: one stream,
    # no host synchronisation in between
    devb.set_stream_rates_device(d_t0.data_ptr(), h)
    devb.process_device(out0.data_ptr(), in0.data_ptr(), vad0.data_ptr(), g0.data_ptr(), 4, h)
    devb.set_stream_rates_device(d_t1.data_ptr(), h)
    devb.reset_streams_device(d_changed.data_ptr(), len(changed), h)
    devb.process_device(out1.data_ptr(), in1.data_ptr(), vad1.data_ptr(), g1.data_ptr(), T - 4, h)
    st.synchronize()
    assert_bits_equal(devb.stream_rates(), (48000 // new).astype(np.int32), "device table read back")
    want0 = run_masked(host, pcm0)
    host.set_stream_rates(48000 // new)
    host.reset_streams(changed)
    want1 = run_masked(host, pcm1)
    for name, got, w in zip(("out", "vad", "gains") * 2, (out0, vad0, g0, out1, vad1, g1), want0 + want1):
        assert_bits_equal(got.cpu().numpy(), w, f"device-setter sequence = host-setter sequence: {name}")
    # ... and both are the chains: the bad entries ran at 48 kHz, the changed streams restarted from rnnoise_init's state
    rows = sorted({*bad, *(int(s) for s in changed), 0, 1, 2})
    chains = {s: chain(blob_default, Ls[s]) for s in rows}
    check(chains, Ls, pcm0, out0.cpu().numpy(), vad0.cpu().numpy(), g0.cpu().numpy(), "device setter, first table")
    for s in changed:
        chains[int(s)] = chain(blob_default, new[s])
    check(chains, new, pcm1, out1.cpu().numpy(), vad1.cpu().numpy(), g1.cpu().numpy(), "device setter, second table")
    host.close()
    devb.close()


# ---- 7. snapshots ----
def test_snapshots_carry_each_streams_own_divisor(model, blob_default):
    n, T = 200, 8
    Ls, sig = divisors(n), Signals(T, seed=55)
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    a.set_stream_rates(48000 // Ls)
    Lb = np.roll(Ls, 7)  # the destination's table: a permutation under which some streams keep their divisor and some do not
    same = Lb == Ls
    assert same.any() and (~same).any() and {int(L) for L in Ls[same]} == {1, 2, 3, 6}
    b.set_stream_rates(48000 // Lb)
    rows = sorted({*picked(Ls, n), *(int(s) for s in np.nonzero(same)[0][:6]), *(int(s) for s in np.nonzero(~same)[0][:6])})
    chains = {s: chain(blob_default, Ls[s]) for s in rows}
    pcm = sig.rows(Ls, slice(0, 4))
    check(chains, Ls, pcm, *run_masked(a, pcm), "source")
    snap = a.save_streams()
    assert_bits_equal(snap[:, capi.SNAP_OFF_L].view(np.int32), Ls.astype(np.int32), "RN_SNAP_OFF_L of every record")
    assert (snap[:, capi.SNAP_OFF_MAGIC].view(np.int32) == capi.SNAP_MAGIC).all()
    b.load_streams(snap)
    # same divisor: continues bit for bit, history included; another divisor: its DenoiseState with zero history
    for s in rows:
        if not same[s]:
            chains[s] = chain(blob_default, Lb[s], o=chains[s].o)
    pcm_b = sig.rows(Lb, slice(4, T))
    got = run_masked(b, pcm_b)
    check(chains, Lb, pcm_b, *got, "destination")
    check_states(b, chains, "destination")
    # ... every stream that kept its divisor, against the source going on
    cont = run_masked(a, sig.rows(Ls, slice(4, T)))
    idx = np.nonzero(same)[0]
    for name, g, w in zip(("out", "vad", "gains"), got, cont):
        assert_bits_equal(g[:, idx], w[:, idx], f"streams that kept their divisor continue as in the source: {name}")
    a.close()
    b.close()


# ---- 8. together with the other per-stream features ----
class CtlChain:
    """one stream on the ctl oracle (tests/ctl_oracle.py) with the resampler chain of its divisor"""

    def __init__(self, blob, ctl, L):
        self.o, self.ctl, self.L = CtlOracle(blob), ctl, int(L)
        if self.L > 1:
            self.up, self.dn = resample.Up(self.L), resample.Down(self.L)

    def frame(self, x):
        x = np.asarray(x, np.float32)
        o, v, g = self.o.process(self.up(x) if self.L > 1 else x, self.ctl)
        return (self.dn(o) if self.L > 1 else o), v, g


def test_with_model_slots_controls_and_masks(model, blob_default, blob_little):
    n, T = 600, 12
    Ls, sig, act = divisors(n), Signals(T, seed=66), masks(n, T, 8)
    little = capi.Model(blob_little)
    slots = (np.arange(n) % 3 == 1).astype(np.uint8)
    ctl = capi.controls_table(n, limit_db=np.where(np.arange(n) % 2, 12.0, np.inf), vad_threshold=np.where(np.arange(n) % 4 < 2, 0.6, 0.0),
                              hold_frames=2)
    b = capi.Batch(model, n)
    b.set_nn_path(1)
    b.add_model(little)
    b.set_stream_models(slots)
    b.set_stream_controls(ctl)
    b.set_stream_rates(48000 // Ls)
    combos = [int(np.nonzero((slots == k) & (Ls == L))[0][3]) for k in (0, 1) for L in (1, 2, 3, 6)]  # every (slot, rate) pair
    rows = picked(Ls, n, extra=(1, 2, 3, *combos))
    chains = {s: CtlChain(blob_little if slots[s] else blob_default, ctl[s], Ls[s]) for s in rows}
    for sl in (slice(0, 5), slice(5, 6), slice(6, T)):
        pcm = sig.rows(Ls, sl)
        check(chains, Ls, pcm, *run_masked(b, pcm, act[sl]), f"all features, frames {sl}", active=act[sl])
    for s in rows:
        assert_bits_equal(b.export_state(s), chains[s].o.state, f"all features: state of stream {s}")
    b.close()
    little.close()


# ---- 9. training features ----
def test_train_features_refused_while_a_table_is_set(model):
    n, T = 64, 2
    Ls = divisors(n)
    noisy = tiled(fuzz_pcm(16, T, 9), n)
    args = (noisy * np.float32(0.5), noisy, np.zeros((T, n), np.float32), np.full(n, 481), np.full(n, 32), np.zeros(n))
    b, plain = capi.Batch(model, n), capi.Batch(model, n)
    b.set_stream_rates(48000 // Ls)
    with pytest.raises(RuntimeError):
        b.train_features(*args)
    b.set_stream_rates(None)
    assert_bits_equal(b.train_features(*args), plain.train_features(*args), "train_features after the table is dropped")
    b.close()
    plain.close()
