"""Low-rate PCM on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate).  Every checked stream must equal, bit for bit,
the chain resample.Up -> Oracle.process per frame -> resample.Down, in out, vad, gains and the exported state."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from oracle.binding import Oracle
from rnnoise_amd import capi, resample
from test_gpu_parity import fuzz_pcm

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)
RATE_L = {24000: 2, 16000: 3, 8000: 6}


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


def low_pcm(distinct, T, L, seed):
    """the fuzz and edge signals of test_gpu_parity resampled to 48000 / L: (T, distinct, 480 / L) float32"""
    hi = fuzz_pcm(distinct, T, seed)
    dn = resample.Down(L, (distinct,))
    return np.stack([dn(hi[t]) for t in range(T)]).astype(np.float32)


def tiled(base, n):
    d = base.shape[1]
    return np.ascontiguousarray(np.tile(base, (1, (n + d - 1) // d, 1))[:, :n])


class Chain:
    """the reference chain of one stream: up -> rnnoise_process_frame -> down"""

    def __init__(self, blob, L):
        self.blob, self.L = blob, L
        self.reset()

    def reset(self, keep_state=False):
        if not keep_state:
            self.o = Oracle(self.blob)
        self.up, self.dn = resample.Up(self.L), resample.Down(self.L)

    def frame(self, x):
        ro, rv, rec = self.o.process(self.up(x))
        return self.dn(np.asarray(ro, np.float32)), np.float32(rv), np.frombuffer(rec.gains, np.float32)


def check_rows(chains, pcm, out, vad, gains, rows, what, active=None, s16=False):
    """rows: {stream: chain key}; chains advance over the call's frames"""
    for t in range(pcm.shape[0]):
        for s, c in rows.items():
            if active is not None and not active[t, s]:
                assert (out[t, s].view(np.uint32 if not s16 else np.uint16) == (SENTINEL.view(np.uint32) if not s16 else np.uint16(0x8000))).all(), f"{what} stream {s} frame {t}: absent row written"
                assert vad[t, s] == 0 and not gains[t, s].any()
                continue
            x = pcm[t, s].astype(np.float32)
            y, v, g = chains[c].frame(x)
            if s16:
                y = resample.to_s16(y)
            tag = f"{what} stream {s} frame {t}"
            assert_bits_equal(out[t, s], y, tag + " out")
            assert_bits_equal(vad[t, s], v, tag + " vad")
            assert_bits_equal(gains[t, s], g, tag + " gains")


CALLS = [1, 4, 1, 3]


# every rate at sizes that reach every dispatch form of the other kernels
SIZES = [(r, n) for n in (37, 600, 2100, 4096, 10277) for r in (24000, 16000, 8000)]


@pytest.mark.parametrize("rate,n", SIZES)
def test_sizes_and_call_shapes_follow_the_chain(model, blob_default, rate, n):
    L = RATE_L[rate]
    T = sum(CALLS)
    distinct = 37
    base = low_pcm(distinct, T, L, seed=n + L)
    pcm = tiled(base, n)
    b = capi.Batch(model, n)
    assert b.set_pcm_rate(rate) == 48000 and b.pcm_rate == rate
    rows = sorted({0, 1, distinct - 1, n // 2, n - 1})
    chains = {s: Chain(blob_default, L) for s in rows}
    t0 = 0
    for k in CALLS:
        sl = slice(t0, t0 + k)
        out, vad, gains = b.process(pcm[sl])
        assert out.shape == (k, n, 480 // L)
        check_rows(chains, pcm[sl], out, vad, gains, {s: s for s in rows}, f"R={rate} n={n} call at {t0}")
        t0 += k
    for s in rows:
        assert_bits_equal(b.export_state(s), chains[s].o.get_state(), f"R={rate} n={n} state of stream {s}")


@pytest.mark.parametrize("rate", [24000, 16000, 8000])
@pytest.mark.parametrize("n", [64, 4096])
def test_s16_host_and_device_forms(model, blob_default, n, rate):
    torch = pytest.importorskip("torch")
    L, T = RATE_L[rate], 5
    base = low_pcm(16, T, L, seed=7)
    pcm16 = np.clip(np.round(tiled(base, n)), -32768, 32767).astype(np.int16)
    rows = [0, 5, n - 1]
    host, dev_b = capi.Batch(model, n), capi.Batch(model, n)
    host.set_pcm_rate(rate)
    dev_b.set_pcm_rate(rate)
    chains = {s: Chain(blob_default, L) for s in rows}
    out, vad, gains = host.process_s16(pcm16)
    check_rows(chains, pcm16, out, vad, gains, {s: s for s in rows}, f"s16 host n={n}", s16=True)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(pcm16).to(dev)
    d_out = torch.empty_like(d_in)
    d_vad = torch.empty((T, n), device=dev)
    d_g = torch.empty((T, n, 32), device=dev)
    torch.cuda.synchronize()
    dev_b.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), 2, 0, s16=True)
    f = (n * (480 // L))
    dev_b.process_device(d_out.data_ptr() + 2 * f * 2, d_in.data_ptr() + 2 * f * 2, d_vad.data_ptr() + 2 * n * 4,
                         d_g.data_ptr() + 2 * n * 32 * 4, T - 2, 0, s16=True)
    torch.cuda.synchronize()
    assert_bits_equal(d_out.cpu().numpy(), out, "s16 device form = host form")
    assert_bits_equal(d_vad.cpu().numpy(), vad, "s16 device vad")
    assert_bits_equal(d_g.cpu().numpy(), gains, "s16 device gains")


@pytest.mark.parametrize("rate", [24000, 16000, 8000])
def test_float_device_form_matches_host_form(model, rate):
    torch = pytest.importorskip("torch")
    n, L, T = 3000, RATE_L[rate], 6
    pcm = tiled(low_pcm(16, T, L, seed=11), n)
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    a.set_pcm_rate(rate)
    b.set_pcm_rate(rate)
    want = a.process(pcm)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(pcm).to(dev)
    d_out, d_vad, d_g = torch.empty_like(d_in), torch.empty((T, n), device=dev), torch.empty((T, n, 32), device=dev)
    torch.cuda.synchronize()
    b.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), T, 0)
    torch.cuda.synchronize()
    for name, got, w in zip(("out", "vad", "gains"), (d_out, d_vad, d_g), want):
        assert_bits_equal(got.cpu().numpy(), w, f"float device form {name}")


@pytest.mark.parametrize("n", [160, 4096])
def test_masks_leave_history_and_state_alone(model, blob_default, n):
    L, T = 6, 9
    pcm = tiled(low_pcm(40, T, L, seed=5), n)
    rng = np.random.default_rng(n)
    act = (rng.random((T, n)) < 0.6).astype(np.uint8)
    act[:, 0] = 0
    act[:, 1] = np.arange(T) % 2
    act[:, 2] = 1
    rows = [0, 1, 2, 3, n - 1]
    b = capi.Batch(model, n)
    b.set_pcm_rate(8000)
    chains = {s: Chain(blob_default, L) for s in rows}
    for sl in (slice(0, 4), slice(4, 5), slice(5, T)):
        out = np.full(pcm[sl].shape, SENTINEL, np.float32)
        out, vad, gains = b.process_masked(pcm[sl], act[sl], out=out)
        check_rows(chains, pcm[sl], out, vad, gains, {s: s for s in rows}, f"masked n={n}", active=act[sl])
    for s in rows:
        assert_bits_equal(b.export_state(s), chains[s].o.get_state(), f"masked n={n} state of stream {s}")


@pytest.mark.parametrize("n", [100, 3000])
def test_masked_device_s16(model, blob_default, n):
    """rnnoise_batch_process_device_masked_s16 at 16 kHz: absent rows untouched, present rows the chain, history kept over gaps"""
    torch = pytest.importorskip("torch")
    L, T = 3, 7
    pcm = np.clip(np.round(tiled(low_pcm(20, T, L, seed=n), n)), -32768, 32767).astype(np.int16)
    rng = np.random.default_rng(n + 1)
    act = (rng.random((T, n)) < 0.6).astype(np.uint8)
    act[:, 0] = np.arange(T) % 2
    act[:, 1] = 1
    rows = [0, 1, 2, n - 1]
    b = capi.Batch(model, n)
    b.set_pcm_rate(16000)
    chains = {s: Chain(blob_default, L) for s in rows}
    dev = torch.device("cuda", 0)
    d_in, d_act = torch.from_numpy(pcm).to(dev), torch.from_numpy(act).to(dev)
    d_out = torch.full_like(d_in, -32768)
    d_vad, d_g = torch.empty((T, n), device=dev), torch.empty((T, n, 32), device=dev)
    torch.cuda.synchronize()
    b.process_masked_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), d_act.data_ptr(), T, 0, s16=True)
    torch.cuda.synchronize()
    check_rows(chains, pcm, d_out.cpu().numpy(), d_vad.cpu().numpy(), d_g.cpu().numpy(), {s: s for s in rows}, f"masked device s16 n={n}",
               active=act, s16=True)


def test_resets_host_and_device_lists(model, blob_default):
    torch = pytest.importorskip("torch")
    n, L, T = 600, 3, 4
    pcm = tiled(low_pcm(30, 3 * T, L, seed=9), n)
    rows = [0, 1, 2, 3, 599]
    b = capi.Batch(model, n)
    b.set_pcm_rate(16000)
    chains = {s: Chain(blob_default, L) for s in rows}
    out, vad, gains = b.process(pcm[:T])
    check_rows(chains, pcm[:T], out, vad, gains, {s: s for s in rows}, "before reset")
    b.reset_streams([1, 599])
    for s in (1, 599):
        chains[s].reset()
    out, vad, gains = b.process(pcm[T:2 * T])
    check_rows(chains, pcm[T:2 * T], out, vad, gains, {s: s for s in rows}, "after host-list reset")
    dev = torch.device("cuda", 0)
    d_list = torch.tensor([2, 3], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    b.reset_streams_device(d_list.data_ptr(), 2, 0)
    torch.cuda.synchronize()
    for s in (2, 3):
        chains[s].reset()
    out, vad, gains = b.process(pcm[2 * T:])
    check_rows(chains, pcm[2 * T:], out, vad, gains, {s: s for s in rows}, "after device-list reset")


def test_rate_switches_zero_history_and_carry_state(model, blob_default):
    n, T = 300, 3
    rows = [0, 7, 299]
    b = capi.Batch(model, n)
    # 48 kHz frames first, straight through the oracle
    hi = tiled(fuzz_pcm(20, T, 2), n)
    o = {s: Oracle(blob_default) for s in rows}
    out, vad, _ = b.process(hi)
    for s in rows:
        for t in range(T):
            ro, rv, _ = o[s].process(hi[t, s])
            assert_bits_equal(out[t, s], ro, f"48k stream {s} frame {t}")
    for rate in (16000, 8000):
        L = RATE_L[rate]
        b.set_pcm_rate(rate)
        chains = {}
        for s in rows:
            c = Chain(blob_default, L)
            c.o = o[s]  # the DenoiseState carries over; the histories start from zero
            chains[s] = c
        pcm = tiled(low_pcm(20, T, L, seed=rate), n)
        out, vad, gains = b.process(pcm)
        check_rows(chains, pcm, out, vad, gains, {s: s for s in rows}, f"after switch to {rate}")
    for s in rows:
        assert_bits_equal(b.export_state(s), o[s].get_state(), f"state of stream {s} after the switches")


def test_48k_rate_is_a_no_op_and_refusals(model):
    n, T = 100, 4
    pcm = tiled(fuzz_pcm(10, T, 4), n)
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    assert b.set_pcm_rate(48000) == 48000
    for x, y in zip(a.process(pcm), b.process(pcm)):
        assert_bits_equal(y, x, "set_pcm_rate(48000) on a fresh batch")
    with pytest.raises(ValueError):
        b.set_pcm_rate(44100)
    assert b.pcm_rate == 48000
    b.set_pcm_rate(8000)
    assert capi.lib().rnnoise_batch_set_pcm_rate(b.h, 12345) == -1 and b.pcm_rate == 8000
    z = np.zeros((1, n, 480), np.float32)
    with pytest.raises(RuntimeError):
        b.train_features(z, z, np.zeros((1, n), np.float32), np.full(n, 481), np.full(n, 32), np.zeros(n))
    # back to 48 kHz: the batch runs 48 kHz frames again, continuing its DenoiseState
    b.set_pcm_rate(48000)
    a2 = capi.Batch(model, n)
    a2.process(pcm)
    for s in (0, 50):
        a2.import_state(s, b.export_state(s))
    got = b.process(pcm)
    want = a2.process(pcm)
    for s in (0, 50):
        assert_bits_equal(got[0][:, s], want[0][:, s], f"48k again, stream {s}")


def test_import_zeroes_history(model, blob_default):
    n, L, T = 50, 2, 4
    pcm = tiled(low_pcm(10, 2 * T, L, seed=13), n)
    b = capi.Batch(model, n)
    b.set_pcm_rate(24000)
    b.process(pcm[:T])
    src = Oracle(blob_default)
    for t in range(3):
        src.process(fuzz_pcm(1, 3, 21)[t, 0])
    b.import_state(4, src.get_state())
    c = Chain(blob_default, L)
    c.o = src
    out, vad, gains = b.process(pcm[T:])
    check_rows({4: c}, pcm[T:], out, vad, gains, {4: 4}, "after import")


def test_torch_op_at_16k(model, blob_default):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, L, T = 40, 3, 4
    pcm = tiled(low_pcm(40, T, L, seed=17), n)
    dev = torch.device("cuda", 0)
    op = RNNoiseOp(blob_default, n, rate=16000)
    out, vad = op(torch.from_numpy(pcm).to(dev))[:2]
    torch.cuda.synchronize()
    assert tuple(out.shape) == (T, n, 160)
    b = capi.Batch(model, n)
    b.set_pcm_rate(16000)
    want = b.process(pcm)
    assert_bits_equal(out.cpu().numpy(), want[0], "torch op out")
    assert_bits_equal(vad.cpu().numpy(), want[1], "torch op vad")
