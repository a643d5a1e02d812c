"""Masked calls and per-stream reset on the GPU (include/rnnoise_amd.h): every stream must give, bit for bit, what the oracle gives
when it runs rnnoise_process_frame() on that stream's PRESENT frames only; absent frames leave `out` as the caller had it, read
vad 0 and zero gains, and touch no state; a reset stream equals a fresh rnnoise_create() state and no other stream changes."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from oracle.binding import Oracle
from rnnoise_amd import capi
from test_gpu_parity import fuzz_pcm

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


class Refs:
    """one oracle per checked stream, fed only that stream's present frames"""

    def __init__(self, blob, streams):
        self.blob = blob
        self.o = {s: Oracle(blob) for s in streams}

    def reset(self, s):
        self.o[s] = Oracle(self.blob)

    def check(self, pcm, active, out, vad, gains, what=""):
        T = pcm.shape[0]
        for s, o in self.o.items():
            for t in range(T):
                tag = f"{what} stream {s} frame {t}"
                if active[t, s]:
                    ro, rv, rec = o.process(pcm[t, s])
                    assert_bits_equal(out[t, s], ro, tag + " out")
                    assert_bits_equal(vad[t, s], np.float32(rv), tag + " vad")
                    assert_bits_equal(gains[t, s], np.frombuffer(rec.gains, np.float32), tag + " gains")
                else:
                    assert (out[t, s].view(np.uint32) == SENTINEL.view(np.uint32)).all(), tag + ": absent row written"
                    assert vad[t, s] == 0 and not gains[t, s].any(), tag + ": absent frame has vad / gains"

    def check_state(self, batch, streams=None, what=""):
        for s in (self.o if streams is None else streams):
            assert_bits_equal(batch.export_state(s), self.o[s].get_state(), f"{what} state of stream {s}")


def run_masked(batch, pcm, active):
    out = np.full_like(pcm, SENTINEL)
    return batch.process_masked(pcm, active, out=out)


def tiled_pcm(n, T, seed=1, distinct=160):
    base = fuzz_pcm(distinct, T, seed)
    return np.ascontiguousarray(np.tile(base, (1, (n + distinct - 1) // distinct, 1))[:, :n])


def pattern_mask(n, T, density, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random((T, n)) < density).astype(np.uint8)
    a[:, 0] = 0          # absent throughout
    a[:, 1] = 1
    a[0, 1] = 0          # absent on the first frame
    a[:, 2] = 1
    a[-1, 2] = 0         # absent on the last frame
    a[:, 3] = np.arange(T) % 2  # alternating
    a[:, 4] = 0
    a[T // 3, 4] = 1     # present once
    return a


CALLS = [8, 1, 5]


@pytest.mark.parametrize("n", [1, 65, 512, 513, 2048, 2560, 4096, 10240, 40037])
def test_all_ones_mask_is_the_unmasked_call(model, n):
    T = sum(CALLS)
    pcm = tiled_pcm(n, T, distinct=97)
    a, b, c = capi.Batch(model, n), capi.Batch(model, n), capi.Batch(model, n)
    ones = np.ones((T, n), np.uint8)
    t0 = 0
    for k in CALLS:
        sl = slice(t0, t0 + k)
        want = a.process(pcm[sl])
        got = run_masked(b, pcm[sl], ones[sl])
        nul = c.process_masked(pcm[sl], None)
        for name, x, y, z in zip(("out", "vad", "gains"), want, got, nul):
            assert_bits_equal(y, x, f"n={n} frames {t0}+{k} {name} (all-ones mask)")
            assert_bits_equal(z, x, f"n={n} frames {t0}+{k} {name} (NULL mask)")
        t0 += k
    for s in sorted({0, n // 2, n - 1}):
        assert_bits_equal(b.export_state(s), a.export_state(s), f"n={n} state of stream {s}")


MIXED = [1, 8, 3, 1, 5, 4]


@pytest.mark.parametrize("n", [160, 4096, 10277])
@pytest.mark.parametrize("density", [0.5, 0.875])
def test_random_and_pattern_masks_follow_the_oracle(model, blob_default, n, density):
    T = sum(MIXED)
    pcm = fuzz_pcm(n, T, 3) if n == 160 else tiled_pcm(n, T, seed=3)
    act = pattern_mask(n, T, density, seed=n + int(density * 8))
    checked = range(n) if n == 160 else sorted(set(range(8)) | set(range(8, n, 41)) | {n - 1})
    refs = Refs(blob_default, checked)
    b = capi.Batch(model, n)
    t0 = 0
    for k in MIXED:
        sl = slice(t0, t0 + k)
        out, vad, gains = run_masked(b, pcm[sl], act[sl])
        refs.check(pcm[sl], act[sl], out, vad, gains, f"n={n} d={density} call at {t0}")
        t0 += k
    refs.check_state(b, [s for s in checked if s < 8 or s % 5 == 0], f"n={n} d={density}")
    f, sil, _ = b.debug_last()
    assert sil[0] == 2, "debug_last: a stream absent from the last frame reports silence 2"


def test_masked_unmasked_paths_and_state_import(model, blob_default):
    n, T = 600, 20
    pcm = tiled_pcm(n, T, seed=5)
    act = pattern_mask(n, T, 0.6, seed=11)
    checked = sorted(set(range(8)) | set(range(8, n, 23)))
    refs = Refs(blob_default, checked)
    b = capi.Batch(model, n)
    plan = [(4, True, 0), (3, False, 1), (4, True, 2), (3, True, 1), (2, False, 0), (4, True, 2)]
    t0 = 0
    for i, (k, masked, path) in enumerate(plan):
        b.set_nn_path(path)
        sl = slice(t0, t0 + k)
        a = act[sl] if masked else np.ones((k, n), np.uint8)
        if masked:
            out, vad, gains = run_masked(b, pcm[sl], a)
        else:
            out, vad, gains = b.process(pcm[sl])
        refs.check(pcm[sl], a, out, vad, gains, f"call {i} ({'masked' if masked else 'unmasked'}, path {path})")
        t0 += k
        if i == 2:  # per-stream mode: export, and import another stream's oracle state into stream 7
            refs.check_state(b, [3, 7, 31], "before import")
            b.import_state(7, refs.o[31].get_state())
            refs.o[7].set_state(refs.o[31].get_state())
    refs.check_state(b, checked, "after the plan")
    with pytest.raises(RuntimeError):  # training-feature extraction refuses a batch in per-stream frame phase
        b.train_features(pcm[:1], pcm[:1], np.zeros((1, n), np.float32), np.full(n, 481), np.full(n, 32), np.zeros(n))


@pytest.mark.parametrize("n", [4096, 10240])
def test_reset_streams_mid_run(model, blob_default, n):
    T1, T2 = 6, 6
    pcm = tiled_pcm(n, T1 + T2, seed=7)
    act = pattern_mask(n, T1 + T2, 0.75, seed=n)
    listed = sorted({5, 6, 17, 18, 1000, n - 1})
    checked = sorted(set(listed) | {0, 1, 2, 3, 4, 7, 16, 19, 999, 2049, n - 2})
    refs = Refs(blob_default, checked)
    b = capi.Batch(model, n)  # (10,240 streams: the layer-wise network and its state images)
    out, vad, gains = run_masked(b, pcm[:T1], act[:T1])
    refs.check(pcm[:T1], act[:T1], out, vad, gains, "before reset")
    others = [s for s in checked if s not in listed]
    before = {s: b.export_state(s) for s in others}
    with pytest.raises(ValueError):
        b.reset_streams([0, n])  # out of range: nothing is reset
    b.reset_streams(listed + [5])  # (a duplicate)
    for s in others:
        assert_bits_equal(b.export_state(s), before[s], f"stream {s} changed by a reset of others")
    for s in listed:
        refs.reset(s)
        assert not b.export_state(s).any()
    out, vad, gains = run_masked(b, pcm[T1:], act[T1:])
    refs.check(pcm[T1:], act[T1:], out, vad, gains, "after reset")
    refs.check_state(b, what="end")


def test_reset_streams_device_between_masked_device_calls(model, blob_default):
    torch = pytest.importorskip("torch")
    n, T1, T2 = 4096, 5, 4
    pcm = tiled_pcm(n, T1 + T2, seed=9)
    act = pattern_mask(n, T1 + T2, 0.75, seed=99)
    listed = [3, 64, 65, 4095, 4095, -1, n]  # (duplicate and out-of-range entries: ignored)
    checked = sorted({0, 1, 2, 3, 4, 63, 64, 65, 66, 2000, 4094, 4095})
    refs = Refs(blob_default, checked)
    b = capi.Batch(model, n)
    b.set_nn_path(2)  # the layer-wise network: its state images of the listed tiles must follow the reset
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_act = torch.from_numpy(act).to(dev)
    d_out = torch.full_like(d_pcm, float(SENTINEL))
    d_vad = torch.empty((T1 + T2, n), device=dev)
    d_gains = torch.empty((T1 + T2, n, 32), device=dev)
    d_list = torch.tensor(listed, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        h = s.cuda_stream
        b.process_masked_device(d_out.data_ptr(), d_pcm.data_ptr(), d_vad.data_ptr(), d_gains.data_ptr(), d_act.data_ptr(), T1, h)
        b.reset_streams_device(d_list.data_ptr(), len(listed), h)
        b.process_masked_device(d_out[T1:].data_ptr(), d_pcm[T1:].data_ptr(), d_vad[T1:].data_ptr(), d_gains[T1:].data_ptr(),
                                d_act[T1:].data_ptr(), T2, h)
    s.synchronize()
    out, vad, gains = d_out.cpu().numpy(), d_vad.cpu().numpy(), d_gains.cpu().numpy()
    refs.check(pcm[:T1], act[:T1], out[:T1], vad[:T1], gains[:T1], "before reset")
    for st in (3, 64, 65, 4095):
        refs.reset(st)
    refs.check(pcm[T1:], act[T1:], out[T1:], vad[T1:], gains[T1:], "after device reset")
    refs.check_state(b, what="end")


def s16_of(x):
    """the C float -> short conversion as x86 compiles it (examples/rnnoise_demo.c:58)"""
    x = x.astype(np.float64)
    q = np.where((x >= -2.0 ** 31) & (x < 2.0 ** 31), np.trunc(np.nan_to_num(x)), -2.0 ** 31).astype(np.int64)
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)


def test_s16_masked_is_float_then_cast(model):
    n, T = 700, 12
    pcm = tiled_pcm(n, T, seed=13)
    act = pattern_mask(n, T, 0.5, seed=5)
    bf, bs = capi.Batch(model, n), capi.Batch(model, n)
    sent16 = np.int16(-7777)
    for sl in (slice(0, 7), slice(7, 8), slice(8, T)):
        of, vf, gf = run_masked(bf, pcm[sl], act[sl])
        o16 = np.full(pcm[sl].shape, sent16, np.int16)
        o16, v16, g16 = bs.process_masked_s16(pcm[sl].astype(np.int16), act[sl], out=o16)
        assert_bits_equal(v16, vf, "vad")
        assert_bits_equal(g16, gf, "gains")
        a = act[sl].astype(bool)
        assert np.array_equal(o16[a], s16_of(of[a])), "present rows: the float bits, then the truncating cast"
        assert (o16[~a] == sent16).all(), "absent rows written"
    for s in (0, 3, 350, 699):
        assert_bits_equal(bs.export_state(s), bf.export_state(s), f"state of stream {s}")


def test_torch_op_matches_capi(model, blob_default):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, T = 300, 9
    pcm = tiled_pcm(n, T, seed=17)
    act = pattern_mask(n, T, 0.7, seed=3)
    op = RNNoiseOp(blob_default, n)
    ref = capi.Batch(model, n)
    ref.set_nn_path(1)
    nul = capi.Batch(model, n)
    nul.set_nn_path(1)
    dev = op.device
    for i, sl in enumerate((slice(0, 4), slice(4, 5), slice(5, T))):
        if i == 2:
            op.reset_streams([2, 40, 41])
            ref.reset_streams([2, 40, 41])
        got = op.process_masked(torch.from_numpy(pcm[sl]).to(dev), torch.from_numpy(act[sl].astype(bool)).to(dev))
        torch.cuda.synchronize()
        want = ref.process_masked(pcm[sl], act[sl])  # (absent rows: zeros, as the op returns them)
        for name, g, w in zip(("out", "vad", "gains"), got, want):
            assert_bits_equal(g.cpu().numpy(), w, f"torch op call {i} {name}")
    assert int(op.state.item()) == T
    # a NULL device mask is the unmasked device call
    d_pcm = torch.from_numpy(pcm[:3]).to(dev)
    d_out, d_vad, d_g = torch.empty_like(d_pcm), torch.empty((3, n), device=dev), torch.empty((3, n, 32), device=dev)
    nul.process_masked_device(d_out.data_ptr(), d_pcm.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), 0, 3)
    torch.cuda.synchronize()
    w_out, w_vad, w_g = capi.Batch(model, n).process(pcm[:3])
    assert_bits_equal(d_out.cpu().numpy(), w_out, "NULL device mask: out")
    assert_bits_equal(d_vad.cpu().numpy(), w_vad, "NULL device mask: vad")
    op.close()
