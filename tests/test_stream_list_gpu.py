"""Stream-list calls on the GPU (include/rnnoise_amd.h: rnnoise_batch_process_*list*): a listed stream gets, bit for bit, what the
oracle gives on that stream's listed (and present) frames only, and exactly what a masked call with the same presence in full-size
buffers gives it -- out, vad, gains and state; an unlisted stream is not touched.  Compact buffers are indexed by list position."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from oracle.binding import Oracle
from rnnoise_amd import capi, synth
from test_gpu_parity import fuzz_pcm

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


def tiled_pcm(n, T, seed=1, distinct=97, frame=480):
    base = fuzz_pcm(distinct, T, seed)[:, :, :frame]
    return np.ascontiguousarray(np.tile(base, (1, (n + distinct - 1) // distinct, 1))[:, :n])


def scatter(n, streams, rows_pcm, rows_act):
    """the full-size masked-call buffers that give `streams` the same frames as a list call (unlisted streams absent)"""
    T = rows_pcm.shape[0]
    pcm = np.zeros((T, n) + rows_pcm.shape[2:], rows_pcm.dtype)
    act = np.zeros((T, n), np.uint8)
    pcm[:, streams] = rows_pcm
    act[:, streams] = rows_act
    return pcm, act


def run_list(b, pcm, streams, active=None, s16=False):
    out = np.full(pcm.shape, np.int16(-7777) if s16 else SENTINEL, pcm.dtype)
    fn = b.process_list_s16 if s16 else b.process_list
    return fn(pcm, streams, active, out=out)


def check_against_masked(twin, n, streams, pcm_rows, act_rows, got, what, s16=False):
    """twin takes the same frames through a masked call; got = the list call's (out, vad, gains)"""
    full, act = scatter(n, streams, pcm_rows, act_rows)
    sent = np.int16(-7777) if s16 else SENTINEL
    out_m = np.full(full.shape, sent, full.dtype)
    fn = twin.process_masked_s16 if s16 else twin.process_masked
    want = fn(full, act, out=out_m)
    for name, g, w in zip(("out", "vad", "gains"), got, want):
        assert_bits_equal(g, w[:, streams], f"{what}: {name}")


def check_states(a, b, streams, what):
    for s in streams:
        assert_bits_equal(a.export_state(int(s)), b.export_state(int(s)), f"{what}: state of stream {s}")


CALLS = [1, 5, 1, 8, 5]


def test_list_calls_follow_the_oracle(model, blob_default):
    n, T = 300, sum(CALLS)
    pcm = np.concatenate([fuzz_pcm(150, T, 21), synth.batch_pcm(list(range(150)), T, lead_silence=2)], axis=1).astype(np.float32)
    rng = np.random.default_rng(7)
    never = set(range(280, 300))  # never listed
    b = capi.Batch(model, n)
    fresh = capi.Batch(model, n).export_state(0)
    refs = {s: Oracle(blob_default) for s in range(280)}
    t0 = 0
    for k in CALLS:
        streams = rng.permutation(280)[: int(rng.integers(1, 280))].astype(np.int32)
        rows = np.ascontiguousarray(pcm[t0:t0 + k][:, streams])
        out, vad, gains = run_list(b, rows, streams)
        for i, s in enumerate(streams):
            for t in range(k):
                ro, rv, rec = refs[s].process(rows[t, i])
                tag = f"call at {t0}: row {i} stream {s} frame {t}"
                assert_bits_equal(out[t, i], ro, tag + " out")
                assert_bits_equal(vad[t, i], np.float32(rv), tag + " vad")
                assert_bits_equal(gains[t, i], np.frombuffer(rec.gains, np.float32), tag + " gains")
        t0 += k
    for s in range(280):
        assert_bits_equal(b.export_state(s), refs[s].get_state(), f"state of stream {s}")
    for s in sorted(never):
        assert_bits_equal(b.export_state(s), fresh, f"never-listed stream {s} kept its state")


def device_twins(torch, model, n, rows, frames, nn_path=None):
    """a list batch and a masked twin fed the same frames through the device forms (pipelined when frames > 1)"""
    dev = torch.device("cuda", 0)
    a, m = capi.Batch(model, n), capi.Batch(model, n)
    if nn_path is not None:
        a.set_nn_path(nn_path)
        m.set_nn_path(nn_path)
    return dev, a, m


def dev_list_call(torch, b, d_pcm_full, streams_t, act_rows_t):
    """list call with rows gathered from the full-size pcm; returns device (out, vad, gains)"""
    rows = d_pcm_full[:, streams_t.long()].contiguous()
    T, R = rows.shape[0], rows.shape[1]
    out = torch.full_like(rows, float(SENTINEL))
    vad = torch.empty((T, R), device=rows.device)
    gains = torch.empty((T, R, 32), device=rows.device)
    b.process_list_device(out.data_ptr(), rows.data_ptr(), vad.data_ptr(), gains.data_ptr(), streams_t.data_ptr(), R,
                          act_rows_t.data_ptr() if act_rows_t is not None else 0, T)
    return out, vad, gains


def dev_masked_call(torch, b, d_pcm_full, streams_t, act_rows_t):
    T, n = d_pcm_full.shape[0], d_pcm_full.shape[1]
    act = torch.zeros((T, n), dtype=torch.uint8, device=d_pcm_full.device)
    act[:, streams_t.long()] = act_rows_t if act_rows_t is not None else 1
    out = torch.full_like(d_pcm_full, float(SENTINEL))
    vad = torch.empty((T, n), device=d_pcm_full.device)
    gains = torch.empty((T, n, 32), device=d_pcm_full.device)
    b.process_masked_device(out.data_ptr(), d_pcm_full.data_ptr(), vad.data_ptr(), gains.data_ptr(), act.data_ptr(), T)
    return out, vad, gains


def compare_dev(torch, got, want, streams_t, what):
    idx = streams_t.long()
    torch.cuda.synchronize()
    for name, g, w in zip(("out", "vad", "gains"), got, want):
        assert torch.equal(g.view(torch.int32), w[:, idx].contiguous().view(torch.int32)), f"{what}: {name} differs from the masked call"


@pytest.mark.parametrize("n,rows", [(4096, 1000), (65536, 8192)])
@pytest.mark.parametrize("frames", [1, 16])
def test_list_equals_masked_at_size(model, n, rows, frames):
    torch = pytest.importorskip("torch")
    dev, a, m = device_twins(torch, model, n, rows, frames)
    base = torch.from_numpy(fuzz_pcm(97, 2 * frames, 5)).to(dev)
    d_pcm = base[:, torch.arange(n, device=dev) % 97].contiguous()
    gen = torch.Generator(device="cpu").manual_seed(n + frames)
    checked = set()
    for c in range(2):
        streams = torch.randperm(n, generator=gen)[:rows].to(torch.int32).to(dev)
        act = (torch.rand((frames, rows), generator=gen) < 0.8).to(torch.uint8).to(dev) if c else None
        sl = d_pcm[c * frames:(c + 1) * frames].contiguous()
        got = dev_list_call(torch, a, sl, streams, act)
        want = dev_masked_call(torch, m, sl, streams, act)
        compare_dev(torch, got, want, streams, f"n={n} rows={rows} frames={frames} call {c}")
        checked |= set(streams[:8].cpu().tolist())
    check_states(a, m, sorted(checked | {0, n - 1}), f"n={n} rows={rows} frames={frames}")


def test_layer_wise_images_follow_list_calls(model):
    torch = pytest.importorskip("torch")
    n, rows = 20480, 3000
    dev, a, m = device_twins(torch, model, n, rows, 1)
    base = torch.from_numpy(fuzz_pcm(97, 12, 8)).to(dev)
    d_pcm = base[:, torch.arange(n, device=dev) % 97].contiguous()
    gen = torch.Generator(device="cpu").manual_seed(3)
    streams = None
    for c, (kind, t0, k) in enumerate((("lock", 0, 3), ("list", 3, 2), ("list", 5, 1), ("lock", 6, 3), ("list", 9, 1), ("lock", 10, 2))):
        sl = d_pcm[t0:t0 + k].contiguous()
        if kind == "lock":  # the lock-step device call on both: the layer-wise network from 10,240 streams
            outs = []
            for b in (a, m):
                o, v, g = torch.empty_like(sl), torch.empty((k, n), device=dev), torch.empty((k, n, 32), device=dev)
                b.process_device(o.data_ptr(), sl.data_ptr(), v.data_ptr(), g.data_ptr(), k)
                outs.append((o, v, g))
            torch.cuda.synchronize()
            for name, x, y in zip(("out", "vad", "gains"), *outs):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"lock-step call {c}: {name}"
        else:
            streams = torch.randperm(n, generator=gen)[:rows].to(torch.int32).to(dev)
            compare_dev(torch, dev_list_call(torch, a, sl, streams, None), dev_masked_call(torch, m, sl, streams, None), streams,
                        f"list call {c}")
    check_states(a, m, sorted(set(streams[:6].cpu().tolist()) | {0, 17, n - 1}), "end")


def test_s16_is_float_then_cast(model):
    n, T = 700, 9
    pcm = tiled_pcm(n, T, seed=13)
    streams = np.random.default_rng(1).permutation(n)[:333].astype(np.int32)
    bf, bs = capi.Batch(model, n), capi.Batch(model, n)
    for sl in (slice(0, 1), slice(1, 6), slice(6, T)):
        rows = np.ascontiguousarray(pcm[sl][:, streams])
        of, vf, gf = run_list(bf, rows, streams)
        o16, v16, g16 = run_list(bs, rows.astype(np.int16), streams, s16=True)
        assert_bits_equal(v16, vf, "vad")
        assert_bits_equal(g16, gf, "gains")
        x = of.astype(np.float64)
        q = np.where((x >= -2.0 ** 31) & (x < 2.0 ** 31), np.trunc(x), -2.0 ** 31).astype(np.int64)
        assert np.array_equal(o16, (q & 0xFFFF).astype(np.uint16).view(np.int16)), "the float bits, then the truncating cast"
    check_states(bf, bs, streams[:5], "s16")


@pytest.mark.parametrize("rate", [16000, 8000])
def test_low_rate_rows(model, rate):
    n, T = 500, 10
    L = 48000 // rate
    pcm = tiled_pcm(n, T, seed=rate, frame=480 // L)
    streams = np.random.default_rng(rate).permutation(n)[:180].astype(np.int32)
    act = (np.random.default_rng(2).random((T, 180)) < 0.7).astype(np.uint8)
    a, m = capi.Batch(model, n), capi.Batch(model, n)
    a.set_pcm_rate(rate)
    m.set_pcm_rate(rate)
    for sl in (slice(0, 4), slice(4, 5), slice(5, T)):
        rows = np.ascontiguousarray(pcm[sl][:, streams])
        check_against_masked(m, n, streams, rows, act[sl], run_list(a, rows, streams, act[sl]), f"{rate} Hz frames {sl}")
    check_states(a, m, list(streams[:5]) + [int(np.setdiff1d(np.arange(n), streams)[0])], f"{rate} Hz")


def test_model_slots_controls_mask_and_device_reset(model, blob_little):
    """two model slots with the list spanning both, suppression controls with the VAD gate, an active mask on top of the list, and
    rnnoise_batch_reset_streams_device between list calls -- against a twin that takes the same frames through masked calls"""
    torch = pytest.importorskip("torch")
    n, T = 1200, 12
    pcm = tiled_pcm(n, T, seed=31)
    little = capi.Model(blob_little)
    slots = (np.arange(n) % 3 == 1).astype(np.uint8)
    ctl = capi.controls_table(n, limit_db=np.where(np.arange(n) % 2, 12.0, np.inf), vad_threshold=np.where(np.arange(n) % 4 < 2, 0.6, 0.0),
                              hold_frames=2)
    a, m = capi.Batch(model, n), capi.Batch(model, n)
    for b in (a, m):
        b.set_nn_path(1)
        b.add_model(little)
        b.set_stream_models(slots)
        b.set_stream_controls(ctl)
    rng = np.random.default_rng(4)
    dev = torch.device("cuda", 0)
    reset = torch.tensor([5, 6, 7, 1199], dtype=torch.int32, device=dev)
    for c, sl in enumerate((slice(0, 5), slice(5, 6), slice(6, T))):
        if c == 2:
            for b in (a, m):
                b.reset_streams_device(reset.data_ptr(), int(reset.numel()))
            torch.cuda.synchronize()
        others = np.setdiff1d(np.arange(n), [5, 6, 1199])
        streams = rng.permutation(np.concatenate([[5, 6, 1199], rng.permutation(others)[:397]])).astype(np.int32)
        act = (rng.random((sl.stop - sl.start, 400)) < 0.75).astype(np.uint8)
        rows = np.ascontiguousarray(pcm[sl][:, streams])
        check_against_masked(m, n, streams, rows, act, run_list(a, rows, streams, act), f"call {c}")
    check_states(a, m, [5, 6, 7, 1199, 0, 1, 2, 3], "end")
    for b in (a, m):
        b.close()
    little.close()


def test_refusals_and_edges(model):
    torch = pytest.importorskip("torch")
    n, T = 64, 3
    pcm = tiled_pcm(n, T, seed=2)
    a, m = capi.Batch(model, n), capi.Batch(model, n)
    check_against_masked(m, n, np.arange(0, 64, 2, dtype=np.int32), pcm[:1, ::2].copy(), np.ones((1, 32), np.uint8),
                         run_list(a, np.ascontiguousarray(pcm[:1, ::2]), np.arange(0, 64, 2, dtype=np.int32)), "first call")
    before = [a.export_state(s) for s in range(n)]
    rows = np.ascontiguousarray(pcm[1:2, :3])
    for bad in ([1, 2, 1], [1, 2, 64], [-1, 2, 3]):
        with pytest.raises(ValueError):
            run_list(a, rows, np.array(bad, np.int32))
    L = capi.lib()
    buf = (np.zeros((1, 65, 480), np.float32))
    fp = buf.ctypes.data_as(capi.C.POINTER(capi.C.c_float))
    idx = np.arange(65, dtype=np.int32)
    ip = idx.ctypes.data_as(capi.C.POINTER(capi.C.c_int))
    assert L.rnnoise_batch_process_list(a.h, fp, fp, None, None, ip, 65, None, 1) == -1  # n_rows > n_streams
    assert L.rnnoise_batch_process_list(a.h, fp, fp, None, None, None, 1, None, 1) == -1  # NULL list
    assert L.rnnoise_batch_process_list(a.h, fp, fp, None, None, ip, 0, None, 1) == 0  # n_rows == 0: a no-op
    assert L.rnnoise_batch_process_device_list(a.h, None, None, None, None, None, 0, None, 1, None) == 0
    assert L.rnnoise_batch_process_device_list(a.h, None, None, None, None, None, 65, None, 1, None) == -1
    for s in range(n):
        assert_bits_equal(a.export_state(s), before[s], f"refused calls left stream {s} alone")
    # out-of-range device entries: absent rows -- out not written, vad 0, gains 0 -- and the valid rows as the masked call
    dev = torch.device("cuda", 0)
    lst = [3, -1, 9, 64, 1 << 30, 10]
    streams_t = torch.tensor(lst, dtype=torch.int32, device=dev)
    d_rows = torch.from_numpy(np.ascontiguousarray(pcm[1:3][:, [3, 0, 9, 0, 0, 10]])).to(dev)
    out = torch.full_like(d_rows, float(SENTINEL))
    vad = torch.full((2, 6), 7.0, device=dev)
    gains = torch.full((2, 6, 32), 7.0, device=dev)
    a.process_list_device(out.data_ptr(), d_rows.data_ptr(), vad.data_ptr(), gains.data_ptr(), streams_t.data_ptr(), 6, 0, 2)
    torch.cuda.synchronize()
    out, vad, gains = out.cpu().numpy(), vad.cpu().numpy(), gains.cpu().numpy()
    ok = [0, 2, 5]
    for i in (1, 3, 4):
        assert (out[:, i].view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"absent row {i} written"
        assert (vad[:, i] == 0).all() and not gains[:, i].any(), f"absent row {i}: vad / gains not zero"
    check_against_masked(m, n, np.array([3, 9, 10], np.int32), pcm[1:3][:, [3, 9, 10]].copy(), np.ones((2, 3), np.uint8),
                         (out[:, ok], vad[:, ok], gains[:, ok]), "out-of-range device entries")
    check_states(a, m, range(n), "after the device call")


def test_torch_op_matches_capi(model, blob_default):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, T = 300, 9
    pcm = tiled_pcm(n, T, seed=17)
    op = RNNoiseOp(blob_default, n)
    ref = capi.Batch(model, n)
    ref.set_nn_path(1)
    dev = op.device
    rng = np.random.default_rng(6)
    for i, sl in enumerate((slice(0, 4), slice(4, 5), slice(5, T))):
        streams = rng.permutation(n)[:120].astype(np.int32)
        act = (rng.random((sl.stop - sl.start, 120)) < 0.7) if i else None
        rows = np.ascontiguousarray(pcm[sl][:, streams])
        got = op.process_list(torch.from_numpy(rows).to(dev), torch.from_numpy(streams).to(dev),
                              None if act is None else torch.from_numpy(act).to(dev))
        torch.cuda.synchronize()
        want = ref.process_list(rows, streams, act)  # (absent rows: zeros, as the op returns them)
        for name, g, w in zip(("out", "vad", "gains"), got, want):
            assert_bits_equal(g.cpu().numpy(), w, f"torch op call {i} {name}")
    assert int(op.state.item()) == T
    op.close()
