"""Several models in one batch (include/rnnoise_amd.h: rnnoise_batch_add_model, the stream-model map) on the GPU.

Every stream of a mixed batch must give, bit for bit, what the same stream gives in a batch of its own model alone fed the same PCM --
out, vad, gains and the exported state -- on every network form; a sample of streams is also run through the oracle with the blob of
its model.  A stream whose model changes between two calls must give what the oracle gives when its state is carried into a state
initialised with the new model (get_state / set_state).  Masked calls, silence, per-stream reset, the host-fed path, int16 and 16 kHz
calls work on a mixed batch as on a one-model one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, load_blob
from oracle.binding import Oracle
from rnnoise_amd import blob as rb
from rnnoise_amd import capi
from test_masked_gpu import SENTINEL, pattern_mask, tiled_pcm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def blobs():
    # default and little from tests/golden, then synthetic models of the same architecture: eight slots' worth
    return [load_blob("default"), load_blob("little")] + [rb.synth_model(seed=40 + i) for i in range(6)]


@pytest.fixture(scope="module")
def models(blobs):
    return [capi.Model(b) for b in blobs]


def slot_map(kind, n, k, seed=5):
    s = np.arange(n)
    if kind == "group":        # whole 64-stream groups (and so whole 16-stream tiles) on one slot
        m = (s // 64) % k
    elif kind == "interleaved":
        m = s % k
    else:
        m = np.random.default_rng(seed).integers(0, k, n)
    return np.ascontiguousarray(m, np.uint8)


def mixed_batch(models, k, n, slots, path=None):
    b = capi.Batch(models[0], n)
    for i in range(1, k):
        assert b.add_model(models[i]) == i
    b.set_stream_models(slots)
    if path is not None:
        b.set_nn_path(path)
    return b


def single_batch(model, n, path=None):
    b = capi.Batch(model, n)
    if path is not None:
        b.set_nn_path(path)
    return b


def run_calls(b, pcm, calls, fn="process"):
    outs, vads, gains, t = [], [], [], 0
    for c in calls:
        o, v, g = getattr(b, fn)(pcm[t:t + c])
        outs.append(o)
        vads.append(v)
        gains.append(g)
        t += c
    assert t == pcm.shape[0]
    return np.concatenate(outs), np.concatenate(vads), np.concatenate(gains)


def compare_with_singles(models, mb, got, slots, run_single, state_sample=6, what=""):
    """every stream of the mixed result `got` against the same stream of a one-model batch of its slot's model"""
    for j in sorted(set(slots.tolist())):
        sel = np.nonzero(slots == j)[0]
        sb, want = run_single(models[j])
        for name, a, w in zip(("out", "vad", "gains"), got, want):
            assert_bits_equal(a[:, sel], w[:, sel], f"{what} slot {j} {name}")
        for s in sel[np.linspace(0, sel.size - 1, min(state_sample, sel.size)).astype(int)]:
            assert_bits_equal(mb.export_state(int(s)), sb.export_state(int(s)), f"{what} slot {j} state of stream {s}")
        sb.close()


def check_oracle(blobs, slots, pcm, got, mb, streams):
    for s in streams:
        o = Oracle(blobs[slots[s]])
        want = o.run(pcm[:, s])
        for name, a in zip(("out", "vad", "gains"), got):
            assert_bits_equal(a[:, s], want[name], f"oracle, stream {s} (slot {slots[s]}) {name}")
        assert_bits_equal(mb.export_state(int(s)), o.get_state(), f"oracle, state of stream {s}")


# (path, streams): path 0 at <= 512 streams runs rn_nn_one_kernel, above rn_nn_vector_kernel; path 1 runs the tile kernel -- the
# sixteen-wave form in the one-frame calls of batches with a tile per CU, the eight-wave form in multi-frame calls; path 2 the
# layer-wise network (front, GRU x 3, dense)
FORMS = [(0, 300), (0, 1000), (1, 1000), (1, 4099), (2, 1000), (2, 4099)]
MAPS = [("group", 2), ("interleaved", 3), ("random", 8)]
CALLS = [5, 1, 1, 4]


@pytest.mark.parametrize("kind,k", MAPS, ids=[m for m, _ in MAPS])
@pytest.mark.parametrize("path,n", FORMS, ids=[f"p{p}-n{n}" for p, n in FORMS])
def test_every_network_form(models, blobs, path, n, kind, k):
    T = sum(CALLS)
    pcm = tiled_pcm(n, T, seed=3, distinct=97)
    pcm[:3, ::11] = 0  # silent frames on some streams of every slot
    slots = slot_map(kind, n, k)
    mb = mixed_batch(models, k, n, slots, path)
    got = run_calls(mb, pcm, CALLS)
    assert (mb.stream_models() == slots).all()

    def run_single(m):
        sb = single_batch(m, n, path)
        return sb, run_calls(sb, pcm, CALLS)

    compare_with_singles(models, mb, got, slots, run_single, what=f"path {path}, {n} streams, {kind} map of {k}")
    check_oracle(blobs, slots, pcm, got, mb, [0, n - 1] + ([int(np.nonzero(slots == k - 1)[0][0])] if kind != "group" else []))
    mb.close()


def test_large_batch_two_models(models):
    """at size: 40,963 streams (layer-wise network by default), two models on a random map, against two one-model batches"""
    n, calls = 40963, [3, 1]
    pcm = tiled_pcm(n, sum(calls), seed=4, distinct=97)
    slots = slot_map("random", n, 2, seed=9)
    mb = mixed_batch(models, 2, n, slots)
    got = run_calls(mb, pcm, calls)

    def run_single(m):
        sb = single_batch(m, n)
        return sb, run_calls(sb, pcm, calls)

    compare_with_singles(models, mb, got, slots, run_single, state_sample=3, what="40,963 streams")
    mb.close()


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_switch_mid_stream(models, blobs, path, form):
    """process -> new map -> process, on one non-default HIP stream with no host synchronisation between the calls (device form), or
    with the synchronous host setter: each stream continues from its state with the weights of its new slot"""
    torch = pytest.importorskip("torch")
    n, k, T, t1 = 200, 3, 10, 4
    pcm = tiled_pcm(n, T, seed=6, distinct=61)
    a = slot_map("interleaved", n, k)
    b_ = np.ascontiguousarray((np.arange(n) // 2 + 1) % k, np.uint8)
    mb = mixed_batch(models, k, n, a, path)
    if form == "device":
        st = torch.cuda.Stream()
        d_in = torch.from_numpy(pcm).cuda()
        d_out = torch.empty_like(d_in)
        d_vad = torch.empty((T, n), device="cuda")
        d_gains = torch.empty((T, n, capi.NB_BANDS), device="cuda")
        d_map = torch.from_numpy(b_).cuda()
        torch.cuda.synchronize()
        h = st.cuda_stream
        mb.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_gains.data_ptr(), t1, h)
        mb.set_stream_models_device(d_map.data_ptr(), h)
        mb.process_device(d_out[t1:].data_ptr(), d_in[t1:].data_ptr(), d_vad[t1:].data_ptr(), d_gains[t1:].data_ptr(), T - t1, h)
        st.synchronize()
        got = (d_out.cpu().numpy(), d_vad.cpu().numpy(), d_gains.cpu().numpy())
    else:
        g1 = mb.process(pcm[:t1])
        mb.set_stream_models(b_)
        g2 = mb.process(pcm[t1:])
        got = tuple(np.concatenate([x, y]) for x, y in zip(g1, g2))
    assert (mb.stream_models() == b_).all()
    for s in range(12):  # streams that keep their slot and streams that change it, from and to every slot
        o = Oracle(blobs[a[s]])
        want = [o.run(pcm[:t1, s])]
        o2 = Oracle(blobs[b_[s]])
        o2.set_state(o.get_state())
        want.append(o2.run(pcm[t1:, s]))
        for name, x in zip(("out", "vad", "gains"), got):
            assert_bits_equal(x[:, s], np.concatenate([w[name] for w in want]), f"stream {s} ({a[s]} -> {b_[s]}) {name}")
        assert_bits_equal(mb.export_state(s), o2.get_state(), f"stream {s} state")
    mb.close()


def masked_device_run(torch, b, pcm, active, calls):
    """masked device calls with sentinels in every output buffer: rows nobody writes stay sentinels"""
    T, n = active.shape
    d_in = torch.from_numpy(pcm).cuda()
    d_out = torch.full_like(d_in, float(SENTINEL))
    d_vad = torch.full((T, n), float(SENTINEL), device="cuda")
    d_gains = torch.full((T, n, capi.NB_BANDS), float(SENTINEL), device="cuda")
    d_act = torch.from_numpy(active).cuda()
    t = 0
    for c in calls:
        if c == "reset":
            idx = torch.tensor([0, 3, 64, 65, n - 1], dtype=torch.int32, device="cuda")
            b.reset_streams_device(idx.data_ptr(), int(idx.numel()))
            continue
        b.process_masked_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(),
                                d_act[t:].data_ptr(), c)
        t += c
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_vad.cpu().numpy(), d_gains.cpu().numpy()


@pytest.mark.parametrize("path", [0, 1, 2])
def test_masked_calls_silence_and_reset(models, path):
    torch = pytest.importorskip("torch")
    n, k, calls = 1000, 3, [5, 1, "reset", 4]
    T = sum(c for c in calls if c != "reset")
    pcm = tiled_pcm(n, T, seed=8, distinct=97)
    pcm[2:6, ::9] = 0
    active = pattern_mask(n, T, 0.7, seed=2)
    slots = slot_map("random", n, k, seed=3)
    mb = mixed_batch(models, k, n, slots, path)
    got = masked_device_run(torch, mb, pcm, active, calls)
    out, vad, gains = got
    absent = active == 0
    assert (out[absent].view(np.uint32) == SENTINEL.view(np.uint32)).all(), "an absent row of out was written"
    assert not vad[absent].any() and not gains[absent].any(), "an absent frame has vad / gains"
    assert not (vad.view(np.uint32) == SENTINEL.view(np.uint32)).any(), "a vad row was not written"
    assert not (gains.view(np.uint32) == SENTINEL.view(np.uint32)).any(), "a gains row was not written"

    def run_single(m):
        sb = single_batch(m, n, path)
        return sb, masked_device_run(torch, sb, pcm, active, calls)

    compare_with_singles(models, mb, got, slots, run_single, what=f"masked, path {path}")
    mb.close()


@pytest.mark.parametrize("io", ["host", "s16", "16k"])
def test_host_fed_int16_and_16k(models, io):
    n, k, calls = 1000, 2, [6, 1, 3]
    pcm = tiled_pcm(n, sum(calls), seed=10, distinct=97)
    fn = "process"
    if io == "s16":
        pcm = np.clip(np.rint(pcm), -32768, 32767).astype(np.int16)
        fn = "process_s16"
    elif io == "16k":
        pcm = np.ascontiguousarray(pcm[:, :, :160])
    slots = slot_map("interleaved", n, k)

    def prep(b):
        if io == "16k":
            b.set_pcm_rate(16000)
        return b

    mb = prep(mixed_batch(models, k, n, slots))
    got = run_calls(mb, pcm, calls, fn)

    def run_single(m):
        sb = prep(single_batch(m, n))
        return sb, run_calls(sb, pcm, calls, fn)

    compare_with_singles(models, mb, got, slots, run_single, what=io)
    mb.close()


def test_slots_added_but_unused_change_nothing(models):
    n, calls = 700, [3, 1, 2]
    pcm = tiled_pcm(n, sum(calls), seed=12, distinct=97)
    mb = mixed_batch(models, 4, n, np.zeros(n, np.uint8))
    plain = capi.Batch(models[0], n)
    got, want = run_calls(mb, pcm, calls), run_calls(plain, pcm, calls)
    for name, a, w in zip(("out", "vad", "gains"), got, want):
        assert_bits_equal(a, w, name)
    for s in (0, 350, n - 1):
        assert_bits_equal(mb.export_state(s), plain.export_state(s), f"state {s}")
    mb.close()
    plain.close()


def test_device_map_entry_naming_no_slot_runs_as_slot_0(models):
    torch = pytest.importorskip("torch")
    n, k, T = 300, 3, 4
    pcm = tiled_pcm(n, T, seed=13, distinct=97)
    raw = np.ascontiguousarray(np.array([0, 1, 2, 3, 9, 255], np.uint8)[np.arange(n) % 6])
    eff = np.where(raw < k, raw, 0).astype(np.uint8)
    mb = mixed_batch(models, k, n, np.zeros(n, np.uint8))
    d_map = torch.from_numpy(raw).cuda()
    mb.set_stream_models_device(d_map.data_ptr())
    torch.cuda.synchronize()
    assert (mb.stream_models() == raw).all()  # (the map holds what was copied; the kernels read entries >= k as slot 0)
    got = mb.process(pcm)
    ref = mixed_batch(models, k, n, eff)
    want = ref.process(pcm)
    for name, a, w in zip(("out", "vad", "gains"), got, want):
        assert_bits_equal(a, w, name)
    mb.close()
    ref.close()


def test_slot_table_and_host_map_errors(models):
    L = capi.lib()
    n = 40
    b = capi.Batch(models[0], n)
    assert (b.stream_models() == 0).all()
    assert L.rnnoise_batch_add_model(b.h, None) == -1
    for i in range(1, capi.MAX_MODELS):
        assert b.add_model(models[i % len(models)]) == i
    assert L.rnnoise_batch_add_model(b.h, models[0].h) == -1  # the ninth
    with pytest.raises(RuntimeError):
        b.add_model(models[1])
    m = slot_map("random", n, capi.MAX_MODELS, seed=1)
    b.set_stream_models(m)
    bad = m.copy()
    bad[17] = capi.MAX_MODELS
    assert L.rnnoise_batch_set_stream_models(b.h, bad.ctypes.data_as(C.POINTER(C.c_ubyte))) == -1
    with pytest.raises(ValueError):
        b.set_stream_models(bad)
    assert (b.stream_models() == m).all()
    b.close()


def test_torch_op_with_extra_models(blobs):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, T = 96, 6
    pcm = tiled_pcm(n, T, seed=14, distinct=48)
    op = RNNoiseOp(blobs[0], n, extra_models=(blobs[1],))
    slots = slot_map("interleaved", n, 2)
    op.set_stream_models(torch.from_numpy(slots).cuda())
    out, vad, gains = op(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    for s in (0, 1, n - 1):
        want = Oracle(blobs[slots[s]]).run(pcm[:, s])
        assert_bits_equal(out[:, s].cpu().numpy(), want["out"], f"stream {s} out")
        assert_bits_equal(vad[:, s].cpu().numpy(), want["vad"], f"stream {s} vad")
    op.close()


@pytest.mark.parametrize("env", [dict(RNNOISE_AMD_TILE_WAVES="16", RNNOISE_AMD_GRU_VARIANT="w4"),
                                 dict(RNNOISE_AMD_TILE_WAVES="8", RNNOISE_AMD_GRU_VARIANT="w8")], ids=["t16-w4", "t8-w8"])
def test_forced_forms(env):
    """the tile kernel's other form in each kind of call ($RNNOISE_AMD_TILE_WAVES) and both GRU layer forms ($RNNOISE_AMD_GRU_VARIANT),
    read once per process: the mixed-batch cases of paths 1 and 2 rerun in a child process"""
    if os.environ.get("RNNOISE_AMD_TILE_WAVES"):
        pytest.skip("already inside a forced run")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", __file__, "-k",
                        "test_every_network_form and (p1-n1000 or p2-n1000) or test_masked_calls_silence_and_reset"],
                       env=dict(os.environ, **env), capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
