"""Chunk calls on the GPU (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks): any number of samples per stream and call.
The yardstick is not the code under test.  A few lines of numpy deques (Fifos) do the bookkeeping -- which samples form which frame,
and when --, and the arithmetic comes from the masked calls, which the suite holds to the oracle: a second batch runs process_masked
on the frames and the mask the model assembles.  The 48 kHz float configuration is compared with the CPU oracle directly as well.
Everything is bit for bit."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from oracle.binding import Oracle
from rnnoise_amd import capi, synth

pytestmark = pytest.mark.gpu
SENT_F, SENT_S = np.float32(-12345.5), np.int16(-21846)
SPECIAL = [0, 1, 479, 480, 481, 960, 1024]


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


def cast_s16(v):
    """the library's float -> int16 of its int16 calls: truncation to 32 bits (0x80000000 out of range or NaN), then the low 16"""
    v = np.asarray(v, np.float32)
    ok = (v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))
    q = np.where(ok, np.trunc(np.where(ok, v, 0)), -2147483648.0).astype(np.int64)
    return (q & 0xFFFF).astype(np.uint16).view(np.int16)


class Fifos:
    """the semantics of the issue, per stream: pending input, and an output FIFO that starts as M zeros"""

    def __init__(self, n, M):
        self.n, self.M = n, M
        self.inq = [np.zeros(0, np.float32) for _ in range(n)]
        self.outq = [np.zeros(M, np.float32) for _ in range(n)]

    def restart(self, streams):
        for s in streams:
            self.inq[s], self.outq[s] = np.zeros(0, np.float32), np.zeros(self.M, np.float32)

    def push(self, rows, counts, F):
        """-> the frames (F, n, M) and the mask (F, n) of the masked call this push amounts to, and k per stream"""
        M = self.M
        frames, mask, k = np.zeros((F, self.n, M), np.float32), np.zeros((F, self.n), np.uint8), np.zeros(self.n, np.int32)
        for s in range(self.n):
            cat = np.concatenate([self.inq[s], rows[s, :counts[s]].astype(np.float32)])
            k[s] = len(cat) // M
            frames[:k[s], s] = cat[:k[s] * M].reshape(k[s], M)
            mask[:k[s], s] = 1
            self.inq[s] = cat[k[s] * M:]
        return frames, mask, k

    def pop(self, ref_out, k, counts):
        want = []
        for s in range(self.n):
            q = np.concatenate([self.outq[s], ref_out[:k[s], s].reshape(-1)])
            assert len(q) >= counts[s]
            want.append(q[:counts[s]])
            self.outq[s] = q[counts[s]:]
        return want

    def fill(self):
        return np.array([len(q) for q in self.inq], np.int32)


def host_call(b, s16):
    def call(rows, counts, out):
        return (b.process_chunks_s16 if s16 else b.process_chunks)(rows, counts, out=out)
    return call


def one_push(call, ref, fifos, rows, counts, max_count, s16, what, given=None, b=None):
    """one push through `call` (the chunk call under test) and through the model + the masked reference batch; every output compared.
    given: the counts as handed to the call where they differ from what they mean (device counts out of range); b: the batch under
    test, for its fills after the push"""
    n, M = fifos.n, fifos.M
    F = capi.chunk_frames(M, max_count)
    out = np.full((n, max_count), SENT_S if s16 else SENT_F)
    got_out, vad, gains, frames = call(rows, counts if given is None else given, out)
    x, mask, k = fifos.push(rows, counts, F)
    sent = np.full_like(x, SENT_F)
    r_out, r_vad, r_gains = ref.process_masked(x, mask, out=sent)
    want = fifos.pop(r_out, k, counts)
    assert_bits_equal(frames, k, f"{what} frames")
    for s in range(n):
        w = cast_s16(want[s]) if s16 else want[s]
        assert_bits_equal(got_out[s, :counts[s]], w, f"{what} stream {s} out")
        rest = got_out[s, counts[s]:]
        assert (rest.view(np.uint16 if s16 else np.uint32) == (SENT_S.view(np.uint16) if s16 else SENT_F.view(np.uint32))).all(), \
            f"{what} stream {s}: samples behind its count were written"
    assert_bits_equal(vad, r_vad, f"{what} vad")
    assert_bits_equal(gains, r_gains, f"{what} gains")
    for s in range(n):
        assert not vad[k[s]:, s].any() and not gains[k[s]:, s].any(), f"{what} stream {s}: rows beyond its frames"
    if b is not None:
        assert_bits_equal(b.chunk_fill(), fifos.fill(), f"{what} chunk_fill")
    return got_out, r_out, k, vad, gains


def samples(streams, total, int16=False):
    """(n, total) samples from rnnoise_amd.synth, one generator stream per row"""
    T = -(-total // synth.FRAME)
    x = np.stack([synth.stream_pcm(s, T)[:total] for s in streams])
    return x if int16 else x.astype(np.float32)


def core_counts(n, pushes, max_count, seed):
    """every stream sees each of SPECIAL at least once (a Latin arrangement over the first pushes), then counts from the seed"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, max_count + 1, (pushes, n)).astype(np.int32)
    for p in range(len(SPECIAL)):
        for s in range(n):
            c[p, s] = SPECIAL[(s + p) % len(SPECIAL)]
    return c


def run_plan(call, ref, fifos, x, counts, max_count, s16, what, at=None, b=None, side=None):
    """the pushes of `counts` (pushes, n) over the sample rows x; -> per stream everything returned, and the reference's frames;
    with `side` (a list), per stream the vad and gains rows of its completed frames are appended to it as (stream, vad, gains)"""
    n = fifos.n
    at = np.zeros(n, np.int64) if at is None else at
    y, z = [[] for _ in range(n)], [[] for _ in range(n)]
    for p, c in enumerate(counts):
        rows = np.full((n, max_count), 999, x.dtype)  # (the tails of `in`: any value)
        for s in range(n):
            rows[s, :c[s]] = x[s, at[s]:at[s] + c[s]]
            at[s] += c[s]
        out, r_out, k, vad, gains = one_push(call, ref, fifos, rows, c, max_count, s16, f"{what} push {p}", b=b)
        for s in range(n):
            y[s].append(out[s, :c[s]])
            z[s].append(r_out[:k[s], s].reshape(-1))
            if side is not None:
                side.append((s, vad[:k[s], s], gains[:k[s], s]))
    return [np.concatenate(v) for v in y], [np.concatenate(v) for v in z]


def check_end(b, ref, fifos, what, streams=None):
    assert_bits_equal(b.chunk_fill(), fifos.fill(), f"{what} chunk_fill")
    for s in (range(fifos.n) if streams is None else streams):
        assert_bits_equal(b.export_state(s), ref.export_state(s), f"{what} state of stream {s}")


def test_core_float_against_the_masked_reference_and_the_oracle(model, blob_default):
    """7 streams, 48 kHz, 14 pushes of up to 1024 samples, every stream seeing 0, 1, 479, 480, 481, 960 and 1024"""
    n, M, max_count = 7, 480, 1024
    counts = core_counts(n, 14, max_count, seed=7)
    for s in range(n):
        assert set(SPECIAL) <= set(counts[:, s].tolist())
    x = samples(range(10, 10 + n), int(counts.sum(0).max()))
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    assert not b.chunk_fill().any()
    side = []
    y, z = run_plan(host_call(b, False), ref, fifos, x, counts, max_count, False, "core", b=b, side=side)
    check_end(b, ref, fifos, "core")
    for s in range(n):
        # the concatenated output: M zeros, then what the lock-step call returns for the input cut into frames
        assert_bits_equal(y[s], np.concatenate([np.zeros(M, np.float32), z[s]])[:len(y[s])], f"core stream {s}: y = 0^M ++ z")
        T = len(z[s]) // M
        want = Oracle(blob_default).run(x[s, :T * M].reshape(T, M))
        assert_bits_equal(z[s].reshape(T, M), want["out"], f"core stream {s}: the reference against the oracle")
        assert_bits_equal(y[s][M:], want["out"].reshape(-1)[:len(y[s]) - M], f"core stream {s}: the chunk output against the oracle")
        assert_bits_equal(np.concatenate([v for i, v, _ in side if i == s]), want["vad"], f"core stream {s}: vad against the oracle")
        assert_bits_equal(np.concatenate([g for i, _, g in side if i == s]), want["gains"], f"core stream {s}: gains against the oracle")


def test_core_int16_is_the_float_run_followed_by_the_cast(model):
    n, M, max_count = 5, 480, 1024
    counts = core_counts(n, 14, max_count, seed=8)
    x = samples(range(20, 20 + n), int(counts.sum(0).max()), int16=True)
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    y, z = run_plan(host_call(b, True), ref, fifos, x, counts, max_count, True, "int16", b=b)
    check_end(b, ref, fifos, "int16")
    for s in range(n):
        assert_bits_equal(y[s], cast_s16(np.concatenate([np.zeros(M, np.float32), z[s]])[:len(y[s])]), f"int16 stream {s}")


@pytest.mark.parametrize("hz,max_count", [(8000, 128), (16000, 441), (32000, 1023)])
@pytest.mark.parametrize("s16", [False, True])
def test_rates(model, hz, max_count, s16):
    n, M = 5, 480 * hz // 48000
    rng = np.random.default_rng(hz)
    counts = rng.integers(0, max_count + 1, (8, n)).astype(np.int32)
    counts[0, 0], counts[1, 0], counts[2, 1], counts[3, 2] = max_count, 0, M, M - 1
    x = samples(range(30, 30 + n), int(counts.sum(0).max()), int16=s16)
    b, ref = capi.Batch(model, n), capi.Batch(model, n)
    b.set_pcm_rate(hz)
    ref.set_pcm_rate(hz)
    fifos = Fifos(n, M)
    run_plan(host_call(b, s16), ref, fifos, x, counts, max_count, s16, f"{hz} Hz")
    check_end(b, ref, fifos, f"{hz} Hz")


def test_small_pushes_return_from_the_output_fifo(model):
    """12 pushes of exactly 128 at 48 kHz: F is 1 and most pushes complete no frame"""
    n, M, max_count = 3, 480, 128
    assert capi.chunk_frames(M, max_count) == 1
    counts = np.full((12, n), 128, np.int32)
    x = samples(range(40, 40 + n), 12 * 128)
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    y, z = run_plan(host_call(b, False), ref, fifos, x, counts, max_count, False, "small")
    check_end(b, ref, fifos, "small")
    assert len(z[0]) == 3 * M and len(y[0]) == 12 * 128  # (three frames completed; every push returned its 128)
    assert y[0][M:].any()


def device_call(b, torch, s16, alias=False, stream=None, poison_in=None):
    """the device form through torch buffers.  alias: `in` is `out`.  The rows' tails of `in` are overwritten with poison_in"""
    def call(rows, counts, out):
        n, max_count = rows.shape
        F = capi.chunk_frames(b.frame, max_count)
        rows = rows.copy()
        if poison_in is not None:
            for s in range(n):
                rows[s, max(0, min(int(counts[s]), max_count)):] = poison_in
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
        with ctx:
            d_in = torch.from_numpy(rows).cuda()
            if alias:  # the tails must read as the caller's `out` afterwards: they are the input's own
                d_out = d_in
            else:
                d_out = torch.from_numpy(out).cuda()
            d_counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
            d_vad = torch.full((F, n), 7.0, device="cuda")
            d_gains = torch.full((F, n, 32), 7.0, device="cuda")
            d_frames = torch.full((n,), -1, device="cuda", dtype=torch.int32)
            b.process_chunks_device(d_out.data_ptr(), d_in.data_ptr(), d_counts.data_ptr(), max_count, d_vad.data_ptr(),
                                    d_gains.data_ptr(), d_frames.data_ptr(), torch.cuda.current_stream().cuda_stream, s16=s16)
        torch.cuda.synchronize()
        res = d_out.cpu().numpy()
        if alias:  # (compare the tails against the sentinel the checker expects: they kept the input's bytes)
            for s in range(n):
                c = max(0, min(int(counts[s]), max_count))
                assert_bits_equal(res[s, c:], rows[s, c:], f"alias: tail of row {s}")
                res[s, c:] = out[s, c:]
        return res, d_vad.cpu().numpy(), d_gains.cpu().numpy(), d_frames.cpu().numpy()
    return call


@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("form", ["plain", "alias", "stream"])
def test_untouched_bytes_aliasing_and_a_stream_of_the_callers(model, s16, form):
    """`out` poisoned, `in` poisoned beyond the counts: the samples of out[s] beyond counts[s] keep the caller's bytes and the result
    does not depend on the tails of `in`; the same with `in` aliasing `out`, and on a non-default HIP stream"""
    torch = pytest.importorskip("torch")
    n, M, max_count = 4, 480, 601
    rng = np.random.default_rng(5)
    counts = rng.integers(0, max_count + 1, (6, n)).astype(np.int32)
    counts[0], counts[1, 0], counts[2, 1] = [0, 1, 600, 601], 601, 0
    x = samples(range(50, 50 + n), int(counts.sum(0).max()), int16=s16)
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    st = torch.cuda.Stream() if form == "stream" else None
    call = device_call(b, torch, s16, alias=form == "alias", stream=st, poison_in=31000 if s16 else np.float32(np.nan))
    run_plan(call, ref, fifos, x, counts, max_count, s16, form)
    check_end(b, ref, fifos, form)


def test_device_counts_out_of_range_and_the_host_forms_refusal(model):
    torch = pytest.importorskip("torch")
    n, M, max_count = 4, 480, 500
    x = samples(range(60, 60 + n), 4 * max_count)
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    call = device_call(b, torch, False)
    at = np.zeros(n, np.int64)
    for p, (given, means) in enumerate([([200, -3, max_count + 5, 77], [200, 0, max_count, 77]),
                                        ([-1, 300, 2**31 - 1, -2**31], [0, 300, max_count, 0])]):
        rows = np.zeros((n, max_count), np.float32)
        for s in range(n):
            rows[s, :means[s]] = x[s, at[s]:at[s] + means[s]]
            at[s] += means[s]
        one_push(call, ref, fifos, rows, np.array(means, np.int32), max_count, False, f"clamped push {p}", given=np.array(given, np.int32))
    check_end(b, ref, fifos, "clamped")
    # the host form checks first: -1, fills and states as they were
    fill, snap = b.chunk_fill(), b.save_streams()
    for bad in ([10, 10, -1, 10], [10, max_count + 1, 10, 10]):
        with pytest.raises(ValueError):
            b.process_chunks(np.zeros((n, max_count), np.float32), bad)
    assert_bits_equal(b.chunk_fill(), fill, "fills after a refused host call")
    assert_bits_equal(b.save_streams(), snap, "states after a refused host call")


def test_restarts(model):
    n, M, max_count = 6, 480, 700
    rng = np.random.default_rng(9)
    x = samples(range(70, 70 + n), 40 * max_count)
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    at = np.zeros(n, np.int64)
    call = host_call(b, False)

    def some_pushes(what):
        counts = rng.integers(1, max_count + 1, (1, n)).astype(np.int32)
        run_plan(call, ref, fifos, x, counts, max_count, False, what, at=at)
        # ... and one that leaves every stream 100 + 37 s samples pending, so that a restart has something to drop
        last = (np.array([100 + 37 * s for s in range(n)]) - fifos.fill()) % M
        run_plan(call, ref, fifos, x, np.where(last == 0, M, last).astype(np.int32)[None], max_count, False, what + " (last)", at=at)
        assert_bits_equal(fifos.fill(), np.array([100 + 37 * s for s in range(n)], np.int32), "the plan")
        check_end(b, ref, fifos, what)

    some_pushes("before any restart")
    b.reset_streams([1, 4])  # exactly their FIFOs
    ref.reset_streams([1, 4])
    fifos.restart([1, 4])
    assert_bits_equal(b.chunk_fill(), fifos.fill(), "fills after reset_streams")
    some_pushes("after reset_streams")
    b.load_streams(b.save_streams([2, 5]), [2, 5])  # the same states back: only the FIFOs of 2 and 5 restart
    fifos.restart([2, 5])
    assert_bits_equal(b.chunk_fill(), fifos.fill(), "fills after load_streams")
    some_pushes("after load_streams")
    b.import_state(3, b.export_state(3))
    fifos.restart([3])
    assert_bits_equal(b.chunk_fill(), fifos.fill(), "fills after import_state")
    some_pushes("after import_state")
    assert b.set_pcm_rate(48000) == 48000  # every FIFO; the states stay
    fifos.restart(range(n))
    assert not b.chunk_fill().any()
    some_pushes("after set_pcm_rate")
    b.reset()
    ref.reset()
    fifos.restart(range(n))
    assert not b.chunk_fill().any()
    some_pushes("after reset")


def test_model_slots_and_a_gate_ride_through(model, blob_little):
    n, M, max_count = 6, 480, 1024
    little = capi.Model(blob_little)
    slots = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    ctl = capi.controls_table(n, limit_db=[0, 6, 12, 20, 6, 0], vad_threshold=[0.0, 0.6, 0.9, 0.5, 0.0, 0.99], hold_frames=[0, 1, 0, 2, 0, 1])
    b, ref = capi.Batch(model, n), capi.Batch(model, n)
    for q in (b, ref):
        assert q.add_model(little) == 1
        q.set_stream_models(slots)
        q.set_stream_controls(ctl)
    fifos = Fifos(n, M)
    counts = core_counts(n, 10, max_count, seed=11)
    x = samples(range(80, 80 + n), int(counts.sum(0).max()))
    run_plan(host_call(b, False), ref, fifos, x, counts, max_count, False, "slots + gate")
    check_end(b, ref, fifos, "slots + gate")


def test_refusals_change_nothing(model):
    torch = pytest.importorskip("torch")
    n, M, max_count = 4, 480, 300
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    x = samples(range(90, 90 + n), 8 * max_count)
    at = np.zeros(n, np.int64)
    counts = np.array([[300, 250, 200, 7], [300, 1, 299, 150]], np.int32)
    run_plan(host_call(b, False), ref, fifos, x, counts, max_count, False, "before", at=at)
    fill, snap = b.chunk_fill(), b.save_streams()
    assert fill.any()
    rows = np.ones((n, max_count), np.float32)
    d_rows, d_counts = torch.ones((n, max_count), device="cuda"), torch.full((n,), 5, device="cuda", dtype=torch.int32)
    configs = [("a rate table", lambda: b.set_stream_rates(np.full(n, 48000)), lambda: b.set_stream_rates(None)),
               ("a format table", lambda: b.set_stream_formats(np.zeros(n, np.uint8)), lambda: b.set_stream_formats(None)),
               ("a PCM layout", lambda: b.set_pcm_layout(M, 4 * M), lambda: b.set_pcm_layout(0, 0)),
               ("two channels", lambda: b.set_pcm_channels(2), lambda: b.set_pcm_channels(1)),
               ("a link of two", lambda: b.set_gain_link(2), lambda: b.set_gain_link(1))]
    for what, on, off in configs:
        on()
        for s16 in (False, True):
            with pytest.raises(ValueError):
                (b.process_chunks_s16 if s16 else b.process_chunks)(rows.astype(np.int16) if s16 else rows, [5, 5, 5, 5])
            with pytest.raises(RuntimeError):  # (the float rows are large enough for either sample type)
                b.process_chunks_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), max_count, s16=s16)
        off()
        assert_bits_equal(b.chunk_fill(), fill, f"fills after a call refused for {what}")
        assert_bits_equal(b.save_streams(), snap, f"states after a call refused for {what}")
    # ... and the batch goes on where it was
    run_plan(host_call(b, False), ref, fifos, x, counts[::-1], max_count, False, "after", at=at)
    check_end(b, ref, fifos, "after the refusals")


def test_beyond_one_k0_form(model):
    """4,099 streams, 3 pushes of up to 600 samples: the lane = stream high-pass and the four-stream analysis forms, a ragged tile"""
    n, M, max_count, distinct = 4099, 480, 600, 61
    rng = np.random.default_rng(13)
    counts = rng.integers(0, max_count + 1, (3, n)).astype(np.int32)
    counts[:, 0], counts[:, 1], counts[:, n - 1] = [600, 600, 600], [0, 480, 0], [479, 1, 600]
    base = samples(range(100, 100 + distinct), 3 * max_count)
    x = base[np.arange(n) % distinct]
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    run_plan(host_call(b, False), ref, fifos, x, counts, max_count, False, "4099")
    check_end(b, ref, fifos, "4099", streams=[0, 1, 2, 2047, 2048, 4095, 4096, 4098])


@pytest.mark.parametrize("s16", [False, True])
def test_torch_op(blob_default, model, s16):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, M, max_count = 4, 480, 777
    F = capi.chunk_frames(M, max_count)
    op = RNNoiseOp(blob_default, n)
    b = capi.Batch(model, n)
    b.set_nn_path(1)  # (the op's default path; every path gives the same bits)
    rng = np.random.default_rng(17)
    x = samples(range(110, 110 + n), 4 * max_count, int16=s16)
    at = np.zeros(n, np.int64)
    for p in range(4):
        c = rng.integers(0, max_count + 1, n).astype(np.int32)
        rows = np.zeros((n, max_count), x.dtype)
        for s in range(n):
            rows[s, :c[s]] = x[s, at[s]:at[s] + c[s]]
            at[s] += c[s]
        out, vad, gains, frames = op.process_chunks(torch.from_numpy(rows).cuda(), torch.from_numpy(c).cuda())
        torch.cuda.synchronize()
        w_out, w_vad, w_gains, w_frames = (b.process_chunks_s16 if s16 else b.process_chunks)(rows, c)
        assert_bits_equal(out.cpu().numpy(), w_out, f"torch push {p} out")
        assert_bits_equal(vad.cpu().numpy(), w_vad, f"torch push {p} vad")
        assert_bits_equal(gains.cpu().numpy(), w_gains, f"torch push {p} gains")
        assert_bits_equal(frames.cpu().numpy(), w_frames, f"torch push {p} frames")
        assert int(op.state.item()) == (p + 1) * F
    with torch._subclasses.fake_tensor.FakeTensorMode():
        fo, fv, fg, ff = torch.ops.rnnoise_amd.process_chunks(
            torch.empty((n, max_count), device="cuda", dtype=torch.int16 if s16 else torch.float32),
            torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), op.handle)
        assert fo.shape == (n, max_count) and fo.dtype == (torch.int16 if s16 else torch.float32)
        assert fv.shape == (F, n) and fg.shape == (F, n, 32) and ff.shape == (n,) and ff.dtype == torch.int32
        assert fv.dtype == torch.float32 and fg.dtype == torch.float32
    op.close()
