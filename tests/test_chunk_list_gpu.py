"""Chunk calls on a stream list and FIFO records on the GPU (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks_list,
rnnoise_batch_save_chunk_fifos).  The contract is the yardstick: a listed stream gets what the full-size chunk call gives it with a
count of 0 for every unlisted stream, and a leg moved with its snapshot and its FIFO record continues as if it had stayed.  So the
list form runs beside a twin batch that makes the full-size call, and beside the numpy deques and the masked reference batch of
tests/test_chunks_gpu.py, whose helpers this file uses through an adaptor: the list call's compact results are spread into full-size
arrays and checked by the same code.  Everything is bit for bit."""
import numpy as np
import pytest

from conftest import assert_bits_equal
from rnnoise_amd import capi
from test_chunks_gpu import SENT_F, SENT_S, SPECIAL, Fifos, check_end, run_plan, samples

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


def spread(n, idx, out, got, vad, gains, frames):
    """a list call's results by row -> full-size arrays by stream: unlisted streams keep `out`, no frames, zero vad and gains"""
    F = vad.shape[0]
    full_out, full_vad = out.copy(), np.zeros((F, n), np.float32)
    full_gains, full_frames = np.zeros((F, n, 32), np.float32), np.zeros(n, np.int32)
    full_out[idx], full_vad[:, idx], full_gains[:, idx], full_frames[idx] = got, vad, gains, frames
    return full_out, full_vad, full_gains, full_frames


def list_call(b, lists, s16, twin=None):
    """the call signature of test_chunks_gpu's helpers: push p goes through the list form with lists[p] (None: the full-size form);
    the counts of unlisted streams must be 0.  twin: a second batch that makes the full-size chunk call; every result is compared"""
    at = {"p": 0}

    def call(rows, counts, out):
        idx, counts, n = lists[at["p"]], np.asarray(counts, np.int32), rows.shape[0]
        at["p"] += 1
        if idx is None:
            res = (b.process_chunks_s16 if s16 else b.process_chunks)(rows, counts, out=out.copy())
        else:
            idx = np.asarray(idx, np.int32)
            assert not np.delete(counts, idx).any(), "the plan pushes samples into an unlisted stream"
            got = (b.process_chunks_list_s16 if s16 else b.process_chunks_list)(rows[idx], counts[idx], idx, out=out[idx].copy())
            res = spread(n, idx, out, *got)
        if twin is not None:
            want = (twin.process_chunks_s16 if s16 else twin.process_chunks)(rows, counts, out=out.copy())
            for g, w, what in zip(res, want, ("out", "vad", "gains", "frames")):
                assert_bits_equal(g, w, f"push {at['p'] - 1}: {what} against the full-size call")
        return res
    return call


def special_plan(n, sizes, max_count, seed):
    """lists of sizes[p] distinct streams in shuffled order, and counts (pushes, n) -- 0 for unlisted streams -- such that every stream
    is LISTED with each count of SPECIAL (0 among them) once; what is left over gets counts from the seed"""
    rng = np.random.default_rng(seed)
    todo = [list(np.roll(SPECIAL, s)) for s in range(n)]
    lists, counts = [], np.zeros((len(sizes), n), np.int32)
    for p, k in enumerate(sizes):
        order = sorted(range(n), key=lambda s: (-len(todo[s]), (s + p) % n))[:k]
        rng.shuffle(order)
        for s in order:
            counts[p, s] = todo[s].pop() if todo[s] else rng.integers(0, max_count + 1)
        lists.append(order)
    assert not any(todo), "the plan is too short for every special count"
    return lists, counts


def ends_equal(b, twin, what):
    assert_bits_equal(b.chunk_fill(), twin.chunk_fill(), f"{what}: chunk_fill of the two batches")
    assert_bits_equal(b.save_streams(), twin.save_streams(), f"{what}: snapshots of the two batches")
    assert_bits_equal(b.save_chunk_fifos(), twin.save_chunk_fifos(), f"{what}: FIFO records of the two batches")


@pytest.mark.parametrize("s16", [False, True])
def test_core_against_the_full_size_call_and_the_masked_reference(model, s16):
    """9 streams, 14 calls, lists of 1 to 5 rows in changing order, every stream listed with 0, 1, 479, 480, 481, 960 and 1024"""
    n, M, max_count = 9, 480, 1024
    sizes = [5, 5, 4, 5, 5, 3, 5, 5, 5, 1, 5, 5, 5, 5]
    lists, counts = special_plan(n, sizes, max_count, seed=21)
    assert len(lists) == 14 and {len(v) for v in lists} == {1, 3, 4, 5}
    x = samples(range(200, 200 + n), int(counts.sum(0).max()), int16=s16)
    b, twin, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    y, z = run_plan(list_call(b, lists, s16, twin), ref, fifos, x, counts, max_count, s16, "core", b=b)
    check_end(b, ref, fifos, "core")
    ends_equal(b, twin, "core")
    assert any(len(v) > M and v[M:].any() for v in y)  # (real output came back)


@pytest.mark.parametrize("hz,max_count", [(16000, 441), (32000, 1023)])
@pytest.mark.parametrize("s16", [False, True])
def test_rates(model, hz, max_count, s16):
    n, M = 6, 480 * hz // 48000
    rng = np.random.default_rng(hz + s16)
    lists = [list(rng.permutation(n)[:rng.integers(1, 5)]) for _ in range(8)]
    counts = np.zeros((8, n), np.int32)
    for p, idx in enumerate(lists):
        counts[p, idx] = rng.integers(0, max_count + 1, len(idx))
    counts[0, lists[0][0]], counts[1, lists[1][0]], counts[2, lists[2][0]] = max_count, M, M - 1
    x = samples(range(230, 230 + n), int(counts.sum(0).max()), int16=s16)
    b, twin, ref = capi.Batch(model, n), capi.Batch(model, n), capi.Batch(model, n)
    for q in (b, twin, ref):
        q.set_pcm_rate(hz)
    fifos = Fifos(n, M)
    run_plan(list_call(b, lists, s16, twin), ref, fifos, x, counts, max_count, s16, f"{hz} Hz", b=b)
    check_end(b, ref, fifos, f"{hz} Hz")
    ends_equal(b, twin, f"{hz} Hz")


def test_full_size_and_list_calls_interleaved_on_one_batch(model):
    """the two forms work on the same FIFOs: a stream is pushed through either from one call to the next"""
    n, M, max_count = 6, 480, 700
    rng = np.random.default_rng(31)
    lists = [None if p % 3 == 1 else list(rng.permutation(n)[:rng.integers(1, 6)]) for p in range(10)]
    counts = np.zeros((10, n), np.int32)
    for p, idx in enumerate(lists):
        sel = np.arange(n) if idx is None else idx
        counts[p, sel] = rng.integers(0, max_count + 1, len(sel))
    x = samples(range(240, 240 + n), int(counts.sum(0).max()))
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    run_plan(list_call(b, lists, False), ref, fifos, x, counts, max_count, False, "mixed forms", b=b)
    check_end(b, ref, fifos, "mixed forms")


def device_list_call(b, torch, lists, s16, alias=False, stream=None):
    """the device form through torch buffers, with the signature of test_chunks_gpu's helpers.  Every push: poison behind the counts
    in `in`, one more row whose entry is outside the batch (with samples and a count of its own), counts handed in out of range where
    they are 0 or max_count (-3 and max_count + 5).  alias: `in` is `out`"""
    at = {"p": 0}
    poison = 31000 if s16 else np.float32(np.nan)

    def call(rows, counts, out):
        p = at["p"]
        at["p"] += 1
        n, max_count = rows.shape
        idx, counts = np.asarray(lists[p], np.int32), np.asarray(counts, np.int32)
        R, F = len(idx) + 1, capi.chunk_frames(b.frame, max_count)
        gone = p % R  # the row of the entry outside the batch
        live = np.delete(np.arange(R), gone)
        d_idx = np.zeros(R, np.int32)
        d_idx[live], d_idx[gone] = idx, (n + p, -1 - p)[p & 1]
        c = np.zeros(R, np.int32)
        c[live], c[gone] = counts[idx], max_count // 2
        r_in = np.full((R, max_count), poison, rows.dtype)
        for i in range(R):
            r_in[i, :c[i]] = rows[idx[list(live).index(i)], :c[i]] if i != gone else 77
        r_out = np.full((R, max_count), SENT_S if s16 else SENT_F)
        r_out[live] = out[idx]
        given = np.where(c == 0, -3, np.where(c == max_count, max_count + 5, c)).astype(np.int32)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            d_in = torch.from_numpy(r_in).cuda()
            d_out = d_in if alias else torch.from_numpy(r_out).cuda()
            d_counts, d_list = torch.from_numpy(given).cuda(), torch.from_numpy(d_idx).cuda()
            d_vad = torch.full((F, R), 7.0, device="cuda")
            d_gains = torch.full((F, R, 32), 7.0, device="cuda")
            d_frames = torch.full((R,), -1, device="cuda", dtype=torch.int32)
            b.process_chunks_list_device(d_out.data_ptr(), d_in.data_ptr(), d_counts.data_ptr(), max_count, d_list.data_ptr(), R,
                                         d_vad.data_ptr(), d_gains.data_ptr(), d_frames.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream, s16=s16)
        torch.cuda.synchronize()
        res, frames = d_out.cpu().numpy(), d_frames.cpu().numpy()
        assert_bits_equal(res[gone], (r_in if alias else r_out)[gone], f"push {p}: the out row of an entry outside the batch")
        assert frames[gone] == 0, f"push {p}: frames of an entry outside the batch"
        if alias:  # the tails kept the input's bytes; the checker expects the caller's `out` there
            for i in live:
                assert_bits_equal(res[i, c[i]:], r_in[i, c[i]:], f"push {p}: alias: tail of row {i}")
                res[i, c[i]:] = r_out[i, c[i]:]
        return spread(n, idx, out, res[live], d_vad.cpu().numpy()[:, live], d_gains.cpu().numpy()[:, live], frames[live])
    return call


@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("form", ["plain", "alias", "stream"])
def test_device_form_on_a_callers_stream(model, s16, form):
    torch = pytest.importorskip("torch")
    n, M, max_count = 5, 480, 601
    rng = np.random.default_rng(41)
    lists = [list(rng.permutation(n)[:k]) for k in (4, 1, 3, 2, 4, 3)]
    counts = np.zeros((6, n), np.int32)
    for p, idx in enumerate(lists):
        counts[p, idx] = rng.integers(0, max_count + 1, len(idx))
    counts[0, lists[0]], counts[1, lists[1][0]], counts[2, lists[2][0]] = [0, 1, 600, 601], 601, 0
    x = samples(range(250, 250 + n), int(counts.sum(0).max()), int16=s16)
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    st = torch.cuda.Stream() if form == "stream" else None
    run_plan(device_list_call(b, torch, lists, s16, alias=form == "alias", stream=st), ref, fifos, x, counts, max_count, s16, form, b=b)
    check_end(b, ref, fifos, form)


def test_refusals_change_nothing(model):
    torch = pytest.importorskip("torch")
    n, M, max_count = 4, 480, 300
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    x = samples(range(260, 260 + n), 8 * max_count)
    at = np.zeros(n, np.int64)
    lists, counts = [[2, 0, 3], [1, 3]], np.array([[300, 0, 200, 7], [0, 250, 0, 150]], np.int32)
    run_plan(list_call(b, lists, False), ref, fifos, x, counts, max_count, False, "before", at=at)
    fill, snap, rec = b.chunk_fill(), b.save_streams(), b.save_chunk_fifos()
    assert fill.any()

    def unchanged(what):
        assert_bits_equal(b.chunk_fill(), fill, f"fills after {what}")
        assert_bits_equal(b.save_streams(), snap, f"states after {what}")
        assert_bits_equal(b.save_chunk_fifos(), rec, f"FIFO records after {what}")

    rows = np.ones((3, max_count), np.float32)
    for what, idx, c in [("a duplicate entry", [1, 2, 1], [5, 5, 5]), ("an entry above the batch", [1, n, 2], [5, 5, 5]),
                         ("a negative entry", [-1, 0, 2], [5, 5, 5]), ("a negative count", [0, 1, 2], [5, -1, 5]),
                         ("a count above max_count", [0, 1, 2], [5, 5, max_count + 1])]:
        for s16 in (False, True):
            with pytest.raises(ValueError):
                (b.process_chunks_list_s16 if s16 else b.process_chunks_list)(rows.astype(np.int16) if s16 else rows, c, idx)
        unchanged(what)
    with pytest.raises(ValueError):  # n_rows > n_streams
        b.process_chunks_list(np.ones((n + 1, max_count), np.float32), [5] * (n + 1), list(range(n)) + [0])
    unchanged("more rows than streams")
    d_rows, d_counts = torch.ones((3, max_count), device="cuda"), torch.full((3,), 5, device="cuda", dtype=torch.int32)
    d_idx = torch.tensor([0, 1, 2], device="cuda", dtype=torch.int32)
    for bad_rows in (-1, n + 1):
        with pytest.raises(RuntimeError):
            b.process_chunks_list_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), max_count, d_idx.data_ptr(), bad_rows)
    with pytest.raises(RuntimeError):  # a NULL list with rows
        b.process_chunks_list_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), max_count, 0, 3)
    with pytest.raises(RuntimeError):
        b.process_chunks_list_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), -1, d_idx.data_ptr(), 3)
    b.process_chunks_list_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), max_count, d_idx.data_ptr(), 0)  # no-ops
    b.process_chunks_list_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), 0, d_idx.data_ptr(), 3)
    torch.cuda.synchronize()
    unchanged("the device forms' refusals and no-ops")
    configs = [("a rate table", lambda: b.set_stream_rates(np.full(n, 48000)), lambda: b.set_stream_rates(None)),
               ("a format table", lambda: b.set_stream_formats(np.zeros(n, np.uint8)), lambda: b.set_stream_formats(None)),
               ("a PCM layout", lambda: b.set_pcm_layout(M, 4 * M), lambda: b.set_pcm_layout(0, 0)),
               ("two channels", lambda: b.set_pcm_channels(2), lambda: b.set_pcm_channels(1)),
               ("a link of two", lambda: b.set_gain_link(2), lambda: b.set_gain_link(1))]
    for what, on, off in configs:
        on()
        for s16 in (False, True):
            with pytest.raises(ValueError):
                (b.process_chunks_list_s16 if s16 else b.process_chunks_list)(rows.astype(np.int16) if s16 else rows, [5, 5, 5], [0, 1, 2])
            with pytest.raises(RuntimeError):  # (the float rows are large enough for either sample type)
                b.process_chunks_list_device(d_rows.data_ptr(), d_rows.data_ptr(), d_counts.data_ptr(), max_count, d_idx.data_ptr(), 3,
                                             s16=s16)
        off()
        unchanged(f"a call refused for {what}")
    # ... and the batch goes on where it was
    run_plan(list_call(b, lists[::-1], False), ref, fifos, x, counts[::-1], max_count, False, "after", at=at)
    check_end(b, ref, fifos, "after the refusals")


def test_model_slots_a_gate_and_resets_ride_through(model, blob_little):
    n, M, max_count = 6, 480, 1024
    little = capi.Model(blob_little)
    slots = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    ctl = capi.controls_table(n, limit_db=[0, 6, 12, 20, 6, 0], vad_threshold=[0.0, 0.6, 0.9, 0.5, 0.0, 0.99], hold_frames=[0, 1, 0, 2, 0, 1])
    b, twin, ref = capi.Batch(model, n), capi.Batch(model, n), capi.Batch(model, n)
    for q in (b, twin, ref):
        assert q.add_model(little) == 1
        q.set_stream_models(slots)
        q.set_stream_controls(ctl)
    fifos = Fifos(n, M)
    rng = np.random.default_rng(51)
    x = samples(range(270, 270 + n), 12 * max_count)
    at = np.zeros(n, np.int64)

    def pushes(k, what):
        lists = [list(rng.permutation(n)[:rng.integers(2, 5)]) for _ in range(k)]
        counts = np.zeros((k, n), np.int32)
        for p, idx in enumerate(lists):
            counts[p, idx] = rng.integers(1, max_count + 1, len(idx))
        run_plan(list_call(b, lists, False, twin), ref, fifos, x, counts, max_count, False, what, at=at, b=b)
        check_end(b, ref, fifos, what)

    pushes(5, "slots + gate")
    for q in (b, twin, ref):
        q.reset_streams([1, 4])
    fifos.restart([1, 4])
    assert_bits_equal(b.chunk_fill(), fifos.fill(), "fills after reset_streams")
    pushes(5, "after reset_streams")
    ends_equal(b, twin, "slots + gate")


def test_beyond_one_k0_form_and_the_shared_staging_buffer(model):
    """4,099 streams: 130 listed rows, then 3 on the same batch (the staging buffer is larger than the call needs: the mask sits at
    the call's own offset), then a full-size call (it has to grow), then a list call again"""
    n, M, max_count, distinct = 4099, 480, 600, 61
    rng = np.random.default_rng(61)
    edge = [0, n - 1, 2048, 4096]
    big = edge + [int(s) for s in rng.permutation(n) if s not in edge][:126]
    lists = [big, [4098, 7, 2047], None, [int(s) for s in big[::-1][:40]]]
    counts = np.zeros((4, n), np.int32)
    counts[0, big] = rng.integers(0, max_count + 1, 130)
    counts[0, big[:4]] = [600, 479, 481, 0]
    counts[1, lists[1]] = [600, 1, 480]
    counts[2] = rng.integers(0, max_count + 1, n)
    counts[3, lists[3]] = rng.integers(0, max_count + 1, 40)
    base = samples(range(300, 300 + distinct), 4 * max_count)
    x = base[np.arange(n) % distinct]
    b, ref, fifos = capi.Batch(model, n), capi.Batch(model, n), Fifos(n, M)
    run_plan(list_call(b, lists, False), ref, fifos, x, counts, max_count, False, "4099", b=b)
    check_end(b, ref, fifos, "4099", streams=[0, 7, 2047, 2048, 4096, 4098, int(big[5])])


def leg_blocks(stream_seed, hz, block, pushes, s16=False):
    x = samples([stream_seed], pushes * block, int16=s16)[0]
    return x.reshape(pushes, block)


@pytest.mark.parametrize("hz,block", [(48000, 1024), (16000, 441)])
def test_a_leg_moved_mid_frame_continues_as_if_it_had_stayed(model, hz, block):
    """5 pushes, then snapshot + FIFO record into another stream index of a second batch while a twin stays behind; 6 more pushes"""
    M = 480 * hz // 48000
    src, dst, lost = capi.Batch(model, 3), capi.Batch(model, 4), capi.Batch(model, 4)
    for q in (src, dst, lost):
        q.set_pcm_rate(hz)
    blocks = leg_blocks(280, hz, block, 11)
    for p in range(5):
        src.process_chunks_list(blocks[p][None], [block], [1])
    r = (5 * block) % M
    assert r != 0 and src.chunk_fill()[1] == r  # (mid-frame)
    snap, rec = src.save_streams([1]), src.save_chunk_fifos([1])
    hdr = rec.view(np.int32)[0]
    assert (hdr[capi.CHUNK_OFF_FILL], hdr[capi.CHUNK_OFF_M], hdr[capi.CHUNK_OFF_MAGIC], hdr[963]) == (r, M, capi.CHUNK_MAGIC, 0)
    assert not rec[0, r:480].view(np.uint32).any() and not rec[0, 480 + M - r:960].view(np.uint32).any()
    assert rec[0, :r].any() and rec[0, 480:480 + M - r].any()
    assert_bits_equal(src.save_chunk_fifos([1]), rec, "saving twice")
    # the move, in the documented order: the snapshot restarts the FIFOs, the FIFO record goes in behind it
    dst.load_streams(snap, [2])
    assert dst.chunk_fill()[2] == 0
    dst.load_chunk_fifos(rec, [2])
    assert dst.chunk_fill()[2] == r
    assert_bits_equal(dst.save_chunk_fifos([2]), rec, "the record, saved again on the destination")
    lost.load_streams(snap, [2])  # ... and without it
    diverged = False
    for p in range(5, 11):
        stay = src.process_chunks_list(blocks[p][None], [block], [1])
        moved = dst.process_chunks_list(blocks[p][None], [block], [2])
        for g, w, what in zip(moved, stay, ("out", "vad", "gains", "frames")):
            assert_bits_equal(g, w, f"push {p}: {what} of the moved leg")
        alone = lost.process_chunks_list(blocks[p][None], [block], [2])
        if p == 5:  # the documented loss: M zeros come out first, and the r pending samples are gone with the frame they began
            assert not alone[0][0, :M].any() and stay[0][0, :M - r].any()
            assert alone[3][0] == block // M and stay[3][0] == (r + block) // M
        diverged = diverged or alone[0].tobytes() != stay[0].tobytes()
    assert diverged, "load_streams alone lost nothing: the comparison above proves nothing"
    assert src.chunk_fill()[1] == dst.chunk_fill()[2] == (11 * block) % M != lost.chunk_fill()[2]
    assert_bits_equal(dst.save_streams([2]), src.save_streams([1]), "snapshots at the end")
    assert_bits_equal(dst.save_chunk_fifos([2]), src.save_chunk_fifos([1]), "FIFO records at the end")
    # the other streams of the destination: never touched
    fresh = capi.Batch(model, 4)
    fresh.set_pcm_rate(hz)
    assert_bits_equal(dst.save_streams([0, 1, 3]), fresh.save_streams([0, 1, 3]), "the destination's other streams")
    assert_bits_equal(dst.save_chunk_fifos([0, 1, 3]), fresh.save_chunk_fifos([0, 1, 3]), "the destination's other FIFOs")


def test_records_before_any_chunk_call_and_loads_that_touch_nothing(model):
    torch = pytest.importorskip("torch")
    n, M = 4, 480
    b = capi.Batch(model, n)
    want = np.zeros((n, capi.CHUNK_REC_FLOATS), np.int32)
    want[:, capi.CHUNK_OFF_M], want[:, capi.CHUNK_OFF_MAGIC] = M, capi.CHUNK_MAGIC
    assert_bits_equal(b.save_chunk_fifos().view(np.int32), want, "records of a batch that has made no chunk call")
    assert_bits_equal(b.save_chunk_fifos([3, 1]).view(np.int32), want[:2], "... with a list")
    x = samples(range(290, 290 + n), 700)
    b.process_chunks_list(x[[2, 0]], [700, 333], [2, 0])
    b.process_chunks(x[:, :500], [100, 200, 0, 500])
    fill, snap, rec = b.chunk_fill(), b.save_streams(), b.save_chunk_fifos()
    assert fill.tolist() == [(333 + 100) % M, 200, 700 % M, 500 % M]

    def unchanged(what):
        assert_bits_equal(b.chunk_fill(), fill, f"fills after {what}")
        assert_bits_equal(b.save_streams(), snap, f"states after {what}")
        assert_bits_equal(b.save_chunk_fifos(), rec, f"FIFO records after {what}")

    # a NaN with a payload among the samples survives the round trip as bits
    marked = rec.copy()
    marked.view(np.uint32)[1, 5] = 0x7FC12345
    b.load_chunk_fifos(marked[[1]], [3])
    assert_bits_equal(b.save_chunk_fifos([3]), marked[[1]], "a loaded record, saved again")
    assert b.chunk_fill()[3] == fill[1]
    assert_bits_equal(b.save_streams(), snap, "states after a load")
    b.load_chunk_fifos(rec)  # (the whole batch, no list)
    unchanged("loading every record back")
    # device load: rows that are no records of this frame length, and entries outside the batch
    bad = np.stack([rec[1], rec[1], rec[1], rec[1], rec[1], rec[1]]).copy()
    h = bad.view(np.int32)
    h[0, capi.CHUNK_OFF_MAGIC] = capi.SNAP_MAGIC
    h[1, capi.CHUNK_OFF_M] = 160
    h[2, capi.CHUNK_OFF_FILL] = -1
    h[3, capi.CHUNK_OFF_FILL] = M
    d_bad = torch.from_numpy(bad).cuda()
    d_idx = torch.tensor([0, 2, 3, 0, n, -1], device="cuda", dtype=torch.int32)  # (rows 4 and 5: good records, no such stream)
    b.load_chunk_fifos_device(d_bad.data_ptr(), d_idx.data_ptr(), 4, torch.cuda.current_stream().cuda_stream)
    b.load_chunk_fifos_device(d_bad[4:].data_ptr(), d_idx[4:].data_ptr(), 2, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError):  # (more rows than streams)
        b.load_chunk_fifos_device(d_bad.data_ptr(), d_idx.data_ptr(), 6, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    unchanged("a device load of bad rows")
    # device save: an entry outside the batch gets magic 0 and nothing else
    d_rec = torch.full((3, capi.CHUNK_REC_FLOATS), 7.0, device="cuda")
    b.save_chunk_fifos_device(d_rec.data_ptr(), torch.tensor([2, n + 1, 1], device="cuda", dtype=torch.int32).data_ptr(), 3,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_rec.cpu().numpy()
    assert_bits_equal(got[[0, 2]], rec[[2, 1]], "device save")
    empty = np.full(capi.CHUNK_REC_FLOATS, 7.0, np.float32)
    empty.view(np.int32)[capi.CHUNK_OFF_MAGIC] = 0
    assert_bits_equal(got[1], empty, "device save: the row of an entry outside the batch")
    # host load: every row is checked first
    for k in range(4):
        with pytest.raises(ValueError):
            b.load_chunk_fifos(np.stack([rec[2], bad[k]]), [0, 1])
    for idx in ([0, 0], [0, n], [-1, 1]):
        with pytest.raises(ValueError):
            b.load_chunk_fifos(rec[:2], idx)
    with pytest.raises(ValueError):
        b.save_chunk_fifos([0, n])
    unchanged("refused host loads")
    # a record belongs to its frame length: after a rate change it is refused
    b.set_pcm_rate(16000)
    with pytest.raises(ValueError):
        b.load_chunk_fifos(rec[[0]], [0])
    assert not b.chunk_fill().any()


@pytest.mark.parametrize("s16", [False, True])
def test_torch_op(blob_default, model, s16):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, M, max_count = 5, 480, 777
    F = capi.chunk_frames(M, max_count)
    op, b = RNNoiseOp(blob_default, n), capi.Batch(model, n)
    b.set_nn_path(1)  # (the op's default path; every path gives the same bits)
    rng = np.random.default_rng(71)
    x = samples(range(310, 310 + n), 4 * max_count, int16=s16)
    at = np.zeros(n, np.int64)
    for p in range(4):
        idx = rng.permutation(n)[:rng.integers(1, 5)].astype(np.int32)
        c = rng.integers(0, max_count + 1, len(idx)).astype(np.int32)
        rows = np.zeros((len(idx), max_count), x.dtype)
        for i, s in enumerate(idx):
            rows[i, :c[i]] = x[s, at[s]:at[s] + c[i]]
            at[s] += c[i]
        got = op.process_chunks_list(torch.from_numpy(rows).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(idx).cuda())
        torch.cuda.synchronize()
        want = (b.process_chunks_list_s16 if s16 else b.process_chunks_list)(rows, c, idx)
        for g, w, what in zip(got, want, ("out", "vad", "gains", "frames")):
            assert_bits_equal(g.cpu().numpy(), w, f"torch push {p} {what}")
        assert int(op.state.item()) == (p + 1) * F
    assert_bits_equal(op.save_chunk_fifos().cpu().numpy(), b.save_chunk_fifos(), "torch: FIFO records")
    assert_bits_equal(op.save_chunk_fifos([3, 0]).cpu().numpy(), b.save_chunk_fifos([3, 0]), "torch: FIFO records of a list")
    # a move inside the op: stream 3 -> stream 1, snapshot first, FIFO record behind it
    op.load_streams(op.save_streams([3]), [1])
    op.load_chunk_fifos(op.save_chunk_fifos([3]), [1])
    torch.cuda.synchronize()
    rec = op.save_chunk_fifos().cpu().numpy()
    assert_bits_equal(rec[1], rec[3], "torch: the moved FIFOs")
    assert_bits_equal(op.batch.chunk_fill()[[1]], b.chunk_fill()[[3]], "torch: the moved fill")
    with torch._subclasses.fake_tensor.FakeTensorMode():
        fo, fv, fg, ff = torch.ops.rnnoise_amd.process_chunks_list(
            torch.empty((3, max_count), device="cuda", dtype=torch.int16 if s16 else torch.float32),
            torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"),
            torch.zeros(1, dtype=torch.int64, device="cuda"), op.handle)
        assert fo.shape == (3, max_count) and fo.dtype == (torch.int16 if s16 else torch.float32)
        assert fv.shape == (F, 3) and fg.shape == (F, 3, 32) and ff.shape == (3,) and ff.dtype == torch.int32
    op.close()
