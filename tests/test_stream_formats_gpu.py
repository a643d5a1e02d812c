"""Per-stream G.711 on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats): mu-law / A-law bytes in and out of the int16
calls.  The oracle of every test is the int16 path itself, which the rest of the suite pins to the reference: batch A carries a format
table and is fed bytes, batch B carries none and is fed g711.decode of the same bytes.  A's vad, gains and snapshots must equal B's,
A's output bytes must equal g711.encode of B's int16 output, the tail of every companded row of `out` must keep the sentinel written
there, and every linear stream must equal its twin in every bit of its row.  All comparisons are exact.

Signals: rnnoise_amd.synth streams scaled by 8, 2 and 0.5 (stream index mod 3) and clipped to int16.  At 8 the input is clipped hard
(peaks of 48,000 before the clip) and the int16 output of the table-less batch reaches +-16,384 and beyond, i.e. segment 7 of both laws
with both signs (found with the CPU oracle: a gain of 4 stops at +-12,700, 5.3 reaches segment 7 on some streams only, 6 and 8 on
every stream tried); the conditions are asserted on B in every run of the equivalence test."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import assert_bits_equal
from rnnoise_amd import capi, g711, resample, synth

pytestmark = pytest.mark.gpu
SENT = np.int16(-32768)  # what `out` holds before a call
JUNK16, JUNK8 = np.int16(7777), np.uint8(0xA5)  # what the unread part of an `in` row holds
LS4 = np.array([1, 2, 3, 6])
DISTINCT = 12
GAINS = (8.0, 2.0, 0.5)
CALLS = (4, 1, 3, 3)  # lock-step pipelined, one frame, masked, list
T_ALL = sum(CALLS)
ALL16 = sorted((s, n) for s in range(8) for n in (False, True))


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


@pytest.fixture(scope="module")
def base():
    """{L: (T_ALL, DISTINCT, 480 / L) int16}: the scaled synth streams at every rate"""
    hi = np.stack([np.clip(synth.stream_pcm(3 + 11 * d, T_ALL).astype(np.float64) * GAINS[d % 3], -32768, 32767).reshape(T_ALL, 480)
                   for d in range(DISTINCT)], axis=1).astype(np.float32)
    out = {1: hi.astype(np.int16)}
    for L in (2, 3, 6):
        dn = resample.Down(L, (DISTINCT,))
        out[L] = np.clip(np.round(np.stack([dn(hi[t]) for t in range(T_ALL)])), -32768, 32767).astype(np.int16)
    return out


def layout(n, Lb, mixed):
    """(divisor, format) of every stream: neighbours differ in both, and all twelve pairs occur in every run of twelve streams"""
    s = np.arange(n)
    Ls = LS4[s % 4] if mixed else np.full(n, Lb)
    return Ls, ((s + s // 4) % 3).astype(np.uint8)


class Pair:
    """batch A (format table, bytes) and batch B (no table, decoded int16) with everything else alike"""

    def __init__(self, model, n, Lb=1, mixed=False, dressed=False, extra_model=None, fmts=None):
        self.n, self.Lb, self.F = n, Lb, 480 // Lb
        self.Ls, self.fmts = layout(n, Lb, mixed)
        if fmts is not None:
            self.fmts = np.asarray(fmts, np.uint8)
        self.M = 480 // self.Ls
        self.A, self.B = capi.Batch(model, n), capi.Batch(model, n)
        for b in (self.A, self.B):
            if Lb != 1:
                b.set_pcm_rate(48000 // Lb)
            if mixed:
                b.set_stream_rates(48000 // self.Ls)
            if dressed:
                assert b.add_model(extra_model) == 1
                b.set_stream_models((np.arange(n) // 3) % 2)
                s = np.arange(n)
                # a floor on the odd streams, a gate with a hold on the streams of the middle gain (the loudest ones stay open)
                b.set_stream_controls(capi.controls_table(n, np.where(s % 2, 12.0, np.inf), np.where(s % 3 == 1, 0.3, 0.0),
                                                          np.where(s % 3 == 1, 4, 0)))
        self.A.set_stream_formats(self.fmts)
        assert_bits_equal(self.A.stream_formats(), self.fmts, "stream_formats")
        assert not self.B.stream_formats().any()

    def close(self):
        self.A.close()
        self.B.close()

    def rows(self, base, sl, streams=None, cover=()):
        """the call's `in` buffers (frames, rows, F) int16 for A and for B; streams: the stream of every row (default: its own);
        cover: streams whose first 256 input bytes of the slice are a permutation of all 256 codes"""
        streams = np.arange(self.n) if streams is None else np.asarray(streams)
        k = sl.stop - sl.start
        a = np.full((k, len(streams), self.F), JUNK16, np.int16)
        b = a.copy()
        a8 = a.view(np.uint8).reshape(k, len(streams), 2 * self.F)
        for i, s in enumerate(streams):
            M, f = int(self.M[s]), int(self.fmts[s])
            x = base[int(self.Ls[s])][sl, s % DISTINCT]
            if not f:
                a[:, i, :M] = b[:, i, :M] = x
                continue
            codes = g711.encode(x, f)
            if s in cover:
                codes.reshape(-1)[:256] = np.random.Generator(np.random.PCG64(int(s))).permutation(256).astype(np.uint8)
            a8[:, i, :] = JUNK8
            a8[:, i, :M] = codes
            b[:, i, :M] = g711.decode(codes, f)
        return a, b

    def expect_a(self, out_b, present=None, streams=None):
        """A's `out` from B's: encode() of the present frames of the companded rows, the sentinel behind them, linear rows as they are"""
        streams = np.arange(self.n) if streams is None else np.asarray(streams)
        e = out_b.copy()
        e8 = e.view(np.uint8).reshape(e.shape[0], e.shape[1], 2 * self.F)
        for i, s in enumerate(streams):
            M, f = int(self.M[s]), int(self.fmts[s])
            if not f:
                continue
            assert (out_b[:, i, M:] == SENT).all(), f"B wrote behind the frame of stream {s}"
            e[:, i, :] = SENT
            for t in range(e.shape[0]):
                if present is None or present[t, i]:
                    e8[t, i, :M] = g711.encode(out_b[t, i, :M], f)
        return e


def dev_call(torch, b, pcm, form="lock", active=None, streams=None):
    """one device call on int16 rows; `out` pre-filled with the sentinel -> (out, vad, gains) as numpy"""
    dev = torch.device("cuda", 0)
    k, r = pcm.shape[:2]
    d_in = torch.from_numpy(np.ascontiguousarray(pcm)).to(dev)
    d_out = torch.full_like(d_in, int(SENT))
    d_vad, d_g = torch.empty((k, r), device=dev), torch.empty((k, r, 32), device=dev)
    d_act = torch.from_numpy(np.ascontiguousarray(active, np.uint8)).to(dev) if active is not None else None
    torch.cuda.synchronize()
    if form == "lock":
        b.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), k, 0, s16=True)
    elif form == "masked":
        b.process_masked_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), d_act.data_ptr(), k, 0, s16=True)
    else:
        d_list = torch.from_numpy(np.ascontiguousarray(streams, np.int32)).to(dev)
        b.process_list_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr(), d_g.data_ptr(), d_list.data_ptr(), r,
                              d_act.data_ptr() if d_act is not None else 0, k, 0, s16=True)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_vad.cpu().numpy(), d_g.cpu().numpy()


def both(torch, p, base, sl, what, form="lock", active=None, streams=None, cover=(), seen=None):
    """the same call on A and B, A checked against B; returns B's (out, vad, gains)"""
    a_in, b_in = p.rows(base, sl, streams, cover)
    oa, va, ga = dev_call(torch, p.A, a_in, form, active, streams)
    ob, vb, gb = dev_call(torch, p.B, b_in, form, active, streams)
    assert_bits_equal(va, vb, what + ": vad")
    assert_bits_equal(ga, gb, what + ": gains")
    assert_bits_equal(oa, p.expect_a(ob, active, streams), what + ": out (bytes of the companded rows, sentinel behind them, linear rows)")
    if seen is not None:  # B's encoded output per law: the segments and signs it reaches
        rows = np.arange(p.n) if streams is None else np.asarray(streams)
        for i, s in enumerate(rows):
            f = int(p.fmts[s])
            if f:
                keep = np.ones(ob.shape[0], bool) if active is None else np.asarray(active)[:, i] != 0
                seg, neg = g711.segment(g711.encode(ob[keep, i, :int(p.M[s])], f), f)
                seen[f].update(zip(seg.ravel().tolist(), neg.ravel().tolist()))
    return ob, vb, gb


# ---- 1. equivalence: every call form, every rate, every K0 / K3 regime of the table-less plan ----
# shapes: "48k" a 48 kHz batch WITHOUT a rate table -- the one shape whose plan the format table changes: at 2,600 streams the
# table-less batch B runs rn_hp_kernel (lane = stream, which knows no formats) and A must be forced to rn_hp_one_kernel, and every
# companded stream goes through the in-place reader (hp_one_body) and the body's byte stores; "8k" a uniform 8 kHz batch and "mixed"
# a 48 kHz batch with a rate table (both low-rate plans: the prologue / epilogue paths, rs_up_stream and rs_down_stream).
# sizes: RN_K3_FEW | mid | above K0's and K1's switches; the dressed batch (two model slots, a control table) at the two ends
def cover_streams(p):
    """per law, the first stream at the lowest rate and the first at the highest: all 256 codes go through rs_up_stream (L > 1) and
    through hp_one_body's dword loads (L = 1) wherever the shape has both"""
    return tuple(sorted({int(np.flatnonzero((p.fmts == f) & (p.Ls == L))[0]) for f in (1, 2) for L in (p.Ls.max(), p.Ls.min())}))


@pytest.mark.parametrize("n,shape", [(n, s) for s in ("48k", "8k", "mixed") for n in (96, 1200, 2600)] + [(96, "mixed-dressed"), (2600, "mixed-dressed")])
def test_a_format_table_is_decode_then_the_int16_call_then_encode(torch, model, blob_little, base, n, shape):
    extra = capi.Model(blob_little) if shape == "mixed-dressed" else None
    p = Pair(model, n, Lb=6 if shape == "8k" else 1, mixed=shape.startswith("mixed"), dressed=extra is not None, extra_model=extra)
    rng = np.random.Generator(np.random.PCG64(n))
    cover = cover_streams(p)
    assert len(cover) == (4 if shape.startswith("mixed") else 2)
    seen = {1: set(), 2: set()}
    tag = f"{shape} n={n}"
    _, v1, _ = both(torch, p, base, slice(0, 4), tag + " lock-step 4 frames", cover=cover, seen=seen)
    _, v2, _ = both(torch, p, base, slice(4, 5), tag + " one frame", seen=seen)
    act = rng.random((3, n)) < 0.6
    both(torch, p, base, slice(5, 8), tag + " masked", "masked", act, seen=seen)
    lst = rng.permutation(n)[:n // 2 + 1]
    both(torch, p, base, slice(8, 11), tag + " list", "list", rng.random((3, len(lst))) < 0.7, lst, seen=seen)
    both(torch, p, base, slice(8, 9), tag + " lock-step after the list call", seen=seen)
    assert_bits_equal(p.A.save_streams(), p.B.save_streams(), tag + ": snapshots of every stream")
    # the conditions that keep the comparison honest, on the reference side
    assert (np.concatenate([v1, v2]) > 0).any(axis=0).all(), tag + ": a stream of B never had a frame with vad > 0"
    for f in (1, 2):
        assert sorted(seen[f]) == ALL16, (tag, g711.NAMES[f], "segments / signs B's output misses", sorted(set(ALL16) - seen[f]))
    p.close()
    if extra is not None:
        extra.close()


def test_decode_coverage_streams_hold_all_256_codes(base):
    """the inputs of the equivalence test: the two cover streams' first call carries every code of their law (a check of the test's
    own construction, on the host)"""
    class Stub(Pair):
        def __init__(self, Lb, mixed):
            self.n, self.Lb, self.F = 24, Lb, 480 // Lb
            self.Ls, self.fmts = layout(24, Lb, mixed)
            self.M = 480 // self.Ls
    for Lb, mixed in ((6, False), (1, False), (1, True)):
        p = Stub(Lb, mixed)
        cover = cover_streams(p)
        assert {int(p.fmts[s]) for s in cover} == {1, 2} and {int(p.Ls[s]) for s in cover} == {int(p.Ls.min()), int(p.Ls.max())}
        a, b = p.rows(base, slice(0, 4), cover=cover)
        for s in cover:
            M = int(p.M[s])
            codes = a.view(np.uint8).reshape(4, 24, 2 * p.F)[:, s, :M]
            assert len(set(codes.ravel().tolist())) == 256
            assert_bits_equal(b[:, s, :M], g711.decode(codes, int(p.fmts[s])), "B is fed the decoded bytes")


# ---- 2. isolation: a linear stream between two companded ones ----
@pytest.mark.parametrize("n", [3, 2600])
def test_a_linear_stream_between_companded_ones_keeps_every_bit(torch, model, base, n):
    fmts = np.array([1, 0, 2] * (n // 3 + 1), np.uint8)[:n]
    p = Pair(model, n, fmts=fmts)
    plain = capi.Batch(model, n)
    lin = np.flatnonzero(fmts == 0)
    for sl in (slice(0, 3), slice(3, 4)):
        a_in, b_in = p.rows(base, sl)
        oa, va, ga = dev_call(torch, p.A, a_in)
        op, vp, gp = dev_call(torch, plain, b_in)
        assert_bits_equal(oa[:, lin], op[:, lin], f"n={n} {sl}: the linear streams' whole rows")
        assert_bits_equal(va[:, lin], vp[:, lin], "vad")
        assert_bits_equal(ga[:, lin], gp[:, lin], "gains")
        # ... and their companded neighbours are what the table-less batch gives for the decoded bytes (at 2,600 streams that batch
        # runs the lane = stream K0: the forced form is what keeps these equal)
        assert_bits_equal(oa, p.expect_a(op), f"n={n} {sl}: every row, the companded ones as bytes")
        assert_bits_equal(va, vp, "vad of every stream")
        assert_bits_equal(ga, gp, "gains of every stream")
    assert_bits_equal(p.A.save_streams(lin), plain.save_streams(lin), "snapshots of the linear streams")
    plain.close()
    p.close()


# ---- 3. the table's semantics ----
def test_table_semantics(torch, model, base):
    n = 70
    p = Pair(model, n, Lb=6)
    L = capi.lib()
    up = C.POINTER(C.c_ubyte)
    # the host setter refuses a 3: -1, nothing changed
    for bad in (3, 4, 255):
        t = p.fmts.copy()
        t[5] = bad
        assert L.rnnoise_batch_set_stream_formats(p.A.h, t.ctypes.data_as(up)) == -1, bad
    assert_bits_equal(p.A.stream_formats(), p.fmts, "table after the refusals")
    assert L.rnnoise_batch_set_stream_formats_device(p.A.h, None, None) == -1
    assert L.rnnoise_batch_stream_formats(p.A.h, None) == -1
    both(torch, p, base, slice(0, 2), "after the refusals")
    # the table survives reset, reset_streams, set_pcm_rate, set_stream_rates and load_streams
    snap = p.A.save_streams()
    for b in (p.A, p.B):
        b.reset()
        b.reset_streams([0, 1, 2])
        b.set_pcm_rate(16000)
        b.set_pcm_rate(8000)
        b.set_stream_rates(np.full(n, 8000))
        b.set_stream_rates(None)
        b.load_streams(snap)
        b.set_nn_path(b.set_nn_path(2))
    assert_bits_equal(p.A.stream_formats(), p.fmts, "table after reset / rate changes / load")
    both(torch, p, base, slice(2, 5), "after reset / rate changes / load")
    # the device setter takes anything; a byte that names no law runs the stream as linear
    wild = p.fmts.copy()
    wild[1::7] = 3
    wild[2::7] = 200
    d = torch.from_numpy(wild).to("cuda:0")
    p.A.set_stream_formats_device(d.data_ptr(), 0)
    seen_as = np.where(wild > 2, 0, wild).astype(np.uint8)
    assert_bits_equal(p.A.stream_formats(), seen_as, "getter reads the table as the kernels do")
    p.fmts = seen_as
    both(torch, p, base, slice(5, 7), "device setter with bytes that name no law")
    # float calls ignore the table: the float bits of a batch without one
    x = base[6][7:9][:, np.arange(n) % DISTINCT].astype(np.float32)
    fa, fb = p.A.process(x), p.B.process(x)
    for a, b, what in zip(fa, fb, ("out", "vad", "gains")):
        assert_bits_equal(a, b, "float call with a table: " + what)
    # NULL drops the table: the next call is a table-less batch's
    p.A.set_stream_formats(None)
    assert not p.A.stream_formats().any()
    p.fmts = np.zeros(n, np.uint8)
    a_in, b_in = p.rows(base, slice(9, 11))
    assert_bits_equal(a_in, b_in, "no companded stream left")
    for a, b, what in zip(dev_call(torch, p.A, a_in), dev_call(torch, p.B, b_in), ("out", "vad", "gains")):
        assert_bits_equal(a, b, "after dropping the table: " + what)
    assert_bits_equal(p.A.save_streams(), p.B.save_streams(), "snapshots at the end")
    p.close()


# ---- 4. a slot recycled for a leg of another codec (the serving snippet of INTEGRATION.md) ----
def test_a_recycled_slot_equals_a_fresh_stream_of_the_new_codec(torch, model, base):
    n, slot = 40, 17
    Ls, fmts = layout(n, 1, True)
    p = Pair(model, n, mixed=True)
    both(torch, p, base, slice(0, 3), "before the slot is recycled")
    newL, newf = (6, 2) if (int(Ls[slot]), int(fmts[slot])) != (6, 2) else (3, 1)
    Ls2, fmts2 = Ls.copy(), fmts.copy()
    Ls2[slot], fmts2[slot] = newL, newf
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_r, d_f = torch.from_numpy(Ls2.astype(np.uint8)).to("cuda:0"), torch.from_numpy(fmts2).to("cuda:0")
        d_i = torch.tensor([slot], dtype=torch.int32, device="cuda:0")
        h = st.cuda_stream
        p.A.set_stream_rates_device(d_r.data_ptr(), h)
        p.A.set_stream_formats_device(d_f.data_ptr(), h)
        p.A.reset_streams_device(d_i.data_ptr(), 1, h)
    st.synchronize()
    p.B.set_stream_rates_device(d_r.data_ptr(), 0)
    p.B.reset_streams([slot])
    p.Ls, p.fmts, p.M = Ls2, fmts2, 480 // Ls2
    assert_bits_equal(p.A.stream_formats(), fmts2, "formats after the device setter")
    # a fresh one-stream batch of the new codec, fed the slot's frames
    fresh = capi.Batch(model, 1)
    fresh.set_stream_rates([48000 // newL])
    for sl in (slice(3, 6), slice(6, 7)):
        ob, vb, gb = both(torch, p, base, sl, f"after the slot is recycled {sl}")  # no other stream moves: A == B in every row
        _, b_in = p.rows(base, sl)
        of, vf, gf = dev_call(torch, fresh, np.ascontiguousarray(b_in[:, slot:slot + 1]))
        assert_bits_equal(ob[:, slot], of[:, 0], "the recycled slot = a fresh stream: out")
        assert_bits_equal(vb[:, slot], vf[:, 0], "vad")
        assert_bits_equal(gb[:, slot], gf[:, 0], "gains")
    fresh.close()
    p.close()


# ---- 5. the host forms against the device forms ----
def test_host_forms_equal_the_device_forms(torch, model, base):
    n = 50
    host, dev = Pair(model, n, mixed=True), Pair(model, n, mixed=True)
    rng = np.random.Generator(np.random.PCG64(5))
    vad, gains = np.empty((2, n), np.float32), np.empty((2, n, 32), np.float32)
    # rnnoise_batch_process_s16
    a_in, _ = host.rows(base, slice(0, 2))
    out = np.full_like(a_in, SENT)
    host.A.process_into(out.ctypes.data, a_in.ctypes.data, vad.ctypes.data, gains.ctypes.data, 2, s16=True)
    for a, b, what in zip((out, vad, gains), dev_call(torch, dev.A, a_in), ("out", "vad", "gains")):
        assert_bits_equal(a, b, "process_s16 host = device: " + what)
    # rnnoise_batch_process_masked_s16
    a_in, _ = host.rows(base, slice(2, 4))
    act = rng.random((2, n)) < 0.6
    got = host.A.process_masked_s16(a_in, act, out=np.full_like(a_in, SENT))
    for a, b, what in zip(got, dev_call(torch, dev.A, a_in, "masked", act), ("out", "vad", "gains")):
        assert_bits_equal(a, b, "process_masked_s16 host = device: " + what)
    # rnnoise_batch_process_list_s16
    lst = rng.permutation(n)[:20]
    a_in, _ = host.rows(base, slice(4, 6), lst)
    act = rng.random((2, 20)) < 0.7
    got = host.A.process_list_s16(a_in, lst, act, out=np.full_like(a_in, SENT))
    for a, b, what in zip(got, dev_call(torch, dev.A, a_in, "list", act, lst), ("out", "vad", "gains")):
        assert_bits_equal(a, b, "process_list_s16 host = device: " + what)
    assert_bits_equal(host.A.save_streams(), dev.A.save_streams(), "snapshots")
    host.close()
    dev.close()


# ---- 6. the torch op and the CLI ----
def test_torch_op_sets_the_table_on_the_current_stream(torch, blob_default, base):
    from rnnoise_amd.torch_op import RNNoiseOp
    n = 12
    op, ref = RNNoiseOp(blob_default, n), RNNoiseOp(blob_default, n)
    fmts = layout(n, 1, False)[1]
    op.set_stream_formats(torch.from_numpy(fmts).to("cuda:0"))
    assert_bits_equal(op.batch.stream_formats(), fmts, "the op's table")
    p = Pair.__new__(Pair)
    p.n, p.Lb, p.F, p.Ls, p.fmts, p.M, p.A, p.B = n, 1, 480, np.ones(n, int), fmts, np.full(n, 480), op.batch, ref.batch
    both(torch, p, base, slice(0, 3), "int16 device calls on the op's batch")
    # the op's own float calls ignore the table
    x = torch.from_numpy(base[1][3:5][:, np.arange(n) % DISTINCT].astype(np.float32)).to("cuda:0")
    for a, b, what in zip(op(x), ref(x), ("out", "vad", "gains")):
        assert_bits_equal(a.cpu().numpy(), b.cpu().numpy(), "the op's float call with a table: " + what)
    op.close()
    ref.close()


def test_cli_reads_and_writes_companded_files(blob_default, base, tmp_path):
    from rnnoise_amd import cli
    T = 8
    x = base[6][:T, 0].reshape(-1)
    codes = g711.ulaw_encode(x)
    lin = base[1][:T, 1].reshape(-1)
    (tmp_path / "a.ul").write_bytes(codes.tobytes())
    (tmp_path / "a.raw").write_bytes(g711.ulaw_decode(codes).tobytes())
    (tmp_path / "b.raw").write_bytes(lin.tobytes())
    ins_a = [str(tmp_path / "a.ul"), str(tmp_path / "b.raw")]
    ins_b = [str(tmp_path / "a.raw"), str(tmp_path / "b.raw")]
    assert cli.denoise_files(blob_default, ins_a, str(tmp_path / "A"), chunk_frames=3, rates=[8000, 48000], formats=["ulaw", "s16"]) == [T, T]
    assert cli.denoise_files(blob_default, ins_b, str(tmp_path / "B"), chunk_frames=3, rates=[8000, 48000]) == [T, T]
    got = np.frombuffer((tmp_path / "A" / "a.ul.denoised.raw").read_bytes(), np.uint8)
    want = np.frombuffer((tmp_path / "B" / "a.raw.denoised.raw").read_bytes(), np.int16)
    assert got.size == want.size == (T - 1) * 80
    assert_bits_equal(got, g711.ulaw_encode(want), "the .ul file out = encode of the s16 run on the decoded file")
    assert (tmp_path / "A" / "b.raw.denoised.raw").read_bytes() == (tmp_path / "B" / "b.raw.denoised.raw").read_bytes()
    with pytest.raises(ValueError):
        cli.denoise_files(blob_default, ins_a, str(tmp_path / "C"), formats=["ulaw"])
    assert os.path.getsize(tmp_path / "A" / "a.ul.denoised.raw") * 2 == os.path.getsize(tmp_path / "B" / "a.raw.denoised.raw")
