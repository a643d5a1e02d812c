"""Linked gains on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_gain_link): every test compares the batch with the link oracle
(tests/csrc/link_oracle.c: rno_link_group_frame) bit for bit -- out, vad, gains, the exported state and, with controls, the gate
counters -- over 12 frames in calls of 5 + 1 + 6, so the pipelined and the one-frame paths both run.  Both synthesis kernel forms (few:
up to 256 rows; wide: 264), K = 2, 3 and 8; masks with an absent sibling and silent frames; a list call over non-adjacent streams;
controls with a gate; mixed rates and G.711 formats, two model slots, interleaved int16 under a layout and the staged host forms inside
one group; K = 1 after K = 2 and groups of identical rows against the unlinked batch; the setter on a live batch; the torch op; the CLI.
The rows of a group carry different signals, and every oracle run first shows on its own numbers that the link bites.
At these sizes the dispatch plan picks rn_nn_one_kernel, the one-wave high-pass and the one-stream analysis kernel throughout; every
other form of every stage under a link -- with controls, two model slots, masks and group-wise list calls on the mixed stream block --
runs in tests/test_gpu_at_size.py (test_stream_mix_linked_at_every_form, test_stream_mix_linked_masked_and_listed_at_every_form)."""
import functools

import numpy as np
import pytest

from conftest import assert_bits_equal, load_blob
from ctl_oracle import CtlOracle
from link_oracle import LinkGroup
from rnnoise_amd import capi, g711, resample, synth, wav
from test_masked_gpu import s16_of

pytestmark = pytest.mark.gpu
CALLS = (5, 1, 6)
T = sum(CALLS)
SENT = np.float32(123.0)  # what `out` holds before a call


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def blob():
    return load_blob("default")


@pytest.fixture(scope="module")
def model(blob):
    return capi.Model(blob)


@functools.lru_cache(maxsize=None)
def _signals(n):
    pcm = synth.batch_pcm(range(3, 3 + n), T)  # a different synthetic voice per row
    pcm[:2, 1::5] = 0                          # rows 1, 6, 11, ... start with two silent frames
    return pcm


def signals(n):
    """(T, n, 480) float32: a copy of the shared signals"""
    return _signals(n).copy()


class Want:
    """the link oracle's run of some groups of a call: rows (T, R, 480) taken K at a time; groups: which (default all);
    blobs: one blob, or one per row; ctl (R, 3) or None; active (T, R) or None"""

    def __init__(self, blobs, K, pcm, groups=None, ctl=None, active=None, bites=True):
        R = pcm.shape[1]
        assert R % K == 0
        self.K, self.groups = K, list(range(R // K)) if groups is None else list(groups)
        blobs = [blobs] * R if isinstance(blobs, (bytes, bytearray)) else blobs
        self.g, self.r = {}, {}
        for j in self.groups:
            rows = slice(K * j, K * j + K)
            self.g[j] = LinkGroup(blobs[rows], K, None if ctl is None else ctl[rows])
            self.r[j] = self.g[j].run(pcm[:, rows], None if active is None else active[:, rows])
            if bites:
                self.assert_bites(j)

    def assert_bites(self, j):
        """on the oracle's numbers alone: in at least half of the group's non-silent frames the linked gain differs from some
        participant's own in some band -- else the comparison could pass with the branch never taken"""
        r = self.r[j]
        live = [t for t in range(T) if r["n"][t] > 0]
        hit = [t for t in live if any((r["g_link"][t].view(np.uint32) != r["gains"][t, k].view(np.uint32)).any()
                                      for k in range(self.K) if r["silence"][t, k] == 0)]
        assert live and 2 * len(hit) >= len(live), f"group {j}: the link bites in {len(hit)} of {len(live)} frames"

    def rows(self):
        return [self.K * j + k for j in self.groups for k in range(self.K)]

    def check(self, got, what="", s16=False, active=None):
        """got = (out, vad, gains), each (T, R, ...): every row of the checked groups, every frame it has"""
        out, vad, gains = got
        for j in self.groups:
            r = self.r[j]
            for k in range(self.K):
                i = self.K * j + k
                for t in range(T):
                    tag = f"{what} row {i} frame {t}"
                    if not r["present"][t, k]:
                        continue
                    assert_bits_equal(out[t, i], s16_of(r["out"][t, k]) if s16 else r["out"][t, k], tag + " out")
                    assert_bits_equal(vad[t, i], r["vad"][t, k], tag + " vad")
                    assert_bits_equal(gains[t, i], r["gains"][t, k], tag + " gains")

    def check_state(self, b, streams=None, what="", gate=False):
        """the complete state (and the gate counter) of every checked row's stream; streams: the stream of every row of the call"""
        rows = self.rows()
        st = rows if streams is None else [int(streams[i]) for i in rows]
        snap = b.save_streams(st)
        for x, i in enumerate(rows):
            j, k = divmod(i, self.K)
            assert_bits_equal(snap[x, :capi.STATE_FLOATS], self.g[j].state[k], f"{what} state of row {i}")
            if gate:
                assert int(snap[x, capi.SNAP_OFF_GATE:capi.SNAP_OFF_GATE + 1].view(np.int32)[0]) == int(self.g[j].c[k]), \
                    f"{what} gate counter of row {i}"


def device_run(torch, b, pcm, active=None, streams=None, s16=False, sent=SENT):
    """device calls of 5 + 1 + 6 frames on one non-default HIP stream, no host synchronisation between them; streams: a list call"""
    R = pcm.shape[1]
    st = torch.cuda.Stream()
    h = st.cuda_stream
    d_in = torch.from_numpy(np.ascontiguousarray(pcm)).cuda()
    d_out = torch.full_like(d_in, int(sent) if s16 else float(sent))
    d_vad = torch.zeros((T, R), device="cuda")
    d_gains = torch.zeros((T, R, capi.NB_BANDS), device="cuda")
    d_act = torch.from_numpy(np.ascontiguousarray(active, np.uint8)).cuda() if active is not None else None
    d_list = torch.from_numpy(np.ascontiguousarray(streams, np.int32)).cuda() if streams is not None else None
    torch.cuda.synchronize()
    t = 0
    for c in CALLS:
        a = d_act[t:].data_ptr() if d_act is not None else 0
        if d_list is not None:
            b.process_list_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(),
                                  d_list.data_ptr(), R, a, c, h, s16=s16)
        elif d_act is not None:
            b.process_masked_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(), a, c, h,
                                    s16=s16)
        else:
            b.process_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(), c, h, s16=s16)
        t += c
    st.synchronize()
    return d_out.cpu().numpy(), d_vad.cpu().numpy(), d_gains.cpu().numpy()


def host_run(b, pcm, s16=False):
    res, t = [], 0
    for c in CALLS:
        res.append((b.process_s16 if s16 else b.process)(pcm[t:t + c]))
        t += c
    return tuple(np.concatenate([r[k] for r in res]) for k in range(3))


# ---- 1. both kernel forms, K = 2, 3, 8 ----
SIZES = [(4, 2), (6, 3), (16, 8), (264, 2), (264, 3), (264, 8)]


@pytest.mark.parametrize("n,K", SIZES, ids=[f"n{n}-k{K}" for n, K in SIZES])
def test_link_follows_the_oracle(torch, model, blob, n, K):
    pcm = signals(n)
    G = n // K
    # at 264 streams (the wide form; the few form serves up to 256 rows): the first groups, the groups at row 256 and the last ones
    groups = None if n <= 16 else sorted({0, 1, G // 2, 255 // K, 256 // K, G - 2, G - 1})
    want = Want(blob, K, pcm, groups)
    b = capi.Batch(model, n)
    assert b.gain_link == 1 and b.set_gain_link(K) == 1 and b.gain_link == K
    got = device_run(torch, b, pcm)
    want.check(got, f"n {n} K {K}")
    want.check_state(b, what=f"n {n} K {K}")
    b.close()


# ---- 2. a mask with an absent sibling, silent frames ----
@pytest.mark.parametrize("n", [6, 264])
def test_masked_call_absent_and_silent_rows(torch, model, blob, n):
    K = 3
    pcm = signals(n).copy()
    pcm[4:7, 5] = 0  # (frames of zeros in mid-stream: not silent by the reference's rule -- the high-pass rings on -- but distinct input)
    active = np.ones((T, n), np.uint8)
    active[:, 0] = 0        # group 0: row 0 absent throughout; row 1 starts silent, so frames 0 and 1 have ONE participant
    active[3:8, 4] = 0      # group 1: row 4 absent in frames 3 .. 7
    active[0, 3] = 0
    active[-1, 5] = 0
    want = Want(blob, K, pcm, sorted({0, 1, n // K - 1}), active=active)
    r0 = want.r[0]
    assert (r0["silence"][:2, 1] == 1).all() and (r0["n"][:2] == 1).all() and (r0["n"][2:] == 2).all()
    b = capi.Batch(model, n)
    b.set_gain_link(K)
    got = device_run(torch, b, pcm, active=active)
    want.check(got, "masked")
    want.check_state(b, what="masked")
    assert (got[0][:, 0] == SENT).all() and (got[0][3:8, 4] == SENT).all()  # an absent row's `out` is not written
    assert not b.export_state(0).any()                                      # nor its state
    b.close()


# ---- 3. a list call: groups of non-adjacent streams ----
def test_list_call(torch, model, blob):
    n, K = 12, 3
    streams = np.array([10, 1, 7, 4, 11, 2], np.int32)
    pcm = signals(6)
    want = Want(blob, K, pcm)
    b = capi.Batch(model, n)
    b.set_gain_link(K)
    got = device_run(torch, b, pcm, streams=streams)
    want.check(got, "list")
    want.check_state(b, streams, "list")
    for s in sorted(set(range(n)) - set(streams.tolist())):
        assert not b.export_state(s).any(), f"stream {s} is not listed"
    # rows that fill no whole groups: refused with nothing launched, on the device and on the host path
    before = b.save_streams()
    d = torch.zeros((1, 5, 480), device="cuda")
    idx = torch.from_numpy(streams[:5].copy()).cuda()
    with pytest.raises(RuntimeError):
        b.process_list_device(d.data_ptr(), d.data_ptr(), 0, 0, idx.data_ptr(), 5, 0, 1, 0)
    with pytest.raises(ValueError):
        b.process_list(np.zeros((1, 4, 480), np.float32), streams[:4])
    torch.cuda.synchronize()
    assert_bits_equal(b.save_streams(), before, "after the refused calls")
    b.close()


# ---- 4. controls with a gate ----
def gate_pcm():
    """group 0 = rows 0, 1: a voice and a steady noise; group 1 = rows 2, 3: the same the other way round"""
    v = signals(4)
    rng = np.random.default_rng(5)
    noise = (rng.standard_normal((2, T, 480)) * 300).astype(np.float32)
    return np.ascontiguousarray(np.stack([v[:, 0], noise[0], noise[1], v[:, 2]], axis=1))


@pytest.mark.parametrize("n", [4, 264])
def test_gate_opens_and_closes_with_the_group(torch, model, blob, n):
    K = 2
    pcm = signals(n).copy()
    pcm[:, :4] = gate_pcm()
    ctl = np.zeros((n, 3), np.float32)
    ctl[0] = ctl[1] = (0.1, 0.7, 0)                   # equal thr and hold: the rows open and close together
    ctl[2], ctl[3] = (0.0, 0.8, 0), (0.25, 0.6, 3)    # different thr and hold: each row on its own, from the group's VAD
    if n > 4:
        ctl[4:] = capi.controls_table(n - 4, 20.0, 0.7, 1)
    groups = [0, 1] if n == 4 else [0, 1, 2, n // K - 1]
    want = Want(blob, K, pcm, groups, ctl=ctl)
    # on the oracle's numbers: alone, the noise row has frames below the threshold while the voice is above it; linked, its counter is
    # the voice row's on every frame
    r = want.r[0]
    alone = (r["vad"][:, 1] < 0.7) & (r["vad"][:, 0] >= 0.7)
    assert alone.sum() >= 3 and (r["vad_link"] == np.maximum(r["vad"][:, 0], r["vad"][:, 1])).all()
    chk, solo = LinkGroup(blob, K, ctl[:2]), CtlOracle(blob)
    apart = 0
    for t in range(T):
        chk.process(pcm[t, :2])
        solo.process(pcm[t, 1], ctl[1])
        assert chk.c[0] == chk.c[1], f"frame {t}: the rows of group 0 share thr and hold"
        apart += int(solo.c > 0 and chk.c[1] == 0)  # closed alone, open with the group
    assert apart >= 3
    b = capi.Batch(model, n)
    b.set_stream_controls(ctl)
    b.set_gain_link(K)
    got = device_run(torch, b, pcm)
    want.check(got, "gate")
    want.check_state(b, what="gate", gate=True)
    b.close()


# ---- 5. combinations inside one group ----
def test_two_model_slots_in_one_group(torch, model, blob):
    n, K = 4, 2
    little_blob = load_blob("little")
    little = capi.Model(little_blob)
    slots = np.array([0, 1, 1, 0], np.uint8)
    pcm = signals(n)
    want = Want([little_blob if s else blob for s in slots], K, pcm)
    b = capi.Batch(model, n)
    assert b.add_model(little) == 1
    b.set_stream_models(slots)
    b.set_gain_link(K)
    got = device_run(torch, b, pcm)
    want.check(got, "two models")
    want.check_state(b, what="two models")
    b.close()


def test_mixed_rates_and_g711_in_one_group(model, blob):
    """a 48 kHz batch with a rate table and a format table, int16 host calls (the staged path): each row at its own rate and in its
    own format; the oracle sees the expanded, upsampled frames and its output goes down and is compressed the same way"""
    n, K = 4, 2
    hz = [48000, 16000, 8000, 48000]
    fmt = ["s16", "ulaw", "alaw", "s16"]
    Ls = [48000 // h for h in hz]
    hi = signals(n)
    rows = np.full((T, n, 480), 7777, np.int16)
    seen = np.zeros((T, n, 480), np.float32)  # what the oracle gets: every row's frames at 48 kHz
    for s in range(n):
        L, M, f = Ls[s], 480 // Ls[s], g711.code(fmt[s])
        x = hi[:, s]
        if L > 1:
            dn = resample.Down(L)
            x = np.stack([dn(hi[t, s]) for t in range(T)])
        x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
        if f:
            codes = g711.encode(x, f)
            rows[:, s].view(np.uint8).reshape(T, 960)[:, :M] = codes
            x = g711.decode(codes, f)
        else:
            rows[:, s, :M] = x
        up = resample.Up(L) if L > 1 else None
        seen[:, s] = np.stack([up(x[t].astype(np.float32)) if up else x[t].astype(np.float32) for t in range(T)])
    want = Want(blob, K, seen)
    b = capi.Batch(model, n)
    b.set_stream_rates(hz)
    b.set_stream_formats(fmt)
    b.set_gain_link(K)
    res, t = [], 0
    for c in CALLS:
        o = np.full((c, n, 480), -32768, np.int16)
        res.append(b.process_s16(rows[t:t + c], out=o))
        t += c
    out, vad, gains = (np.concatenate([r[k] for r in res]) for k in range(3))
    for s in range(n):
        j, k = divmod(s, K)
        L, M, f = Ls[s], 480 // Ls[s], g711.code(fmt[s])
        dn = resample.Down(L) if L > 1 else None
        for t in range(T):
            o = want.r[j]["out"][t, k]
            o = resample.to_s16(dn(o)) if dn else s16_of(o)
            tag = f"stream {s} ({hz[s]} Hz, {fmt[s]}) frame {t}"
            if f:
                got8 = out[t, s].view(np.uint8)
                assert np.array_equal(got8[:M], g711.encode(o, f)), tag + " out"
                assert np.array_equal(got8[M:], np.full(480, -32768, np.int16).view(np.uint8)[M:]), tag + " tail"
            else:
                assert np.array_equal(out[t, s, :M], o), tag + " out"
                assert (out[t, s, M:] == -32768).all(), tag + " tail"
            assert_bits_equal(vad[t, s], want.r[j]["vad"][t, k], tag + " vad")
            assert_bits_equal(gains[t, s], want.r[j]["gains"][t, k], tag + " gains")
    want.check_state(b, what="rates and formats")
    b.close()


@pytest.mark.parametrize("s16", [False, True], ids=["float", "int16"])
def test_host_forms_take_the_staged_path(model, blob, s16):
    n, K = 6, 2
    pcm = signals(n)
    want = Want(blob, K, pcm)
    b = capi.Batch(model, n)
    b.set_gain_link(K)
    got = host_run(b, pcm.astype(np.int16) if s16 else pcm, s16)  # (the signals are whole numbers in int16's range)
    want.check(got, "host", s16=s16)
    want.check_state(b, what="host")
    b.close()


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_torch_op_process_channels_link(torch, blob, dtype):
    """interleaved channels with C = K = 2 under the [G][T][C] layout of the torch op, int16 and float"""
    from rnnoise_amd.torch_op import RNNoiseOp
    G, C = 3, 2
    n = G * C
    pcm = signals(n)
    want = Want(blob, C, pcm)
    op = RNNoiseOp(blob, n)
    res, t = [], 0
    for c in CALLS:
        x = pcm[t:t + c].reshape(c, G, C, 480).transpose(1, 0, 3, 2).reshape(G, c * 480, C)  # (G, T * 480, C)
        x = torch.from_numpy(np.ascontiguousarray(x).astype(dtype)).cuda()
        o, v, g = op.process_channels(x, link=True if t == 0 else None)
        torch.cuda.synchronize()
        o = o.cpu().numpy().reshape(G, c, 480, C).transpose(1, 0, 3, 2).reshape(c, n, 480)
        res.append((o, v.cpu().numpy(), g.cpu().numpy()))
        t += c
    assert op.batch.gain_link == C and op.batch.pcm_channels == C
    got = tuple(np.concatenate([r[k] for r in res]) for k in range(3))
    want.check(got, "torch op", s16=dtype == "int16")
    want.check_state(op.batch, what="torch op")
    assert op.set_gain_link(1) == C
    op.process_channels(x, link=True)
    assert op.batch.gain_link == C
    op.process_channels(x, link=False)
    assert op.batch.gain_link == 1
    op.close()


# ---- 6. identity runs ----
@pytest.mark.parametrize("n", [4, 264])
def test_k1_after_k2_is_the_unlinked_batch(torch, model, n):
    pcm = signals(n)
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    assert b.set_gain_link(2) == 1 and b.set_gain_link(1) == 2 and b.gain_link == 1
    ga, gb = device_run(torch, a, pcm), device_run(torch, b, pcm)
    for name, x, y in zip(("out", "vad", "gains"), ga, gb):
        assert_bits_equal(y, x, name)
    assert_bits_equal(b.save_streams(), a.save_streams(), "snapshots")
    a.close()
    b.close()


@pytest.mark.parametrize("n,K", [(6, 2), (264, 8)])
def test_identical_rows_give_the_unlinked_bits(torch, model, n, K):
    pcm = np.ascontiguousarray(np.repeat(signals(n // K), K, axis=1))  # every group: K copies of one signal
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    b.set_gain_link(K)
    ga, gb = device_run(torch, a, pcm), device_run(torch, b, pcm)
    for name, x, y in zip(("out", "vad", "gains"), ga, gb):
        assert_bits_equal(y, x, name)
    assert_bits_equal(b.save_streams(), a.save_streams(), "snapshots")
    a.close()
    b.close()


# ---- 7. the setter on a live batch ----
def test_setter_on_a_live_batch(model):
    b = capi.Batch(model, 12)
    L, h = capi.lib(), b.h
    assert b.gain_link == 1
    for bad in (0, -1, 9, 5, 8):  # out of range, and no divisors of 12
        assert L.rnnoise_batch_set_gain_link(h, bad) == -1 and b.gain_link == 1
        with pytest.raises(ValueError):
            b.set_gain_link(bad)
    assert b.set_gain_link(3) == 1 and b.set_gain_link(3) == 3 and b.set_gain_link(4) == 3 and b.gain_link == 4
    assert L.rnnoise_batch_set_gain_link(h, 7) == -1 and b.gain_link == 4
    # configuration, not state
    b.reset()
    assert b.gain_link == 4
    b.set_pcm_rate(16000)
    assert b.gain_link == 4
    b.set_pcm_rate(48000)
    b.set_pcm_channels(2)
    assert b.gain_link == 4 and b.pcm_channels == 2
    b.set_pcm_channels(1)
    b.set_stream_controls(capi.controls_table(12, 12.0, 0.5, 2))
    b.reset_streams([0, 5])
    b.import_state(3, b.export_state(4))
    b.load_streams(b.save_streams())
    assert b.gain_link == 4
    assert b.set_gain_link(1) == 4
    b.close()


# ---- 8. the CLI ----
def test_cli_link_channels(tmp_path, blob):
    from rnnoise_amd import cli
    pcm = signals(3)
    st = pcm[:, :2].astype(np.int16)                                 # (T, 2, 480): two different channels
    mono = pcm[:, 2].astype(np.int16)
    d = tmp_path / "in"
    d.mkdir()
    wav.write(str(d / "st.wav"), wav.WavInfo(48000, 2, "s16", False, 0, 0), st.transpose(0, 2, 1).reshape(T * 480, 2))
    wav.write(str(d / "m.wav"), wav.WavInfo(48000, 1, "s16", False, 0, 0), mono.reshape(-1, 1))
    (tmp_path / "w.blob").write_bytes(blob)
    args = ["denoise", "--model", str(tmp_path / "w.blob"), "--chunk-frames", "5"]
    cli.main(args + ["--out-dir", str(tmp_path / "a"), "--link-channels", str(d / "st.wav"), str(d / "m.wav")])
    cli.main(args + ["--out-dir", str(tmp_path / "b"), str(d / "st.wav"), str(d / "m.wav")])
    want = Want(blob, 2, st.astype(np.float32))
    _, linked = wav.read(str(tmp_path / "a" / "st.wav.denoised.wav"))
    _, plain = wav.read(str(tmp_path / "b" / "st.wav.denoised.wav"))
    assert linked.shape == ((T - 1) * 480, 2)
    for c in range(2):  # (the first output frame is dropped, as the reference's demo drops it)
        assert np.array_equal(linked[:, c].reshape(T - 1, 480), s16_of(want.r[0]["out"][1:, c])), f"channel {c}"
    assert not np.array_equal(linked, plain)
    _, m_a = wav.read(str(tmp_path / "a" / "m.wav.denoised.wav"))
    _, m_b = wav.read(str(tmp_path / "b" / "m.wav.denoised.wav"))
    assert np.array_equal(m_a, m_b) and m_a.any()  # a mono input is unaffected
