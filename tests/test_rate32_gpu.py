"""32 kHz PCM on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate(32000), RNNOISE_AMD_RATE_32K).  The oracle of a stream is
the chain numpy up32 -> the reference frame function -> numpy down32 (test_resample_gpu.Chain at the code of 32 kHz), computed once per
module for DISTINCT signals; every comparison is bit for bit, on out, vad, gains and the exported state.  Sizes: 5 streams, 70 (across
a 64-stream group) and 261 (K3's wide form: dispatch.h plans the few-streams form up to 256; K0 of a low-rate batch has one form)."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal, use_rcp_profile
from rnnoise_amd import capi, g711, resample, wav
from test_gpu_parity import fuzz_pcm
from test_resample_gpu import Chain, check_rows, low_pcm, tiled

pytestmark = pytest.mark.gpu
L32 = resample.RATE_32K
M32 = 320
SENTINEL = np.float32(-12345.5)
SENTINEL16 = np.int16(-32768)
JUNK = 7777.0
DISTINCT, T = 5, 6
CALLS = (1, 2, 3)  # the histories cross calls


@pytest.fixture(scope="module")
def model(blob_default):
    return capi.Model(blob_default)


def to16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def ref(blob_default):
    """{s16: (pcm (T, DISTINCT, 320), out, vad, gains, [final state])}: the chain of every distinct signal over T frames"""
    use_rcp_profile("intel")
    base = low_pcm(DISTINCT, T, L32, seed=32)
    res = {}
    for s16 in (False, True):
        pcm = to16(base) if s16 else base
        out, vad, gains = np.empty(pcm.shape, pcm.dtype), np.empty((T, DISTINCT), np.float32), np.empty((T, DISTINCT, 32), np.float32)
        states = []
        for d in range(DISTINCT):
            c = Chain(blob_default, L32)
            for t in range(T):
                y, vad[t, d], gains[t, d] = c.frame(pcm[t, d].astype(np.float32))
                out[t, d] = resample.to_s16(y) if s16 else y
            states.append(c.o.get_state())
        res[s16] = (pcm, out, vad, gains, states)
    return res


def batch32(model, n):
    b = capi.Batch(model, n)
    assert b.set_pcm_rate(32000) == 48000 and b.pcm_rate == 32000 and b.frame == M32
    return b


def run_calls(b, pcm, s16=False, calls=CALLS):
    """the host (staged) lock-step call over `calls` -> out, vad, gains of all frames"""
    res, t0 = [], 0
    for k in calls:
        res.append((b.process_s16 if s16 else b.process)(pcm[t0:t0 + k]))
        t0 += k
    return tuple(np.concatenate([r[i] for r in res]) for i in range(3))


# ---- 1. the uniform 32 kHz batch is the chain: every stream, float and int16, K3's two forms ----
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
@pytest.mark.parametrize("n", [5, 70, 261])
def test_uniform_batch_follows_the_chain(model, ref, n, s16):
    pcm, want_out, want_vad, want_gains, states = ref[s16]
    b = batch32(model, n)
    out, vad, gains = run_calls(b, tiled(pcm, n), s16)
    assert out.shape == (T, n, M32) and out.dtype == pcm.dtype
    assert_bits_equal(out, tiled(want_out, n), f"n={n}: out of every stream")
    assert_bits_equal(vad, tiled(want_vad[:, :, None], n)[:, :, 0], f"n={n}: vad")
    assert_bits_equal(gains, tiled(want_gains, n), f"n={n}: gains")
    for s in sorted({0, 1, n // 2, n - 1}):
        assert_bits_equal(b.export_state(s), states[s % DISTINCT], f"n={n}: state of stream {s}")
    b.close()


def test_device_calls_equal_the_host_staged_calls(model, ref):
    torch = pytest.importorskip("torch")
    n = 70
    dev = torch.device("cuda", 0)
    for s16 in (False, True):
        pcm = tiled(ref[s16][0], n)
        b = batch32(model, n)
        d_in = torch.from_numpy(pcm).to(dev)
        d_out, d_vad, d_g = torch.empty_like(d_in), torch.empty((T, n), device=dev), torch.empty((T, n, 32), device=dev)
        torch.cuda.synchronize()
        t0, it = 0, pcm.itemsize
        for k in CALLS:
            b.process_device(d_out.data_ptr() + t0 * n * M32 * it, d_in.data_ptr() + t0 * n * M32 * it, d_vad.data_ptr() + t0 * n * 4,
                             d_g.data_ptr() + t0 * n * 32 * 4, k, 0, s16=s16)
            t0 += k
        torch.cuda.synchronize()
        assert_bits_equal(d_out.cpu().numpy(), tiled(ref[s16][1], n), f"s16={s16}: device out")
        assert_bits_equal(d_vad.cpu().numpy(), tiled(ref[s16][2][:, :, None], n)[:, :, 0], f"s16={s16}: device vad")
        assert_bits_equal(d_g.cpu().numpy(), tiled(ref[s16][3], n), f"s16={s16}: device gains")
        b.close()


# ---- 2. rate tables ----
CODES = {48000: 1, 32000: 32, 24000: 2, 16000: 3, 8000: 6}


@pytest.fixture(scope="module")
def signals(ref):
    """{rate: (T, DISTINCT, M) float32}"""
    sig = {48000: fuzz_pcm(DISTINCT, T, 48), 32000: ref[False][0]}
    for rate in (24000, 16000, 8000):
        sig[rate] = low_pcm(DISTINCT, T, CODES[rate], seed=rate)
    return sig


def mixed_rows(signals, rates, M_b):
    """(T, n, M_b): stream s carries signal s % DISTINCT of its rate at the front of its row, junk behind it"""
    pcm = np.full((T, len(rates), M_b), JUNK, np.float32)
    for s, r in enumerate(rates):
        pcm[:, s, :480 * r // 48000] = signals[r][:, s % DISTINCT]
    return pcm


def uniform_result(model, signals, rate, n):
    b = capi.Batch(model, n)
    if rate != 48000:
        b.set_pcm_rate(rate)
    res = run_calls(b, tiled(signals[rate], n))
    b.close()
    return res


def check_mixed(model, signals, b, rates, M_b, what):
    """the mixed batch b against the uniform batch of every rate, stream by stream; the tails of the `out` rows keep the caller's bytes"""
    n = len(rates)
    pcm = mixed_rows(signals, rates, M_b)
    res, t0 = [], 0
    for k in CALLS:
        out = np.full((k, n, M_b), SENTINEL, np.float32)
        vad, gains = np.empty((k, n), np.float32), np.empty((k, n, 32), np.float32)
        b.process_into(out.ctypes.data, np.ascontiguousarray(pcm[t0:t0 + k]).ctypes.data, vad.ctypes.data, gains.ctypes.data, k)
        res.append((out, vad, gains))
        t0 += k
    out, vad, gains = (np.concatenate([r[i] for r in res]) for i in range(3))
    for rate in sorted(set(rates)):
        M, idx = 480 * rate // 48000, [s for s, r in enumerate(rates) if r == rate]
        o, v, g = uniform_result(model, signals, rate, n)
        assert_bits_equal(out[:, idx, :M], o[:, idx], f"{what}: {rate} Hz streams = their uniform batch: out")
        assert_bits_equal(vad[:, idx], v[:, idx], f"{what}: {rate} Hz: vad")
        assert_bits_equal(gains[:, idx], g[:, idx], f"{what}: {rate} Hz: gains")
        assert_bits_equal(out[:, idx, M:], np.full((T, len(idx), M_b - M), SENTINEL), f"{what}: {rate} Hz: rows behind the frames")
    return out, vad, gains


def test_48k_batch_with_all_five_rates(model, signals, ref):
    rates = [48000, 32000, 24000, 16000, 8000] * 2
    b = capi.Batch(model, len(rates))
    b.set_stream_rates(rates)
    assert b.stream_rates().tolist() == rates and b.frame == 480
    codes = np.empty(len(rates), np.uint8)
    assert capi.lib().rnnoise_batch_stream_rates(b.h, codes.ctypes.data_as(C.POINTER(C.c_ubyte))) == 0
    assert codes.tolist() == [1, 32, 2, 3, 6] * 2
    out, vad, gains = check_mixed(model, signals, b, rates, 480, "48 kHz batch")
    # ... and the 32 kHz streams against the chain itself
    for s in (1, 6):
        assert_bits_equal(out[:, s, :M32], ref[False][1][:, s % DISTINCT], f"stream {s} = the chain")
        assert_bits_equal(b.export_state(s), ref[False][4][s % DISTINCT], f"state of stream {s}")
    b.close()


def test_32k_batch_takes_32_24_16_8_and_the_refusals(model, signals):
    rates = [32000, 24000, 16000, 8000] * 2
    n = len(rates)
    b = batch32(model, n)
    b.set_stream_rates(rates)
    assert b.stream_rates().tolist() == rates and b.frame == M32
    L = capi.lib()

    def c_set(bt, codes):
        a = np.asarray(codes, np.uint8)
        return L.rnnoise_batch_set_stream_rates(bt.h, a.ctypes.data_as(C.POINTER(C.c_ubyte)))
    # a 480-sample frame does not fit a 320-sample row: code 1 is refused, and so is anything that is no code; nothing changes
    for bad in (1, 0, 4, 31, 33, 255):
        assert c_set(b, [32, 2, 3, 6, bad, 2, 3, 6]) == -1, bad
    with pytest.raises(ValueError):
        b.set_stream_rates([48000] + rates[1:])
    assert b.stream_rates().tolist() == rates
    check_mixed(model, signals, b, rates, M32, "32 kHz batch")
    b.close()
    # a 320-sample frame does not fit a 240-sample row
    low = capi.Batch(model, 4)
    low.set_pcm_rate(24000)
    assert c_set(low, [2, 32, 3, 6]) == -1 and low.stream_rates().tolist() == [24000] * 4
    with pytest.raises(ValueError):
        low.set_stream_rates([24000, 32000, 16000, 8000])
    assert c_set(low, [2, 2, 3, 6]) == 0 and low.stream_rates().tolist() == [24000, 24000, 16000, 8000]
    low.close()
    # the other rates stay refused, and training features at 32 kHz
    b = batch32(model, 4)
    for hz in (44100, 12000, 11025):
        assert L.rnnoise_batch_set_pcm_rate(b.h, hz) == -1 and b.pcm_rate == 32000
    z = np.zeros((1, 4, 480), np.float32)
    with pytest.raises(RuntimeError):
        b.train_features(z, z, np.zeros((1, 4), np.float32), np.full(4, 481), np.full(4, 32), np.zeros(4))
    b.close()


def test_device_table_byte_32_in_a_16k_batch_reads_as_16k(model, signals):
    torch = pytest.importorskip("torch")
    n = 4
    b = capi.Batch(model, n)
    b.set_pcm_rate(16000)
    d_t = torch.tensor([32, 3, 6, 32], dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    b.set_stream_rates_device(d_t.data_ptr(), 0)
    torch.cuda.synchronize()
    rates = [16000, 16000, 8000, 16000]
    assert b.stream_rates().tolist() == rates
    check_mixed(model, signals, b, rates, 160, "16 kHz batch, byte 32")
    b.close()
    # ... and in a 48 kHz batch as 32 kHz
    b = capi.Batch(model, n)
    b.set_stream_rates_device(d_t.data_ptr(), 0)
    torch.cuda.synchronize()
    assert b.stream_rates().tolist() == [32000, 16000, 8000, 32000]
    check_mixed(model, signals, b, [32000, 16000, 8000, 32000], 480, "48 kHz batch, byte 32")
    b.close()


# ---- 3. masked and list calls, reset_streams ----
@pytest.mark.parametrize("n", [6, 261])
def test_masked_and_list_calls_keep_histories_and_resets_zero_them(model, blob_default, ref, n):
    pcm = tiled(ref[False][0], n)
    rows = [0, 1, 2, 3, 4, n - 1]
    chains = {s: Chain(blob_default, L32) for s in rows}
    b = batch32(model, n)
    act = np.ones((T, n), np.uint8)
    act[:, 0] = 0                    # never present in the masked calls
    act[:, 1] = np.arange(T) % 2     # every other frame
    act[1:3, 3] = 0                  # a gap of two frames
    # a masked call of three frames: absent rows keep the caller's bytes, present rows are the chain over the present frames only
    out = np.full((3, n, M32), SENTINEL, np.float32)
    out, vad, gains = b.process_masked(pcm[:3], act[:3], out=out)
    check_rows(chains, pcm[:3], out, vad, gains, {s: s for s in rows}, f"masked n={n}", active=act[:3])
    # a list call of two frames in scrambled order, one of its rows absent in its first frame
    listed = [n - 1, 0, 3, 1]
    la = np.ones((2, len(listed)), np.uint8)
    la[0, 2] = 0
    lp = np.ascontiguousarray(pcm[3:5][:, listed])
    out = np.full(lp.shape, SENTINEL, np.float32)
    out, vad, gains = b.process_list(lp, listed, active=la, out=out)
    check_rows(chains, lp, out, vad, gains, dict(enumerate(listed)), f"list n={n}", active=la)
    # reset_streams zeroes both histories with the state; the other streams go on
    b.reset_streams([1, n - 1])
    for s in (1, n - 1):
        chains[s].reset()
    out = np.full((1, n, M32), SENTINEL, np.float32)
    out, vad, gains = b.process_masked(pcm[5:], act[5:], out=out)
    check_rows(chains, pcm[5:], out, vad, gains, {s: s for s in rows}, f"after reset n={n}", active=act[5:])
    for s in rows:
        assert_bits_equal(b.export_state(s), chains[s].o.get_state(), f"n={n}: state of stream {s}")
    b.close()


# ---- 4. snapshots ----
def test_snapshots_carry_code_32_and_the_history(model, ref, signals):
    n = 4
    pcm = tiled(ref[False][0], n)
    a, b = batch32(model, n), batch32(model, n)
    a.process(pcm[:3])
    snap = a.save_streams()
    assert (snap[:, capi.SNAP_OFF_L].view(np.int32) == 32).all() and (snap[:, capi.SNAP_OFF_MAGIC].view(np.int32) == capi.SNAP_MAGIC).all()
    hist = snap[:, capi.SNAP_OFF_HIST:]
    assert hist[:, :47].any() and hist[:, 48:118].any() and not hist[:, 47].any() and not hist[:, 118:].any()
    # into 32 kHz streams of another batch: they continue bit for bit (the chain's frames 3..5)
    b.load_streams(snap)
    out, vad, gains = b.process(pcm[3:])
    assert_bits_equal(out, tiled(ref[False][1], n)[3:], "loaded streams continue: out")
    assert_bits_equal(vad, tiled(ref[False][2][:, :, None], n)[3:, :, 0], "loaded streams continue: vad")
    assert_bits_equal(gains, tiled(ref[False][3], n)[3:], "loaded streams continue: gains")
    for s in range(n):
        assert_bits_equal(b.export_state(s), ref[False][4][s % DISTINCT], f"state of loaded stream {s}")
    # into 16 kHz streams: the DenoiseState with a zero history -- what import_state of the same state gives
    c, d = capi.Batch(model, n), capi.Batch(model, n)
    for x in (c, d):
        x.set_pcm_rate(16000)
        x.process(tiled(signals[16000], n)[:2])  # (their histories are not zero when the records arrive)
    c.load_streams(snap)
    assert not c.save_streams()[:, capi.SNAP_OFF_HIST:].any(), "history of a 16 kHz stream loaded from a 32 kHz record"
    for s in range(n):
        d.import_state(s, a.export_state(s))
    p16 = tiled(signals[16000], n)[2:]
    for name, got, want in zip(("out", "vad", "gains"), c.process(p16), d.process(p16)):
        assert_bits_equal(got, want, f"16 kHz streams loaded from 32 kHz records: {name}")
    for x in (a, b, c, d):
        x.close()


# ---- 5. one case each against the plain 32 kHz result ----
def test_mulaw_at_32k(model, ref):
    """a companded stream's bytes fill the first 320 bytes of its int16 row; the other stream of the batch stays linear"""
    n = 2
    codes = g711.encode(ref[True][0][:, 0], "ulaw")                    # (T, 320) uint8
    lin = np.stack([g711.decode(codes, "ulaw"), ref[True][0][:, 1]], axis=1).astype(np.int16)
    plain = batch32(model, n)
    want, want_vad, want_gains = run_calls(plain, lin, s16=True)
    b = batch32(model, n)
    b.set_stream_formats(["ulaw", "s16"])
    rows = lin.copy()
    r8 = rows.view(np.uint8).reshape(T, n, 2 * M32)
    r8[:, 0, :] = 0x55
    r8[:, 0, :M32] = codes
    out = np.full((T, n, M32), SENTINEL16, np.int16)
    vad, gains = np.empty((T, n), np.float32), np.empty((T, n, 32), np.float32)
    b.process_into(out.ctypes.data, rows.ctypes.data, vad.ctypes.data, gains.ctypes.data, T, s16=True)
    o8 = out.view(np.uint8).reshape(T, n, 2 * M32)
    assert_bits_equal(o8[:, 0, :M32], g711.encode(want[:, 0], "ulaw"), "mu-law bytes out")
    assert_bits_equal(out[:, 0, M32 // 2:], np.full((T, M32 // 2), SENTINEL16), "the row behind the bytes keeps the caller's")
    assert_bits_equal(out[:, 1], want[:, 1], "the linear neighbour")
    assert_bits_equal(vad, want_vad, "vad")
    assert_bits_equal(gains, want_gains, "gains")
    plain.close()
    b.close()


def test_two_interleaved_channels_at_32k(model, ref):
    n, Cn = 4, 2
    for s16 in (False, True):
        pcm = tiled(ref[s16][0], n)
        b = batch32(model, n)
        b.set_pcm_channels(Cn)
        inter = np.ascontiguousarray(pcm.reshape(T, n // Cn, Cn, M32).transpose(0, 1, 3, 2))  # (T, G, 320, C)
        out, vad, gains = (b.process_s16 if s16 else b.process)(inter)
        assert out.shape == inter.shape
        assert_bits_equal(out.transpose(0, 1, 3, 2).reshape(T, n, M32), tiled(ref[s16][1], n), f"s16={s16}: interleaved out")
        assert_bits_equal(vad, tiled(ref[s16][2][:, :, None], n)[:, :, 0], f"s16={s16}: vad")
        assert_bits_equal(gains, tiled(ref[s16][3], n), f"s16={s16}: gains")
        b.close()


def test_stream_contiguous_layout_with_frame_stride_320(model, ref):
    n = 5
    L = capi.lib()
    assert L.rnnoise_amd_pcm_layout_fits(M32, T * M32, M32, n, T) == 1
    assert L.rnnoise_amd_pcm_layout_fits(M32, T * M32, 480, n, T) == 0     # (a 48 kHz frame would overlap its successor)
    assert L.rnnoise_amd_pcm_channels_fit(2 * M32, 2 * T * M32, M32, 2, 4, T) == 1
    b = batch32(model, n)
    b.set_pcm_layout(M32, T * M32)
    x, out = b.pcm_array(T), b.pcm_array(T, fill=SENTINEL)
    assert x.base.shape == (n * T * M32,)   # [B][T * 320]: one run of samples per stream
    x[:] = ref[False][0]
    out, vad, gains = b.process(x, out=out)
    assert_bits_equal(np.ascontiguousarray(out), ref[False][1], "[B][T] layout: out")
    assert_bits_equal(out.base.reshape(n, T, M32), ref[False][1].transpose(1, 0, 2), "... where the layout puts it")
    assert_bits_equal(vad, ref[False][2], "vad")
    assert_bits_equal(gains, ref[False][3], "gains")
    b.close()


# ---- 6. the CLI: a 2-channel 32 kHz PCM16 WAV ----
def test_cli_denoises_a_32k_stereo_wav(tmp_path, blob_default, ref):
    from rnnoise_amd import cli
    pcm, want = ref[True][0], ref[True][1]
    st = np.stack([pcm[:, 0].reshape(-1), pcm[:, 1].reshape(-1)], axis=1)   # (T * 320, 2)
    d = tmp_path / "in"
    d.mkdir()
    wav.write(str(d / "st.wav"), wav.WavInfo(32000, 2, "s16", False, 0, 0), st)
    (tmp_path / "w.blob").write_bytes(blob_default)
    cli.main(["denoise", "--model", str(tmp_path / "w.blob"), "--out-dir", str(tmp_path / "o"), "--chunk-frames", "4", str(d / "st.wav")])
    info, y = wav.read(str(tmp_path / "o" / "st.wav.denoised.wav"))
    assert (info.rate, info.channels, info.codec) == (32000, 2, "s16") and y.shape == ((T - 1) * M32, 2)
    for c in range(2):  # (the first output frame is dropped, as the reference's demo does)
        assert_bits_equal(y[:, c], want[1:, c].reshape(-1), f"channel {c} = the batch result")
    # --rate 32000 on RAW files: the same samples from a uniform 32 kHz batch
    for c in range(2):
        st[:, c].tofile(str(d / f"c{c}.raw"))
    cli.main(["denoise", "--model", str(tmp_path / "w.blob"), "--out-dir", str(tmp_path / "r"), "--rate", "32000",
              str(d / "c0.raw"), str(d / "c1.raw")])
    for c in range(2):
        assert_bits_equal(np.fromfile(str(tmp_path / "r" / f"c{c}.raw.denoised.raw"), np.int16), want[1:, c].reshape(-1), f"RAW file {c}")
