"""32 kHz PCM on the CPU (include/rnnoise_amd.h: rnnoise_batch_set_pcm_rate, RNNOISE_AMD_RATE_32K): the 2:3 resampler of
rnnoise_amd/resample.py -- its taps are the committed ones of L = 3, read at a 96 kHz grid --, its streaming form, its 47-sample delay
and the design of the prototype at that grid; the rate code in the header and the bindings; what needs no GPU of the C API and of
rnnoise_amd/wav.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from rnnoise_amd import capi, resample, wav
from test_resample_cpu import HEADER, response_db

L32 = resample.RATE_32K


def test_taps_are_the_committed_ones_of_L3_and_the_header_is_generated():
    text = open(HEADER).read()
    assert text == resample.header_text(), "rs_coeffs.h is not what `python -m rnnoise_amd.resample --header` emits"
    arrays = resample.parse_header(text)
    h3 = resample.h(3)
    up, dn = resample.Up(L32), resample.Down(L32)
    # up: rn_rs_up3 as it stands
    assert up.taps.shape == (3, 48)
    assert up.taps.reshape(-1).view(np.uint32).tolist() == arrays["rn_rs_up3"].view(np.uint32).tolist()
    # down: hd[e][k] = 2 h3[2 k + e], an exact doubling
    assert dn.taps.shape == (2, 72) and dn.D == 70 and resample.down_hist(L32) == 70
    want = np.stack([np.float32(2) * h3[e::2] for e in range(2)])
    assert (want.astype(np.float64) == 2 * h3.astype(np.float64).reshape(72, 2).T).all(), "the doubling is exact"
    assert dn.taps.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert arrays["rn_rs_hd32"].view(np.uint32).tolist() == want.reshape(-1).view(np.uint32).tolist()
    # the arrays the other rates use keep their names and contents
    assert arrays["rn_rs_h_all"].view(np.uint32).tolist() == np.concatenate([resample.h(L) for L in (2, 3, 6)]).view(np.uint32).tolist()
    assert resample.RATES[32000] == L32 == 32 and resample.frame_samples(L32) == 320
    assert [resample.frame_samples(L) for L in (1, 2, 3, 6)] == [480, 240, 160, 80]


def fir4(taps, window):
    """one output in the project's summation order, scalar float32"""
    a = [None] * 4
    for k in range(len(taps)):
        p = np.float32(taps[k]) * np.float32(window(k))
        a[k & 3] = p if a[k & 3] is None else np.float32(a[k & 3] + p)
    return np.float32(np.float32(a[0] + a[1]) + np.float32(a[2] + a[3]))


def test_whole_signal_form_is_the_index_arithmetic_of_the_header():
    """u[J] over q = floor(2 J / 3), p = 2 J mod 3; y[m] over e = m & 1, n0 = (3 m + 2) >> 1 -- at frame edges and inside"""
    rng = np.random.default_rng(32)
    x = (rng.standard_normal(960) * 3000).astype(np.float32)
    u = resample.up32(x)
    assert u.shape == (1440,)
    xs, hu = np.concatenate([np.zeros(47, np.float32), x]), resample.hup(3)
    for J in (0, 1, 2, 3, 4, 70, 71, 72, 478, 479, 480, 481, 959, 960, 1439):
        q, p = 2 * J // 3, 2 * J % 3
        assert fir4(hu[p], lambda k: xs[47 + q - k]).view(np.uint32) == u[J].view(np.uint32), J
    y = resample.down32(u)
    assert y.shape == (960,)
    vs, hd = np.concatenate([np.zeros(70, np.float32), u]), resample.hd32()
    for m in (0, 1, 2, 3, 46, 47, 318, 319, 320, 321, 639, 640, 959):
        e, n0 = m & 1, (3 * m + 2) >> 1
        assert fir4(hd[e], lambda k: vs[70 + n0 - k]).view(np.uint32) == y[m].view(np.uint32), m
    assert ((3 * 0 + 2) >> 1) - 71 == -70, "m = 0 reaches v[-70]"


def test_streaming_equals_whole_signal():
    rng = np.random.default_rng(L32)
    M, T, S = 320, 7, 3
    x = (rng.standard_normal((S, M * T)) * 3000).astype(np.float32)
    up, dn = resample.Up(L32, (S,)), resample.Down(L32, (S,))
    u = np.concatenate([up(x[:, t * M:(t + 1) * M]) for t in range(T)], axis=-1)
    y = np.concatenate([dn(u[:, t * 480:(t + 1) * 480]) for t in range(T)], axis=-1)
    assert u.shape == (S, 480 * T) and y.shape == (S, M * T)
    assert u.view(np.uint32).tolist() == resample.up32(x).view(np.uint32).tolist()
    assert y.view(np.uint32).tolist() == resample.down32(resample.up32(x)).view(np.uint32).tolist()
    assert up.hist.shape == (S, 47) and dn.hist.shape == (S, 70)


def test_up_then_down_is_a_delay_of_47_samples():
    """the three-tone signal and the thresholds of test_resample_cpu at R = 32000 (float64 measures 91.6 / 1.3 / 1.3 dB)"""
    R = 32000
    t = np.arange(6000)
    x = sum(a * np.sin(2 * np.pi * fr / R * t + ph) for a, fr, ph in
            ((3000, 0.02 * R, 0.1), (2000, 0.17 * R, 1.3), (1500, 0.34 * R, 2.2))).astype(np.float32)
    y = resample.down32(resample.up32(x))
    assert resample.DELAY == 47

    def snr(d):
        ref, got = x[300:len(x) - d].astype(np.float64), y[300 + d:].astype(np.float64)
        return 10 * np.log10((ref ** 2).sum() / ((got - ref) ** 2).sum())

    print(f"SNR at delay 46 / 47 / 48: {snr(46):.1f} / {snr(47):.1f} / {snr(48):.1f} dB")
    assert snr(47) > 60
    assert snr(46) < 10 and snr(48) < 10


def test_design_of_h3_read_at_the_96k_grid():
    h = resample.h(3)
    assert len(h) == 144
    f = np.linspace(0, 48000, 24001)
    db = response_db(h, f / 96000)
    assert np.ptp(db[f <= 12800]) <= 0.01, "passband ripple to 12.8 kHz"
    assert -db[f >= 16000].max() >= 70, "stopband attenuation from 16 kHz"
    # every phase of both filters has unit DC gain (the issue: within 1.4e-5)
    assert np.abs(resample.hup(3).astype(np.float64).sum(axis=1) - 1).max() <= 1.4e-5
    assert np.abs(resample.hd32().astype(np.float64).sum(axis=1) - 1).max() <= 1.4e-5


def test_rate_code_in_the_headers_and_the_bindings():
    text = open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    assert len(re.findall(r"^#define RNNOISE_AMD_RATE_32K 32\b", text, re.M)) == 1
    assert re.search(r"#define RNNOISE_AMD_RESAMPLE_DELAY 47\b", text)
    dev = open(os.path.join(ROOT, "rnnoise_amd", "csrc", "rn_dev.h")).read()
    assert re.search(r"^#define RN_RATE_32K 32\b", dev, re.M)
    assert capi.RATE_32K == 32
    assert capi.PCM_RATES_ALL == (48000, 32000, 24000, 16000, 8000)
    assert capi.PCM_RATES == (48000, 24000, 16000, 8000)
    assert capi.rate_code(np.array(capi.PCM_RATES_ALL)).tolist() == [1, 32, 2, 3, 6]
    assert capi.code_rate(np.array([1, 32, 2, 3, 6])).tolist() == list(capi.PCM_RATES_ALL)


def test_null_batch_calls_return_minus_one():
    L = capi.lib()
    assert L.rnnoise_batch_set_pcm_rate(None, 32000) == -1 and L.rnnoise_batch_pcm_rate(None) == -1
    buf = (C.c_ubyte * 4)(32, 2, 3, 6)
    assert L.rnnoise_batch_set_stream_rates(None, buf) == -1
    assert L.rnnoise_batch_set_stream_rates_device(None, C.cast(buf, C.c_void_p), None) == -1
    assert L.rnnoise_batch_stream_rates(None, buf) == -1
    assert list(buf) == [32, 2, 3, 6]


class _FakeLib:
    def __init__(self, rate):
        self.calls, self.rate = [], rate

    def rnnoise_batch_set_stream_rates(self, h, p):
        self.calls.append([p[i] for i in range(5)])
        return 0

    def rnnoise_batch_pcm_rate(self, h):
        return self.rate


def test_capi_maps_hz_to_codes_and_keeps_the_row_rule():
    def fake(rate):
        b = capi.Batch.__new__(capi.Batch)
        b._L, b.h, b.n = _FakeLib(rate), 1, 5
        return b
    b = fake(48000)
    b.set_stream_rates([48000, 32000, 24000, 16000, 8000])
    assert b._L.calls == [[1, 32, 2, 3, 6]] and b.frame == 480
    mid = fake(32000)
    assert mid.frame == 320
    mid.set_stream_rates([32000, 24000, 16000, 8000, 32000])
    assert mid._L.calls == [[32, 2, 3, 6, 32]]
    with pytest.raises(ValueError):
        mid.set_stream_rates([48000, 32000, 32000, 32000, 32000])  # a 480-sample frame in a 320-sample row
    low = fake(24000)
    with pytest.raises(ValueError):
        low.set_stream_rates([32000, 24000, 24000, 24000, 24000])  # a 320-sample frame in a 240-sample row
    for bad in (44100, 12000, 11025):
        with pytest.raises(ValueError):
            b.set_stream_rates([48000, bad, 24000, 16000, 8000])
    assert len(b._L.calls) == 1 and len(mid._L.calls) == 1 and not low._L.calls
    for x in (b, mid, low):
        x.h = None  # (nothing to destroy)


def test_wav_takes_32k_and_still_refuses_44100(tmp_path):
    assert 32000 in wav.RATES and 44100 not in wav.RATES
    x = (np.arange(640 * 2, dtype=np.int16) * 7).reshape(640, 2)
    p = str(tmp_path / "a.wav")
    wav.write(p, wav.WavInfo(32000, 2, "s16", False, 0, 0), x)
    info, y = wav.read(p)
    assert (info.rate, info.channels, info.codec, info.data_bytes) == (32000, 2, "s16", x.nbytes) and np.array_equal(y, x)
    raw = bytearray(open(p, "rb").read())
    at = raw.index(b"fmt ") + 8 + 4
    assert int.from_bytes(raw[at:at + 4], "little") == 32000 and int.from_bytes(raw[at + 4:at + 8], "little") == 32000 * 4
    raw[at:at + 4] = (44100).to_bytes(4, "little")
    q = str(tmp_path / "b.wav")
    open(q, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="sample rate"):
        wav.read_info(q)
    with pytest.raises(ValueError):
        wav.header(wav.WavInfo(44100, 1, "s16", False, 0, 0), 0)
