"""The resampler behind rnnoise_batch_set_pcm_rate, on the CPU: the committed filter table (rnnoise_amd/resample.py and
rnnoise_amd/csrc/rs_coeffs.h, bit-identical), its design properties, the streaming reference, the 47-sample delay, and the C API
surface in both product libraries and the ctypes binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from rnnoise_amd import capi, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rnnoise_amd", "csrc", "rs_coeffs.h")


def test_header_and_python_tables_are_bit_identical():
    text = open(HEADER).read()
    assert text == resample.header_text(), "rs_coeffs.h is not what `python -m rnnoise_amd.resample --header` emits"
    arrays = resample.parse_header(text)
    for L in (2, 3, 6):
        assert arrays[f"rn_rs_h{L}"].view(np.uint32).tolist() == resample.h(L).view(np.uint32).tolist()
        assert arrays[f"rn_rs_up{L}"].view(np.uint32).tolist() == resample.hup(L).reshape(-1).view(np.uint32).tolist()


def response_db(taps, f_norm):
    n = np.arange(len(taps))
    H = np.abs(np.exp(-2j * np.pi * np.outer(f_norm, n)) @ taps.astype(np.float64))
    return 20 * np.log10(np.maximum(H, 1e-30))


@pytest.mark.parametrize("L", [2, 3, 6])
def test_design_properties(L):
    h = resample.h(L)
    assert len(h) == 48 * L and np.array_equal(h, h[::-1]), "linear phase"
    np.testing.assert_allclose(h, resample.design(L), rtol=0, atol=1e-7)  # (the table is this design, up to a last bit)
    R = 48000 / L
    f = np.linspace(0, 24000, 12001)
    db = response_db(h, f / 48000)
    assert np.ptp(db[f <= 0.4 * R]) <= 0.01, "passband ripple"
    assert -db[f >= 0.5 * R].max() >= 70, "stopband attenuation"
    # the L-phase up filter as one 48 kHz filter: its taps interleaved back, gain L
    hu = resample.hup(L)
    inter = np.empty(48 * L, np.float64)
    for p in range(L):
        inter[p::L] = hu[p]
    dbu = response_db(inter / L, f / 48000)
    assert -dbu[f >= 0.5 * R].max() >= 70, "stopband attenuation of the up filter"
    assert np.abs(hu.astype(np.float64).sum(axis=1) - 1).max() <= 1e-4, "each up phase sums to 1"


@pytest.mark.parametrize("L", [2, 3, 6])
def test_streaming_equals_whole_signal(L):
    rng = np.random.default_rng(L)
    M, T, S = 480 // L, 7, 3
    x = (rng.standard_normal((S, M * T)) * 3000).astype(np.float32)
    up, dn = resample.Up(L, (S,)), resample.Down(L, (S,))
    u = np.concatenate([up(x[:, t * M:(t + 1) * M]) for t in range(T)], axis=-1)
    y = np.concatenate([dn(u[:, t * 480:(t + 1) * 480]) for t in range(T)], axis=-1)
    assert u.view(np.uint32).tolist() == resample.up(x, L).view(np.uint32).tolist()
    assert y.view(np.uint32).tolist() == resample.down(resample.up(x, L), L).view(np.uint32).tolist()


@pytest.mark.parametrize("L", [2, 3, 6])
def test_up_then_down_is_a_delay_of_47_samples(L):
    R = 48000 / L
    t = np.arange(6000)
    x = sum(a * np.sin(2 * np.pi * fr / R * t + ph) for a, fr, ph in
            ((3000, 0.02 * R, 0.1), (2000, 0.17 * R, 1.3), (1500, 0.34 * R, 2.2))).astype(np.float32)
    y = resample.down(resample.up(x, L), L)
    assert resample.DELAY == 47

    def snr(d):
        ref, got = x[300:len(x) - d].astype(np.float64), y[300 + d:].astype(np.float64)
        return 10 * np.log10((ref ** 2).sum() / ((got - ref) ** 2).sum())

    assert snr(47) > 60
    assert snr(46) < 10 and snr(48) < 10


def test_to_s16_is_the_truncating_cast():
    y = np.array([1.9, -1.9, 32767.9, 40000.0, -40000.0, 3e9, np.nan], np.float32)
    assert resample.to_s16(y).tolist() == [1, -1, 32767, 40000 - 65536, -40000 + 65536, 0, 0]


def test_header_declares_the_rate_calls():
    text = open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    assert re.search(r"RNNOISE_EXPORT int rnnoise_batch_set_pcm_rate\(RNNoiseBatch \*b, int hz\);", text)
    assert re.search(r"RNNOISE_EXPORT int rnnoise_batch_pcm_rate\(const RNNoiseBatch \*b\);", text)
    assert re.search(r"#define RNNOISE_AMD_RESAMPLE_DELAY 47\b", text)


@pytest.mark.parametrize("name", ["librnnoise_amd.so", "librnnoise.so.0"])
def test_both_product_libraries_export_the_rate_calls(name):
    path = os.path.join(ROOT, "rnnoise_amd", name)
    if not os.path.exists(path):
        pytest.fail(f"{path} not built")
    lib = ctypes.CDLL(path)
    for sym in ("rnnoise_batch_set_pcm_rate", "rnnoise_batch_pcm_rate"):
        assert hasattr(lib, sym), f"{name} lacks {sym}"


def test_capi_binds_the_rate_calls():
    assert {"rnnoise_batch_set_pcm_rate", "rnnoise_batch_pcm_rate"} <= set(capi.EXPORTS)
    L = capi.lib()
    assert L.rnnoise_batch_set_pcm_rate.argtypes is not None and L.rnnoise_batch_pcm_rate.argtypes is not None
    assert L.rnnoise_batch_set_pcm_rate(None, 16000) == -1 and L.rnnoise_batch_pcm_rate(None) == -1
    assert hasattr(capi.Batch, "set_pcm_rate") and hasattr(capi.Batch, "pcm_rate")
    assert capi.PCM_RATES == (48000, 24000, 16000, 8000)
