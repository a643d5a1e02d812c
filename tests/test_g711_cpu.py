"""The G.711 codec of the per-stream formats (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats), without a GPU: the four numpy
functions of rnnoise_amd/g711.py against the formulas (restated here as scalar Python, input by input), against CPython's audioop where
this Python still ships it, and their pinned properties -- round trips, ranges, monotony; and the library's own arithmetic
(rnnoise_amd/csrc/g711.h, the text the kernels compile) against the numpy definition for every input, compiled for the host."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rnnoise_amd import g711

X = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
B = np.arange(256, dtype=np.uint8)


def _ulaw_enc(x):
    p = x >> 2
    neg = p < 0
    p = min((-p if neg else p) + 33, 8191)
    seg = p.bit_length() - 1 - 5
    assert 0 <= seg <= 7
    return ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ (0x7F if neg else 0xFF)


def _ulaw_dec(b):
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return 132 - t if u & 0x80 else t - 132


def _alaw_enc(x):
    i = x >> 3
    neg = i < 0
    if neg:
        i = ~i
    seg = 0 if i < 32 else i.bit_length() - 1 - 4
    assert 0 <= seg <= 7
    m = (i >> 1) & 15 if seg < 2 else (i >> seg) & 15
    return ((seg << 4) | m) ^ (0x55 if neg else 0xD5)


def _alaw_dec(b):
    a = b ^ 0x55
    t = (a & 15) << 4
    seg = (a >> 4) & 7
    t = t + 8 if seg == 0 else (t + 0x108) << (seg - 1)
    return t if a & 0x80 else -t


def test_numpy_functions_are_the_formulas_for_every_input():
    assert g711.ulaw_encode(X).tolist() == [_ulaw_enc(int(x)) for x in X]
    assert g711.alaw_encode(X).tolist() == [_alaw_enc(int(x)) for x in X]
    assert g711.ulaw_decode(B).tolist() == [_ulaw_dec(int(b)) for b in B]
    assert g711.alaw_decode(B).tolist() == [_alaw_dec(int(b)) for b in B]
    assert g711.ulaw_encode(X).dtype == np.uint8 and g711.alaw_decode(B).dtype == np.int16


def test_against_audioop_where_python_ships_it():
    audioop = pytest.importorskip("audioop")  # (gone from CPython 3.13)
    assert audioop.lin2ulaw(X.tobytes(), 2) == g711.ulaw_encode(X).tobytes()
    assert audioop.lin2alaw(X.tobytes(), 2) == g711.alaw_encode(X).tobytes()
    assert audioop.ulaw2lin(B.tobytes(), 2) == g711.ulaw_decode(B).astype("<i2").tobytes()
    assert audioop.alaw2lin(B.tobytes(), 2) == g711.alaw_decode(B).astype("<i2").tobytes()


def test_round_trips_and_ranges():
    rt = g711.ulaw_encode(g711.ulaw_decode(B))
    assert np.flatnonzero(rt != B).tolist() == [0x7F] and rt[0x7F] == 0xFF  # negative zero re-encodes as positive zero
    assert np.array_equal(g711.alaw_encode(g711.alaw_decode(B)), B)
    u, a = g711.ulaw_decode(B).astype(np.int32), g711.alaw_decode(B).astype(np.int32)
    assert (u.min(), u.max()) == (-32124, 32124)
    assert (a.min(), a.max()) == (-32256, 32256)
    assert len(set(u.tolist())) == 255 and len(set(a.tolist())) == 256  # (mu-law has two zeros)
    # every code is reached by the encoders, except mu-law's negative zero
    assert set(g711.ulaw_encode(X).tolist()) == set(range(256)) - {0x7F}
    assert set(g711.alaw_encode(X).tolist()) == set(range(256))


@pytest.mark.parametrize("fmt", ["ulaw", "alaw"])
def test_decode_of_encode_is_monotonic_and_close(fmt):
    y = g711.decode(g711.encode(X, fmt), fmt).astype(np.int32)
    assert (np.diff(y) >= 0).all()
    # the quantisation step of the top segment is 1024 (both laws); mu-law clips at 32124, A-law at 32256
    assert np.abs(y - X.astype(np.int32)).max() <= 1024
    # decode(encode()) is idempotent
    assert np.array_equal(g711.decode(g711.encode(y.astype(np.int16), fmt), fmt), y.astype(np.int16))


def test_names_codes_and_the_linear_format():
    assert (g711.code("s16"), g711.code("ulaw"), g711.code("alaw")) == (0, 1, 2) == (g711.LINEAR, g711.ULAW, g711.ALAW)
    assert [g711.code(c) for c in (0, 1, 2)] == [0, 1, 2]
    for bad in ("pcm", "mulaw", 3, -1, 255):
        with pytest.raises(ValueError):
            g711.code(bad)
    assert np.array_equal(g711.encode(X, "s16"), X) and np.array_equal(g711.decode(X, 0), X)
    assert np.array_equal(g711.encode(X, 1), g711.ulaw_encode(X)) and np.array_equal(g711.decode(B, "alaw"), g711.alaw_decode(B))
    for fmt in ("ulaw", "alaw"):  # the segments and signs of all 256 codes: 16 codes in each of the 8 x 2
        seg, neg = g711.segment(B, fmt)
        assert sorted(zip(seg.tolist(), neg.tolist())) == sorted([(s, n) for s in range(8) for n in (False, True)] * 16)
        x = g711.decode(B, fmt).astype(np.int32)
        assert ((x < 0) <= neg).all() and ((x > 0) <= ~neg).all()


def test_the_librarys_arithmetic_is_the_numpy_definition_for_every_input(tmp_path):
    """rnnoise_amd/csrc/g711.h -- what hp_kernel.hip and dsp_kernels.hip compile for the device -- compiled for the host"""
    exe = str(tmp_path / "g711_sweep")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "g711_sweep.cpp"), "-o", exe], check=True)
    raw = subprocess.run([exe], capture_output=True, check=True).stdout
    assert len(raw) == 2 * 65536 + 2 * 256 * 2
    enc = np.frombuffer(raw[:2 * 65536], np.uint8).reshape(2, 65536)
    dec = np.frombuffer(raw[2 * 65536:], "<i2").reshape(2, 256)
    assert np.array_equal(enc[0], g711.ulaw_encode(X)) and np.array_equal(enc[1], g711.alaw_encode(X))
    assert np.array_equal(dec[0], g711.ulaw_decode(B)) and np.array_equal(dec[1], g711.alaw_decode(B))
