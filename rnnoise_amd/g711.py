"""G.711 companding of the batch API's int16 calls (include/rnnoise_amd.h: rnnoise_batch_set_stream_formats).

A stream whose format is mu-law or A-law sends and receives one byte per sample in the rows of the `_s16` calls: the library expands
the byte to int16 in front of the denoiser and compresses the int16 output behind it.  This module states the four mappings in
integer numpy; they are the definition the library's kernels (rnnoise_amd/csrc/g711.h) and the tests are held to, bit for bit.
`>>` is an arithmetic shift, x an int16 widened to int32, b a byte.

  mu-law encode  p = x >> 2; neg = p < 0; p = min((neg ? -p : p) + 33, 8191); seg = floor(log2(p)) - 5  (0..7)
                 b = ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ (neg ? 0x7F : 0xFF)
  mu-law decode  u = ~b & 0xFF; t = (((u & 15) << 3) + 132) << ((u >> 4) & 7); x = (u & 0x80) ? 132 - t : t - 132
  A-law encode   i = x >> 3; neg = i < 0; if (neg) i = ~i; seg = i < 32 ? 0 : floor(log2(i)) - 4  (0..7)
                 m = seg < 2 ? (i >> 1) & 15 : (i >> seg) & 15; b = ((seg << 4) | m) ^ (neg ? 0x55 : 0xD5)
  A-law decode   a = b ^ 0x55; t = (a & 15) << 4; seg = (a >> 4) & 7; t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1)
                 x = (a & 0x80) ? t : -t

This is the 14-bit / 13-bit form whose four tables equal CPython's audioop.lin2ulaw / ulaw2lin / lin2alaw / alaw2lin at width 2 for
every input.  encode(decode(b)) == b for every A-law code and every mu-law code except 0x7F (negative zero, which re-encodes as
0xFF); the decoders range over +-32124 (mu-law) and +-32256 (A-law).
"""
from __future__ import annotations

import numpy as np

LINEAR, ULAW, ALAW = 0, 1, 2  # RNNOISE_AMD_PCM_LINEAR / _ULAW / _ALAW
FORMATS = {"s16": LINEAR, "ulaw": ULAW, "alaw": ALAW}
NAMES = {v: k for k, v in FORMATS.items()}


def _floor_log2(p: np.ndarray) -> np.ndarray:
    """floor(log2(p)) of positive int32 values below 2^15, in integers"""
    r = np.zeros(p.shape, np.int32)
    for k in range(1, 15):
        r += (p >> k) != 0
    return r


def ulaw_encode(x) -> np.ndarray:
    """int16 -> mu-law bytes"""
    p = np.asarray(x, np.int16).astype(np.int32) >> 2
    neg = p < 0
    p = np.minimum(np.where(neg, -p, p) + 33, 8191)
    seg = _floor_log2(p) - 5
    b = ((seg << 4) | ((p >> (seg + 1)) & 15)) ^ np.where(neg, 0x7F, 0xFF)
    return b.astype(np.uint8)


def ulaw_decode(b) -> np.ndarray:
    """mu-law bytes -> int16"""
    u = ~np.asarray(b, np.uint8).astype(np.int32) & 0xFF
    t = (((u & 15) << 3) + 132) << ((u >> 4) & 7)
    return np.where(u & 0x80, 132 - t, t - 132).astype(np.int16)


def alaw_encode(x) -> np.ndarray:
    """int16 -> A-law bytes"""
    i = np.asarray(x, np.int16).astype(np.int32) >> 3
    neg = i < 0
    i = np.where(neg, ~i, i)
    seg = np.where(i < 32, 0, _floor_log2(np.maximum(i, 1)) - 4)
    m = np.where(seg < 2, (i >> 1) & 15, (i >> seg) & 15)
    b = ((seg << 4) | m) ^ np.where(neg, 0x55, 0xD5)
    return b.astype(np.uint8)


def alaw_decode(b) -> np.ndarray:
    """A-law bytes -> int16"""
    a = np.asarray(b, np.uint8).astype(np.int32) ^ 0x55
    t = (a & 15) << 4
    seg = (a >> 4) & 7
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


def code(fmt) -> int:
    """the format code of a name ("s16" | "ulaw" | "alaw") or of a code 0..2"""
    if isinstance(fmt, str):
        if fmt not in FORMATS:
            raise ValueError(f"PCM format {fmt!r} unsupported (one of {sorted(FORMATS)})")
        return FORMATS[fmt]
    v = int(fmt)
    if v not in NAMES:
        raise ValueError(f"PCM format code {v} unsupported (0 s16, 1 ulaw, 2 alaw)")
    return v


def encode(x, fmt) -> np.ndarray:
    """int16 -> the bytes of format `fmt` (a name or a code; linear: the int16 values unchanged)"""
    c = code(fmt)
    return ulaw_encode(x) if c == ULAW else alaw_encode(x) if c == ALAW else np.asarray(x, np.int16)


def decode(b, fmt) -> np.ndarray:
    """the bytes of format `fmt` -> int16 (linear: the int16 values unchanged)"""
    c = code(fmt)
    return ulaw_decode(b) if c == ULAW else alaw_decode(b) if c == ALAW else np.asarray(b, np.int16)


def segment(b, fmt) -> np.ndarray:
    """(segment 0..7, negative) of companded bytes: the chord of the code and its sign"""
    c = code(fmt)
    v = np.asarray(b, np.uint8).astype(np.int32)
    if c == ULAW:
        u = ~v & 0xFF
        return (u >> 4) & 7, (u & 0x80) != 0
    a = v ^ 0x55
    return (a >> 4) & 7, (a & 0x80) == 0
