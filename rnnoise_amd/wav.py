"""A small RIFF / WAVE header reader and writer for the file front end (rnnoise_amd/cli.py).  Host only.

The standard library's `wave` module refuses everything but format 1; telephony files are format 6 (A-law) and 7 (mu-law).  This
module reads and writes exactly what a batch can take where it lies (include/rnnoise_amd.h: the rate table, the format table and the
channel count):

    format 1 (PCM) with 16-bit samples, format 6 (A-law) and format 7 (mu-law) with 8-bit samples,
    WAVE_FORMAT_EXTENSIBLE (0xFFFE) whose sub-format is one of those three,
    1 to 8 channels, interleaved,  at 8000, 16000, 24000, 32000 or 48000 Hz.

Chunks other than `fmt ` and `data` are skipped (with the pad byte of an odd length); the `data` length is the header's, but never
beyond the end of the file (a recording cut short, or a writer that left 0 / 0xFFFFFFFF there: the rest of the file).  Anything else
raises a ValueError that names the file and the field.  No sample is touched: the caller reads and writes the `data` bytes itself.
"""
from __future__ import annotations

import os
import struct
from typing import NamedTuple

import numpy as np

RATES = (8000, 16000, 24000, 32000, 48000)
MAX_CHANNELS = 8
CODECS = {1: "s16", 6: "alaw", 7: "ulaw"}            # wFormatTag -> sample format (rnnoise_amd/g711.py names)
TAGS = {v: k for k, v in CODECS.items()}
BITS = {"s16": 16, "alaw": 8, "ulaw": 8}
EXTENSIBLE = 0xFFFE
# the 14 bytes every KSDATAFORMAT_SUBTYPE_<wave format> GUID ends with; its first two are the format tag
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


class WavInfo(NamedTuple):
    rate: int           # samples per second and channel
    channels: int       # interleaved channels
    codec: str          # "s16" | "alaw" | "ulaw"
    extensible: bool    # the header is WAVE_FORMAT_EXTENSIBLE
    data_offset: int    # where the samples start in the file
    data_bytes: int     # bytes of samples (a whole number of blocks)

    @property
    def width(self) -> int:
        """bytes per sample"""
        return BITS[self.codec] // 8

    @property
    def block(self) -> int:
        """bytes per sample of every channel"""
        return self.width * self.channels


def is_wav(path: str) -> bool:
    """whether the file starts with RIFF....WAVE"""
    with open(path, "rb") as f:
        h = f.read(12)
    return len(h) == 12 and h[:4] == b"RIFF" and h[8:] == b"WAVE"


def read_info(path: str) -> WavInfo:
    """the header of a WAV file; ValueError (naming the file and the field) for anything this module does not take"""
    def bad(field, what):
        return ValueError(f"{path}: {field}: {what}")

    size = os.path.getsize(path)
    with open(path, "rb") as f:
        h = f.read(12)
        if len(h) < 12 or h[:4] != b"RIFF" or h[8:] != b"WAVE":
            raise bad("RIFF header", "not a RIFF / WAVE file")
        fmt = None
        while True:
            pos = f.tell()
            ch = f.read(8)
            if len(ch) < 8:
                raise bad("data chunk", "none in the file") if fmt else bad("fmt chunk", "none in the file")
            cid, n = ch[:4], struct.unpack("<I", ch[4:])[0]
            if cid == b"fmt ":
                body = f.read(n)
                if n < 16 or len(body) < n:
                    raise bad("fmt chunk", f"{min(n, len(body))} bytes, at least 16 expected")
                tag, channels, rate, _, block, bits = struct.unpack("<HHIIHH", body[:16])
                extensible = tag == EXTENSIBLE
                if extensible:
                    if n < 40 or struct.unpack("<H", body[16:18])[0] < 22:
                        raise bad("fmt chunk", f"{n} bytes, 40 expected for WAVE_FORMAT_EXTENSIBLE")
                    if body[26:40] != GUID_TAIL:
                        raise bad("sub-format", f"GUID {body[24:40].hex()} is no wave format")
                    tag = struct.unpack("<H", body[24:26])[0]
                    if tag not in CODECS:
                        raise bad("sub-format", f"{tag} unsupported (1 PCM, 6 A-law, 7 mu-law)")
                elif tag not in CODECS:
                    raise bad("format tag", f"{tag} unsupported (1 PCM, 6 A-law, 7 mu-law, 0xFFFE extensible)")
                codec = CODECS[tag]
                if bits != BITS[codec]:
                    raise bad("bits per sample", f"{bits} unsupported for format {tag} ({BITS[codec]} expected)")
                if not 1 <= channels <= MAX_CHANNELS:
                    raise bad("channels", f"{channels} unsupported (1 .. {MAX_CHANNELS})")
                if rate not in RATES:
                    raise bad("sample rate", f"{rate} unsupported (one of {RATES})")
                if block != channels * bits // 8:
                    raise bad("block align", f"{block} for {channels} channels of {bits} bits")
                fmt = (rate, channels, codec, extensible)
            elif cid == b"data":
                if fmt is None:
                    raise bad("fmt chunk", "none in front of the data chunk")
                start = pos + 8
                have = min(n, max(size - start, 0))  # (never beyond the end of the file)
                blk = fmt[1] * BITS[fmt[2]] // 8
                return WavInfo(*fmt, start, have - have % blk)
            else:
                f.seek(n, 1)
            if n & 1:
                f.seek(1, 1)  # (chunks are word-aligned: an odd length is followed by a pad byte)


def header(info: WavInfo, data_bytes: int) -> bytes:
    """the bytes in front of `data_bytes` bytes of samples, in the form `info` describes: the 16-byte fmt chunk for PCM, the 18-byte
    one and a fact chunk for the companded formats, the 40-byte one (and a fact chunk) for WAVE_FORMAT_EXTENSIBLE"""
    if info.codec not in TAGS or not 1 <= info.channels <= MAX_CHANNELS or info.rate not in RATES:
        raise ValueError(f"cannot write a WAV header for {info}")
    tag, bits = TAGS[info.codec], BITS[info.codec]
    block = info.channels * bits // 8
    base = struct.pack("<HHIIHH", EXTENSIBLE if info.extensible else tag, info.channels, info.rate, info.rate * block, block, bits)
    if info.extensible:
        mask = (1 << info.channels) - 1 if info.channels > 2 else (4, 3)[info.channels - 1]  # (front centre; front left | right)
        base += struct.pack("<HHI", 22, bits, mask) + struct.pack("<H", tag) + GUID_TAIL
    elif tag != 1:
        base += struct.pack("<H", 0)
    chunks = b"fmt " + struct.pack("<I", len(base)) + base
    if info.extensible or tag != 1:
        chunks += b"fact" + struct.pack("<II", 4, data_bytes // block)
    chunks += b"data" + struct.pack("<I", data_bytes)
    pad = data_bytes & 1
    return b"RIFF" + struct.pack("<I", 4 + len(chunks) + data_bytes + pad) + b"WAVE" + chunks


def read(path: str):
    """(info, samples): samples (frames, channels) int16, or uint8 codes for a companded file, as they lie in the file"""
    info = read_info(path)
    with open(path, "rb") as f:
        f.seek(info.data_offset)
        raw = f.read(info.data_bytes)
    raw = raw[:len(raw) - len(raw) % info.block]
    return info, np.frombuffer(raw, np.int16 if info.width == 2 else np.uint8).reshape(-1, info.channels)


def write(path: str, info: WavInfo, samples) -> None:
    """samples (frames, channels) -- int16, or uint8 codes for a companded format -- under the header `info` describes"""
    a = np.ascontiguousarray(samples, np.int16 if BITS[info.codec] == 16 else np.uint8)
    if a.ndim != 2 or a.shape[1] != info.channels:
        raise ValueError(f"{path}: samples {a.shape} for {info.channels} channels")
    data = a.tobytes()
    with open(path, "wb") as f:
        f.write(header(info, len(data)))
        f.write(data)
        if len(data) & 1:
            f.write(b"\0")
