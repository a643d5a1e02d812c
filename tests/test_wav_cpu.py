"""The RIFF / WAVE reader and writer of the file front end (rnnoise_amd/wav.py), without a GPU: every header form it accepts makes
the round trip, unknown chunks are skipped with their pad byte, a data chunk never reaches past the end of the file, and everything
else is refused with a message that names the file and the field."""
import struct

import numpy as np
import pytest

from rnnoise_amd import wav


def _fmt(tag, channels, rate, bits, block=None, ext=None, cb=None):
    block = channels * bits // 8 if block is None else block
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    if ext is not None:
        body += struct.pack("<HHI", 22 if cb is None else cb, bits, 0) + ext
    return b"fmt " + struct.pack("<I", len(body)) + body


def _riff(*chunks, form=b"WAVE"):
    body = b"".join(chunks)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + form + body


def _data(payload, n=None):
    return b"data" + struct.pack("<I", len(payload) if n is None else n) + payload + (b"\0" if len(payload) & 1 else b"")


def _guid(tag):
    return struct.pack("<H", tag) + wav.GUID_TAIL


FORMS = [(codec, ext, ch, rate) for codec in ("s16", "alaw", "ulaw") for ext in (False, True)
         for ch, rate in ((1, 8000), (2, 48000), (3, 16000), (8, 24000))]


@pytest.mark.parametrize("codec,ext,ch,rate", FORMS)
def test_round_trip(tmp_path, codec, ext, ch, rate):
    rng = np.random.default_rng(ch * rate)
    frames = 37  # (odd: a companded mono file ends on a pad byte)
    x = rng.integers(-32768, 32768, (frames, ch)).astype(np.int16) if codec == "s16" else rng.integers(0, 256, (frames, ch)).astype(np.uint8)
    p = str(tmp_path / "a.wav")
    info = wav.WavInfo(rate, ch, codec, ext, 0, 0)
    wav.write(p, info, x)
    assert wav.is_wav(p)
    got, y = wav.read(p)
    assert (got.rate, got.channels, got.codec, got.extensible) == (rate, ch, codec, ext)
    assert got.data_bytes == x.nbytes and got.width == x.itemsize and got.block == ch * x.itemsize
    assert y.dtype == x.dtype and np.array_equal(y, x)
    raw = open(p, "rb").read()
    assert raw[got.data_offset:got.data_offset + got.data_bytes] == x.tobytes()
    assert struct.unpack("<I", raw[4:8])[0] == len(raw) - 8 and len(raw) % 2 == 0  # the RIFF size covers the file, pad byte included
    assert wav.header(got, got.data_bytes) == raw[:got.data_offset]                 # ... and the writer reproduces the header it read
    if codec == "s16" and not ext:  # the plain form is what the standard library writes and reads
        import wave
        with wave.open(p, "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (ch, 2, rate, frames)


def test_reads_what_the_standard_library_writes(tmp_path):
    import wave
    p = str(tmp_path / "std.wav")
    x = np.arange(-300, 300, dtype=np.int16).reshape(-1, 2)
    with wave.open(p, "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(x.tobytes())
    info, y = wav.read(p)
    assert (info.rate, info.channels, info.codec, info.extensible, info.data_offset) == (16000, 2, "s16", False, 44)
    assert np.array_equal(y, x)


def test_unknown_chunks_are_skipped_with_their_pad_byte(tmp_path):
    p = str(tmp_path / "chunks.wav")
    payload = bytes(range(40))
    odd = b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\0"      # odd length: one pad byte follows
    even = b"bext" + struct.pack("<I", 6) + b"123456"
    open(p, "wb").write(_riff(odd, _fmt(1, 2, 48000, 16), even, b"junk" + struct.pack("<I", 1) + b"x\0", _data(payload), odd))
    info, y = wav.read(p)
    assert info.data_bytes == 40 and y.shape == (10, 2) and y.tobytes() == payload
    assert info.data_offset == 12 + len(odd) + 24 + len(even) + 10 + 8


def test_fmt_chunk_of_18_bytes(tmp_path):
    p = str(tmp_path / "ul.wav")
    body = struct.pack("<HHIIHHH", 7, 1, 8000, 8000, 1, 8, 0)
    open(p, "wb").write(_riff(b"fmt " + struct.pack("<I", 18) + body, b"fact" + struct.pack("<II", 4, 5), _data(b"\xff" * 5)))
    info, y = wav.read(p)
    assert (info.codec, info.rate, info.channels, info.data_bytes) == ("ulaw", 8000, 1, 5) and y.shape == (5, 1)


@pytest.mark.parametrize("claimed", [1000, 0xFFFFFFFF, 25])
def test_truncated_data_chunk(tmp_path, claimed):
    """the header's length, but never beyond the end of the file -- and a whole number of blocks"""
    p = str(tmp_path / "cut.wav")
    payload = bytes(range(22))  # 5 blocks of 4 bytes and half a block
    open(p, "wb").write(_riff(_fmt(1, 2, 48000, 16)) + b"data" + struct.pack("<I", claimed) + payload)
    info, y = wav.read(p)
    assert info.data_bytes == 20 and y.shape == (5, 2) and y.tobytes() == payload[:20]


def test_data_length_shorter_than_the_file(tmp_path):
    p = str(tmp_path / "short.wav")
    open(p, "wb").write(_riff(_fmt(1, 1, 8000, 16), _data(bytes(12), 8), b"LIST" + struct.pack("<I", 4) + b"tail"))
    assert wav.read_info(p).data_bytes == 8


REJECT = [
    ("RIFF header", lambda: b"RIFX" + _riff(_fmt(1, 1, 8000, 16), _data(b"ab"))[4:]),
    ("RIFF header", lambda: _riff(_fmt(1, 1, 8000, 16), _data(b"ab"), form=b"AVI ")),
    ("RIFF header", lambda: b"RIFF\0\0"),
    ("fmt chunk", lambda: _riff(_data(b"abcd"))),
    ("fmt chunk", lambda: _riff(b"LIST" + struct.pack("<I", 2) + b"ab")),
    ("fmt chunk", lambda: _riff(b"fmt " + struct.pack("<I", 14) + bytes(14), _data(b"abcd"))),
    ("fmt chunk", lambda: _riff(_fmt(0xFFFE, 2, 48000, 16) + b"", _data(b"abcd"))),
    ("data chunk", lambda: _riff(_fmt(1, 1, 8000, 16), b"LIST" + struct.pack("<I", 2) + b"ab")),
    ("format tag", lambda: _riff(_fmt(3, 1, 48000, 32), _data(b"abcd"))),
    ("format tag", lambda: _riff(_fmt(2, 1, 8000, 4, block=256), _data(b"abcd"))),
    ("bits per sample", lambda: _riff(_fmt(1, 1, 48000, 8), _data(b"abcd"))),
    ("bits per sample", lambda: _riff(_fmt(1, 1, 48000, 24), _data(b"abc"))),
    ("bits per sample", lambda: _riff(_fmt(7, 1, 8000, 16), _data(b"abcd"))),
    ("channels", lambda: _riff(_fmt(1, 0, 48000, 16), _data(b"abcd"))),
    ("channels", lambda: _riff(_fmt(1, 9, 48000, 16), _data(bytes(18)))),
    ("sample rate", lambda: _riff(_fmt(1, 1, 44100, 16), _data(b"abcd"))),
    ("sample rate", lambda: _riff(_fmt(6, 1, 11025, 8), _data(b"abcd"))),
    ("block align", lambda: _riff(_fmt(1, 2, 48000, 16, block=2), _data(b"abcd"))),
    ("sub-format", lambda: _riff(_fmt(0xFFFE, 2, 48000, 32, ext=_guid(3)), _data(bytes(8)))),
    ("sub-format", lambda: _riff(_fmt(0xFFFE, 2, 48000, 16, ext=struct.pack("<H", 1) + bytes(14)), _data(bytes(8)))),
    ("fmt chunk", lambda: _riff(_fmt(0xFFFE, 2, 48000, 16, ext=_guid(1), cb=0), _data(bytes(8)))),
]


@pytest.mark.parametrize("field,make", REJECT, ids=[f"{i}-{f.replace(' ', '_')}" for i, (f, _) in enumerate(REJECT)])
def test_rejections_name_the_file_and_the_field(tmp_path, field, make):
    p = str(tmp_path / "bad.wav")
    open(p, "wb").write(make())
    with pytest.raises(ValueError) as e:
        wav.read_info(p)
    assert str(e.value).startswith(f"{p}: {field}: "), str(e.value)


def test_extensible_bits_follow_the_sub_format(tmp_path):
    p = str(tmp_path / "ext.wav")
    open(p, "wb").write(_riff(_fmt(0xFFFE, 2, 8000, 8, ext=_guid(6)), _data(bytes(6))))
    info = wav.read_info(p)
    assert (info.codec, info.extensible, info.channels, info.data_bytes) == ("alaw", True, 2, 6)
    open(p, "wb").write(_riff(_fmt(0xFFFE, 2, 8000, 16, ext=_guid(6)), _data(bytes(8))))
    with pytest.raises(ValueError, match="bits per sample"):
        wav.read_info(p)


def test_writer_refuses_what_the_reader_would():
    for info in (wav.WavInfo(44100, 1, "s16", False, 0, 0), wav.WavInfo(48000, 9, "s16", False, 0, 0), wav.WavInfo(48000, 1, "f32", False, 0, 0)):
        with pytest.raises(ValueError):
            wav.header(info, 0)


def test_is_wav_on_raw_bytes(tmp_path):
    p = str(tmp_path / "a.raw")
    open(p, "wb").write(bytes(100))
    assert not wav.is_wav(p)
    open(p, "wb").write(b"RIFF")
    assert not wav.is_wav(p)
