"""ctypes binding of librnnoise_amd_score.so (include/rnnoise_amd_score.h): denoised PCM scored against the clean signal on the
device -- eight double sums per sequence, in an order the header fixes -- and the metrics read off those sums.

  score_device(...)   raw device pointers, asynchronous on a stream: the planes where they lie, through strides
  score(...)          numpy arrays, synchronous (the library's host form)
  metrics(sums, ...)  SNR, SI-SDR, their improvements and the segmental SNR per sequence; summary() their means

The library is a separate one: nothing here goes through rnnoise_amd.capi's prototype table, and the product libraries do not know it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librnnoise_amd_score.so")

FRAME = 480  # RNNOISE_AMD_SCORE_FRAME
SLOTS = 8    # RNNOISE_AMD_SCORE_SLOTS: r*r, x*x, y*y, x*r, y*r, (x-r)^2, (y-r)^2, 1 -- r clean, x noisy, y denoised
DELAY = 960  # RNNOISE_AMD_SCORE_DELAY: samples by which the denoiser delays its input
SEG_MIN_DB, SEG_MAX_DB = -10.0, 35.0  # the clamp of a frame's SNR in the segmental SNR


class Plane(C.Structure):
    """RNNoiseAudioPlane: sample i of frame t of row s at p[t * frame_stride + s * row_stride + i], strides in floats"""
    _fields_ = [("p", C.c_void_p), ("frame_stride", C.c_long), ("row_stride", C.c_long)]


class Call(C.Structure):
    """RNNoiseAudioScore"""
    _fields_ = [("ref", Plane), ("in_", Plane), ("out", Plane), ("n_rows", C.c_int), ("t0", C.c_int), ("n_frames", C.c_int),
                ("first", C.c_int), ("delay", C.c_int), ("terms_frames", C.c_int)]


_int, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
# symbol -> (restype, argtypes), in the header's order; tests/test_audio_score_cpu.py holds the table against the header
PROTOTYPES = {
    "rnnoise_amd_audio_score_check": (_int, (C.POINTER(Call),)),
    "rnnoise_amd_audio_score_device": (_int, (_int, _vp, _vp, C.POINTER(Call), _vp)),
    "rnnoise_amd_audio_score": (_int, (_int, _dp, _dp, C.POINTER(Call))),
}
EXPORTS = list(PROTOTYPES)

def lib():
    return _sidelib.load(LIB_PATH, PROTOTYPES)


def layout_frames(n_rows: int):
    """(frame_stride, row_stride) of a [T][n_rows][480] plane: what the training-mix and the process calls use"""
    return n_rows * FRAME, FRAME


def layout_streams(n_frames: int, pad: int = 0):
    """(frame_stride, row_stride) of a stream-contiguous [n_rows][n_frames * 480 + pad] plane"""
    return FRAME, n_frames * FRAME + pad


def make_call(ref, inp, out, n_rows, t0, n_frames, first=2, delay=DELAY, terms_frames=0) -> Call:
    """ref, inp, out: (pointer, frame_stride, row_stride) each, the pointer an int"""
    planes = [Plane(int(p) or None, int(fs), int(rs)) for p, fs, rs in (ref, inp, out)]
    return Call(*planes, int(n_rows), int(t0), int(n_frames), int(first), int(delay), int(terms_frames))


def check(call: Call) -> bool:
    """whether the score calls accept `call` (rnnoise_amd_audio_score_check; host only, nothing is dereferenced)"""
    return lib().rnnoise_amd_audio_score_check(C.byref(call)) == 0


def score_device(d_sums: int, ref, inp, out, n_rows: int, t0: int, n_frames: int, first: int = 2, delay: int = DELAY,
                 d_frame_terms: int = 0, terms_frames: int = 0, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_audio_score_device on raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle): ADDS the sums
    of output frames [max(t0, first), t0 + n_frames) of n_rows sequences to d_sums [n_rows][8] float64 and, with d_frame_terms
    [n_rows][terms_frames][8], writes those frames' records.  ref, inp, out: (pointer, frame_stride, row_stride) each, planes that
    hold the sequences from frame 0.  ValueError where the library refuses the arguments."""
    call = make_call(ref, inp, out, n_rows, t0, n_frames, first, delay, terms_frames)
    if lib().rnnoise_amd_audio_score_device(int(device), d_sums or None, d_frame_terms or None, C.byref(call), stream or None):
        raise ValueError("rnnoise_amd_audio_score_device refused the call (include/rnnoise_amd_score.h: a null or unaligned plane, a "
                         "stride below 480 or no multiple of 4, first * 480 < delay, counts out of range) or could not launch")


def _plane(a, name):
    """(pointer, frame_stride, row_stride) of a (T, N, 480) float32 array or view whose samples are contiguous"""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == FRAME):
        raise ValueError(f"{name}: a (frames, rows, 480) float32 array")
    if a.strides[2] != 4 or a.strides[0] % 16 or a.strides[1] % 16 or a.ctypes.data % 16:
        raise ValueError(f"{name}: contiguous samples, strides that are multiples of 4 floats and a 16-byte aligned base")
    return a.ctypes.data, a.strides[0] // 4, a.strides[1] // 4


def score(ref, inp, out, t0: int = 0, n_frames=None, first: int = 2, delay: int = DELAY, sums=None, frame_terms=None, device: int = 0):
    """rnnoise_amd_audio_score on host arrays, synchronous.  ref, inp, out: (T, N, 480) float32 arrays or views -- any strides the
    header allows; a stream-contiguous (N, T * 480) array `a` goes in as a.reshape(N, T, 480).transpose(1, 0, 2) -- holding the
    sequences from frame 0.  Scores output frames [max(t0, first), t0 + n_frames); n_frames None: to the end.  sums: (N, 8) float64,
    ADDED to in place (None: zeros); frame_terms: None or (N, T, 8) float64, written at the scored frames.  -> sums"""
    T, N = out.shape[0], out.shape[1]
    n_frames = T - t0 if n_frames is None else n_frames
    planes = [_plane(a, n) for a, n in ((ref, "ref"), (inp, "inp"), (out, "out"))]
    for a in (ref, inp):
        if a.shape[1] != N or a.shape[0] < t0 + n_frames:
            raise ValueError("ref / inp: the rows of out and at least its frames")
    if t0 + n_frames > T:
        raise ValueError(f"frames [{t0}, {t0 + n_frames}) of {T}")
    if sums is None:
        sums = np.zeros((N, SLOTS), np.float64)
    if not (sums.dtype == np.float64 and sums.shape == (N, SLOTS) and sums.flags.c_contiguous):
        raise ValueError("sums: a contiguous (rows, 8) float64 array")
    terms_frames = 0
    if frame_terms is not None:
        if not (frame_terms.dtype == np.float64 and frame_terms.ndim == 3 and frame_terms.shape[0] == N and frame_terms.shape[2] == SLOTS
                and frame_terms.flags.c_contiguous):
            raise ValueError("frame_terms: a contiguous (rows, frames, 8) float64 array")
        terms_frames = frame_terms.shape[1]
    call = make_call(*planes, N, t0, n_frames, first, delay, terms_frames)
    if lib().rnnoise_amd_audio_score(int(device), sums.ctypes.data_as(_dp),
                                     frame_terms.ctypes.data_as(_dp) if frame_terms is not None else None, C.byref(call)):
        raise ValueError("rnnoise_amd_audio_score refused the call or failed (include/rnnoise_amd_score.h)")
    return sums


def _db(num, den):
    """10 log10(num / den) with 0 / 0 -> nan, x / 0 -> +inf, 0 / x -> -inf, and a negative side (rounding) as zero"""
    num, den = np.maximum(np.asarray(num, np.float64), 0.0), np.maximum(np.asarray(den, np.float64), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(num / den)


def metrics(sums, frame_terms=None, active=None):
    """Per-sequence metrics from the sums (S, 8) of the score calls, r the clean, x the noisy, y the denoised signal:

      snr_in, snr_out          10 log10(sum r^2 / sum (x - r)^2)  and the same with y
      si_sdr_in, si_sdr_out    10 log10(target / distortion), target = (sum x r)^2 / sum r^2, distortion = sum x^2 - target;
                               the same with y -- the scale-invariant SDR
      snr_gain, si_sdr_gain    out - in
      seg_snr_in, seg_snr_out  with frame_terms (S, T, 8), zeroed before the score call: the mean, over the scored frames (slot 7
                               non-zero) with non-zero clean energy, of the frame's SNR in dB clamped to [-10, 35].  active: (S, T),
                               non-zero where a frame counts (the generator's vad_target, moved to the output frames by the delay);
                               a sequence with no such frame gets nan.

    Sequences with zero clean energy have no such ratio: they are left out -- `kept` is the (S,) bool mask of the others, `excluded`
    their number -- and every array below has kept.sum() entries, in sequence order.  An output equal to the clean signal has no error
    energy: its snr_out, si_sdr_out and both gains are +inf (a frame without error counts as 35 dB in the segmental SNR), and summary()
    averages what it is given, so it reports inf there too.  -> dict"""
    sums = np.asarray(sums, np.float64)
    assert sums.ndim == 2 and sums.shape[1] == SLOTS, sums.shape
    kept = sums[:, 0] > 0
    s = sums[kept]
    out = dict(kept=kept, excluded=int((~kept).sum()), sequences=int(kept.sum()))
    out["snr_in"], out["snr_out"] = _db(s[:, 0], s[:, 5]), _db(s[:, 0], s[:, 6])
    for name, cross, own in (("si_sdr_in", 3, 1), ("si_sdr_out", 4, 2)):
        target = s[:, cross] * s[:, cross] / s[:, 0]
        out[name] = _db(target, s[:, own] - target)
    with np.errstate(invalid="ignore"):
        out["snr_gain"], out["si_sdr_gain"] = out["snr_out"] - out["snr_in"], out["si_sdr_out"] - out["si_sdr_in"]
    if frame_terms is not None:
        ft = np.asarray(frame_terms, np.float64)[kept]
        assert ft.ndim == 3 and ft.shape[2] == SLOTS, ft.shape
        use = (ft[:, :, 7] != 0) & (ft[:, :, 0] > 0)
        if active is not None:
            act = np.asarray(active)[kept]
            assert act.shape == use.shape, (act.shape, use.shape)
            use &= act != 0
        n = use.sum(1)
        for name, err in (("seg_snr_in", 5), ("seg_snr_out", 6)):
            db = np.clip(_db(np.where(use, ft[:, :, 0], 1.0), np.where(use, ft[:, :, err], 1.0)), SEG_MIN_DB, SEG_MAX_DB)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[name] = np.where(use, db, 0.0).sum(1) / n
        out["seg_frames"] = n
    return out


SUMMARY_KEYS = ("snr_in", "snr_out", "snr_gain", "si_sdr_in", "si_sdr_out", "si_sdr_gain", "seg_snr_in", "seg_snr_out")


def summary(m) -> dict:
    """the means over sequences of metrics()' arrays (nan entries -- sequences without a frame for the segmental SNR -- left out of
    their mean), with `sequences` and `excluded`"""
    out = dict(sequences=m["sequences"], excluded=m["excluded"])
    for k in SUMMARY_KEYS:
        if k in m:
            v = m[k][~np.isnan(m[k])]
            with np.errstate(invalid="ignore"):  # (+inf and -inf among them: nan)
                out[k] = float(v.mean()) if v.size else float("nan")
    return out
