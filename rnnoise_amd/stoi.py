"""ctypes binding of librnnoise_amd_stoi.so (include/rnnoise_amd_stoi.h): STOI and ESTOI of denoised PCM against the clean signal on
the device -- eight doubles per sequence, by a definition and in an order the header fixes -- and the measures read off them.

  score_device(...)   raw device pointers, asynchronous on a stream: the planes where they lie, through strides, scratch from the caller
  score(...)          torch device tensors (in slabs of rows, scratch below SCRATCH_CAP) or numpy arrays (the library's host form)
  metrics(results)    stoi_in, stoi_out, estoi_in, estoi_out per sequence, and their means

The library is a separate one: nothing here goes through rnnoise_amd.capi's prototype table, and no other library knows it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librnnoise_amd_stoi.so")

FRAME = 480         # RNNOISE_AMD_STOI_FRAME
SLOTS = 8           # RNNOISE_AMD_STOI_SLOTS: STOI sum, ESTOI sum, segments, kept frames of in / ref; the same of out / ref
MAX_ROWS = 32768    # RNNOISE_AMD_STOI_MAX_ROWS
MAX_FRAMES = 8192   # RNNOISE_AMD_STOI_MAX_FRAMES
DELAY = 960         # samples by which the denoiser delays its input (rnnoise_amd_score.h)
SCRATCH_CAP = 1 << 30  # bytes of scratch score() takes at a time on the device: it cuts the rows into slabs below it (one row at least)
KERNELS = ("rn_stoi_resample_kernel", "rn_stoi_keep_kernel", "rn_stoi_bands_kernel", "rn_stoi_segments_kernel", "rn_stoi_sum_kernel")


class Plane(C.Structure):
    """RNNoiseStoiPlane: sample i of frame t of row s at p[t * frame_stride + s * row_stride + i], strides in floats"""
    _fields_ = [("p", C.c_void_p), ("frame_stride", C.c_long), ("row_stride", C.c_long)]


class Call(C.Structure):
    """RNNoiseStoi"""
    _fields_ = [("ref", Plane), ("in_", Plane), ("out", Plane), ("n_rows", C.c_int), ("n_frames", C.c_int), ("first", C.c_int),
                ("delay", C.c_int)]


_int, _ll, _vp, _dp = C.c_int, C.c_longlong, C.c_void_p, C.POINTER(C.c_double)
# symbol -> (restype, argtypes), in the header's order; tests/test_stoi_cpu.py holds the table against the header
PROTOTYPES = {
    "rnnoise_amd_stoi_check": (_int, (C.POINTER(Call),)),
    "rnnoise_amd_stoi_workspace": (_ll, (_int, _int)),
    "rnnoise_amd_stoi_device": (_int, (_int, _vp, _vp, _ll, C.POINTER(Call), _vp)),
    "rnnoise_amd_stoi": (_int, (_int, _dp, C.POINTER(Call))),
}
EXPORTS = list(PROTOTYPES)


def lib():
    return _sidelib.load(LIB_PATH, PROTOTYPES)


def make_call(ref, inp, out, n_rows, n_frames, first=2, delay=DELAY) -> Call:
    """ref, inp, out: (pointer, frame_stride, row_stride) each, the pointer an int; inp None or with a 0 pointer: no noisy plane"""
    planes = [Plane(int(p) or None, int(fs), int(rs)) for p, fs, rs in (ref, inp or (0, 0, 0), out)]
    return Call(*planes, int(n_rows), int(n_frames), int(first), int(delay))


def check(call: Call) -> bool:
    """whether the calls accept `call` (rnnoise_amd_stoi_check; host only, nothing is dereferenced)"""
    return lib().rnnoise_amd_stoi_check(C.byref(call)) == 0


def workspace_formula(n_rows: int, n_frames: int) -> int:
    """the header's formula for the scratch of the device form, in bytes"""
    c = 100 * n_frames
    g = 0 if c < 256 else (c - 256) // 128 + 1
    return n_rows * (8 * (3 * c + 50 * g) + 4 * (g + g % 2) + 8)


def workspace(n_rows: int, n_frames: int) -> int:
    """rnnoise_amd_stoi_workspace: bytes of scratch for n_rows rows of n_frames frames; ValueError outside the limits"""
    n = lib().rnnoise_amd_stoi_workspace(int(n_rows), int(n_frames))
    if n < 0:
        raise ValueError(f"rnnoise_amd_stoi_workspace: {n_rows} rows of {n_frames} frames are outside the limits ({MAX_ROWS}, {MAX_FRAMES})")
    return n


def score_device(d_results: int, d_scratch: int, scratch_bytes: int, ref, inp, out, n_rows: int, n_frames: int, first: int = 2,
                 delay: int = DELAY, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_stoi_device on raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle): WRITES d_results
    [n_rows][8] float64.  ref, inp, out: (pointer, frame_stride, row_stride) each; inp None: slots 0..3 are zeros.  ValueError where
    the library refuses the arguments."""
    call = make_call(ref, inp, out, n_rows, n_frames, first, delay)
    if lib().rnnoise_amd_stoi_device(int(device), d_results or None, d_scratch or None, int(scratch_bytes), C.byref(call), stream or None):
        raise ValueError("rnnoise_amd_stoi_device refused the call (include/rnnoise_amd_stoi.h: a null or unaligned plane, a stride below "
                         "480 or no multiple of 4, first * 480 < delay, sizes beyond the limits, scratch too small) or could not launch")


def _host_plane(a, name):
    """(pointer, frame_stride, row_stride) of a (T, N, 480) float32 array or view whose samples are contiguous"""
    if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == FRAME):
        raise ValueError(f"{name}: a (frames, rows, 480) float32 array")
    if a.strides[2] != 4 or a.strides[0] % 16 or a.strides[1] % 16 or a.ctypes.data % 16:
        raise ValueError(f"{name}: contiguous samples, strides that are multiples of 4 floats and a 16-byte aligned base")
    return a.ctypes.data, a.strides[0] // 4, a.strides[1] // 4


def _device_plane(t, name):
    import torch
    if not (t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == FRAME and t.stride(2) == 1):
        raise ValueError(f"{name}: a (frames, rows, 480) float32 tensor with contiguous samples")
    return t.data_ptr(), t.stride(0), t.stride(1)


def score(ref, inp, out, n_frames=None, first: int = 2, delay: int = DELAY, device: int = 0, scratch_cap: int = SCRATCH_CAP):
    """The eight doubles of every row -> (N, 8) float64 numpy array.  ref, inp, out: (T, N, 480) float32, all three torch tensors on
    cuda:`device` or all three numpy arrays -- any strides the header allows; a stream-contiguous (N, T * 480) array `a` goes in as
    a.reshape(N, T, 480).transpose(1, 0, 2) --; inp may be None.  n_frames: the frames of a sequence (None: all T of out).  Device
    tensors are scored where they lie, the rows in slabs whose scratch stays below scratch_cap bytes (one row at least); numpy arrays go
    through the library's host form."""
    T, N = out.shape[0], out.shape[1]
    n_frames = T if n_frames is None else int(n_frames)
    for a in (ref, inp, out):
        if a is not None and (a.shape[1] != N or a.shape[0] < n_frames):
            raise ValueError("ref / inp / out: the same rows and at least n_frames frames")
    if isinstance(out, np.ndarray):
        planes = [_host_plane(a, n) if a is not None else None for a, n in ((ref, "ref"), (inp, "inp"), (out, "out"))]
        res = np.zeros((N, SLOTS), np.float64)
        call = make_call(*planes, N, n_frames, first, delay)
        if lib().rnnoise_amd_stoi(int(device), res.ctypes.data_as(_dp), C.byref(call)):
            raise ValueError("rnnoise_amd_stoi refused the call or failed (include/rnnoise_amd_stoi.h)")
        return res
    import torch
    planes = [_device_plane(a, n) if a is not None else None for a, n in ((ref, "ref"), (inp, "inp"), (out, "out"))]
    slab = max(1, min(N, MAX_ROWS, scratch_cap // max(1, workspace(1, n_frames))))
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        nbytes = workspace(slab, n_frames)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        res = torch.empty((N, SLOTS), dtype=torch.float64, device=dev)
        for r0 in range(0, N, slab):
            rows = min(slab, N - r0)
            at = [None if p is None else (p[0] + 4 * r0 * p[2], p[1], p[2]) for p in planes]
            score_device(res[r0:].data_ptr(), scratch.data_ptr(), nbytes, *at, rows, n_frames, first, delay, device, st.cuda_stream)
        return res.cpu().numpy()  # (waits for the stream)


METRIC_KEYS = ("stoi_in", "stoi_out", "estoi_in", "estoi_out")


def metrics(results) -> dict:
    """From the (S, 8) results of the calls: stoi_in, stoi_out, estoi_in, estoi_out per sequence -- sum / segments, NaN for a
    sequence without a segment (fewer than 31 kept frames) and for the in side of a call without a noisy plane -- and `summary`: their
    means over the sequences that have a segment, with `sequences` (those) and `excluded` (the others)."""
    r = np.asarray(results, np.float64)
    assert r.ndim == 2 and r.shape[1] == SLOTS, r.shape
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, s, n in (("stoi_in", 0, 2), ("estoi_in", 1, 2), ("stoi_out", 4, 6), ("estoi_out", 5, 6)):
            out[name] = np.where(r[:, n] > 0, r[:, s] / r[:, n], np.nan)
    kept = r[:, 6] > 0
    summary = dict(sequences=int(kept.sum()), excluded=int((~kept).sum()))
    for k in METRIC_KEYS:
        v = out[k][kept & (r[:, 2 if k.endswith("_in") else 6] > 0)]
        summary[k] = float(v.mean()) if v.size else float("nan")
    out["kept"], out["summary"] = kept, summary
    return out
