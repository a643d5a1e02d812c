"""ctypes binding of librnnoise_amd_fnet.so (include/rnnoise_amd_fnet.h): the float network of a trainer checkpoint as a streaming
runtime on the device -- the two convolutions, the three GRUs and the two heads on this project's own kernels, any cond_size /
gru_size the GRU cell takes, per-row state that lives on the device from call to call.

  FloatNetRuntime(source)   a FloatNet, a state dict or a checkpoint path -> a callable with FloatNet's streaming shape:
                            runtime(features [N, T, 65]) -> (gains [N, T, 32], vad [N, T, 1]), reset(), reset_rows(rows)
  weights(state_dict)       the header's RNNoiseFnetWeights over host copies of the tensors
  check / rows_check / nbytes   the library's host-only calls

Because the call shape and reset() are FloatNet's, RNNoiseOp.denoise_with(runtime, pcm), evaluate.evaluate_audio and the cli's denoise
loop take a runtime where they take a FloatNet.  The library is a separate one: nothing here goes through rnnoise_amd.capi's prototype
table, and no other library knows it.  There is no fallback: what the library does not take raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _sidelib

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librnnoise_amd_fnet.so")

FEATURES, BANDS, LOOKAHEAD = 65, 32, 4  # RNNOISE_AMD_FNET_FEATURES, _BANDS, _LOOKAHEAD
MIN_COND, MAX_COND = 16, 1024           # RNNOISE_AMD_FNET_MIN_COND, _MAX_COND
MIN_GRU, MAX_GRU = 16, 4096             # RNNOISE_AMD_FNET_MIN_GRU, _MAX_GRU
MAX_ROWS = 1048560                      # RNNOISE_AMD_FNET_MAX_ROWS
MAX_FRAMES = 4096                       # RNNOISE_AMD_FNET_MAX_FRAMES
KERNELS = ("rn_fnet_reset_kernel", "rn_fnet_gather_kernel", "rn_fnet_conv1_kernel", "rn_fnet_conv2_kernel", "rn_fnet_gru_kernel",
           "rn_fnet_heads_kernel")

_fp = C.c_void_p  # (a const float *: the tables hold plain addresses)


class Rows(C.Structure):
    """RNNoiseFnetRows: frame t of row s at base + t * frame_stride + s * row_stride, in floats; {0, 0}: [frame][n_rows][row]"""
    _fields_ = [("frame_stride", C.c_long), ("row_stride", C.c_long)]


class Weights(C.Structure):
    """RNNoiseFnetWeights: host pointers to the trainer's tensors in torch's layouts"""
    _fields_ = [("cond_size", C.c_int), ("gru_size", C.c_int),
                ("conv1_weight", _fp), ("conv1_bias", _fp), ("conv2_weight", _fp), ("conv2_bias", _fp),
                ("gru_weight_ih", _fp * 3), ("gru_weight_hh", _fp * 3), ("gru_bias_ih", _fp * 3), ("gru_bias_hh", _fp * 3),
                ("dense_out_weight", _fp), ("dense_out_bias", _fp), ("vad_dense_weight", _fp), ("vad_dense_bias", _fp)]


_int, _ll, _vp, _wp, _rp = C.c_int, C.c_longlong, C.c_void_p, C.POINTER(Weights), C.POINTER(Rows)
# symbol -> (restype, argtypes), in the header's order; tests/test_fnet_cpu.py holds the table against the header
PROTOTYPES = {
    "rnnoise_amd_fnet_check": (_int, (_wp, _int, _int)),
    "rnnoise_amd_fnet_rows_check": (_int, (_rp, _int, _int, _int)),
    "rnnoise_amd_fnet_bytes": (_ll, (_int, _int, _int, _int)),
    "rnnoise_amd_fnet_create": (_vp, (_int, _wp, _int, _int)),
    "rnnoise_amd_fnet_destroy": (None, (_vp,)),
    "rnnoise_amd_fnet_reset": (_int, (_vp, _vp)),
    "rnnoise_amd_fnet_reset_rows_device": (_int, (_vp, _vp, _int, _vp)),
    "rnnoise_amd_fnet_reset_rows": (_int, (_vp, C.POINTER(C.c_int), _int)),
    "rnnoise_amd_fnet_process_device": (_int, (_vp, _vp, _rp, _vp, _rp, _vp, _rp, _int, _vp)),
    "rnnoise_amd_fnet_process": (_int, (_vp, _vp, _rp, _vp, _rp, _vp, _rp, _int)),
}
EXPORTS = list(PROTOTYPES)

# the state dict's names, in the order of Weights' pointers
_SINGLE = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")
_HEADS = ("dense_out.weight", "dense_out.bias", "vad_dense.weight", "vad_dense.bias")
_GRU = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
TENSORS = _SINGLE + tuple(f"gru{l}.{n}" for n in _GRU for l in (1, 2, 3)) + _HEADS


def lib():
    return _sidelib.load(LIB_PATH, PROTOTYPES)


def weights(state_dict):
    """(Weights, the float32 numpy arrays it points into -- keep them while the struct is in use) of a trainer state dict (torch
    tensors or numpy arrays); the dimensions are read off the tensors.  ValueError for a missing tensor or a shape that does not fit."""
    missing = [n for n in TENSORS if n not in state_dict]
    if missing:
        raise ValueError(f"state dict lacks {missing}")
    host = {}
    for n in TENSORS:
        v = state_dict[n]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        host[n] = np.ascontiguousarray(v, dtype=np.float32)
    cond, gru = host["conv1.weight"].shape[0], host["conv2.weight"].shape[0]
    shapes = {"conv1.weight": (cond, FEATURES, 3), "conv1.bias": (cond,), "conv2.weight": (gru, cond, 3), "conv2.bias": (gru,),
              "dense_out.weight": (BANDS, 4 * gru), "dense_out.bias": (BANDS,), "vad_dense.weight": (1, 4 * gru), "vad_dense.bias": (1,)}
    for l in (1, 2, 3):
        shapes.update({f"gru{l}.weight_ih_l0": (3 * gru, gru), f"gru{l}.weight_hh_l0": (3 * gru, gru), f"gru{l}.bias_ih_l0": (3 * gru,),
                       f"gru{l}.bias_hh_l0": (3 * gru,)})
    for n, want in shapes.items():
        if host[n].shape != want:
            raise ValueError(f"{n}: shape {host[n].shape}, not {want}")
    p = lambda n: host[n].ctypes.data
    w = Weights(cond, gru, p("conv1.weight"), p("conv1.bias"), p("conv2.weight"), p("conv2.bias"),
                *[(_fp * 3)(*[p(f"gru{l}.{n}") for l in (1, 2, 3)]) for n in _GRU],
                p("dense_out.weight"), p("dense_out.bias"), p("vad_dense.weight"), p("vad_dense.bias"))
    return w, host


def check(w: Weights, n_rows: int, max_frames: int) -> bool:
    """whether rnnoise_amd_fnet_create accepts the arguments (host only, nothing is dereferenced)"""
    return lib().rnnoise_amd_fnet_check(C.byref(w), int(n_rows), int(max_frames)) == 0


def rows_check(rows, row_floats: int, n_rows: int, n_frames: int) -> bool:
    """whether the process calls accept (frame_stride, row_stride) -- None: the default -- for rows of row_floats floats"""
    r = None if rows is None else C.byref(Rows(int(rows[0]), int(rows[1])))
    return lib().rnnoise_amd_fnet_rows_check(r, int(row_floats), int(n_rows), int(n_frames)) == 1


def bytes_formula(cond: int, gru: int, n_rows: int, max_frames: int) -> int:
    """the header's formula for the device bytes of a runtime"""
    C_, H, N, M = cond, gru, n_rows, max_frames
    weights_ = 4 * (196 * C_ + C_ + 3 * C_ * H + H + 18 * H * H + 18 * H + 48 * 4 * H + 48)
    state = 4 * (65 * (M + 4) * N + 3 * N * H) + 8 * N
    work = 4 * ((M + 2) * N * C_ + 4 * M * N * H + 12 * N * H + N)
    return weights_ + state + work


def nbytes(cond: int, gru: int, n_rows: int, max_frames: int) -> int:
    """rnnoise_amd_fnet_bytes; ValueError outside the limits"""
    n = lib().rnnoise_amd_fnet_bytes(int(cond), int(gru), int(n_rows), int(max_frames))
    if n < 0:
        raise ValueError(f"rnnoise_amd_fnet_bytes: cond_size {cond}, gru_size {gru}, {n_rows} rows, max_frames {max_frames} are outside the limits "
                         f"(multiples of 16 in {MIN_COND} .. {MAX_COND} and {MIN_GRU} .. {MAX_GRU}, 1 .. {MAX_ROWS}, 1 .. {MAX_FRAMES})")
    return n


def launches_formula(n_frames: int, max_frames: int, seen: int) -> int:
    """the header's formula for the launches of a process call on a runtime every row of which has had `seen` frames since the last
    reset of all rows"""
    n = 0
    for t0 in range(0, n_frames, max_frames):
        T = min(max_frames, n_frames - t0)
        G = T - min(T, max(0, LOOKAHEAD - (seen + t0)))
        n += 4 + (G + 2 if G > 0 else 0)
    return n


def _rows_of(t):
    """Rows of a [N, T, W] tensor read where it lies: frames at stride(1), rows at stride(0); a dimension of one gets the stride a
    dense tensor would have (torch leaves it arbitrary)"""
    N, T, W = t.shape
    fs = t.stride(1) if T > 1 else W
    rs = t.stride(0) if N > 1 else max(fs * T, W)
    return Rows(fs, rs)


class FloatNetRuntime:
    """The streaming float network on librnnoise_amd_fnet.so, with FloatNet.forward's call shape.

    source: a float_net.FloatNet (or any module with its parameter names), a state dict, or a checkpoint path (a .pth with
    'state_dict', or a bare state dict); the dimensions are read off the tensors.  The weights are copied when the runtime is made:
    later changes of the module do not reach it.  device: the HIP device (int, or a torch device); None: that of the first features.
    max_frames: the frames a piece of a call holds in the workspace -- a longer call cuts itself into pieces, and no float depends on
    it.  The device runtime is created on the first call and again when the number of rows changes, as FloatNet.forward starts over
    then."""

    def __init__(self, source, device=None, max_frames: int = 16):
        if isinstance(source, (str, os.PathLike)):
            import torch
            sd = torch.load(os.fspath(source), map_location="cpu")
            sd = sd["state_dict"] if "state_dict" in sd else sd
        elif hasattr(source, "state_dict"):
            sd = source.state_dict()
        else:
            sd = source
        self._w, self._host = weights(sd)
        self.cond_size, self.gru_size = self._w.cond_size, self._w.gru_size
        if not 1 <= int(max_frames) <= MAX_FRAMES:
            raise ValueError(f"max_frames: 1 .. {MAX_FRAMES}, not {max_frames}")
        self.max_frames = int(max_frames)
        if device is not None and not isinstance(device, int):
            import torch
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError(f"FloatNetRuntime runs on the device, not on {device}: use float_net.FloatNet there")
            device = device.index or 0
        self.device = device
        self._h, self._n = None, 0

    # ---- the device runtime ----
    def _ensure(self, n, device):
        if self._h is not None and self._n == n and self._at == device:
            return
        self.close()
        if not check(self._w, n, self.max_frames):
            raise ValueError(f"librnnoise_amd_fnet.so refuses cond_size {self.cond_size}, gru_size {self.gru_size}, {n} rows, max_frames "
                             f"{self.max_frames} (include/rnnoise_amd_fnet.h: multiples of 16 in {MIN_COND} .. {MAX_COND} and {MIN_GRU} .. "
                             f"{MAX_GRU}, 1 .. {MAX_ROWS} rows)")
        h = lib().rnnoise_amd_fnet_create(device, C.byref(self._w), n, self.max_frames)
        if not h:
            raise RuntimeError(f"rnnoise_amd_fnet_create failed on device {device} ({nbytes(self.cond_size, self.gru_size, n, self.max_frames)} bytes)")
        self._h, self._n, self._at = h, n, device

    def open(self, n_rows: int, device: int = None):
        """the device runtime for n_rows rows now, every row at the start of a sequence, instead of on the first call"""
        self._ensure(int(n_rows), self.device or 0 if device is None else int(device))
        return self

    def process_device(self, d_gains: int, gain_rows, d_vad: int, vad_rows, d_features: int, feat_rows, n_frames: int, stream: int = 0) -> int:
        """rnnoise_amd_fnet_process_device on raw device pointers (ints) of an open runtime; *_rows: (frame_stride, row_stride) or
        None for the default [frame][n_rows][row] -> the call's return value"""
        r = [None if x is None else C.byref(Rows(int(x[0]), int(x[1]))) for x in (gain_rows, vad_rows, feat_rows)]
        return lib().rnnoise_amd_fnet_process_device(self._h, d_gains or None, r[0], d_vad or None, r[1], d_features or None, r[2], int(n_frames),
                                                     stream or None)

    def process_host(self, features):
        """rnnoise_amd_fnet_process, the library's host form, on an open runtime: features (T, N, 65) float32 numpy, dense ->
        gains (T, N, 32), vad (T, N)"""
        f = np.ascontiguousarray(features, dtype=np.float32)
        T, N = f.shape[0], f.shape[1]
        if f.shape != (T, self._n, FEATURES):
            raise ValueError(f"features: (T, {self._n}, 65), not {f.shape}")
        gains, vad = np.zeros((T, N, BANDS), np.float32), np.zeros((T, N), np.float32)
        if lib().rnnoise_amd_fnet_process(self._h, gains.ctypes.data, None, vad.ctypes.data, None, f.ctypes.data, None, T):
            raise RuntimeError("rnnoise_amd_fnet_process refused the call or failed")
        return gains, vad

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().rnnoise_amd_fnet_destroy(self._h)
        self._h, self._n = None, 0

    def __del__(self):
        try:
            self.close()
        except Exception:  # (the interpreter is going down: the process takes the device memory with it)
            pass

    def _stream(self):
        import torch
        return torch.cuda.current_stream(torch.device("cuda", self._at)).cuda_stream

    # ---- FloatNet's streaming shape ----
    def reset(self):
        """a new sequence for every row (asynchronous, on torch's current stream of the runtime's device)"""
        if self._h is not None and lib().rnnoise_amd_fnet_reset(self._h, self._stream() or None):
            raise RuntimeError("rnnoise_amd_fnet_reset failed")

    def reset_rows(self, rows):
        """a new sequence for the listed rows only: an int32 device tensor (asynchronous, read where it lies), or any sequence of ints
        (the library's host form, synchronous).  Before the first call there is nothing to reset."""
        if self._h is None:
            return
        if hasattr(rows, "is_cuda"):
            import torch
            if not rows.is_cuda or rows.dtype != torch.int32 or rows.dim() != 1 or (rows.numel() > 1 and rows.stride(0) != 1):
                raise ValueError("reset_rows: a dense 1-d int32 tensor on the device, or a sequence of ints")
            rc = lib().rnnoise_amd_fnet_reset_rows_device(self._h, rows.data_ptr() or None, rows.numel(), self._stream() or None)
        else:
            a = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1), dtype=np.int32)
            rc = lib().rnnoise_amd_fnet_reset_rows(self._h, a.ctypes.data_as(C.POINTER(C.c_int)), a.size)
        if rc:
            raise ValueError(f"reset_rows: the library refused the list (at most {self._n} entries)")

    def __call__(self, features):
        """features [N, T, 65] float32 on the device, any strides with contiguous rows -> gains [N, T, 32], vad [N, T, 1]"""
        import torch
        if not isinstance(features, torch.Tensor) or not features.is_cuda or features.dtype != torch.float32:
            kind = f"{features.dtype} on {features.device}" if isinstance(features, torch.Tensor) else type(features).__name__
            raise ValueError(f"FloatNetRuntime runs float32 tensors on the device, not {kind}: there is no fallback (float_net.FloatNet "
                             "runs anywhere)")
        if features.dim() != 3 or features.shape[2] != FEATURES:
            raise ValueError(f"features: [N, T, 65], not {tuple(features.shape)}")
        if self.device is not None and features.device.index != self.device:
            raise ValueError(f"features on {features.device}, the runtime on cuda:{self.device}")
        N, T = features.shape[0], features.shape[1]
        if features.stride(2) != 1 and T * N > 0:
            features = features.contiguous()
        self._ensure(N, features.device.index)
        gains = torch.empty((N, T, BANDS), device=features.device, dtype=torch.float32)
        vad = torch.empty((N, T, 1), device=features.device, dtype=torch.float32)
        if T == 0:
            return gains, vad
        fr = _rows_of(features)
        if not rows_check((fr.frame_stride, fr.row_stride), FEATURES, N, T):
            features = features.contiguous()
            fr = _rows_of(features)
        with torch.cuda.device(features.device):
            rc = lib().rnnoise_amd_fnet_process_device(self._h, gains.data_ptr(), C.byref(_rows_of(gains)), vad.data_ptr(), C.byref(_rows_of(vad)),
                                                       features.data_ptr(), C.byref(fr), T, self._stream() or None)
        if rc:
            raise RuntimeError("rnnoise_amd_fnet_process_device refused the call or could not launch (include/rnnoise_amd_fnet.h)")
        return gains, vad

    forward = __call__
