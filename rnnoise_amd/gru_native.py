"""ctypes binding of librnnoise_amd_gru.so (include/rnnoise_amd_gru.h): the recurrence of a float GRU layer over a sequence on
hand-written kernels, forward and backward, one launch per step from a loop inside the library.

  gru_sequence_ref(gi, w_hh, b_hh, h0)         the header's formulas in plain torch, any dtype, any device: the tests' reference
  gru_sequence_ref_backward(...)               and the backward formulas likewise
  forward_device / backward_device             the two device calls on raw pointers, asynchronous on a stream
  GruSequence                                  a torch.autograd.Function: y = GruSequence.apply(gi, w_hh, b_hh, h0), gi and y [N, T, .]

What stays torch's: the input projection gi = W_ih x + b_ih (one product over all steps, the caller's F.linear, through which
autograd carries dgi on into W_ih, b_ih and the layer below), and dW_hh, db_hh (one product and one sum over all steps, in
GruSequence.backward).  The library is a separate one: nothing here goes through rnnoise_amd.capi's prototype table.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librnnoise_amd_gru.so")

TILE = 16                 # RNNOISE_AMD_GRU_TILE
MIN_HIDDEN = 16           # RNNOISE_AMD_GRU_MIN_HIDDEN
MAX_HIDDEN = 4096         # RNNOISE_AMD_GRU_MAX_HIDDEN
MAX_ROWS = 1048560        # RNNOISE_AMD_GRU_MAX_ROWS
KERNELS = ("rn_gru_step_kernel", "rn_gru_step_grad_kernel")


class Seq(C.Structure):
    """RNNoiseGruSeq"""
    _fields_ = [("gi", C.c_void_p), ("gi_frame_stride", C.c_long), ("gi_row_stride", C.c_long),
                ("w_hh", C.c_void_p), ("b_hh", C.c_void_p), ("h0", C.c_void_p),
                ("y", C.c_void_p), ("y_frame_stride", C.c_long), ("y_row_stride", C.c_long),
                ("n_rows", C.c_int), ("n_frames", C.c_int), ("hidden", C.c_int)]


class SeqGrad(C.Structure):
    """RNNoiseGruSeqGrad"""
    _fields_ = [("dy", C.c_void_p), ("dy_frame_stride", C.c_long), ("dy_row_stride", C.c_long),
                ("y", C.c_void_p), ("y_frame_stride", C.c_long), ("y_row_stride", C.c_long),
                ("w_hh", C.c_void_p), ("h0", C.c_void_p), ("dhT", C.c_void_p),
                ("dgi", C.c_void_p), ("dgi_frame_stride", C.c_long), ("dgi_row_stride", C.c_long),
                ("dgh", C.c_void_p), ("dh0", C.c_void_p),
                ("n_rows", C.c_int), ("n_frames", C.c_int), ("hidden", C.c_int)]


_int, _vp, _sp = C.c_int, C.c_void_p, C.POINTER(C.c_size_t)
# symbol -> (restype, argtypes), in the header's order; tests/test_gru_native_cpu.py holds the table against the header
PROTOTYPES = {
    "rnnoise_amd_gru_check": (_int, (C.POINTER(Seq),)),
    "rnnoise_amd_gru_grad_check": (_int, (C.POINTER(SeqGrad),)),
    "rnnoise_amd_gru_workspace": (_int, (C.POINTER(Seq), _sp, _sp)),
    "rnnoise_amd_gru_forward_device": (_int, (_int, C.POINTER(Seq), _vp, _vp)),
    "rnnoise_amd_gru_backward_device": (_int, (_int, C.POINTER(SeqGrad), _vp, _vp, _vp)),
}
EXPORTS = list(PROTOTYPES)

def lib():
    return _sidelib.load(LIB_PATH, PROTOTYPES)


def make_seq(gi, w_hh, b_hh, y, n_rows, n_frames, hidden, h0=0) -> Seq:
    """gi, y: (pointer, frame_stride, row_stride) each; w_hh, b_hh, h0: pointers (ints; h0 0: zeros)"""
    c = Seq()
    (c.gi, c.gi_frame_stride, c.gi_row_stride) = (int(gi[0]) or None, int(gi[1]), int(gi[2]))
    (c.y, c.y_frame_stride, c.y_row_stride) = (int(y[0]) or None, int(y[1]), int(y[2]))
    c.w_hh, c.b_hh, c.h0 = int(w_hh) or None, int(b_hh) or None, int(h0) or None
    c.n_rows, c.n_frames, c.hidden = int(n_rows), int(n_frames), int(hidden)
    return c


def make_grad(dy, y, w_hh, dgi, dgh, dh0, n_rows, n_frames, hidden, h0=0, dhT=0) -> SeqGrad:
    """dy, y, dgi: (pointer, frame_stride, row_stride) each; the rest pointers (ints; h0, dhT 0: zeros)"""
    c = SeqGrad()
    (c.dy, c.dy_frame_stride, c.dy_row_stride) = (int(dy[0]) or None, int(dy[1]), int(dy[2]))
    (c.y, c.y_frame_stride, c.y_row_stride) = (int(y[0]) or None, int(y[1]), int(y[2]))
    (c.dgi, c.dgi_frame_stride, c.dgi_row_stride) = (int(dgi[0]) or None, int(dgi[1]), int(dgi[2]))
    c.w_hh, c.h0, c.dhT, c.dgh, c.dh0 = int(w_hh) or None, int(h0) or None, int(dhT) or None, int(dgh) or None, int(dh0) or None
    c.n_rows, c.n_frames, c.hidden = int(n_rows), int(n_frames), int(hidden)
    return c


def check(call) -> bool:
    """whether the device call of `call` (a Seq: forward, a SeqGrad: backward) accepts it; host only, nothing is dereferenced"""
    fn = lib().rnnoise_amd_gru_grad_check if isinstance(call, SeqGrad) else lib().rnnoise_amd_gru_check
    return fn(C.byref(call)) == 0


def workspace(n_rows: int, n_frames: int, hidden: int):
    """(saved_floats, scratch_floats) of a call of these sizes (rnnoise_amd_gru_workspace): T N 4H and 2 N H.  ValueError where the
    library refuses the sizes."""
    return _workspace("librnnoise_amd_gru.so", lib().rnnoise_amd_gru_workspace, Seq, n_rows, n_frames, hidden)


def refusal(n_rows, n_frames, hidden) -> str:
    """why librnnoise_amd_gru.so does not take these sizes (include/rnnoise_amd_gru.h)"""
    return _refusal("librnnoise_amd_gru.so", n_rows, n_frames, hidden)


def _workspace(library, symbol, struct, n_rows, n_frames, hidden):
    """the workspace call `symbol` of `library` on a `struct` of these sizes (the gru stack library's too: the limits are the same)"""
    c = struct()
    c.n_rows, c.n_frames, c.hidden = int(n_rows), int(n_frames), int(hidden)
    saved, scratch = C.c_size_t(0), C.c_size_t(0)
    if symbol(C.byref(c), C.byref(saved), C.byref(scratch)):
        raise ValueError(_refusal(library, n_rows, n_frames, hidden))
    return saved.value, scratch.value


def _refusal(library, n_rows, n_frames, hidden) -> str:
    return (f"{library} takes a hidden size that is a multiple of {TILE} from {MIN_HIDDEN} to {MAX_HIDDEN}, 1 to {MAX_ROWS} "
            f"rows and 0 or more steps: not hidden {hidden}, {n_rows} rows, {n_frames} steps")


def forward_device(call: Seq, d_saved: int, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_gru_forward_device on raw device pointers, asynchronous on `stream` (a hipStream_t handle): n_frames launches"""
    if lib().rnnoise_amd_gru_forward_device(int(device), C.byref(call), d_saved or None, stream or None):
        raise ValueError("rnnoise_amd_gru_forward_device refused the call (include/rnnoise_amd_gru.h: a null or unaligned buffer, "
                         "overlapping slots, sizes out of range) or could not launch")


def backward_device(call: SeqGrad, d_saved: int, d_scratch: int, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_gru_backward_device likewise: n_frames launches from the last step down"""
    if lib().rnnoise_amd_gru_backward_device(int(device), C.byref(call), d_saved or None, d_scratch or None, stream or None):
        raise ValueError("rnnoise_amd_gru_backward_device refused the call (include/rnnoise_amd_gru.h: a null or unaligned buffer, "
                         "overlapping slots, dh0 on dhT, sizes out of range) or could not launch")


# ---- the formulas in plain torch ----
def gru_sequence_ref(gi, w_hh, b_hh, h0=None, return_saved: bool = False):
    """The header's forward formulas: gi [N, T, 3H], w_hh [3H, H], b_hh [3H], h0 [N, H] or None -> y [N, T, H]; with return_saved
    also saved [T, N, 4H] = r, z, n, hn.  Differentiable by torch's autograd; any dtype, any device."""
    import torch
    N, T, H = gi.shape[0], gi.shape[1], w_hh.shape[1]
    h = torch.zeros((N, H), dtype=gi.dtype, device=gi.device) if h0 is None else h0
    ys, saved = [], []
    for t in range(T):
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = torch.tanh(gi[:, t, 2 * H:] + r * hn)
        h = (1 - z) * n + z * h
        ys.append(h)
        saved.append(torch.cat([r, z, n, hn], dim=1))
    y = torch.stack(ys, dim=1) if T else torch.zeros((N, 0, H), dtype=gi.dtype, device=gi.device)
    if return_saved:
        return y, (torch.stack(saved) if T else torch.zeros((0, N, 4 * H), dtype=gi.dtype, device=gi.device))
    return y


def gru_sequence_ref_backward(dy, y, saved, w_hh, h0=None, dhT=None):
    """The header's backward formulas: dy, y [N, T, H], saved [T, N, 4H] -> dgi [N, T, 3H], dW_hh [3H, H], db_hh [3H], dh0 [N, H]"""
    import torch
    N, T, H = y.shape
    dh = torch.zeros((N, H), dtype=y.dtype, device=y.device) if dhT is None else dhT
    zero = torch.zeros((N, H), dtype=y.dtype, device=y.device)
    dgi = torch.zeros((N, T, 3 * H), dtype=y.dtype, device=y.device)
    dW, db = torch.zeros_like(w_hh), torch.zeros((3 * H,), dtype=y.dtype, device=y.device)
    for t in range(T - 1, -1, -1):
        r, z, n, hn = saved[t, :, :H], saved[t, :, H:2 * H], saved[t, :, 2 * H:3 * H], saved[t, :, 3 * H:]
        prev = y[:, t - 1] if t else (zero if h0 is None else h0)
        dh = dh + dy[:, t]
        a_n = dh * (1 - z) * (1 - n * n)
        a_z = dh * (prev - n) * z * (1 - z)
        a_r = a_n * hn * r * (1 - r)
        dgi[:, t] = torch.cat([a_r, a_z, a_n], dim=1)
        dgh = torch.cat([a_r, a_z, a_n * r], dim=1)
        dW = dW + dgh.t() @ prev
        db = db + dgh.sum(0)
        dh = dh * z + dgh @ w_hh
    return dgi, dW, db, dh


# ---- device tensors ----
def _slots(t, width, name):
    """(pointer, frame_stride, row_stride) of a (rows, steps, width) float32 device tensor the kernels can take where it lies"""
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == width):
        raise ValueError(f"{name}: a (rows, steps, {width}) float32 device tensor")
    assert t.stride(2) == 1 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0, name
    return t.data_ptr(), t.stride(1), t.stride(0)


def _fit(t):
    """t, or a contiguous copy where the kernels cannot take it where it lies (16-byte pieces: unit stride inside a slot, slot
    strides that are multiples of 4, an aligned start; a single row or step leaves its stride free, which torch may set to anything)"""
    ok = t.stride(2) == 1 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 and t.data_ptr() % 16 == 0
    ok = ok and t.stride(1) >= t.shape[2] and (t.stride(0) >= t.shape[1] * t.stride(1) or t.stride(1) >= t.shape[0] * t.stride(0))
    return t if ok else t.contiguous()


def _dense(t, shape, name):
    import torch
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: a float32 device tensor of shape {tuple(shape)}")
    return t.contiguous()


def sequence_forward(gi, w_hh, b_hh, h0=None, y=None):
    """The forward call on torch device tensors where they lie: gi [N, T, 3H] (any slot strides the header allows: batch-first
    tensors, or transposed views of frame-major ones), w_hh [3H, H], b_hh [3H], h0 [N, H] or None -> y [N, T, H] (allocated
    contiguous unless given), saved (T N 4H floats).  T launches, asynchronous on torch's current stream."""
    import torch
    H = w_hh.shape[1]
    if gi.dim() != 3 or gi.shape[2] != 3 * H or tuple(w_hh.shape) != (3 * H, H):
        raise ValueError("gi (rows, steps, 3H), w_hh (3H, H), b_hh (3H,)")
    N, T = gi.shape[0], gi.shape[1]
    if not gi.is_cuda:
        raise ValueError("librnnoise_amd_gru.so runs on the device: gi is a CPU tensor (gru_sequence_ref is the formulas in plain torch)")
    n_saved, _ = workspace(N, T, H)
    gi, w, b, h0 = _fit(gi), _dense(w_hh, (3 * H, H), "w_hh"), _dense(b_hh, (3 * H,), "b_hh"), _dense(h0, (N, H), "h0")
    dev = gi.device
    if y is None:
        y = torch.empty((N, T, H), dtype=torch.float32, device=dev)
    saved = torch.empty((max(n_saved, 4),), dtype=torch.float32, device=dev)
    if T:
        call = make_seq(_slots(gi, 3 * H, "gi"), w.data_ptr(), b.data_ptr(), _slots(y, H, "y"), N, T, H, h0.data_ptr() if h0 is not None else 0)
        with torch.cuda.device(dev):
            forward_device(call, saved.data_ptr(), dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
    return y, saved


def sequence_backward(dy, y, saved, w_hh, h0=None, dhT=None, dgi=None):
    """The backward call likewise: dy, y [N, T, H], saved as sequence_forward left it -> dgi [N, T, 3H] (allocated contiguous unless
    given), dgh [T, N, 3H], dh0 [N, H].  T launches."""
    import torch
    N, T, H = y.shape
    dev = y.device
    dy, w, h0, dhT = _fit(dy), _dense(w_hh, (3 * H, H), "w_hh"), _dense(h0, (N, H), "h0"), _dense(dhT, (N, H), "dhT")
    _, n_scratch = workspace(N, T, H)
    if dgi is None:
        dgi = torch.empty((N, T, 3 * H), dtype=torch.float32, device=dev)
    dgh = torch.empty((T, N, 3 * H), dtype=torch.float32, device=dev)
    if T == 0:
        return dgi, dgh, (dhT.clone() if dhT is not None else torch.zeros((N, H), dtype=torch.float32, device=dev))
    dh0 = torch.empty((N, H), dtype=torch.float32, device=dev)
    scratch = torch.empty((n_scratch,), dtype=torch.float32, device=dev)
    call = make_grad(_slots(dy, H, "dy"), _slots(y, H, "y"), w.data_ptr(), _slots(dgi, 3 * H, "dgi"), dgh.data_ptr(), dh0.data_ptr(), N, T, H,
                     h0.data_ptr() if h0 is not None else 0, dhT.data_ptr() if dhT is not None else 0)
    with torch.cuda.device(dev):
        backward_device(call, saved.data_ptr(), scratch.data_ptr(), dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
    return dgi, dgh, dh0


def weight_grads(dgh, y, h0=None, block: int = 256):
    """dW_hh = sum_t dgh[t]^T y[t-1] and db_hh = sum dgh, in torch: dgh [T, N, 3H], y [N, T, H], h0 [N, H] or None (y[-1]).
    A weight's gradient adds T N terms -- 255,488 at the training size.  One float32 product over all of them was measured 9 ulp of
    the largest gradient off at T N = 2,345, where nn.GRU's own stays within one; the same product in float64 is exact enough and
    costs 29 ms a layer at the training size, as much as the backward recurrence.  So: one float32 product per step (N terms each,
    torch.bmm over blocks of `block` steps on y where it lies), the steps' products added in float64 and rounded once."""
    import torch
    T, H = dgh.shape[0], y.shape[2]
    dW = torch.zeros((3 * H, H), dtype=torch.float64, device=dgh.device)
    if T and h0 is not None:
        dW += dgh[0].t() @ h0
    prev = y.transpose(0, 1)  # [T, N, H] as a view: prev[t - 1] is y[t-1]
    for lo in range(1, T, block):
        hi = min(T, lo + block)
        dW += torch.bmm(dgh[lo:hi].transpose(1, 2), prev[lo - 1:hi - 1]).sum(0, dtype=torch.float64)
    return dW.to(dgh.dtype), dgh.sum((0, 1))


def _function():
    import torch

    class GruSequence(torch.autograd.Function):
        """y = GruSequence.apply(gi, w_hh, b_hh, h0): the recurrence of one GRU layer on librnnoise_amd_gru.so.  gi [N, T, 3H] is the
        input projection W_ih x + b_ih, h0 [N, H] or None, y [N, T, H]; y[:, -1] is the final state.  The forward makes T launches and
        keeps saved; the backward makes T launches, then dW_hh and db_hh in torch, and returns dgi, dW_hh, db_hh, dh0.  Float32 device
        tensors only: ValueError on anything else."""

        @staticmethod
        def forward(ctx, gi, w_hh, b_hh, h0=None):
            y, saved = sequence_forward(gi.detach(), w_hh.detach(), b_hh.detach(), None if h0 is None else h0.detach())
            ctx.save_for_backward(y, saved, w_hh, h0)
            return y

        @staticmethod
        def backward(ctx, dy):
            y, saved, w_hh, h0 = ctx.saved_tensors
            dgi, dgh, dh0 = sequence_backward(dy, y, saved, w_hh.detach(), h0)
            dW, db = (None, None)
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                dW, db = weight_grads(dgh, y, h0)
            return dgi, dW, db, (dh0 if h0 is not None and ctx.needs_input_grad[3] else None)

    return GruSequence


_GruSequence = None


def __getattr__(name):  # GruSequence is made on first use: importing this module does not import torch
    global _GruSequence
    if name == "GruSequence":
        if _GruSequence is None:
            _GruSequence = _function()
        return _GruSequence
    raise AttributeError(name)
