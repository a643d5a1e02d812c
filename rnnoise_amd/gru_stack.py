"""ctypes binding of librnnoise_amd_gru_stack.so (include/rnnoise_amd_gru_stack.h): the network's three chained GRU layers on
hand-written kernels as one diagonal launch a step -- layer 1 at step t, layer 2 at t - 1, layer 3 at t - 2 in one grid, T + 2 launches
each way from a loop inside the library.

  gru_stack_ref(gi0, w_ih, b_ih, w_hh, b_hh, h0)   the header's formulas in plain torch, any dtype, any device: the tests' reference
  gru_stack_ref_backward(...)                      and the backward formulas likewise
  forward_device / backward_device                 the two device calls on raw pointers, asynchronous on a stream
  stack_forward / stack_backward                   the same on torch device tensors where they lie
  GruStack                                         a torch.autograd.Function:
                                                   y1, y2, y3 = GruStack.apply(gi0, w_ih2, b_ih2, w_ih3, b_ih3, w_hh1, w_hh2, w_hh3,
                                                                               b_hh1, b_hh2, b_hh3, h01, h02, h03)

What stays torch's: layer 1's input projection gi0 = W_ih x + b_ih (one product over all steps, the caller's F.linear, through which
autograd carries dgi0 on), and every weight gradient (dW_hh, db_hh of the three layers, dW_ih, db_ih of layers 2 and 3: products and
sums over all steps, in GruStack.backward).  The library is a separate one: nothing here goes through rnnoise_amd.capi's prototype
table, and nothing through librnnoise_amd_gru.so.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib, gru_native

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librnnoise_amd_gru_stack.so")

LAYERS = 3                # RNNOISE_AMD_GRU_STACK_LAYERS
TILE = 16                 # RNNOISE_AMD_GRU_STACK_TILE
MIN_HIDDEN = 16           # RNNOISE_AMD_GRU_STACK_MIN_HIDDEN
MAX_HIDDEN = 4096         # RNNOISE_AMD_GRU_STACK_MAX_HIDDEN
MAX_ROWS = 1048560        # RNNOISE_AMD_GRU_STACK_MAX_ROWS
KERNELS = ("rn_gru_stack_kernel", "rn_gru_stack_grad_kernel")

_p3, _l3 = C.c_void_p * 3, C.c_long * 3


class Stack(C.Structure):
    """RNNoiseGruStack"""
    _fields_ = [("gi0", C.c_void_p), ("gi0_frame_stride", C.c_long), ("gi0_row_stride", C.c_long),
                ("w_ih", _p3), ("b_ih", _p3), ("w_hh", _p3), ("b_hh", _p3), ("h0", _p3),
                ("y", _p3), ("y_frame_stride", _l3), ("y_row_stride", _l3),
                ("n_rows", C.c_int), ("n_frames", C.c_int), ("hidden", C.c_int)]


class StackGrad(C.Structure):
    """RNNoiseGruStackGrad"""
    _fields_ = [("dy", _p3), ("dy_frame_stride", _l3), ("dy_row_stride", _l3),
                ("y", _p3), ("y_frame_stride", _l3), ("y_row_stride", _l3),
                ("w_ih", _p3), ("w_hh", _p3), ("h0", _p3), ("dhT", _p3),
                ("dgi", _p3), ("dgi0_frame_stride", C.c_long), ("dgi0_row_stride", C.c_long),
                ("dgh", _p3), ("dh0", _p3),
                ("n_rows", C.c_int), ("n_frames", C.c_int), ("hidden", C.c_int)]


_int, _vp, _sp = C.c_int, C.c_void_p, C.POINTER(C.c_size_t)
# symbol -> (restype, argtypes), in the header's order; tests/test_gru_stack_cpu.py holds the table against the header
PROTOTYPES = {
    "rnnoise_amd_gru_stack_check": (_int, (C.POINTER(Stack),)),
    "rnnoise_amd_gru_stack_grad_check": (_int, (C.POINTER(StackGrad),)),
    "rnnoise_amd_gru_stack_workspace": (_int, (C.POINTER(Stack), _sp, _sp)),
    "rnnoise_amd_gru_stack_forward_device": (_int, (_int, C.POINTER(Stack), _vp, _vp)),
    "rnnoise_amd_gru_stack_backward_device": (_int, (_int, C.POINTER(StackGrad), _vp, _vp, _vp)),
}
EXPORTS = list(PROTOTYPES)

def lib():
    return _sidelib.load(LIB_PATH, PROTOTYPES)


def _ptrs(values):
    """three pointers (ints; 0 or None: NULL) as a C array"""
    assert len(values) == LAYERS
    return _p3(*[int(v) if v else None for v in values])


def _triples(slots):
    """three (pointer, frame_stride, row_stride) as three C arrays"""
    assert len(slots) == LAYERS
    return _ptrs([s[0] for s in slots]), _l3(*[int(s[1]) for s in slots]), _l3(*[int(s[2]) for s in slots])


def make_stack(gi0, w_ih, b_ih, w_hh, b_hh, y, n_rows, n_frames, hidden, h0=(0, 0, 0)) -> Stack:
    """gi0: (pointer, frame_stride, row_stride); y: three of them; w_ih, b_ih, w_hh, b_hh, h0: three pointers each (ints; w_ih[0],
    b_ih[0] are not looked at; h0 0: zeros)"""
    c = Stack()
    (c.gi0, c.gi0_frame_stride, c.gi0_row_stride) = (int(gi0[0]) or None, int(gi0[1]), int(gi0[2]))
    c.w_ih, c.b_ih, c.w_hh, c.b_hh, c.h0 = _ptrs(w_ih), _ptrs(b_ih), _ptrs(w_hh), _ptrs(b_hh), _ptrs(h0)
    c.y, c.y_frame_stride, c.y_row_stride = _triples(y)
    c.n_rows, c.n_frames, c.hidden = int(n_rows), int(n_frames), int(hidden)
    return c


def make_grad(dy, y, w_ih, w_hh, dgi0, dgi, dgh, dh0, n_rows, n_frames, hidden, h0=(0, 0, 0), dhT=(0, 0, 0)) -> StackGrad:
    """dy, y: three (pointer, frame_stride, row_stride) each; dgi0: one; dgi: (ignored, dgi[1], dgi[2]) dense; the rest three
    pointers each (ints; h0, dhT 0: zeros)"""
    c = StackGrad()
    c.dy, c.dy_frame_stride, c.dy_row_stride = _triples(dy)
    c.y, c.y_frame_stride, c.y_row_stride = _triples(y)
    c.w_ih, c.w_hh, c.h0, c.dhT = _ptrs(w_ih), _ptrs(w_hh), _ptrs(h0), _ptrs(dhT)
    c.dgi = _ptrs([dgi0[0], dgi[1], dgi[2]])
    c.dgi0_frame_stride, c.dgi0_row_stride = int(dgi0[1]), int(dgi0[2])
    c.dgh, c.dh0 = _ptrs(dgh), _ptrs(dh0)
    c.n_rows, c.n_frames, c.hidden = int(n_rows), int(n_frames), int(hidden)
    return c


def check(call) -> bool:
    """whether the device call of `call` (a Stack: forward, a StackGrad: backward) accepts it; host only, nothing is dereferenced"""
    fn = lib().rnnoise_amd_gru_stack_grad_check if isinstance(call, StackGrad) else lib().rnnoise_amd_gru_stack_check
    return fn(C.byref(call)) == 0


def workspace(n_rows: int, n_frames: int, hidden: int):
    """(saved_floats, scratch_floats) of a call of these sizes (rnnoise_amd_gru_stack_workspace): 3 T N 4H and (3 + 2) 2 N H.
    ValueError where the library refuses the sizes."""
    return gru_native._workspace("librnnoise_amd_gru_stack.so", lib().rnnoise_amd_gru_stack_workspace, Stack, n_rows, n_frames, hidden)


def refusal(n_rows, n_frames, hidden) -> str:
    """why librnnoise_amd_gru_stack.so does not take these sizes (include/rnnoise_amd_gru_stack.h: the gru library's limits)"""
    return gru_native._refusal("librnnoise_amd_gru_stack.so", n_rows, n_frames, hidden)


def forward_device(call: Stack, d_saved: int, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_gru_stack_forward_device on raw device pointers, asynchronous on `stream` (a hipStream_t handle): n_frames + 2
    launches"""
    if lib().rnnoise_amd_gru_stack_forward_device(int(device), C.byref(call), d_saved or None, stream or None):
        raise ValueError("rnnoise_amd_gru_stack_forward_device refused the call (include/rnnoise_amd_gru_stack.h: a null or unaligned "
                         "buffer, overlapping slots or outputs, sizes out of range) or could not launch")


def backward_device(call: StackGrad, d_saved: int, d_scratch: int, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_gru_stack_backward_device likewise: n_frames + 2 launches from the last step down"""
    if lib().rnnoise_amd_gru_stack_backward_device(int(device), C.byref(call), d_saved or None, d_scratch or None, stream or None):
        raise ValueError("rnnoise_amd_gru_stack_backward_device refused the call (include/rnnoise_amd_gru_stack.h: a null or unaligned "
                         "buffer, overlapping slots, dh0 on dhT, sizes out of range) or could not launch")


# ---- the formulas in plain torch ----
def gru_stack_ref(gi0, w_ih, b_ih, w_hh, b_hh, h0=(None, None, None), return_saved: bool = False):
    """The header's forward formulas: gi0 [N, T, 3H]; w_ih, b_ih, w_hh, b_hh, h0: three each (w_ih[0], b_ih[0] are not looked at; h0
    None: zeros) -> [y1, y2, y3], each [N, T, H]; with return_saved also saved [3, T, N, 4H].  Differentiable by torch's autograd; any
    dtype, any device."""
    import torch
    ys, saved, gi = [], [], gi0
    for l in range(LAYERS):
        if l:
            gi = torch.nn.functional.linear(ys[l - 1], w_ih[l], b_ih[l])
        y, s = gru_native.gru_sequence_ref(gi, w_hh[l], b_hh[l], h0[l], return_saved=True)
        ys.append(y)
        saved.append(s)
    return (ys, torch.stack(saved)) if return_saved else ys


def gru_stack_ref_backward(dy, y, saved, w_ih, w_hh, h0=(None, None, None), dhT=(None, None, None)):
    """The header's backward formulas: dy, y: three [N, T, H] each, saved [3, T, N, 4H] -> a dict of dgi (three [N, T, 3H]; dgi[0] is
    what goes back into the caller's projection), dW_hh, db_hh, dh0 (three each), dW_ih, db_ih (None, layer 2's, layer 3's)"""
    N, T, H = y[0].shape
    out = dict(dgi=[None] * 3, dW_hh=[None] * 3, db_hh=[None] * 3, dh0=[None] * 3, dW_ih=[None] * 3, db_ih=[None] * 3)
    dx = None
    for l in (2, 1, 0):
        d = dy[l] if dx is None else dy[l] + dx
        dgi, out["dW_hh"][l], out["db_hh"][l], out["dh0"][l] = gru_native.gru_sequence_ref_backward(d, y[l], saved[l], w_hh[l], h0[l], dhT[l])
        out["dgi"][l] = dgi
        if l:
            dx = dgi @ w_ih[l]
            out["dW_ih"][l] = dgi.reshape(-1, 3 * H).t() @ y[l - 1].reshape(-1, H)
            out["db_ih"][l] = dgi.sum((0, 1))
    return out


# ---- device tensors ----
_slots, _fit, _dense = gru_native._slots, gru_native._fit, gru_native._dense


def _need_device(t, name):
    import torch
    if not (t.is_cuda and t.dtype == torch.float32):
        raise ValueError(f"librnnoise_amd_gru_stack.so runs float32 tensors on the device: {name} is {t.dtype} on {t.device} "
                         "(gru_stack_ref is the formulas in plain torch)")


def stack_forward(gi0, w_ih, b_ih, w_hh, b_hh, h0=(None, None, None), y=None):
    """The forward call on torch device tensors where they lie: gi0 [N, T, 3H] (any slot strides the header allows); w_ih, b_ih
    (index 0 not looked at), w_hh, b_hh, h0: three each -> [y1, y2, y3] (each [N, T, H]; allocated as the slices 1 .. 3 of one
    [N, T, 4H] buffer unless three are given), saved (3 T N 4H floats).  T + 2 launches, asynchronous on torch's current stream."""
    import torch
    H = w_hh[0].shape[1]
    if gi0.dim() != 3 or gi0.shape[2] != 3 * H:
        raise ValueError("gi0 (rows, steps, 3H), w_hh (3H, H), b_hh (3H,)")
    _need_device(gi0, "gi0")
    N, T = gi0.shape[0], gi0.shape[1]
    n_saved, _ = workspace(N, T, H)
    gi0 = _fit(gi0)
    w_hh = [_dense(w, (3 * H, H), "w_hh") for w in w_hh]
    b_hh = [_dense(b, (3 * H,), "b_hh") for b in b_hh]
    w_ih = [None] + [_dense(w, (3 * H, H), "w_ih") for w in w_ih[1:]]
    b_ih = [None] + [_dense(b, (3 * H,), "b_ih") for b in b_ih[1:]]
    h0 = [_dense(h, (N, H), "h0") for h in h0]
    dev = gi0.device
    if y is None:
        cat = torch.empty((N, T, 4 * H), dtype=torch.float32, device=dev)
        y = [cat[:, :, (l + 1) * H:(l + 2) * H] for l in range(LAYERS)]
    saved = torch.empty((max(n_saved, 4),), dtype=torch.float32, device=dev)
    if T:
        ptr = lambda ts: [0 if t is None else t.data_ptr() for t in ts]
        call = make_stack(_slots(gi0, 3 * H, "gi0"), ptr(w_ih), ptr(b_ih), ptr(w_hh), ptr(b_hh), [_slots(t, H, "y") for t in y], N, T, H, ptr(h0))
        with torch.cuda.device(dev):
            forward_device(call, saved.data_ptr(), dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
    return list(y), saved


def stack_backward(dy, y, saved, w_ih, w_hh, h0=(None, None, None), dhT=(None, None, None), dgi0=None):
    """The backward call likewise: dy, y: three [N, T, H] each, saved as stack_forward left it -> dgi (three: [N, T, 3H], allocated
    contiguous unless dgi0 is given, and [T, N, 3H] for layers 2 and 3), dgh (three [T, N, 3H]), dh0 (three [N, H]).  T + 2 launches."""
    import torch
    N, T, H = y[0].shape
    dev = y[0].device
    for t in dy:
        _need_device(t, "dy")
    dy = [_fit(t) for t in dy]
    w_hh = [_dense(w, (3 * H, H), "w_hh") for w in w_hh]
    w_ih = [None] + [_dense(w, (3 * H, H), "w_ih") for w in w_ih[1:]]
    h0, dhT = [_dense(h, (N, H), "h0") for h in h0], [_dense(h, (N, H), "dhT") for h in dhT]
    _, n_scratch = workspace(N, T, H)
    if dgi0 is None:
        dgi0 = torch.empty((N, T, 3 * H), dtype=torch.float32, device=dev)
    dense = lambda: torch.empty((T, N, 3 * H), dtype=torch.float32, device=dev)
    dgi, dgh = [dgi0, dense(), dense()], [dense(), dense(), dense()]
    if T == 0:
        return dgi, dgh, [h.clone() if h is not None else torch.zeros((N, H), dtype=torch.float32, device=dev) for h in dhT]
    dh0 = [torch.empty((N, H), dtype=torch.float32, device=dev) for _ in range(LAYERS)]
    scratch = torch.empty((n_scratch,), dtype=torch.float32, device=dev)
    ptr = lambda ts: [0 if t is None else t.data_ptr() for t in ts]
    call = make_grad([_slots(t, H, "dy") for t in dy], [_slots(t, H, "y") for t in y], ptr(w_ih), ptr(w_hh), _slots(dgi0, 3 * H, "dgi0"),
                     ptr(dgi), ptr(dgh), ptr(dh0), N, T, H, ptr(h0), ptr(dhT))
    with torch.cuda.device(dev):
        backward_device(call, saved.data_ptr(), scratch.data_ptr(), dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
    return dgi, dgh, dh0


def input_weight_grads(dgi, x, per_step: bool = True, block: int = 256):
    """dW_ih = sum_t dgi[t]^T x[t] and db_ih = sum dgi of a layer that projects its own input, in torch: dgi [T, N, 3H] as the
    backward call leaves it, x [N, T, H] the output of the layer below.  per_step: the form of gru_native.weight_grads -- one float32
    product per step, the steps' products added in float64 and rounded once; otherwise one float32 product over all T N terms
    (DESIGN.md 4.34 has both measured)."""
    import torch
    T, H = dgi.shape[0], x.shape[2]
    if not per_step:
        return dgi.reshape(-1, 3 * H).t() @ x.transpose(0, 1).reshape(-1, H), dgi.sum((0, 1))
    dW = torch.zeros((3 * H, H), dtype=torch.float64, device=dgi.device)
    xt = x.transpose(0, 1)  # [T, N, H] as a view
    for lo in range(0, T, block):
        hi = min(T, lo + block)
        dW += torch.bmm(dgi[lo:hi].transpose(1, 2), xt[lo:hi]).sum(0, dtype=torch.float64)
    return dW.to(dgi.dtype), dgi.sum((0, 1))


def _function():
    import torch

    class GruStack(torch.autograd.Function):
        """y1, y2, y3 = GruStack.apply(gi0, w_ih2, b_ih2, w_ih3, b_ih3, w_hh1, w_hh2, w_hh3, b_hh1, b_hh2, b_hh3, h01, h02, h03): the
        three chained GRU layers on librnnoise_amd_gru_stack.so.  gi0 [N, T, 3H] is layer 1's input projection, the h0 [N, H] or None,
        the y [N, T, H] (slices of one [N, T, 4H] buffer whose first H floats a caller may fill); y[:, -1] is a layer's final state.
        The forward makes T + 2 launches and keeps saved; the backward makes T + 2 launches, then every weight gradient in torch.
        Float32 device tensors only: ValueError on anything else."""

        @staticmethod
        def forward(ctx, gi0, w_ih2, b_ih2, w_ih3, b_ih3, w_hh1, w_hh2, w_hh3, b_hh1, b_hh2, b_hh3, h01=None, h02=None, h03=None):
            d = lambda t: None if t is None else t.detach()
            w_ih, b_ih = [None, d(w_ih2), d(w_ih3)], [None, d(b_ih2), d(b_ih3)]
            ys, saved = stack_forward(gi0.detach(), w_ih, b_ih, [d(w_hh1), d(w_hh2), d(w_hh3)], [d(b_hh1), d(b_hh2), d(b_hh3)],
                                      [d(h01), d(h02), d(h03)])
            ctx.save_for_backward(saved, w_ih2, w_ih3, w_hh1, w_hh2, w_hh3, h01, h02, h03, *ys)
            return tuple(ys)

        @staticmethod
        def backward(ctx, dy1, dy2, dy3):
            saved, w_ih2, w_ih3, w_hh1, w_hh2, w_hh3, h01, h02, h03, y1, y2, y3 = ctx.saved_tensors
            ys, h0 = [y1, y2, y3], [h01, h02, h03]
            dgi, dgh, dh0 = stack_backward([dy1, dy2, dy3], ys, saved, [None, w_ih2.detach(), w_ih3.detach()],
                                           [w_hh1.detach(), w_hh2.detach(), w_hh3.detach()], h0)
            need = ctx.needs_input_grad
            dW_ih, db_ih = [None] * 3, [None] * 3
            for l in (1, 2):
                if need[2 * l - 1] or need[2 * l]:
                    dW_ih[l], db_ih[l] = input_weight_grads(dgi[l], ys[l - 1])
            dW_hh, db_hh = [None] * 3, [None] * 3
            for l in range(LAYERS):
                if need[5 + l] or need[8 + l]:
                    dW_hh[l], db_hh[l] = gru_native.weight_grads(dgh[l], ys[l], h0[l])
            dh = [dh0[l] if h0[l] is not None and need[11 + l] else None for l in range(LAYERS)]
            return (dgi[0], dW_ih[1], db_ih[1], dW_ih[2], db_ih[2], *dW_hh, *db_hh, *dh)

    return GruStack


_GruStack = None


def __getattr__(name):  # GruStack is made on first use: importing this module does not import torch
    global _GruStack
    if name == "GruStack":
        if _GruStack is None:
            _GruStack = _function()
        return _GruStack
    raise AttributeError(name)
