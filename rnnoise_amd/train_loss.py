"""ctypes binding of librnnoise_amd_train.so (include/rnnoise_amd_train.h): the reference trainer's loss with its gradient, on the
device, in double -- the terms and the order of additions of rnnoise_batch_score_records, so that the loss a training step reports,
the loss `eval-records` prints and the loss of the exported blob come from the same doubles.

  loss_device(...)    raw device pointers, asynchronous on a stream: two launches
  loss_and_grad(...)  torch device tensors through their own strides -> sums, grad_gains, grad_vad
  TrainerLoss         a torch.autograd.Function: (loss, gain_loss, vad_loss) forward, the stored gradients scaled in backward

The library is a separate one: nothing here goes through rnnoise_amd.capi's prototype table, and the product libraries do not know it.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _sidelib, capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librnnoise_amd_train.so")

RECORD = 98       # RNNOISE_AMD_TRAIN_RECORD
BANDS = 32        # RNNOISE_AMD_TRAIN_BANDS
SUMS = 4          # RNNOISE_AMD_TRAIN_SUMS: gain terms, vad terms, frames scored, 0
FRAME_BLOCK = 16  # RNNOISE_AMD_TRAIN_FRAME_BLOCK: steps of a workgroup of rn_train_loss_kernel
KERNELS = ("rn_train_loss_kernel", "rn_train_loss_sums_kernel")


class Call(C.Structure):
    """RNNoiseTrainLoss"""
    _fields_ = [("records", C.c_void_p), ("rec_frame_stride", C.c_long), ("rec_row_stride", C.c_long),
                ("gains", C.c_void_p), ("gain_frame_stride", C.c_long), ("gain_row_stride", C.c_long),
                ("vad", C.c_void_p), ("vad_frame_stride", C.c_long), ("vad_row_stride", C.c_long),
                ("grad_gains", C.c_void_p), ("grad_vad", C.c_void_p),
                ("n_rows", C.c_int), ("t0", C.c_int), ("n_frames", C.c_int), ("first", C.c_int),
                ("gamma", C.c_double), ("w_gain", C.c_double), ("w_vad", C.c_double)]


_int, _vp, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_double)
# symbol -> (restype, argtypes), in the header's order; tests/test_train_loss_cpu.py holds the table against the header
PROTOTYPES = {
    "rnnoise_amd_train_loss_check": (_int, (C.POINTER(Call),)),
    "rnnoise_amd_train_loss_device": (_int, (_int, _vp, _vp, C.POINTER(Call), _vp)),
    "rnnoise_amd_train_loss": (_int, (_int, _dp, _dp, C.POINTER(Call))),
}
EXPORTS = list(PROTOTYPES)

def lib():
    return _sidelib.load(LIB_PATH, PROTOTYPES)


def make_call(records, gains, vad, n_rows, t0, n_frames, first=4, gamma=.25, w_gain=0.0, w_vad=0.0, grad_gains=0, grad_vad=0) -> Call:
    """records, gains, vad: (pointer, frame_stride, row_stride) each, the pointer an int; grad_*: pointers (0: none)"""
    c = Call()
    (c.records, c.rec_frame_stride, c.rec_row_stride) = (int(records[0]) or None, int(records[1]), int(records[2]))
    (c.gains, c.gain_frame_stride, c.gain_row_stride) = (int(gains[0]) or None, int(gains[1]), int(gains[2]))
    (c.vad, c.vad_frame_stride, c.vad_row_stride) = (int(vad[0]) or None, int(vad[1]), int(vad[2]))
    c.grad_gains, c.grad_vad = int(grad_gains) or None, int(grad_vad) or None
    c.n_rows, c.t0, c.n_frames, c.first = int(n_rows), int(t0), int(n_frames), int(first)
    c.gamma, c.w_gain, c.w_vad = float(gamma), float(w_gain), float(w_vad)
    return c


def check(call: Call) -> bool:
    """whether the loss calls accept `call` (rnnoise_amd_train_loss_check; host only, nothing is dereferenced)"""
    return lib().rnnoise_amd_train_loss_check(C.byref(call)) == 0


def loss_device(d_sums: int, d_frame_terms: int, call: Call, device: int = 0, stream: int = 0) -> None:
    """rnnoise_amd_train_loss_device on raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle): ADDS the sums of
    the call's scored steps to d_sums [n_rows][4] float64 through the workspace d_frame_terms [n_rows][n_frames][2] float64, and
    writes the gradients where the call names them.  ValueError where the library refuses the arguments."""
    if lib().rnnoise_amd_train_loss_device(int(device), d_sums or None, d_frame_terms or None, C.byref(call), stream or None):
        raise ValueError("rnnoise_amd_train_loss_device refused the call (include/rnnoise_amd_train.h: a null buffer, overlapping "
                         "slots, one gradient without the other, gamma, weights or counts out of range) or could not launch")


def _strides(t, width, name):
    """(pointer, frame_stride, row_stride) of a (rows, steps, width) float32 device tensor whose last dimension is contiguous"""
    import torch
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] >= width and (t.stride(2) == 1 or t.shape[2] == 1)):
        raise ValueError(f"{name}: a (rows, steps, >= {width}) float32 device tensor with contiguous last dimension")
    return t.data_ptr(), t.stride(1), t.stride(0)


def loss_and_grad(records, gains, vad, t0: int = 4, first: int = 4, gamma: float = .25, w_gain=None, w_vad=None, sums=None,
                  want_grad: bool = True):
    """The trainer's loss of predictions against records, and its gradient, on torch device tensors as they lie (any strides the
    header allows).  records: (rows, T, >= 98) float32 from record 0; gains (rows, n, 32) and vad (rows, n, 1) or (rows, n): the
    predictions of steps t0 .. t0 + n - 1 -- FloatNet.forward_sequence's outputs with t0 = 4.  w_gain, w_vad: the weights of the two
    sums in the loss the gradient is of; None: the trainer's means 1 / (32 F) and .001 / F, F the scored steps of all rows (known on
    the host: rows * the call's scored steps).  sums: (rows, 4) float64 device tensor ADDED to (None: zeros).
    -> sums, grad_gains, grad_vad (shaped as gains and vad; None, None without want_grad).  Asynchronous on torch's current stream."""
    import torch
    if vad.dim() == 2:
        vad = vad.unsqueeze(-1)
    R, n = gains.shape[0], gains.shape[1]
    rec, g, v = _strides(records, RECORD, "records"), _strides(gains, BANDS, "gains"), _strides(vad, 1, "vad")
    if gains.shape[2] != BANDS or vad.shape != (R, n, 1) or records.shape[0] != R or records.shape[1] < t0 + n - 1:
        raise ValueError("gains (rows, n, 32), vad (rows, n, 1), records (rows, >= t0 + n - 1, 98)")
    dev = gains.device
    F = R * max(0, t0 + n - max(t0, first, 1))
    if w_gain is None:
        w_gain = 1.0 / (BANDS * F) if F else 0.0
    if w_vad is None:
        w_vad = .001 / F if F else 0.0
    if sums is None:
        sums = torch.zeros((R, SUMS), dtype=torch.float64, device=dev)
    if not (sums.is_cuda and sums.dtype == torch.float64 and sums.shape == (R, SUMS) and sums.is_contiguous()):
        raise ValueError("sums: a contiguous (rows, 4) float64 device tensor")
    terms = torch.empty((R, max(n, 1), 2), dtype=torch.float64, device=dev)
    gg = gv = None
    if want_grad:  # laid out as the predictions: the same strides
        gg, gv = torch.empty_strided(gains.shape, gains.stride(), dtype=torch.float32, device=dev), \
            torch.empty_strided(vad.shape, vad.stride(), dtype=torch.float32, device=dev)
    call = make_call(rec, g, v, R, t0, n, first, gamma, w_gain, w_vad, gg.data_ptr() if want_grad else 0, gv.data_ptr() if want_grad else 0)
    with torch.cuda.device(dev):
        loss_device(sums.data_ptr(), terms.data_ptr(), call, dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
    return sums, gg, gv


def means(sums):
    """(loss, gain_loss, vad_loss) from sums (rows, 4) as evaluate's means take them: the sums over rows in float64, gain_loss =
    sum of gain terms / (32 frames), vad_loss = sum of vad terms / frames, loss = gain_loss + .001 vad_loss.  sums: a host array"""
    losses = capi.eval_losses(sums)
    return losses["loss"], losses["gain_loss"], losses["vad_loss"]


def _function():
    import torch

    class TrainerLoss(torch.autograd.Function):
        """loss, gain_loss, vad_loss = TrainerLoss.apply(gains, vad, records, t0, first, gamma): the trainer's three means of
        predictions (rows, n, 32) / (rows, n, 1) against records (rows, T, 98), as float64 scalar device tensors computed from the
        library's doubles exactly as evaluate's means are.  The forward makes the two launches with the gradient of `loss`; the
        backward scales the stored gradients by the incoming gradient of `loss` (gain_loss and vad_loss are for reporting: no
        gradient flows through them)."""

        @staticmethod
        def forward(ctx, gains, vad, records, t0=4, first=4, gamma=.25):
            sums, gg, gv = loss_and_grad(records, gains.detach(), vad.detach(), t0, first, gamma)
            ctx.save_for_backward(gg, gv)
            ctx.vad_shape = vad.shape
            ctx.sums = sums
            # the means are taken on the host by the code evaluate's means go through (capi.eval_losses): the same additions in the
            # same order; this waits for the two launches, as the trainer's own .item() calls do
            loss, gain_loss, vad_loss = (torch.tensor(x, dtype=torch.float64, device=gains.device) for x in means(sums.cpu().numpy()))
            ctx.mark_non_differentiable(gain_loss, vad_loss)
            return loss, gain_loss, vad_loss

        @staticmethod
        def backward(ctx, g_loss, _g_gain, _g_vad):
            gg, gv = ctx.saved_tensors
            s = g_loss.to(torch.float32)
            return gg * s, (gv * s).reshape(ctx.vad_shape), None, None, None, None

    return TrainerLoss


_TrainerLoss = None


def __getattr__(name):  # TrainerLoss is made on first use: importing this module does not import torch
    global _TrainerLoss
    if name == "TrainerLoss":
        if _TrainerLoss is None:
            _TrainerLoss = _function()
        return _TrainerLoss
    raise AttributeError(name)
