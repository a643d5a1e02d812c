"""The float network in this project's own words: a torch module whose parameter names are the reference trainer's
(conv1, conv2, gru1 .. gru3, dense_out, vad_dense), so that load_state_dict takes a checkpoint of torch/rnnoise/train_rnnoise.py as it
is.  Two valid convolutions of three taps, tanh each; three GRUs in a chain; both outputs a sigmoid of one linear layer over the
concatenation [conv2 | gru1 | gru2 | gru3].

  forward_sequence(features [N, T, 65]) -> gains [N, T - 4, 32], vad [N, T - 4, 1]
      the trainer's view of a sequence: output k has seen features k .. k + 4; zero GRU states, or given ones
  forward(features [N, T, 65]) -> gains [N, T, 32], vad [N, T, 1]
      the streaming view, aligned as the C runtime is: the module keeps the last four feature frames and the three GRU states from
      call to call, frame k + 4 after a reset is output k of forward_sequence on the frames since that reset, and a stream cut into
      calls of any lengths gives what one call gives.  The first four frames after a reset have no output in the trainer's view: the
      GRUs do not run on them, and their gains and vad are zeros -- what the blob's network leaves on a silent frame.  reset() starts a
      new sequence.  This is the stateful net of RNNoiseOp.denoise_with(net, pcm) and of cli denoise --checkpoint.

The module itself only runs forward; rnnoise_amd.train.fit trains it -- forward_sequence with carried states, torch's autograd through
these layers, the loss and its gradient from librnnoise_amd_train.so.  With gru_impl = "native" the three GRUs'
recurrences, forward and backward, run on librnnoise_amd_gru.so instead of torch's nn.GRU; with "stack" the three
layers run on librnnoise_amd_gru_stack.so as one diagonal launch a step; "torch" is the default."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

FEATURES, BANDS, LOOKAHEAD = 65, 32, 4


GRU_IMPLS = ("torch", "native", "stack")


class FloatNet(nn.Module):
    def __init__(self, cond_size: int = 128, gru_size: int = 384, gru_impl: str = "torch"):
        """gru_impl: what runs the three GRUs -- "torch": nn.GRU as it is; "native": the recurrence on librnnoise_amd_gru.so
        (rnnoise_amd.gru_native.GruSequence) with the nn.GRU modules' own parameters, float32 on the device only;
        "stack": the three layers on librnnoise_amd_gru_stack.so, one diagonal launch a step (rnnoise_amd.gru_stack.GruStack; DESIGN.md
        4.34), likewise.
        An attribute, not a parameter: it may be set afterwards, and checkpoints do not carry it."""
        super().__init__()
        if gru_impl not in GRU_IMPLS:
            raise ValueError(f"gru_impl: one of {GRU_IMPLS}, not {gru_impl!r}")
        self.cond_size, self.gru_size, self.gru_impl = cond_size, gru_size, gru_impl
        self.conv1 = nn.Conv1d(FEATURES, cond_size, kernel_size=3)
        self.conv2 = nn.Conv1d(cond_size, gru_size, kernel_size=3)
        self.gru1 = nn.GRU(gru_size, gru_size, batch_first=True)
        self.gru2 = nn.GRU(gru_size, gru_size, batch_first=True)
        self.gru3 = nn.GRU(gru_size, gru_size, batch_first=True)
        self.dense_out = nn.Linear(4 * gru_size, BANDS)
        self.vad_dense = nn.Linear(4 * gru_size, 1)
        self.reset()

    # ---- the layers ----
    def _front(self, features):
        """[N, T, 65] -> [N, T - 4, gru_size]: the two convolutions over time"""
        x = features.transpose(1, 2)
        x = torch.tanh(self.conv2(torch.tanh(self.conv1(x))))
        return x.transpose(1, 2)

    def _back(self, c, states):
        """conv2's frames [N, K, gru_size] and three states [1, N, gru_size] -> gains, vad, the states after frame K - 1"""
        if self.gru_impl == "torch":
            g1, s1 = self.gru1(c, states[0])
            g2, s2 = self.gru2(g1, states[1])
            g3, s3 = self.gru3(g2, states[2])
        elif self.gru_impl == "native":
            g1, s1 = self._native_gru(self.gru1, c, states[0])
            g2, s2 = self._native_gru(self.gru2, g1, states[1])
            g3, s3 = self._native_gru(self.gru3, g2, states[2])
        elif self.gru_impl == "stack":
            (g1, g2, g3), (s1, s2, s3) = self._stack_grus(c, states)
        else:
            raise ValueError(f"gru_impl: one of {GRU_IMPLS}, not {self.gru_impl!r}")
        cat = torch.cat([c, g1, g2, g3], dim=-1)
        return torch.sigmoid(self.dense_out(cat)), torch.sigmoid(self.vad_dense(cat)), [s1, s2, s3]

    def _native_gru(self, gru, x, state):
        """one nn.GRU's layer on the native recurrence: x [N, K, in], state [1, N, H] -> output [N, K, H], state after [1, N, H].
        The input projection is torch's, one product over all steps; there is no fallback: what the library does not take raises."""
        from . import gru_native
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError(f'gru_impl "native" runs float32 tensors on the device, not {x.dtype} on {x.device}: use gru_impl "torch"')
        if self.gru_size % gru_native.TILE or not gru_native.MIN_HIDDEN <= self.gru_size <= gru_native.MAX_HIDDEN:
            raise ValueError('gru_impl "native": ' + gru_native.refusal(x.shape[0], x.shape[1], self.gru_size))
        gi = F.linear(x, gru.weight_ih_l0, gru.bias_ih_l0)
        y = gru_native.GruSequence.apply(gi, gru.weight_hh_l0, gru.bias_hh_l0, state[0])
        return y, y[:, -1].unsqueeze(0).contiguous()

    def _stack_grus(self, x, states):
        """the three nn.GRU layers on the stack library: x [N, K, in], three states [1, N, H] -> three outputs [N, K, H], three states
        after [1, N, H].  Layer 1's input projection is torch's, one product over all steps; there is no fallback."""
        from . import gru_stack
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError(f'gru_impl "stack" runs float32 tensors on the device, not {x.dtype} on {x.device}: use gru_impl "torch"')
        if self.gru_size % gru_stack.TILE or not gru_stack.MIN_HIDDEN <= self.gru_size <= gru_stack.MAX_HIDDEN:
            raise ValueError('gru_impl "stack": ' + gru_stack.refusal(x.shape[0], x.shape[1], self.gru_size))
        g = (self.gru1, self.gru2, self.gru3)
        gi0 = F.linear(x, g[0].weight_ih_l0, g[0].bias_ih_l0)
        ys = gru_stack.GruStack.apply(gi0, g[1].weight_ih_l0, g[1].bias_ih_l0, g[2].weight_ih_l0, g[2].bias_ih_l0,
                                      *[m.weight_hh_l0 for m in g], *[m.bias_hh_l0 for m in g], *[s[0] for s in states])
        return ys, [y[:, -1].unsqueeze(0).contiguous() for y in ys]

    def _zero_states(self, n, like):
        return [torch.zeros((1, n, self.gru_size), device=like.device, dtype=like.dtype) for _ in range(3)]

    # ---- the trainer's view ----
    def forward_sequence(self, features, states=None, return_states: bool = False):
        assert features.dim() == 3 and features.shape[2] == FEATURES and features.shape[1] > LOOKAHEAD, tuple(features.shape)
        c = self._front(features)
        gains, vad, states = self._back(c, self._zero_states(features.shape[0], c) if states is None else states)
        return (gains, vad, states) if return_states else (gains, vad)

    # ---- the streaming view ----
    def reset(self):
        """a new sequence for every stream: no history, zero states; the next call sets the number of streams"""
        self._hist, self._states, self._seen = None, None, 0

    def forward(self, features):
        assert features.dim() == 3 and features.shape[2] == FEATURES, tuple(features.shape)
        n, t = features.shape[0], features.shape[1]
        if self._hist is None or self._hist.shape[0] != n or self._hist.device != features.device or self._hist.dtype != features.dtype:
            self.reset()
            self._hist = torch.zeros((n, LOOKAHEAD, FEATURES), device=features.device, dtype=features.dtype)
            self._states = self._zero_states(n, features)
        gains = torch.zeros((n, t, BANDS), device=features.device, dtype=features.dtype)
        vad = torch.zeros((n, t, 1), device=features.device, dtype=features.dtype)
        if t == 0:
            return gains, vad
        x = torch.cat([self._hist, features], dim=1)
        skip = max(0, min(t, LOOKAHEAD - self._seen))  # frames of this call that still lack their four predecessors
        if skip < t:
            g, v, self._states = self._back(self._front(x[:, skip:]), self._states)
            gains[:, skip:], vad[:, skip:] = g, v
        self._hist = x[:, -LOOKAHEAD:].detach().clone()
        self._states = [s.detach() for s in self._states]
        self._seen += t
        return gains, vad


def load_checkpoint(path: str, device=None) -> FloatNet:
    """a FloatNet in eval mode holding the weights of a trainer checkpoint (rnnoise_amd.export.load_state_dict_file: a .pth with
    'state_dict', or a bare state dict); the dimensions are read off the tensors"""
    from .export import load_state_dict_file
    try:
        sd = load_state_dict_file(path)
    except ValueError:  # (dimensions the blob does not hold: the float network runs them all the same)
        sd = torch.load(path, map_location="cpu")["state_dict"]
    net = FloatNet(cond_size=sd["conv1.weight"].shape[0], gru_size=sd["conv2.weight"].shape[0])
    net.load_state_dict(sd)
    net.eval()
    return net.to(device) if device is not None else net
