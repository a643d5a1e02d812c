"""librnnoise_amd_gru_stack.so on the device (include/rnnoise_amd_gru_stack.h, rnnoise_amd/gru_stack.py): the two diagonal kernels
against the header's formulas in float64 and beside three chained nn.GRU in float32; determinism, cuts, guard words, a poisoned row;
and the switch value "stack" in FloatNet, fit and the command line.

THE BOUND (tests/test_gru_native_gpu.py's).  X64 is gru_stack.gru_stack_ref (and its backward) in float64 on the CPU.  For every
output X -- y1 .. y3, dgi0, dh0 x 3, dW_hh and db_hh x 3, dW_ih and db_ih of layers 2 and 3 -- with e_stack = max |X - X64| and
e_torch = max |X of three chained nn.GRU in float32 on the device - X64|:

    e_stack <= 4 max(e_torch, 2^-23 max |X64|)

nn.GRU does not show dgi, so torch's first layer here has the identity as W_ih and no b_ih over inputs of 3H floats: then its gi is
its input and its input gradient is dgi0, both exactly.  The largest ratio e_stack / max(e_torch, floor) per output is printed;
DESIGN.md 4.34 records the measured ones."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_loss_ref as R
from conftest import assert_bits_equal
from gru_cases import DEV, FILL, filled, lay, net_outputs, ratios, slot_mask, u32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L3 = range(3)
OUTPUTS = tuple(f"{k}{l}" for k in ("y", "dh0_", "dW_hh", "db_hh") for l in L3) + ("dgi0", "dW_ih1", "dW_ih2", "db_ih1", "db_ih2")


def problem(N, T, H, with_states, seed=0):
    """float32 inputs on the CPU: gi0, per layer w_ih, b_ih (None for layer 0), w_hh, b_hh, h0, dhT (None without states), dy"""
    gen = torch.Generator().manual_seed(seed * 1000003 + N * 10007 + T * 101 + H)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    sc = 1.0 / np.sqrt(H)
    return dict(gi0=rnd(N, T, 3 * H), w_ih=[None, rnd(3 * H, H) * sc, rnd(3 * H, H) * sc], b_ih=[None, rnd(3 * H) * .3, rnd(3 * H) * .3],
                w_hh=[rnd(3 * H, H) * sc for _ in L3], b_hh=[rnd(3 * H) * .3 for _ in L3],
                h0=[rnd(N, H).tanh() if with_states else None for _ in L3], dhT=[rnd(N, H) if with_states else None for _ in L3],
                dy=[rnd(N, T, H) for _ in L3])


def convert(p, fn):
    return {k: (fn(v) if torch.is_tensor(v) else [None if t is None else fn(t) for t in v]) for k, v in p.items()}


def named(ys, out, dh0=True):
    d = {f"y{l}": ys[l] for l in L3}
    d["dgi0"] = out["dgi"][0]
    for l in L3:
        d[f"dh0_{l}"] = out["dh0"][l] if dh0 else None
        d[f"dW_hh{l}"], d[f"db_hh{l}"] = out["dW_hh"][l], out["db_hh"][l]
    for l in (1, 2):
        d[f"dW_ih{l}"], d[f"db_ih{l}"] = out["dW_ih"][l], out["db_ih"][l]
    return d


def reference64(p):
    from rnnoise_amd import gru_stack as S
    d = convert(p, lambda t: t.double())
    ys, saved = S.gru_stack_ref(d["gi0"], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], d["h0"], return_saved=True)
    return named(ys, S.gru_stack_ref_backward(d["dy"], ys, saved, d["w_ih"], d["w_hh"], d["h0"], d["dhT"]))


def torch_grus32(p):
    """three chained nn.GRU in float32 on the device, the first with W_ih = I, b_ih = 0 over 3H inputs: gi0 in, dgi0 out"""
    N, T, H = p["dy"][0].shape
    grus = [torch.nn.GRU(3 * H if l == 0 else H, H, batch_first=True).to(DEV) for l in L3]
    with torch.no_grad():
        grus[0].weight_ih_l0.copy_(torch.eye(3 * H))
        grus[0].bias_ih_l0.zero_()
        for l in L3:
            grus[l].weight_hh_l0.copy_(p["w_hh"][l])
            grus[l].bias_hh_l0.copy_(p["b_hh"][l])
            if l:
                grus[l].weight_ih_l0.copy_(p["w_ih"][l])
                grus[l].bias_ih_l0.copy_(p["b_ih"][l])
    x = p["gi0"].to(DEV).requires_grad_(True)
    h0 = [None if h is None else h.to(DEV).requires_grad_(True) for h in p["h0"]]
    ys, inp, loss = [], x, 0
    for l in L3:
        y, hT = grus[l](inp, None if h0[l] is None else h0[l].unsqueeze(0))
        loss = loss + (y * p["dy"][l].to(DEV)).sum()
        if p["dhT"][l] is not None:
            loss = loss + (hT[0] * p["dhT"][l].to(DEV)).sum()
        ys.append(y)
        inp = y
    loss.backward()
    out = dict(dgi=[x.grad, None, None], dh0=[None if h is None else h.grad for h in h0], dW_hh=[g.weight_hh_l0.grad for g in grus],
               db_hh=[g.bias_hh_l0.grad for g in grus], dW_ih=[None] + [g.weight_ih_l0.grad for g in grus[1:]],
               db_ih=[None] + [g.bias_ih_l0.grad for g in grus[1:]])
    return named([y.detach() for y in ys], out)


def stack32(p, frame_major=False):
    """the two device calls on their own (dhT goes into the backward call as it is), and the wrapper's weight gradients.  Batch-first:
    y1 .. y3 are the slices 1 .. 3 of one [N, T, 4H] buffer and dy1 .. dy3 slices of another; frame-major: three buffers each."""
    from rnnoise_amd import gru_native, gru_stack as S
    N, T, H = p["dy"][0].shape
    d = convert({k: v for k, v in p.items() if k not in ("gi0", "dy")}, lambda t: t.to(DEV))
    gi0 = lay(p["gi0"], frame_major)
    if frame_major:
        dy, y_buf = [lay(t, True) for t in p["dy"]], [lay(torch.zeros(N, T, H), True) for _ in L3]
    else:
        cat = torch.zeros(N, T, 4 * H, device=DEV)
        cat[:, :, H:] = torch.cat(p["dy"], dim=2).to(DEV)
        dy, y_buf = [cat[:, :, (l + 1) * H:(l + 2) * H] for l in L3], None
    dgi0_buf = lay(torch.zeros(N, T, 3 * H), frame_major)
    ys, saved = S.stack_forward(gi0, d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], d["h0"], y=y_buf)
    dgi, dgh, dh0 = S.stack_backward(dy, ys, saved, d["w_ih"], d["w_hh"], d["h0"], d["dhT"], dgi0=dgi0_buf)
    assert dgi[0].data_ptr() == dgi0_buf.data_ptr()  # written where they lie
    if frame_major:
        assert all(ys[l].data_ptr() == y_buf[l].data_ptr() for l in L3)
    else:
        assert ys[1].data_ptr() - ys[0].data_ptr() == 4 * H and ys[0].stride() == (T * 4 * H, 4 * H, 1)
    out = dict(dgi=dgi, dh0=dh0, dW_hh=[None] * 3, db_hh=[None] * 3, dW_ih=[None] * 3, db_ih=[None] * 3)
    for l in L3:
        out["dW_hh"][l], out["db_hh"][l] = gru_native.weight_grads(dgh[l], ys[l], d["h0"][l])
        if l:
            out["dW_ih"][l], out["db_ih"][l] = S.input_weight_grads(dgi[l], ys[l - 1])
    res = named(ys, out)
    res.update(saved=saved, dgh=torch.stack(dgh), dgi_upper=torch.stack(dgi[1:]), dh0=torch.stack(dh0))
    return res


WORST = {}


@pytest.mark.parametrize("N", [1, 16, 17, 67])
@pytest.mark.parametrize("H", [16, 48, 384])
def test_parity_with_float64_beside_torch(H, N):
    """T 1, 2 (fewer steps than layers: fill and drain overlap), 3 (the diagonal's depth), 4 (one steady-state launch), 35 (both
    halves of every ping-pong many times); each with zero states in batch-first buffers and with given h0 and dhT in frame-major ones
    -- and at T 3 the other way round"""
    for T in (1, 2, 3, 4, 35):
        for with_states, frame_major in ((False, False), (True, True)) + (((True, False), (False, True)) if T == 3 else ()):
            p = problem(N, T, H, with_states)
            want = reference64(p)
            got, other = stack32(p, frame_major), torch_grus32(p)
            r = ratios(got, other, want, OUTPUTS)
            assert set(r) == set(OUTPUTS) - (set() if with_states else {"dh0_0", "dh0_1", "dh0_2"})  # (torch shows no dh0 without an h0)
            for k, v in r.items():
                WORST[k] = max(WORST.get(k, 0.0), v)
                assert v <= 4.0, (k, v, H, N, T, with_states, frame_major)
    print(f"H {H} N {N}: largest e_stack / max(e_torch, floor) so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_autograd_function_gives_the_calls_numbers():
    """GruStack.apply under torch's autograd: the bits of the two calls, dhT arriving through y[:, -1]"""
    from rnnoise_amd import gru_stack as S
    N, T, H = 17, 5, 48
    p = problem(N, T, H, True, seed=2)
    leaf = lambda t: t.to(DEV).requires_grad_(True)
    gi0, w_ih, b_ih = leaf(p["gi0"]), [None] + [leaf(t) for t in p["w_ih"][1:]], [None] + [leaf(t) for t in p["b_ih"][1:]]
    w_hh, b_hh, h0 = [leaf(t) for t in p["w_hh"]], [leaf(t) for t in p["b_hh"]], [leaf(t) for t in p["h0"]]
    ys = S.GruStack.apply(gi0, w_ih[1], b_ih[1], w_ih[2], b_ih[2], *w_hh, *b_hh, *h0)
    sum((ys[l] * p["dy"][l].to(DEV)).sum() for l in L3).backward()
    raw = stack32(dict(p, dhT=[None] * 3))
    pairs = [("dgi0", gi0.grad)] + [(f"y{l}", ys[l]) for l in L3] + [(f"dW_hh{l}", w_hh[l].grad) for l in L3] + \
            [(f"db_hh{l}", b_hh[l].grad) for l in L3] + [(f"dh0_{l}", h0[l].grad) for l in L3] + \
            [(f"dW_ih{l}", w_ih[l].grad) for l in (1, 2)] + [(f"db_ih{l}", b_ih[l].grad) for l in (1, 2)]
    assert len(pairs) == len(OUTPUTS)
    for name, a in pairs:
        assert_bits_equal(u32(a), u32(raw[name]), name)
    # without states, without weight gradients, and with only the last layer's output used
    gi2 = leaf(p["gi0"])
    det = lambda ts: [None if t is None else t.detach() for t in ts]
    y2 = S.GruStack.apply(gi2, *[t for l in (1, 2) for t in (det(w_ih)[l], det(b_ih)[l])], *det(w_hh), *det(b_hh), None, None, None)
    (y2[2] * p["dy"][2].to(DEV)).sum().backward()
    q = dict(p, dhT=[None] * 3, h0=[None] * 3, dy=[torch.zeros(N, T, H), torch.zeros(N, T, H), p["dy"][2]])
    raw2 = stack32(q)
    assert_bits_equal(u32(y2[2]), u32(raw2["y2"]), "y3, no states")
    assert_bits_equal(u32(gi2.grad), u32(raw2["dgi0"]), "dgi0, no states")
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(ValueError):  # H 24
        S.GruStack.apply(z(2, 3, 72), z(72, 24), z(72), z(72, 24), z(72), z(72, 24), z(72, 24), z(72, 24), z(72), z(72), z(72), None, None, None)
    with pytest.raises(ValueError):  # float64
        S.GruStack.apply(*[t.double() for t in (z(2, 3, 48), z(48, 16), z(48), z(48, 16), z(48), z(48, 16), z(48, 16), z(48, 16), z(48), z(48), z(48))],
                         None, None, None)


def test_two_runs_are_bit_identical():
    p = problem(67, 35, 384, True, seed=3)
    a, b = stack32(p), stack32(p)
    for k in OUTPUTS + ("saved", "dgh", "dgi_upper"):
        assert_bits_equal(u32(a[k]), u32(b[k]), k)


@pytest.mark.parametrize("cuts", [((0, 16), (16, 17), (17, 35)), ((0, 2), (2, 3), (3, 35))])
def test_cuts_give_the_bits_of_one_call(cuts):
    """T = 35 as 16 + 1 + 18 and as 2 + 1 + 32 (calls shorter than the diagonal): forward with the states carried, backward in reverse
    with dh0 carried into dhT"""
    from rnnoise_amd import gru_stack as S
    N, T, H = 17, 35, 48
    p = problem(N, T, H, True, seed=4)
    whole = stack32(p)
    d = convert(p, lambda t: t.to(DEV))
    y = [torch.zeros(N, T, H, device=DEV) for _ in L3]
    state, saved = d["h0"], []
    for lo, hi in cuts:
        _, s = S.stack_forward(d["gi0"][:, lo:hi], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], state, y=[t[:, lo:hi] for t in y])
        saved.append(s)
        state = [t[:, hi - 1] for t in y]
    for l in L3:
        assert_bits_equal(u32(y[l]), u32(whole[f"y{l}"]), f"y{l} of the cuts")
    dgi0, dgh, upper, dh = torch.zeros(N, T, 3 * H, device=DEV), [None] * 3, [None] * 3, d["dhT"]
    for k in (2, 1, 0):
        lo, hi = cuts[k]
        first = d["h0"] if lo == 0 else [t[:, lo - 1] for t in y]
        dgi, g, dh = S.stack_backward([t[:, lo:hi] for t in d["dy"]], [t[:, lo:hi] for t in y], saved[k], d["w_ih"], d["w_hh"], first, dh,
                                      dgi0=dgi0[:, lo:hi])
        dgh[k], upper[k] = torch.stack(g), torch.stack(dgi[1:])
    assert_bits_equal(u32(dgi0), u32(whole["dgi0"]), "dgi0 of the cuts")
    assert_bits_equal(u32(torch.cat(dgh, dim=1)), u32(whole["dgh"]), "dgh of the cuts")
    assert_bits_equal(u32(torch.cat(upper, dim=1)), u32(whole["dgi_upper"]), "dgi of layers 2, 3 of the cuts")
    assert_bits_equal(u32(torch.stack(dh)), u32(whole["dh0"]), "dh0 of the cuts")
    # an empty cut: nothing launched, the states and the gradients pass through
    y0, _ = S.stack_forward(d["gi0"][:, :0], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], state)
    assert [tuple(t.shape) for t in y0] == [(N, 0, H)] * 3
    _, _, dh_same = S.stack_backward([t[:, :0] for t in d["dy"]], [t[:, :0] for t in y], torch.zeros(4, device=DEV), d["w_ih"], d["w_hh"],
                                     [None] * 3, dh)
    assert all(torch.equal(a, b) for a, b in zip(dh_same, dh))


@pytest.mark.parametrize("H", [16, 48, 384])
def test_one_cell_in_both_libraries(H):
    """Both libraries compile one cell (rnnoise_amd/csrc/gru_cell.h), so where the stack does what the single layer does the bits are
    the same: layer 1 forward is a layer that is given its gi, and layer 3 backward is a layer nobody adds a dx to (that it leaves one
    for the layer below changes none of its own sums).  h0 and dhT given; N 17: a ragged row tile; T 3: the first length with a full
    diagonal; H 16 and 48 have the remainder loop only, H 384 the blocks of 6, 3 and 2 chunks."""
    from rnnoise_amd import gru_native as G, gru_stack as S
    N, T = 17, 3
    p = problem(N, T, H, True, seed=5)
    d = convert(p, lambda t: t.to(DEV))
    ys, saved = S.stack_forward(d["gi0"], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], d["h0"])
    dgi, dgh, dh0 = S.stack_backward(d["dy"], ys, saved, d["w_ih"], d["w_hh"], d["h0"], d["dhT"])
    layer = saved.view(-1)[:3 * T * N * 4 * H].view(3, T * N * 4 * H)
    y1, saved1 = G.sequence_forward(d["gi0"], d["w_hh"][0], d["b_hh"][0], d["h0"][0])
    assert_bits_equal(u32(ys[0]), u32(y1), "y of layer 1")
    assert_bits_equal(u32(layer[0]), u32(saved1.view(-1)[:T * N * 4 * H]), "saved of layer 1")
    dgi3, dgh3, dh03 = G.sequence_backward(d["dy"][2], ys[2], layer[2].contiguous(), d["w_hh"][2], d["h0"][2], d["dhT"][2])
    assert_bits_equal(u32(dgi[2].transpose(0, 1)), u32(dgi3), "dgi of layer 3")
    assert_bits_equal(u32(dgh[2]), u32(dgh3), "dgh of layer 3")
    assert_bits_equal(u32(dh0[2]), u32(dh03), "dh0 of layer 3")


@pytest.mark.parametrize("N,T,H", [(17, 3, 48), (5, 2, 16), (16, 4, 48)])
def test_guard_words_keep_their_fill(N, T, H):
    """padded strides in both orders, with room for the rows N .. 16 ceil(N / 16) - 1 that do not exist, and every dense buffer with
    a tail beyond its documented size: only the slots are written, and the inputs are read only"""
    from rnnoise_amd import gru_stack as S
    p = problem(N, T, H, True, seed=5)
    want = stack32(p)
    n_saved, n_scratch = S.workspace(N, T, H)
    tail, off = 16 * 4 * H * 2, 64
    d = convert({k: v for k, v in p.items() if k not in ("gi0", "dy")}, lambda t: t.to(DEV).contiguous())
    ptr = lambda ts: [0 if t is None else t.data_ptr() for t in ts]
    for order in ("rows in a frame", "frames in a row"):
        if order == "rows in a frame":  # a frame holds 32 row slots: the rows beyond N would land in the gap
            y_rs, gi_rs = H + 4, 3 * H + 8
            y_fs, gi_fs = 32 * y_rs, 32 * gi_rs
        else:
            y_fs, gi_fs = H + 4, 3 * H + 8
            y_rs, gi_rs = (T + 2) * y_fs, (T + 2) * gi_fs
        y_total = off + (T - 1) * y_fs + (N - 1) * y_rs + H + 32 * max(y_rs, y_fs)
        gi_total = off + (T - 1) * gi_fs + (N - 1) * gi_rs + 3 * H + 32 * max(gi_rs, gi_fs)
        view = lambda buf, fs, rs, M: torch.as_strided(buf, (N, T, M), (rs, fs, 1), off)
        gi_buf, dy_buf = filled(gi_total), [filled(y_total) for _ in L3]
        view(gi_buf, gi_fs, gi_rs, 3 * H).copy_(p["gi0"].to(DEV))
        for l in L3:
            view(dy_buf[l], y_fs, y_rs, H).copy_(p["dy"][l].to(DEV))
        y_buf, dgi_buf = [filled(y_total) for _ in L3], filled(gi_total)
        dense = dict(saved=filled(n_saved + tail), scratch=filled(n_scratch + tail))
        for l in L3:
            dense[f"dgh{l}"], dense[f"dh0_{l}"] = filled(T * N * 3 * H + tail), filled(N * H + tail)
            if l:
                dense[f"dgi{l}"] = filled(T * N * 3 * H + tail)
        at = lambda buf, fs, rs: (buf.data_ptr() + 4 * off, fs, rs)
        call = S.make_stack(at(gi_buf, gi_fs, gi_rs), ptr(d["w_ih"]), ptr(d["b_ih"]), ptr(d["w_hh"]), ptr(d["b_hh"]),
                            [at(b, y_fs, y_rs) for b in y_buf], N, T, H, ptr(d["h0"]))
        assert S.check(call)
        stream = torch.cuda.current_stream(DEV).cuda_stream
        S.forward_device(call, dense["saved"].data_ptr(), 0, stream)
        grad = S.make_grad([at(b, y_fs, y_rs) for b in dy_buf], [at(b, y_fs, y_rs) for b in y_buf], ptr(d["w_ih"]), ptr(d["w_hh"]),
                           at(dgi_buf, gi_fs, gi_rs), [0, dense["dgi1"].data_ptr(), dense["dgi2"].data_ptr()],
                           [dense[f"dgh{l}"].data_ptr() for l in L3], [dense[f"dh0_{l}"].data_ptr() for l in L3], N, T, H, ptr(d["h0"]), ptr(d["dhT"]))
        assert S.check(grad)
        S.backward_device(grad, dense["saved"].data_ptr(), dense["scratch"].data_ptr(), 0, stream)
        torch.cuda.synchronize()
        strided = [(f"y{l}", y_buf[l], y_fs, y_rs, H) for l in L3] + [("dgi0", dgi_buf, gi_fs, gi_rs, 3 * H)]
        for name, buf, fs, rs, M in strided:
            words, mask = u32(buf), slot_mask(buf.numel(), off, fs, rs, T, N, M)
            assert np.all(words[~mask] == FILL), (name, order, int((words[~mask] != FILL).sum()))
            assert_bits_equal(u32(view(buf, fs, rs, M)), u32(want[name]), f"{name}, {order}")
        expected = dict(saved=want["saved"][:n_saved])
        for l in L3:
            expected[f"dgh{l}"], expected[f"dh0_{l}"] = want["dgh"][l], want["dh0"][l]
            if l:
                expected[f"dgi{l}"] = want["dgi_upper"][l - 1]
        for name, buf in dense.items():
            size = n_scratch if name == "scratch" else expected[name].numel()
            words = u32(buf)
            assert np.all(words[size:] == FILL), (name, order)
            if name != "scratch":
                assert_bits_equal(words[:size], u32(expected[name]).reshape(-1), f"{name}, {order}")
        # the scratch: three dh pairs, then two dx pairs, N H floats a half.  A layer hands dh on T - 1 times, alternating; layers 2 and
        # 3 leave a dx at every step
        used = (u32(dense["scratch"])[:n_scratch] != FILL).reshape(10, N * H)
        for pair in range(3):
            assert used[2 * pair:2 * pair + 2].all(axis=1).sum() == min(T - 1, 2), (order, pair)
        for pair in (3, 4):
            assert used[2 * pair:2 * pair + 2].all(axis=1).sum() == min(T, 2), (order, pair)
        assert np.all(used.all(axis=1) | ~used.any(axis=1))
        # the inputs are read only
        assert np.all(u32(gi_buf)[~slot_mask(gi_buf.numel(), off, gi_fs, gi_rs, T, N, 3 * H)] == FILL)
        assert_bits_equal(u32(view(gi_buf, gi_fs, gi_rs, 3 * H)), u32(p["gi0"]), "gi0")
        for l in L3:
            assert np.all(u32(dy_buf[l])[~slot_mask(y_total, off, y_fs, y_rs, T, N, H)] == FILL)
            assert_bits_equal(u32(view(dy_buf[l], y_fs, y_rs, H)), u32(p["dy"][l]), f"dy{l}")
        for k in ("w_ih", "b_ih", "w_hh", "b_hh", "h0", "dhT"):
            for l in L3:
                if d[k][l] is not None:
                    assert_bits_equal(u32(d[k][l]), u32(p[k][l]), f"{k}{l}")


@pytest.mark.parametrize("N,row", [(17, 16), (16, 3)])
def test_a_poisoned_row_poisons_only_itself(N, row):
    T, H = 5, 48
    p = problem(N, T, H, True, seed=6)
    clean = stack32(p)
    q = dict(p, gi0=p["gi0"].clone())
    q["gi0"][row, 2, 7] = float("nan")
    bad = stack32(q)
    others = [s for s in range(N) if s != row]
    for k in ("y0", "y1", "y2", "dgi0"):
        assert_bits_equal(u32(bad[k][others]), u32(clean[k][others]), k)
        assert torch.isnan(bad[k][row, 2:]).any() and not torch.isnan(bad[k][others]).any(), k
    for l in L3:  # the poison reaches every layer at step 2, and none before
        assert torch.isnan(bad[f"y{l}"][row, 2]).any(), l
        assert_bits_equal(u32(bad[f"y{l}"][row, :2]), u32(clean[f"y{l}"][row, :2]), f"layer {l}: the row before the poison")
    assert_bits_equal(u32(bad["dh0"][:, others]), u32(clean["dh0"][:, others]), "dh0")
    assert_bits_equal(u32(bad["dgh"][:, :, others]), u32(clean["dgh"][:, :, others]), "dgh")
    assert_bits_equal(u32(bad["dgi_upper"][:, :, others]), u32(clean["dgi_upper"][:, :, others]), "dgi of layers 2, 3")


# ---- the network ----
@pytest.mark.parametrize("cond,gru,N,T", [(16, 32, 4, 24), (128, 384, 3, 12)])
def test_float_net_stack_beside_torch(cond, gru, N, T):
    """gains, vad and every parameter gradient of (gains A).sum() + (vad B).sum(): the bound, X64 the float64 CPU net"""
    from rnnoise_amd import train
    net64 = train.new_network(cond, gru, seed=9).double()
    gen = torch.Generator().manual_seed(10)
    x = torch.randn(N, T, 65, generator=gen)
    A, B = torch.randn(N, T - 4, 32, generator=gen), torch.randn(N, T - 4, 1, generator=gen)
    want = net_outputs(net64, x.double(), A.double(), B.double())
    net = train.new_network(cond, gru, seed=9).to(DEV)
    net.load_state_dict({k: v.float() for k, v in net64.state_dict().items()})
    other = net_outputs(net, x.to(DEV), A.to(DEV), B.to(DEV))
    net.gru_impl = "stack"
    got = net_outputs(net, x.to(DEV), A.to(DEV), B.to(DEV))
    assert set(got) == set(want) and len(got) == 22
    r = ratios(got, other, want, names=sorted(want))
    print(f"FloatNet {cond}/{gru}: largest ratio {max(r.values()):.3f} ({max(r, key=r.get)})")
    for k, v in r.items():
        assert v <= 4.0, (k, v)
    # the streaming view runs the same layers: calls of uneven lengths carry the stack's states
    stream = {}
    for impl in ("torch", "stack"):
        net.gru_impl = impl
        net.reset()
        with torch.no_grad():
            g = torch.cat([net(x[:, a:b].to(DEV))[0] for a, b in ((0, 3), (3, 9), (9, T))], dim=1)
        assert torch.all(g[:, :4] == 0)
        stream[impl] = dict(gains=g[:, 4:])
    assert ratios(stream["stack"], stream["torch"], want, names=("gains",))["gains"] <= 4.0


def test_fit_stack_beside_fit_torch(tmp_path):
    from rnnoise_amd import train
    records = R.training_records(np.random.default_rng(8), 4, 24)
    runs = {}
    for impl in ("torch", "stack"):
        steps = []
        hist = train.fit(train.RecordFile(records, 24, 4), str(tmp_path / impl), epochs=3, cond_size=16, gru_size=32, seed=7, gru=impl,
                         on_step=lambda info: steps.append((info["loss"], info["gain_loss"], info["vad_loss"])), log=None)
        runs[impl] = (hist, steps)
    hist, steps = runs["stack"]
    assert len(steps) == 3 and np.all(np.isfinite(steps)) and all(np.isfinite(h["loss"]) for h in hist)
    a, b = (torch.load(runs[k][0][-1]["checkpoint"], map_location="cpu") for k in ("stack", "torch"))
    assert set(a) == set(b) and a["model_kwargs"] == b["model_kwargs"]
    assert list(a["state_dict"]) == list(b["state_dict"])
    assert all(a["state_dict"][k].shape == b["state_dict"][k].shape and a["state_dict"][k].dtype == b["state_dict"][k].dtype for k in a["state_dict"])
    # the first step's three losses: float64 on the CPU from the same initialisation and the same shuffled batch
    net64 = train.new_network(16, 32, seed=7).double()
    feats, rec = next(iter(train.RecordFile(records, 24, 4).batches(np.random.default_rng(7), "cpu")))
    with torch.no_grad():
        g, v = net64.forward_sequence(feats.double())
        want = R.trainer_loss(g, v, rec[:, 3:-1, R.FEATURES:R.FEATURES + R.BANDS].double(), rec[:, 3:-1, R.REC - 1:].double(), .25)
    for k, w in enumerate(want):
        w = float(w)
        e_n, e_t = abs(runs["stack"][1][0][k] - w), abs(runs["torch"][1][0][k] - w)
        print(f"first step, loss {k}: float64 {w:.12g}, stack off by {e_n:.3e}, torch by {e_t:.3e}")
        assert e_n <= 4 * max(e_t, 1e-6 * abs(w)), (k, e_n, e_t, w)


def test_cli_train_stack_then_export(tmp_path):
    records = R.training_records(np.random.default_rng(9), 2, 12)
    rec = tmp_path / "rec.f32"
    records.tofile(str(rec))
    out = tmp_path / "run"
    run = lambda *argv: subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    r = run("train", str(rec), str(out), "--gru", "stack", "--epochs", "1", "--batch-size", "2", "--sequence-length", "12", "--seed", "5")
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("epoch 1: loss ") and "(1 batches, step 1)" in line and np.isfinite(float(line.split()[3]))
    ckpt = out / "checkpoints" / "rnnoise_1.pth"
    assert ckpt.exists()
    r = run("export", str(ckpt), str(tmp_path / "net.blob"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "net.blob").read_bytes()[:4] == b"DNNw"
