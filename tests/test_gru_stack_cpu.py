"""CPU checks of the gru stack library (include/rnnoise_amd_gru_stack.h, rnnoise_amd/csrc/gru_stack/gru_stack.hip,
rnnoise_amd/gru_stack.py): the formulas of the header in plain torch against three chained nn.GRU and torch's autograd in float64;
what the library declares, exports, accepts and refuses (its host-only calls run here: nothing is dereferenced and no device is
touched); and the switch value "stack" in FloatNet, fit and the command line.  (The kernels themselves: tests/test_gru_stack_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import train_loss_ref as R
from gru_cases import _declarations, _fields, _injected_loss, assert_shares_only_the_two_headers
from rnnoise_amd import capi, float_net, train
from rnnoise_amd import gru_native
from rnnoise_amd import gru_stack as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
HEADER = os.path.join(ROOT, "include", "rnnoise_amd_gru_stack.h")


# ---- the formulas ----
@pytest.mark.parametrize("N,T,H", [(3, 5, 16), (17, 35, 48)])
@pytest.mark.parametrize("with_states", [False, True])
def test_reference_formulas_against_three_nn_gru_in_float64(N, T, H, with_states):
    """y1 .. y3, dgi0 (through dx and dW_ih of layer 1, which are products of it), dW_ih and db_ih of layers 2 and 3, dW_hh and db_hh
    of all three, dh0 of all three: 1e-12 absolute"""
    gen = torch.Generator().manual_seed(1000 * N + T)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    grus = [torch.nn.GRU(H, H, batch_first=True).double() for _ in range(3)]
    with torch.no_grad():
        for g in grus:
            for p in g.parameters():
                p.copy_(rnd(*p.shape) * .3)
    x = rnd(N, T, H).requires_grad_(True)
    h0 = [rnd(N, H).requires_grad_(True) if with_states else None for _ in range(3)]
    dy, dhT = [rnd(N, T, H) for _ in range(3)], [rnd(N, H) if with_states else None for _ in range(3)]
    want_y, inp, loss = [], x, 0
    for l, g in enumerate(grus):
        y, hT = g(inp, None if h0[l] is None else h0[l].unsqueeze(0))
        want_y.append(y)
        loss = loss + (y * dy[l]).sum() + ((hT[0] * dhT[l]).sum() if with_states else 0)
        inp = y
    loss.backward()

    err = lambda a, b: float((a - b).abs().max())
    with torch.no_grad():
        gi0 = torch.nn.functional.linear(x, grus[0].weight_ih_l0, grus[0].bias_ih_l0)
        w_ih, b_ih = [None] + [g.weight_ih_l0 for g in grus[1:]], [None] + [g.bias_ih_l0 for g in grus[1:]]
        w_hh, b_hh = [g.weight_hh_l0 for g in grus], [g.bias_hh_l0 for g in grus]
        h0_ = [None if h is None else h.detach() for h in h0]
        y, saved = S.gru_stack_ref(gi0, w_ih, b_ih, w_hh, b_hh, h0_, return_saved=True)
        assert saved.shape == (3, T, N, 4 * H)
        out = S.gru_stack_ref_backward(dy, y, saved, w_ih, w_hh, h0_, dhT)
        for l in range(3):
            assert err(y[l], want_y[l]) <= 1e-12, l
            assert err(out["dW_hh"][l], grus[l].weight_hh_l0.grad) <= 1e-12 and err(out["db_hh"][l], grus[l].bias_hh_l0.grad) <= 1e-12, l
            if with_states:
                assert err(out["dh0"][l], h0[l].grad) <= 1e-12, l
        dgi0 = out["dgi"][0]
        assert err(dgi0 @ grus[0].weight_ih_l0, x.grad) <= 1e-12                                                    # dx
        assert err(dgi0.reshape(-1, 3 * H).t() @ x.detach().reshape(-1, H), grus[0].weight_ih_l0.grad) <= 1e-12      # dW_ih of layer 1
        assert err(dgi0.sum((0, 1)), grus[0].bias_ih_l0.grad) <= 1e-12
        for l in (1, 2):
            assert err(out["dW_ih"][l], grus[l].weight_ih_l0.grad) <= 1e-12 and err(out["db_ih"][l], grus[l].bias_ih_l0.grad) <= 1e-12, l
        assert out["dW_ih"][0] is None and out["db_ih"][0] is None
        # the wrapper's two torch-side forms of dW_ih give the formula's number
        for per_step in (True, False):
            dW, db = S.input_weight_grads(out["dgi"][1].transpose(0, 1).contiguous(), y[0], per_step=per_step)
            assert err(dW, out["dW_ih"][1]) <= 1e-12 and err(db, out["db_ih"][1]) <= 1e-12


# ---- the surface ----
def test_prototype_table_matches_the_header():
    decl = _declarations(HEADER)
    assert [d[1] for d in decl] == list(S.PROTOTYPES) == S.EXPORTS and len(decl) == 5
    assert S.EXPORTS == ["rnnoise_amd_gru_stack_check", "rnnoise_amd_gru_stack_grad_check", "rnnoise_amd_gru_stack_workspace",
                         "rnnoise_amd_gru_stack_forward_device", "rnnoise_amd_gru_stack_backward_device"]
    for ret, name, params in decl:
        restype, argtypes = S.PROTOTYPES[name]
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == params.count(",") + 1, (name, params)
    src = open(HEADER).read()
    for macro, value in (("LAYERS", S.LAYERS), ("TILE", S.TILE), ("MIN_HIDDEN", S.MIN_HIDDEN), ("MAX_HIDDEN", S.MAX_HIDDEN),
                         ("MAX_ROWS", S.MAX_ROWS)):
        assert int(re.search(rf"#define RNNOISE_AMD_GRU_STACK_{macro} (\d+)", src)[1]) == value, macro
    assert S.LAYERS == 3
    # the limits are the gru library's
    assert (S.TILE, S.MIN_HIDDEN, S.MAX_HIDDEN, S.MAX_ROWS) == (gru_native.TILE, gru_native.MIN_HIDDEN, gru_native.MAX_HIDDEN, gru_native.MAX_ROWS)
    same = lambda a, b: [(n, (t._type_, t._length_) if hasattr(t, "_length_") else t) for n, t in a] == \
                        [(n, (t._type_, t._length_) if hasattr(t, "_length_") else t) for n, t in b]
    assert same(_fields(HEADER, "RNNoiseGruStack"), S.Stack._fields_)
    assert same(_fields(HEADER, "RNNoiseGruStackGrad"), S.StackGrad._fields_)


def test_library_exports_the_header_and_nothing_else():
    nm = subprocess.run(["nm", "-D", "--defined-only", S.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert syms == set(S.EXPORTS), sorted(syms ^ set(S.EXPORTS))
    L = S.lib()
    assert all(hasattr(L, n) for n in S.EXPORTS)


def test_two_kernels_of_its_own_and_nothing_shared():
    """name sets only"""
    strings = lambda p: subprocess.run(["strings", "-a", p], capture_output=True, text=True, check=True).stdout
    own = strings(S.LIB_PATH)
    assert set(re.findall(r"\b(rn_\w+)\.kd\b", own)) == set(S.KERNELS) == {"rn_gru_stack_kernel", "rn_gru_stack_grad_kernel"}
    assert not re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", own)  # no environment variable
    for name in ("librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so", "librnnoise_amd_score.so", "librnnoise_amd_train.so",
                 "librnnoise_amd_gru.so"):
        assert "rn_gru_stack" not in strings(os.path.join(PKG, name)), name
    ldd = subprocess.run(["ldd", S.LIB_PATH], capture_output=True, text=True).stdout
    assert "librnnoise" not in ldd
    for header in ("rnnoise_amd.h", "rnnoise_amd_gru.h"):
        assert "gru_stack" not in open(os.path.join(ROOT, "include", header)).read(), header
    assert not [n for n in list(capi.PROTOTYPES) + list(gru_native.PROTOTYPES) if "gru_stack" in n]
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "build_gru_stack" in re.search(r"^clean:\n\t(.*)$", mk, re.M)[1] and "librnnoise_amd_gru_stack.so" in re.search(r"^all:(.*)$", mk, re.M)[1]
    assert_shares_only_the_two_headers(PKG, os.path.join("gru_stack", "gru_stack.hip"), "rnnoise_amd_gru_stack.h")
    assert "rnnoise_amd_gru.h" not in open(os.path.join(PKG, "csrc", "gru_stack", "gru_stack.hip")).read()


# ---- the argument checks ----
N_, T_, H_ = 3, 10, 32
MB = 1 << 20
Y_ = [(3 * MB, N_ * H_, H_), (9 * MB, N_ * H_, H_), (10 * MB, N_ * H_, H_)]      # three [frame][row] buffers at made-up addresses
CAT_ = [(3 * MB + 4 * (l + 1) * H_, 4 * H_, T_ * 4 * H_) for l in range(3)]      # slices 1 .. 3 of a batch-first [N][T][4H] buffer
CAT_FM_ = [(3 * MB + 4 * (l + 1) * H_, N_ * 4 * H_, 4 * H_) for l in range(3)]   # ... of a frame-major [T][N][4H] one


def _three(base, **at):
    """three values, `at` replacing some by index (l0=..., l1=..., l2=...)"""
    v = list(base)
    for k, x in at.items():
        v[int(k[1])] = x
    return v


def _stack(**kw):
    """a forward call that is accepted: 3 rows, 10 steps, H 32"""
    d = dict(gi0=(4096, N_ * 3 * H_, 3 * H_), w_ih=[0, 11 * MB, 12 * MB], b_ih=[0, 13 * MB, 14 * MB], w_hh=[1 * MB, 15 * MB, 16 * MB],
             b_hh=[2 * MB, 17 * MB, 18 * MB], y=Y_, n_rows=N_, n_frames=T_, hidden=H_, h0=[4 * MB, 19 * MB, 20 * MB])
    d.update(kw)
    return S.make_stack(**d)


DGI_, DGH_, DH0_, DHT_ = [0, 21 * MB, 22 * MB], [6 * MB, 23 * MB, 24 * MB], [7 * MB, 25 * MB, 31 * MB], [8 * MB, 26 * MB, 32 * MB]  # dhT[l] = dh0[l] + MB
DY_ = [(4096, N_ * H_, H_), (29 * MB, N_ * H_, H_), (30 * MB, N_ * H_, H_)]


def _grad(**kw):
    d = dict(dy=DY_, y=Y_, w_ih=[0, 11 * MB, 12 * MB], w_hh=[1 * MB, 15 * MB, 16 * MB], dgi0=(5 * MB, N_ * 3 * H_, 3 * H_), dgi=DGI_, dgh=DGH_,
             dh0=DH0_, n_rows=N_, n_frames=T_, hidden=H_, h0=[4 * MB, 19 * MB, 20 * MB], dhT=DHT_)
    d.update(kw)
    return S.make_grad(**d)


def _per_layer(name, base, bad, layers=(0, 1, 2)):
    return {f"{name}_{l}": _three(base, **{f"l{l}": bad(base[l])}) for l in layers}


STACK_REFUSED = dict(
    null_gi0=dict(gi0=(0, 288, 96)), no_rows=dict(n_rows=0), negative_rows=dict(n_rows=-1), negative_frames=dict(n_frames=-1),
    too_many_rows=dict(n_rows=S.MAX_ROWS + 1, gi0=(4096, 96, 960), y=[(p, 32, 320) for p in (1 << 40, 2 << 40, 3 << 40)]),
    hidden_8=dict(hidden=8, gi0=(4096, 72, 24), y=[(p, 24, 8) for p, _, _ in Y_]),
    hidden_24=dict(hidden=24, gi0=(4096, 216, 72), y=[(p, 72, 24) for p, _, _ in Y_]), hidden_0=dict(hidden=0),
    hidden_above=dict(hidden=S.MAX_HIDDEN + 16, gi0=(4096, 9 * (S.MAX_HIDDEN + 16), 3 * (S.MAX_HIDDEN + 16)),
                      y=[(p, 3 * (S.MAX_HIDDEN + 16), S.MAX_HIDDEN + 16) for p, _, _ in Y_]),
    gi0_rows_overlap=dict(gi0=(4096, 288, 92)), gi0_frames_overlap=dict(gi0=(4096, 284, 96)), gi0_unaligned=dict(gi0=(4096 + 4, 288, 96)),
    stride_negative=dict(gi0=(4096, -288, 96)), extent_overflow=dict(gi0=(4096, 2 ** 62, 96)),
    # two layers' outputs on each other: the same buffer, a buffer that starts inside another's extent, slices of a concatenation
    # that are too close, slices with different strides
    y_1_on_0=dict(y=_three(Y_, l1=Y_[0])), y_2_into_1=dict(y=_three(Y_, l2=(9 * MB + 4 * 16, N_ * H_, H_))),
    y_2_on_0=dict(y=_three(Y_, l2=(3 * MB + 4 * (N_ * H_ * T_ - 4), N_ * H_, H_))),
    cat_slices_overlap=dict(y=_three(CAT_, l2=(CAT_[1][0] + 4 * 16, 4 * H_, T_ * 4 * H_))),
    cat_slice_over_the_pitch=dict(y=_three(CAT_, l2=(CAT_[0][0] + 4 * (4 * H_ - 16), 4 * H_, T_ * 4 * H_))),
    cat_other_strides=dict(y=_three(CAT_, l2=(CAT_[2][0], 4 * H_, (T_ + 1) * 4 * H_))),
)
for _name, _base, _bad in (("null_w_hh", [1 * MB, 15 * MB, 16 * MB], lambda p: 0), ("null_b_hh", [2 * MB, 17 * MB, 18 * MB], lambda p: 0),
                           ("w_hh_unaligned", [1 * MB, 15 * MB, 16 * MB], lambda p: p + 4), ("b_hh_unaligned", [2 * MB, 17 * MB, 18 * MB], lambda p: p + 2),
                           ("h0_unaligned", [4 * MB, 19 * MB, 20 * MB], lambda p: p + 4)):
    _key = _name.replace("null_", "").replace("_unaligned", "")
    STACK_REFUSED.update({k: {_key: v} for k, v in _per_layer(_name, _base, _bad).items()})
for _name, _key, _base, _bad in (("null_w_ih", "w_ih", [0, 11 * MB, 12 * MB], lambda p: 0), ("null_b_ih", "b_ih", [0, 13 * MB, 14 * MB], lambda p: 0),
                                 ("w_ih_unaligned", "w_ih", [0, 11 * MB, 12 * MB], lambda p: p + 8), ("b_ih_unaligned", "b_ih", [0, 13 * MB, 14 * MB], lambda p: p + 1)):
    STACK_REFUSED.update({k: {_key: v} for k, v in _per_layer(_name, _base, _bad, layers=(1, 2)).items()})
for _name, _bad in (("null_y", lambda s: (0, s[1], s[2])), ("y_unaligned", lambda s: (s[0] + 8, s[1], s[2])), ("y_rows_overlap", lambda s: (s[0], 96, 28)),
                    ("y_frames_overlap", lambda s: (s[0], 92, 32)), ("y_stride_zero", lambda s: (s[0], 0, 0)), ("y_stride_odd", lambda s: (s[0], 98, 32)),
                    ("y_row_major_short", lambda s: (s[0], 32, 32 * 9))):
    STACK_REFUSED.update({k: dict(y=v) for k, v in _per_layer(_name, Y_, _bad).items()})
STACK_ACCEPTED = (dict(), dict(h0=[0, 0, 0]), dict(h0=[4 * MB, 0, 20 * MB]), dict(n_frames=0), dict(n_frames=0, y=[Y_[0]] * 3),  # (no slot: nothing to overlap)
                  dict(w_ih=[4, 11 * MB, 12 * MB], b_ih=[2, 13 * MB, 14 * MB]),  # index 0 is not looked at
                  dict(gi0=(4096, 96, 960), y=CAT_), dict(y=CAT_FM_), dict(y=[CAT_[2], CAT_[0], CAT_[1]]),
                  dict(y=_three(Y_, l1=(3 * MB + 4 * N_ * H_ * T_, N_ * H_, H_))),  # right behind layer 0's
                  dict(gi0=(4096, 300, 100), y=[(p, 120, 36) for p, _, _ in Y_]),
                  dict(hidden=16, gi0=(4096, 144, 48), y=[(p, 48, 16) for p, _, _ in Y_]), dict(n_rows=1), dict(b_hh=[2 * MB + 4, 17 * MB, 18 * MB]),
                  dict(hidden=S.MAX_HIDDEN, gi0=(4096, 9 * S.MAX_HIDDEN, 3 * S.MAX_HIDDEN), y=[(p, 3 * S.MAX_HIDDEN, S.MAX_HIDDEN) for p, _, _ in Y_]))

GRAD_REFUSED = dict(
    no_rows=dict(n_rows=0), negative_frames=dict(n_frames=-1), hidden_8=dict(hidden=8), hidden_24=dict(hidden=24),
    null_dgi0=dict(dgi0=(0, 288, 96)), dgi0_overlap=dict(dgi0=(5 * MB, 288, 92)), dgi0_frames_overlap=dict(dgi0=(5 * MB, 284, 96)),
    dgi0_unaligned=dict(dgi0=(5 * MB + 4, 288, 96)),
)
for _name, _key, _base, _bad, _layers in (
        ("null_w_hh", "w_hh", [1 * MB, 15 * MB, 16 * MB], lambda p: 0, (0, 1, 2)), ("null_w_ih", "w_ih", [0, 11 * MB, 12 * MB], lambda p: 0, (1, 2)),
        ("null_dgi", "dgi", DGI_, lambda p: 0, (1, 2)), ("dgi_unaligned", "dgi", DGI_, lambda p: p + 4, (1, 2)),
        ("null_dgh", "dgh", DGH_, lambda p: 0, (0, 1, 2)), ("dgh_unaligned", "dgh", DGH_, lambda p: p + 4, (0, 1, 2)),
        ("null_dh0", "dh0", DH0_, lambda p: 0, (0, 1, 2)), ("dhT_unaligned", "dhT", DHT_, lambda p: p + 8, (0, 1, 2)),
        ("dh0_on_dhT", "dh0", DH0_, lambda p: p + MB, (0, 1, 2)), ("dh0_into_dhT", "dh0", DH0_, lambda p: p + MB + 4 * (N_ * H_ - 4), (0, 1, 2)),
        ("dhT_into_dh0", "dhT", DHT_, lambda p: p - MB + 16, (0, 1, 2)),
        ("null_dy", "dy", DY_, lambda s: (0, s[1], s[2]), (0, 1, 2)), ("dy_overlap", "dy", DY_, lambda s: (s[0], 96, 28), (0, 1, 2)),
        ("null_y", "y", Y_, lambda s: (0, s[1], s[2]), (0, 1, 2)), ("y_overlap", "y", Y_, lambda s: (s[0], 92, 32), (0, 1, 2))):
    GRAD_REFUSED.update({k: {_key: v} for k, v in _per_layer(_name, _base, _bad, _layers).items()})
GRAD_ACCEPTED = (dict(), dict(h0=[0, 0, 0], dhT=[0, 0, 0]), dict(n_frames=0), dict(dy=CAT_, y=CAT_, dgi0=(5 * MB, 96, 960)), dict(dy=CAT_FM_, y=CAT_FM_),
                 dict(dy=[DY_[0]] * 3),  # inputs may be the same memory
                 dict(dh0=_three(DH0_, l1=DHT_[1] + 4 * N_ * H_)),  # dh0 right behind dhT
                 dict(dh0=_three(DH0_, l2=DHT_[2] + 4 * N_ * H_)), dict(w_ih=[4, 11 * MB, 12 * MB]))


def test_check_accepts_and_refuses():
    L = S.lib()
    assert L.rnnoise_amd_gru_stack_check(None) == -1 and L.rnnoise_amd_gru_stack_grad_check(None) == -1
    assert len(STACK_REFUSED) >= 60 and len(GRAD_REFUSED) > 40
    for kw in STACK_ACCEPTED:
        assert S.check(_stack(**kw)), kw
    for name, kw in STACK_REFUSED.items():
        assert not S.check(_stack(**kw)), name
    for kw in GRAD_ACCEPTED:
        assert S.check(_grad(**kw)), kw
    for name, kw in GRAD_REFUSED.items():
        assert not S.check(_grad(**kw)), name


def test_device_calls_refuse_before_they_touch_a_pointer_or_a_device():
    """every pointer of these calls is a made-up address and this process has no device: a call that went on would not come back"""
    L = S.lib()
    for name, kw in STACK_REFUSED.items():
        assert L.rnnoise_amd_gru_stack_forward_device(0, C.byref(_stack(**kw)), C.c_void_p(64), None) == -1, name
    for name, kw in GRAD_REFUSED.items():
        assert L.rnnoise_amd_gru_stack_backward_device(0, C.byref(_grad(**kw)), C.c_void_p(64), C.c_void_p(128), None) == -1, name
    assert L.rnnoise_amd_gru_stack_forward_device(0, C.byref(_stack()), None, None) == -1            # no saved
    assert L.rnnoise_amd_gru_stack_forward_device(0, C.byref(_stack()), C.c_void_p(68), None) == -1  # unaligned saved
    assert L.rnnoise_amd_gru_stack_backward_device(0, C.byref(_grad()), None, C.c_void_p(128), None) == -1
    assert L.rnnoise_amd_gru_stack_backward_device(0, C.byref(_grad()), C.c_void_p(64), None, None) == -1
    assert L.rnnoise_amd_gru_stack_backward_device(0, C.byref(_grad()), C.c_void_p(64), C.c_void_p(132), None) == -1
    assert L.rnnoise_amd_gru_stack_forward_device(0, None, None, None) == -1
    assert L.rnnoise_amd_gru_stack_backward_device(0, None, None, None, None) == -1
    # an empty call is accepted and does nothing
    assert L.rnnoise_amd_gru_stack_forward_device(0, C.byref(_stack(n_frames=0)), C.c_void_p(64), None) == 0
    assert L.rnnoise_amd_gru_stack_backward_device(0, C.byref(_grad(n_frames=0)), C.c_void_p(64), C.c_void_p(128), None) == 0
    with pytest.raises(ValueError):
        S.forward_device(_stack(hidden=24), 64)
    with pytest.raises(ValueError):
        S.backward_device(_grad(dgh=[0, 0, 0]), 64, 128)


def test_workspace_sizes_are_the_documented_formulas():
    for N, T, H in ((1, 0, 16), (3, 10, 32), (17, 35, 48), (128, 1996, 384), (67, 1, 1024)):
        assert S.workspace(N, T, H) == (3 * T * N * 4 * H, (3 + 2) * 2 * N * H)
    L = S.lib()
    c, one = _stack(), C.c_size_t(7)
    assert L.rnnoise_amd_gru_stack_workspace(C.byref(c), None, C.byref(one)) == 0 and one.value == 10 * N_ * H_  # either result may be left out
    assert L.rnnoise_amd_gru_stack_workspace(C.byref(c), C.byref(one), None) == 0 and one.value == 3 * T_ * N_ * 4 * H_
    assert L.rnnoise_amd_gru_stack_workspace(None, None, None) == -1
    for N, T, H in ((0, 1, 16), (1, -1, 16), (1, 1, 8), (1, 1, 24), (1, 1, S.MAX_HIDDEN + 16)):
        with pytest.raises(ValueError):
            S.workspace(N, T, H)


# ---- the launch schedule on the host, under the sanitizers ----
def test_launch_schedule_reads_what_an_earlier_launch_wrote(tmp_path):
    """tests/csrc/gru_stack_main.cpp: the unit's host half (and the gru library's, as a stack of one layer) as plain C++ with every
    launch handed to a model of the memory -- which layer runs which step in launch s, what it reads and writes, and that the kernel
    boundary is ordering enough; with the address and undefined-behaviour sanitizers on the host code"""
    exe = str(tmp_path / "gru_stack_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-Wno-unknown-pragmas", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "csrc"),
                    "-I", os.path.join(PKG, "csrc", "gru_stack"), "-I", os.path.join(PKG, "csrc", "gru"),
                    os.path.join(ROOT, "tests", "csrc", "gru_stack_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == "ok 192"  # 96 shapes, the stack and the single layer on each


# ---- the switch ----
def test_float_net_stack_raises_on_the_cpu_and_the_default_is_unchanged():
    torch.manual_seed(2)
    plain, stack = float_net.FloatNet(8, 16), float_net.FloatNet(8, 16, gru_impl="stack")
    assert plain.gru_impl == "torch" and stack.gru_impl == "stack" and float_net.GRU_IMPLS == ("torch", "native", "stack")
    assert list(plain.state_dict()) == list(stack.state_dict()) and len(plain.state_dict()) == 20
    x = torch.randn(2, 9, 65)
    with pytest.raises(ValueError, match="stack"):
        stack.forward_sequence(x)
    with pytest.raises(ValueError, match="stack"):
        stack(x)
    with pytest.raises(ValueError, match="stack"):
        stack.double().forward_sequence(x.double())
    stack.float()
    stack.gru_impl = "torch"  # set afterwards: the same module runs torch's GRUs
    plain.load_state_dict(stack.state_dict())
    for a, b in zip(stack.forward_sequence(x), plain.forward_sequence(x)):
        assert torch.equal(a, b)
    z = torch.zeros
    with pytest.raises(ValueError):  # CPU tensors: no silent fallback
        S.GruStack.apply(z(2, 3, 48), z(48, 16), z(48), z(48, 16), z(48), z(48, 16), z(48, 16), z(48, 16), z(48), z(48), z(48), None, None, None)


def test_load_checkpoint_leaves_the_default(tmp_path):
    net = float_net.FloatNet(8, 16, gru_impl="stack")
    path = str(tmp_path / "ck.pth")
    torch.save(dict(state_dict=net.state_dict(), model_kwargs=dict(cond_size=8, gru_size=16)), path)
    assert float_net.load_checkpoint(path).gru_impl == "torch"


def test_fit_stack_raises_on_the_cpu(tmp_path):
    records = R.training_records(np.random.default_rng(1), 4, 12)
    with pytest.raises(ValueError, match="stack"):  # the stack does not run on the CPU, and says so
        train.fit(train.RecordFile(records, 12, 4), str(tmp_path / "c"), epochs=1, cond_size=8, gru_size=16, seed=5, loss=_injected_loss,
                  device="cpu", log=None, gru="stack")
    with pytest.raises(ValueError):
        train.new_network(8, 16, gru="diagonal")


def test_train_command_takes_the_switch(monkeypatch, capsys):
    from rnnoise_amd import cli
    seen = {}
    monkeypatch.setattr(train, "train_files", lambda **kw: (seen.clear(), seen.update(kw)))
    cli.main(["train", "rec.f32", "out"])
    assert "gru" not in seen  # the default run passes what it passed before
    cli.main(["train", "rec.f32", "out", "--gru", "stack"])
    assert seen["gru"] == "stack" and seen["records"] == "rec.f32"
    cli.main(["train", "rec.f32", "out", "--gru", "native"])
    assert seen["gru"] == "native"
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.main(["train", "--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "librnnoise_amd_gru_stack.so" in out and "librnnoise_amd_gru.so" in out
