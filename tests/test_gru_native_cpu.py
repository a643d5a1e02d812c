"""CPU checks of the gru library (include/rnnoise_amd_gru.h, rnnoise_amd/csrc/gru/gru_seq.hip, rnnoise_amd/gru_native.py): the
formulas of the header in plain torch against nn.GRU and torch's autograd in float64; what the library declares, exports, accepts and
refuses (its host-only calls run here: nothing is dereferenced and no device is touched); and the switch in FloatNet and fit, whose
default leaves everything as it was.  (The kernels themselves: tests/test_gru_native_gpu.py.)"""
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
from rnnoise_amd import gru_native as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
HEADER = os.path.join(ROOT, "include", "rnnoise_amd_gru.h")


# ---- the formulas ----
@pytest.mark.parametrize("N,T,H", [(3, 5, 16), (17, 35, 48)])
@pytest.mark.parametrize("with_h0", [False, True])
@pytest.mark.parametrize("with_dhT", [False, True])
def test_reference_formulas_against_nn_gru_in_float64(N, T, H, with_h0, with_dhT):
    """y, dgi (through dx and dW_ih, which are products of it), dW_hh, db_hh, dh0: 1e-12 absolute"""
    gen = torch.Generator().manual_seed(1000 * N + T)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    gru = torch.nn.GRU(H, H, batch_first=True).double()
    with torch.no_grad():
        for p in gru.parameters():
            p.copy_(rnd(*p.shape) * .3)
    x = rnd(N, T, H).requires_grad_(True)
    h0 = rnd(N, H).requires_grad_(True) if with_h0 else None
    dy, dhT = rnd(N, T, H), (rnd(N, H) if with_dhT else None)
    want_y, want_hT = gru(x, None if h0 is None else h0.unsqueeze(0))
    loss = (want_y * dy).sum() + ((want_hT[0] * dhT).sum() if with_dhT else 0)
    loss.backward()

    with torch.no_grad():
        gi = torch.nn.functional.linear(x, gru.weight_ih_l0, gru.bias_ih_l0)
        h0_ = None if h0 is None else h0.detach()
        y, saved = G.gru_sequence_ref(gi, gru.weight_hh_l0, gru.bias_hh_l0, h0_, return_saved=True)
        assert saved.shape == (T, N, 4 * H)
        dgi, dW, db, dh0 = G.gru_sequence_ref_backward(dy, y, saved, gru.weight_hh_l0, h0_, dhT)
        err = lambda a, b: float((a - b).abs().max())
        assert err(y, want_y) <= 1e-12 and err(y[:, -1], want_hT[0]) <= 1e-12
        assert err(dgi @ gru.weight_ih_l0, x.grad) <= 1e-12                                                # dx
        assert err(dgi.reshape(-1, 3 * H).t() @ x.detach().reshape(-1, H), gru.weight_ih_l0.grad) <= 1e-12  # dW_ih
        assert err(dgi.sum((0, 1)), gru.bias_ih_l0.grad) <= 1e-12
        assert err(dW, gru.weight_hh_l0.grad) <= 1e-12 and err(db, gru.bias_hh_l0.grad) <= 1e-12
        if with_h0:
            assert err(dh0, h0.grad) <= 1e-12
    # ... and the forward formulas are differentiable as they stand: autograd through them gives the backward formulas' numbers
    gi2 = gi.clone().requires_grad_(True)
    w2, b2 = gru.weight_hh_l0.detach().clone().requires_grad_(True), gru.bias_hh_l0.detach().clone().requires_grad_(True)
    y2 = G.gru_sequence_ref(gi2, w2, b2, h0_)
    ((y2 * dy).sum() + ((y2[:, -1] * dhT).sum() if with_dhT else 0)).backward()
    assert err(gi2.grad, dgi) <= 1e-12 and err(w2.grad, dW) <= 1e-12 and err(b2.grad, db) <= 1e-12


# ---- the surface ----
def test_prototype_table_matches_the_header():
    decl = _declarations(HEADER)
    assert [d[1] for d in decl] == list(G.PROTOTYPES) == G.EXPORTS and len(decl) == 5
    for ret, name, params in decl:
        restype, argtypes = G.PROTOTYPES[name]
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == params.count(",") + 1, (name, params)
    src = open(HEADER).read()
    for macro, value in (("TILE", G.TILE), ("MIN_HIDDEN", G.MIN_HIDDEN), ("MAX_HIDDEN", G.MAX_HIDDEN), ("MAX_ROWS", G.MAX_ROWS)):
        assert int(re.search(rf"#define RNNOISE_AMD_GRU_{macro} (\d+)", src)[1]) == value, macro
    assert G.MIN_HIDDEN <= 16 and G.MAX_HIDDEN >= 1024 and G.TILE == 16
    assert _fields(HEADER, "RNNoiseGruSeq") == list(G.Seq._fields_)
    assert _fields(HEADER, "RNNoiseGruSeqGrad") == list(G.SeqGrad._fields_)


def test_library_exports_the_header_and_nothing_else():
    nm = subprocess.run(["nm", "-D", "--defined-only", G.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert syms == set(G.EXPORTS), sorted(syms ^ set(G.EXPORTS))
    L = G.lib()
    assert all(hasattr(L, n) for n in G.EXPORTS)


def test_two_kernels_of_its_own_and_nothing_shared():
    """name sets only"""
    strings = lambda p: subprocess.run(["strings", "-a", p], capture_output=True, text=True, check=True).stdout
    own = strings(G.LIB_PATH)
    assert set(re.findall(r"\b(rn_\w+)\.kd\b", own)) == set(G.KERNELS) == {"rn_gru_step_kernel", "rn_gru_step_grad_kernel"}
    assert not re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", own)  # no environment variable
    for name in ("librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so", "librnnoise_amd_score.so", "librnnoise_amd_train.so"):
        assert "rn_gru_step" not in strings(os.path.join(PKG, name)), name
    ldd = subprocess.run(["ldd", G.LIB_PATH], capture_output=True, text=True).stdout
    assert "librnnoise" not in ldd
    assert "rnnoise_amd_gru" not in open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    assert not [n for n in capi.PROTOTYPES if "amd_gru" in n]
    assert_shares_only_the_two_headers(PKG, os.path.join("gru", "gru_seq.hip"), "rnnoise_amd_gru.h")


# ---- the argument checks ----
N_, T_, H_ = 3, 10, 32


def _seq(**kw):
    """a forward call that is accepted: 3 rows, 10 steps, H 32, [frame][row] buffers at made-up addresses"""
    d = dict(gi=(4096, N_ * 3 * H_, 3 * H_), w_hh=1 << 20, b_hh=2 << 20, y=(3 << 20, N_ * H_, H_), n_rows=N_, n_frames=T_, hidden=H_, h0=4 << 20)
    d.update(kw)
    return G.make_seq(**d)


def _grad(**kw):
    d = dict(dy=(4096, N_ * H_, H_), y=(3 << 20, N_ * H_, H_), w_hh=1 << 20, dgi=(5 << 20, N_ * 3 * H_, 3 * H_), dgh=6 << 20, dh0=7 << 20,
             n_rows=N_, n_frames=T_, hidden=H_, h0=4 << 20, dhT=8 << 20)
    d.update(kw)
    return G.make_grad(**d)


SEQ_REFUSED = dict(
    null_gi=dict(gi=(0, 288, 96)), null_w=dict(w_hh=0), null_b=dict(b_hh=0), null_y=dict(y=(0, 96, 32)),
    no_rows=dict(n_rows=0), negative_rows=dict(n_rows=-1), too_many_rows=dict(n_rows=G.MAX_ROWS + 1, gi=(4096, 96, 96 * 10), y=(3 << 20, 32, 320)),
    negative_frames=dict(n_frames=-1),
    hidden_8=dict(hidden=8, gi=(4096, 72, 24), y=(3 << 20, 24, 8)), hidden_24=dict(hidden=24, gi=(4096, 216, 72), y=(3 << 20, 72, 24)),
    hidden_0=dict(hidden=0), hidden_above=dict(hidden=G.MAX_HIDDEN + 16, gi=(4096, 3 * 3 * (G.MAX_HIDDEN + 16), 3 * (G.MAX_HIDDEN + 16)),
                                              y=(3 << 20, 3 * (G.MAX_HIDDEN + 16), G.MAX_HIDDEN + 16)),
    gi_rows_overlap=dict(gi=(4096, 288, 92)), gi_frames_overlap=dict(gi=(4096, 284, 96)),
    y_rows_overlap=dict(y=(3 << 20, 96, 28)), y_frames_overlap=dict(y=(3 << 20, 92, 32)),
    y_row_major_short=dict(y=(3 << 20, 32, 32 * 9)),  # [row][step] with rows of 9 steps for a call of 10
    stride_zero=dict(y=(3 << 20, 0, 0)), stride_negative=dict(gi=(4096, -288, 96)), stride_odd=dict(y=(3 << 20, 98, 32)),
    extent_overflow=dict(gi=(4096, 2 ** 62, 96)),
    gi_unaligned=dict(gi=(4096 + 4, 288, 96)), y_unaligned=dict(y=((3 << 20) + 8, 96, 32)), w_unaligned=dict(w_hh=(1 << 20) + 4),
    h0_unaligned=dict(h0=(4 << 20) + 4), b_unaligned=dict(b_hh=(2 << 20) + 2),
)
SEQ_ACCEPTED = (dict(), dict(h0=0), dict(n_frames=0), dict(gi=(4096, 96, 960), y=(3 << 20, 32, 320)),  # frames within a row: batch-first
                dict(gi=(4096, 300, 100), y=(3 << 20, 120, 36)), dict(gi=(4096, 100, 1000 + 12), y=(3 << 20, 36, 360 + 4)),  # padded, both orders
                dict(hidden=16, gi=(4096, 144, 48), y=(3 << 20, 48, 16)), dict(n_rows=1), dict(b_hh=(2 << 20) + 4),
                dict(hidden=G.MAX_HIDDEN, gi=(4096, 9 * G.MAX_HIDDEN, 3 * G.MAX_HIDDEN), y=(3 << 20, 3 * G.MAX_HIDDEN, G.MAX_HIDDEN)))
GRAD_REFUSED = dict(
    null_dy=dict(dy=(0, 96, 32)), null_y=dict(y=(0, 96, 32)), null_w=dict(w_hh=0), null_dgi=dict(dgi=(0, 288, 96)), null_dgh=dict(dgh=0),
    null_dh0=dict(dh0=0), no_rows=dict(n_rows=0), negative_frames=dict(n_frames=-1), hidden_8=dict(hidden=8), hidden_24=dict(hidden=24),
    dy_overlap=dict(dy=(4096, 96, 28)), y_overlap=dict(y=(3 << 20, 92, 32)), dgi_overlap=dict(dgi=(5 << 20, 288, 92)),
    dgi_frames_overlap=dict(dgi=(5 << 20, 284, 96)), dgh_unaligned=dict(dgh=(6 << 20) + 4), dhT_unaligned=dict(dhT=(8 << 20) + 8),
    dh0_on_dhT=dict(dh0=8 << 20), dh0_into_dhT=dict(dh0=(8 << 20) + 4 * (N_ * H_ - 4)), dhT_into_dh0=dict(dhT=(7 << 20) + 16),
)
GRAD_ACCEPTED = (dict(), dict(h0=0, dhT=0), dict(n_frames=0), dict(dy=(4096, 32, 320), y=(3 << 20, 32, 320), dgi=(5 << 20, 96, 960)),
                 dict(dh0=(8 << 20) + 4 * N_ * H_))  # dh0 right behind dhT


def test_check_accepts_and_refuses():
    L = G.lib()
    assert L.rnnoise_amd_gru_check(None) == -1 and L.rnnoise_amd_gru_grad_check(None) == -1
    for kw in SEQ_ACCEPTED:
        assert G.check(_seq(**kw)), kw
    for name, kw in SEQ_REFUSED.items():
        assert not G.check(_seq(**kw)), name
    for kw in GRAD_ACCEPTED:
        assert G.check(_grad(**kw)), kw
    for name, kw in GRAD_REFUSED.items():
        assert not G.check(_grad(**kw)), name


def test_device_calls_refuse_before_they_touch_a_pointer_or_a_device():
    """every pointer of these calls is a made-up address and this process has no device: a call that went on would not come back"""
    L = G.lib()
    for name, kw in SEQ_REFUSED.items():
        assert L.rnnoise_amd_gru_forward_device(0, C.byref(_seq(**kw)), C.c_void_p(64), None) == -1, name
    for name, kw in GRAD_REFUSED.items():
        assert L.rnnoise_amd_gru_backward_device(0, C.byref(_grad(**kw)), C.c_void_p(64), C.c_void_p(128), None) == -1, name
    assert L.rnnoise_amd_gru_forward_device(0, C.byref(_seq()), None, None) == -1            # no saved
    assert L.rnnoise_amd_gru_forward_device(0, C.byref(_seq()), C.c_void_p(68), None) == -1  # unaligned saved
    assert L.rnnoise_amd_gru_backward_device(0, C.byref(_grad()), None, C.c_void_p(128), None) == -1
    assert L.rnnoise_amd_gru_backward_device(0, C.byref(_grad()), C.c_void_p(64), None, None) == -1
    assert L.rnnoise_amd_gru_forward_device(0, None, None, None) == -1 and L.rnnoise_amd_gru_backward_device(0, None, None, None, None) == -1
    # an empty call is accepted and does nothing
    assert L.rnnoise_amd_gru_forward_device(0, C.byref(_seq(n_frames=0)), C.c_void_p(64), None) == 0
    assert L.rnnoise_amd_gru_backward_device(0, C.byref(_grad(n_frames=0)), C.c_void_p(64), C.c_void_p(128), None) == 0
    with pytest.raises(ValueError):
        G.forward_device(_seq(hidden=24), 64)
    with pytest.raises(ValueError):
        G.backward_device(_grad(dgh=0), 64, 128)


def test_workspace_sizes_are_the_documented_formulas():
    for N, T, H in ((1, 0, 16), (3, 10, 32), (17, 35, 48), (128, 1996, 384), (67, 1, 1024)):
        assert G.workspace(N, T, H) == (T * N * 4 * H, 2 * N * H)
    L = G.lib()
    c, one = _seq(), C.c_size_t(7)
    assert L.rnnoise_amd_gru_workspace(C.byref(c), None, C.byref(one)) == 0 and one.value == 2 * N_ * H_  # either result may be left out
    assert L.rnnoise_amd_gru_workspace(C.byref(c), C.byref(one), None) == 0 and one.value == T_ * N_ * 4 * H_
    assert L.rnnoise_amd_gru_workspace(None, None, None) == -1
    for N, T, H in ((0, 1, 16), (1, -1, 16), (1, 1, 8), (1, 1, 24), (1, 1, G.MAX_HIDDEN + 16)):
        with pytest.raises(ValueError):
            G.workspace(N, T, H)


# ---- the switch ----
def test_float_net_native_raises_on_the_cpu_and_the_default_is_unchanged():
    torch.manual_seed(2)
    plain, native = float_net.FloatNet(8, 16), float_net.FloatNet(8, 16, gru_impl="native")
    assert plain.gru_impl == "torch" and native.gru_impl == "native"
    assert list(plain.state_dict()) == list(native.state_dict()) == [
        "conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
        "gru1.weight_ih_l0", "gru1.weight_hh_l0", "gru1.bias_ih_l0", "gru1.bias_hh_l0",
        "gru2.weight_ih_l0", "gru2.weight_hh_l0", "gru2.bias_ih_l0", "gru2.bias_hh_l0",
        "gru3.weight_ih_l0", "gru3.weight_hh_l0", "gru3.bias_ih_l0", "gru3.bias_hh_l0",
        "dense_out.weight", "dense_out.bias", "vad_dense.weight", "vad_dense.bias"]
    x = torch.randn(2, 9, 65)
    with pytest.raises(ValueError, match="native"):
        native.forward_sequence(x)
    with pytest.raises(ValueError, match="native"):
        native(x)
    native.gru_impl = "torch"  # set afterwards: the same module runs torch's GRUs
    plain.load_state_dict(native.state_dict())
    for a, b in zip(native.forward_sequence(x), plain.forward_sequence(x)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        float_net.FloatNet(8, 16, gru_impl="fast")
    with pytest.raises(ValueError):
        G.GruSequence.apply(torch.zeros(2, 3, 48), torch.zeros(48, 16), torch.zeros(48), None)  # CPU tensors: no silent fallback


def test_load_checkpoint_leaves_the_default(tmp_path):
    net = float_net.FloatNet(8, 16, gru_impl="native")
    path = str(tmp_path / "ck.pth")
    torch.save(dict(state_dict=net.state_dict(), model_kwargs=dict(cond_size=8, gru_size=16)), path)
    assert float_net.load_checkpoint(path).gru_impl == "torch"


def test_fit_with_gru_torch_is_fit_without_the_argument(tmp_path):
    records = R.training_records(np.random.default_rng(1), 4, 12)
    run = lambda out, **kw: train.fit(train.RecordFile(records, 12, 4), str(tmp_path / out), epochs=3, cond_size=8, gru_size=16, seed=5,
                                      loss=_injected_loss, device="cpu", log=None, **kw)
    a, b = run("a"), run("b", gru="torch")
    strip = lambda hist: [{k: v for k, v in h.items() if k != "checkpoint"} for h in hist]
    assert strip(a) == strip(b) and len(a) == 3
    sa, sb = (torch.load(h[-1]["checkpoint"], map_location="cpu")["state_dict"] for h in (a, b))
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    with pytest.raises(ValueError, match="native"):  # the native GRUs do not run on the CPU, and say so
        run("c", gru="native")


def test_train_command_takes_the_switch(monkeypatch, capsys):
    from rnnoise_amd import cli
    seen = {}
    monkeypatch.setattr(train, "train_files", lambda **kw: (seen.clear(), seen.update(kw)))
    cli.main(["train", "rec.f32", "out"])
    assert "gru" not in seen  # the default run passes what it passed before
    cli.main(["train", "rec.f32", "out", "--gru", "torch"])
    assert "gru" not in seen
    cli.main(["train", "rec.f32", "out", "--gru", "native"])
    assert seen["gru"] == "native" and seen["records"] == "rec.f32"
    with pytest.raises(SystemExit):
        cli.main(["train", "rec.f32", "out", "--gru", "fast"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        cli.main(["train", "--help"])
    assert "librnnoise_amd_gru.so" in capsys.readouterr().out
