"""librnnoise_amd_gru.so on the device (include/rnnoise_amd_gru.h, rnnoise_amd/gru_native.py): the two kernels against the header's
formulas in float64 and beside torch's own nn.GRU in float32; determinism, cuts, guard words, a poisoned row; and the switch in
FloatNet, fit and the command line.

THE BOUND.  X64 is gru_native.gru_sequence_ref (and its backward) in float64 on the CPU.  For every output X -- y, dgi, dh0, dW_hh,
db_hh -- with e_native = max |X - X64| and e_torch = max |X of nn.GRU in float32 on the device - X64|:

    e_native <= 4 max(e_torch, 2^-23 max |X64|)

nn.GRU does not show dgi, so torch's layer here has the identity as W_ih and no b_ih over inputs of 3H floats: then its gi is its
input and its input gradient is dgi, both exactly.  The largest ratio e_native / max(e_torch, floor) per output is printed; DESIGN.md
4.33 records the measured ones."""
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
OUTPUTS = ("y", "dgi", "dh0", "dW_hh", "db_hh")


def problem(N, T, H, with_h0, seed=0):
    """float32 inputs on the CPU: gi, w_hh, b_hh, h0 (or None), dy, dhT (or None, as h0)"""
    gen = torch.Generator().manual_seed(seed * 1000003 + N * 10007 + T * 101 + H)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    w = rnd(3 * H, H) * (1.0 / np.sqrt(H))
    return dict(gi=rnd(N, T, 3 * H), w=w, b=rnd(3 * H) * .3, h0=rnd(N, H).tanh() if with_h0 else None, dy=rnd(N, T, H),
                dhT=rnd(N, H) if with_h0 else None)


def reference64(p):
    from rnnoise_amd import gru_native as G
    d = {k: (None if v is None else v.double()) for k, v in p.items()}
    y, saved = G.gru_sequence_ref(d["gi"], d["w"], d["b"], d["h0"], return_saved=True)
    dgi, dW, db, dh0 = G.gru_sequence_ref_backward(d["dy"], y, saved, d["w"], d["h0"], d["dhT"])
    return dict(y=y, dgi=dgi, dh0=dh0, dW_hh=dW, db_hh=db)


def torch_gru32(p):
    """nn.GRU in float32 on the device with W_ih = I, b_ih = 0 over 3H inputs: gi in, dgi out"""
    N, T, H = p["dy"].shape
    gru = torch.nn.GRU(3 * H, H, batch_first=True).to(DEV)
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.eye(3 * H))
        gru.bias_ih_l0.zero_()
        gru.weight_hh_l0.copy_(p["w"])
        gru.bias_hh_l0.copy_(p["b"])
    x = p["gi"].to(DEV).requires_grad_(True)
    h0 = None if p["h0"] is None else p["h0"].to(DEV).requires_grad_(True)
    y, hT = gru(x, None if h0 is None else h0.unsqueeze(0))
    loss = (y * p["dy"].to(DEV)).sum()
    if p["dhT"] is not None:
        loss = loss + (hT[0] * p["dhT"].to(DEV)).sum()
    loss.backward()
    dh0 = h0.grad if h0 is not None else None
    return dict(y=y.detach(), dgi=x.grad, dh0=dh0, dW_hh=gru.weight_hh_l0.grad, db_hh=gru.bias_hh_l0.grad)


def native32(p, frame_major=False):
    """the two device calls on their own (dhT goes into the backward call as it is), and the wrapper's weight gradients"""
    from rnnoise_amd import gru_native as G
    N, T, H = p["dy"].shape
    dev = lambda v: None if v is None else v.to(DEV)
    gi, dy, w, b, h0, dhT = lay(p["gi"], frame_major), lay(p["dy"], frame_major), dev(p["w"]), dev(p["b"]), dev(p["h0"]), dev(p["dhT"])
    y_buf = lay(torch.zeros(N, T, H), frame_major)
    dgi_buf = lay(torch.zeros(N, T, 3 * H), frame_major)
    y, saved = G.sequence_forward(gi, w, b, h0, y=y_buf)
    dgi, dgh, dh0 = G.sequence_backward(dy, y, saved, w, h0, dhT, dgi=dgi_buf)
    assert y.data_ptr() == y_buf.data_ptr() and dgi.data_ptr() == dgi_buf.data_ptr()  # written where they lie
    dW, db = G.weight_grads(dgh, y, h0)
    return dict(y=y, dgi=dgi, dh0=dh0, dW_hh=dW, db_hh=db, saved=saved, dgh=dgh)


WORST = {}


@pytest.mark.parametrize("N", [1, 15, 16, 17, 67])
@pytest.mark.parametrize("H", [16, 48, 384])
def test_parity_with_float64_beside_torch(H, N):
    """T 1, 2, 3, 35: the step that reads h0 alone, both halves of the dh scratch, and a sequence; each with zero state in batch-first
    buffers and with given h0 and dhT in frame-major ones -- and once the other way round"""
    for T in (1, 2, 3, 35):
        for with_h0, frame_major in ((False, False), (True, True)) + (((True, False), (False, True)) if T == 3 else ()):
            p = problem(N, T, H, with_h0)
            want = reference64(p)
            got, other = native32(p, frame_major), torch_gru32(p)
            if not with_h0:
                want["dh0"] = None  # torch has none to show; the library's is checked in the cuts below
            r = ratios(got, other, want, OUTPUTS)
            for k, v in r.items():
                WORST[k] = max(WORST.get(k, 0.0), v)
                assert v <= 4.0, (k, v, H, N, T, with_h0, frame_major)
    print(f"H {H} N {N}: largest e_native / max(e_torch, floor) so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def test_autograd_function_gives_the_calls_numbers():
    """GruSequence.apply under torch's autograd: the bits of the two calls, dhT arriving through y[:, -1]"""
    from rnnoise_amd import gru_native as G
    N, T, H = 17, 5, 48
    p = problem(N, T, H, True, seed=2)
    gi, w, b, h0 = (p[k].to(DEV).requires_grad_(True) for k in ("gi", "w", "b", "h0"))
    y = G.GruSequence.apply(gi, w, b, h0)
    (y * p["dy"].to(DEV)).sum().backward()
    q = dict(p, dhT=None)
    raw = native32(q)
    for name, a, c in (("y", y, raw["y"]), ("dgi", gi.grad, raw["dgi"]), ("dW_hh", w.grad, raw["dW_hh"]), ("db_hh", b.grad, raw["db_hh"]),
                       ("dh0", h0.grad, raw["dh0"])):
        assert_bits_equal(u32(a), u32(c), name)
    # without a state, and without weight gradients
    gi2 = p["gi"].to(DEV).requires_grad_(True)
    y2 = G.GruSequence.apply(gi2, w.detach(), b.detach(), None)
    (y2 * p["dy"].to(DEV)).sum().backward()
    raw2 = native32(dict(q, h0=None))
    assert_bits_equal(u32(y2), u32(raw2["y"]), "y, no state")
    assert_bits_equal(u32(gi2.grad), u32(raw2["dgi"]), "dgi, no state")
    with pytest.raises(ValueError):
        G.GruSequence.apply(torch.zeros(2, 3, 72, device=DEV), torch.zeros(72, 24, device=DEV), torch.zeros(72, device=DEV), None)  # H 24


def test_two_runs_are_bit_identical():
    p = problem(67, 35, 384, True, seed=3)
    a, b = native32(p), native32(p)
    for k in OUTPUTS + ("saved", "dgh"):
        assert_bits_equal(u32(a[k]), u32(b[k]), k)


def test_cuts_give_the_bits_of_one_call():
    """T = 35 as 16 + 1 + 18: forward with the state carried, backward in reverse with dh0 carried into dhT"""
    from rnnoise_amd import gru_native as G
    N, T, H = 17, 35, 48
    p = problem(N, T, H, True, seed=4)
    whole = native32(p)
    gi, dy, w, b = p["gi"].to(DEV), p["dy"].to(DEV), p["w"].to(DEV), p["b"].to(DEV)
    y = torch.zeros(N, T, H, device=DEV)
    cuts, state, saved = ((0, 16), (16, 17), (17, 35)), p["h0"].to(DEV), []
    for lo, hi in cuts:
        _, s = G.sequence_forward(gi[:, lo:hi], w, b, state, y=y[:, lo:hi])
        saved.append(s)
        state = y[:, hi - 1]
    assert_bits_equal(u32(y), u32(whole["y"]), "y of the cuts")
    dgi, dgh, dh = torch.zeros(N, T, 3 * H, device=DEV), [None] * 3, p["dhT"].to(DEV)
    for k in (2, 1, 0):
        lo, hi = cuts[k]
        first = p["h0"].to(DEV) if lo == 0 else y[:, lo - 1]
        _, dgh[k], dh = G.sequence_backward(dy[:, lo:hi], y[:, lo:hi], saved[k], w, first, dh, dgi=dgi[:, lo:hi])
    assert_bits_equal(u32(dgi), u32(whole["dgi"]), "dgi of the cuts")
    assert_bits_equal(u32(torch.cat(dgh)), u32(whole["dgh"]), "dgh of the cuts")
    assert_bits_equal(u32(dh), u32(whole["dh0"]), "dh0 of the cuts")
    # an empty cut: nothing launched, the state and the gradient pass through
    y0, _ = G.sequence_forward(gi[:, :0], w, b, state)
    assert y0.shape == (N, 0, H)
    _, _, dh_same = G.sequence_backward(dy[:, :0], y[:, :0], torch.zeros(4, device=DEV), w, None, dh)
    assert torch.equal(dh_same, dh)


@pytest.mark.parametrize("N,T,H", [(17, 3, 48), (5, 2, 16), (16, 4, 48)])
def test_guard_words_keep_their_fill(N, T, H):
    """padded strides in both orders, with room for the rows N .. 16 ceil(N / 16) - 1 that do not exist, and every dense buffer with
    a tail beyond its documented size: only the slots are written"""
    from rnnoise_amd import gru_native as G
    p = problem(N, T, H, True, seed=5)
    n_saved, n_scratch = G.workspace(N, T, H)
    tail, off = 16 * 4 * H * 2, 64
    w, b, h0, dhT = (p[k].to(DEV).contiguous() for k in ("w", "b", "h0", "dhT"))
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
        gi_buf, dy_buf = filled(gi_total), filled(y_total)
        view(gi_buf, gi_fs, gi_rs, 3 * H).copy_(p["gi"].to(DEV))
        view(dy_buf, y_fs, y_rs, H).copy_(p["dy"].to(DEV))
        y_buf, dgi_buf = filled(y_total), filled(gi_total)
        saved, dgh, dh0, scratch = filled(n_saved + tail), filled(T * N * 3 * H + tail), filled(N * H + tail), filled(n_scratch + tail)
        seq = G.make_seq((gi_buf.data_ptr() + 4 * off, gi_fs, gi_rs), w.data_ptr(), b.data_ptr(), (y_buf.data_ptr() + 4 * off, y_fs, y_rs),
                         N, T, H, h0.data_ptr())
        assert G.check(seq)
        stream = torch.cuda.current_stream(DEV).cuda_stream
        G.forward_device(seq, saved.data_ptr(), 0, stream)
        grad = G.make_grad((dy_buf.data_ptr() + 4 * off, y_fs, y_rs), (y_buf.data_ptr() + 4 * off, y_fs, y_rs), w.data_ptr(),
                           (dgi_buf.data_ptr() + 4 * off, gi_fs, gi_rs), dgh.data_ptr(), dh0.data_ptr(), N, T, H, h0.data_ptr(), dhT.data_ptr())
        assert G.check(grad)
        G.backward_device(grad, saved.data_ptr(), scratch.data_ptr(), 0, stream)
        torch.cuda.synchronize()
        want = native32(p)
        for name, buf, fs, rs, M in (("y", y_buf, y_fs, y_rs, H), ("dgi", dgi_buf, gi_fs, gi_rs, 3 * H)):
            words, mask = u32(buf), slot_mask(buf.numel(), off, fs, rs, T, N, M)
            assert np.all(words[~mask] == FILL), (name, order, int((words[~mask] != FILL).sum()))
            assert_bits_equal(u32(view(buf, fs, rs, M)), u32(want[name]), f"{name}, {order}")
        for name, buf, size in (("saved", saved, n_saved), ("dgh", dgh, T * N * 3 * H), ("dh0", dh0, N * H), ("scratch", scratch, n_scratch)):
            words = u32(buf)
            assert np.all(words[size:] == FILL), (name, order)
            if name != "scratch":
                assert_bits_equal(words[:size], u32(want[name]).reshape(-1)[:size], f"{name}, {order}")
        used = u32(scratch)[:n_scratch] != FILL  # T - 1 steps hand dh on through the scratch: one half each, alternating
        for half, steps in ((used[:N * H], 2), (used[N * H:], 3)):
            assert half.all() if T >= steps else not half.any(), (order, steps)
        # the inputs are read only
        assert np.all(u32(gi_buf)[~slot_mask(gi_buf.numel(), off, gi_fs, gi_rs, T, N, 3 * H)] == FILL)
        assert_bits_equal(u32(view(gi_buf, gi_fs, gi_rs, 3 * H)), u32(p["gi"]), "gi")


@pytest.mark.parametrize("N,row", [(17, 16), (16, 3)])
def test_a_poisoned_row_poisons_only_itself(N, row):
    T, H = 5, 48
    p = problem(N, T, H, True, seed=6)
    clean = native32(p)
    q = dict(p, gi=p["gi"].clone())
    q["gi"][row, 2, 7] = float("nan")
    bad = native32(q)
    others = [s for s in range(N) if s != row]
    for k in ("y", "dgi"):
        assert_bits_equal(u32(bad[k][others]), u32(clean[k][others]), k)
        assert torch.isnan(bad[k][row, 2:]).any() and not torch.isnan(bad[k][others]).any(), k
    assert_bits_equal(u32(bad["y"][row, :2]), u32(clean["y"][row, :2]), "the row before the poison")
    assert_bits_equal(u32(bad["dh0"][others]), u32(clean["dh0"][others]), "dh0")
    assert_bits_equal(u32(bad["dgh"][:, others]), u32(clean["dgh"][:, others]), "dgh")


# ---- the network ----
@pytest.mark.parametrize("cond,gru,N,T", [(16, 32, 4, 24), (128, 384, 3, 12)])
def test_float_net_native_beside_torch(cond, gru, N, T):
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
    net.gru_impl = "native"
    got = net_outputs(net, x.to(DEV), A.to(DEV), B.to(DEV))
    assert set(got) == set(want) and len(got) == 22
    r = ratios(got, other, want, names=sorted(want))
    print(f"FloatNet {cond}/{gru}: largest ratio {max(r.values()):.3f} ({max(r, key=r.get)})")
    for k, v in r.items():
        assert v <= 4.0, (k, v)
    # the streaming view runs the same layers: calls of uneven lengths carry the native states
    stream = {}
    for impl in ("torch", "native"):
        net.gru_impl = impl
        net.reset()
        with torch.no_grad():
            g = torch.cat([net(x[:, a:b].to(DEV))[0] for a, b in ((0, 3), (3, 9), (9, T))], dim=1)
        assert torch.all(g[:, :4] == 0)
        stream[impl] = dict(gains=g[:, 4:])
    assert ratios(stream["native"], stream["torch"], want, names=("gains",))["gains"] <= 4.0


def test_fit_native_beside_fit_torch(tmp_path):
    from rnnoise_amd import train
    records = R.training_records(np.random.default_rng(8), 4, 24)
    runs = {}
    for impl in ("torch", "native"):
        steps = []
        hist = train.fit(train.RecordFile(records, 24, 4), str(tmp_path / impl), epochs=3, cond_size=16, gru_size=32, seed=7, gru=impl,
                         on_step=lambda info: steps.append((info["loss"], info["gain_loss"], info["vad_loss"])), log=None)
        runs[impl] = (hist, steps)
    hist, steps = runs["native"]
    assert len(steps) == 3 and np.all(np.isfinite(steps)) and all(np.isfinite(h["loss"]) for h in hist)
    a, b = (torch.load(runs[k][0][-1]["checkpoint"], map_location="cpu") for k in ("native", "torch"))
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
        e_n, e_t = abs(runs["native"][1][0][k] - w), abs(runs["torch"][1][0][k] - w)
        print(f"first step, loss {k}: float64 {w:.12g}, native off by {e_n:.3e}, torch by {e_t:.3e}")
        assert e_n <= 4 * max(e_t, 1e-6 * abs(w)), (k, e_n, e_t, w)


def test_cli_train_native_then_export(tmp_path):
    records = R.training_records(np.random.default_rng(9), 2, 12)
    rec = tmp_path / "rec.f32"
    records.tofile(str(rec))
    out = tmp_path / "run"
    run = lambda *argv: subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", *argv], cwd=ROOT, capture_output=True, text=True, timeout=300)
    r = run("train", str(rec), str(out), "--gru", "native", "--epochs", "1", "--batch-size", "2", "--sequence-length", "12", "--seed", "5")
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    assert line.startswith("epoch 1: loss ") and "(1 batches, step 1)" in line and np.isfinite(float(line.split()[3]))
    ckpt = out / "checkpoints" / "rnnoise_1.pth"
    assert ckpt.exists()
    r = run("export", str(ckpt), str(tmp_path / "net.blob"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "net.blob").read_bytes()[:4] == b"DNNw"
