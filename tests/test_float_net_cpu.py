"""rnnoise_amd.float_net on the CPU: the float network in this project's words against the reference's outputs.

tests/golden/torch_float_default.npz holds the reference module's float32 outputs (gains, vad) on `features`, for the checkpoint
oracle/_ref/gen_default/synth.pth; the tests that need the checkpoint run where the oracle recipe left it, and skip elsewhere.

TOLERANCE.  E = the largest absolute difference between the golden float32 outputs and this module evaluated in float64 on the CPU;
every float32 comparison is bounded at 4 E: two float32 evaluations of one network in different summation orders can each be E from
the exact result (2 E), doubled for the GEMM blocking that changes with T.  Measured: E = 8.44e-07 (gains; vad 2.6e-07), so 4 E =
3.4e-06; own float32 against golden 0, streaming against sequence at offset 4: 0, cuts 1 / 5 / 1 / 8 against one call 6.6e-07."""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT

torch = pytest.importorskip("torch")
CKPT = os.path.join(ROOT, "oracle", "_ref", "gen_default", "synth.pth")
REF = os.environ.get("RNNOISE_REFERENCE", "/root/reference")
needs_ckpt = pytest.mark.skipif(not os.path.exists(CKPT), reason="oracle/_ref/gen_default/synth.pth: the oracle recipe has not run here")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "torch_float_default.npz"))


@pytest.fixture(scope="module")
def net():
    from rnnoise_amd import float_net
    return float_net.load_checkpoint(CKPT)


@pytest.fixture(scope="module")
def bound(net, gold):
    """4 E"""
    n64 = copy.deepcopy(net).double()
    with torch.no_grad():
        g, v = n64.forward_sequence(torch.from_numpy(gold["features"]).double()[None])
    E = max(float(np.abs(g[0].numpy() - gold["gains"]).max()), float(np.abs(v[0, :, 0].numpy() - gold["vad"]).max()))
    print(f"\n[float-net] E = {E:.3e} (float64 on the CPU against the golden float32 outputs); bound 4 E = {4 * E:.3e}")
    assert 0 < E < 1e-5   # (float32 rounding of a network of this depth; anything larger is not rounding)
    return 4 * E


def worst(a, b):
    return float((a - b).abs().max())


@needs_ckpt
def test_sequence_forward_against_the_golden_outputs(net, gold, bound):
    f = torch.from_numpy(gold["features"])[None]
    with torch.no_grad():
        g, v = net.forward_sequence(f)
    assert g.shape == (1, 116, 32) and v.shape == (1, 116, 1)
    dg, dv = np.abs(g[0].numpy() - gold["gains"]).max(), np.abs(v[0, :, 0].numpy() - gold["vad"]).max()
    print(f"[float-net] own float32 against golden: gains {dg:.3e}, vad {dv:.3e}")
    assert dg <= bound and dv <= bound


@needs_ckpt
def test_streaming_is_the_sequence_at_offset_four_in_any_cut(net, gold, bound):
    f = torch.from_numpy(gold["features"])[None].repeat(3, 1, 1)
    f[1] = f[1].flip(0)   # (three streams, two distinct)
    with torch.no_grad():
        gs, vs = net.forward_sequence(f)
        net.reset()
        g1, v1 = net(f)
        assert g1.shape == (3, 120, 32) and v1.shape == (3, 120, 1)
        assert float(g1[:, :4].abs().max()) == 0 and float(v1[:, :4].abs().max()) == 0   # no output in the trainer's view: zeros
        d = (worst(g1[:, 4:], gs), worst(v1[:, 4:], vs))
        # without a reset the module goes on with the same streams: another sequence behind the first is not the first again
        g2, _ = net(f)
        assert worst(g2[:, 4:], gs) > 100 * bound
        net.reset()
        outs, t, cuts = [], 0, (1, 5, 1, 8)
        while t < 120:
            for k in cuts:
                if t < 120:
                    outs.append(net(f[:, t:t + k]))
                    t += k
        gc, vc = torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1)
        e = (worst(gc, g1), worst(vc, v1))
        net.reset()
    print(f"[float-net] streaming against sequence at offset 4: gains {d[0]:.3e}, vad {d[1]:.3e}; cuts against one call: {e[0]:.3e}, {e[1]:.3e}")
    assert max(d) <= bound and max(e) <= bound and gc.shape == g1.shape


@needs_ckpt
def test_given_states_continue_a_sequence(net, gold, bound):
    """forward_sequence on frames 0 .. 63, then on frames 60 .. 119 from the states it returned: the second half of one call"""
    f = torch.from_numpy(gold["features"])[None]
    with torch.no_grad():
        g, v = net.forward_sequence(f)
        ga, va, st = net.forward_sequence(f[:, :64], return_states=True)
        gb, vb = net.forward_sequence(f[:, 60:], states=st)
    assert worst(torch.cat([ga, gb], 1), g) <= bound and worst(torch.cat([va, vb], 1), v) <= bound


@needs_ckpt
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "torch", "rnnoise")), reason="the reference tree is not mounted")
def test_own_module_against_the_reference_module_live(net, gold, bound):
    """both modules on the CPU in one process, the same checkpoint, the same features; the parameter names are the trainer's:
    load_state_dict is strict on both sides"""
    sys.path.insert(0, os.path.join(REF, "torch", "rnnoise"))
    try:
        import rnnoise as ref_rnnoise
    finally:
        sys.path.pop(0)
    ck = torch.load(CKPT, map_location="cpu")
    ref = ref_rnnoise.RNNoise(*ck["model_args"], **ck["model_kwargs"])
    ref.load_state_dict(ck["state_dict"])
    ref.eval()
    assert set(net.state_dict()) == set(ck["state_dict"])
    f = torch.from_numpy(gold["features"])[None].repeat(2, 1, 1)
    f[1] = f[1].flip(0)
    with torch.no_grad():
        rg, rv, _ = ref(f)
        g, v = net.forward_sequence(f)
    assert np.abs(rg[0].numpy() - gold["gains"]).max() <= bound   # (the golden file is this module's output)
    assert worst(g, rg) <= bound and worst(v, rv) <= bound


def test_parameter_names_and_shapes_are_the_trainers():
    from rnnoise_amd import export, float_net
    n = float_net.FloatNet()
    assert {k: tuple(v.shape) for k, v in n.state_dict().items()} == dict(export.SHAPES)
    small = float_net.FloatNet(cond_size=32, gru_size=48)
    with torch.no_grad():
        g, v = small.forward_sequence(torch.zeros(2, 9, 65))
        gs, vs = small(torch.zeros(2, 9, 65))
    assert g.shape == (2, 5, 32) and v.shape == (2, 5, 1) and gs.shape == (2, 9, 32) and vs.shape == (2, 9, 1)
    assert worst(gs[:, 4:], g) == 0 and float(gs[:, :4].abs().max()) == 0
