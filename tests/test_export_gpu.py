"""Checkpoint to blob on the GPU, on the seeded state dict of tests/export_cases.py pruned to .3 / .2 / .5:

  a  the exported blob loads and runs a short process call, bit-identical to the oracle on that blob
  b  the float network on the GPU against itself on the CPU, inside 4 E (tests/test_float_net_cpu.py: E is the distance of a float32
     evaluation from the float64 one; here measured on this state dict the same way, and on the default checkpoint against the golden
     outputs where the oracle recipe has left it)
  c  evaluate_checkpoint against the float64 restatement of the loss (tests/eval_cases.py) over forward_sequence's own outputs,
     relative difference at most 1e-10, over two slabs and several groups; the blob's band means through evaluate_records(bands=True)
  d  cli export, cli eval-records --checkpoint and cli denoise --checkpoint on 3 streams x 12 frames: the JSON carries the deltas and
     the 32 band means"""
import copy
import json
import os

import numpy as np
import pytest

import eval_cases as ec
import export_cases as xc
from conftest import GOLD, ROOT, assert_bits_equal
from rnnoise_amd import capi, cli, evaluate, export, float_net, synth

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T = ec.T


@pytest.fixture(scope="module")
def seeded_net():
    sd, _ = xc.pruned_blob()
    net = float_net.FloatNet()
    net.load_state_dict(sd)
    return net.eval()


@pytest.fixture(scope="module")
def ckpt_file(tmp_path_factory):
    sd, _ = xc.pruned_blob()
    path = tmp_path_factory.mktemp("ckpt") / "seeded.pth"
    torch.save({"model_args": (), "model_kwargs": {"cond_size": 128, "gru_size": 384}, "state_dict": dict(sd)}, path)
    return str(path)


# ---- a. the blob runs ----
def test_exported_blob_runs_bit_identical_to_the_oracle():
    from oracle.binding import Oracle
    _, data = xc.pruned_blob()
    streams = [3, 77, 130]
    pcm = synth.batch_pcm(streams, T, lead_silence=2)
    model = capi.Model(data)
    b = capi.Batch(model, len(streams))
    out, vad, gains = b.process(pcm)
    b.close(), model.close()
    assert gains.std() > 0.01   # (the network says something)
    for i in range(len(streams)):
        want = Oracle(data).run(pcm[:, i])
        assert_bits_equal(out[:, i], want["out"], f"pcm of stream {streams[i]}")
        assert_bits_equal(vad[:, i], want["vad"], f"vad of stream {streams[i]}")
        assert_bits_equal(gains[:, i], want["gains"], f"gains of stream {streams[i]}")


# ---- b. the float network on the GPU ----
def gpu_against_cpu(net, feats, E):
    dev = torch.device("cuda", 0)
    on = copy.deepcopy(net).to(dev)
    with torch.no_grad():
        g, v = net.forward_sequence(feats)
        gg, gv = on.forward_sequence(feats.to(dev))
        on.reset()
        parts = [on(feats[:, a:b].to(dev)) for a, b in ((0, 1), (1, 6), (6, 7), (7, 15), (15, feats.shape[1]))]
    sg, sv = torch.cat([p[0] for p in parts], 1).cpu(), torch.cat([p[1] for p in parts], 1).cpu()
    d = (float((gg.cpu() - g).abs().max()), float((gv.cpu() - v).abs().max()),
         float((sg[:, 4:] - g).abs().max()), float((sv[:, 4:] - v).abs().max()))
    print(f"\n[float-net] GPU against CPU: sequence gains {d[0]:.3e}, vad {d[1]:.3e}; streaming in cuts at offset 4: {d[2]:.3e}, {d[3]:.3e}; "
          f"E = {E:.3e}, bound {4 * E:.3e}")
    assert float(sg[:, :4].abs().max()) == 0
    assert max(d) <= 4 * E, d


def test_float_network_on_the_gpu_seeded(seeded_net):
    feats = torch.from_numpy(np.load(os.path.join(GOLD, "torch_float_default.npz"))["features"])[None]
    with torch.no_grad():
        g32, v32 = seeded_net.forward_sequence(feats)
        g64, v64 = copy.deepcopy(seeded_net).double().forward_sequence(feats.double())
    E = max(float((g64 - g32).abs().max()), float((v64 - v32).abs().max()))
    assert 0 < E < 1e-5
    gpu_against_cpu(seeded_net, feats, E)


def test_float_network_on_the_gpu_default_checkpoint():
    path = os.path.join(ROOT, "oracle", "_ref", "gen_default", "synth.pth")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref/gen_default/synth.pth: the oracle recipe has not run here")
    gold = np.load(os.path.join(GOLD, "torch_float_default.npz"))
    net = float_net.load_checkpoint(path)
    feats = torch.from_numpy(gold["features"])[None]
    with torch.no_grad():
        g64, v64 = copy.deepcopy(net).double().forward_sequence(feats.double())
    E = max(float(np.abs(g64[0].numpy() - gold["gains"]).max()), float(np.abs(v64[0, :, 0].numpy() - gold["vad"]).max()))
    gpu_against_cpu(net, feats, E)


# ---- c. evaluate_checkpoint ----
class Recording(torch.nn.Module):
    """the float network, keeping what forward_sequence returned: the predictions that were scored"""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []
        self.cond_size, self.gru_size = net.cond_size, net.gru_size

    def forward_sequence(self, features):
        g, v = self.net.forward_sequence(features)
        self.seen.append((g.detach().cpu().numpy().copy(), v.detach().cpu().numpy().copy()))
        return g, v


def test_evaluate_checkpoint_against_the_float64_restatement(seeded_net):
    rec = ec.records()                                            # (T, D, 98)
    D = rec.shape[1]
    seqs = np.ascontiguousarray(rec.transpose(1, 0, 2))           # the file's order: [sequence][frame][98]
    net = Recording(copy.deepcopy(seeded_net))
    width = capi.FEATURES + 2 * 128 + 10 * 384
    res = evaluate.evaluate_checkpoint(seqs, net, sequence_length=T, max_streams=64, group_bytes=25 * T * width * 4)
    assert [g.shape[0] for g, _ in net.seen] == [25, 25, 14, 25, 14]  # slabs of 64 and 39 sequences in groups of 25
    g = np.concatenate([a for a, _ in net.seen])                  # (D, T - 4, 32): output k is step k + 4
    v = np.concatenate([a for _, a in net.seen])[:, :, 0]
    gains, vad = np.zeros((T, D, 32), np.float32), np.zeros((T, D), np.float32)
    gains[4:], vad[4:] = g.transpose(1, 0, 2), v.T
    exp = ec.expected_sums(rec, gains, vad)
    want = capi.eval_losses(exp)
    print(f"\n[evaluate-checkpoint] loss {res['loss']:.6f} (gain {res['gain_loss']:.6f}, vad {res['vad_loss']:.6f}), "
          f"relative difference to float64 numpy: {ec.rel_diff(res['loss'], want['loss']):.3e}")
    assert res["sequences"] == D and res["frames_scored"] == D * (T - 4) == want["frames_scored"]
    for k in ("gain_loss", "vad_loss", "loss"):
        assert ec.rel_diff(res[k], want[k]) <= 1e-10, (k, res[k], want[k])
    per = res["per_sequence"]
    assert ec.rel_diff(per["gain_loss"], exp[:, 0] / (32 * exp[:, 2])) <= 1e-10 and ec.rel_diff(per["vad_loss"], exp[:, 1] / exp[:, 2]) <= 1e-10
    bands = np.zeros((D, 32))
    for t in range(4, T):
        bands += ec.loss_terms(rec[t - 1][:, ec.TARGETS], rec[t - 1][:, ec.VAD], gains[t], vad[t])[0]
    assert len(res["band_gain_loss"]) == 32 and ec.rel_diff(res["band_gain_loss"], bands.sum(0) / exp[:, 2].sum()) <= 1e-10
    assert ec.rel_diff(np.mean(res["band_gain_loss"]), res["gain_loss"]) <= 1e-12
    # first below 4 scores from step 4 all the same; a later first scores fewer
    assert evaluate.evaluate_checkpoint(seqs[:5], net, sequence_length=T, first=0)["frames_scored"] == 5 * (T - 4)
    assert evaluate.evaluate_checkpoint(seqs[:5], net, sequence_length=T, first=9)["frames_scored"] == 5 * (T - 9)


def test_evaluate_records_with_bands_gives_the_sums_of_one_call():
    """bands=True walks the file in segments and scores eval_records' outputs once more: the same three means as the plain walk, to the
    bit, and 32 band means whose mean is the gain loss"""
    _, data = xc.pruned_blob()
    seqs = np.ascontiguousarray(ec.records().transpose(1, 0, 2))[:70]
    plain = evaluate.evaluate_records(seqs, [data], sequence_length=T)[0]
    seg = evaluate.evaluate_records(seqs, [data], sequence_length=T, bands=True, segment_bytes=70 * 33 * 4 * 5)[0]   # segments of 5 frames
    assert "band_gain_loss" not in plain and len(seg["band_gain_loss"]) == 32
    for k in ("gain_loss", "vad_loss", "loss", "frames_scored"):
        assert plain[k] == seg[k], k
    assert ec.rel_diff(np.mean(seg["band_gain_loss"]), seg["gain_loss"]) <= 1e-12


# ---- d. the command line ----
def test_cli_export_eval_records_and_denoise_with_a_checkpoint(ckpt_file, tmp_path, capsys):
    blob_path, out_dir = str(tmp_path / "out.blob"), str(tmp_path / "out")
    cli.main(["export", ckpt_file, blob_path])
    assert open(blob_path, "rb").read() == xc.pruned_blob()[1]
    rec_path = str(tmp_path / "val.f32")
    np.ascontiguousarray(ec.records().transpose(1, 0, 2))[[0, 50, 100]].tofile(rec_path)
    capsys.readouterr()
    cli.main(["eval-records", rec_path, "--model", blob_path, "--checkpoint", ckpt_file, "--sequence-length", str(T)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    ck, (m,) = line["checkpoint"], line["models"]
    assert ck["sequences"] == m["sequences"] == 3 and ck["frames_scored"] == m["frames_scored"] == 3 * (T - 4)
    assert len(ck["band_gain_loss"]) == len(m["band_gain_loss"]) == len(m["band_delta_to_checkpoint"]) == 32
    for k in ("gain_loss", "vad_loss", "loss"):
        assert m["delta_to_checkpoint"][k] == m[k] - ck[k] and np.isfinite(m[k]) and np.isfinite(ck[k])
    print(f"\n[cli eval-records] checkpoint loss {ck['loss']:.6f}, blob loss {m['loss']:.6f}, delta {m['delta_to_checkpoint']['loss']:+.3e}")
    assert m["delta_to_checkpoint"]["loss"] != 0   # (int8 against float, and a causal start against the trainer's: they differ)
    # denoise: the float network between the split calls, the DSP's batch on the blob the checkpoint exports to
    streams = [3, 77, 130]
    pcm = synth.batch_pcm(streams, T, lead_silence=1)
    files = []
    for i, s in enumerate(streams):
        files.append(str(tmp_path / f"s{s}.raw"))
        pcm[:, i].astype(np.int16).tofile(files[-1])
    cli.main(["denoise", "--checkpoint", ckpt_file, "--out-dir", out_dir] + files)
    cli.main(["denoise", "--checkpoint", ckpt_file, "--model", blob_path, "--out-dir", out_dir + "2"] + files)
    for f in files:
        a = np.fromfile(os.path.join(out_dir, os.path.basename(f) + ".denoised.raw"), np.int16)
        b = np.fromfile(os.path.join(out_dir + "2", os.path.basename(f) + ".denoised.raw"), np.int16)
        # (two runs of one float32 network on the GPU may round differently -- the library picks its GEMMs per process --, so the
        # samples, truncated to int16 behind gains that differ in the 7th digit, may differ by one step)
        assert a.size == (T - 1) * 480 and b.size == a.size and np.abs(a.astype(np.int32) - b).max() <= 1
        assert (a[:3 * 480] == 0).all() and np.abs(a[4 * 480:].astype(np.int32)).max() > 0   # the float network's first four frames: no output
    with pytest.raises(ValueError, match="max-store-gb"):
        cli.main(["denoise", "--checkpoint", ckpt_file, "--out-dir", out_dir, "--max-store-gb", "1e-9"] + files)
