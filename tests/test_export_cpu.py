"""rnnoise_amd.export on the CPU: checkpoint to blob.

  a  where the oracle recipe has left oracle/_ref/gen_<name>/synth.pth and oracle/_ref/<name>.blob (skipped elsewhere):
     blob_from_state_dict of default, little and dense equals the reference exporter's and writer's blob BYTE FOR BYTE; default's also
     equals tests/golden/default.blob.xz unpacked
  b  without the reference: a state dict drawn from a numpy seed (tests/export_cases.py), pruned to .3 / .2 / .5, exports to a blob
     with the 43 records in order that the library packs, whose kept blocks sit where prune_state_dict left weights
  c  refusals: other dimensions, weight-norm keys, missing and surplus tensors, non-finite weights -- each names the split calls;
     the exporter's own "value out of bounds" stays an error
  d  synth_model's bytes are what they were before _linear_int8 learnt the exporter's order of scale and diagonal
  e  where the reference tree is mounted (skipped elsewhere): prune_state_dict of the dense ancestors of synth.pth, drawn as
     oracle/gen_model.py draws them, gives synth.pth's tensors -- the masks of the reference's sparsify_matrix -- bit for bit
  f  the command line
"""
import hashlib
import lzma
import os
import subprocess
import sys

import numpy as np
import pytest

import export_cases as xc
from conftest import GOLD, ROOT
from rnnoise_amd import blob, capi, export

REF = os.environ.get("RNNOISE_REFERENCE", "/root/reference")
ORACLE = os.path.join(ROOT, "oracle", "_ref")
VARIANTS = {"default": (0.3, 0.2, 0.5, 1234), "little": (0.15, 0.1, 0.25, 4321), "dense": (1.0, 1.0, 1.0, 777)}  # (oracle/gen_model.py)
ORDER = [n for layer, kind in (("conv1", "f"), ("conv2", "q"), ("gru1_input", "s"), ("gru1_recurrent", "d"), ("gru2_input", "s"),
                              ("gru2_recurrent", "d"), ("gru3_input", "s"), ("gru3_recurrent", "d"), ("dense_out", "f"), ("vad_dense", "f"))
         for n in ([layer + "_weights_float", layer + "_bias"] if kind == "f" else
                   ([layer + "_weights_diag"] if kind == "d" else []) + [layer + "_weights_int8"] +
                   ([layer + "_weights_idx"] if kind in "sd" else []) + [layer + s for s in ("_subias", "_scale", "_bias")])]


def have(name):
    return os.path.exists(os.path.join(ORACLE, f"gen_{name}", "synth.pth")) and os.path.exists(os.path.join(ORACLE, name + ".blob"))


# ---- a. byte for byte ----
@pytest.mark.parametrize("name", list(VARIANTS))
def test_blob_is_the_reference_exporters_byte_for_byte(name):
    if not have(name):
        pytest.skip(f"oracle/_ref/gen_{name}/synth.pth and oracle/_ref/{name}.blob: the oracle recipe has not run here")
    got = export.blob_from_state_dict(export.load_state_dict_file(os.path.join(ORACLE, f"gen_{name}", "synth.pth")))
    want = open(os.path.join(ORACLE, name + ".blob"), "rb").read()
    if got != want:
        a, b = blob.read_blob(got), blob.read_blob(want)
        assert list(a) == list(b)
        assert [k for k in a if a[k].shape != b[k].shape or (a[k] != b[k]).any()] == []
    assert got == want
    if name == "default":
        assert got == lzma.decompress(open(os.path.join(GOLD, "default.blob.xz"), "rb").read())


# ---- b. a seeded state dict, no reference ----
def test_seeded_pruned_state_dict_exports_to_a_blob_the_library_packs():
    sd, data = xc.pruned_blob()
    rec = blob.read_blob(data)
    assert len(ORDER) == 43 and list(rec) == ORDER
    m = capi.Model(data)   # rnnoise_amd_model_pack accepts it
    pack = m.pack()
    m.close()
    head = blob.read_pack_header(pack)
    dense = export.check_state_dict(xc.state_dict())
    for k in (1, 2, 3):
        for side, layer in (("ih", "input"), ("hh", "recurrent")):
            name = f"gru{k}_{layer}"
            W = export._zrn(sd[f"gru{k}.weight_{side}_l0"].numpy()).T.copy()    # [in][out], gates z, r, n
            if side == "hh":
                for g in range(3):
                    W[np.arange(384), g * 384 + np.arange(384)] = 0
            idx, q = rec[name + "_weights_idx"], rec[name + "_weights_int8"].reshape(-1, 8, 4)
            kept = np.abs(W).reshape(96, 4, 144, 8).sum(axis=(1, 3)) > 1e-10    # [in / 4][out / 8]
            pos = blk = 0
            for i in range(144):
                n = idx[pos]
                cols = idx[pos + 1:pos + 1 + n]
                assert (cols % 4 == 0).all() and (cols >= 0).all() and (cols < 384).all() and (np.diff(cols) > 0).all(), (name, i)
                assert (cols // 4 == np.flatnonzero(kept[:, i])).all(), (name, i)
                pos, blk = pos + 1 + n, blk + n
            assert pos == idx.size and blk == q.shape[0] == kept.sum()
            layer_head = next(l for l in head["layers"] if l["name"] == name)
            assert layer_head["nblocks"] == blk and layer_head["has_diag"] == (side == "hh")
            # the densities: r .3, z .2, n .5 of 96 x 48 blocks per gate on the torch layout -> blob gates z, r, n
            per_gate = [int(kept[:, g * 48:(g + 1) * 48].sum()) for g in range(3)]
            want = [round(96 * 48 * d) for d in (0.2, 0.3, 0.5)]
            assert all(w <= p <= w + 8 for p, w in zip(per_gate, want)), (name, per_gate, want)   # (ties at the threshold survive)
            if side == "hh":   # the diagonal is spared, in float, in the blob's gate order
                d = export._zrn(dense[f"gru{k}.weight_hh_l0"])
                assert (rec[name + "_weights_diag"] == np.concatenate([np.diag(d[g * 384:(g + 1) * 384]) for g in range(3)])).all()
    # what is not pruned is not touched
    for key in ("conv1.weight", "conv2.bias", "gru2.bias_hh_l0", "dense_out.weight"):
        assert (sd[key].numpy() == dense[key]).all()
    assert (rec["conv1_weights_float"] == np.transpose(dense["conv1.weight"], (2, 1, 0)).reshape(-1)).all()
    assert (rec["dense_out_weights_float"] == dense["dense_out.weight"].T.reshape(-1)).all()
    assert "density" in blob.describe(data)


def test_prune_keeps_the_largest_blocks_and_is_idempotent():
    import torch
    sd = xc.state_dict()
    once = export.prune_state_dict(sd, xc.DENSITIES)
    twice = export.prune_state_dict(once, xc.DENSITIES)
    for k in once:
        assert torch.equal(once[k], twice[k]), k
    W, P = sd["gru1.weight_ih_l0"][:384], once["gru1.weight_ih_l0"][:384].numpy()       # the reset gate, density .3
    e = (W.astype(np.float64) ** 2).reshape(48, 8, 96, 4).sum(axis=(1, 3))
    kept = np.abs(P).reshape(48, 8, 96, 4).sum(axis=(1, 3)) > 0
    assert kept.sum() == round(48 * 96 * 0.3) and e[kept].min() > e[~kept].max()
    assert (P[np.repeat(np.repeat(kept, 8, 0), 4, 1)] == W[np.repeat(np.repeat(kept, 8, 0), 4, 1)]).all()
    full = export.prune_state_dict(sd, (1.0, 1.0, 1.0))
    assert all((full[k].numpy() == sd[k]).all() for k in sd)
    with pytest.raises(ValueError):
        export.prune_state_dict(sd, (0.3, 0.2))
    with pytest.raises(ValueError):
        export.prune_state_dict(sd, (0.3, 0.2, 1.5))


# ---- c. refusals ----
def test_refusals_name_the_split_calls():
    sd = xc.state_dict()

    def refused(change, word):
        bad = dict(sd)
        change(bad)
        with pytest.raises(ValueError) as e:
            export.blob_from_state_dict(bad)
        assert word in str(e.value) and "split calls" in str(e.value) and "rnnoise_batch_analyze" in str(e.value), str(e.value)

    refused(lambda d: d.update({"conv1.weight": np.zeros((256, 65, 3), np.float32), "conv1.bias": np.zeros(256, np.float32)}), "cond_size")
    refused(lambda d: d.update({"gru1.weight_hh_l0": np.zeros((768, 256), np.float32)}), "gru_size")
    refused(lambda d: (d.update({"conv1.weight_g": np.ones((128, 1, 1), np.float32), "conv1.weight_v": d["conv1.weight"]}),
                       d.pop("conv1.weight")), "weight-norm")
    refused(lambda d: d.pop("gru3.bias_ih_l0"), "lacks")
    refused(lambda d: d.update({"gru4.weight_ih_l0": np.zeros((1152, 384), np.float32)}), "no place")
    for value in (np.nan, np.inf):
        w = sd["gru2.weight_ih_l0"].copy()
        w[5, 7] = value
        refused(lambda d: d.update({"gru2.weight_ih_l0": w}), "not finite")
    # the exporter's own error stays one
    with pytest.raises(ValueError, match="out of bounds"):
        blob._quantize(np.array([[200.0]]), np.array([1.0]))


# ---- d. synth_model is what it was ----
# sha256 of blob.synth_model(seed, density, boost) from the parent commit's function (taken before _linear_int8 gained its parameter)
SYNTH_DIGESTS = {(1, 1 / 3, 3.0): "ac7f255ef0adb8fdc49f67632903cb291f5b3c0631d94bfc0eb590d01764ea2c",
                 (7, 0.2, 2.0): "911c8555205aac1ce415983d5d490e85177fb6113b5fbb0d5b093dffddd7cdae",
                 (3, 1.0, 3.0): "839bf4731d2a4b24aaccb66e90e8996d79778d094366be2aa9a45adfe0cc2c4f"}


@pytest.mark.parametrize("args", list(SYNTH_DIGESTS))
def test_synth_model_bytes_are_unchanged(args):
    assert hashlib.sha256(blob.synth_model(*args)).hexdigest() == SYNTH_DIGESTS[args]


def test_scale_before_the_diagonal_is_what_differs():
    """the one step the exporter takes in another order than synth_model: only the recurrent int8 weights, subias and scale move"""
    from collections import OrderedDict
    sd = export.check_state_dict(xc.state_dict())
    w, b = export._zrn(sd["gru1.weight_hh_l0"]).T, export._zrn(sd["gru1.bias_hh_l0"])
    w = w.copy()
    w[3, 3] = 40 * np.abs(w).max()   # a diagonal entry that dominates its column's scale
    a, c = OrderedDict(), OrderedDict()
    blob._linear_int8(a, "x", w, b, sparse=True, diagonal=True)
    blob._linear_int8(c, "x", w, b, sparse=True, diagonal=True, scale_with_diagonal=True)
    assert list(a) == list(c)
    moved = {k for k in a if a[k].shape != c[k].shape or (a[k] != c[k]).any()}
    assert "x_scale" in moved and moved <= {"x_weights_int8", "x_subias", "x_scale"}
    assert c["x_scale"][3] > 10 * a["x_scale"][3] and (np.delete(c["x_scale"], 3) >= np.delete(a["x_scale"], 3)).all()


# ---- e. the reference's masks, live ----
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "torch", "rnnoise")), reason="the reference tree is not mounted")
@pytest.mark.parametrize("name", ["default", "little"])
def test_prune_gives_the_reference_sparsifiers_masks(name):
    if not have(name):
        pytest.skip("the oracle recipe has not run here")
    import torch
    sys.path.insert(0, os.path.join(REF, "torch", "rnnoise"))
    try:
        import rnnoise as ref_rnnoise
    finally:
        sys.path.pop(0)
    sys.path.insert(0, os.path.join(REF, "torch"))
    try:
        from sparsification.common import sparsify_matrix
    finally:
        sys.path.pop(0)
    dr, dz, dn, seed = VARIANTS[name]
    torch.manual_seed(seed)   # the dense ancestor, drawn as oracle/gen_model.py draws it (boost 3)
    model = ref_rnnoise.RNNoise(cond_size=128, gru_size=384)
    with torch.no_grad():
        model.conv1.weight.mul_(3.0)
        model.conv2.weight.mul_(3.0)
        for gru in (model.gru1, model.gru2, model.gru3):
            gru.weight_ih_l0.mul_(3.0)
            gru.bias_ih_l0.mul_(3.0)
        model.dense_out.weight.mul_(6.0)
        model.dense_out.bias.uniform_(-1.0, 1.0)
        model.vad_dense.weight.mul_(6.0)
    ancestor = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pruned = export.prune_state_dict(ancestor, (dr, dz, dn))
    want = export.load_state_dict_file(os.path.join(ORACLE, f"gen_{name}", "synth.pth"))
    assert set(pruned) == set(want)
    for k in want:
        assert torch.equal(pruned[k], want[k]), k
    # and one matrix against sparsify_matrix itself, mask for mask
    W = ancestor["gru2.weight_hh_l0"][384:768]
    ref_w, ref_mask = sparsify_matrix(W, dz, [8, 4], True, return_mask=True)
    got = pruned["gru2.weight_hh_l0"][384:768]
    assert torch.equal(got, ref_w)
    off = ~torch.eye(384, dtype=torch.bool)
    assert torch.equal((got != 0) & off, (ref_mask != 0) & off & (W != 0))


# ---- f. the command line ----
def test_cli_export_and_blob_info(tmp_path):
    import torch
    ck = tmp_path / "ckpt.pth"
    torch.save({"model_args": (), "model_kwargs": {"cond_size": 128, "gru_size": 384},
                "state_dict": {k: torch.from_numpy(v) for k, v in xc.state_dict().items()}}, ck)
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], cwd=ROOT, capture_output=True, text=True)
    r = run("rnnoise_amd.cli", "export", "--densities", ".3,.2,.5", str(ck), str(tmp_path / "out.blob"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.blob").read_bytes() == xc.pruned_blob()[1]
    r = run("rnnoise_amd.cli", "export", "--densities", ".3,.2,.5", "--pack", str(ck), str(tmp_path / "out.rnpk"))
    assert r.returncode == 0 and (tmp_path / "out.rnpk").read_bytes()[:4] == b"RNPK", r.stderr
    for f, word in (("out.blob", "43 records"), ("out.rnpk", "RNPK version")):
        r = run("rnnoise_amd.blob", "info", str(tmp_path / f))
        assert r.returncode == 0 and word in r.stdout, (r.stdout, r.stderr)
    torch.save({"model_kwargs": {"cond_size": 256, "gru_size": 384}, "state_dict": {}}, ck)
    r = run("rnnoise_amd.cli", "export", str(ck), str(tmp_path / "no.blob"))
    assert r.returncode != 0 and "split calls" in r.stderr and not (tmp_path / "no.blob").exists()
    h = run("rnnoise_amd.cli", "export", "--help").stdout
    assert "--densities" in h and "--pack" in h
    assert "--checkpoint" in run("rnnoise_amd.cli", "eval-records", "--help").stdout
    assert "--checkpoint" in run("rnnoise_amd.cli", "denoise", "--help").stdout
