"""Checkpoint to blob: what the reference makes of a trainer checkpoint in three steps --
torch/rnnoise/dump_rnnoise_weights.py --quantize, the generated C file, src/write_weights.c -DDISABLE_DEBUG_FLOAT -- restated as one
host function on numpy arrays, byte for byte.  torch is needed only to read a .pth file.

  blob_from_state_dict(sd)             the "DNNw" blob of a state dict of the trainer's model (cond_size 128, gru_size 384)
  prune_state_dict(sd, densities)      the trainer's block sparsification in one shot: a sparser variant of a checkpoint
  load_state_dict_file(path)           the state dict of a trainer checkpoint (a .pth with 'state_dict', or a bare state dict)

  python -m rnnoise_amd.cli export CKPT OUT [--densities R,Z,N] [--pack]

The arithmetic that the byte comparison of tests/test_export_cpu.py holds in place (blob._linear_int8 does most of it):
  - float32 arrays as they come out of the checkpoint; conv1, dense_out and vad_dense stay float
  - the scale of a layer from the float32 matrix (largest magnitude / 127 against largest pair sum / 129), weight / (scale + 1e-30)
    rounded half to even
  - subias = bias - sum(q * scale) formed in float64 and rounded once to float32 (the C file carries the double's shortest decimal
    representation, which the compiler reads back exactly); scale / 127 likewise
  - a block of 4 inputs x 8 outputs is kept when the sum of its float magnitudes exceeds 1e-10
  - the scale of a recurrent matrix is taken BEFORE its three diagonals leave it (print_linear_layer computes it, print_sparse_weight
    then extracts the diagonals and quantises the rest with it)
Other dimensions, weight-norm checkpoints and anything else this refuses are heard through the split calls instead
(rnnoise_batch_analyze / rnnoise_batch_synthesize; cli denoise --checkpoint / --torch-net)."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from . import blob

COND, GRU = 128, 384
FEATURES, BANDS = 65, 32
SHAPES = OrderedDict([
    ("conv1.weight", (COND, FEATURES, 3)), ("conv1.bias", (COND,)),
    ("conv2.weight", (GRU, COND, 3)), ("conv2.bias", (GRU,)),
    *[(f"gru{k}.{p}_l0", shape) for k in (1, 2, 3)
      for p, shape in (("weight_ih", (3 * GRU, GRU)), ("weight_hh", (3 * GRU, GRU)), ("bias_ih", (3 * GRU,)), ("bias_hh", (3 * GRU,)))],
    ("dense_out.weight", (BANDS, 4 * GRU)), ("dense_out.bias", (BANDS,)),
    ("vad_dense.weight", (1, 4 * GRU)), ("vad_dense.bias", (1,)),
])
_SPLIT = "run such a network between the split calls instead (rnnoise_batch_analyze / rnnoise_batch_synthesize; cli denoise --torch-net)"


def _array(t) -> np.ndarray:
    """a tensor or array of the state dict as a float32 numpy array (a copy)"""
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.array(t, dtype=np.float32)


def check_state_dict(sd) -> "OrderedDict[str, np.ndarray]":
    """the state dict as float32 arrays in SHAPES' order; ValueError, naming the split calls, on weight-norm keys, missing or surplus
    tensors, other dimensions, and weights that are not finite"""
    keys = list(sd.keys())
    wn = [k for k in keys if k.endswith(("_g", "_v", "original0", "original1"))]
    if wn:
        raise ValueError(f"weight-norm parameters in the checkpoint ({wn[0]}, ...): remove the weight norm before exporting, or {_SPLIT}")
    missing = [k for k in SHAPES if k not in sd]
    if missing:
        raise ValueError(f"the checkpoint lacks {missing}: not the trainer's model; {_SPLIT}")
    surplus = [k for k in keys if k not in SHAPES]
    if surplus:
        raise ValueError(f"tensors the blob has no place for: {surplus}; {_SPLIT}")
    out = OrderedDict()
    for k, shape in SHAPES.items():
        a = _array(sd[k])
        if a.shape != shape:
            raise ValueError(f"{k} is {a.shape}, the blob holds {shape} (cond_size {COND}, gru_size {GRU}); {_SPLIT}")
        if not np.isfinite(a).all():
            raise ValueError(f"{k} holds weights that are not finite; nothing to export ({_SPLIT} to hear what it does)")
        out[k] = a
    return out


def _zrn(a: np.ndarray) -> np.ndarray:
    """torch's gate order r, z, n along axis 0 -> the C runtime's z, r, n"""
    return np.concatenate([a[GRU:2 * GRU], a[:GRU], a[2 * GRU:]], axis=0)


def blob_from_state_dict(sd) -> bytes:
    """The "DNNw" blob the reference's exporter and writer make of this state dict: 43 records, same order, same bytes.  ValueError
    where check_state_dict refuses, and the exporter's own "value out of bounds" where a weight does not fit its int8."""
    w = check_state_dict(sd)
    rec: "OrderedDict[str, np.ndarray]" = OrderedDict()

    def floats(name, lin, bias):
        rec[name + "_weights_float"] = np.ascontiguousarray(lin, np.float32).reshape(-1)
        rec[name + "_bias"] = bias

    conv = lambda a: np.transpose(a, (2, 1, 0)).reshape(-1, a.shape[0])  # [out][in][tap] -> [tap * in][out]
    floats("conv1", conv(w["conv1.weight"]), w["conv1.bias"])
    blob._linear_int8(rec, "conv2", conv(w["conv2.weight"]), w["conv2.bias"])
    for k in (1, 2, 3):
        g = lambda p: _zrn(w[f"gru{k}.{p}_l0"])
        blob._linear_int8(rec, f"gru{k}_input", g("weight_ih").T, g("bias_ih"), sparse=True)
        blob._linear_int8(rec, f"gru{k}_recurrent", g("weight_hh").T, g("bias_hh"), sparse=True, diagonal=True, scale_with_diagonal=True)
    floats("dense_out", w["dense_out.weight"].T, w["dense_out.bias"])
    floats("vad_dense", w["vad_dense.weight"].T, w["vad_dense.bias"])
    assert len(rec) == 43
    return blob.write_blob(rec)


def prune_state_dict(sd, densities=(0.3, 0.2, 0.5)):
    """The trainer's sparsification (torch/sparsification: sparsify_matrix as GRUSparsifier applies it once its schedule has ended)
    in one shot: in every GRU matrix of a copy of `sd`, gate by gate (densities: reset, update, new), the round(blocks * density) blocks
    of 8 x 4 on the torch layout with the largest sum of squares survive (threshold by sort; ties at the threshold survive), the
    others become zero; the diagonal of a recurrent gate matrix is outside the energies and is kept.  The reductions are torch's, as
    the reference's, so that the masks agree with its own.  Returns an OrderedDict of torch tensors."""
    import torch
    if len(densities) != 3 or not all(0.0 <= float(d) <= 1.0 for d in densities):
        raise ValueError("densities: three values in [0, 1] for the reset, update and new gates")
    out = OrderedDict((k, torch.as_tensor(np.array(v.detach().cpu().numpy() if hasattr(v, "detach") else v))) for k, v in sd.items())
    for k in (1, 2, 3):
        for side in ("ih", "hh"):
            W = out[f"gru{k}.weight_{side}_l0"]
            n = W.shape[0] // 3
            for gate, density in enumerate(densities):
                m = W[gate * n:(gate + 1) * n]
                rows, cols = m.shape
                if rows % 8 or cols % 4:
                    raise ValueError(f"8 x 4 blocks do not divide a gate matrix of {tuple(m.shape)}")
                spared = torch.diag(torch.diag(m)) if side == "hh" else torch.zeros_like(m)
                rest = m - spared
                energy = torch.sum(torch.sum(torch.reshape(rest, (rows // 8, 8, cols // 4, 4)) ** 2, dim=3), dim=1)
                survivors = round(energy.numel() * float(density))
                threshold = torch.sort(torch.flatten(energy)).values[-survivors] if survivors else 0
                mask = torch.ones_like(energy)
                mask[energy < threshold] = 0
                mask = torch.repeat_interleave(torch.repeat_interleave(mask, 8, dim=0), 4, dim=1)
                W[gate * n:(gate + 1) * n] = mask * rest + spared
    return out


def load_state_dict_file(path: str):
    """the state dict of a trainer checkpoint: torch.save({'state_dict': ..., 'model_kwargs': ...}) as train_rnnoise.py writes it, or
    a bare state dict.  model_kwargs that name other dimensions are refused here, before any tensor is looked at."""
    import torch
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except TypeError:  # (a torch without the argument)
        ck = torch.load(path, map_location="cpu")
    if isinstance(ck, dict) and "state_dict" in ck:
        kw = ck.get("model_kwargs") or {}
        if kw.get("cond_size", COND) != COND or kw.get("gru_size", GRU) != GRU:
            raise ValueError(f"the checkpoint is of cond_size {kw.get('cond_size')}, gru_size {kw.get('gru_size')}; the blob holds "
                             f"{COND} / {GRU}; {_SPLIT}")
        ck = ck["state_dict"]
    return ck


def export_file(checkpoint: str, out: str, densities=None, pack: bool = False) -> int:
    """cli export: checkpoint -> blob file (densities: prune first; pack: the RNPK form, through rnnoise_amd_model_pack); returns the
    bytes written"""
    sd = load_state_dict_file(checkpoint)
    if densities is not None:
        sd = prune_state_dict(sd, densities)
    data = blob_from_state_dict(sd)
    if pack:
        data = blob.pack(data)
    with open(out, "wb") as f:
        f.write(data)
    return len(data)
