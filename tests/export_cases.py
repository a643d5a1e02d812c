"""What the exporter's tests share (plain helper module: tests/test_export_cpu.py, tests/test_export_gpu.py): a state dict of the
trainer's model drawn from a numpy seed, so that the exporter, the pruning and the float network are tested where no reference tree and
no oracle/_ref exist.  The magnitudes follow rnnoise_amd.blob.synth_model: large enough that tanh and the sigmoids leave their linear
range now and then."""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np

DENSITIES = (0.3, 0.2, 0.5)


def state_dict(seed: int = 11, boost: float = 3.0) -> "OrderedDict[str, np.ndarray]":
    """float32 numpy arrays under the trainer's parameter names (rnnoise_amd.export.SHAPES), dense"""
    from rnnoise_amd import export
    rng = np.random.Generator(np.random.PCG64(seed))
    bound = {"conv1": boost / np.sqrt(195), "conv2": boost / np.sqrt(384), "dense_out": 2 * boost / np.sqrt(1536),
             "vad_dense": 2 * boost / np.sqrt(1536)}
    sd = OrderedDict()
    for name, shape in export.SHAPES.items():
        layer, par = name.split(".")
        if layer.startswith("gru"):
            a = (boost if "_ih_" in par else 2.0 if par.startswith("weight") else 1.0) / np.sqrt(384)
        elif par == "bias":
            a = {"dense_out": 1.0, "vad_dense": 0.1}.get(layer, 1 / np.sqrt(384))
        else:
            a = bound[layer]
        sd[name] = rng.uniform(-a, a, size=shape).astype(np.float32)
    return sd


@functools.lru_cache(None)
def pruned_blob(seed: int = 11):
    """(the pruned state dict as torch tensors, its blob): state_dict(seed) at DENSITIES through prune_state_dict, exported"""
    from rnnoise_amd import export
    sd = export.prune_state_dict(state_dict(seed), DENSITIES)
    return sd, export.blob_from_state_dict(sd)
