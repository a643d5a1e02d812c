"""Loading a side library (librnnoise_amd_score.so, _train.so, _gru.so, _gru_stack.so, _stoi.so, _fnet.so): each is a library of its
own with a prototype table of its own in its module; how it is loaded is the same for all six."""
from __future__ import annotations

import ctypes as C
import os

from . import capi

_loaded = {}


def load(lib_path: str, prototypes: dict):
    """the library at lib_path with `prototypes` (symbol -> (restype, argtypes)) set on it; loaded once per path"""
    L = _loaded.get(lib_path)
    if L is None:
        capi._share_hip_runtime_with_torch()  # (one HIP runtime per process, as for the product library)
        if not os.path.exists(lib_path):
            raise RuntimeError(f"{lib_path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = C.CDLL(lib_path)
        for name, (restype, argtypes) in prototypes.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _loaded[lib_path] = L
    return L
