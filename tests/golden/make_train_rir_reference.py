"""Records tests/golden/train_rir_reference.npz from the reference's own rir_filter_sequence (tests/csrc/ref_dump_harness.c; needs the
reference's sources and oracle/_ref): python tests/golden/make_train_rir_reference.py [directory to write into instead].  The recipe
of its inputs and what it keeps are in tests/test_train_rir_cpu.py (reference_recipe, record_reference), which also checks the
committed file against the reference."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_train_rir_cpu as t  # noqa: E402
from train_support import reference_dump_features  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        L = reference_dump_features(d)
        if isinstance(L, str):
            sys.exit(L)
        np.savez(os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "train_rir_reference.npz"), **t.record_reference(L, d))
