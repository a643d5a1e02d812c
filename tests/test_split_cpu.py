"""The split calls without a GPU (include/rnnoise_amd.h: rnnoise_batch_analyze, rnnoise_batch_synthesize):

  a  the header, the exported symbols and their capi mirrors
  b  rnnoise_amd_split_rows_check at its boundaries, rnnoise_amd_split_frame_bytes
  c  NULL arguments
  d  the split oracle (tests/csrc/split_oracle.c), which tests/test_split_gpu.py checks arbitrary gains against: fed the oracle's own
     gains and vad it equals Oracle.run bit for bit -- out, features, silence and every float of the state --, silent frames
     included, whatever the number of frames between analysis and synthesis
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, load_blob
from oracle.binding import Oracle
from rnnoise_amd import capi, synth

NAMES = ["rnnoise_amd_split_frame_bytes", "rnnoise_amd_split_rows_check", "rnnoise_batch_split_reserve", "rnnoise_batch_split_pending",
         "rnnoise_batch_analyze_device", "rnnoise_batch_analyze_device_s16", "rnnoise_batch_analyze", "rnnoise_batch_analyze_s16",
         "rnnoise_batch_synthesize_device", "rnnoise_batch_synthesize_device_s16", "rnnoise_batch_synthesize",
         "rnnoise_batch_synthesize_s16"]


# ---- a. the surface ----
def test_header_exports_and_mirrors():
    h = open(os.path.join(ROOT, "include", "rnnoise_amd.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(rf"RNNOISE_EXPORT (int|long) {name}\(", h), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert int(re.search(r"#define RNNOISE_AMD_FEATURES (\d+)", h).group(1)) == capi.FEATURES == capi.NB_FEATURES == 65
    assert re.search(r"typedef struct RNNoiseRows \{\s*long frame_stride, row_stride;", h)
    assert C.sizeof(capi.Rows) == 2 * C.sizeof(C.c_long) and [f[0] for f in capi.Rows._fields_] == ["frame_stride", "row_stride"]
    for name in ("analyze", "synthesize", "analyze_device", "synthesize_device", "split_reserve"):
        assert callable(getattr(capi.Batch, name)), name
    assert isinstance(capi.Batch.split_pending, property)


# ---- b. the two host-only functions ----
def ok(rows, row, n, T):
    return capi.split_rows_check(rows, row, n, T)


@pytest.mark.parametrize("row", [65, 32, 1])
def test_rows_check_boundaries(row):
    n, T = 7, 12
    L = capi.lib()
    # NULL and {0, 0} are [frame][n][row]
    assert ok(None, row, n, T) and ok((0, 0), row, n, T) and ok(None, row, 1, 0) and ok(None, row, n, 1)
    assert L.rnnoise_amd_split_rows_check(C.byref(capi.Rows(0, 0)), row, n, T) == 1
    assert not ok(None, 0, n, T) and not ok(None, row, 0, T) and not ok(None, row, n, -1) and not ok((n * row, row), row, -1, T)
    # one stride without the other, or a negative one
    assert not ok((n * row, 0), row, n, T) and not ok((0, row), row, n, T) and not ok((-n * row, row), row, n, T)
    assert not ok((n * row, -row), row, n, T)
    # [frame][n][row]: tight and padded; nothing has to be a multiple of anything
    assert ok((n * row, row), row, n, T) and ok((n * (row + 3) + 1, row + 3), row, n, T)
    assert not ok((n * row - 1, row), row, n, T)                        # frames overlap
    if row > 1:
        assert not ok((n * row, row - 1), row, n, T)                    # rows overlap
    # [n][T][row], the trainer's batch-first tensor
    assert ok((row, T * row), row, n, T) and ok((row + 2, T * (row + 2) + 5), row, n, T)
    assert not ok((row, T * row - 1), row, n, T)                        # streams overlap
    if row > 1:
        assert not ok((row - 1, T * row), row, n, T)                    # frames overlap
    # no slot at all fits whatever the strides
    assert ok((1, 1), row, n, 0)


def test_frame_bytes():
    # per stream and frame: the X and P spectra (481 complex each, rows padded to 964 floats), Ex | Ep | Exp, the silence word
    per_stream = (2 * 964 + 96 + 1) * 4
    for n in (1, 3, 64, 257, 4096, 65536):
        v = capi.split_frame_bytes(n)
        assert v % 256 == 0 and n * per_stream <= v < n * per_stream + 4 * 256, (n, v)
    assert capi.lib().rnnoise_amd_split_frame_bytes(0) == -1 and capi.lib().rnnoise_amd_split_frame_bytes(-5) == -1
    with pytest.raises(ValueError):
        capi.split_frame_bytes(0)


# ---- c. NULL ----
def test_null_arguments():
    L = capi.lib()
    assert L.rnnoise_batch_split_pending(None) == -1 and L.rnnoise_batch_split_reserve(None, 4) == -1
    for fn in (L.rnnoise_batch_analyze_device, L.rnnoise_batch_analyze_device_s16):
        assert fn(None, None, None, None, None, 1, None) == -1
    for fn in (L.rnnoise_batch_analyze, L.rnnoise_batch_analyze_s16):
        assert fn(None, None, None, None, None, 1) == -1
    for fn in (L.rnnoise_batch_synthesize_device, L.rnnoise_batch_synthesize_device_s16):
        assert fn(None, None, None, None, None, None, 0, None) == -1
    for fn in (L.rnnoise_batch_synthesize, L.rnnoise_batch_synthesize_s16):
        assert fn(None, None, None, None, None, None, 0) == -1


# ---- d. the split oracle against the oracle ----
@pytest.mark.parametrize("pair", [1, 5, 14])
def test_split_oracle_with_the_oracles_gains_is_the_oracle(pair):
    """stream 77 with three leading silent frames, 14 frames: analysis runs `pair` frames ahead of synthesis"""
    from split_oracle import SplitStream
    blob = load_blob("default")
    pcm = synth.batch_pcm([77], 14, lead_silence=3)[:, 0]
    o = Oracle(blob)
    want = o.run(pcm)
    assert want["silence"][:3].all() and not want["silence"][3:].any()
    # a  with rno_compute_rnn in the middle, on the same flat state
    s = SplitStream()
    got = s.run_with_model(blob, pcm, pair)
    for k in ("out", "vad", "gains", "features", "silence"):
        assert_bits_equal(got[k], want[k], f"pair {pair}: {k}")
    assert_bits_equal(s.state, o.state, f"pair {pair}: the state")
    # b  fed the recorded gains and vad, garbage on the silent frames: everything but the network state
    s2 = SplitStream()
    g, v = want["gains"].copy(), want["vad"].copy()
    g[:3], v[:3] = np.nan, 7.0
    out = []
    for t0 in range(0, 14, pair):
        feats, sil = s2.analyze(pcm[t0:t0 + pair])
        assert_bits_equal(sil, want["silence"][t0:t0 + pair], "silence words")
        out.append(s2.synthesize(g[t0:t0 + pair], v[t0:t0 + pair]))
    assert_bits_equal(np.concatenate(out), want["out"], f"pair {pair}: out from recorded gains")
    nn = slice(2724, 4262)  # include/rn_layout.h: RN_OFF_CONV1 .. RN_OFF_DELAYED_X, the network's histories and GRU states
    keep = np.ones(len(o.state), bool)
    keep[nn] = False
    assert_bits_equal(s2.state[keep], o.state[keep], "the DSP state from recorded gains")
    assert not s2.state[nn].any(), "the split oracle touched the network state"
