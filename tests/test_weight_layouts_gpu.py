"""Every weight layout of tests/weight_layouts.py that the loader accepts, through every network path, stream by stream
against the oracle.  Each path reads its own device copy of the int8 layers: the vector kernel the block stream, the
one-stream kernel and the drop-in row kernels the row-major chunks, the tile kernels and the layer-wise GRU the dense MFMA
image.  Gains, VAD and PCM are compared bit for bit, and the exported state of the first, middle and last streams.

tests/test_gpu_parity.py re-runs these cases with the throughput kernels forced onto small batches
(test_throughput_kernels_at_small_sizes: rn_nn_vector_kernel, the sixteen-wave tile) and with the at-size kernels
(test_at_size_kernels_on_small_ragged_batches: the four-wave GRU layer kernel, the layer-wise network from size 0)."""
import numpy as np
import pytest

import weight_layouts as wl
from conftest import assert_bits_equal
from oracle.binding import Oracle
from rnnoise_amd import capi, synth

pytestmark = pytest.mark.gpu

T = 24
_models, _oracle = {}, {}


def _model(name):
    if name not in _models:
        _models[name] = capi.Model(wl.make(name))
    return _models[name]


def _key(s):
    """(signal, silent for the first five frames, silent in the middle): the oracle runs once per key and layout"""
    return (7 * s) % 5, s % 3 == 0, s % 4 == 1


def _signals(n):
    pcm = synth.batch_pcm([_key(s)[0] for s in range(n)], T)
    for s in range(n):
        _, lead, mid = _key(s)
        if lead:
            pcm[:5, s] = 0
        if mid:
            pcm[10:14, s] = 0
    return pcm


def _want(name, pcm, s):
    k = (name, _key(s))
    if k not in _oracle:
        o = Oracle(wl.make(name))
        _oracle[k] = (o.run(pcm[:, s]), o.get_state())
    return _oracle[k]


ROUTES = {  # route: (streams, nn path, frames per call)
    "path0_37": (37, 0, T),          # rn_nn_one_kernel (rn_nn_vector_kernel in the forced run)
    "path1_37": (37, 1, T),          # tile kernel, eight-wave form, one 24-frame call
    "path1_37_by_frame": (37, 1, 1),  # tile kernel, sixteen-wave form: 24 one-frame calls
    "path2_70": (70, 2, T),          # layer-wise network: partial 16-stream tile, partial 64-stream group
}


@pytest.mark.parametrize("route", list(ROUTES) + ["dropin"])
@pytest.mark.parametrize("name", wl.ACCEPTED)
def test_weight_layout_on_every_network_path(name, route):
    m = _model(name)
    if route == "dropin":   # three drop-in states: rnnoise_create(model) / rnnoise_process_frame, the row kernels
        pcm = _signals(3)
        states = [capi.DenoiseState(m) for _ in range(3)]
        for s, st in enumerate(states):
            want, _ = _want(name, pcm, s)
            for t in range(T):
                out, vad = st.process_frame(pcm[t, s])
                assert_bits_equal(out, want["out"][t], f"{name}: drop-in state {s}, frame {t}: pcm")
                assert_bits_equal(np.float32(vad), want["vad"][t], f"{name}: drop-in state {s}, frame {t}: vad")
            st.close()
        return
    n, path, per_call = ROUTES[route]
    pcm = _signals(n)
    b = capi.Batch(m, n)
    b.set_nn_path(path)
    res = [b.process(pcm[t:t + per_call]) for t in range(0, T, per_call)]
    out, vad, gains = (np.concatenate([r[k] for r in res]) for k in range(3))
    for s in range(n):
        want, state = _want(name, pcm, s)
        assert_bits_equal(gains[:, s], want["gains"], f"{name}: gains of stream {s}")
        assert_bits_equal(vad[:, s], want["vad"], f"{name}: vad of stream {s}")
        assert_bits_equal(out[:, s], want["out"], f"{name}: pcm of stream {s}")
        if s in (0, n // 2, n - 1):
            assert_bits_equal(b.export_state(s), state, f"{name}: state of stream {s}")
    assert any(_want(name, pcm, s)[0]["silence"].any() for s in range(n))
    b.close()
