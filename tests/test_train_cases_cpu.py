"""The stream set of tests/train_cases.py, without a GPU: that the oracle alone, run over it, takes every branch the set is there for
-- the clamp of the gain targets, the TRAINING build's silence rule in both outcomes, empty bands beside valid ones, the vad == 0 &&
noise_free rule, the band_lp rule and the whole pitch range.  The GPU tests that run the set (tests/test_train_features_gpu.py) are
only as good as what is checked here."""
import numpy as np
import pytest

import train_cases as tc
from conftest import bits


@pytest.fixture(scope="module")
def run():
    c = tc.cases()
    return c, tc.oracle_records(c)


def streams(c, label):
    return [s for s in range(c.n) if c.labels[s] == label]


def test_the_set_is_deterministic_and_every_category_is_there(run):
    c, rec = run
    tc.cases.cache_clear()
    again = tc.cases()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c[:6], again[:6])) and again.labels == c.labels
    assert c.clean.shape == c.noisy.shape == (tc.T, tc.D, 480) and c.vad.shape == (tc.T, tc.D) and rec.shape == (tc.T, tc.D, tc.REC)
    assert all(a.dtype == np.float32 for a in c[:3]) and all(a.dtype == np.int32 and a.shape == (tc.D,) for a in c[3:6])
    counts = {k: c.labels.count(k) for k in set(c.labels)}
    assert set(counts) == {"pitch", "louder", "threshold", "empty", "zeros", "vad", "recipe"} and min(counts.values()) >= 5
    assert np.isfinite(rec).all()
    assert (bits(rec[..., 97]) == bits(c.vad)).all(), "the record passes the VAD target through"
    # the VAD targets: 0, -0.0, a non-binary value and 1, under noise_free 0 and 1
    v = streams(c, "vad")
    for nf in (0, 1):
        seen = {int(b) for s in v if c.noise_free[s] == nf for b in bits(c.vad[:, s])}
        assert seen >= {0x00000000, 0x80000000, 0x3F000000, 0x3F800000}, nf
    # cycled over 64-stream waves, every wave of a batch sees several categories
    for n in (130, 483):
        lab = tc.cycled(n, slice(0, 1)).labels
        assert all(len(set(lab[w:w + 64])) >= 5 for w in range(0, n, 64) if n - w >= 8)


def test_clean_louder_than_noisy_clamps_most_targets(run):
    c, rec = run
    for s in streams(c, "louder"):
        assert (c.lowpass[s], c.band_lp[s], c.noise_free[s]) == (481, 32, 0) and (c.vad[:, s] == 1).all()
        g = rec[:, s, tc.TARGETS]
        assert (g == 1.0).mean() >= 0.5, (s, (g == 1.0).mean())
        assert (g[:8] == 1.0).mean() >= 0.5, "also in the frames of the short GPU runs"


def test_the_threshold_streams_are_silent_and_live(run):
    """E < 0.1 with nothing else in the way: all 32 targets -1 in some frames, a valid target in others -- beyond the first frame,
    whose window is half empty"""
    c, rec = run
    both, silent, live = [], [], []
    for s in streams(c, "threshold"):
        assert (c.lowpass[s], c.band_lp[s], c.noise_free[s]) == (481, 32, 0) and (c.vad[:, s] == 1).all()
        g = rec[1:, s, tc.TARGETS]
        sil, ok = (g == -1).all(1), (g >= 0).any(1)
        assert (sil | ok).all()
        (both if sil.any() and ok.any() else silent if sil.all() else live).append(s)
    assert len(both) >= 3 and silent and live, (both, silent, live)
    # in the frames of the short GPU runs too
    assert sum(1 for s in both if len({bool(x) for x in (rec[1:8, s, tc.TARGETS] == -1).all(1)}) == 2) >= 3


def test_empty_bands_beside_valid_ones(run):
    c, rec = run
    mixed = []
    for s in streams(c, "empty"):
        assert (c.lowpass[s], c.band_lp[s], c.noise_free[s]) == (481, 32, 0) and (c.vad[:, s] == 1).all()
        g = rec[:, s, tc.TARGETS]
        live = ~(g == -1).all(1)
        if ((g[live] == -1).any(1) & (g[live] >= 0).any(1)).sum() >= tc.T // 2:
            mixed.append(s)
    assert len(mixed) >= 3, mixed


def test_exact_zero_frames_in_either_signal_and_in_both(run):
    c, _ = run
    z = streams(c, "zeros")
    zc, zx = ~c.clean[:, z].any(-1), ~c.noisy[:, z].any(-1)                  # (T, streams): the frame is zero
    assert (zc & ~zx).any() and (~zc & zx).any() and (zc & zx).any()
    assert zc.all(0).any() and (zc & zx).all(0).any(), "one stream is zero throughout"
    for t in (1, 7, 8):                                                      # a run starts or ends at every call boundary of the GPU tests
        assert ((zc[t] != zc[t - 1]) | (zx[t] != zx[t - 1])).any(), t


def test_noise_free_pairs_differ_exactly_where_vad_is_zero(run):
    c, rec = run
    prs = tc.pairs(c, "noise_free")
    assert len(prs) >= 5
    for i, j in prs:
        ne = bits(rec[:, i]) != bits(rec[:, j])
        assert not ne[:, :65].any() and not ne[:, 97].any()
        zero = c.vad[:, i] == 0                                              # (+0 and -0)
        assert zero.any() and not zero.all() and zero[:8].any()
        assert ne[zero][:, tc.TARGETS].all() and not ne[~zero].any(), (i, j)
    assert any((bits(c.vad[:, i]) == 0x80000000).any() for i, _ in prs)


def test_band_lp_pairs_differ_only_above_the_limit(run):
    c, rec = run
    prs = tc.pairs(c, "band_lp")
    assert len(prs) >= 3
    some = False
    for i, j in prs:
        assert {int(c.band_lp[i]), int(c.band_lp[j])} == {32, 16}
        ne = bits(rec[:, i]) != bits(rec[:, j])
        assert not ne[:, :65 + 17].any() and not ne[:, 97].any()
        live = ~((c.vad[:, i] == 0) & (c.noise_free[i] != 0))
        assert ne[live][:, 65 + 17:97].all(), (i, j)
        some |= bool(live[:8].any())
    assert some


def test_the_pitch_feature_spans_the_whole_range(run):
    """feature 64 = .01 * (pitch - 300), src/denoise.c:377, pitch 60 .. 767: the ends fuzz_pcm is documented to reach"""
    c, rec = run
    lo, hi = np.float32(0.01 * (60 - 300)), np.float32(0.01 * (767 - 300))
    for r in (rec, rec[:8]):
        assert r[..., 64].min() == lo and r[..., 64].max() == hi, (r[..., 64].min(), r[..., 64].max())
    assert len(np.unique(rec[..., 64])) >= 250


def test_the_edge_subset_covers_every_band_limit_and_category():
    e = tc.edge_subset()
    assert 12 <= e.n <= 16 and e.clean.shape[0] == 16
    assert set(e.lowpass.tolist()) == set(tc.EDGE_LOWPASS) and set(e.band_lp.tolist()) == set(tc.EDGE_BAND_LP)
    assert set(e.labels) == set(tc.cases().labels) and set(e.noise_free.tolist()) == {0, 1}
