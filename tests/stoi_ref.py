"""The definition of include/rnnoise_amd_stoi.h restated in numpy float64 -- what the kernels of librnnoise_amd_stoi.so are held to -- and
the signals the tests feed them.

  score_row(ref, deg)      STOI and ESTOI sums, K, segments and the silent-frame margin of one aligned pair of spans
  score(ref, inp, out..)   the library's (N, 8) results for (T, N, 480) planes, with the margins
  make_signal, degrade     broadband noise under a 3 Hz speech-like envelope, float32; the same plus white noise

Every sum is written out in the header's order (seqsum: one accumulator, ascending).  `fft` and `descending` give the same numbers
in other orders: np.fft.rfft against an explicit DFT matrix product, band and column sums ascending against descending -- the
differences between them are the reference's own error, which sets the tolerance of tests/test_stoi_gpu.py.
"""
import numpy as np

from rnnoise_amd import stoi_tables as TB

FRAME = 480
EPS = 2.0 ** -52
CLIP = 6.623413251903491  # 1 + 10 ** (15 / 20)
WIN, HOP, NFFT, NSEG, NBANDS = 256, 128, 512, 30, 15
assert CLIP == 1.0 + 10.0 ** 0.75


def seqsum(a, axis=-1, descending=False):
    """the sum along `axis` by one accumulator from 0.0, ascending (or descending) along it"""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    acc = np.zeros(a.shape[1:], np.float64)
    for i in (range(a.shape[0] - 1, -1, -1) if descending else range(a.shape[0])):
        acc = acc + a[i]
    return acc


def resample(x):
    """48 -> 10 kHz: y[m] = 5 sum_n h[1152 + 24 m - 5 n] x[n], the taps of an output in ascending k; x: L samples, L % 24 == 0"""
    x = np.asarray(x, np.float64)
    L = x.size
    assert L % 24 == 0
    Q = L // 24  # outputs per phase
    pad = 240
    xp = np.concatenate([np.zeros(pad), x, np.zeros(pad + 24)])
    y = np.zeros(5 * Q)
    for r in range(5):
        k0, c = (24 * r + TB.CENTRE) % 5, (24 * r + TB.CENTRE) // 5
        at = pad + c + 24 * np.arange(Q)
        acc = np.zeros(Q)
        for j in range(TB.PHASE_TAPS):
            acc = acc + TB.H[k0 + 5 * j] * xp[at - j]
        y[r::5] = 5.0 * acc
    return y


def n_frames_10k(l10):
    return 0 if l10 < WIN else (l10 - WIN) // HOP + 1


def frames(y, n):
    """(n, 256) windowed frames of y at hop 128"""
    return TB.W * y[HOP * np.arange(n)[:, None] + np.arange(WIN)[None, :]]


def _dft_matrix():
    k, n = np.arange(NFFT // 2 + 1)[None, :], np.arange(WIN)[:, None]
    return np.exp(-2j * np.pi * ((k * n) % NFFT) / NFFT)


def envelopes(c, M, fft="rfft", descending=False):
    """(M, 15) band envelopes of the compacted signal c"""
    z = frames(c, M)
    spec = np.fft.rfft(z, NFFT, axis=1) if fft == "rfft" else z @ _dft_matrix()
    power = spec.real * spec.real + spec.imag * spec.imag
    return np.stack([np.sqrt(seqsum(power[:, a:b], 1, descending)) for a, b in TB.BANDS], axis=1)


def segment_terms(X, Y, descending=False):
    """the STOI and ESTOI terms of every segment: X, Y (M, 15) envelopes of ref and degraded -> two (M - 29,) arrays"""
    M = X.shape[0]
    n = M - NSEG + 1
    if n <= 0:
        return np.zeros(0), np.zeros(0)
    at = np.arange(n)[:, None] + np.arange(NSEG)[None, :]
    x, y = X[at].transpose(0, 2, 1), Y[at].transpose(0, 2, 1)  # (segments, bands, columns)
    s = lambda a, axis=-1: seqsum(a, axis, descending)
    rows = lambda a: (a - (s(a) / NSEG)[..., None])
    unit = lambda a, axis=-1: a / np.expand_dims(np.sqrt(s(a * a, axis)) + EPS, axis)
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = np.sqrt(s(x * x)) / (np.sqrt(s(y * y)) + EPS)
        yp = np.minimum(alpha[..., None] * y, x * CLIP)
        xn, pn = unit(rows(x)), unit(rows(yp))
        stoi = s(s(xn * pn), -1) / NBANDS
        yn = unit(rows(y))
        cols = lambda a: unit(a - np.expand_dims(s(a, 1) / NBANDS, 1), 1)
        estoi = s(s(cols(xn) * cols(yn), 1), -1) / NSEG
    return stoi, estoi


def keep(ref10):
    """the kept frames of a 10 kHz ref signal -> (indices, margin in dB)"""
    F = n_frames_10k(ref10.size)
    if F == 0:
        return np.zeros(0, np.int64), np.inf
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = frames(ref10, F)
        e = 20.0 * np.log10(np.sqrt(seqsum(w * w, 1)) + EPS)
        limit = np.max(e) - 40.0
        return np.nonzero(e > limit)[0], float(np.min(np.abs(e - limit)))


def compact(y10, idx):
    c = np.zeros(HOP * (idx.size + 1))
    for k, j in enumerate(idx):
        c[HOP * k:HOP * k + WIN] += TB.W * y10[HOP * j:HOP * j + WIN]
    return c


def score_row(ref, deg, fft="rfft", descending=False, ref10=None):
    """ref, deg: the aligned spans (L float32 or float64 samples each) -> dict(stoi, estoi: the sums over segments; segments; K; margin)"""
    ref10 = resample(ref) if ref10 is None else ref10
    deg10 = ref10 if deg is ref else resample(deg)
    idx, margin = keep(ref10)
    K = idx.size
    out = dict(stoi=0.0, estoi=0.0, segments=0, K=K, margin=margin)
    if K > NSEG:
        X, Y = (envelopes(compact(v, idx), K - 1, fft, descending) for v in (ref10, deg10))
        st, es = segment_terms(X, Y, descending)
        out.update(stoi=float(seqsum(st, 0, descending)), estoi=float(seqsum(es, 0, descending)), segments=st.size)
    return out


def sequences(plane, n_frames):
    """(N, n_frames * 480) float64 from a (T, N, 480) plane"""
    return np.asarray(plane[:n_frames], np.float64).transpose(1, 0, 2).reshape(plane.shape[1], -1)


def score(ref, inp, out, n_frames, first=2, delay=960, fft="rfft", descending=False):
    """the library's results for (T, N, 480) planes (inp may be None) -> ((N, 8) float64, (N,) margins)"""
    N = out.shape[1]
    res, margins = np.zeros((N, 8)), np.zeros(N)
    r, y = sequences(ref, n_frames), sequences(out, n_frames)
    x = sequences(inp, n_frames) if inp is not None else None
    a, b = first * FRAME, n_frames * FRAME
    for s in range(N):
        rs = r[s, a - delay:b - delay]
        ref10 = resample(rs)
        for base, d in ((0, x), (4, y)):
            if d is None:
                continue
            ds = d[s, a:b] if d is y else d[s, a - delay:b - delay]
            g = score_row(rs, ds, fft, descending, ref10)
            res[s, base:base + 4] = g["stoi"], g["estoi"], g["segments"], g["K"]
            margins[s] = g["margin"]
    return res, margins


def make_signal(seed, T):
    """T frames at 48 kHz: white noise (every band carries energy) under a 3 Hz raised envelope that falls 80 dB between its
    bursts (silent-frame removal removes frames), float32 at PCM scale"""
    rng = np.random.default_rng(seed)
    n = T * FRAME
    t = np.arange(n) / 48000.0
    env = np.maximum(np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 2 * np.pi)), 0.0) ** 2 + 1e-4
    return (3000.0 * env * rng.standard_normal(n)).astype(np.float32)


def degrade(clean, snr_db, seed):
    """clean plus white noise at snr_db, float32"""
    rng = np.random.default_rng(seed)
    c = np.asarray(clean, np.float64)
    noise = rng.standard_normal(c.size) * np.sqrt(np.mean(c * c) / 10.0 ** (snr_db / 10.0))
    return (c + noise).astype(np.float32)
