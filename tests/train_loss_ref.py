"""The reference for librnnoise_amd_train.so's numbers (TEST INFRASTRUCTURE): the loss of the reference trainer
(torch/rnnoise/train_rnnoise.py:147-156) written in torch and evaluated in float64 on the CPU; its autograd gradient with respect
to the float predictions cast to double is the reference for the library's gradients.  Also the case set the CPU and GPU tests share,
the bound of the gradient comparison, and the layouts."""
import numpy as np
import torch

REC, BANDS, FEATURES = 98, 32, 65

# the values the tests must cover; 3.0 is an addition: tanh(24)^2 rounds to 1 in double, so tg = 3 exactly and a float p can EQUAL tg
# (for the other targets tg is no float, and p = float32(tg) is the nearest miss: the cancellation case of the bound instead)
TARGETS = (-1.0, 0.0, 1e-3, .5, 1.0, 1.5, 3.0)
VAD_TARGETS = (0.0, 1.0, .5, .3)
P_KINDS = ("zero", "tiny", "small", "tg", "one")  # 0, 1e-30, 1e-3, float32(tg), 1
Q_VALUES = (0.0, .5, 1.0)

# K of the gain gradient's bound: 4 x the larger of the two measured values, host program 0.990 and device 0.987
# (tests/test_train_loss_cpu.py's docstring has the measurements); beyond 64 the kernel would be wrong, whatever was measured
GRAD_K = 3.96


def shaped_target(g):
    """tg of the header, in float64 numpy"""
    g = np.maximum(np.asarray(g, np.float64), 0.0)
    return g * np.tanh(8.0 * g) ** 2


def terms(gain_t, vad_t, pred_gain, pred_vad, gamma):
    """the trainer's two per-element terms before its means, float64 torch: gain (..., 32) and vad (..., 1)"""
    target_gain = torch.clamp(gain_t, min=0)
    target_gain = target_gain * (torch.tanh(8 * target_gain) ** 2)
    e = pred_gain ** gamma - target_gain ** gamma
    gain = (1 + 5. * vad_t) * torch.clamp(gain_t + 1, max=1) * (e ** 2)
    vad = torch.abs(2 * vad_t - 1) * (-vad_t * torch.log(.01 + pred_vad) - (1 - vad_t) * torch.log(1.01 - pred_vad))
    return gain, vad


def trainer_loss(pred_gain, pred_vad, gain_t, vad_t, gamma=.25):
    """train_rnnoise.py:149-156 on already cut tensors, in whatever dtype they have -> (loss, gain_loss, vad_loss)"""
    gain, vad = terms(gain_t, vad_t, pred_gain, pred_vad, gamma)
    gain_loss, vad_loss = torch.mean(gain), torch.mean(vad)
    return gain_loss + .001 * vad_loss, gain_loss, vad_loss


def reference(records, gains, vad, t0, first, gamma, w_gain, w_vad):
    """records (T_rec, R, >= 98) from record 0, gains (n, R, 32) and vad (n, R) float32 numpy: the predictions of steps t0 .. t0 + n - 1.
    -> sums (R, 4) float64 {gain terms, vad terms, frames, 0} (plain float64 sums: close to the library's, not its bits),
    grad_gains (n, R, 32), grad_vad (n, R) float64: the gradient of w_gain * sum(gain terms) + w_vad * sum(vad terms), zeros at
    the steps that are not scored.  Where p <= 0 torch's gradient is infinite or NaN; those entries come back as they are."""
    n, R = gains.shape[0], gains.shape[1]
    f_first = min(max(max(first, 1) - t0, 0), n)
    sums, gg, gv = np.zeros((R, 4)), np.zeros((n, R, BANDS)), np.zeros((n, R))
    if f_first == n:
        return sums, gg, gv
    rec = torch.from_numpy(np.ascontiguousarray(records[t0 + f_first - 1:t0 + n - 1, :, FEATURES:REC])).double()
    p = torch.from_numpy(np.ascontiguousarray(gains[f_first:])).double().requires_grad_(True)
    q = torch.from_numpy(np.ascontiguousarray(vad[f_first:])).double().unsqueeze(-1).requires_grad_(True)
    gain, vt = terms(rec[..., :BANDS], rec[..., BANDS:], p, q, gamma)
    (w_gain * gain.sum() + w_vad * vt.sum()).backward()
    sums[:, 0], sums[:, 1], sums[:, 2] = gain.detach().sum((0, 2)).numpy(), vt.detach().sum((0, 2)).numpy(), n - f_first
    gg[f_first:], gv[f_first:] = p.grad.numpy(), q.grad.numpy()[..., 0]
    return sums, gg, gv


def ulp32(x):
    """the spacing of float32 at |x|, as float64"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def gain_scale(records, gains, t0, first, gamma, w_gain):
    """S of the gain gradient's bound: the factor that multiplies d, |w_gain| 2 (1 + 5 v) m gamma pw / p, per (step, row, band);
    0 at unscored steps and where p <= 0"""
    n = gains.shape[0]
    f_first = min(max(max(first, 1) - t0, 0), n)
    S = np.zeros(gains.shape, np.float64)
    if f_first < n:
        rec = records[t0 + f_first - 1:t0 + n - 1].astype(np.float64)
        g, v, p = rec[..., FEATURES:FEATURES + BANDS], rec[..., REC - 1:REC], gains[f_first:].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = abs(w_gain) * 2 * (1 + 5 * v) * np.minimum(g + 1, 1) * gamma * np.power(p, gamma) / p
        S[f_first:] = np.where(p > 0, s, 0.0)
    return S


def vad_bound(records, vad, t0, first, w_vad, ref):
    """the VAD gradient's bound per (step, row): ulp32(ref) + 2^-50 |w_vad| |2v - 1| (v / (.01 + q) + (1 - v) / (1.01 - q))"""
    n = vad.shape[0]
    f_first = min(max(max(first, 1) - t0, 0), n)
    b = ulp32(ref)
    if f_first < n:
        v, q = records[t0 + f_first - 1:t0 + n - 1, :, REC - 1].astype(np.float64), vad[f_first:].astype(np.float64)
        b[f_first:] += 2.0 ** -50 * abs(w_vad) * np.abs(2 * v - 1) * (v / (.01 + q) + (1 - v) / (1.01 - q))
    return b


def measured_k(got, ref, S):
    """the largest (|got - ref| - ulp32(ref)) / (2^-52 S) over the entries with S > 0 (0 where every entry is within one ulp32)"""
    use = S > 0
    if not use.any():
        return 0.0
    excess = np.abs(got.astype(np.float64)[use] - ref[use]) - ulp32(ref[use])
    return float(max(0.0, np.max(excess / (2.0 ** -52 * S[use]))))


# ---- the case set ----
def p_value(kind, g):
    if kind == "tg":
        return float(np.float32(shaped_target(g)))
    return {"zero": 0.0, "tiny": 1e-30, "small": 1e-3, "one": 1.0}[kind]


COMBOS = [(g, kind) for g in TARGETS for kind in P_KINDS]               # 35 band cases
FRAME_KINDS = [(v, q) for v in VAD_TARGETS for q in Q_VALUES]           # 12 frame cases


def case_buffers(n_rows, T, t_base=0):
    """records (T - 1 + ..., rows, 98) and the predictions gains (T - t_base, rows, 32), vad (T - t_base, rows) of steps
    t_base .. T - 1, dense float32: step t of row s is frame case (s * T + t) % 12 and its band b is band case
    ((s * T + t) * 32 + b) % 35, so 32 | 35 - coprime strides walk the whole cross product as the frames go by.
    -> records (T, rows, 98) (record T - 1 is never read), gains, vad, and cover: the set of (band case, frame case) pairs present"""
    rec = np.zeros((T, n_rows, REC), np.float32)
    rec[..., :FEATURES] = 9e9  # (features are not read: a value that would show)
    gains, vad = np.zeros((T, n_rows, BANDS), np.float32), np.zeros((T, n_rows), np.float32)
    cover = set()
    for s in range(n_rows):
        for t in range(1, T):
            k = s * T + t
            v, q = FRAME_KINDS[k % len(FRAME_KINDS)]
            rec[t - 1, s, REC - 1], vad[t, s] = v, q
            for b in range(BANDS):
                c = (k * BANDS + b) % len(COMBOS)
                g, kind = COMBOS[c]
                rec[t - 1, s, FEATURES + b], gains[t, s, b] = g, p_value(kind, g)
                cover.add((c, k % len(FRAME_KINDS)))
    return rec, gains[t_base:], vad[t_base:], cover


def random_buffers(rng, n_rows, T):
    """random frames in the ranges training sees: targets in [-1, 1.5] with masked bands, VAD targets 0 / 1 / in between,
    predictions log-uniform in [1e-6, 1], VAD predictions in [0, 1]"""
    rec = np.zeros((T, n_rows, REC), np.float32)
    g = rng.uniform(-.2, 1.5, (T, n_rows, BANDS))
    g[rng.random(g.shape) < .1] = -1.0
    rec[..., FEATURES:FEATURES + BANDS] = g
    v = rng.random((T, n_rows))
    v = np.where(rng.random(v.shape) < .6, np.round(v), v)
    rec[..., REC - 1] = v
    gains = np.exp(rng.uniform(np.log(1e-6), 0.0, (T, n_rows, BANDS))).astype(np.float32)
    vad = rng.random((T, n_rows)).astype(np.float32)
    return rec, gains, vad


def training_records(rng, n_sequences, T):
    """(sequences, T, 98) float32 records a small network can learn from: normal features, gain targets that are a squashed mix of
    the features of the frame (some bands masked with -1), a VAD target that is the sign of one of them"""
    rec = np.zeros((n_sequences, T, REC), np.float32)
    feats = rng.normal(0, 1, (n_sequences, T, FEATURES))
    mix = rng.normal(0, .3, (FEATURES, BANDS))
    g = 1 / (1 + np.exp(-(feats @ mix)))
    g[rng.random(g.shape) < .05] = -1.0
    rec[..., :FEATURES], rec[..., FEATURES:FEATURES + BANDS], rec[..., REC - 1] = feats, g, feats[..., 0] > 0
    return rec


# ---- layouts: (array that owns the memory, view shaped (steps, rows, width)) ----
def lay_out(a, layout, rng=None, pad=5):
    """a (steps, rows, width) array copied into memory of the named layout; -> view of the same shape whose strides are the layout's.
    frames: [step][row] contiguous; rows: torch's [row][step]; padded: [row][step] with `pad` floats between steps and 3 * width + 1
    between rows (the gaps hold a fill value)"""
    n, R, W = a.shape
    if layout == "frames":
        return np.ascontiguousarray(a)
    if layout == "rows":
        return np.ascontiguousarray(a.transpose(1, 0, 2)).transpose(1, 0, 2)
    assert layout == "padded", layout
    fs = W + pad
    rs = n * fs + 3 * W + 1
    flat = np.full(R * rs + 8, -3.0, a.dtype)
    view = np.lib.stride_tricks.as_strided(flat, (n, R, W), (fs * a.itemsize, rs * a.itemsize, a.itemsize))
    view[...] = a
    return view


def strides_of(view):
    """(frame_stride, row_stride) in elements of a (steps, rows, width) view"""
    return view.strides[0] // view.itemsize, view.strides[1] // view.itemsize


# ---- the assertions the host program and the device share ----
W_GAIN, W_VAD = 1.0 / (32 * 100), .001 / 100  # the weights the tests call with: the trainer's means over 100 frames


def check_against_reference(rec, gains, vad, t0, first, sums, gg, gv, K, what):
    """assertions (c) and (d) of the gradient, and the sums within float64 summation error of the reference's"""
    want, rg, rv = reference(rec, gains, vad, t0, first, .25, W_GAIN, W_VAD)
    scored = want[:, 2] > 0
    assert np.array_equal(sums[:, 2], want[:, 2]) and np.all(sums[:, 3] == 0), what
    for k in (0, 1):
        assert np.all(np.abs(sums[scored, k] - want[scored, k]) <= 1e-12 * np.abs(want[scored, k]) + 1e-300), (what, k)
    S = gain_scale(rec, gains, t0, first, .25, W_GAIN)
    pos = np.asarray(gains) > 0
    err = np.abs(gg.astype(np.float64) - np.where(pos, rg, 0.0))
    bound = ulp32(np.where(pos, rg, 0.0)) + K * 2.0 ** -52 * S
    assert np.all(err[pos] <= bound[pos]), (what, float(np.max((err - bound)[pos])))
    assert np.all(gg[~pos] == 0), what  # p <= 0: the header's rule, where the trainer's formula is infinite
    assert np.all(np.abs(gv.astype(np.float64) - rv) <= vad_bound(rec, vad, t0, first, W_VAD, rv)), what
    f_first = min(max(max(first, 1) - t0, 0), gains.shape[0])
    assert np.all(gg[:f_first] == 0) and np.all(gv[:f_first] == 0), what  # unscored steps: zeros
    if f_first < gains.shape[0]:
        g = rec[t0 + f_first - 1:t0 + gains.shape[0] - 1, :, FEATURES:FEATURES + BANDS]
        p = np.asarray(gains[f_first:]).astype(np.float64)
        exact = (g == -1.0) | ((g == 3.0) & (p == 3.0)) | (p == 0.0)  # a masked band, p = tg, p = 0
        assert exact.any() and np.all(gg[f_first:][exact] == 0), what
    return measured_k(gg, np.where(pos, rg, 0.0), S)
