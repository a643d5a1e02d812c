"""librnnoise_amd_train.so on the device (include/rnnoise_amd_train.h): the two launches against rnnoise_batch_score_records_device
on the same buffers (sums bit for bit, in every cut), the gradients bit-identical across cuts and layouts and within the bound of
tests/train_loss_ref.py of the float64 torch reference, exact zeros where the header promises them, and nothing written beside the
outputs.  The measured K of the gain gradient's bound is printed by the last test: 0.987 on the case set and 0.000 on 10^5 random
cases on an MI355X, beside the host program's 0.990 and 0.000 (tests/test_train_loss_cpu.py); asserted is 4 x the larger, 3.96."""
import numpy as np
import pytest

import train_loss_ref as R
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

GUARD = 64  # elements of sentinel on either side of every output
FB = 16
ROWS = (1, 3, 67)
FRAMES = (1, FB - 1, FB, FB + 1, 2 * FB + 3)
LAYOUTS = ("frames", "rows", "padded")


@pytest.fixture(scope="module")
def dev():
    import torch
    from rnnoise_amd import blob as blob_tools
    from rnnoise_amd import capi
    from rnnoise_amd import train_loss as TL
    assert TL.FRAME_BLOCK == FB
    model = capi.Model(blob_tools.synth_model())  # (a score call reads no model: the batch only names the device)
    batch = capi.Batch(model, 1, device=0)
    yield dict(torch=torch, TL=TL, batch=batch, device=torch.device("cuda", 0))
    batch.close()
    model.close()


_cases, _first_layout = {}, {}


def cases(n_rows, n, t_base=4):
    """the case buffers of a shape with their reference, made once"""
    key = (n_rows, n, t_base)
    if key not in _cases:
        rec, gains, vad, _ = R.case_buffers(n_rows, n + t_base)
        _cases[key] = (rec, gains[t_base:], vad[t_base:])
    return _cases[key]


class Guarded:
    """a device tensor between two runs of sentinel; .t is the part in between"""

    def __init__(self, torch, device, shape, dtype, fill):
        n = int(np.prod(shape))
        self.fill = fill
        self.flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
        self.t = self.flat[GUARD:GUARD + n].view(*shape)

    def intact(self):
        return bool((self.flat[:GUARD] == self.fill).all() and (self.flat[-GUARD:] == self.fill).all())


def upload(d, view, guarded=False, fill=-3.0):
    """the memory of a (steps, rows, width) numpy view on the device as it lies -> (flat tensor or Guarded, pointer, strides, extent)"""
    torch = d["torch"]
    fs, rs = R.strides_of(view)
    n = (view.shape[0] - 1) * fs + (view.shape[1] - 1) * rs + view.shape[2]
    flat = np.lib.stride_tricks.as_strided(view, (n,), (view.itemsize,))
    if guarded:
        g = Guarded(torch, d["device"], (n,), torch.float32, fill)
        return g, g.t.data_ptr(), (fs, rs), n
    t = torch.from_numpy(np.array(flat)).to(d["device"])
    return t, t.data_ptr(), (fs, rs), n


def dense(flat_tensor, like):
    """a device buffer's (steps, rows, width) slots as a dense numpy array, through the strides of the numpy view `like`"""
    host = flat_tensor.cpu().numpy()
    return np.ascontiguousarray(np.lib.stride_tricks.as_strided(host, like.shape, like.strides))


def run(d, rec_l, gains_l, vad_l, t_base, first, cuts, sums0, grads=True, w=(R.W_GAIN, R.W_VAD)):
    """the library over `cuts` of buffers laid out as the views say -> sums, grad_gains, grad_vad (dense numpy), and what must stay
    untouched is checked on the way: the guards of every output and, where a buffer has gaps, the gaps"""
    torch, TL = d["torch"], d["TL"]
    n_rows, n = gains_l.shape[1], gains_l.shape[0]
    rec_t, rec_p, rec_s, _ = upload(d, rec_l)
    g_t, g_p, g_s, _ = upload(d, gains_l)
    v_t, v_p, v_s, _ = upload(d, vad_l)
    gg, gg_p, _, gg_n = upload(d, gains_l, guarded=True, fill=-7.0)
    gv, gv_p, _, gv_n = upload(d, vad_l, guarded=True, fill=-7.0)
    sums = Guarded(torch, d["device"], (n_rows, 4), torch.float64, -5.0)
    sums.t.copy_(torch.from_numpy(sums0))
    st = torch.cuda.current_stream().cuda_stream
    for t0, k in cuts:
        terms = Guarded(torch, d["device"], (n_rows, max(k, 1), 2), torch.float64, -9.0)
        df = t0 - t_base
        call = TL.make_call((rec_p, *rec_s), (g_p + 4 * df * g_s[0], *g_s), (v_p + 4 * df * v_s[0], *v_s), n_rows, t0, k, first, .25, w[0], w[1],
                            gg_p + 4 * df * g_s[0] if grads else 0, gv_p + 4 * df * v_s[0] if grads else 0)
        TL.loss_device(sums.t.data_ptr(), terms.t.data_ptr(), call, 0, st)
        torch.cuda.synchronize()
        assert terms.intact(), "frame terms: guard bytes"
    assert sums.intact() and gg.intact() and gv.intact(), "guard bytes"
    out_g, out_v = dense(gg.t, gains_l), dense(gv.t, vad_l)
    # the gaps of a padded gradient buffer still hold the fill
    for buf, like, got in ((gg, gains_l, out_g), (gv, vad_l, out_v)):
        host = buf.t.cpu().numpy().copy()
        np.lib.stride_tricks.as_strided(host, like.shape, like.strides)[...] = -7.0
        assert np.all(host == -7.0), "written between the slots"
    if not grads:
        assert np.all(out_g == -7.0) and np.all(out_v == -7.0), "gradients written without being asked for"
    return sums.t.cpu().numpy(), out_g, out_v[..., 0]


def score(d, rec_l, gains_l, vad_l, t_base, first, cuts, sums0):
    """rnnoise_batch_score_records_device over the same cuts of the same layouts -> sums"""
    torch = d["torch"]
    n_rows = gains_l.shape[1]
    rec_t, rec_p, rec_s, _ = upload(d, rec_l)
    g_t, g_p, g_s, _ = upload(d, gains_l)
    v_t, v_p, v_s, _ = upload(d, vad_l)
    sums = torch.from_numpy(sums0.copy()).to(d["device"])
    for t0, k in cuts:
        df = t0 - t_base
        d["batch"].score_records_device(sums.data_ptr(), 0, g_p + 4 * df * g_s[0], v_p + 4 * df * v_s[0], rec_p, n_rows, t0, k, gain_strides=g_s,
                                        vad_strides=v_s, rec_strides=rec_s, gamma=.25, first=first,
                                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def uneven(t0, n):
    """[t0, t0 + n) in calls of 1, about half, 0 and the rest"""
    a = min(1, n)
    b = (n - a) // 2
    return [(t0, a), (t0 + a, b), (t0 + a + b, 0), (t0 + a + b, n - a - b)]


def same_bits(a, b, what):
    assert_bits_equal(np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32),
                      np.ascontiguousarray(b).view(np.uint64 if b.dtype == np.float64 else np.uint32), what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_sums_are_the_score_calls_and_gradients_the_references(dev, n_rows, layout):
    rng = np.random.default_rng(n_rows)
    for n in FRAMES:
        rec, gains, vad = cases(n_rows, n)
        rec_l, gains_l, vad_l = R.lay_out(rec, layout), R.lay_out(gains, layout), R.lay_out(vad[..., None], layout)
        sums0 = rng.uniform(-1e3, 1e3, (n_rows, 4))
        sums0[:, 3] = 0
        what = f"{n_rows} rows x {n} steps, {layout}"
        whole = run(dev, rec_l, gains_l, vad_l, 4, 4, [(4, n)], sums0)
        same_bits(whole[0], score(dev, rec_l, gains_l, vad_l, 4, 4, [(4, n)], sums0), f"(a) sums, {what}")
        cut = run(dev, rec_l, gains_l, vad_l, 4, 4, uneven(4, n), sums0)
        same_bits(cut[0], score(dev, rec_l, gains_l, vad_l, 4, 4, uneven(4, n), sums0), f"(a) sums in uneven cuts, {what}")
        same_bits(cut[0], whole[0], f"(a) sums, cuts against one call, {what}")
        same_bits(cut[1], whole[1], f"(b) gain gradients across cuts, {what}")
        same_bits(cut[2], whole[2], f"(b) vad gradients across cuts, {what}")
        first = _first_layout.setdefault((n_rows, n), (layout, whole[1], whole[2]))
        same_bits(whole[1], first[1], f"(b) gain gradients, {layout} against {first[0]}, {what}")
        same_bits(whole[2], first[2], f"(b) vad gradients, {layout} against {first[0]}, {what}")
        zero = run(dev, rec_l, gains_l, vad_l, 4, 4, [(4, n)], np.zeros((n_rows, 4)))
        same_bits(zero[1], whole[1], f"gradients do not depend on the sums, {what}")
        R.check_against_reference(rec, gains, vad, 4, 4, zero[0], zero[1], zero[2], R.GRAD_K, f"(c), (d) {what}")  # (c), (d)
        only = run(dev, rec_l, gains_l, vad_l, 4, 4, [(4, n)], sums0, grads=False)  # (e)
        same_bits(only[0], whole[0], f"(e) sums without gradients, {what}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_unscored_steps_are_zeros_and_a_later_start_reads_the_record_before(dev, layout):
    n_rows, T = 3, 2 * FB + 3
    rec, gains, vad = cases(n_rows, T, 0)
    lay = lambda a: R.lay_out(a, layout)
    zeros = np.zeros((n_rows, 4))
    a = run(dev, lay(rec), lay(gains), lay(vad[..., None]), 0, 4, [(0, T)], zeros)  # t0 = 0, first = 4: four unscored steps
    assert np.all(a[1][:4] == 0) and np.all(a[2][:4] == 0) and np.all(a[0][:, 2] == T - 4)
    same_bits(a[0], score(dev, lay(rec), lay(gains), lay(vad[..., None]), 0, 4, [(0, T)], zeros), "sums, t0 = 0")
    R.check_against_reference(rec, gains, vad, 0, 4, *a, R.GRAD_K, "t0 = 0")
    b = run(dev, lay(rec), lay(gains[7:]), lay(vad[7:, :, None]), 7, 4, [(7, T - 7)], zeros)  # t0 = 7: reads record 6
    same_bits(b[0], score(dev, lay(rec), lay(gains[7:]), lay(vad[7:, :, None]), 7, 4, [(7, T - 7)], zeros), "sums, t0 = 7")
    same_bits(b[1], a[1][7:], "gain gradients of steps 7 .. from t0 = 7")
    same_bits(b[2], a[2][7:], "vad gradients of steps 7 .. from t0 = 7")
    R.check_against_reference(rec, gains[7:], vad[7:], 7, 4, *b, R.GRAD_K, "t0 = 7")
    cut = run(dev, lay(rec), lay(gains), lay(vad[..., None]), 0, 4, [(0, 2), (2, 5), (7, T - 7)], zeros)  # cuts through the unscored steps
    for k in range(3):
        same_bits(cut[k], a[k], "cuts through the unscored steps")
    # a call wholly below `first`: zeros in its gradients, nothing else anywhere
    c = run(dev, lay(rec), lay(gains), lay(vad[..., None]), 0, 9, [(0, 5)], np.ones((n_rows, 4)))
    assert np.all(c[0] == 1) and np.all(c[1][:5] == 0) and np.all(c[1][5:] == -7) and np.all(c[2][:5] == 0) and np.all(c[2][5:] == -7)


def test_host_form_gives_the_device_forms_numbers(dev):
    import ctypes as C
    TL = dev["TL"]
    n_rows, n = 3, FB + 1
    rec, gains, vad = cases(n_rows, n)
    want = run(dev, rec, gains, np.ascontiguousarray(vad[..., None]), 4, 4, [(4, n)], np.zeros((n_rows, 4)))
    gains_p = R.lay_out(gains, "padded")
    gg, gv = R.lay_out(np.full_like(gains, -7.0), "padded"), np.full((n, n_rows, 1), -7.0, np.float32)
    sums, terms = np.zeros((n_rows, 4)), np.full((n_rows, n, 2), -9.0)
    call = TL.make_call((rec.ctypes.data, *R.strides_of(rec)), (gains_p.ctypes.data, *R.strides_of(gains_p)), (vad.ctypes.data, n_rows, 1),
                        n_rows, 4, n, 4, .25, R.W_GAIN, R.W_VAD, gg.ctypes.data, gv.ctypes.data)
    dp = lambda a: a.ctypes.data_as(TL._dp)
    assert TL.lib().rnnoise_amd_train_loss(0, dp(sums), dp(terms), C.byref(call)) == 0
    same_bits(sums, want[0], "host form: sums")
    same_bits(np.ascontiguousarray(gg), want[1], "host form: gain gradients")
    same_bits(gv[..., 0], want[2], "host form: vad gradients")
    assert not np.any(terms == -9.0)  # (every step of this call is scored: each has its record)
    sums2 = np.zeros((n_rows, 4))
    call.grad_gains, call.grad_vad = None, None
    assert TL.lib().rnnoise_amd_train_loss(0, dp(sums2), None, C.byref(call)) == 0  # no frame terms, no gradients
    same_bits(sums2, want[0], "host form: sums only")


def test_measured_k_on_the_device(dev):
    """the case set's whole cross product and 10^5 random cases; prints what tests/test_train_loss_cpu.py's docstring records"""
    n_rows, T = 67, 2 * FB + 3 + 1
    rec, gains, vad, cover = R.case_buffers(n_rows, T)
    assert len(cover) == 420
    got = run(dev, rec, gains[1:], np.ascontiguousarray(vad[1:, :, None]), 1, 1, [(1, T - 1)], np.zeros((n_rows, 4)))
    k_set = R.check_against_reference(rec, gains[1:], vad[1:], 1, 1, *got, R.GRAD_K, "case set")
    rng = np.random.default_rng(11)
    rec, gains, vad = R.random_buffers(rng, 25, 126)
    got = run(dev, rec, gains[1:], np.ascontiguousarray(vad[1:, :, None]), 1, 1, [(1, 125)], np.zeros((25, 4)))
    want, rg, rv = R.reference(rec, gains[1:], vad[1:], 1, 1, .25, R.W_GAIN, R.W_VAD)
    S = R.gain_scale(rec, gains[1:], 1, 1, .25, R.W_GAIN)
    k_rand = R.measured_k(got[1], rg, S)
    print(f"measured K on the device: case set {k_set:.3f}, random {k_rand:.3f}; asserted {R.GRAD_K}")
    assert np.all(np.abs(got[1].astype(np.float64) - rg) <= R.ulp32(rg) + R.GRAD_K * 2.0 ** -52 * S)
    assert np.all(np.abs(got[2].astype(np.float64) - rv) <= R.vad_bound(rec, vad[1:], 1, 1, R.W_VAD, rv))
    assert max(k_set, k_rand) <= R.GRAD_K <= 64
