"""The kernels of librnnoise_amd_fnet.so (rnnoise_amd/csrc/fnet/fnet.hip) through rnnoise_amd.fnet.FloatNetRuntime: against this
repository's own FloatNet (float64 on the CPU as the reference, float32 on the device as the yardstick of the error); bit-identical
under every cut of the frames into calls and pieces; rows alone; per-row reset; every layout with guard words; the host form; and
through the DSP (RNNoiseOp.denoise_with, cli denoise, cli eval-audio, tools/fnet_serve.c).

Shapes (tests/fnet_cases.py): (cond, gru) in (16, 16), (32, 48), (128, 384); 1, 15, 16, 17, 67 rows; 12 or 35 frames."""
import os
import subprocess

import numpy as np
import pytest

import fnet_cases as fc
from conftest import ROOT, load_blob
from rnnoise_amd import fnet, synth

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = fc.DEV

# e_fnet <= F * max(e_torch, 2^-23 max |X64|), errors against FloatNet.forward in float64 on the CPU, e_torch that of FloatNet.forward
# in float32 on the device.  Measured over the whole case set below (3 sizes x 5 row counts x 2 lengths, gains and vad, and frame 4
# against forward_sequence) and the DSP test, three runs: the largest ratio was 2.20 in each (128 / 384, gains of frame 4 against
# forward_sequence: e_fnet 1.460e-07 over a floor of 6.622e-08); the next sizes stay below 2.  F is twice that -- the rule: 2 x the
# largest measured ratio, at most 16.
MEASURED_RATIO = 2.20
F = 2 * MEASURED_RATIO


def _bits_equal(a, b, what):
    a, b = fc.u32(a), fc.u32(b)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} words differ"


def _x(n, t, seed=0):
    return fc.features(seed)[:n, :t].to(DEV)


# ---- 1. against FloatNet ----
@pytest.mark.parametrize("t", fc.FRAMES)
@pytest.mark.parametrize("n", fc.ROWS)
@pytest.mark.parametrize("cond,gru", fc.SIZES)
def test_against_float_net(cond, gru, n, t):
    x = _x(n, t)
    rt = fc.runtime(cond, gru)
    gains, vad = rt(x)
    net = fc.device_net(cond, gru)
    net.reset()
    with torch.no_grad():
        tg, tv = net(x)
        sg, sv = net.forward_sequence(x)
    g64, v64 = fc.x64(cond, gru, t)
    assert gains.shape == (n, t, 32) and vad.shape == (n, t, 1)
    # the first four frames after a reset: exact zeros
    assert not fc.u32(gains[:, :4]).any() and not fc.u32(vad[:, :4]).any()
    assert float(gains[:, 4:].min()) > 0 and float(vad[:, 4:].min()) > 0
    for name, got, other, want in (("gains", gains, tg, g64[:n]), ("vad", vad, tv, v64[:n])):
        r, e, floor = fc.ratio(got, other, want)
        print(f"\n[fnet] {cond}/{gru} N={n} T={t} {name}: e_fnet {e:.3e}, floor {floor:.3e}, ratio {r:.2f}")
        assert r <= F, (name, r)
    # frame 4 is forward_sequence's output 0
    q64 = fc.seq64(cond, gru, t)
    for name, got, other, want in (("gains", gains[:, 4], sg[:, 0], q64[0][:n, 0]), ("vad", vad[:, 4], sv[:, 0], q64[1][:n, 0])):
        r, e, floor = fc.ratio(got, other, want)
        print(f"[fnet] {cond}/{gru} N={n} T={t} {name} frame 4 against forward_sequence: e_fnet {e:.3e}, floor {floor:.3e}, ratio {r:.2f}")
        assert r <= F, (name, r)
    rt.close()


# ---- 2. cuts ----
@pytest.mark.parametrize("cond,gru,n", [(16, 16, 17), (32, 48, 67), (128, 384, 17)])
def test_cuts_give_the_same_bits(cond, gru, n):
    t = 35
    x = _x(n, t)
    want = None
    for max_frames, cuts in ((16, (35,)), (16, (35,)), (16, (1,) * 35), (16, (16, 1, 18)), (16, (2, 1, 32)), (1, (35,)), (2, (35,)), (2, (2, 1, 32)),
                             (1, (16, 1, 18)), (64, (35,))):
        rt = fc.runtime(cond, gru, max_frames)
        got = fc.run_cuts(rt, x, cuts)
        rt.close()
        if want is None:
            want = got
            assert float(want[0][:, 4:].std()) > 0
        _bits_equal(got[0], want[0], f"gains, max_frames {max_frames}, cuts {cuts[:4]}")
        _bits_equal(got[1], want[1], f"vad, max_frames {max_frames}, cuts {cuts[:4]}")


# ---- 3. rows are alone ----
@pytest.mark.parametrize("cond,gru", fc.SIZES)
def test_rows_are_alone(cond, gru):
    n, t = 67, 12
    x = _x(n, t)
    rt = fc.runtime(cond, gru)
    gains, vad = rt(x)
    for r in (0, 15, 16, 66):
        one = fc.runtime(cond, gru)
        g1, v1 = one(x[r:r + 1])
        one.close()
        _bits_equal(g1[0], gains[r], f"gains of row {r} alone")
        _bits_equal(v1[0], vad[r], f"vad of row {r} alone")
    # a NaN in one row's features from frame 5 on poisons that row from there, and no other
    bad = x.clone()
    bad[16, 5:] = float("nan")
    rt.reset()
    gb, vb = rt(bad)
    rt.close()
    keep = [r for r in range(n) if r != 16]
    _bits_equal(gb[keep], gains[keep], "gains of the other rows")
    _bits_equal(vb[keep], vad[keep], "vad of the other rows")
    _bits_equal(gb[16, :5], gains[16, :5], "gains of the row before the NaN")
    assert bool(torch.isnan(gb[16, 5:]).all()) and bool(torch.isnan(vb[16, 5:]).all())


# ---- 4. per-row reset ----
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("cond,gru", [(32, 48), (128, 384)])
def test_reset_rows(cond, gru, on_device):
    n, rows = 67, [0, 16, 66]
    first, second = _x(n, 10), _x(n, 12, seed=1)
    rt, twin, fresh = fc.runtime(cond, gru), fc.runtime(cond, gru), fc.runtime(cond, gru)
    rt(first), twin(first)
    rt.reset_rows(torch.tensor(rows, dtype=torch.int32, device=DEV) if on_device else rows)
    got = fc.run_cuts(rt, second, (3, 1, 8))
    never = fc.run_cuts(twin, second, (3, 1, 8))
    alone = fresh(second[rows].contiguous())
    others = [r for r in range(n) if r not in rows]
    for k, name in enumerate(("gains", "vad")):
        _bits_equal(got[k][rows], alone[k], f"{name} of the rows that were reset")
        assert not fc.u32(got[k][rows][:, :4]).any()
        _bits_equal(got[k][others], never[k][others], f"{name} of the rows that were not")
        assert not np.array_equal(fc.u32(got[k][rows][:, 4:]), fc.u32(never[k][rows][:, 4:]))
    for r in (rt, twin, fresh):
        r.close()


# ---- 5. layouts and guards ----
def _slots(total, off, fs, rs, t, n, w):
    m = np.zeros(total, bool)
    for f in range(t):
        for s in range(n):
            m[off + f * fs + s * rs: off + f * fs + s * rs + w] = True
    return m


@pytest.mark.parametrize("layout", ["default", "batch_first", "padded"])
def test_layouts_and_guards(layout):
    cond, gru, n, t, off = 32, 48, 17, 12, 7
    x = _x(n, t)
    rt = fc.runtime(cond, gru)
    want_g, want_v = rt(x)
    rt.reset()

    def strides(w):
        if layout == "default":
            return n * w, w
        if layout == "batch_first":
            return w, t * w
        return n * (w + 2) + 5, w + 2  # odd pitches: 67 / 34 / 3 floats a row, and five more a frame

    bufs, rows = {}, {}
    for name, w in (("feat", 65), ("gains", 32), ("vad", 1)):
        fs, rs = strides(w)
        total = off + (t - 1) * fs + (n - 1) * rs + w + 9
        buf = fc.filled(total)
        bufs[name], rows[name] = buf, (fs, rs, total, w)
        if name == "feat":
            torch.as_strided(buf, (n, t, w), (rs, fs, 1), off).copy_(x)
    at = lambda name: bufs[name].data_ptr() + 4 * off
    pass_rows = lambda name: None if layout == "default" else rows[name][:2]
    st = torch.cuda.current_stream(DEV).cuda_stream
    # n_frames 0 writes nothing, whatever the pointers are
    assert rt.process_device(0, None, 0, None, 0, None, 0, st) == 0
    assert rt.process_device(at("gains"), pass_rows("gains"), at("vad"), pass_rows("vad"), at("feat"), pass_rows("feat"), 0, st) == 0
    torch.cuda.synchronize()
    for name in ("gains", "vad"):
        assert (fc.u32(bufs[name]) == fc.FILL).all(), name
    assert rt.process_device(at("gains"), pass_rows("gains"), at("vad"), pass_rows("vad"), at("feat"), pass_rows("feat"), t, st) == 0
    torch.cuda.synchronize()
    for name, want in (("gains", want_g), ("vad", want_v)):
        fs, rs, total, w = rows[name]
        _bits_equal(torch.as_strided(bufs[name], (n, t, w), (rs, fs, 1), off), want, f"{name}, layout {layout}")
        words = fc.u32(bufs[name])
        assert (words[~_slots(total, off, fs, rs, t, n, w)] == fc.FILL).all(), f"{name}: a guard word changed"
    fs, rs, total, w = rows["feat"]
    assert (fc.u32(bufs["feat"])[~_slots(total, off, fs, rs, t, n, w)] == fc.FILL).all()
    # refusals, with nothing launched: NULL buffers, rows that overlap
    assert rt.process_device(0, None, at("vad"), None, at("feat"), None, t, st) == -1
    assert rt.process_device(at("gains"), (32, 16), at("vad"), None, at("feat"), None, t, st) == -1
    assert rt.process_device(at("gains"), None, at("vad"), None, at("feat"), (65, 64), t, st) == -1
    rt.close()


def test_host_form_in_two_pieces():
    cond, gru, n, t = 32, 48, 17, 12
    x = _x(n, t)
    rt = fc.runtime(cond, gru, max_frames=4)
    want_g, want_v = rt(x)
    rt.reset()
    torch.cuda.synchronize()
    h = np.ascontiguousarray(x.cpu().numpy().transpose(1, 0, 2))
    g1, v1 = rt.process_host(h[:7])
    g2, v2 = rt.process_host(h[7:])
    rt.close()
    got_g, got_v = np.concatenate([g1, g2]).transpose(1, 0, 2), np.concatenate([v1, v2]).T[:, :, None]
    assert np.array_equal(got_g.view(np.uint32), fc.u32(want_g)) and np.array_equal(np.ascontiguousarray(got_v).view(np.uint32), fc.u32(want_v))


def test_runtime_starts_over_when_the_rows_change():
    rt = fc.runtime(16, 16)
    a = rt(_x(3, 6))
    b = rt(_x(5, 6))  # another N: a new runtime, every row at the start of a sequence
    c = rt(_x(5, 6, seed=1))  # ... which then goes on
    assert not fc.u32(b[0][:, :4]).any() and float(c[0].min()) > 0 and a[0].shape == (3, 6, 32)
    rt.close()


# ---- 6. through the DSP ----
def test_through_the_dsp():
    from rnnoise_amd.torch_op import RNNoiseOp
    cond, gru = 128, 384
    streams, t = [3, 77, 130], 12
    pcm = torch.from_numpy(synth.batch_pcm(streams, t, lead_silence=2).astype(np.float32)).to(DEV)
    net, rt = fc.device_net(cond, gru), fc.runtime(cond, gru)
    net.reset()
    op = RNNoiseOp(load_blob("default"), len(streams), device=0)
    with torch.no_grad():
        feats, _ = op.analyze(pcm)
        op.synthesize(*net(feats), like=pcm)
        n64 = fc.copy.deepcopy(fc.net(cond, gru)).double()
        g64, v64 = n64(feats.cpu().double())
    net.reset(), op.reset()
    out_t = op.denoise_with(net, pcm)
    op.reset()
    out_n = op.denoise_with(rt, pcm)
    rt.reset(), net.reset()
    with torch.no_grad():
        g_n, v_n = rt(feats)
        g_t, v_t = net(feats)
    for name, got, other, want in (("gains", g_n, g_t, g64), ("vad", v_n, v_t, v64)):
        r, e, floor = fc.ratio(got, other, want)
        print(f"\n[fnet dsp] {name}: e_fnet {e:.3e}, floor {floor:.3e}, ratio {r:.2f}")
        assert r <= F, (name, r)
    # the PCM: a sample is a sum of band-interpolated gains times spectrum, so it moves by at most the largest gain difference
    # times the largest sample of the frames around it, overlap-add of two windows <= 1 each (x 2), pitch filter and the rounding of
    # the transforms aside (x 2 again)
    dg = float((g_n - g_t).abs().max())
    bound = 4 * dg * float(pcm.abs().max()) + 4 * float(np.spacing(np.float32(out_t.abs().max().item())))  # (and four ulps of the peak)
    d = float((out_n - out_t).abs().max())
    print(f"[fnet dsp] gains differ by {dg:.3e}, pcm by {d:.3e} (bound {bound:.3e}), pcm peak {float(out_t.abs().max()):.1f}")
    assert float(out_t.abs().max()) > 0 and d <= bound
    rt.close()


@pytest.fixture(scope="module")
def ckpt_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("fnet") / "small.pth"
    net = fc.net(32, 48)
    torch.save({"model_args": (), "model_kwargs": {"cond_size": 32, "gru_size": 48}, "state_dict": net.state_dict()}, path)
    return str(path)


def test_cli_denoise_and_eval_audio_native(ckpt_file, tmp_path, capsys):
    """a checkpoint of a size no blob holds, heard and scored through the native runtime"""
    from rnnoise_amd import cli
    from test_stoi_gpu import make_corpora
    blob = tmp_path / "default.blob"
    blob.write_bytes(load_blob("default"))
    streams, t = [3, 77], 12
    pcm = synth.batch_pcm(streams, t, lead_silence=1)
    files = []
    for i, s in enumerate(streams):
        files.append(str(tmp_path / f"s{s}.raw"))
        pcm[:, i].astype(np.int16).tofile(files[-1])
    out_dir = str(tmp_path / "out")
    cli.main(["denoise", "--checkpoint", ckpt_file, "--float-net", "native", "--model", str(blob), "--out-dir", out_dir] + files)
    assert "denoised 2 streams" in capsys.readouterr().out
    for f in files:
        a = np.fromfile(os.path.join(out_dir, os.path.basename(f) + ".denoised.raw"), np.int16)
        assert a.size == (t - 1) * 480 and (a[:3 * 480] == 0).all() and np.abs(a[4 * 480:].astype(np.int32)).max() > 0
    names = []
    for k, c in enumerate(make_corpora(40, 8)):
        names.append(str(tmp_path / f"c{k}.pcm"))
        c.tofile(names[-1])
    cli.main(["eval-audio", *names, "--model", str(blob), "--checkpoint", ckpt_file, "--float-net", "native", "--count", "2", "--frames", "40",
              "--seed", "21", "--streams", "2"])
    lines = capsys.readouterr().out.splitlines()
    row = [ln for ln in lines if ln.startswith(ckpt_file[-20:]) or ckpt_file in ln][0]
    numbers = [float(v) for v in row.replace(ckpt_file, "").split()]
    assert len(numbers) >= 8 and all(np.isfinite(v) for v in numbers), row


def test_the_c_example_runs(tmp_path):
    exe, blob = fc.build_c_example(str(tmp_path)), tmp_path / "default.blob"
    blob.write_bytes(load_blob("default"))
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert r.stdout.splitlines()[-1] == "ok"
