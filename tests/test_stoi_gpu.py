"""The kernels of librnnoise_amd_stoi.so (rnnoise_amd/csrc/stoi/stoi.hip) against the float64 restatement of their definition
(tests/stoi_ref.py): counts exactly, sums within a tolerance that comes from the restatement's own error; every layout, a missing noisy
plane, aliased planes, determinism, rows that are too short, silent or not finite, guard words, the host form; and
evaluate.evaluate_audio(stoi=True) and `cli eval-audio --stoi` end to end.

Shapes: 120-frame sequences (92 frames at 10 kHz, about half of them kept, 10 to 22 segments a row), five distinct signals tiled
over 1, 3 and 65 rows; first 0 with delay 0, and first 2 with delay 960 where the degraded planes are shifted by the delay."""
import numpy as np
import pytest
import torch

import stoi_ref as R
from conftest import assert_bits_equal, load_blob
from rnnoise_amd import evaluate, train_data
from rnnoise_amd import stoi as S
from train_support import guarded, guards_intact

pytestmark = pytest.mark.gpu

T = 120
SEEDS = 5
DEV = "cuda:0"
CONFIGS = ((0, 0), (2, 960))  # (first, delay)
SUMS = [0, 1, 4, 5]
u64 = lambda a: np.ascontiguousarray(a).view(np.uint64)


def shifted(x, delay):
    """x delayed by `delay` samples: what a denoiser with that delay would put out"""
    return np.concatenate([np.zeros(delay, np.float32), x[:x.size - delay]])


def make_planes(delay, rows=SEEDS):
    """(T, rows, 480) float32 planes ref, inp, out of distinct signals: inp at 5 dB (read at n - delay, as ref is), out at 20 dB and
    delayed"""
    ref = np.stack([R.make_signal(s, T) for s in range(rows)])
    inp = np.stack([R.degrade(ref[s], 5, 100 + s) for s in range(rows)])
    out = np.stack([shifted(R.degrade(ref[s], 20, 200 + s), delay) for s in range(rows)])
    return [np.ascontiguousarray(p.reshape(rows, T, 480).transpose(1, 0, 2)) for p in (ref, inp, out)]


@pytest.fixture(scope="module")
def base():
    """per (first, delay): the five base rows' planes, the reference's results and margins, the reference's own error e_ref and the
    tolerance of every sum.  Computed once and only read."""
    made = {}
    for first, delay in CONFIGS:
        planes = make_planes(delay)
        want, margins = R.score(*planes, T, first, delay)
        # the inputs are admissible only if no frame lies within 1e-6 dB of the silent-frame threshold
        assert (margins >= 1e-6).all(), margins
        assert (want[:, 7] >= 31).all() and len(set(want[:, 7])) >= 3, want[:, 7]  # segments in every row, distinct K
        other, _ = R.score(*planes, T, first, delay, fft="dft", descending=True)
        assert np.array_equal(other[:, [2, 3, 6, 7]], want[:, [2, 3, 6, 7]])
        e_ref = float(np.abs(other[:, SUMS] - want[:, SUMS]).max())
        tol = np.maximum(16 * e_ref, 1e-13 * np.abs(want[:, SUMS]))
        made[first, delay] = dict(planes=planes, want=want, e_ref=e_ref, tol=tol)
    return made


def tiled(a, n_rows, axis):
    return np.ascontiguousarray(np.take(a, np.arange(n_rows) % a.shape[axis], axis=axis))


def upload(planes, n_rows, layout="frames"):
    """(T, n_rows, 480) host planes on the device, laid out as `layout` -> (tensors, (pointer, frame_stride, row_stride) triples).
    Entries of `planes` that are the same object become the same device memory: aliased planes."""
    keep, at, seen = [], [], {}
    for p in planes:
        if id(p) not in seen:
            if layout == "frames":  # [T][N][480]
                d = torch.from_numpy(np.ascontiguousarray(p)).to(DEV)
                seen[id(p)] = (d.data_ptr(), n_rows * 480, 480)
            else:                   # stream-contiguous [N][T * 480 + pad]
                pad = 52
                rows = np.zeros((n_rows, p.shape[0] * 480 + pad), np.float32)
                rows[:, :p.shape[0] * 480] = p.transpose(1, 0, 2).reshape(n_rows, -1)
                d = torch.from_numpy(rows).to(DEV)
                seen[id(p)] = (d.data_ptr(), 480, p.shape[0] * 480 + pad)
            assert d.data_ptr() % 16 == 0
            keep.append(d)
        at.append(seen[id(p)])
    return keep, at


def run_triples(at, n_rows, first, delay, n_frames=T, with_in=True):
    """the device form on planes that lie on the device, as (pointer, frame_stride, row_stride) triples ref, inp, out; results and
    scratch between guard words -> (n_rows, 8)"""
    nbytes = S.workspace(n_rows, n_frames)
    assert nbytes == S.workspace_formula(n_rows, n_frames) and nbytes % 8 == 0
    rb, rv, rfill = guarded((n_rows, 8), torch.float64, -3.25)
    sb, sv, sfill = guarded((nbytes // 8,), torch.float64, -3.25)
    S.score_device(rv.data_ptr(), sv.data_ptr(), nbytes, at[0], at[1] if with_in else None, at[2], n_rows, n_frames, first, delay, 0,
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    guards_intact(rb, rfill, "results")
    guards_intact(sb, sfill, "scratch")
    return rv.cpu().numpy()


def run_device(planes, n_rows, first, delay, n_frames=T, layout="frames", with_in=True):
    """the device form on (T, n_rows, 480) host planes, laid out as `layout` -> (n_rows, 8)"""
    keep, at = upload(planes, n_rows, layout)
    got = run_triples(at, n_rows, first, delay, n_frames, with_in)
    del keep
    return got


def assert_close(got, b, n_rows, what):
    """counts exactly, sums within the tolerance, for rows that repeat the five base rows"""
    want, tol = tiled(b["want"], n_rows, 0), tiled(b["tol"], n_rows, 0)
    assert np.array_equal(got[:, [2, 3, 6, 7]], want[:, [2, 3, 6, 7]]), what
    err = np.abs(got[:, SUMS] - want[:, SUMS])
    print(f"{what}: e_ref {b['e_ref']:.3e}, largest error {err.max():.3e}, tolerance {tol.min():.3e} .. {tol.max():.3e}")
    assert (err <= tol).all(), (what, err.max(), b["e_ref"])


@pytest.mark.parametrize("first,delay", CONFIGS)
@pytest.mark.parametrize("n_rows", [1, 3, 65])
def test_counts_and_sums_against_the_reference(base, n_rows, first, delay):
    b = base[first, delay]
    got = run_device([tiled(p, n_rows, 1) for p in b["planes"]], n_rows, first, delay)
    assert_close(got, b, n_rows, f"{n_rows} rows, first {first}, delay {delay}")
    m = S.metrics(got)
    assert m["summary"]["sequences"] == n_rows and m["summary"]["excluded"] == 0
    assert ((m["stoi_in"] < m["stoi_out"]) & (m["stoi_out"] < 1) & (m["estoi_in"] < m["estoi_out"])).all()  # 5 dB against 20 dB


@pytest.mark.parametrize("first,delay", CONFIGS)
def test_layouts_give_identical_bits(base, first, delay):
    planes = [tiled(p, 3, 1) for p in base[first, delay]["planes"]]
    a, b = run_device(planes, 3, first, delay, layout="frames"), run_device(planes, 3, first, delay, layout="streams")
    assert_bits_equal(u64(a), u64(b), "[T][N][480] against [N][T * 480 + pad]")


def test_without_a_noisy_plane(base):
    b = base[2, 960]
    both, alone = run_device(b["planes"], SEEDS, 2, 960), run_device(b["planes"], SEEDS, 2, 960, with_in=False)
    assert (alone[:, :4] == 0).all() and not np.signbit(alone[:, :4]).any()
    assert_bits_equal(u64(alone[:, 4:]), u64(both[:, 4:]), "the out side with and without in")
    m = S.metrics(alone)
    assert np.isnan(m["stoi_in"]).all() and np.isnan(m["summary"]["estoi_in"]) and m["summary"]["sequences"] == SEEDS


def test_aliased_planes_score_one(base):
    """ref, in and out are the same device memory: one upload, one pointer three times"""
    b = base[0, 0]
    ref = b["planes"][0]
    keep, at = upload([ref, ref, ref], SEEDS)
    assert len(keep) == 1 and at[0] == at[1] == at[2]
    got = run_triples(at, SEEDS, 0, 0)
    segs = b["want"][:, 6]
    assert np.array_equal(got[:, 6], segs) and np.array_equal(got[:, 2], segs)
    for k in SUMS:
        assert (np.abs(got[:, k] - segs) <= np.maximum(16 * b["e_ref"], 1e-13 * segs)).all(), (k, got[:, k] - segs)
    # out alone aliasing ref, beside a noisy plane of its own: the out side scores one, the in side is the batch's
    keep, at = upload([ref, b["planes"][1], ref], SEEDS)
    assert len(keep) == 2 and at[0] == at[2] != at[1]
    got = run_triples(at, SEEDS, 0, 0)
    for k in (4, 5):
        assert (np.abs(got[:, k] - segs) <= np.maximum(16 * b["e_ref"], 1e-13 * segs)).all(), (k, got[:, k] - segs)
    assert (np.abs(got[:, :2] - b["want"][:, :2]) <= b["tol"][:, :2]).all() and np.array_equal(got[:, 2:4], b["want"][:, 2:4])


def test_a_long_row_takes_several_blocks_of_the_kept_list():
    """700 frames: 545 frames at 10 kHz, three blocks of 256 in the kept-list kernel's prefix sum, against the reference"""
    frames = 700
    ref = R.make_signal(11, frames)
    planes = [p.reshape(frames, 1, 480) for p in (ref, R.degrade(ref, 5, 111), shifted(R.degrade(ref, 20, 211), 960))]
    want, margins = R.score(*planes, frames, 2, 960)
    assert R.n_frames_10k(100 * (frames - 2)) == 544 and margins[0] >= 1e-6 and want[0, 7] > 256 and want[0, 6] == want[0, 7] - 30
    other, _ = R.score(*planes, frames, 2, 960, fft="dft", descending=True)
    e_ref = float(np.abs(other[:, SUMS] - want[:, SUMS]).max())
    got = run_device(planes, 1, 2, 960, n_frames=frames)
    assert np.array_equal(got[:, [2, 3, 6, 7]], want[:, [2, 3, 6, 7]])
    err, tol = np.abs(got[:, SUMS] - want[:, SUMS]), np.maximum(16 * e_ref, 1e-13 * np.abs(want[:, SUMS]))
    print(f"700 frames: kept {want[0, 7]:.0f}, e_ref {e_ref:.3e}, largest error {err.max():.3e}, tolerance {tol.min():.3e}")
    assert (err <= tol).all(), (err, tol)


def test_host_form_in_several_pieces():
    """100 rows of 400 frames are more than one 256 MiB piece of the host form (3.4 MB of PCM and scratch a row: 75 rows).  The rows
    are windows of one signal, 480 samples apart (frame stride 480, row stride 480 -- planes may overlap), so the planes stay small"""
    frames, rows = 400, 100
    assert 256 * 2 ** 20 // (3 * frames * 1920 + S.workspace(1, frames) + 64) < rows
    sig = R.make_signal(12, frames + rows)
    host = [sig, R.degrade(sig, 5, 112), R.degrade(sig, 20, 212)]
    views = [np.lib.stride_tricks.as_strided(h, (frames, rows, 480), (1920, 1920, 4), writeable=False) for h in host]
    assert all(v.ctypes.data % 16 == 0 for v in views)
    keep = [torch.from_numpy(h).to(DEV) for h in host]
    dev = run_triples([(d.data_ptr(), 480, 480) for d in keep], rows, 0, 0, n_frames=frames)
    assert (dev[:, 6] > 0).all() and len(set(dev[:, 4])) == rows  # every row scored, every row its own
    assert_bits_equal(u64(S.score(*views, frames, 0, 0)), u64(dev), "host form in two pieces against the device form")
    one = run_triples([(d.data_ptr() + 4 * 480 * 80, 480, 480) for d in keep], 1, 0, 0, n_frames=frames)
    assert_bits_equal(u64(one[0]), u64(dev[80]), "row 80 alone")


def test_two_runs_and_any_batch_give_the_same_bits(base):
    b = base[2, 960]
    planes = [tiled(p, 65, 1) for p in b["planes"]]
    one, two = run_device(planes, 65, 2, 960), run_device(planes, 65, 2, 960)
    assert_bits_equal(u64(one), u64(two), "two runs")
    alone = run_device([p[:, :1] for p in planes], 1, 2, 960)
    assert_bits_equal(u64(alone[0]), u64(one[0]), "row 0 alone against row 0 of 65")
    assert_bits_equal(u64(one[:60]), u64(np.tile(one[:5], (12, 1))), "equal rows, wherever they lie in the batch")


def test_edge_rows_stay_alone(base):
    """rows 5..8 beside the five healthy ones: a 45-frame sequence followed by digital silence (fewer than 31 kept frames), an
    all-zero ref (every frame is kept, every term is 0.0), a NaN sample in out, a NaN sample in ref"""
    b = base[0, 0]
    healthy = run_device(b["planes"], SEEDS, 0, 0)
    ref, inp, out = (np.concatenate([p, p[:, :4]], axis=1) for p in b["planes"])
    for p in (ref, inp, out):
        p[45:, 5] = 0
    ref[:, 6] = 0
    out[60, 7, 17] = np.nan
    ref[60, 8, 17] = np.nan
    want, _ = R.score(ref[:, 5:7], inp[:, 5:7], out[:, 5:7], T, 0, 0)
    assert 0 < want[0, 7] < 31 and want[0, 6] == 0 and want[1, 7] == 92 and want[1, 6] == 62 and (want[:, SUMS] == 0).all()
    got = run_device([ref, inp, out], SEEDS + 4, 0, 0)
    assert_bits_equal(u64(got[:SEEDS]), u64(healthy), "the healthy rows beside the edge rows")
    assert_bits_equal(u64(got[5:7]), u64(want), "the short and the silent row")
    # a NaN in out: the out side of its row is NaN, its in side is the healthy row's (row 7 repeats row 2)
    assert np.isnan(got[7, 4]) and np.isnan(got[7, 5]) and np.array_equal(got[7, [6, 7]], healthy[2, [6, 7]])
    assert_bits_equal(u64(got[7, :4]), u64(healthy[2, :4]), "the in side of the row with a NaN in out")
    # a NaN in ref: the maximum of the frame norms is NaN, no frame is kept
    assert (got[8] == 0).all()
    m = S.metrics(got)
    assert m["summary"]["sequences"] == SEEDS + 2 and m["summary"]["excluded"] == 2 and np.isnan(m["summary"]["stoi_out"])


def test_sequences_too_short_for_a_frame_or_a_segment():
    """n_frames - first of 0, 2 (200 samples at 10 kHz: no frame), 3 (one frame) and 40 (no segment): zeros, and the kept frames"""
    for n_frames, first in ((2, 2), (2, 0), (3, 0), (40, 0)):
        planes = [p[:n_frames] for p in make_planes(0, 2)]
        got = run_device(planes, 2, first, 0, n_frames=n_frames)
        want, _ = R.score(*planes, n_frames, first, 0)
        assert_bits_equal(u64(got), u64(want), f"{n_frames} frames from {first}")
        assert (got[:, SUMS] == 0).all() and (got[:, 6] == 0).all()


def test_host_form_gives_the_device_forms_doubles(base):
    for (first, delay), b in base.items():
        planes = [tiled(p, 7, 1) for p in b["planes"]]
        dev = run_device(planes, 7, first, delay)
        assert_bits_equal(u64(S.score(*planes, T, first, delay)), u64(dev), "host form")
        views = [np.ascontiguousarray(p.transpose(1, 0, 2)).transpose(1, 0, 2) for p in planes]  # stream-contiguous memory
        assert_bits_equal(u64(S.score(views[0], None, views[2], T, first, delay))[:, 4:], u64(dev)[:, 4:], "host form, no noisy plane")
        tensors = [torch.from_numpy(p).to(DEV) for p in planes]
        slabs = S.score(*tensors, T, first, delay, scratch_cap=3 * S.workspace(1, T))  # three slabs: 3 + 3 + 1 rows
        assert_bits_equal(u64(slabs), u64(dev), "score() on device tensors, in slabs")


def make_corpora(frames, seed):
    """three int16 corpora a little longer than a sequence: loud speech with silences, two noises"""
    rng = np.random.default_rng(seed)
    span = 480 * frames
    lens = (span + 2001, span + 778, span + 1)
    env = np.repeat(rng.choice([0.0, 200.0, 6000.0, 20000.0], lens[0] // 240 + 1), 240)[:lens[0]]
    speech = np.clip(np.rint(rng.standard_normal(lens[0]) * env), -32768, 32767).astype(np.int16)
    noise = np.clip(np.rint(rng.standard_normal(lens[1]) * 3000), -32768, 32767).astype(np.int16)
    fg = np.clip(np.rint(rng.standard_normal(lens[2]) * 9000 * (rng.random(lens[2]) < .05)), -32768, 32767).astype(np.int16)
    return [speech, noise, fg]


def test_evaluate_audio_with_stoi():
    frames, seqs = 80, 3
    corpora = [torch.from_numpy(c).to(DEV) for c in make_corpora(frames, 31)]
    draws = train_data.draw(np.random.default_rng(99), seqs, [c.numel() for c in corpora], frames)
    rounds = []
    tap = lambda s0, k, clean, noisy, outs: rounds.append((s0, k, clean.clone(), noisy.clone(), [o.clone() for o in outs]))
    blob = load_blob("default")
    res = evaluate.eval_audio(corpora, [blob, blob], draws, frames, streams=2, tap=tap, stoi=True)
    plain = evaluate.evaluate_audio(corpora, [blob], draws, frames, streams=2)[0]
    assert not [k for k in plain if "stoi" in k]
    for r in res:
        assert set(S.METRIC_KEYS) <= set(r) and r["stoi_results"].shape == (seqs, 8)
        assert_bits_equal(u64(r["sums"]), u64(plain["sums"]), "the waveform sums beside STOI")
        assert all(np.isfinite(r[k]) for k in S.METRIC_KEYS), {k: r[k] for k in S.METRIC_KEYS}
        assert 0 < r["stoi_in"] <= 1 and 0 < r["stoi_out"] <= 1
        assert r["stoi_per_sequence"]["summary"]["sequences"] == seqs and (r["stoi_results"][:, 6] > 0).all()
    # the second denoiser reuses the first one's noisy side
    assert_bits_equal(u64(res[1]["stoi_results"]), u64(res[0]["stoi_results"]), "the same blob twice")
    assert [(s0, k) for s0, k, *_ in rounds] == [(0, 2), (2, 1)]
    for s0, k, clean, noisy, outs in rounds:
        for r, out in zip(res, outs):
            want = S.score(clean[:, :k], noisy[:, :k], out[:, :k], frames, 2, 960)
            assert_bits_equal(u64(r["stoi_results"][s0:s0 + k]), u64(want), f"sequences {s0}..{s0 + k - 1}")
    m = S.metrics(res[0]["stoi_results"])
    assert res[0]["stoi_out"] == m["summary"]["stoi_out"] and res[0]["estoi_in"] == m["summary"]["estoi_in"]


def test_cli_eval_audio_stoi_prints_a_blob_and_a_checkpoint(tmp_path, capsys):
    """eval-audio --stoi on generated sequences, in process: the default blob and a seeded checkpoint through the float network --
    four more columns, the blob's holding evaluate_audio(stoi=True)'s means for the same seed; both rows share the noisy side"""
    import export_cases as xc
    from rnnoise_amd import cli
    frames, count = 80, 3
    corpora = make_corpora(frames, 8)
    names = []
    for k, c in enumerate(corpora):
        names.append(str(tmp_path / f"c{k}.pcm"))
        c.tofile(names[-1])
    blob = tmp_path / "default.blob"
    blob.write_bytes(load_blob("default"))
    ckpt = tmp_path / "seeded.pth"
    torch.save({"model_args": (), "model_kwargs": {"cond_size": 128, "gru_size": 384}, "state_dict": dict(xc.pruned_blob()[0])}, ckpt)
    cli.main(["eval-audio", *names, "--model", str(blob), "--checkpoint", str(ckpt), "--count", str(count), "--frames", str(frames),
              "--seed", "21", "--streams", "2", "--stoi"])
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 5 and lines[1].split()[-8:] == ["STOI", "in", "STOI", "out", "ESTOI", "in", "ESTOI", "out"]
    rows = [ln.split() for ln in lines[2:]]
    assert rows[0][0] == str(blob) and rows[1][0] == str(ckpt) and rows[2][:2] == ["d", str(ckpt)]
    assert len(rows[0]) == 15 and len(rows[1]) == 15 and len(rows[2]) == 14
    dev_corpora = [torch.from_numpy(c).to(DEV) for c in corpora]
    draws = train_data.draw(np.random.default_rng(21), count, [len(c) for c in corpora], frames)
    want = evaluate.evaluate_audio(dev_corpora, [load_blob("default")], draws, frames, streams=3, stoi=True)[0]
    assert rows[0][-4:] == [f"{want[k]:.3f}" for k in ("stoi_in", "stoi_out", "estoi_in", "estoi_out")]
    assert rows[1][-4] == rows[0][-4] and rows[1][-2] == rows[0][-2] and float(rows[2][-4]) == 0.0  # one noisy side for both
    assert all(0 < float(v) <= 1 for v in rows[0][-4:] + rows[1][-4:])
