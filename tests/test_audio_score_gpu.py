"""GPU checks of the audio score library (include/rnnoise_amd_score.h): rn_audio_score_kernel against the numpy restatement of its
ORDER (tests/audio_score_ref.py) bit for bit -- every delay alignment, both layouts, ragged grids, cuts, ADD, untouched records,
non-finite rows, the host form --; evaluate_audio end to end on small generated sequences; and the 960-sample delay seen through the
score itself.  (What needs no device: tests/test_audio_score_cpu.py.)"""
import numpy as np
import pytest
import torch

import audio_score_ref as R
from conftest import assert_bits_equal, load_blob
from rnnoise_amd import audio_score as A
from rnnoise_amd import capi, evaluate, synth, train_data
from train_support import guarded, guards_intact

planes = R.planes

pytestmark = pytest.mark.gpu

T = 7
DELAYS = (0, 1, 479, 480, 960, 963)
CUTS = ([(0, 7)], [(t, 1) for t in range(7)], [(0, 2), (2, 1), (3, 4)])
DEV = "cuda:0"
u64 = lambda a: np.ascontiguousarray(a).view(np.uint64)


def first_of(D):
    return -(-D // 480)


def upload(p):
    """(flat, fs, rs) -> (device tensor, (pointer, fs, rs))"""
    d = torch.from_numpy(p[0]).to(DEV)
    assert d.data_ptr() % 16 == 0
    return d, (d.data_ptr(), p[1], p[2])


def run_device(dplanes, n_rows, D, cuts, sums0, ft0):
    """the device form over `cuts`, on guarded sums and records -> (sums, frame_terms) on the host"""
    sb, sv, sfill = guarded((n_rows, 8), torch.float64, -3.25)
    fb, fv, ffill = guarded((n_rows, T, 8), torch.float64, -3.25)
    sv.copy_(torch.from_numpy(sums0))
    fv.copy_(torch.from_numpy(ft0))
    for t0, n in cuts:
        A.score_device(sv.data_ptr(), *dplanes, n_rows, t0, n, first_of(D), D, fv.data_ptr(), T, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    guards_intact(sb, sfill, "sums")
    guards_intact(fb, ffill, "frame records")
    return sv.cpu().numpy(), fv.cpu().numpy()


@pytest.mark.parametrize("layout", ["frames", "streams"])
@pytest.mark.parametrize("n_rows", [1, 5, 64, 65, 513])
def test_kernel_is_the_restatement_bit_for_bit(n_rows, layout):
    rng = np.random.default_rng(1000 * n_rows + len(layout))
    host = planes(rng, n_rows, T, layout)
    keep = [upload(p) for p in host]
    dplanes = [k[1] for k in keep]
    views = [R.rows_view(*p, n_rows, T).transpose(1, 0, 2) for p in host]  # (T, N, 480) views for the host form
    for D in DELAYS:
        first = first_of(D)
        sums0 = rng.uniform(-1e6, 1e6, (n_rows, 8))  # the calls ADD
        ft0 = np.full((n_rows, T, 8), -11.0)         # sentinel: records outside the scored frames stay
        want, want_ft = sums0.copy(), ft0.copy()
        R.score(*host, n_rows, 0, T, first, D, want, want_ft)
        assert (want_ft[:, :first] == -11.0).all() and (want_ft[:, first:, 7] == 480).all()
        for cuts in CUTS:
            got, got_ft = run_device(dplanes, n_rows, D, cuts, sums0, ft0)
            assert_bits_equal(u64(got), u64(want), f"sums, D={D}, cuts={cuts}")
            assert_bits_equal(u64(got_ft), u64(want_ft), f"frame records, D={D}, cuts={cuts}")
        hs, hft = sums0.copy(), ft0.copy()
        A.score(*views, 0, T, first, D, hs, hft)  # the host form, staged through device memory
        assert_bits_equal(u64(hs), u64(want), f"host form sums, D={D}")
        assert_bits_equal(u64(hft), u64(want_ft), f"host form frame records, D={D}")
    # without frame records, and a call that scores nothing
    sv = torch.zeros((n_rows, 8), dtype=torch.float64, device=DEV)
    A.score_device(sv.data_ptr(), *dplanes, n_rows, 0, T, 2, 960)
    A.score_device(sv.data_ptr(), *dplanes, n_rows, 0, 2, 2, 960)
    A.score_device(sv.data_ptr(), *dplanes, n_rows, 3, 0, 2, 960)
    torch.cuda.synchronize()
    assert_bits_equal(u64(sv.cpu().numpy()), u64(R.score(*host, n_rows, 0, T, 2, 960, np.zeros((n_rows, 8)))), "no records")


def test_non_finite_rows_stay_alone():
    """5 rows: row 3 is +-3e38 throughout, row 4 holds one NaN -- its sums are NaN from that frame on, and no other row's bits move
    when the NaN is replaced by a number"""
    n_rows, D = 5, 960
    rng = np.random.default_rng(77)
    host = planes(rng, n_rows, T, "frames")
    zero, ft0 = np.zeros((n_rows, 8)), np.zeros((n_rows, T, 8))
    keep = [upload(p) for p in host]  # (the tensors live as long as their pointers are used)
    got, got_ft = run_device([k[1] for k in keep], n_rows, D, CUTS[0], zero, ft0)
    assert np.isnan(got[4, [2, 4, 6]]).all() and np.isfinite(got[4, [0, 1, 3, 5, 7]]).all() and np.isfinite(got[:4]).all()
    assert np.isnan(got_ft[4, T - 1, 2]) and np.isfinite(got_ft[4, :T - 1]).all()
    assert got[3, 0] > 1e79 and got[3, 6] > 1e79  # 480 * 5 * 9e76 and more: far beyond float32, nothing for a double
    clean = [(p[0].copy(), p[1], p[2]) for p in host]
    clean[2][0][np.isnan(clean[2][0])] = 1.0
    keep = [upload(p) for p in clean]
    again, again_ft = run_device([k[1] for k in keep], n_rows, D, CUTS[0], zero, ft0)
    assert_bits_equal(u64(again[:4]), u64(got[:4]), "the other rows' sums")
    assert_bits_equal(u64(again_ft[:4]), u64(got_ft[:4]), "the other rows' records")
    assert np.isfinite(again).all()


@pytest.mark.parametrize("D", DELAYS)
def test_an_output_that_is_the_delayed_clean_signal_has_no_error(D):
    n_rows = 5
    rng = np.random.default_rng(D)
    fs, rs = A.layout_frames(n_rows)
    ref = rng.uniform(-32768, 32767, (n_rows, T * 480)).astype(np.float32)
    noisy = (ref + rng.uniform(-500, 500, ref.shape)).astype(np.float32)
    out = np.zeros_like(ref)
    out[:, D:] = ref[:, :T * 480 - D]
    flat = lambda a: (np.ascontiguousarray(a.reshape(n_rows, T, 480).transpose(1, 0, 2)).reshape(-1), fs, rs)
    keep = [upload(flat(a)) for a in (ref, noisy, out)]
    got, _ = run_device([k[1] for k in keep], n_rows, D, CUTS[2], np.zeros((n_rows, 8)), np.zeros((n_rows, T, 8)))
    assert (got[:, 6] == 0.0).all() and not np.signbit(got[:, 6]).any() and (got[:, 5] > 0).all()
    assert_bits_equal(u64(got[:, 2]), u64(got[:, 0]), "y.y against r.r")
    assert_bits_equal(u64(got[:, 4]), u64(got[:, 0]), "y.r against r.r")
    m = A.metrics(got)
    assert np.isposinf(m["snr_out"]).all() and np.isposinf(m["si_sdr_out"]).all() and np.isfinite(m["snr_in"]).all()


# ---- end to end ----
SEQS, FRAMES = 9, 30


def make_corpora(frames, seed):
    """three int16 corpora a little longer than a sequence, as the training tests make theirs: loud speech with silences, two noises"""
    rng = np.random.default_rng(seed)
    span = 480 * frames
    lens = (span + 2001, span + 778, span + 1)
    env = np.repeat(rng.choice([0.0, 200.0, 6000.0, 20000.0], lens[0] // 240 + 1), 240)[:lens[0]]
    speech = np.clip(np.rint(rng.standard_normal(lens[0]) * env), -32768, 32767).astype(np.int16)
    noise = np.clip(np.rint(rng.standard_normal(lens[1]) * 3000), -32768, 32767).astype(np.int16)
    fg = np.clip(np.rint(rng.standard_normal(lens[2]) * 9000 * (rng.random(lens[2]) < .05)), -32768, 32767).astype(np.int16)
    return [speech, noise, fg]


@pytest.fixture(scope="module")
def passes():
    """evaluate_audio on 9 sequences of 30 frames: the default blob on batches of 4 (three rounds, the last partial) and of 3 streams,
    the little blob alone, and both blobs in one pass -- each with the planes of every round copied back"""
    corpora = [torch.from_numpy(c).to(DEV) for c in make_corpora(FRAMES, 31)]
    draws = train_data.draw(np.random.default_rng(99), SEQS, [c.numel() for c in corpora], FRAMES)
    blobs = dict(default=load_blob("default"), little=load_blob("little"))

    def run(names, streams):
        rounds = []
        tap = lambda s0, k, clean, noisy, outs: rounds.append((s0, k, clean.cpu().numpy(), noisy.cpu().numpy(), [o.cpu().numpy() for o in outs]))
        return evaluate.evaluate_audio(corpora, [blobs[n] for n in names], draws, FRAMES, streams=streams, tap=tap), rounds
    return dict(four=run(["default"], 4), three=run(["default"], 3), little=run(["little"], 4), both=run(["default", "little"], 4)), blobs


def test_evaluate_audio_does_not_depend_on_the_batch_size(passes):
    (four, rounds4), (three, rounds3) = passes[0]["four"], passes[0]["three"]
    assert [(s0, k) for s0, k, *_ in rounds4] == [(0, 4), (4, 4), (8, 1)] and [(s0, k) for s0, k, *_ in rounds3] == [(0, 3), (3, 3), (6, 3)]
    assert four[0]["sums"].shape == (SEQS, 8) and (four[0]["sums"][:, 7] == (FRAMES - 2) * 480).all()
    assert_bits_equal(u64(four[0]["sums"]), u64(three[0]["sums"]), "sums, 4 against 3 streams")
    assert_bits_equal(u64(four[0]["frame_terms"]), u64(three[0]["frame_terms"]), "frame records, 4 against 3 streams")
    assert np.array_equal(four[0]["active"], three[0]["active"]) and four[0]["sequences"] + four[0]["excluded"] == SEQS
    assert (four[0]["frame_terms"][:, :2] == 0).all()
    for key in A.SUMMARY_KEYS:
        assert four[0][key] == three[0][key] or (np.isnan(four[0][key]) and np.isnan(three[0][key])), key


def test_evaluate_audio_is_the_restatement_on_its_planes(passes):
    res, rounds = passes[0]["four"]
    N = 4
    fs, rs = A.layout_frames(N)
    for s0, k, clean, noisy, outs in rounds:
        assert clean.shape == noisy.shape == outs[0].shape == (FRAMES, N, 480)
        want, want_ft = np.zeros((k, 8)), np.zeros((k, FRAMES, 8))
        R.score(*[(a.reshape(-1), fs, rs) for a in (clean, noisy, outs[0])], k, 0, FRAMES, 2, A.DELAY, want, want_ft)
        assert_bits_equal(u64(res[0]["sums"][s0:s0 + k]), u64(want), f"sums of sequences {s0}..")
        assert_bits_equal(u64(res[0]["frame_terms"][s0:s0 + k]), u64(want_ft), f"frame records of sequences {s0}..")
    assert np.isfinite(res[0]["snr_in"]) and np.isfinite(res[0]["si_sdr_out"])


def test_evaluate_audio_scores_what_a_reset_batch_makes_of_the_noisy_plane(passes):
    (res, rounds), blobs = passes[0]["four"], passes[1]
    model = capi.Model(blobs["default"])
    for s0, k, _clean, noisy, outs in rounds:
        b = capi.Batch(model, noisy.shape[1])
        out, _vad, _gains = b.process(np.ascontiguousarray(noisy), want_gains=False)
        b.close()
        assert_bits_equal(out[:, :k], outs[0][:, :k], f"out plane of the round at sequence {s0}")
    model.close()


def test_two_blobs_in_one_pass_are_two_passes(passes):
    p = passes[0]
    both = p["both"][0]
    assert len(both) == 2
    for got, alone, name in ((both[0], p["four"][0][0], "default"), (both[1], p["little"][0][0], "little")):
        assert_bits_equal(u64(got["sums"]), u64(alone["sums"]), f"{name}: sums")
        assert_bits_equal(u64(got["frame_terms"]), u64(alone["frame_terms"]), f"{name}: frame records")
    assert not np.array_equal(both[0]["sums"][:, 2], both[1]["sums"][:, 2])  # (two different models were run)
    for a, b in zip(p["both"][1], p["four"][1]):  # the same planes in both passes
        assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


# ---- alignment ----
def test_the_score_is_best_at_a_delay_of_960_samples():
    """a net that passes everything (gains 1, VAD 1) leaves the DSP's own delay: scored against its input, the output is closest at
    960 samples -- no dB figure is asserted"""
    from rnnoise_amd.torch_op import RNNoiseOp
    streams, frames = [3, 77, 130], 24
    pcm = torch.from_numpy(synth.batch_pcm(streams, frames)).to(DEV)
    op = RNNoiseOp(load_blob("default"), len(streams))
    ones = lambda feats: (torch.ones((feats.shape[0], feats.shape[1], 32), device=feats.device),
                          torch.ones((feats.shape[0], feats.shape[1], 1), device=feats.device))
    out = op.denoise_with(ones, pcm).contiguous()
    assert out.shape == pcm.shape
    fs, rs = A.layout_frames(len(streams))
    si_sdr = {}
    for D in (0, 480, 959, 960, 961, 1440):
        sums = torch.zeros((len(streams), 8), dtype=torch.float64, device=DEV)
        A.score_device(sums.data_ptr(), (pcm.data_ptr(), fs, rs), (pcm.data_ptr(), fs, rs), (out.data_ptr(), fs, rs), len(streams), 0, frames, 3, D,
                       stream=torch.cuda.current_stream().cuda_stream)
        si_sdr[D] = A.metrics(sums.cpu().numpy())["si_sdr_out"]
    op.close()
    print({D: v.round(2).tolist() for D, v in si_sdr.items()})
    for D, v in si_sdr.items():
        if D != 960:
            assert (si_sdr[960] > v).all(), (D, si_sdr[960], v)


# ---- the command line ----
def test_cli_eval_audio_prints_a_blob_and_a_checkpoint(tmp_path, capsys):
    """eval-audio on generated sequences: the default blob and a seeded checkpoint through the float network, in process -- the blob's
    row holds evaluate_audio's means for the same seed, the checkpoint's row and the difference row are there"""
    import export_cases as xc
    from rnnoise_amd import cli
    frames, count = 12, 5
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
              "--seed", "21", "--streams", "2"])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith(f"eval-audio: {count} sequences of {frames} frames") and len(lines) == 5
    rows = [ln.split() for ln in lines[2:]]
    assert rows[0][0] == str(blob) and rows[1][0] == str(ckpt) and rows[2][:2] == ["d", str(ckpt)]
    dev_corpora = [torch.from_numpy(c).to(DEV) for c in corpora]
    draws = train_data.draw(np.random.default_rng(21), count, [len(c) for c in corpora], frames)
    want = evaluate.evaluate_audio(dev_corpora, [load_blob("default")], draws, frames, streams=5)[0]
    assert [int(rows[0][1]), int(rows[0][2])] == [want["sequences"], want["excluded"]]
    for got, key in zip(rows[0][3:], A.SUMMARY_KEYS):
        assert got == f"{want[key]:.3f}", key
    assert len(rows[1]) == 11 and len(rows[2]) == 10
