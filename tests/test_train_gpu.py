"""Training on the device (rnnoise_amd/train.py, train_loss.py): the autograd function against the library's own gradients and against
evaluate's means, the device form of the record generator against generate_rounds, and the loop itself -- a descent, a sparsified run
and an online epoch whose checkpoint the exporter takes."""
import numpy as np
import pytest
import torch

import train_loss_ref as R
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def u32(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def tensors():
    """5 sequences of 23 records on the device with predictions of steps 4 .. 22 that came out of a small float network"""
    from rnnoise_amd import train
    records = torch.from_numpy(R.training_records(np.random.default_rng(6), 5, 23)).to(DEV)
    net = train.new_network(8, 16, seed=3).to(DEV)
    with torch.no_grad():
        gains, vad = net.forward_sequence(records[:, :, :R.FEATURES])
    return records, gains.contiguous(), vad.contiguous()


def test_trainer_loss_backward_is_the_librarys_gradient_times_the_incoming_scalar(tensors):
    from rnnoise_amd import train_loss as TL
    records, gains, vad = tensors
    _, gg, gv = TL.loss_and_grad(records, gains, vad, 4, 4, .25)
    for scale in (1.0, 3.0, -.37):
        g, v = gains.clone().requires_grad_(True), vad.clone().requires_grad_(True)
        loss, gain_loss, vad_loss = TL.TrainerLoss.apply(g, v, records, 4, 4, .25)
        assert loss.dtype == torch.float64 and loss.requires_grad and not gain_loss.requires_grad and not vad_loss.requires_grad
        (loss * scale).backward()
        s = torch.tensor(scale, dtype=torch.float64, device=DEV).to(torch.float32)
        assert_bits_equal(u32(g.grad), u32(gg * s), f"gain gradients x {scale}")
        assert_bits_equal(u32(v.grad), u32(gv * s), f"vad gradients x {scale}")
    assert g.grad.shape == gains.shape and v.grad.shape == vad.shape and float(gg.abs().max()) > 0 and float(gv.abs().max()) > 0
    # the gradient is the reference's: the trainer's means are the library's default weights
    rec, p, q = records.cpu().numpy().transpose(1, 0, 2), gains.cpu().numpy().transpose(1, 0, 2), vad.cpu().numpy()[..., 0].T
    F = 5 * 19
    _, rg, rv = R.reference(rec, p, q, 4, 4, .25, 1 / (32 * F), .001 / F)
    S = R.gain_scale(rec, p, 4, 4, .25, 1 / (32 * F))
    got_g, got_v = gg.cpu().numpy().transpose(1, 0, 2).astype(np.float64), gv.cpu().numpy()[..., 0].T.astype(np.float64)
    assert np.all(np.abs(got_g - rg) <= R.ulp32(rg) + R.GRAD_K * 2.0 ** -52 * S)
    assert np.all(np.abs(got_v - rv) <= R.vad_bound(rec, q, 4, 4, .001 / F, rv))


def test_trainer_loss_forward_is_evaluates_means_of_score_records(tensors):
    from rnnoise_amd import blob as blob_tools
    from rnnoise_amd import capi
    from rnnoise_amd import train_loss as TL
    records, gains, vad = tensors
    n, K, T = gains.shape[0], gains.shape[1], records.shape[1]
    model = capi.Model(blob_tools.synth_model())
    batch = capi.Batch(model, 1, device=0)
    sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=DEV)
    batch.score_records_device(sums.data_ptr(), 0, gains.data_ptr(), vad.data_ptr(), records.data_ptr(), n, 4, K, gain_strides=(32, K * 32),
                               vad_strides=(1, K), rec_strides=(98, T * 98), gamma=.25, first=4,
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = capi.eval_losses(sums.cpu().numpy())
    batch.close()
    model.close()
    loss, gain_loss, vad_loss = TL.TrainerLoss.apply(gains, vad, records, 4, 4, .25)
    assert (float(loss), float(gain_loss), float(vad_loss)) == (want["loss"], want["gain_loss"], want["vad_loss"])
    assert want["frames_scored"] == n * K and np.isfinite(want["loss"]) and want["loss"] > 0
    # ... and the float32 torch formula agrees to float precision: the same loss, other arithmetic
    ref = R.trainer_loss(gains, vad, records[:, 3:-1, 65:97], records[:, 3:-1, 97:])
    assert float(ref[0]) == pytest.approx(want["loss"], rel=1e-4)


def corpora(frames):
    from rnnoise_amd import synth
    return [synth.stream_pcm(s, frames + extra).reshape(-1) for s, extra in ((3, 5), (77, 2), (130, 1))]


def test_generate_rounds_device_gives_the_bytes_of_generate_rounds(blob_default):
    from rnnoise_amd import capi, train_data
    frames, count, N = 9, 5, 2
    host = corpora(frames)
    dev = [torch.from_numpy(c).to(DEV) for c in host]
    draws = train_data.draw(np.random.default_rng(12), count, [len(c) for c in host], frames)
    model = capi.Model(blob_default)
    got = []
    for fn in (train_data.generate_rounds, train_data.generate_rounds_device):
        b = capi.Batch(model, N, device=0)
        with torch.cuda.device(DEV):
            rounds = list(fn(b, *dev, draws, frames)) if fn is train_data.generate_rounds else \
                [rec.permute(1, 0, 2)[:k].contiguous().cpu().numpy() for k, rec in fn(b, *dev, draws, frames)]
        b.close()
        got.append(rounds)
    model.close()
    assert [r.shape for r in got[0]] == [(2, frames, 98), (2, frames, 98), (1, frames, 98)] == [r.shape for r in got[1]]
    for a, b in zip(*got):
        assert_bits_equal(a.view(np.uint32), b.view(np.uint32), "records of a round")
    with torch.cuda.device(DEV):  # the device form: the generator's own [frame][stream][98] tensor, strides (N * 98, 98)
        b = capi.Batch(capi.Model(blob_default), N, device=0)
        k, rec = next(iter(train_data.generate_rounds_device(b, *dev, draws, frames)))
        assert k == N and rec.is_cuda and rec.shape == (frames, N, 98) and rec.stride() == (N * 98, 98, 1)
        b.close()


def test_fit_descends_on_the_device(tmp_path):
    """the setup tests/test_train_cpu.py shows descending with the reference loss, here with the library's"""
    from rnnoise_amd import float_net, train
    records = R.training_records(np.random.default_rng(3), 8, 36)
    steps = []
    hist = train.fit(train.RecordFile(records, 36, 8), str(tmp_path), epochs=40, cond_size=16, gru_size=32, seed=7,
                     on_step=lambda info: steps.append(info["loss"]), log=None)
    assert len(steps) == 40 and np.all(np.isfinite(steps)) and steps[-1] < steps[0], (steps[0], steps[-1])
    net = float_net.load_checkpoint(hist[-1]["checkpoint"])
    assert (net.cond_size, net.gru_size) == (16, 32)


def test_sparse_run_ends_at_the_target_densities(tmp_path):
    from rnnoise_amd import train
    records = R.training_records(np.random.default_rng(4), 4, 12)
    did = []
    hist = train.fit(train.RecordFile(records, 12, 4), str(tmp_path), epochs=7, cond_size=8, gru_size=16, seed=1,
                     sparse=train.SparsifySchedule(start=2, stop=6, interval=2), on_step=lambda info: did.append(info["sparsified"]), log=None)
    assert did == [False, True, False, True, False, True, True]
    sd = torch.load(hist[-1]["checkpoint"], map_location="cpu")["state_dict"]
    for k in (1, 2, 3):
        for side in ("ih", "hh"):
            W = sd[f"gru{k}.weight_{side}_l0"]
            for gate, target in enumerate((.3, .2, .5)):
                m = W[gate * 16:(gate + 1) * 16]
                rest = m - torch.diag(torch.diag(m)) if side == "hh" else m
                blocks = (rest.reshape(2, 8, 4, 4) != 0).any(3).any(1)
                assert int(blocks.sum()) == round(8 * target), (k, side, gate)
                if side == "hh":
                    assert torch.all(torch.diag(m) != 0), (k, gate)


def test_an_online_epoch_writes_a_checkpoint_the_exporter_takes(tmp_path, capsys):
    from rnnoise_amd import blob as blob_tools
    from rnnoise_amd import cli
    frames = 12
    names = []
    for k, c in enumerate(corpora(frames)):
        names.append(str(tmp_path / f"c{k}.pcm"))
        c.tofile(names[-1])
    out = tmp_path / "run"
    cli.main(["train", str(out), "--online", *names, "--sequences-per-epoch", "2", "--batch-size", "2", "--sequence-length", str(frames),
              "--epochs", "1", "--seed", "5"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("epoch 1: loss ") and "gain_loss" in line and "vad_loss" in line and "(1 batches, step 1)" in line
    assert np.isfinite(float(line.split()[3]))
    ckpt = out / "checkpoints" / "rnnoise_1.pth"
    assert ckpt.exists()
    cli.main(["export", str(ckpt), str(tmp_path / "net.blob")])
    data = (tmp_path / "net.blob").read_bytes()
    assert data[:4] == b"DNNw" and len(data) > 1 << 20 and len(blob_tools.read_blob(data)) == 43
