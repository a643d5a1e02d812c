"""CPU checks of rnnoise_amd/train.py: the loop driven with the reference loss injected (tests/train_loss_ref.py: plain torch, so
nothing here needs a device), its checkpoints, its learning rate and its carried states; the sparsifier's schedule against the
reference's GRUSparsifier where the reference is mounted; and the `train` command's arguments.  (The loop with the library's loss:
tests/test_train_gpu.py.)"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import train_loss_ref as R
from rnnoise_amd import cli, float_net, train

REFERENCE = os.environ.get("RNNOISE_REFERENCE", "/root/reference")


def injected_loss(gains, vad, records, gamma):
    """train_rnnoise.py:147-156: the targets cut as [:, 3:-1], the trainer's three means"""
    return R.trainer_loss(gains, vad, records[:, 3:-1, R.FEATURES:R.FEATURES + R.BANDS], records[:, 3:-1, R.REC - 1:], gamma)


def test_fit_carries_states_writes_the_references_checkpoint_and_decays_the_rate(tmp_path, monkeypatch):
    records = R.training_records(np.random.default_rng(1), 4, 12)
    seen, steps = [], []
    forward = float_net.FloatNet.forward_sequence

    def spy(self, features, states=None, return_states=False):
        seen.append(states)
        return forward(self, features, states, return_states)
    monkeypatch.setattr(float_net.FloatNet, "forward_sequence", spy)
    lines = []
    hist = train.fit(train.RecordFile(records, 12, 4), str(tmp_path), epochs=3, cond_size=8, gru_size=16, suffix="_t", seed=5,
                     loss=injected_loss, device="cpu", on_step=lambda info: steps.append(info), log=lines.append)
    assert len(hist) == len(steps) == len(lines) == 3 and [s["step"] for s in steps] == [1, 2, 3]
    # states: none at the start, then those the step before left, detached
    assert seen[0] is None
    for k in (1, 2):
        assert len(seen[k]) == 3
        for got, left in zip(seen[k], steps[k - 1]["states"]):
            assert got is left and not got.requires_grad and got.grad_fn is None and got.shape == (1, 4, 16)
    assert not torch.equal(steps[0]["states"][0], steps[1]["states"][0])
    # the learning rate a step is taken with: lr / (1 + decay * steps before it)
    assert [s["lr"] for s in steps] == pytest.approx([1e-3 / (1 + 5e-5 * x) for x in range(3)], rel=1e-15)
    # the checkpoints: the reference's keys and names, loadable as they are
    for epoch, h in enumerate(hist, 1):
        assert h["checkpoint"] == str(tmp_path / "checkpoints" / f"rnnoise_t_{epoch}.pth") and os.path.exists(h["checkpoint"])
        ck = torch.load(h["checkpoint"], map_location="cpu")
        assert set(ck) == {"model_args", "model_kwargs", "state_dict", "loss", "epoch"}
        assert ck["model_args"] == () and ck["model_kwargs"] == {"cond_size": 8, "gru_size": 16} and ck["epoch"] == epoch
        assert ck["loss"] == h["loss"] == steps[epoch - 1]["loss"]  # (one batch per epoch: its mean is the step's loss)
        assert list(ck["state_dict"]) == list(float_net.FloatNet(8, 16).state_dict())
        assert f"epoch {epoch}: loss {h['loss']:.6f} gain_loss {h['gain_loss']:.6f} vad_loss {h['vad_loss']:.6f}" in lines[epoch - 1]
    net = float_net.load_checkpoint(hist[-1]["checkpoint"])
    assert (net.cond_size, net.gru_size) == (8, 16) and not net.training
    g, v = net.forward_sequence(torch.from_numpy(records[:, :, :R.FEATURES]))
    assert g.shape == (4, 8, 32) and v.shape == (4, 8, 1)
    assert h["loss"] == pytest.approx(h["gain_loss"] + .001 * h["vad_loss"], rel=1e-6)
    # a second run from the last checkpoint starts where it stopped
    first = []
    train.fit(train.RecordFile(records, 12, 4), str(tmp_path / "again"), epochs=1, cond_size=8, gru_size=16, seed=5, loss=injected_loss,
              device="cpu", initial_checkpoint=hist[-1]["checkpoint"], on_step=lambda info: first.append(info), log=None)
    with torch.no_grad():
        want = injected_loss(g, v, torch.from_numpy(records), .25)[0]
    assert first[0]["loss"] == pytest.approx(float(want), rel=1e-5)


def test_record_file_shuffles_whole_batches_and_drops_the_rest():
    records = R.training_records(np.random.default_rng(2), 7, 6)
    data = train.RecordFile(records.reshape(-1), 6, 3)
    assert len(data) == 2
    a = [rec.numpy() for _, rec in data.batches(np.random.default_rng(9), "cpu")]
    b = [rec.numpy() for _, rec in data.batches(np.random.default_rng(9), "cpu")]
    assert len(a) == 2 and all(np.array_equal(x, y) for x, y in zip(a, b))  # seeded
    rows = np.concatenate(a)
    assert rows.shape == (6, 6, 98)
    ids = [int(np.flatnonzero([np.array_equal(r, s) for s in records])[0]) for r in rows]
    assert len(set(ids)) == 6  # six of the seven sequences, each once
    for feats, rec in data.batches(np.random.default_rng(9), "cpu"):
        assert feats.is_contiguous() and torch.equal(feats, rec[:, :, :65])
    with pytest.raises(ValueError):
        train.RecordFile(records, 6, 8)


def test_the_gpu_tests_setup_descends_with_the_injected_loss(tmp_path):
    """8 fixed sequences x 36 frames, cond_size 16, gru_size 32, one batch, 40 steps: what tests/test_train_gpu.py trains with the
    library's loss descends with the reference's, so a failure there is not the setup's"""
    records = R.training_records(np.random.default_rng(3), 8, 36)
    steps = []
    train.fit(train.RecordFile(records, 36, 8), str(tmp_path), epochs=40, cond_size=16, gru_size=32, seed=7, loss=injected_loss, device="cpu",
              on_step=lambda info: steps.append(info["loss"]), log=None)
    assert len(steps) == 40 and steps[-1] < steps[0] and steps[-1] < .9 * steps[0], (steps[0], steps[-1])


# ---- the sparsifier ----
def test_density_formula_at_start_middle_and_stop():
    s = train.SparsifySchedule(start=2, stop=8, interval=2)
    assert s.densities(1) is None and s.densities(3) is None and s.densities(5) is None
    assert s.densities(2) == (1.0, 1.0, 1.0)  # alpha = 1 at the start: everything survives
    alpha = ((8 - 4) / (8 - 2)) ** 3
    assert s.densities(4) == pytest.approx(tuple(alpha + (1 - alpha) * t for t in (.3, .2, .5)), rel=1e-15)
    assert s.densities(8) == (.3, .2, .5) and s.densities(9) == (.3, .2, .5) and s.densities(1000) == (.3, .2, .5)  # every step from stop on
    d = train.SparsifySchedule()  # the reference's own schedule
    assert (d.start, d.stop, d.interval, d.exponent, d.targets) == (6000, 20000, 100, 3, (.3, .2, .5))
    assert d.densities(5999) is None and d.densities(6000) == (1.0, 1.0, 1.0) and d.densities(6050) is None
    assert d.densities(13000) == pytest.approx(tuple(.125 + .875 * t for t in (.3, .2, .5)))
    with pytest.raises(ValueError):
        train.SparsifySchedule(start=8, stop=8)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "torch", "sparsification")), reason="the reference is not mounted here")
def test_schedule_against_the_references_sparsifier(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(REFERENCE, "torch"))
    for name in [m for m in sys.modules if m == "sparsification" or m.startswith("sparsification.")]:
        monkeypatch.delitem(sys.modules, name)
    from sparsification import GRUSparsifier
    params = {"W_hr": (0.3, [8, 4], True), "W_hz": (0.2, [8, 4], True), "W_hn": (0.5, [8, 4], True),
              "W_ir": (0.3, [8, 4], False), "W_iz": (0.2, [8, 4], False), "W_in": (0.5, [8, 4], False)}
    torch.manual_seed(4)
    ours = train.new_network(8, 16)
    theirs = copy.deepcopy(ours)
    ref = [GRUSparsifier([(g, params)], 2, 8, 2, 3) for g in (theirs.gru1, theirs.gru2, theirs.gru3)]
    schedule = train.SparsifySchedule(start=2, stop=8, interval=2)
    gen = torch.Generator().manual_seed(8)
    names = [f"gru{k}.weight_{side}_l0" for k in (1, 2, 3) for side in ("ih", "hh")]
    for step in range(1, 12):
        with torch.no_grad():  # what an optimiser step would do, the same on both sides: every weight moves, zeros too
            for n in names:
                delta = .05 * torch.randn(48, 16, generator=gen)
                dict(ours.named_parameters())[n].add_(delta)
                dict(theirs.named_parameters())[n].add_(delta)
        did = schedule.step(ours)
        for r in ref:
            r.step()
        assert did == (step in (2, 4, 6) or step >= 8), step
        for n in names:
            a, b = dict(ours.named_parameters())[n].detach(), dict(theirs.named_parameters())[n].detach()
            assert torch.equal(a == 0, b == 0), (step, n)  # the masks
            assert torch.equal(a, b), (step, n)            # and the weights
    # ... and the schedule ends at the target block densities with the recurrent diagonals kept
    for n in names:
        W = dict(ours.named_parameters())[n].detach()
        for gate, target in enumerate((.3, .2, .5)):
            m = W[gate * 16:(gate + 1) * 16]
            rest = m - torch.diag(torch.diag(m)) if "hh" in n else m
            blocks = (rest.reshape(2, 8, 4, 4) != 0).any(3).any(1)
            assert int(blocks.sum()) == round(8 * target), (n, gate)
            if "hh" in n:
                assert torch.all(torch.diag(m) != 0)


# ---- the command line ----
def test_train_arguments(monkeypatch):
    seen = {}
    monkeypatch.setattr(train, "train_files", lambda **kw: seen.update(kw))
    cli.main(["train", "rec.f32", "out"])
    assert seen == dict(records="rec.f32", out="out", online=None, sequences_per_epoch=None, rir_list=None, epochs=200, batch_size=128,
                        sequence_length=2000, lr=1e-3, lr_decay=5e-5, gamma=.25, sparse=False, initial_checkpoint=None, cond_size=128,
                        gru_size=384, suffix="", seed=None, device=0)  # the reference's defaults
    cli.main(["train", "rec.f32", "out", "--epochs", "3", "--batch-size", "16", "--sequence-length", "500", "--lr", "2e-3", "--lr-decay", "1e-4",
              "--gamma", ".5", "--sparse", "--initial-checkpoint", "a.pth", "--cond-size", "64", "--gru-size", "128", "--suffix", "_x",
              "--seed", "11", "--device", "1"])
    assert seen == dict(records="rec.f32", out="out", online=None, sequences_per_epoch=None, rir_list=None, epochs=3, batch_size=16,
                        sequence_length=500, lr=2e-3, lr_decay=1e-4, gamma=.5, sparse=True, initial_checkpoint="a.pth", cond_size=64,
                        gru_size=128, suffix="_x", seed=11, device=1)
    cli.main(["train", "out", "--online", "s.pcm", "n.pcm", "f.pcm", "--sequences-per-epoch", "256", "--rir-list", "rirs.txt"])
    assert (seen["records"], seen["out"], seen["online"], seen["sequences_per_epoch"], seen["rir_list"]) == \
        (None, "out", ("s.pcm", "n.pcm", "f.pcm"), 256, "rirs.txt")
    for argv in (["train", "rec.f32"], ["train", "a", "b", "c"], ["train", "out", "--online", "s", "n", "f"],
                 ["train", "rec.f32", "out", "--online", "s", "n", "f", "--sequences-per-epoch", "256"],
                 ["train", "out", "--online", "s", "n", "f", "--sequences-per-epoch", "64"], ["train", "rec.f32", "out", "--rir-list", "r"],
                 ["train", "rec.f32", "out", "--epochs", "0"], ["train", "rec.f32", "out", "--gamma", "0"],
                 ["train", "rec.f32", "out", "--sequence-length", "5"]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    with pytest.raises(SystemExit):  # the other commands parse as before
        cli.main(["eval-records"])
