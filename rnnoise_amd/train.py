"""Training on the device: the loop of the reference's torch/rnnoise/train_rnnoise.py in this project's words.

  fit(data, out, ...)   FloatNet.forward_sequence on batches of sequences, the GRU states carried from batch to batch and detached, the
                        loss of librnnoise_amd_train.so (train_loss.TrainerLoss: the doubles of eval-records, and their gradient),
                        AdamW, the 1 / (1 + decay * step) learning rate, optionally the GRU block sparsifier, one checkpoint per epoch
                        under out/checkpoints/ with the reference's keys -- what the reference's dump_rnnoise_weights.py, cli export
                        and float_net.load_checkpoint take as it is.
  RecordFile            the data of a record file (dump_features' output), as the reference's RNNoiseDataset and DataLoader serve it
  OnlineRecords         fresh sequences every epoch, generated on the device (train_data.generate_rounds_device) and never copied
                        back: the records are scored in place through their strides, only the 65 features are gathered for torch
  SparsifySchedule      the schedule of the reference's GRUSparsifier on export.prune_state_dict's mask

  python -m rnnoise_amd.cli train records.f32 out [--epochs N ...]
  python -m rnnoise_amd.cli train out --online speech.pcm noise.pcm fgnoise.pcm --sequences-per-epoch N [...]

The network's forward and backward are torch's (its GRU dominates the step: profiles/train_step.txt); the loss is this project's.
With gru="native" the GRUs' recurrences run on this project's kernels as well (gru_native), with gru="stack" the
three layers as one diagonal launch a step (gru_stack); torch's nn.GRU is the default.
"""
from __future__ import annotations

import os

import numpy as np

from . import evaluate, export, float_net

FEATURES = float_net.FEATURES
ADAM_BETAS, ADAM_EPS = (0.8, 0.98), 1e-8
# the reference's torch/rnnoise/rnnoise.py:38-50
SPARSIFY = dict(start=6000, stop=20000, interval=100, exponent=3, targets=(0.3, 0.2, 0.5))


class SparsifySchedule:
    """The reference's GRUSparsifier (torch/sparsification/gru_sparsifier.py) for the three GRUs of a FloatNet: step() counts a
    training step and, from `start` on every `interval`-th step and from `stop` on every step, sparsifies all six GRU matrices in
    blocks of 8 x 4, gate by gate (targets: reset, update, new), the recurrent diagonals kept, to the density

        alpha + (1 - alpha) * target,   alpha = ((stop - i) / (stop - start)) ** exponent,   0 from `stop` on

    The mask is export.prune_state_dict's: the one the exporter applies in one shot, so a network trained here and exported with
    --densities loses nothing more."""

    def __init__(self, start=SPARSIFY["start"], stop=SPARSIFY["stop"], interval=SPARSIFY["interval"], exponent=SPARSIFY["exponent"],
                 targets=SPARSIFY["targets"]):
        if not (0 <= start < stop and interval >= 1 and len(targets) == 3):
            raise ValueError("sparsify schedule: 0 <= start < stop, interval >= 1, three target densities")
        self.start, self.stop, self.interval, self.exponent, self.targets = start, stop, interval, exponent, tuple(targets)
        self.step_counter = 0

    def densities(self, i: int):
        """the three densities step i sparsifies to, or None where step i does not sparsify"""
        if i < self.start:
            return None
        if i < self.stop:
            if i % self.interval:
                return None
            alpha = ((self.stop - i) / (self.stop - self.start)) ** self.exponent
        else:
            alpha = 0
        return tuple(alpha + (1 - alpha) * t for t in self.targets)

    def step(self, net) -> bool:
        """call after optimizer.step(); -> whether the weights were sparsified"""
        import torch
        self.step_counter += 1
        d = self.densities(self.step_counter)
        if d is None:
            return False
        names = [f"gru{k}.weight_{side}_l0" for k in (1, 2, 3) for side in ("ih", "hh")]
        params = dict(net.named_parameters())
        with torch.no_grad():
            pruned = export.prune_state_dict({n: params[n] for n in names}, d)
            for n in names:
                params[n].copy_(pruned[n])
        return True


class RecordFile:
    """The sequences of a record file or array (evaluate.map_records: whole sequences of sequence_length records of 98 floats) in
    shuffled batches of batch_size, the last partial batch dropped: the reference's RNNoiseDataset behind its DataLoader."""

    def __init__(self, path_or_array, sequence_length: int = 2000, batch_size: int = 128):
        self.data = evaluate.map_records(path_or_array, sequence_length)
        self.batch_size = batch_size
        if self.data.shape[0] < batch_size:
            raise ValueError(f"{self.data.shape[0]} whole sequences of {sequence_length} records: fewer than one batch of {batch_size}")

    def __len__(self):
        return self.data.shape[0] // self.batch_size

    def batches(self, rng: np.random.Generator, device):
        """yields (features (B, T, 65), records (B, T, 98)) float32 tensors on `device`, the features contiguous"""
        import torch
        order = rng.permutation(self.data.shape[0])[:len(self) * self.batch_size].reshape(len(self), self.batch_size)
        for idx in order:
            rec = torch.from_numpy(np.stack([self.data[i] for i in idx])).to(device)
            yield rec[:, :, :FEATURES].contiguous(), rec


class OnlineRecords:
    """Fresh training sequences every epoch, generated on the device: sequences_per_epoch sequences of sequence_length frames drawn
    from three int16 corpora (1-D torch tensors on the device) as dump_features draws them (train_data.draw with this object's own
    generator, seeded), in rounds of batch_size -- one round is one batch, a partial last round is dropped.  The 98-float records stay
    where the features call wrote them, [frame][sequence][98]: the loss reads them through the strides (batch_size * 98, 98) and
    only the 65 features are gathered into the (B, T, 65) tensor torch's layers take.  responses: room impulse responses for the
    reference's -rir_list stage, or None.  model_blob: any "DNNw" blob -- a batch needs one, the extraction runs no network."""

    def __init__(self, speech, noise, fgnoise, sequences_per_epoch: int, sequence_length: int = 2000, batch_size: int = 128, seed=None,
                 responses=None, model_blob=None, device: int = 0, vad: str = "auto", rir_work_bytes: int = 256 << 20):
        import torch

        from . import blob as blob_tools
        from . import capi, train_data
        if sequences_per_epoch < batch_size:
            raise ValueError(f"{sequences_per_epoch} sequences per epoch: fewer than one batch of {batch_size}")
        self.corpora, self.count, self.n_frames, self.batch_size = (speech, noise, fgnoise), sequences_per_epoch, sequence_length, batch_size
        self.count -= self.count % batch_size
        self.rng, self.vad, self.rir_work_bytes = np.random.default_rng(seed), vad, rir_work_bytes
        self.device = torch.device("cuda", device)
        self.model = capi.Model(model_blob if model_blob is not None else blob_tools.synth_model())
        self.batch = capi.Batch(self.model, batch_size, device=device)
        self.spectra = None
        if responses:
            with torch.cuda.device(self.device):
                self.spectra = train_data.rir_spectra(self.batch, responses, self.device)
        self.band_lp = train_data.NB_BANDS

    def __len__(self):
        return self.count // self.batch_size

    def batches(self, rng, device):
        """yields (features (B, T, 65) contiguous, records (B, T, 98): a view of the generator's [T][B][98] tensor, valid until the
        next batch).  `rng` is not used: the draws come from this object's generator."""
        import torch

        from . import train_data
        draws = train_data.draw(self.rng, self.count, [c.numel() for c in self.corpora], self.n_frames, self.band_lp)
        self.band_lp = int(draws.band_lp[-1])
        rirs = None if self.spectra is None else (self.spectra, train_data.draw_rir(self.rng, self.count, len(self.spectra)))
        with torch.cuda.device(self.device):
            for k, rec in train_data.generate_rounds_device(self.batch, *self.corpora, draws, self.n_frames, rirs, self.rir_work_bytes,
                                                            self.vad):
                assert k == self.batch_size
                seq = rec.permute(1, 0, 2)  # (B, T, 98) with strides (98, B * 98, 1)
                yield seq[:, :, :FEATURES].contiguous(), seq

    def close(self):
        self.batch.close()
        self.model.close()


def device_loss(gains, vad, records, gamma):
    """the default loss of fit: train_loss.TrainerLoss on the network's outputs of steps 4 .. T - 1 against records 3 .. T - 2 -- the
    reference's targets [:, 3:-1] -- where they lie -> (loss, gain_loss, vad_loss)"""
    from . import train_loss
    return train_loss.TrainerLoss.apply(gains, vad, records, float_net.LOOKAHEAD, float_net.LOOKAHEAD, gamma)


def new_network(cond_size: int = 128, gru_size: int = 384, seed=None, gru: str = "torch"):
    """a FloatNet initialised as the reference's RNNoise is: torch's defaults, the recurrent GRU weights orthogonal; gru: the
    network's gru_impl (the weights do not depend on it)"""
    import torch
    if seed is not None:
        torch.manual_seed(seed)
    net = float_net.FloatNet(cond_size=cond_size, gru_size=gru_size, gru_impl=gru)
    for gru in (net.gru1, net.gru2, net.gru3):
        torch.nn.init.orthogonal_(gru.weight_hh_l0)
    return net


def checkpoint_path(out: str, epoch: int, suffix: str = "") -> str:
    return os.path.join(out, "checkpoints", f"rnnoise{suffix}_{epoch}.pth")


def fit(data, out: str, epochs: int = 200, lr: float = 1e-3, lr_decay: float = 5e-5, gamma: float = 0.25, sparse=False,
        initial_checkpoint=None, cond_size: int = 128, gru_size: int = 384, suffix: str = "", seed=None, loss=None, device=None,
        on_step=None, log=print, gru: str = "torch"):
    """Trains a FloatNet on `data` -- a RecordFile, an OnlineRecords, or anything with __len__ (batches per epoch) and
    batches(rng, device) -- for `epochs` epochs and writes out/checkpoints/rnnoise{suffix}_{epoch}.pth after each.

    Per batch, as train_rnnoise.py:139-163: zero_grad; gains, vad, states = forward_sequence(features, states) with the states of
    the batch before (None at the start), detached; loss(gains, vad, records, gamma) -> (loss, gain_loss, vad_loss), of which `loss`
    is differentiated; optimizer.step(); with `sparse` the sparsifier's step (True: the reference's schedule, or a SparsifySchedule);
    scheduler.step().  AdamW with betas (.8, .98) and eps 1e-8, LambdaLR 1 / (1 + lr_decay * step).
    loss: a callable; None: device_loss, the two launches of librnnoise_amd_train.so -- then `device` must be a HIP device (None:
    cuda:0).  A loss in plain torch lets the loop run on the CPU (device="cpu").
    seed: the shuffle's (and, without initial_checkpoint, the initialisation's).  on_step: called after every step with a dict
    (epoch, step, loss, gain_loss, vad_loss, lr: the rate the step was taken with, states: the detached states carried on,
    sparsified).  log: called with one line per epoch holding the three means (None: silent).
    gru: "torch" (nn.GRU), "native": the three GRUs' recurrences, forward and backward, on librnnoise_amd_gru.so, or "stack": the
    three layers on librnnoise_amd_gru_stack.so (FloatNet's gru_impl; the device only) -- the same parameters and checkpoints either
    way.
    -> a list with one dict per epoch: epoch, loss, gain_loss, vad_loss (the means over the epoch's batches, as the reference prints
    them), checkpoint (the file)."""
    import torch
    if device is None:
        device = "cuda:0" if loss is None else "cpu"
    device = torch.device(device)
    loss = device_loss if loss is None else loss
    if len(data) < 1:
        raise ValueError("no batch in an epoch")
    os.makedirs(os.path.join(out, "checkpoints"), exist_ok=True)
    checkpoint = dict(model_args=(), model_kwargs=dict(cond_size=cond_size, gru_size=gru_size))
    net = new_network(cond_size, gru_size, seed, gru)
    if initial_checkpoint is not None:
        checkpoint = torch.load(initial_checkpoint, map_location="cpu")
        kw = checkpoint.get("model_kwargs") or {}
        if (kw.get("cond_size", cond_size), kw.get("gru_size", gru_size)) != (cond_size, gru_size):
            raise ValueError(f"{initial_checkpoint} is of cond_size {kw.get('cond_size')}, gru_size {kw.get('gru_size')}")
        net.load_state_dict(checkpoint["state_dict"], strict=False)
    net = net.to(device).train()
    optimizer = torch.optim.AdamW(net.parameters(), lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer=optimizer, lr_lambda=lambda x: 1 / (1 + lr_decay * x))
    schedule = (sparse if isinstance(sparse, SparsifySchedule) else SparsifySchedule()) if sparse else None
    rng = np.random.default_rng(seed)
    states, step, history = None, 0, []
    for epoch in range(1, epochs + 1):
        running = np.zeros(3)
        batches = 0
        for features, records in data.batches(rng, device):
            optimizer.zero_grad()
            gains, vad, states = net.forward_sequence(features, states, return_states=True)
            states = [s.detach() for s in states]
            total, gain_loss, vad_loss = loss(gains, vad, records, gamma)
            total.backward()
            optimizer.step()
            sparsified = schedule.step(net) if schedule is not None else False
            rate = optimizer.param_groups[0]["lr"]
            scheduler.step()
            step += 1
            batches += 1
            values = (float(total.detach()), float(gain_loss.detach()), float(vad_loss.detach()))
            running += values
            if on_step is not None:
                on_step(dict(epoch=epoch, step=step, loss=values[0], gain_loss=values[1], vad_loss=values[2], lr=rate, states=states,
                             sparsified=sparsified))
        means = running / max(batches, 1)
        path = checkpoint_path(out, epoch, suffix)
        checkpoint["state_dict"] = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        checkpoint["loss"] = float(means[0])
        checkpoint["epoch"] = epoch
        torch.save(checkpoint, path)
        history.append(dict(epoch=epoch, loss=float(means[0]), gain_loss=float(means[1]), vad_loss=float(means[2]), checkpoint=path))
        if log is not None:
            log(f"epoch {epoch}: loss {means[0]:.6f} gain_loss {means[1]:.6f} vad_loss {means[2]:.6f} ({batches} batches, step {step})")
    return history


def train_files(records, out: str, online=None, sequences_per_epoch=None, rir_list=None, epochs: int = 200, batch_size: int = 128,
                sequence_length: int = 2000, lr: float = 1e-3, lr_decay: float = 5e-5, gamma: float = 0.25, sparse: bool = False,
                initial_checkpoint=None, cond_size: int = 128, gru_size: int = 384, suffix: str = "", seed=None, device: int = 0,
                log=print, gru: str = "torch"):
    """cli train: a record file, or with online = (speech, noise, fgnoise) file names the corpora behind OnlineRecords (rir_list: a
    file of RIR file names, raw float32, one per line); gru: fit's -> fit's history"""
    import torch
    data = None
    try:
        if online is not None:
            from . import capi
            dev = torch.device("cuda", device)
            corpora = [torch.from_numpy(np.fromfile(p, dtype=np.int16)).to(dev) for p in online]
            responses = None
            if rir_list:
                with open(rir_list) as f:
                    names = [line.rstrip("\n") for line in f if line.rstrip("\n")]
                responses = [np.fromfile(name, dtype=np.float32, count=capi.RIR_MAX) for name in names]
            data = OnlineRecords(*corpora, sequences_per_epoch, sequence_length, batch_size, seed, responses, device=device)
        else:
            data = RecordFile(records, sequence_length, batch_size)
        return fit(data, out, epochs, lr, lr_decay, gamma, sparse, initial_checkpoint, cond_size, gru_size, suffix, seed,
                   device=f"cuda:{device}", log=log, gru=gru)
    finally:
        if isinstance(data, OnlineRecords):
            data.close()
