"""What a training step costs on the device, and what the loss-and-gradient call costs beside torch's own formula.

  python tools/train_bench.py [--rows N] [--frames T] [--rounds R] [--warmup W] [--out FILE]

Two measurements in one job, device events on torch's stream, median of R rounds with the range:

  loss call   rnnoise_amd/train_loss.loss_and_grad (librnnoise_amd_train.so: two launches, double) on N rows x (T - 4) steps against
              the float32 torch formula of the reference trainer, forward + backward, on the same device tensors
  step        one training step at batch N x T frames, split into: online data generation (train_data.generate_rounds_device and the
              gather of the features), the network's forward, the loss (the library's call), the backward through the network, and
              the optimiser -- each part between its own pair of events, the parts run one after the other as train.fit runs them

Writes the table to FILE (default profiles/train_step.txt) and prints it.  Without a GPU it fails: a number that was not measured
is not written.

  python tools/train_bench.py --gru native [--rows N] [--frames T] [--rounds R] [--warmup W] [--out FILE]

measures the native GRUs instead, beside torch's in the same job, the two alternating round by round: the network's
forward and backward with FloatNet's gru_impl "torch" and "native"; and one layer on fixed inputs -- nn.GRU forward and backward
against the forward and backward calls of librnnoise_amd_gru.so, with the per-step time of the latter.  FILE defaults to
profiles/train_step_gru.txt; profiles/train_step.txt is not touched.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def gru_bench(a):
    """--gru native: the network and one layer's recurrence, torch's nn.GRU and librnnoise_amd_gru.so alternating in one job"""
    import torch
    from torch.nn import functional as F

    from rnnoise_amd import gru_native, train
    dev = torch.device("cuda", 0)
    N, T, K, H = a.rows, a.frames, a.frames - 4, 384
    out = a.out or os.path.join(ROOT, "profiles", "train_step_gru.txt")

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(cases):
        """{name: fn} -> {name: times in ms}: round after round, every case once per round"""
        ms = {k: [] for k in cases}
        for r in range(a.warmup + a.rounds):
            for k, fn in cases.items():
                t = once(fn)
                if r >= a.warmup:
                    ms[k].append(t)
        return ms

    fmt = lambda ms: f"{statistics.median(ms):9.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})"
    lines = [f"# tools/train_bench.py --gru native --rows {N} --frames {T} --rounds {a.rounds} --warmup {a.warmup}; "
             f"{torch.cuda.get_device_name(0)}; median of {a.rounds} (min .. max), device events, the implementations alternating"]

    # ---- the network: forward, and backward of a fixed linear functional of its outputs ----
    gen = torch.Generator().manual_seed(1)
    features = torch.randn(N, T, 65, generator=gen).to(dev)
    A, B = torch.randn(N, K, 32, generator=gen).to(dev), torch.randn(N, K, 1, generator=gen).to(dev)
    net = train.new_network(seed=1).to(dev).train()
    held = {}

    def forward(impl):
        def fn():
            net.gru_impl = impl
            net.zero_grad()
            g, v = net.forward_sequence(features)
            held[impl] = (g * A).sum() + (v * B).sum()
        return fn

    def backward(impl):
        return lambda: held.pop(impl).backward()
    ms = alternate({"torch forward": forward("torch"), "torch backward": backward("torch"), "native forward": forward("native"),
                    "native backward": backward("native")})
    lines.append(f"network forward and backward, batch {N} x {T} frames, cond_size 128, gru_size {H}:")
    for k in ms:
        lines.append(f"  {k:34s} {fmt(ms[k])}")

    # ---- one layer's recurrence on fixed gi ----
    gru = torch.nn.GRU(H, H, batch_first=True).to(dev)
    x = torch.randn(N, K, H, generator=gen).to(dev).requires_grad_(True)
    dy = torch.randn(N, K, H, generator=gen).to(dev)
    with torch.no_grad():
        gi = F.linear(x, gru.weight_ih_l0, gru.bias_ih_l0)
    w, b = gru.weight_hh_l0.detach(), gru.bias_hh_l0.detach()
    y, dgi = torch.empty(N, K, H, device=dev), torch.empty(N, K, 3 * H, device=dev)
    kept = {}

    def nn_forward():
        kept["y"] = gru(x)[0]

    def nn_backward():
        x.grad = None
        gru.zero_grad()
        kept.pop("y").backward(dy)

    def native_forward():
        kept["saved"] = gru_native.sequence_forward(gi, w, b, None, y=y)[1]

    def native_backward():
        kept["dgh"] = gru_native.sequence_backward(dy, y, kept["saved"], w, None, None, dgi=dgi)[1]
    ms = alternate({"nn.GRU forward (whole layer)": nn_forward, "nn.GRU backward (whole layer)": nn_backward,
                    "native recurrence forward": native_forward, "native recurrence backward": native_backward,
                    "native dW_hh, db_hh (torch)": lambda: gru_native.weight_grads(kept["dgh"], y, None),
                    "input projection (F.linear)": lambda: F.linear(x.detach(), gru.weight_ih_l0, gru.bias_ih_l0)})
    lines.append(f"one layer, {N} rows x {K} steps, hidden {H} (nn.GRU: projection, recurrence and weight gradients; native: the {K} "
                 "launches of the recurrence alone):")
    for k in ms:
        lines.append(f"  {k:34s} {fmt(ms[k])}")
    for k in ("native recurrence forward", "native recurrence backward"):
        lines.append(f"  {k + ', per step':34s} {1e3 * statistics.median(ms[k]) / K:9.2f} us")
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gru", choices=("torch", "native"), default="torch")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_bench: no GPU: nothing measured")
    if a.gru == "native":
        return gru_bench(a)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "train_step.txt")
    from rnnoise_amd import synth, train, train_loss
    dev = torch.device("cuda", 0)
    N, T = a.rows, a.frames
    K = T - 4

    def timed(fn):
        """the times of fn() in ms over the rounds, after the warm-up"""
        ms = []
        for r in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    fmt = lambda ms: f"{statistics.median(ms):9.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})"
    lines = [f"# tools/train_bench.py --rows {N} --frames {T} --rounds {a.rounds} --warmup {a.warmup}; {torch.cuda.get_device_name(0)}; "
             f"median of {a.rounds} (min .. max), device events"]

    # ---- the online data of one batch, and a network ----
    span = 480 * T
    corpora = [torch.from_numpy(np.tile(synth.stream_pcm(s, 400), -(-(span + extra) // (400 * 480)))[:span + extra].copy()).to(dev)
               for s, extra in ((3, 96001), (77, 48001), (130, 7))]
    data = train.OnlineRecords(*corpora, N, T, N, seed=1)
    state = {}

    def generate():
        state["features"], state["records"] = next(iter(data.batches(None, dev)))
    gen_ms = timed(generate)
    features, records = state["features"], state["records"]
    net = train.new_network(seed=1).to(dev).train()
    optimizer = torch.optim.AdamW(net.parameters(), lr=1e-3, betas=train.ADAM_BETAS, eps=train.ADAM_EPS)

    # ---- the loss call against torch's formula, on the network's own outputs ----
    with torch.no_grad():
        gains, vad = net.forward_sequence(features)
    lib_ms = timed(lambda: train_loss.loss_and_grad(records, gains, vad, 4, 4, .25))
    lib_sums_ms = timed(lambda: train_loss.loss_and_grad(records, gains, vad, 4, 4, .25, want_grad=False))

    def torch_formula():
        p, q = gains.detach().requires_grad_(True), vad.detach().requires_grad_(True)
        g, v = records[:, 3:-1, 65:97], records[:, 3:-1, 97:]
        tg = torch.clamp(g, min=0)
        tg = tg * (torch.tanh(8 * tg) ** 2)
        e = p ** .25 - tg ** .25
        gain_loss = torch.mean((1 + 5. * v) * torch.clamp(g + 1, max=1) * (e ** 2))
        vad_loss = torch.mean(torch.abs(2 * v - 1) * (-v * torch.log(.01 + q) - (1 - v) * torch.log(1.01 - q)))
        (gain_loss + .001 * vad_loss).backward()
    torch_ms = timed(torch_formula)
    lines += [f"loss and gradient, {N} rows x {K} steps (records read in place, strides ({N * 98}, 98)):",
              f"  librnnoise_amd_train.so, sums and gradients (two launches, float64)   {fmt(lib_ms)}",
              f"  librnnoise_amd_train.so, sums only                                    {fmt(lib_sums_ms)}",
              f"  torch, the trainer's formula in float32, forward + backward           {fmt(torch_ms)}"]

    # ---- one training step, part by part ----
    parts = {k: [] for k in ("forward", "loss", "backward", "optimiser")}
    for r in range(a.warmup + a.rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        optimizer.zero_grad()
        ev[0].record()
        g, v, _ = net.forward_sequence(features, None, return_states=True)
        ev[1].record()
        loss, _, _ = train.device_loss(g, v, records, .25)
        ev[2].record()
        loss.backward()
        ev[3].record()
        optimizer.step()
        ev[4].record()
        ev[4].synchronize()
        if r >= a.warmup:
            for k, name in enumerate(parts):
                parts[name].append(ev[k].elapsed_time(ev[k + 1]))
    total = statistics.median(gen_ms) + sum(statistics.median(v) for v in parts.values())
    lines.append(f"one training step, batch {N} x {T} frames, cond_size 128, gru_size 384 (sum of the medians {total:.1f} ms):")
    for name, ms in (("online data: generate + gather", gen_ms), ("network forward (torch)", parts["forward"]),
                     ("loss: the library's call, means", parts["loss"]), ("network backward (torch)", parts["backward"]),
                     ("optimiser (AdamW)", parts["optimiser"])):
        lines.append(f"  {name:34s} {fmt(ms)}  {100 * statistics.median(ms) / total:5.1f} %")
    data.close()
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
