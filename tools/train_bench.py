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

  python tools/train_bench.py --gru stack [--rows N] [--frames T] [--rounds R] [--warmup W] [--out FILE] [--once]

measures the diagonal stack beside the per-layer native path in the same job, the two alternating round by round:
the network's forward and backward with gru_impl "native" and "stack"; the three recurrences alone on fixed inputs -- the native
path's three forward and three backward calls with the two projections between them, against the stack's one forward and one backward
call, with the time per launch over the T + 2 launches; and the torch-side weight gradients of both.  It states whether every stack
round lies below every native round.  FILE defaults to profiles/train_step_gru_stack.txt.  --once makes one forward and one backward
call of the stack and exits: the program for a kernel trace.
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


def stack_bench(a):
    """--gru stack: the network and the three recurrences, librnnoise_amd_gru.so layer by layer and librnnoise_amd_gru_stack.so
    alternating in one job"""
    import torch
    from torch.nn import functional as F

    from rnnoise_amd import gru_native, gru_stack, train
    dev = torch.device("cuda", 0)
    N, T, K, H = a.rows, a.frames, a.frames - 4, 384
    out = a.out or os.path.join(ROOT, "profiles", "train_step_gru_stack.txt")

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(cases):
        ms = {k: [] for k in cases}
        for r in range(a.warmup + a.rounds):
            for k, fn in cases.items():
                t = once(fn)
                if r >= a.warmup:
                    ms[k].append(t)
        return ms

    # ---- the three recurrences on fixed inputs ----
    gen = torch.Generator().manual_seed(1)
    grus = [torch.nn.GRU(H, H, batch_first=True).to(dev) for _ in range(3)]
    w_ih, b_ih = [None] + [g.weight_ih_l0.detach() for g in grus[1:]], [None] + [g.bias_ih_l0.detach() for g in grus[1:]]
    w_hh, b_hh = [g.weight_hh_l0.detach() for g in grus], [g.bias_hh_l0.detach() for g in grus]
    gi0 = torch.randn(N, K, 3 * H, generator=gen).to(dev)
    dcat = torch.randn(N, K, 4 * H, generator=gen).to(dev)
    dy = [dcat[:, :, (l + 1) * H:(l + 2) * H] for l in range(3)]
    kept = {}

    def stack_forward():
        kept["ys"], kept["saved"] = gru_stack.stack_forward(gi0, w_ih, b_ih, w_hh, b_hh)

    def stack_backward():
        kept["dgi"], kept["dgh"], _ = gru_stack.stack_backward(dy, kept["ys"], kept["saved"], w_ih, w_hh)

    if a.once:
        stack_forward()
        stack_backward()
        torch.cuda.synchronize()
        print(f"one forward and one backward call of librnnoise_amd_gru_stack.so, {N} rows x {K} steps: {K + 2} launches each")
        return

    def native_forward():
        gi, kept["nys"], kept["nsaved"] = gi0, [], []
        for l in range(3):
            if l:
                gi = F.linear(kept["nys"][l - 1], w_ih[l], b_ih[l])
            y, s = gru_native.sequence_forward(gi, w_hh[l], b_hh[l], None)
            kept["nys"].append(y)
            kept["nsaved"].append(s)

    def native_backward():
        kept["ndgh"], kept["ndgi"], dx = [None] * 3, [None] * 3, None
        for l in (2, 1, 0):
            d = dy[l] if dx is None else dy[l] + dx
            kept["ndgi"][l], kept["ndgh"][l], _ = gru_native.sequence_backward(d, kept["nys"][l], kept["nsaved"][l], w_hh[l], None, None)
            if l:
                dx = kept["ndgi"][l] @ w_ih[l]

    def stack_weight_grads(per_step):
        def fn():
            for l in range(3):
                gru_native.weight_grads(kept["dgh"][l], kept["ys"][l], None)
                if l:
                    gru_stack.input_weight_grads(kept["dgi"][l], kept["ys"][l - 1], per_step=per_step)
        return fn

    def native_weight_grads():
        for l in range(3):
            gru_native.weight_grads(kept["ndgh"][l], kept["nys"][l], None)
            if l:  # what F.linear's autograd does: one product
                kept["ndgi"][l].reshape(-1, 3 * H).t() @ kept["nys"][l - 1].reshape(-1, H)
                kept["ndgi"][l].sum((0, 1))

    fmt = lambda ms: f"{statistics.median(ms):9.3f} ms  ({min(ms):.3f} .. {max(ms):.3f})"

    def verdict(name, native, stack):
        """the ratio of the medians beside both spreads; "faster" only where every stack round lies below every native round, or the
        gap of the medians exceeds the larger spread"""
        mn, mk = statistics.median(native), statistics.median(stack)
        spread = max(max(native) - min(native), max(stack) - min(stack))
        if max(stack) < min(native) or mn - mk > spread:
            word = "stack faster"
        elif max(native) < min(stack) or mk - mn > spread:
            word = "stack slower"
        else:
            word = "no difference beyond the spread"
        return (f"  {name}: native / stack = {mn / mk:.3f} (medians {mn:.3f} and {mk:.3f} ms; spread native {max(native) - min(native):.3f}, "
                f"stack {max(stack) - min(stack):.3f} ms): {word}")

    lines = [f"# tools/train_bench.py --gru stack --rows {N} --frames {T} --rounds {a.rounds} --warmup {a.warmup}; "
             f"{torch.cuda.get_device_name(0)}; median of {a.rounds} (min .. max), device events, the implementations alternating"]
    rec = alternate({"native: 3 forward calls + 2 projections": native_forward, "native: 3 backward calls + 2 dx products": native_backward,
                     "stack: the forward call": stack_forward, "stack: the backward call": stack_backward,
                     "native: weight gradients (torch)": native_weight_grads,
                     "stack: weight gradients, dW_ih per step": stack_weight_grads(True),
                     "stack: weight gradients, dW_ih one product": stack_weight_grads(False)})

    # ---- the network: forward, and backward of a fixed linear functional of its outputs ----
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
    ms = alternate({"native forward": forward("native"), "native backward": backward("native"), "stack forward": forward("stack"),
                    "stack backward": backward("stack")})
    lines.append(f"network forward and backward, batch {N} x {T} frames, cond_size 128, gru_size {H}:")
    for k in ms:
        lines.append(f"  {k:44s} {fmt(ms[k])}")
    lines.append(verdict("network forward", ms["native forward"], ms["stack forward"]))
    lines.append(verdict("network backward", ms["native backward"], ms["stack backward"]))
    both = lambda impl: [f + b for f, b in zip(ms[impl + " forward"], ms[impl + " backward"])]
    lines.append(verdict("network forward + backward", both("native"), both("stack")))
    lines.append(f"the three recurrences alone, {N} rows x {K} steps, hidden {H}, fixed inputs (native: {3 * K} launches each way and the "
                 f"torch products between the layers; stack: {K + 2} launches each way):")
    for k in rec:
        lines.append(f"  {k:44s} {fmt(rec[k])}")
    for k in ("stack: the forward call", "stack: the backward call"):
        lines.append(f"  {k + ', per launch':44s} {1e3 * statistics.median(rec[k]) / (K + 2):9.2f} us")
    lines.append(verdict("recurrences forward", rec["native: 3 forward calls + 2 projections"], rec["stack: the forward call"]))
    lines.append(verdict("recurrences backward", rec["native: 3 backward calls + 2 dx products"], rec["stack: the backward call"]))
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
    ap.add_argument("--gru", choices=("torch", "native", "stack"), default="torch")
    ap.add_argument("--once", action="store_true", help="with --gru stack: one forward and one backward call, nothing measured")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_bench: no GPU: nothing measured")
    if a.gru == "native":
        return gru_bench(a)
    if a.gru == "stack":
        return stack_bench(a)
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
