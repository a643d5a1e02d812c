"""Per-stream suppression controls on the GPU (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls): an all-zero table gives the
bits of a batch without one on both synthesis kernel forms and every network path; mixed per-stream floors, gate thresholds and holds
follow the ctl oracle (tests/csrc/ctl_oracle.c) bit for bit -- out, vad, gains and the exported state -- through every call form, masks,
per-stream resets, imports, 16 kHz PCM, a two-model batch, the pinned host-fed path and tables changed on the device between calls;
dropping the table, the setters' refusals and clamps, 65,536 streams, and the torch / CLI bindings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, load_blob
from ctl_oracle import C_NONE, CtlOracle
from rnnoise_amd import capi, resample
from test_masked_gpu import pattern_mask, s16_of, tiled_pcm

pytestmark = pytest.mark.gpu

FLOORS = [0.0] + [float(capi.floor_of_limit_db(d)) for d in (6, 20, 40)]
THRS = [0.0, 0.3, 0.6, 0.95]
HOLDS = [0, 3, 20]
N_CLASSES = len(FLOORS) * len(THRS) * len(HOLDS)  # 48
CALLS = [5, 1, 8]


@pytest.fixture(scope="module")
def blob():
    return load_blob("default")


@pytest.fixture(scope="module")
def model(blob):
    return capi.Model(blob)


def classes(n, seed=None):
    """control class of every stream: deterministic (stream s: class s % 48) or random"""
    return np.arange(n) % N_CLASSES if seed is None else np.random.default_rng(seed).integers(0, N_CLASSES, n)


def ctl_table(cls):
    fi, ti, hi = cls % 4, (cls // 4) % 4, cls // 16
    return np.ascontiguousarray(np.stack([np.take(FLOORS, fi), np.take(THRS, ti), np.take(HOLDS, hi)], 1), np.float32)


def pcm_for(n, T, seed=3):
    """fuzz signals with silent frames on some streams (the gate acts on silent frames too)"""
    pcm = tiled_pcm(n, T, seed=seed, distinct=97)
    pcm[1:3, ::7] = 0
    pcm[6:, 5::11] = 0
    return pcm


class Ref:
    """one stream on the ctl oracle (ctl None: no table), with the resampler chain of a batch at 48000 / L"""

    def __init__(self, blob, ctl, L=1):
        self.o, self.ctl, self.L = CtlOracle(blob), ctl, L
        self.closed = 0  # frames synthesised with a closed gate
        self.reset_rs()

    def reset_rs(self):
        if self.L > 1:
            self.up, self.dn = resample.Up(self.L), resample.Down(self.L)

    def reset(self):
        self.o.reset()
        self.reset_rs()

    def frame(self, x):
        x = np.asarray(x, np.float32)
        o, v, g = self.o.process(self.up(x) if self.L > 1 else x, self.ctl)
        if self.ctl is not None and self.ctl[1] > 0 and self.o.c > self.ctl[2]:
            self.closed += 1
        return (self.dn(o) if self.L > 1 else o), v, g


def check(refs, pcm, got, calls, events=None, active=None, s16=False, what=""):
    """every checked stream against its Ref, call by call; events[i](refs) runs before call i (what the batch did between calls)"""
    out, vad, gains = got
    t = 0
    for i, c in enumerate(calls):
        if events and i in events:
            events[i](refs)
        for f in range(t, t + c):
            for s, r in refs.items():
                if active is not None and not active[f, s]:
                    continue
                o, v, g = r.frame(pcm[f, s])
                if s16:
                    o = resample.to_s16(o) if r.L > 1 else s16_of(o)
                tag = f"{what} stream {s} frame {f}"
                assert_bits_equal(out[f, s], o, tag + " out")
                assert_bits_equal(vad[f, s], v, tag + " vad")
                assert_bits_equal(gains[f, s], g, tag + " gains")
        t += c


def check_state(b, refs, what=""):
    for s, r in refs.items():
        assert_bits_equal(b.export_state(s), r.o.state, f"{what} state of stream {s}")


def host_run(b, pcm, calls, between=None, active=None, s16=False):
    res, t = [], 0
    for i, c in enumerate(calls):
        if between:
            between(i, 0)
        x = pcm[t:t + c]
        if active is not None:
            r = (b.process_masked_s16 if s16 else b.process_masked)(x, active[t:t + c])
        else:
            r = (b.process_s16 if s16 else b.process)(x)
        res.append(r)
        t += c
    return tuple(np.concatenate([r[k] for r in res]) for k in range(3))


def device_run(b, pcm, calls, between=None, active=None, s16=False):
    """device calls on one non-default HIP stream, no host synchronisation between them; between(i, stream) before call i"""
    torch = pytest.importorskip("torch")
    T, n = pcm.shape[:2]
    st = torch.cuda.Stream()
    h = st.cuda_stream
    d_in = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros_like(d_in)
    d_vad = torch.zeros((T, n), device="cuda")
    d_gains = torch.zeros((T, n, capi.NB_BANDS), device="cuda")
    d_act = torch.from_numpy(active).cuda() if active is not None else None
    torch.cuda.synchronize()
    t = 0
    for i, c in enumerate(calls):
        if between:
            between(i, h)
        if active is None:
            b.process_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(), c, h, s16=s16)
        else:
            b.process_masked_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(),
                                    d_act[t:].data_ptr(), c, h, s16=s16)
        t += c
    st.synchronize()
    return d_out.cpu().numpy(), d_vad.cpu().numpy(), d_gains.cpu().numpy()


def pinned_run(b, pcm, calls):
    """rnnoise_batch_process on pinned host memory: the host-fed frame ring"""
    torch = pytest.importorskip("torch")
    T, n = pcm.shape[:2]
    t_in = torch.from_numpy(pcm).pin_memory()
    t_out = torch.zeros_like(t_in).pin_memory()
    t_vad = torch.zeros((T, n)).pin_memory()
    t_g = torch.zeros((T, n, capi.NB_BANDS)).pin_memory()
    t = 0
    for c in calls:
        b.process_into(t_out[t:].data_ptr(), t_in[t:].data_ptr(), t_vad[t:].data_ptr(), t_g[t:].data_ptr(), c)
        t += c
    return t_out.numpy().copy(), t_vad.numpy().copy(), t_g.numpy().copy()


# ---- an all-zero table is no table ----
ZERO = [(1, [1, 1, 1, 1], None), (48, [1, 1, 1, 1], None), (256, [1, 1, 1], None), (257, [1, 1, 1], None), (600, [1, 1, 1], None),
        (4096, [1, 1, 1], None), (10277, [5], None), (1000, [3, 1], 0), (1000, [3, 1], 1), (1000, [3, 1], 2)]


@pytest.mark.parametrize("n,calls,path", ZERO, ids=[f"n{n}-{'x'.join(map(str, c))}-p{p}" for n, c, p in ZERO])
def test_all_zero_table_is_no_table(model, n, calls, path):
    pcm = pcm_for(n, sum(calls), seed=7)
    pcm[1, min(2, n - 1), 100] = np.nan  # a NaN-poisoned stream
    a, b = capi.Batch(model, n), capi.Batch(model, n)
    b.set_stream_controls(np.zeros((n, 3), np.float32))
    if path is not None:
        a.set_nn_path(path)
        b.set_nn_path(path)
    ga, gb = host_run(a, pcm, calls), host_run(b, pcm, calls)
    for name, x, y in zip(("out", "vad", "gains"), ga, gb):
        assert_bits_equal(y, x, name)
    for s in sorted({0, min(2, n - 1), n // 2, n - 1}):
        assert_bits_equal(b.export_state(s), a.export_state(s), f"state of stream {s}")
    a.close()
    b.close()


# ---- mixed per-stream controls against the ctl oracle ----
MODES = ["host", "host_s16", "device", "device_s16", "masked", "masked_device_s16", "reset_streams", "reset_streams_device",
         "import", "rate16k", "two_models", "pinned", "device_setter"]


@pytest.mark.parametrize("n", [100, 300])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_controls_follow_the_oracle(model, blob, mode, n):
    torch = pytest.importorskip("torch")
    T = sum(CALLS)
    cls = classes(n)
    table = ctl_table(cls)
    rows = list(range(N_CLASSES)) + [n - 1]  # every class once, and the last stream
    L = 3 if mode == "rate16k" else 1
    s16 = mode.endswith("s16")
    if L > 1:
        from test_resample_gpu import low_pcm, tiled
        pcm = tiled(low_pcm(97, T, L, 3), n)
        pcm[1:3, ::7] = 0
    else:
        pcm = pcm_for(n, T)
    if s16:
        pcm = np.clip(np.round(pcm), -32768, 32767).astype(np.int16)
    blobs = {0: blob}
    b = capi.Batch(model, n)
    slots = np.zeros(n, np.uint8)
    if mode == "two_models":
        blobs[1] = load_blob("little")
        little = capi.Model(blobs[1])
        assert b.add_model(little) == 1
        slots = (np.arange(n) // 3 % 2).astype(np.uint8)
        b.set_stream_models(slots)
    if L > 1:
        b.set_pcm_rate(16000)
    b.set_stream_controls(table)
    assert_bits_equal(b.stream_controls(), table, "readback")
    refs = {s: Ref(blobs[int(slots[s])], table[s], L) for s in rows}
    active = pattern_mask(n, T, 0.7, 11) if mode.startswith("masked") else None
    keep = []  # device buffers of the between-call actions, alive until the calls are done
    events, between = {}, None
    reset_list = [0, 5, 17, 33, n - 1]
    if mode in ("reset_streams", "reset_streams_device"):
        def between(i, h):
            if i == 1 and mode == "reset_streams":
                b.reset_streams(reset_list)
            elif i == 1:
                idx = torch.tensor(reset_list, dtype=torch.int32, device="cuda")
                keep.append(idx)
                torch.cuda.synchronize()
                b.reset_streams_device(idx.data_ptr(), len(reset_list), h)
        events[1] = lambda r: [r[s].reset() for s in reset_list]
    elif mode == "import":
        def between(i, h):
            if i == 2:
                b.import_state(3, b.export_state(40))

        def ev(r):
            r[3].o.state[:] = r[40].o.state
            r[3].o.c = C_NONE
        events[2] = ev
    elif mode == "device_setter":
        table2 = ctl_table(classes(n, seed=5))

        def between(i, h):
            if i in (1, 2):
                d = torch.from_numpy(table2 if i == 1 else table).cuda()
                keep.append(d)
                torch.cuda.synchronize()
                b.set_stream_controls_device(d.data_ptr(), h)

        def setter(tab):
            def ev(r):
                for s in r:
                    r[s].ctl = tab[s]  # (the counters carry on)
            return ev
        events[1], events[2] = setter(table2), setter(table)
    if mode in ("host", "host_s16", "masked", "reset_streams", "import", "rate16k", "two_models"):
        got = host_run(b, pcm, CALLS, between, active, s16)
    elif mode == "pinned":
        got = pinned_run(b, pcm, CALLS)
    else:
        got = device_run(b, pcm, CALLS, between, active, s16)
    check(refs, pcm, got, CALLS, events, active, s16, what=mode)
    check_state(b, refs, mode)
    closed = sum(r.closed for r in refs.values())
    assert 0 < closed < sum(CALLS) * len(refs), f"{closed} gated frames: the gate never acts, or always"
    b.close()


# ---- dropping the table ----
def test_dropping_the_table(model, blob):
    n, calls = 300, [5, 4, 3]
    pcm = pcm_for(n, sum(calls), seed=9)
    table = ctl_table(classes(n))
    rows = list(range(N_CLASSES))
    b = capi.Batch(model, n)
    b.set_stream_controls(table)
    refs = {s: Ref(blob, table[s]) for s in rows}

    def between(i, h):
        if i == 1:
            b.set_stream_controls(None)
            assert not b.stream_controls().any()
        elif i == 2:
            b.set_stream_controls(table)  # every counter restarts at 65536

    def drop(r):
        for x in r.values():
            x.ctl = None

    def again(r):
        for s, x in r.items():
            x.ctl, x.o.c = table[s], C_NONE
    got = host_run(b, pcm, calls, between)
    check(refs, pcm, got, calls, {1: drop, 2: again}, what="drop")
    check_state(b, refs, "drop")
    b.close()


# ---- the setters ----
def test_host_setter_refuses_and_changes_nothing(model):
    n = 50
    b = capi.Batch(model, n)
    table = ctl_table(classes(n))
    b.set_stream_controls(table)
    for s, k, v in [(3, 0, np.nan), (4, 1, np.inf), (5, 2, -np.inf), (6, 0, 1.5), (7, 0, -0.1), (8, 1, 1.01), (9, 1, -1e-6),
                    (10, 2, 2.5), (11, 2, 65536), (12, 2, -1), (13, 2, 1e-3)]:
        bad = table.copy()
        bad[s, k] = v
        with pytest.raises(ValueError):
            b.set_stream_controls(bad)
        assert_bits_equal(b.stream_controls(), table, f"after refusing {v} at ({s}, {k})")
    edge = table.copy()
    edge[0] = (1.0, 1.0, 65535)
    b.set_stream_controls(edge)
    assert_bits_equal(b.stream_controls(), edge, "edges of the ranges")
    b.close()


def test_device_setter_clamps(model, blob):
    """entries the host setter refuses go through the device setter as they are; the kernel reads NaN as 0, clamps and truncates"""
    torch = pytest.importorskip("torch")
    n, calls = 64, [5, 1, 8]
    raw = ctl_table(classes(n))
    weird = [(np.nan, 0.5, 3), (2.0, 0.3, 1.7), (-1, np.nan, 5), (0.1, 1.5, 1e9), (0.2, -0.5, -3), (np.nan, np.nan, np.nan),
             (np.inf, 0.6, np.inf), (0.05, np.inf, 2.99), (-np.inf, 0.95, 0.5)]
    for i, w in enumerate(weird):
        raw[i] = w
    pcm = pcm_for(n, sum(calls), seed=13)
    b = capi.Batch(model, n)
    d = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    b.set_stream_controls_device(d.data_ptr(), 0)
    torch.cuda.synchronize()
    assert_bits_equal(b.stream_controls(), raw, "readback of a device table")
    rows = list(range(len(weird))) + [20, 47, 63]
    refs = {s: Ref(blob, raw[s]) for s in rows}  # (the oracle takes an entry as the kernel does)
    got = device_run(b, pcm, calls)
    check(refs, pcm, got, calls, what="clamped")
    check_state(b, refs, "clamped")
    b.close()


# ---- at size ----
def test_65536_streams_random_map(model, blob):
    torch = pytest.importorskip("torch")
    n, calls = 65536, [5, 1, 8]
    T = sum(calls)
    cls = classes(n, seed=21)
    table = ctl_table(cls)
    pcm = pcm_for(n, T, seed=17)
    b = capi.Batch(model, n)
    b.set_stream_controls(table)
    rows = sorted(int(s) for k in range(N_CLASSES) for s in np.nonzero(cls == k)[0][[0, -1]])  # two of every class: 96
    assert len(rows) >= 64
    st = torch.cuda.Stream()
    d_in = torch.from_numpy(pcm).cuda()
    del pcm
    d_out = torch.empty_like(d_in)
    d_vad = torch.empty((T, n), device="cuda")
    d_gains = torch.empty((T, n, capi.NB_BANDS), device="cuda")
    torch.cuda.synchronize()
    t = 0
    for c in calls:
        b.process_device(d_out[t:].data_ptr(), d_in[t:].data_ptr(), d_vad[t:].data_ptr(), d_gains[t:].data_ptr(), c, st.cuda_stream)
        t += c
    st.synchronize()
    idx = torch.tensor(rows, device="cuda")
    sub = lambda x: x[:, idx].cpu().numpy()  # noqa: E731
    pcm_s, got = sub(d_in), (sub(d_out), sub(d_vad), sub(d_gains))
    refs = {j: Ref(blob, table[s]) for j, s in enumerate(rows)}
    check(refs, pcm_s, got, calls, what="65,536 streams")
    for j, s in enumerate(rows[::8]):
        assert_bits_equal(b.export_state(s), refs[rows.index(s)].o.state, f"state of stream {s}")
    b.close()


# ---- bindings ----
def test_torch_op_matches_capi(model, blob):
    torch = pytest.importorskip("torch")
    from rnnoise_amd.torch_op import RNNoiseOp
    n, T = 96, 9
    pcm = pcm_for(n, T, seed=23)
    lim = np.where(np.arange(n) % 3 == 0, np.inf, np.arange(n) % 4 * 10.0)
    thr = (np.arange(n) % 5) * 0.2
    hold = np.arange(n) % 7
    op = RNNoiseOp(blob, n)
    op.set_stream_controls(limit_db=lim, vad_threshold=thr, hold_frames=hold)
    out, vad, gains = op(torch.from_numpy(pcm).cuda())
    torch.cuda.synchronize()
    b = capi.Batch(model, n)
    b.set_stream_controls(capi.controls_table(n, lim, thr, hold))
    assert_bits_equal(op.batch.stream_controls(), b.stream_controls(), "tables")
    want = b.process(pcm)
    for name, x, y in zip(("out", "vad", "gains"), (out.cpu().numpy(), vad.cpu().numpy(), gains.cpu().numpy()), want):
        assert_bits_equal(x, y, name)
    op.clear_stream_controls()
    assert not op.batch.stream_controls().any()
    op.close()
    b.close()


def test_cli_flags_match_capi(model, blob, tmp_path):
    n, T = 3, 12
    pcm = np.clip(np.round(pcm_for(n, T, seed=29)), -32768, 32767).astype(np.int16)
    bpath = tmp_path / "w.blob"
    bpath.write_bytes(blob)
    files = []
    for s in range(n):
        p = tmp_path / f"s{s}.raw"
        p.write_bytes(pcm[:, s].tobytes())
        files.append(str(p))
    env = dict(os.environ)
    subprocess.run([sys.executable, "-m", "rnnoise_amd.cli", "denoise", "--model", str(bpath), "--out-dir", str(tmp_path / "out"),
                    "--atten-limit-db", "12", "--vad-gate", "0.5", "--vad-hold", "4", *files], cwd=ROOT, env=env, check=True,
                   timeout=300)
    b = capi.Batch(model, n)
    b.set_stream_controls(capi.controls_table(n, 12.0, 0.5, 4))
    want, _, _ = b.process_s16(pcm)
    for s in range(n):
        got = np.fromfile(str(tmp_path / "out" / f"s{s}.raw.denoised.raw"), np.int16).reshape(-1, 480)
        assert_bits_equal(got, want[1:, s], f"file {s}")
    b.close()
