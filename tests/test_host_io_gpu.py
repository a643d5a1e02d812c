"""GPU suite: the pinned ring of the host-fed path (rnnoise_amd/csrc/host_io.cpp) in each of its copy modes -- `sdma` (the two named
copy engines, the default), `one` and `hp` (the runtime's copies on one stream or on two).  $RNNOISE_AMD_HOSTIO_COPY is read once per
process, so every mode runs in ONE fresh child process (this file, run as a script) that does all of its cases on small batches:

  ring edges    the ring has 6 slots and the high-pass runs 3 frames ahead: successive calls of 1, 5, 6, 7 and 13 frames on one batch
                (signal-pool reuse and the running counts carry from call to call), as float PCM with VAD and gains, as int16 PCM with
                both result pointers null (the download's completion count depends on which are present), as int16 PCM with only
                VAD, and a float call after the int16 ones (the slot stride follows the call's sample size);
  a long call   1,025 int16 frames: longer than the count ring, so the engines step aside for that call -- and come back for the
                7-frame call that follows.

What it is compared against: a twin batch of the same model fed the same frames from device memory through process_device, the path
that has no host copies -- PCM, VAD, gains and the exported state of a few streams bit-identical; the five replicas of each of the 8
distinct signals equal; and the 13-frame float call's first block against the oracle.  No case provokes a failed copy or a timeout."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, bits, load_blob, use_rcp_profile

pytestmark = pytest.mark.gpu
LENGTHS = (1, 5, 6, 7, 13)
R = 8  # distinct signals


@pytest.mark.parametrize("mode", ["sdma", "one", "hp"])
def test_pinned_ring_in_each_copy_mode(mode):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("RNNOISE_AMD_HOSTIO_COPY", None)  # (sdma: the default, variable unset)
    if mode != "sdma":
        env["RNNOISE_AMD_HOSTIO_COPY"] = mode
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0 and "every case ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    if mode == "sdma":  # ... or the child has checked the runtime's copies instead of the engines
        assert "unavailable" not in r.stderr and "falling back" not in r.stderr, r.stderr[-3000:]


class _Pair:
    """a batch fed from pinned host memory (process_into: the ring) and its twin fed from device memory (process_device)"""

    def __init__(self, model, n):
        from rnnoise_amd import capi
        self.n, self.ring, self.twin = n, capi.Batch(model, n), capi.Batch(model, n)

    def call(self, pcm, s16, vad, gains, what):
        """one call of both on pcm (T, n, 480) float32; returns what the ring delivered"""
        import torch
        T, n = pcm.shape[0], self.n
        t_in = torch.from_numpy(np.ascontiguousarray(pcm.astype(np.int16) if s16 else pcm)).pin_memory()
        t_out = torch.zeros_like(t_in).pin_memory()
        t_vad = torch.full((T, n), -1.0).pin_memory() if vad else None
        t_g = torch.full((T, n, 32), -1.0).pin_memory() if gains else None
        self.ring.process_into(t_out.data_ptr(), t_in.data_ptr(), t_vad.data_ptr() if vad else 0, t_g.data_ptr() if gains else 0, T, s16=s16)
        d_in = t_in.cuda()
        d_out = torch.zeros_like(d_in)
        d_vad = torch.full((T, n), -1.0, device="cuda") if vad else None
        d_g = torch.full((T, n, 32), -1.0, device="cuda") if gains else None
        self.twin.process_device(d_out.data_ptr(), d_in.data_ptr(), d_vad.data_ptr() if vad else 0, d_g.data_ptr() if gains else 0, T,
                                 torch.cuda.current_stream().cuda_stream, s16=s16)
        torch.cuda.synchronize()
        got = dict(out=t_out.numpy(), vad=t_vad.numpy() if vad else None, gains=t_g.numpy() if gains else None)
        for name, dev in (("out", d_out), ("vad", d_vad), ("gains", d_g)):
            if dev is None:
                continue
            a = got[name]
            assert_bits_equal(a, dev.cpu().numpy(), f"{what}: {name} against the device-fed twin")
            rep = bits(a).reshape(T, n // R, R, -1)
            assert (rep == rep[:, :1]).all(), f"{what}: {name} differs between the replicas of a signal"
        return got

    def states_equal(self, what):
        for s in (0, R - 1, self.n - 1):
            assert_bits_equal(self.ring.export_state(s), self.twin.export_state(s), f"{what}: state of stream {s}")


def _child():
    from oracle.binding import Oracle
    from rnnoise_amd import capi, synth
    use_rcp_profile("intel")
    blob = load_blob("default")
    model = capi.Model(blob)
    mode, t0 = os.environ.get("RNNOISE_AMD_HOSTIO_COPY", "sdma"), time.time()

    # ring edges: 40 streams = 8 signals tiled five times, three passes over the call lengths and one more call on ONE pair of batches
    n, per_pass = 40, sum(LENGTHS)
    base = synth.batch_pcm(range(R), 3 * per_pass + 7, lead_silence=1)  # (frames, 8, 480) s16-valued float32
    pcm = np.ascontiguousarray(np.tile(base, (1, n // R, 1)))
    pair, at = _Pair(model, n), 0
    for label, s16, vad, gains in (("float, vad and gains", False, True, True), ("int16, no results", True, False, False),
                                   ("int16, vad only", True, True, False)):
        for T in LENGTHS:
            got = pair.call(pcm[at:at + T], s16, vad, gains, f"{mode}: {label}, {T} frames at frame {at}")
            if not s16 and T == 13:  # the oracle's first block: the batch has had float frames only so far
                for s in range(R):
                    want = Oracle(blob).run(base[:at + T, s])
                    for name in ("out", "vad", "gains"):
                        assert_bits_equal(got[name][:, s], want[name][at:], f"{mode}: {label}, stream {s}: {name} against the oracle")
            at += T
        pair.states_equal(f"{mode}: after {label}")
        print(f"{mode}: {label}: calls of {LENGTHS} frames ok ({time.time() - t0:.1f} s)", flush=True)
    pair.call(pcm[at:at + 7], False, True, True, f"{mode}: float after int16, 7 frames at frame {at}")
    pair.states_equal(f"{mode}: after the float call behind the int16 calls")
    print(f"{mode}: float call after the int16 calls ok ({time.time() - t0:.1f} s)", flush=True)

    # a call longer than the count ring (1,024 frames), then a short one
    long_pcm = synth.batch_pcm(range(R), 1025 + 7, lead_silence=1)
    pair = _Pair(model, R)
    pair.call(long_pcm[:1025], True, True, True, f"{mode}: int16, 1,025 frames")
    pair.call(long_pcm[1025:], True, True, True, f"{mode}: int16, 7 frames after the long call")
    pair.states_equal(f"{mode}: after the long call")
    print(f"{mode}: 1,025-frame call and the call after it ok ({time.time() - t0:.1f} s)", flush=True)
    print("every case ok", flush=True)


if __name__ == "__main__":
    _child()
