"""Training-feature extraction at size (include/rnnoise_amd.h: rnnoise_batch_train_features[_device]): the
pass-through high-pass kernel (rn_launch_hp_passthrough, 64 streams per wave) and the TRAINING instantiation of the analysis kernel
(rn_train_features_kernel) against oracle.binding.TrainOracle, bit for bit, on the stream set of tests/train_cases.py -- which
tests/test_train_cases_cpu.py holds to its purpose and tests/test_train_features.py pins to the reference at the band-limit edges.

  a  every band limit: lowpass 0 .. 482 (every bin of every lane of the register FFT's permutation, one past the spectrum, none),
     band_lp 0 .. 33, in one-frame and six-frame calls that wrap the 6-slot pitch ring and the 3-slot spectrum ring twice
  b  batch sizes around the 64 streams of a high-pass wave, and one that keeps many workgroups per CU in flight
  c  the device form on a stream of the caller's
  d  reset, and the frame-phase counters extraction shares with rnnoise_batch_process
  e  the model map, the controls and the format table, all of which extraction ignores
  f  NaN / Inf in some streams reach no other stream

The oracle runs once per distinct stream (module fixture), never per batch stream -- but in (a), where every stream has a band
limit of its own."""
import ctypes as C

import numpy as np
import pytest

import train_cases as tc
from conftest import assert_bits_equal, bits, load_blob
from rnnoise_amd import capi

pytestmark = pytest.mark.gpu
SENTINEL = np.array([0xFFC12345], np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def model():
    return capi.Model(load_blob("default"))


@pytest.fixture(scope="module")
def want():
    """(T, D, 98): the oracle's records of the D distinct streams, shared and never written"""
    rec = tc.oracle_records(tc.cases())
    rec.setflags(write=False)
    return rec


def extract(b, c, calls):
    """rnnoise_batch_train_features on batch b over the frames of c, in calls of `calls` frames -> (sum(calls), n, 98)"""
    out, t = [], 0
    for k in calls:
        out.append(b.train_features(*c.args(slice(t, t + k))))
        t += k
    assert t == c.clean.shape[0]
    return np.concatenate(out)


def compare(rec, ref, src, what, skip=()):
    """records (T, n, 98) of a batch whose stream i is distinct stream src[i] of ref (T', D, 98)"""
    T = rec.shape[0]
    for s in range(rec.shape[1]):
        if s not in skip:
            assert_bits_equal(rec[:, s], ref[:T, src[s]], f"{what}: stream {s} (case {src[s]}: {tc.cases().labels[src[s]]})")


# ---- a. every band limit ----
def test_every_band_limit(model):
    """483 = 7 * 64 + 35 streams, lowpass = the stream's index, band_lp = index mod 34, in calls of (1, 6, 1, 6) frames: every record
    of every stream against a TrainOracle of its own.  A stream the high-pass launch did not reach has an empty pitch ring: its
    pitch features (32 .. 64 of the record) differ from the oracle's."""
    n, calls = 483, (1, 6, 1, 6)
    s = np.arange(n)
    c = tc.cycled(n, slice(0, sum(calls)), lowpass=s, band_lp=s % 34, noise_free=(s // 2) % 2)
    ref = tc.oracle_records(c)
    b = capi.Batch(model, n)
    rec = extract(b, c, calls)
    b.close()
    # the limits bite: next to each other, streams of one signal would differ (what a limit off by one bin or one band changes)
    assert (ref[:, :, tc.TARGETS] == -1).any() and (ref[:, :, tc.TARGETS] >= 0).any()
    for i in range(n):
        assert_bits_equal(rec[:, i], ref[:, i], f"stream {i} ({c.labels[i]}, lowpass {i}, band_lp {i % 34}, noise_free {c.noise_free[i]})")


# ---- b. sizes ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4099])
def test_sizes(model, want, n):
    """stream i takes distinct case i mod 97 with its own parameters; 8 frames in calls of (1, 7)"""
    c = tc.cycled(n, slice(0, 8))
    b = capi.Batch(model, n)
    rec = extract(b, c, (1, 7))
    b.close()
    compare(rec, want, np.arange(n) % tc.D, f"{n} streams")


# ---- c. the device form ----
def test_device_form_on_a_stream_of_the_callers(model, want):
    """rnnoise_batch_train_features_device with torch tensors on a non-default stream, in calls of (1, 5, 0, 2) frames: the host
    form's bits after a synchronise of that stream alone, nothing written behind the last frame, no input written"""
    torch = pytest.importorskip("torch")
    n, calls = 130, (1, 5, 0, 2)
    T = sum(calls)
    c = tc.cycled(n, slice(0, T))
    dev = torch.device("cuda", 0)
    host = [np.ascontiguousarray(a) for a in c.args()]
    ins = [torch.from_numpy(a).to(dev) for a in host]
    rec = torch.from_numpy(np.full((T + 1, n, tc.REC), SENTINEL, np.float32)).to(dev)
    torch.cuda.synchronize()                                    # (the uploads ran on torch's own stream)
    st = torch.cuda.Stream(device=dev)
    b = capi.Batch(model, n)
    fn = capi.lib().rnnoise_batch_train_features_device
    t = 0
    for k in calls:
        ptrs = [rec.data_ptr() + t * n * tc.REC * 4, ins[0].data_ptr() + t * n * 480 * 4, ins[1].data_ptr() + t * n * 480 * 4,
                ins[2].data_ptr() + t * n * 4, ins[3].data_ptr(), ins[4].data_ptr(), ins[5].data_ptr()]
        assert fn(b.h, *ptrs, k, C.c_void_p(st.cuda_stream)) == 0, (t, k)
        t += k
    st.synchronize()
    got = rec.cpu().numpy()
    for a, d in zip(host, ins):
        assert_bits_equal(d.cpu().numpy(), a, "an input of the device call")
    b.close()
    assert (bits(got[T]) == bits(SENTINEL)).all(), "the call wrote behind its last frame"
    b2 = capi.Batch(model, n)
    assert_bits_equal(got[:T], extract(b2, c, (1, 5, 2)), "device form against host form")
    b2.close()
    compare(got[:T], want, np.arange(n) % tc.D, "device form")


# ---- d. reset, and the state extraction shares with rnnoise_batch_process ----
def test_reset_between_extraction_and_process(model, want):
    """Extraction advances the batch's ring slot and spectrum parity without counting frames (batch.cpp), seven frames leave both
    rings mid-way (7 is coprime to 6 and 3): after rnnoise_batch_reset the batch is a fresh one, whichever call ran before"""
    from oracle.binding import Oracle
    n, calls = 70, (1, 7)
    c = tc.cycled(n, slice(0, 8))
    src = np.arange(n) % tc.D
    pcm = np.ascontiguousarray(c.noisy)
    seven = tc.cycled(n, slice(8, 15))
    fresh = capi.Batch(model, n)
    rec0 = extract(fresh, c, calls)
    fresh.close()
    compare(rec0, want, src, "fresh batch")
    fresh = capi.Batch(model, n)
    out0, vad0, gains0 = fresh.process(pcm)
    fresh.close()
    # extraction, reset, extraction
    b = capi.Batch(model, n)
    extract(b, seven, (7,))
    b.reset()
    assert_bits_equal(extract(b, c, calls), rec0, "extraction after 7 extraction frames and a reset")
    # process, reset, extraction
    b.reset()
    b.process(np.ascontiguousarray(seven.noisy))
    b.reset()
    assert_bits_equal(extract(b, c, calls), rec0, "extraction after 7 process frames and a reset")
    b.close()
    # extraction, reset, process
    b = capi.Batch(model, n)
    extract(b, seven, (7,))
    b.reset()
    out, vad, gains = b.process(pcm)
    for name, got, ref in (("pcm", out, out0), ("vad", vad, vad0), ("gains", gains, gains0)):
        assert_bits_equal(got, ref, f"process after 7 extraction frames and a reset: {name}")
    for s in (0, 64, n - 1):
        o = Oracle(load_blob("default"))
        r = o.run(pcm[:, s])
        for name, got in (("out", out), ("vad", vad), ("gains", gains)):
            assert_bits_equal(got[:, s], r[name], f"process after extraction and a reset: {name} of stream {s}")
        assert_bits_equal(b.export_state(s), o.get_state(), f"process after extraction and a reset: state of stream {s}")
    b.close()


# ---- e. the tables extraction ignores ----
def test_model_map_controls_and_formats_are_ignored(model, want):
    n = 70
    c = tc.cycled(n, slice(0, 8))
    b = capi.Batch(model, n)
    assert b.add_model(capi.Model(load_blob("little"))) == 1
    b.set_stream_models(np.arange(n) % 2)
    ctl = np.zeros((n, capi.CTL_FLOATS), np.float32)
    ctl[::3] = (0.25, 0.5, 3)
    b.set_stream_controls(ctl)
    b.set_stream_formats(["ulaw" if s % 4 == 0 else "s16" for s in range(n)])
    rec = extract(b, c, (1, 7))
    assert (b.stream_models() == np.arange(n) % 2).all() and (b.stream_formats()[::4] == 1).all()
    b.close()
    plain = capi.Batch(model, n)
    assert_bits_equal(rec, extract(plain, c, (1, 7)), "a batch with a model map, controls and a format table against a plain one")
    plain.close()
    compare(rec, want, np.arange(n) % tc.D, "with tables")


# ---- f. a poisoned stream stays alone ----
def test_poisoned_streams_stay_alone(model, want):
    """NaN and +-Inf in clean and noisy of streams 3, 64 and 129 from frame 2 on (their own records are not specified): lanes of
    three high-pass waves, the last one the batch's last stream"""
    n, bad = 130, (3, 64, 129)
    c = tc.cycled(n, slice(0, 8))
    clean, noisy = c.clean.copy(), c.noisy.copy()
    for x, k in ((clean, 0), (noisy, 11)):
        for s in bad:
            x[2, s, 100 + k] = np.nan
            x[3, s, 7 + k] = np.inf
            x[4:, s, 300 + k:320 + k] = -np.inf
    b = capi.Batch(model, n)
    rec = extract(b, c._replace(clean=clean, noisy=noisy), (1, 7))     # (raises unless the calls return 0)
    b.close()
    compare(rec, want, np.arange(n) % tc.D, "beside poisoned streams", skip=bad)
