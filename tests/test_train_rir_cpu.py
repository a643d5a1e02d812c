"""The RIR calls without a GPU (include/rnnoise_amd.h: RNNoiseTrainRir; the reference's src/dump_features.c:51-144, :449-465).

  a  tests/csrc/rir_oracle.c -- what the GPU tests compare against -- equals the reference's own kiss_fft tables, load_rir and
     rir_filter_sequence (tests/csrc/ref_dump_harness.c, compiled where the reference's sources are), bit for bit
  b  the oracle itself: half a double-precision convolution within the fp32 error of its transforms; blocks independent of later input
  c  rnnoise_amd_train_rir_check, the -1 returns that need no device, the struct's layout, train_data.draw_rir
  d  the kernels' own source run on the host under the address sanitizer (tests/csrc/hip_emul), against the oracle
(the kernels of train_rir.hip by name, their registers, no scratch, no flat accesses: tests/test_product_surface_cpu.py,
tests/test_kernel_budgets_cpu.py)"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rir_oracle as ro
from conftest import GOLD, ROOT, assert_bits_equal
from rnnoise_amd import capi, train_data
from train_support import NFFT_REF, T_REF, reference_dump_features, run_kernel_emul

assert ro.NFFT == NFFT_REF


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the reference's functions (tests/csrc/ref_dump_harness.c: train_support.reference_dump_features)"""
    L = reference_dump_features(tmp_path_factory.mktemp("ref_dump"))
    if isinstance(L, str):
        pytest.skip(L)
    return L


def ref_tables(L):
    tw, rev, fac = np.empty((ro.NFFT, 2), np.float32), np.empty(ro.NFFT, np.int32), np.empty(16, np.int32)
    L.refr_tables(_fp(tw), rev.ctypes.data_as(C.POINTER(C.c_int)), fac.ctypes.data_as(C.POINTER(C.c_int)))
    return tw, rev, fac


def ref_load(L, tmp_path, h, early):
    path = os.path.join(str(tmp_path), "rir.f32")
    np.asarray(h, np.float32).tofile(path)
    spec = np.empty((ro.NFFT, 2), np.float32)
    L.refr_load_rir(str(path).encode(), early, _fp(spec))
    return spec


def ref_filter(L, audio, spec):
    y = np.array(audio, np.float32)
    assert y.shape == (T_REF * 480,)
    L.refr_filter(_fp(y), _fp(np.ascontiguousarray(spec, np.float32)))
    return y


def reference_recipe():
    """the seeded inputs of tests/golden/train_rir_reference.npz: one response, a clean and a noisy 2000-frame signal"""
    return ro.response(12000, 41), ro.signal(T_REF, 42, 2000.0), ro.signal(T_REF, 43, 6000.0)


# the samples the fixture keeps: around the borders of blocks 1, 2, 15 and 29 and the sequence's ends
BORDER_SAMPLES = np.concatenate([np.arange(0, 40)] + [np.arange(b * ro.BLOCK - 40, b * ro.BLOCK + 40) for b in (1, 2, 15, 29)]
                                + [np.arange(T_REF * 480 - 40, T_REF * 480)])


# ---- a. the oracle against the reference ----
def test_oracle_tables_are_the_references(ref):
    tw, rev, fac = ref_tables(ref)
    assert list(fac) == [4, 16384, 4, 4096, 4, 1024, 4, 256, 4, 64, 4, 16, 4, 4, 4, 1]
    assert_bits_equal(ro.twiddles(), tw, "twiddles")
    assert (ro.bitrev() == rev).all()


@pytest.mark.parametrize("length", ro.RIR_LENS)
def test_oracle_load_rir_is_the_references(ref, tmp_path, length):
    h = ro.response(length, 7)
    for early in (0, 1):
        want = ref_load(ref, tmp_path, h, early)
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert_bits_equal(ro.load(h, early), want, f"len {length} early {early}")
    if length <= 720:  # (nothing of the response lies behind the early form's end: only the fade can differ)
        assert (ro.load(h, 0) == ro.load(h, 1)).all() == (length <= 481)   # (sample 480 is faded by the factor 1)


def test_oracle_load_rir_keeps_denormals_as_the_reference_does(ref, tmp_path):
    h = ro.denormal_tail_response()
    spec = ref_load(ref, tmp_path, h, 0)
    assert_bits_equal(ro.load(h, 0), spec, "denormal tail")
    assert_bits_equal(ro.load(h, 1), ref_load(ref, tmp_path, h, 1), "denormal tail, early")
    # the scaled input has denormal samples, and flushing them would change the spectrum's bits
    x = np.zeros((ro.NFFT, 2), np.float32)
    x[:len(h), 0] = h
    scaled = np.float32(1 / 65536) * x[:, 0]
    tiny = (scaled != 0) & (np.abs(scaled) < np.finfo(np.float32).tiny)
    assert tiny.sum() > 100
    x[tiny, 0] = 0
    assert (ro.fft(x) != spec).any()


@pytest.mark.parametrize("name", ["realistic", "beyond int16", "zero"])
def test_oracle_filter_is_the_references_at_2000_frames(ref, tmp_path, name):
    h = ro.response(20000, 11)
    x = {"realistic": ro.signal(T_REF, 1), "beyond int16": ro.signal(T_REF, 2, 30000.0), "zero": np.zeros(T_REF * 480, np.float32)}[name]
    if name == "beyond int16":
        assert np.abs(x).max() > 40000
    for early in (0, 1):
        spec = ref_load(ref, tmp_path, h, early)
        want = ref_filter(ref, x, spec)
        assert name == "zero" or np.abs(want).max() > 1000
        assert_bits_equal(ro.filter(x, spec), want, f"{name} early {early}")


def record_reference(L, where):
    """what tests/golden/train_rir_reference.npz holds, from the reference itself (tests/golden/make_train_rir_reference.py writes it)"""
    h, clean, noisy = reference_recipe()
    yc = ref_filter(L, clean, ref_load(L, where, h, 1))
    yn = ref_filter(L, noisy, ref_load(L, where, h, 0))
    sha = lambda a: np.array(hashlib.sha256(a.tobytes()).hexdigest())
    return dict(twiddles_sha256=sha(ref_tables(L)[0]), clean_sha256=sha(yc), noisy_sha256=sha(yn), at=BORDER_SAMPLES,
                clean_at=yc[BORDER_SAMPLES], noisy_at=yn[BORDER_SAMPLES])


def test_reference_fixture_is_the_references(ref, tmp_path):
    """tests/golden/train_rir_reference.npz, which the GPU test compares against where the reference is not: recorded from the
    reference through the harness, and still what the reference gives"""
    g = np.load(os.path.join(GOLD, "train_rir_reference.npz"))
    now = record_reference(ref, tmp_path)
    assert sorted(g.files) == sorted(now)
    for k, v in now.items():
        assert g[k].dtype == v.dtype and g[k].tobytes() == v.tobytes(), k


def test_reference_fixture_twiddles_are_this_hosts():
    """(must not skip where the fixture was recorded: the twiddles are the host libm's)"""
    g = np.load(os.path.join(GOLD, "train_rir_reference.npz"))
    assert hashlib.sha256(ro.twiddles().tobytes()).hexdigest() == str(g["twiddles_sha256"])


# ---- b. the oracle itself ----
# Bound on the oracle's distance from half the exact convolution.  A radix-2-equivalent FFT of 2^16 points in arithmetic of unit
# roundoff u = 2^-24 with twiddles of relative error <= u has, after Higham (Accuracy and Stability of Numerical Algorithms, Thm 24.2),
# |err|_2 <= 16 eta / (1 - 16 eta) |y|_2 with eta = u + gamma_4 (sqrt(2) + u) ~= 6.66 u: 107 u per transform (a radix-4 stage does
# the work of two radix-2 stages with fewer roundings, so the bound holds for it).  A block goes through three transforms -- the
# signal's, the response's, the inverse -- and one complex product (sqrt(2) gamma_2 < 3 u): (3 * 107 + 3) u = 324 u of the circular
# convolution's 2-norm, which is at most max|H| |x_window|_2 (the exact scalings by 1/65536 and 32768 add nothing).  Every sample
# lies in two windows, so over a sequence |err|_2 <= 324 u * max|H| * sqrt(2) |x|_2; the maximum error is no larger than the 2-norm.
# Observed (this file, the five lengths): at most 0.43 u in those units -- rounding errors add like a random walk, not in line.
U = 2.0 ** -24
BOUND_U = 324


def _exact_half_convolution(x, h):
    if len(x) * len(h) < 1e8:
        y = np.convolve(x.astype(np.float64), h.astype(np.float64))
    else:  # (in double through a transform of its own: error 1e-16, nine orders below what is measured here)
        n = 1 << int(np.ceil(np.log2(len(x) + len(h))))
        y = np.fft.irfft(np.fft.rfft(x.astype(np.float64), n) * np.fft.rfft(h.astype(np.float64), n), n)
    return .5 * y[:len(x)]


@pytest.mark.parametrize("n_frames", [1, 7, 69, 137, 300])
def test_oracle_is_half_the_convolution(n_frames):
    h = ro.response(600 if n_frames == 1 else 9000, 3)
    x = ro.signal(n_frames, 5)
    got = ro.filter(x, ro.load(h, 0)).astype(np.float64)
    want = _exact_half_convolution(x, h)
    assert np.abs(want).max() > 1000
    H = np.abs(np.fft.fft(h.astype(np.float64), ro.NFFT)).max()
    unit = H * np.sqrt(2) * np.linalg.norm(x.astype(np.float64))
    err = np.linalg.norm(got - want) / unit / U
    print(f"n_frames {n_frames}: |err|_2 = {err:.3f} u, max |err| = {np.abs(got - want).max():.3g} on values up to {np.abs(want).max():.0f}")
    assert err <= BOUND_U and np.abs(got - want).max() <= BOUND_U * U * unit


def test_oracle_blocks_do_not_depend_on_later_input():
    """A block's output is a function of its window, the previous block and its own, so every COMPLETE block of a short run has the
    bits of the same block in a longer run.  The short run's last, partial block is padded with zeros where the longer run has
    input: the samples it keeps are the same convolution, but the rounding errors of a transform depend on its whole window, so
    there the two runs agree only within the bound above (271 of the 352 samples of the 69-frame run differ in their last bits)."""
    h, x = ro.response(9000, 3), ro.signal(300, 6)
    spec = ro.load(h, 1)
    long = ro.filter(x, spec)
    unit = np.abs(np.fft.fft(h[:720].astype(np.float64), ro.NFFT)).max() * np.sqrt(2) * np.linalg.norm(x.astype(np.float64))
    for n_frames in (69, 137):   # (both end inside a block)
        n = n_frames * 480
        whole = n // ro.BLOCK * ro.BLOCK
        assert 0 < whole < n
        short = ro.filter(x[:n], spec)
        assert_bits_equal(short[:whole], long[:whole], f"{n_frames} frames")
        assert np.abs(short[whole:].astype(np.float64) - long[whole:n]).max() <= 2 * BOUND_U * U * unit


def test_oracle_clip_quantize():
    x = np.array([-40000, -32767.5, -32767, -.5, -.49, 0, .49, .5, 1.5, 32766.6, 32767, 32767.2, 1e9], np.float32)
    assert list(ro.clip_quantize(x, 1, 0)) == [-32767, -32767, -32767, -.5, np.float32(-.49), 0, np.float32(.49), .5, 1.5,
                                                np.float32(32766.6), 32767, 32767, 32767]
    assert list(ro.clip_quantize(x, 0, 1)) == [-40000, -32767, -32767, 0, 0, 0, 0, 1, 2, 32767, 32767, 32767, 1e9]
    assert list(ro.clip_quantize(x, 1, 1)) == [-32767, -32767, -32767, 0, 0, 0, 0, 1, 2, 32767, 32767, 32767, 32767]
    assert (ro.clip_quantize(x, 0, 0) == x).all()


# ---- c. the check, the -1 returns, the struct, draw_rir ----
def _records(ids, clip=0, quantize=0):
    t = np.zeros(len(ids), capi.RIR_DTYPE)
    t["rir_id"], t["clip"], t["quantize"] = ids, clip, quantize
    return t


def test_check_accepts_the_boundaries_and_refuses_beyond():
    assert capi.train_rir_check(_records([-1, 0, 4, 4, 2], [0, 1, 0, 1, 1], [1, 0, 0, 1, 0]), 5)
    assert capi.train_rir_check(_records([-1, -1]), 0)          # nothing filtered: no list needed
    for ids, n_rirs in (([0, 5], 5), ([-2], 5), ([0], 0), ([2 ** 31 - 1], 5), ([0], -1)):
        assert not capi.train_rir_check(_records(ids), n_rirs), (ids, n_rirs)
    for name in ("clip", "quantize"):
        for v, good in ((1, True), (2, False), (-1, False)):
            t = _records([0, -1, 1])
            t[name][1] = v
            assert capi.train_rir_check(t, 2) == good, (name, v)
    L = capi.lib()
    assert L.rnnoise_amd_train_rir_check(None, 1, 1) == 0
    assert L.rnnoise_amd_train_rir_check(_records([0]).ctypes.data, 0, 1) == 0


def test_work_bytes():
    one = capi.train_rir_work_bytes(1)
    assert one == 2 * ro.NFFT * 8                   # a transform pair: two complex arrays of 65,536 points
    assert capi.train_rir_work_bytes(4096 * 60) == 4096 * 60 * one > 2 ** 31
    assert capi.train_rir_work_bytes(0) == capi.train_rir_work_bytes(-3) == 0


def test_calls_fail_without_a_batch_or_an_argument():
    """(the other -1 returns need a batch: tests/test_train_rir_gpu.py)"""
    L = capi.lib()
    assert {"rnnoise_amd_train_rir_check", "rnnoise_amd_train_rir_work_bytes", "rnnoise_batch_train_rir_load_device",
            "rnnoise_batch_train_rir_device"} <= set(capi.EXPORTS)
    t, lens = _records([0]), np.array([100], np.int32)
    lp = lens.ctypes.data_as(C.POINTER(C.c_int))
    p = 4096  # (never dereferenced: the batch is checked first)
    assert L.rnnoise_batch_train_rir_load_device(None, p, p, lp, 1, None) == -1
    assert L.rnnoise_batch_train_rir_device(None, p, p, p, 1, t.ctypes.data, p, 1 << 20, 2, None) == -1


def test_struct_layout_is_the_headers(tmp_path):
    names = [f[0] for f in capi.TrainRir._fields_]
    prog = tmp_path / "probe.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnnoise_amd.h"\nint main(void) {\n'
                    '  printf("%zu\\n", sizeof(RNNoiseTrainRir));\n'
                    + "".join(f'  printf("%zu\\n", offsetof(RNNoiseTrainRir, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(capi.TrainRir) == capi.RIR_DTYPE.itemsize == 12
    assert out[1:] == [getattr(capi.TrainRir, n).offset for n in names] == [capi.RIR_DTYPE.fields[n][1] for n in names]


def test_draw_rir_frequencies_and_range():
    n, n_rirs = 40000, 7
    rec = train_data.draw_rir(np.random.default_rng(3), n, n_rirs)
    assert rec.dtype == capi.RIR_DTYPE and rec.shape == (n,) and capi.train_rir_check(rec, n_rirs)
    assert (rec["clip"] == 0).all() and (rec["quantize"] == 0).all()
    ids = rec["rir_id"]
    assert ids.min() == -1 and ids.max() == n_rirs - 1

    def near(count, total, p, what):
        sd = np.sqrt(total * p * (1 - p))
        assert abs(count - total * p) <= 5 * sd, (what, count, total * p, sd)
    near((ids >= 0).sum(), n, 1 / 2, "applied")
    for k in range(n_rirs):
        near((ids == k).sum(), (ids >= 0).sum(), 1 / n_rirs, f"id {k}")
    assert set(train_data.draw_rir(np.random.default_rng(4), 500, 1)["rir_id"]) == {-1, 0}
    with pytest.raises(ValueError):
        train_data.draw_rir(np.random.default_rng(4), 5, 0)


def test_draw_is_unchanged_by_draw_rir():
    lens, T = (10 ** 6, 2 * 10 ** 6, 10 ** 7), 50
    a = train_data.draw(np.random.default_rng(9), 300, lens, T)
    rng = np.random.default_rng(9)
    b = train_data.draw(rng, 300, lens, T)
    train_data.draw_rir(rng, 300, 4)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert train_data.N_UNIFORM == 41
    # ... and a generator that has served draw() serves draw_rir() from its next numbers: the command line's order
    want = np.random.default_rng(9)
    want.random((300, train_data.N_UNIFORM))
    u = want.random((300, 2))
    assert ((train_data.draw_rir(np.random.default_rng(9), 300, 4)["rir_id"] >= 0) != (u[:, 0] < .5)).any()   # (another position in the stream)
    rng = np.random.default_rng(9)
    train_data.draw(rng, 300, lens, T)
    assert ((train_data.draw_rir(rng, 300, 4)["rir_id"] >= 0) == (u[:, 0] < .5)).all()


# ---- d. the kernels' own source on the host ----
def test_kernel_source_on_the_host_stays_inside_its_buffers_and_gives_the_oracles_bits(tmp_path):
    """train_rir.hip compiled as plain C++ against a stand-in for shim.h (256 host threads per workgroup), a stand-alone program under
    the address and undefined-behaviour sanitizers: frames, responses, spectra and a one-unit workspace of exact size; two responses
    through the loader, then 3 sequences (two filtered, one only clipped and quantised) of 7 and of 69 frames"""
    r = run_kernel_emul(tmp_path, "train_rir", "rir_main.cpp", "rir_oracle.c")
    assert r.returncode == 0 and r.stdout.strip().endswith("all equal"), r.stdout[-2000:] + r.stderr[-4000:]
