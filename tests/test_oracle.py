"""CPU suite, part 1: pin the oracle (oracle/rn_oracle.c).

The reference ships no golden vectors; the pins are
  (a) tests/golden/*.npz -- outputs of the reference's own sources, compiled unmodified by
      oracle/Makefile and recorded through oracle/ref_harness.c (tests/golden/make_golden.py);
  (b) where oracle/_ref exists (build container), the live reference itself; elsewhere the same comparisons read
      its recorded outputs (tests/golden/reference_pins.npz).
Bar: bit-exact on every float and integer, because the int8 quantisers amplify 1-ULP
differences to >1e-4 gain differences.
"""
import os
import zlib

import numpy as np
import pytest

from conftest import both_profiles, ROOT, assert_bits_equal, golden, load_blob, use_rcp_profile
from oracle.binding import Oracle, RefHarness
from rnnoise_amd import synth


def crc_rows(a):
    return np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) & 0xFFFFFFFF for r in a], np.uint32)


@both_profiles
def test_detail_golden(blob_default):
    g = golden("detail_default.npz")
    for s in (3, 77):
        pcm = g[f"s{s}_pcm"]
        # the deterministic generator reproduces the committed input exactly
        assert np.array_equal(synth.stream_pcm(s, 100, lead_silence=12).reshape(100, 480), pcm)
        o = Oracle(blob_default)
        res = o.run(pcm.astype(np.float32))
        for k in ("out", "vad", "gains", "features", "pitch", "pitch_gain", "silence"):
            assert_bits_equal(res[k], g[f"s{s}_{k}"], f"stream {s} {k}")
        assert_bits_equal(o.get_state(), g[f"s{s}_state"], f"stream {s} state")
        assert res["silence"][:12].all() and not res["silence"][13:].any()


@both_profiles
@pytest.mark.parametrize("s", [0, 1, 159, 4095])
def test_digest_golden(blob_default, s):
    g = golden("digest_default.npz")
    pcm = synth.stream_pcm(s, 400, lead_silence=5).reshape(400, 480)
    assert synth.crc32(pcm) == int(g[f"s{s}_pcm_crc"])
    o = Oracle(blob_default)
    res = o.run(pcm.astype(np.float32))
    assert_bits_equal(res["vad"], g[f"s{s}_vad"], "vad")
    assert np.array_equal(res["pitch"], g[f"s{s}_pitch"])
    assert_bits_equal(res["gains"], g[f"s{s}_gains"], "gains")
    assert np.array_equal(crc_rows(res["out"]), g[f"s{s}_out_crc"])
    assert synth.crc32(o.get_state()) == int(g[f"s{s}_state_crc"])


@both_profiles
@pytest.mark.parametrize("case", ["loud", "dc", "impulses", "gaps"])
def test_edge_golden(blob_default, case):
    g = golden("edge_default.npz")
    o = Oracle(blob_default)
    res = o.run(g[f"{case}_pcm"].astype(np.float32))
    assert_bits_equal(res["vad"], g[f"{case}_vad"], "vad")
    assert np.array_equal(res["pitch"], g[f"{case}_pitch"])
    assert np.array_equal(res["silence"], g[f"{case}_silence"])
    assert_bits_equal(res["gains"], g[f"{case}_gains"], "gains")
    assert np.array_equal(crc_rows(res["out"]), g[f"{case}_out_crc"])
    assert synth.crc32(o.get_state()) == int(g[f"{case}_state_crc"])


@both_profiles
@pytest.mark.parametrize("s", [2, 31])
def test_sparser_model_golden(blob_little, s):
    g = golden("digest_little.npz")
    pcm = synth.stream_pcm(s, 200, lead_silence=3).reshape(200, 480)
    assert synth.crc32(pcm) == int(g[f"s{s}_pcm_crc"])
    o = Oracle(blob_little)
    res = o.run(pcm.astype(np.float32))
    assert_bits_equal(res["vad"], g[f"s{s}_vad"], "vad")
    assert np.array_equal(res["pitch"], g[f"s{s}_pitch"])
    assert_bits_equal(res["gains"], g[f"s{s}_gains"], "gains")
    assert np.array_equal(crc_rows(res["out"]), g[f"s{s}_out_crc"])
    assert synth.crc32(o.get_state()) == int(g[f"s{s}_state_crc"])


# ---- known-answer vectors we author ---------------------------------------------
def test_silence_branch_leaves_network_state_untouched(blob_default):
    o = Oracle(blob_default)
    pcm = synth.stream_pcm(9, 30).astype(np.float32).reshape(30, 480)
    o.run(pcm)
    before = o.get_state()
    out, vad, rec = o.process(np.zeros(480, np.float32))
    # the frame is not yet "silent": the analysis window still holds the previous frame
    for _ in range(8):
        out, vad, rec = o.process(np.zeros(480, np.float32))
    assert rec.silence == 1 and vad == 0.0
    mid = o.get_state()
    out, vad, rec = o.process(np.zeros(480, np.float32))
    after = o.get_state()
    from oracle.binding import STATE_FLOATS  # noqa: F401
    # conv/GRU state and lastg frozen on silent frames (src/denoise.c:389-393,474-495)
    sl = slice(2724 - 32, 2724 + 130 + 256 + 3 * 384)
    assert_bits_equal(mid[sl], after[sl], "network state across a silent frame")
    assert not np.array_equal(before[sl], mid[sl])


def test_all_zero_input_is_silent_and_zero(blob_default):
    o = Oracle(blob_default)
    res = o.run(np.zeros((5, 480), np.float32))
    assert res["silence"].all() and not res["vad"].any() and not res["out"].any()
    assert not o.get_state()[2724 - 32:].any()


def test_reset_equivalence_and_first_frame_zero(blob_default):
    pcm = synth.stream_pcm(4, 20).astype(np.float32).reshape(20, 480)
    a = Oracle(blob_default).run(pcm)
    b = Oracle(blob_default).run(pcm)
    assert_bits_equal(a["out"], b["out"], "two fresh states")
    assert not a["out"][0].any()  # delayed_X starts at 0


def test_fft_impulse_dc_sine():
    x = np.zeros(1920, np.float32)
    x[0] = 960.0  # impulse at n=0 -> flat spectrum of 1 (the transform scales by 1/960)
    y = Oracle.fft(x).reshape(960, 2)
    assert np.allclose(y[:, 0], 1.0, atol=1e-6) and np.allclose(y[:, 1], 0.0, atol=1e-6)
    x = np.zeros(1920, np.float32)
    x[0::2] = 1.0  # DC -> bin 0 only
    y = Oracle.fft(x).reshape(960, 2)
    assert abs(y[0, 0] - 1.0) < 1e-6 and np.abs(y[1:]).max() < 1e-6
    n = np.arange(960)
    x = np.zeros(1920, np.float32)
    x[0::2] = np.cos(2 * np.pi * 37 * n / 960)
    y = Oracle.fft(x).reshape(960, 2)
    mag = np.hypot(y[:, 0], y[:, 1])
    assert abs(mag[37] - 0.5) < 1e-5 and abs(mag[960 - 37] - 0.5) < 1e-5
    mag[[37, 960 - 37]] = 0
    assert mag.max() < 1e-5
    rng = np.random.default_rng(5)
    z = rng.standard_normal(1920).astype(np.float32)
    ref = np.fft.fft(z[0::2].astype(np.float64) + 1j * z[1::2].astype(np.float64)) / 960
    y = Oracle.fft(z).reshape(960, 2)
    assert np.abs(y[:, 0] + 1j * y[:, 1] - ref).max() < 1e-6


def test_pitch_of_pulse_train():
    for period in (100, 160, 333, 480):
        buf = np.zeros(1728, np.float32)
        buf[::period] = 10000.0
        buf += np.random.default_rng(period).standard_normal(1728).astype(np.float32)
        T, gain, _ = Oracle.pitch(buf, 0, 0.0)
        # a sub-multiple may legitimately win (octave check), so accept T = period/k within 1 sample
        assert any(abs(T * k - period) <= k for k in (1, 2, 3, 4, 5, 6)) and gain > 0.5, (period, T, gain)


def test_activation_and_quantiser_edges():
    L = Oracle.lib()
    assert L.rno_tanh(0.0) == 0.0 and L.rno_sigmoid(0.0) == 0.5
    assert L.rno_tanh(20.0) == 1.0 and L.rno_tanh(-20.0) == -1.0
    assert L.rno_sigmoid(40.0) == 1.0 and L.rno_sigmoid(-40.0) == 0.0
    xs = np.linspace(-8, 8, 4001, dtype=np.float32)
    t = np.array([L.rno_tanh(float(v)) for v in xs])
    s = np.array([L.rno_sigmoid(float(v)) for v in xs])
    assert np.abs(t - np.tanh(xs)).max() < 6e-4 and np.abs(s - 1 / (1 + np.exp(-xs.astype(np.float64)))).max() < 3e-4
    import ctypes as C
    x = np.array([-2.0, -1.0, -0.5039370, 0.0, 0.003937, 0.5, 1.0, 1.004, 3.0, 300.0, np.nan], np.float32)
    q = np.zeros(len(x), np.uint8)
    L.rno_quantize_u8(q.ctypes.data_as(C.POINTER(C.c_ubyte)), x.ctypes.data_as(C.POINTER(C.c_float)), len(x))
    # 127+round_even(127x), unsigned-saturated twice; 300*127+127 > 32767 wraps to 0 in packus_epi16; NaN -> 0
    assert q.tolist() == [0, 0, 63, 127, 128, 190, 254, 255, 255, 0, 0]


# ---- rcpps profiles (rnnoise_amd/csrc/rcp_profiles.h; reference: src/vec_avx.h:413,442,484,505) ------------------------
def _rcp_table(name):
    import re
    txt = open(os.path.join(ROOT, "rnnoise_amd", "csrc", f"rcp_profile_{name}.h")).read()
    return np.array([int(v) for v in re.findall(r"\d+", txt.split("{", 1)[1].split("}")[0])], np.uint32)


def test_rcp_profiles_are_distinct_and_within_the_instruction_spec():
    """both committed tables stay inside rcpps's documented error (|rel| <= 1.5 * 2^-12) and differ from each other in about
    half of their entries by at most 2 units of 2^-12: the Intel-vs-AMD gap the drop-in has to follow"""
    intel, amd = _rcp_table("intel"), _rcp_table("amd_zen5")
    assert intel.size == 4096 and amd.size == 4096
    x = 1 + np.arange(4096) / 4096
    for t in (intel, amd):
        r = ((t << 11) + 0x3f000000).astype(np.uint32).view(np.float32).astype(np.float64)
        # checked at both ends of each table interval (the entry serves every x with the same top 12 mantissa bits)
        assert max(np.abs(r * x - 1).max(), np.abs(r * (x + 1 / 4096) - 1).max()) <= 1.5 * 2.0 ** -12
    d = amd.astype(int) - intel.astype(int)
    assert 1500 < (d != 0).sum() < 3000 and np.abs(d).max() <= 2
    assert np.array_equal(intel[0::2], intel[1::2]), "Intel's rcpps depends on 11 mantissa bits only"
    assert not np.array_equal(amd[0::2], amd[1::2]), "Zen 5's needs all 12"


@pytest.mark.parametrize("name", ["intel", "amd-zen5", "host"])
def test_oracle_rcp_follows_the_selected_profile(name):
    from oracle import binding
    binding.set_rcp_profile(name)
    L = Oracle.lib()
    if name != "host":
        t = _rcp_table(name.replace("-", "_"))
        assert binding.rcp_profile() == name
        for xb in (0x3f800000, 0x3f800800, 0x3fc00000 | (1234 << 11) | 77, 0x447a0000, 0x3a83126f):
            want = ((int(t[(xb >> 11) & 0xfff]) << 11) + 0x3f000000 - ((xb & 0x7f800000) - 0x3f800000)) & 0xffffffff
            got = np.float32(L.rno_rcp(float(np.uint32(xb).view(np.float32)))).view(np.uint32)
            assert int(got) == want
    else:  # this CPU: the captured table reproduces the instruction wherever we probe it (numpy has no rcpps; 1/x is within spec)
        for v in (1.0, 1.37, 952.7, 1e-3, 6.02e4):
            assert abs(L.rno_rcp(v) * v - 1) <= 1.5 * 2.0 ** -12


def test_profiles_move_the_gains_by_less_than_the_activation_error(blob_default):
    """measured size of the Intel-vs-AMD gap on a free-running stream (recorded in DESIGN.md section 2)"""
    from oracle import binding
    pcm = synth.stream_pcm(11, 120, lead_silence=3).astype(np.float32).reshape(120, 480)
    binding.set_rcp_profile("intel")
    a = Oracle(blob_default).run(pcm)
    binding.set_rcp_profile("amd-zen5")
    b = Oracle(blob_default).run(pcm)
    dg = np.abs(a["gains"] - b["gains"])
    assert 0 < dg.max() < 0.05 and not np.array_equal(a["out"], b["out"])
    assert np.array_equal(a["features"][:5], b["features"][:5])  # the DSP front end does not depend on the profile
    print(f"intel vs amd-zen5 over 120 frames: max |dgain| {dg.max():.2e}, mean {dg.mean():.2e}; "
          f"max |dvad| {np.abs(a['vad'] - b['vad']).max():.2e}; max |dpcm| {np.abs(a['out'] - b['out']).max():.3f}")


# ---- the reference itself: live where oracle/_ref is built, otherwise its recorded outputs -------------------------------
def reference_pins():
    """tests/golden/reference_pins.npz (tests/golden/make_golden.py): the reference's outputs for the tests below, recorded on
    the host named in the file.  The oracle is switched to that host's rcpps profile, which the stored outputs belong to."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_pins.npz"))
    use_rcp_profile(str(g["rcp_profile"]))
    return g


def test_tables_match_reference_bit_for_bit():
    if RefHarness.available():
        want = RefHarness.tables()
    else:
        g = reference_pins()
        want = [g[f"tables_{k}"] for k in ("window", "dct", "twiddles", "bitrev")]
    for a, b, name in zip(Oracle.tables(), want, ("window", "dct", "twiddles", "bitrev")):
        assert_bits_equal(a, b, name)


@pytest.mark.rcp("host")  # the compiled reference executes this CPU's rcpps: the oracle must carry this CPU's table
def test_live_reference_free_running(blob_default):
    pcm = synth.stream_pcm(11, 250, lead_silence=7).astype(np.float32).reshape(250, 480)
    if RefHarness.available():
        r = RefHarness(blob_default)
        assert r.L.refh_arch(r.h) == 2, "host must select the AVX2 code path (src/x86/x86cpu.c)"
        want = r.run(pcm)
        want_state = r.get_state()
    else:
        g = reference_pins()
        want = {k[5:]: g[k] for k in g.files if k.startswith("free_") and k != "free_state"}
        want_state = g["free_state"]
    o = Oracle(blob_default)
    a = o.run(pcm)
    a["out_crc"] = crc_rows(a["out"])
    assert set(want) - set(a) == set()
    for k in want:
        assert_bits_equal(a[k], want[k], k)
    assert_bits_equal(o.get_state(), want_state, "state")


def test_live_reference_fft_and_pitch():
    g = None if RefHarness.available() else reference_pins()
    rng = np.random.default_rng(3)
    for i in range(4):
        x = (rng.standard_normal(1920) * 3000).astype(np.float32)
        assert_bits_equal(Oracle.fft(x), RefHarness.fft(x) if g is None else g[f"fft{i}"], "fft")
        buf = (rng.standard_normal(1728) * 2000).astype(np.float32)
        a = Oracle.pitch(buf, 200, 0.4)
        b = RefHarness.pitch(buf, 200, 0.4) if g is None else (g[f"pitch{i}_period"], g[f"pitch{i}_gain"], g[f"pitch{i}_x_lp"])
        assert a[0] == b[0]
        assert_bits_equal(np.float32(a[1]), np.float32(b[1]), "pitch gain")
        assert_bits_equal(a[2], b[2], "x_lp")


@pytest.mark.rcp("host")
def test_live_reference_teacher_forced_state_import(blob_default):
    """state exported from the reference mid-stream drives the oracle to the same next frame"""
    pcm = synth.stream_pcm(21, 60).astype(np.float32).reshape(60, 480)
    if RefHarness.available():
        r = RefHarness(blob_default)
        r.run(pcm[:40])
        state = r.get_state()
        want = r.run(pcm[40:])
    else:
        g = reference_pins()
        state = g["forced_state"]
        want = {k[7:]: g[k] for k in g.files if k.startswith("forced_") and k != "forced_state"}
    o = Oracle(blob_default)
    o.set_state(state)
    a = o.run(pcm[40:])
    assert set(a) == set(want)
    for k in a:
        assert_bits_equal(a[k], want[k], k)


@pytest.mark.skipif(not RefHarness.available(), reason="oracle/_ref not built (needs the reference sources at build time)")
def test_reference_pins_are_the_reference():
    """the recorded outputs above are what the compiled reference computes, where it runs on a host of the recording's
    rcpps profile (tests/golden/make_golden.py --pins)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_pins.npz"))
    from oracle import binding
    binding.set_rcp_profile("host")
    if binding.rcp_profile() != str(g["rcp_profile"]):
        pytest.skip(f"pins recorded on the {g['rcp_profile']} profile, this host is {binding.rcp_profile()}")
    for k, v in zip(("window", "dct", "twiddles", "bitrev"), RefHarness.tables()):
        assert_bits_equal(v, g[f"tables_{k}"], k)
    blob = load_blob("default")
    r = RefHarness(blob)
    res = r.run(synth.stream_pcm(11, 250, lead_silence=7).astype(np.float32).reshape(250, 480))
    assert np.array_equal(crc_rows(res["out"]), g["free_out_crc"])
    for k in ("vad", "gains", "features", "pitch", "pitch_gain", "silence"):
        assert_bits_equal(res[k], g[f"free_{k}"], k)
    assert_bits_equal(r.get_state(), g["free_state"], "state")


# ---- the mixed block of tests/stream_mix.py: what every at-size GPU test trusts the oracle on ----
_REF_BLOCK = {}


def _reference_block(run):
    """one run of stream_mix.block_pin_runs() through the compiled reference, once per module"""
    import stream_mix
    tag, name, positions, scheduled = run
    if tag not in _REF_BLOCK:
        _REF_BLOCK[tag] = stream_mix.block_run(load_blob(name), positions, scheduled, engine=RefHarness)
    return _REF_BLOCK[tag]


@pytest.mark.rcp("host")  # the compiled reference executes this CPU's rcpps; the pins belong to the profile of the host that wrote them
@pytest.mark.parametrize("which", range(4), ids=["default_lock", "default_sched", "little_lock", "little_sched"])
def test_the_mixed_block_is_the_reference(which):
    """The block that the at-size tests compare the GPU with -- 389 positions x 30 frames: pitch from 60 to 767, silence that flips at
    call boundaries, zero runs, threshold noise, denormals, +-3e6 sines -- through the reference and through the oracle, position by
    position: in lock step and on each position's present frames under stream_mix.presence() with a fresh state at RESET's restart; on
    the default model, and on the sparser one for 40 of the positions that take it under the link dressing.  Bit identity in out, vad,
    gains, features, pitch, silence and final state: live where oracle/_ref is built, else against the recorded digests
    (tests/golden/block_pins.npz, make_golden.py --block-pins)."""
    import stream_mix
    run = stream_mix.block_pin_runs()[which]
    tag, name, positions, scheduled = run
    assert tag == ["default_lock", "default_sched", "little_lock", "little_sched"][which]
    if RefHarness.available():
        want = _reference_block(run)
        got = stream_mix.block_run(load_blob(name), positions, scheduled)
        assert set(got) == set(want)
        for k in ("out", "vad", "gains", "features", "pitch", "silence", "state"):
            assert_bits_equal(got[k], want[k], f"{tag}: {k}")
        return
    g = golden("block_pins.npz")
    assert g[f"{tag}_positions"].tolist() == positions
    got = stream_mix.block_digest(stream_mix.block_run(load_blob(name), positions, scheduled))
    assert set(got) == set(stream_mix.PIN_KEYS)
    for k, v in got.items():
        pin = g[f"{tag}_{k}"]
        assert v.dtype == pin.dtype
        assert_bits_equal(v, pin, f"{tag}: {k}")


@pytest.mark.rcp("host")  # (as above)
@pytest.mark.parametrize("which", range(3), ids=["16000_int16", "32000_float", "48000_int16"])
def test_the_chunk_dressings_oracle_inputs_are_the_reference(which):
    """The chunk expectation of the at-size tests (stream_mix.chunk_expectation) rests on the oracle over signals that the runs above do
    not contain: the block rounded to int16, and resample.up of the block brought down to 16 kHz (rounded to int16) and to 32 kHz.  All
    389 positions of each in lock step on the default model, through the reference and through the oracle: bit identity in out, vad,
    gains, features, pitch, silence and final state, live where oracle/_ref is built, else against the recorded digests
    (tests/golden/block_pins.npz, make_golden.py --block-pins)."""
    import stream_mix
    tag, hz, typ = stream_mix.chunk_pin_runs()[which]
    assert tag == ["chunk_16000_int16", "chunk_32000_float", "chunk_48000_int16"][which]
    got = stream_mix.chunk_pin_run(load_blob("default"), hz, typ)
    if RefHarness.available():
        want = stream_mix.chunk_pin_run(load_blob("default"), hz, typ, engine=RefHarness)
        assert set(got) == set(want)
        for k in ("out", "vad", "gains", "features", "pitch", "silence", "state"):
            assert_bits_equal(got[k], want[k], f"{tag}: {k}")
        return
    g = golden("block_pins.npz")
    digest = stream_mix.chunk_pin_digest(got)
    assert set(digest) == set(stream_mix.CHUNK_PIN_KEYS)
    for k, v in digest.items():
        pin = g[f"{tag}_{k}"]
        assert v.dtype == pin.dtype
        assert_bits_equal(v, pin, f"{tag}: {k}")


@pytest.mark.skipif(not RefHarness.available(), reason="oracle/_ref not built (needs the reference sources at build time)")
def test_block_pins_are_the_reference():
    """the recorded digests of the block are what the compiled reference computes, where it runs on a host of the recording's rcpps
    profile (tests/golden/make_golden.py --block-pins)"""
    import stream_mix
    from oracle import binding
    binding.set_rcp_profile("host")
    prof = binding.rcp_profile()
    path = os.path.join(ROOT, "tests", "golden", *(() if prof == "intel" else (prof.replace("-", "_"),)), "block_pins.npz")
    if not os.path.exists(path):
        pytest.skip(f"no block_pins.npz fixture for the {prof} profile")
    g = np.load(path)
    assert str(g["rcp_profile"]) == prof
    runs = stream_mix.block_pin_runs()
    chunk_runs = stream_mix.chunk_pin_runs()
    assert {k for k in g.files if k not in ("rcp_profile", "host_cpu")} == (
        {f"{t}_{k}" for t, *_ in runs for k in stream_mix.PIN_KEYS + ("positions",)} | {f"{t}_{k}" for t, *_ in chunk_runs for k in stream_mix.CHUNK_PIN_KEYS})
    for tag, hz, typ in chunk_runs:
        ref = stream_mix.chunk_pin_run(load_blob("default"), hz, typ, engine=RefHarness)
        for k, v in stream_mix.chunk_pin_digest(ref).items():
            assert v.dtype == g[f"{tag}_{k}"].dtype
            assert_bits_equal(v, g[f"{tag}_{k}"], f"{tag}: {k}")
    for run in runs:
        tag, _, positions, _ = run
        assert g[f"{tag}_positions"].tolist() == positions
        for k, v in stream_mix.block_digest(_reference_block(run)).items():
            assert v.dtype == g[f"{tag}_{k}"].dtype
            assert_bits_equal(v, g[f"{tag}_{k}"], f"{tag}: {k}")


def test_x86_float_to_short_model_matches_the_compiler(tmp_path):
    """The int16 entry points (include/rnnoise_amd.h: rnnoise_batch_process_s16) convert on the device "as the reference's only
    caller does" (examples/rnnoise_demo.c:58: tmp[i] = x[i], float -> short).  Out of range that cast is undefined in C; what
    the demo's binary DOES on x86-64 is cvttss2si / cvttps2dq to 32 bits ("integer indefinite" 0x80000000 when out of range or
    NaN) and the low 16 bits of that.  This pins the model the GPU tests compare with (tests/test_gpu_parity.py:
    x86_float_to_short) to what gcc emits on this host, scalar and vectorised."""
    import ctypes as C
    import subprocess
    if os.uname().machine != "x86_64":
        pytest.skip("x86 cast semantics")
    src = tmp_path / "cast.c"
    src.write_text("void cast_loop(const float *x, short *y, int n) { for (int i = 0; i < n; i++) y[i] = x[i]; }\n"
                   "short cast_one(float x) { return x; }\n")
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-40000, 40000, 4096), rng.uniform(-3e9, 3e9, 4096), rng.uniform(-1e6, 1e6, 4096),
                        [0.0, -0.0, 0.999, -0.999, 32767.5, -32768.5, 65535.9, 2147483520.0, 2147483648.0, -2147483648.0,
                         -2147483904.0, 1e20, -1e20, np.inf, -np.inf, np.nan]]).astype(np.float32)
    ok = (x >= np.float32(-2147483648.0)) & (x < np.float32(2147483648.0))
    model = (np.where(ok, np.trunc(np.where(ok, x, 0)), -2147483648.0).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)
    for opt in ("-O0", "-O2", "-O3 -mavx2"):
        so = tmp_path / f"cast{opt.replace(' ', '')}.so"
        subprocess.check_call(["gcc", *opt.split(), "-shared", "-fPIC", str(src), "-o", str(so)])
        L = C.CDLL(str(so))
        y = np.empty(x.size, np.int16)
        L.cast_loop(x.ctypes.data_as(C.POINTER(C.c_float)), y.ctypes.data_as(C.POINTER(C.c_short)), x.size)
        assert np.array_equal(y, model), (opt, np.argwhere(y != model)[:5].tolist())
        L.cast_one.restype = C.c_short
        L.cast_one.argtypes = [C.c_float]
        assert all(L.cast_one(float(v)) == int(m) for v, m in zip(x[-16:-1], model[-16:-1])), opt
