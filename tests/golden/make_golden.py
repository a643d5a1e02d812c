#!/usr/bin/env python3
"""Generate the golden fixtures from the REFERENCE ITSELF (run in the build container only).

The reference has no tests and no golden vectors, so the pin is: the
reference's own sources, compiled unmodified by oracle/Makefile (pinned build, SURVEY fact
8) on this host, driven through oracle/ref_harness.c with the synthetic default-architecture
model exported by the reference's own exporter (oracle/gen_model.py).  Everything written
here is reference OUTPUT; no reference code is involved in producing the files other than by
running it.

  tests/golden/default.blob.xz   -- the "DNNw" weight blob (src/write_weights.c format)
  tests/golden/little.blob.xz    -- higher-sparsity variant (rnnoise_data_little stand-in)
  tests/golden/detail_default.npz-- 2 streams x 100 frames, everything per frame + final state
  tests/golden/digest_default.npz-- 4 streams x 400 frames: vad, pitch, raw gains, CRC32 of PCM out
  tests/golden/edge_default.npz  -- loud noise / DC / impulses / gaps, 60 frames each
  tests/golden/digest_little.npz -- 2 streams x 200 frames on the sparser model
  tests/golden/reference_pins.npz-- what tests/test_oracle.py's and tests/test_train_features.py's reference comparisons
                                    read where oracle/_ref is not built: tables, FFT / pitch search, a free-running and a
                                    teacher-forced stream, training features (`make_golden.py --pins [OUTDIR]` writes only it)
                                    "trainedge<i>": (16, 98) records of stream i of tests/train_cases.py: edge_subset(), the band
                                    limits at and beyond the ends of their ranges.  Keys the file already holds must come out
                                    bit-identical, or nothing is written

  tests/golden/block_pins.npz    -- the mixed block of tests/stream_mix.py through the reference (`make_golden.py --block-pins
                                    [OUTDIR]` writes only it): per run of stream_mix.block_pin_runs() -- every position on the
                                    default model, 40 on the sparser one, in lock step and under the presence schedule with its
                                    restarts -- CRC32 per (frame, position) of out, gains and features, vad, pitch, silence and one
                                    CRC32 of the final state per position; and per run of stream_mix.chunk_pin_runs() -- the oracle inputs
                                    of the chunk dressing: the block rounded to int16, and brought to 16 and 32 kHz and back up, every
                                    position in lock step -- one CRC32 per (frame, position) over all of those, and the state's.  Keys the file already
                                    holds must come out bit-identical, or nothing is written

The reference's tanh / sigmoid execute the generating CPU's `rcpps` (src/vec_avx.h:413,442), so a fixture belongs to one
CPU family and says which ("rcp_profile", "host_cpu" entries).  The Intel build host writes tests/golden/*.npz; run on the
GPU boxes' AMD EPYC host (the compiled reference under oracle/_ref travels there) the same script writes the same streams
into tests/golden/amd_zen5/ -- `python tests/golden/make_golden.py [OUTDIR]`.

Usage:  make -C oracle ref && python tests/golden/make_golden.py
"""
import lzma
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import binding  # noqa: E402
from oracle.binding import RefHarness, RefTrainHarness  # noqa: E402
from rnnoise_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def crc_rows(a):
    return np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) & 0xFFFFFFFF for r in a], np.uint32)


def edge_inputs():
    rng = np.random.Generator(np.random.PCG64(99))
    T = 60
    loud = rng.integers(-32768, 32767, size=(T, 480)).astype(np.int16)
    dc = np.full((T, 480), 12000, np.int16)
    imp = np.zeros((T, 480), np.int16)
    imp[::7, 13] = 30000
    gaps = synth.stream_pcm(5, T).reshape(T, 480).copy()
    gaps[20:35] = 0
    gaps[45:50] //= 1000
    return dict(loud=loud, dc=dc, impulses=imp, gaps=gaps)


def host_profile():
    """The reference executes this CPU's rcpps (src/vec_avx.h:413,442): its outputs belong to one CPU family, and every
    fixture says which (rnnoise_amd/csrc/rcp_profiles.h).  A host whose table is neither built-in one cannot make goldens."""
    binding.set_rcp_profile("host")
    name = binding.rcp_profile()
    assert name in ("intel", "amd-zen5"), "this CPU's rcpps matches no committed profile: capture it first (oracle/rcp_capture.c)"
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown")
    return dict(rcp_profile=np.array(name), host_cpu=np.array(cpu))


def train_case(stream, T, rng):
    """tests/test_train_features.py: make_case"""
    clean = synth.stream_pcm(stream, T).astype(np.float32).reshape(T, 480) * 0.5
    noise = (rng.standard_normal((T, 480)) * (300 + 200 * stream)).astype(np.float32)
    noisy = clean + noise
    clean[10:14] = 0
    noisy[10:14] = noise[10:14] * 1e-4
    vad = (np.arange(T) % 3 != 0).astype(np.float32)
    return clean, noisy, vad


def reference_pins(gold, tag, blob):
    """The inputs are those of the tests that read the file; they regenerate them, so only outputs are stored."""
    d = {}
    for k, v in zip(("window", "dct", "twiddles", "bitrev"), RefHarness.tables()):
        d[f"tables_{k}"] = v
    rng = np.random.default_rng(3)
    for i in range(4):
        x = (rng.standard_normal(1920) * 3000).astype(np.float32)
        d[f"fft{i}"] = RefHarness.fft(x)
        buf = (rng.standard_normal(1728) * 2000).astype(np.float32)
        T, g, lp = RefHarness.pitch(buf, 200, 0.4)
        d[f"pitch{i}_period"], d[f"pitch{i}_gain"], d[f"pitch{i}_x_lp"] = np.int32(T), np.float32(g), lp
    pcm = synth.stream_pcm(11, 250, lead_silence=7).astype(np.float32).reshape(250, 480)
    r = RefHarness(blob)
    assert r.L.refh_arch(r.h) == 2
    for k, v in r.run(pcm).items():
        if k == "out":
            d["free_out_crc"] = crc_rows(v)
        else:
            d[f"free_{k}"] = v
    d["free_state"] = r.get_state()
    pcm = synth.stream_pcm(21, 60).astype(np.float32).reshape(60, 480)
    r = RefHarness(blob)
    r.run(pcm[:40])
    d["forced_state"] = r.get_state()
    for k, v in r.run(pcm[40:]).items():
        d[f"forced_{k}"] = v
    rng = np.random.default_rng(5)
    for stream, (lp, blp, nf) in enumerate([(481, 32, 0), (200, 24, 0), (481, 32, 1), (90, 16, 1)]):
        clean, noisy, vad = train_case(stream, 40, rng)
        rt = RefTrainHarness()
        d[f"train{stream}"] = np.stack([rt.frame(clean[t], noisy[t], lp, blp, vad[t], nf) for t in range(40)])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import train_cases  # noqa: E402  (tests/train_cases.py: test_oracle_train_step_matches_reference_on_the_band_limit_edges)
    e = train_cases.edge_subset()
    for s in range(e.n):
        rt = RefTrainHarness()
        d[f"trainedge{s}"] = np.stack([rt.frame(e.clean[t, s], e.noisy[t, s], int(e.lowpass[s]), int(e.band_lp[s]), e.vad[t, s],
                                                int(e.noise_free[s])) for t in range(train_cases.T)])
    path = os.path.join(gold, "reference_pins.npz")
    if os.path.exists(path):  # what the file pins already stays pinned ("host_cpu" names the machine, not a result)
        old = np.load(path)
        for k in old.files:
            if k != "host_cpu":
                assert k in d or k in tag, f"{k} would be dropped"
                new = np.asarray(d[k] if k in d else tag[k])
                assert new.dtype == old[k].dtype and new.shape == old[k].shape and new.tobytes() == old[k].tobytes(), f"{k} changed"
    np.savez_compressed(path, **d, **tag)


def block_pins(gold, tag):
    """The inputs are stream_mix.block(), which the test that reads the file regenerates; only digests of outputs are stored."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import stream_mix  # noqa: E402  (tests/stream_mix.py: test_oracle.py's block tests)
    d = {}
    for run, name, positions, scheduled in stream_mix.block_pin_runs():
        blob = open(os.path.join(ROOT, "oracle", "_ref", f"{name}.blob"), "rb").read()
        r = stream_mix.block_run(blob, positions, scheduled, engine=RefHarness)
        d[f"{run}_positions"] = np.array(positions, np.int16)
        for k, v in stream_mix.block_digest(r).items():
            d[f"{run}_{k}"] = v
    blob = open(os.path.join(ROOT, "oracle", "_ref", "default.blob"), "rb").read()
    for run, hz, typ in stream_mix.chunk_pin_runs():  # the chunk dressing's oracle inputs: every position, lock step
        for k, v in stream_mix.chunk_pin_digest(stream_mix.chunk_pin_run(blob, hz, typ, engine=RefHarness)).items():
            d[f"{run}_{k}"] = v
    path = os.path.join(gold, "block_pins.npz")
    if os.path.exists(path):  # what the file pins already stays pinned
        old = np.load(path)
        for k in old.files:
            if k != "host_cpu":
                assert k in d or k in tag, f"{k} would be dropped"
                new = np.asarray(d[k] if k in d else tag[k])
                assert new.dtype == old[k].dtype and new.shape == old[k].shape and new.tobytes() == old[k].tobytes(), f"{k} changed"
    np.savez_compressed(path, **d, **tag)
    print(path, os.path.getsize(path))


def main():
    global GOLD
    tag = host_profile()
    pins_only = "--pins" in sys.argv
    if pins_only:
        sys.argv.remove("--pins")
    block_only = "--block-pins" in sys.argv
    if block_only:
        sys.argv.remove("--block-pins")
    blob_dir = GOLD
    if str(tag["rcp_profile"]) != "intel":
        GOLD = os.path.join(GOLD, str(tag["rcp_profile"]).replace("-", "_"))
    if len(sys.argv) > 1:
        GOLD = sys.argv[1]
    os.makedirs(GOLD, exist_ok=True)
    if block_only:
        block_pins(GOLD, tag)
        return
    if pins_only:
        reference_pins(GOLD, tag, open(os.path.join(ROOT, "oracle", "_ref", "default.blob"), "rb").read())
        return
    for name in ("default", "little"):
        blob = open(os.path.join(ROOT, "oracle", "_ref", f"{name}.blob"), "rb").read()
        path = os.path.join(blob_dir, f"{name}.blob.xz")
        if os.path.exists(path) and lzma.decompress(open(path, "rb").read()) == blob:
            continue  # unchanged: keep the committed bytes
        with open(path, "wb") as f:
            f.write(lzma.compress(blob, preset=9))
    blob = open(os.path.join(ROOT, "oracle", "_ref", "default.blob"), "rb").read()

    # ---- detail ----
    d = {}
    for s in (3, 77):
        T = 100
        pcm = synth.stream_pcm(s, T, lead_silence=12).reshape(T, 480)
        r = RefHarness(blob)
        res = r.run(pcm.astype(np.float32))
        d[f"s{s}_pcm"] = pcm
        for k, v in res.items():
            d[f"s{s}_{k}"] = v
        d[f"s{s}_state"] = r.get_state()
    np.savez_compressed(os.path.join(GOLD, "detail_default.npz"), **d, **tag)

    # ---- digest ----
    d = {}
    for s in (0, 1, 159, 4095):
        T = 400
        pcm = synth.stream_pcm(s, T, lead_silence=5).reshape(T, 480)
        r = RefHarness(blob)
        res = r.run(pcm.astype(np.float32))
        d[f"s{s}_pcm_crc"] = np.uint32(synth.crc32(pcm))
        d[f"s{s}_vad"] = res["vad"]
        d[f"s{s}_pitch"] = res["pitch"].astype(np.int16)
        d[f"s{s}_gains"] = res["gains"]
        d[f"s{s}_out_crc"] = crc_rows(res["out"])
        d[f"s{s}_state_crc"] = np.uint32(synth.crc32(r.get_state()))
    np.savez_compressed(os.path.join(GOLD, "digest_default.npz"), **d, **tag)

    # ---- edge cases ----
    d = {}
    for name, pcm in edge_inputs().items():
        r = RefHarness(blob)
        res = r.run(pcm.astype(np.float32))
        d[f"{name}_pcm"] = pcm
        d[f"{name}_vad"] = res["vad"]
        d[f"{name}_pitch"] = res["pitch"].astype(np.int16)
        d[f"{name}_gains"] = res["gains"]
        d[f"{name}_silence"] = res["silence"].astype(np.int8)
        d[f"{name}_out_crc"] = crc_rows(res["out"])
        d[f"{name}_state_crc"] = np.uint32(synth.crc32(r.get_state()))
    np.savez_compressed(os.path.join(GOLD, "edge_default.npz"), **d, **tag)

    # ---- sparser model ----
    blob2 = open(os.path.join(ROOT, "oracle", "_ref", "little.blob"), "rb").read()
    d = {}
    for s in (2, 31):
        T = 200
        pcm = synth.stream_pcm(s, T, lead_silence=3).reshape(T, 480)
        r = RefHarness(blob2)
        res = r.run(pcm.astype(np.float32))
        d[f"s{s}_pcm_crc"] = np.uint32(synth.crc32(pcm))
        d[f"s{s}_vad"] = res["vad"]
        d[f"s{s}_pitch"] = res["pitch"].astype(np.int16)
        d[f"s{s}_gains"] = res["gains"]
        d[f"s{s}_out_crc"] = crc_rows(res["out"])
        d[f"s{s}_state_crc"] = np.uint32(synth.crc32(r.get_state()))
    np.savez_compressed(os.path.join(GOLD, "digest_little.npz"), **d, **tag)
    reference_pins(GOLD, tag, blob)
    block_pins(GOLD, tag)
    for f in sorted(os.listdir(GOLD)):
        print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    main()
