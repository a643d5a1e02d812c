"""Every weight layout of tests/weight_layouts.py on the host: the loader accepts what the oracle accepts (less the two
documented refusals), the three device copies of every int8 layer describe the blob's matrix, packs round-trip, and the
oracle stays bit-identical to the compiled reference on every layout."""
import hashlib

import numpy as np
import pytest

import weight_layouts as wl
from conftest import assert_bits_equal, load_blob
from oracle.binding import Oracle, RefHarness
from rnnoise_amd import blob as rb
from rnnoise_amd import capi, synth


def _accepted_by_loader(blob):
    m = capi.Model(blob)
    try:
        m.weight_bytes
        return True
    except ValueError:
        return False
    finally:
        m.close()


def _accepted_by_oracle(blob):
    try:
        Oracle(blob)
        return True
    except ValueError:
        return False


def test_the_zoo_keeps_its_numeric_contract():
    """every entry but the marked one keeps every same-sign pair sum within 129 (where the reference's maddubs is exact), and
    only int8_extremes leaves the exporter's [-127, 127]"""
    for name in wl.NAMES:
        rec = wl.records(name)
        for layer in wl.INT8_LAYERS:
            w = rec[layer + "_weights_int8"]
            assert (w.min() >= -127) or name == "int8_extremes", (name, layer)
            assert wl.pair_sums_ok(w) or (name == "pair_bound_broken" and layer == "gru2_input"), (name, layer)
        for k, a in rec.items():
            assert a.dtype != np.float32 or np.isfinite(a).all(), (name, k)
    assert wl.records("int8_extremes")["gru1_input_weights_int8"].min() == -128
    assert any((wl.matrix(wl.records("duplicates_overflow"), "gru1_input") > 127).ravel())


@pytest.mark.parametrize("name", wl.NAMES)
def test_loader_accepts_what_the_oracle_accepts(name, capfd):
    """rnnoise_model_from_buffer accepts an entry exactly when the oracle's parser (the reference's rules,
    parse_lpcnet_weights.c:98-121) does, except the two refusals, each with one line on stderr saying why;
    weight_bytes follows SURVEY 8d"""
    blob = wl.make(name)
    e = wl.BY_NAME[name]
    assert _accepted_by_oracle(blob)
    capfd.readouterr()
    ok = _accepted_by_loader(blob)
    err = [l for l in capfd.readouterr().err.splitlines() if "rejected" in l]
    if e.refusal is None:
        assert ok and not err
        assert capi.Model(blob).weight_bytes == wl.weight_bytes(wl.records(name))
    else:
        assert not ok
        assert len(err) == 1, err
        assert {"merged": "outside int8", "pair": "pair sum 130"}[e.refusal] in err[0], err[0]


def _payload(pack, h, layer, key, dtype, count):
    off = h["header_bytes"] + layer["offsets"][key]
    return np.frombuffer(pack, dtype, count, off)


def _mfma_image(pack, h, layer):
    """the int8 MFMA image back in [out][in] order: frag[rt][kt][lane][e] = W[16 rt + lane % 16][64 kt + 16 (lane / 16) + e]"""
    nin, nout = layer["nin"], layer["nout"]
    frag = _payload(pack, h, layer, "wmf", np.int8, nin * nout).reshape(nout // 16, nin // 64, 4, 16, 16)
    return frag.transpose(0, 3, 1, 2, 4).reshape(nout, nin).astype(np.int64)


def _float_operand_order(fw, nin, nout):
    """fw [in][out] in the operand order of the f32 MFMA chains: [rt][t / 4][lane][t % 4] = W[4 t + lane / 16][16 rt + lane % 16]"""
    s4 = (nin + 15) // 16
    wp = np.zeros((16 * s4, nout), np.float32)
    wp[:nin] = fw.reshape(nin, nout)
    v = wp.reshape(s4, 4, 4, nout // 16, 16)           # [t / 4][t % 4][lane / 16][rt][lane % 16]
    return np.ascontiguousarray(v.transpose(3, 0, 2, 4, 1)).reshape(-1)


@pytest.mark.parametrize("name", wl.ACCEPTED)
def test_device_copies_describe_one_matrix(name):
    """the pack is what a blob load uploads: for every int8 layer, the block stream and column table are the blob's, the MFMA
    image (inverted from fragment order) is the int64 sum of the blocks -- repeated blocks added, not overwritten -- and the
    row sums are 128 x that matrix's; every float layer's MFMA copy is its weights in operand order"""
    rec = wl.records(name)
    pack = capi.Model(wl.make(name)).pack()
    h = rb.read_pack_header(pack)
    for layer in h["layers"]:
        nm, nin, nout = layer["name"], layer["nin"], layer["nout"]
        if not layer["is_int8"]:
            fw = rec[nm + "_weights_float"]
            assert_bits_equal(_payload(pack, h, layer, "fw", np.float32, nin * nout), fw, f"{nm} weights")
            assert_bits_equal(_payload(pack, h, layer, "bias", np.float32, nout), rec[nm + "_bias"], f"{nm} bias")
            if nout % 16 == 0:
                want = _float_operand_order(fw, nin, nout)
                assert_bits_equal(_payload(pack, h, layer, "wmf", np.float32, want.size), want, f"{nm} MFMA copy")
            continue
        w = rec[nm + "_weights_int8"]
        assert layer["nblocks"] == w.size // 32
        assert np.array_equal(_payload(pack, h, layer, "w", np.int8, w.size), w), f"{nm}: block stream"
        assert_bits_equal(_payload(pack, h, layer, "bias", np.float32, nout), rec[nm + "_subias"], f"{nm} subias")
        assert_bits_equal(_payload(pack, h, layer, "scale", np.float32, nout), rec[nm + "_scale"], f"{nm} scale")
        cols = _payload(pack, h, layer, "cols", np.uint16, layer["nblocks"]).astype(np.int64)
        grp = _payload(pack, h, layer, "grp", np.int32, nout // 8 + 1)
        if nm + "_weights_idx" in rec:
            gs = wl.groups(rec, nm)
            assert np.array_equal(grp, np.concatenate([[0], np.cumsum([len(g) for g in gs])])), f"{nm}: group starts"
            assert np.array_equal(cols, [c for g in gs for c, _ in g]), f"{nm}: columns"
            if layer["has_diag"]:
                assert_bits_equal(_payload(pack, h, layer, "diag", np.float32, nout), rec[nm + "_weights_diag"], f"{nm} diag")
        else:
            assert np.array_equal(grp, np.arange(nout // 8 + 1) * (nin // 4))
        want = wl.matrix(rec, nm)
        got = _mfma_image(pack, h, layer)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{nm}: MFMA image differs from the sum of the blocks at {len(bad)} weights, first [out, in] = {bad[0]}"
        rs = _payload(pack, h, layer, "rowsum", np.int32, nout)
        assert np.array_equal(rs, 128 * want.sum(axis=1)), f"{nm}: rowsum128"


@pytest.mark.parametrize("name", wl.ACCEPTED)
def test_pack_round_trip(name):
    """a pack of every accepted layout loads (the pack loader bounds the block count by the payload, not by the dense
    count: the duplicates entry has more blocks than a dense matrix) and packs back to the same bytes"""
    blob = wl.make(name)
    p = capi.Model(blob).pack()
    m = capi.Model(p)
    assert m.weight_bytes == capi.Model(blob).weight_bytes
    assert m.pack() == p
    m.close()


# sha256 of the packs of the committed blobs and of synth_model outputs, as the parent commit's loader wrote them: the
# refusals and the merged MFMA image must not touch an exporter-shaped blob
EXPORTER_PACKS = {
    "default": "676994afffd47410c43b5d13138e2e22e2e1617316f566f3f555569ddd21026e",
    "little": "a9a6a58656f9ebb3143d3b2817f79ace25c9a7c9b07c1b1bcf45c26f31ecad9e",
    "synth_7_0.1": "9275fa6eff4a10c3a151807322e7b1613a2ebf7d19d7865e2e7c5bbbd7060e84",
    "synth_7_1.0": "783dc9cc91a75a743c175f32cfdf6fbc5a5f034a6c40bb68d7b27348ae54092f",
}


@pytest.mark.parametrize("which", sorted(EXPORTER_PACKS))
def test_exporter_shaped_blobs_pack_as_before(which):
    if which in ("default", "little"):
        blob = load_blob(which)
    else:
        _, seed, density = which.split("_")
        blob = rb.synth_model(int(seed), float(density))
    assert hashlib.sha256(capi.Model(blob).pack()).hexdigest() == EXPORTER_PACKS[which]


def _signals():
    return [synth.stream_pcm(s, 40, lead_silence=ls).astype(np.float32).reshape(40, 480) for s, ls in ((2, 3), (41, 1))]


@pytest.mark.skipif(not RefHarness.available(), reason="the compiled reference (oracle/_ref) is not built here")
@pytest.mark.rcp("host")  # the compiled reference executes this CPU's rcpps
@pytest.mark.parametrize("name", wl.NAMES)
def test_oracle_equals_the_compiled_reference(name, record_property):
    """the oracle -- the GPU suite's yardstick -- against the reference's own parser and kernels on every layout, refused
    ones included: features, gains, VAD, PCM and state bit-identical, 2 signals x 40 frames with a silent lead.  For the
    pair-bound entry only the divergence is recorded: the loader refuses it on the arithmetic (a pair sum of 130 can
    saturate the reference's int16 pair products), whether or not these frames reach the saturation."""
    blob = wl.make(name)
    diverged = []
    for pcm in _signals():
        o, r = Oracle(blob), RefHarness(blob)
        want, got = o.run(pcm), r.run(pcm)
        keys = ("features", "gains", "vad", "out")
        if name == "pair_bound_broken":
            diverged.append(any(not np.array_equal(want[k].view(np.uint32), got[k].view(np.uint32)) for k in keys) or
                            not np.array_equal(o.get_state().view(np.uint32), r.get_state().view(np.uint32)))
            continue
        assert want["silence"][0] and not want["silence"][-1]
        for k in keys:
            assert_bits_equal(want[k], got[k], f"{name}: {k}")
        assert_bits_equal(o.get_state(), r.get_state(), f"{name}: state")
    if name == "pair_bound_broken":
        record_property("reference_diverges_from_exact_arithmetic", diverged)
        print(f"pair_bound_broken: the reference diverges from exact arithmetic on signals {diverged}")
