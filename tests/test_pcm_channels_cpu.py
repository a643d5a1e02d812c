"""CPU checks of interleaved channels (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels): declared, exported by the product
libraries and the instrumented one, bound by ctypes and the torch op, NULL batches refused without a GPU; the overlap rule of the
process calls against a brute-force enumeration of the slot intervals; and the kernel forms of a step -- what a channel count moves
(K0 above 2,048 streams) and what it cannot."""
import ctypes as C
import os
import re
import subprocess

import pytest

from abi_contract import declared_once, exported
from conftest import ROOT
from rnnoise_amd import capi

NEW = ["rnnoise_batch_set_pcm_channels", "rnnoise_batch_pcm_channels", "rnnoise_amd_pcm_channels_fit"]


def test_prototypes_declared_once_each_with_export():
    src = declared_once(NEW)
    assert re.search(r"#define\s+RNNOISE_AMD_MAX_CHANNELS\s+8\b", src) and capi.MAX_CHANNELS == 8


@pytest.mark.parametrize("so", ["librnnoise_amd.so", "librnnoise.so.0", "librnnoise_amd_instr.so"])
def test_libraries_export_them(so):
    exported(so, NEW)


def test_ctypes_and_torch_bindings():
    L = capi.lib()
    assert len(L.rnnoise_batch_set_pcm_channels.argtypes) == 2
    assert len(L.rnnoise_batch_pcm_channels.argtypes) == 1
    assert len(L.rnnoise_amd_pcm_channels_fit.argtypes) == 6
    assert callable(capi.Batch.set_pcm_channels) and isinstance(capi.Batch.pcm_channels, property)
    assert capi.pcm_channels_fit(960, 3 * 960, 480, 2, 4, 3) is True and capi.pcm_channels_fit(960, 3 * 960, 480, 2, 5, 3) is False
    from rnnoise_amd import torch_op
    assert callable(torch_op.RNNoiseOp.process_channels)


def test_null_batch_returns_minus_one():
    """every call that takes a batch, on NULL: -1 without a device -- the setter for good and bad counts alike, the getter, and the
    process forms a channel count applies to"""
    L = capi.lib()
    for ch in (1, 2, 8, 0, -1, 9):
        assert L.rnnoise_batch_set_pcm_channels(None, ch) == -1
    assert L.rnnoise_batch_pcm_channels(None) == -1
    assert L.rnnoise_batch_process_device(None, None, None, None, None, 1, None) == -1
    assert L.rnnoise_batch_process_device_s16(None, None, None, None, None, 1, None) == -1
    idx = (C.c_int * 3)(0, 1, 2)
    assert L.rnnoise_batch_process_device_list(None, None, None, None, None, idx, 3, None, 1, None) == -1
    assert L.rnnoise_batch_process(None, None, None, None, None, 1) == -1
    assert L.rnnoise_batch_process_s16(None, None, None, None, None, 1) == -1


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("channels_dispatch")
    exes = {}
    for name in ("channels_dispatch_test", "dispatch_test"):
        exes[name] = str(d / name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", name + ".cpp"), "-o",
                        exes[name]], check=True)

    def run(cases, exe="channels_dispatch_test", **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
        env.update({f"RNNOISE_AMD_{k}": str(v) for k, v in knobs.items()})
        return subprocess.run([exes[exe]] + list(cases), capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    return run


def test_setter_rule(prog):
    """1 .. RNNOISE_AMD_MAX_CHANNELS, and a divisor of the batch's streams"""
    cases = {(1, 12): 1, (2, 12): 1, (3, 12): 1, (4, 12): 1, (6, 12): 1, (8, 16): 1, (8, 65536): 1, (1, 1): 1, (1, 7): 1,
             (0, 12): 0, (-1, 12): 0, (-2, 12): 0, (9, 18): 0, (12, 12): 0, (5, 12): 0, (8, 12): 0, (2, 7): 0, (3, 2048): 0}
    got = prog([f"ok:{c},{n}" for c, n in cases])
    assert [int(x) for x in got] == list(cases.values()), list(zip(cases, got))


def _disjoint(starts, length):
    at = sorted(starts)
    return all(b - a >= length for a, b in zip(at, at[1:]))


def _brute(fs, rs, M, ch, rows, frames):
    """whether the group slots [f * fs + g * rs, + M * ch) of a call are pairwise disjoint, by enumeration"""
    if rows % ch:
        return 0
    return int(_disjoint([f * fs + g * rs for f in range(frames) for g in range(rows // ch)], M * ch))


def _brute_nested(fs, rs, M, ch, rows, frames):
    """the documented rule by enumeration: the groups' slots lie disjoint inside each frame's run of n_groups row strides and those
    runs are disjoint (row-major), or the frames' slots lie disjoint inside each group's run of n_frames frame strides and those runs
    are disjoint (stream-contiguous)"""
    G, S = rows // ch, M * ch
    row_major = _disjoint([g * rs for g in range(G)], S) and _disjoint([f * fs for f in range(frames)], G * rs)
    stream_contiguous = _disjoint([f * fs for f in range(frames)], S) and _disjoint([g * rs for g in range(G)], frames * fs)
    return int(row_major or stream_contiguous)


def _fit_cases():
    for ch in (1, 2, 3, 8):
        for M in (80, 480):
            S = M * ch
            for rows in range(0, 7):
                for frames in range(0, 4):
                    # strides around each boundary of the rule: the slot, a frame of groups, a group of frames
                    cands = sorted({b + d for b in (S, (rows // ch) * S, frames * S) for d in (-4, 0, 4) if b + d > 0})
                    for fs in cands:
                        for rs in cands:
                            yield fs, rs, M, ch, rows, frames


def test_overlap_rule_against_brute_force(prog):
    """rnnoise_amd_pcm_channels_fit is the layout rule with the group slot as the row.  It never accepts slots that overlap; and with
    at least two groups and two frames -- where both strides place something -- it accepts exactly the nested arrangements the header
    documents, enumerated as intervals.  (With one group or one frame the unused stride must still clear a slot, and staggered slots
    that happen to be disjoint without nesting are refused: the rule is the existing one, not a looser one.)"""
    L = capi.lib()
    cases = list(_fit_cases())
    assert len(cases) > 5000
    tool = prog([f"fit:{','.join(map(str, c))}" for c in cases[::7]])
    assert [int(x) for x in tool] == [L.rnnoise_amd_pcm_channels_fit(*c) for c in cases[::7]]  # (dispatch.h is what the library runs)
    exact = 0
    for c in cases:
        fs, rs, M, ch, rows, frames = c
        got, want = L.rnnoise_amd_pcm_channels_fit(*c), _brute(*c)
        assert got in (0, 1) and got <= want, c  # (never "fits" for overlapping slots, or for rows that fill no whole groups)
        if rows % ch:
            assert got == 0, c
            continue
        assert got == L.rnnoise_amd_pcm_layout_fits(fs, rs, M * ch, rows // ch, frames), c
        if rows // ch >= 2 and frames >= 2:
            assert got == _brute_nested(*c), c
            exact += 1
    assert exact > 500


def test_equals_the_layout_rule_for_one_channel():
    L = capi.lib()
    from test_pcm_layout_cpu import FITS
    for (fs, rs, M, rows, frames), w in FITS:
        assert L.rnnoise_amd_pcm_channels_fit(fs, rs, M, 1, rows, frames) == w == L.rnnoise_amd_pcm_layout_fits(fs, rs, M, rows, frames)
    for c in _fit_cases():
        if c[3] == 1:
            assert L.rnnoise_amd_pcm_channels_fit(*c) == L.rnnoise_amd_pcm_layout_fits(c[0], c[1], c[2], c[4], c[5]), c
    # strides the layout setter refuses never fit; neither does a count outside 1 .. 8
    assert L.rnnoise_amd_pcm_channels_fit(962, 6 * 962, 480, 2, 4, 6) == 0
    assert L.rnnoise_amd_pcm_channels_fit(0, 0, 480, 2, 4, 6) == 0
    assert L.rnnoise_amd_pcm_channels_fit(960, 6 * 960, 480, 0, 4, 6) == 0
    assert L.rnnoise_amd_pcm_channels_fit(9 * 480, 6 * 9 * 480, 480, 9, 18, 6) == 0
    assert L.rnnoise_amd_pcm_channels_fit(8 * 480, 6 * 8 * 480, 480, 8, 16, 6) == 1


def _reference_plan(prog, n, pipelined, **knobs):
    nn_path = 1 if n > 512 and n >= 16 else 0  # (dispatch.h: rn_default_nn_path at the default switches)
    return prog([f"plan:{n},1,256,{nn_path},{pipelined},0,0"], exe="dispatch_test", **knobs)[0]


# every stream-count switch of the plan (dispatch.h: rn_plan), both sides, at counts 1, 2 and 3 divide: K3 256, the network's 512,
# K0's 2,048, K1's 2,560, the layer-wise network's 10,240.  The channel count can change K0's choice only
SIZES = [6, 252, 258, 510, 516, 2046, 2052, 2556, 2562, 10236, 10242, 65532]


@pytest.mark.parametrize("pipelined", [0, 1])
def test_plan_with_channels(prog, pipelined):
    for n in SIZES:
        one = prog([f"plan:{n},256,{pipelined},1"])[0]
        assert one == _reference_plan(prog, n, pipelined), n  # channels == 1: the plan of a shape without the field
        for ch in (2, 3):
            got = prog([f"plan:{n},256,{pipelined},{ch}"])[0].split()
            assert got[0] == "rn_hp_one_kernel", (n, ch)  # K0 one wave per stream at every size
            assert got[1:] == one.split()[1:], (n, ch)      # nothing else looks at the caller's PCM
        assert one.split()[0] == ("rn_hp_one_kernel" if n <= 2048 else "rn_hp_kernel"), n


def test_plan_with_channels_under_a_moved_switch(prog):
    """with K0's switch moved ($RNNOISE_AMD_HP_ONE_MAX) the channel count still decides, and one channel still follows the switch"""
    for n in (60, 66, 2046, 2052):
        one = prog([f"plan:{n},256,1,1"], HP_ONE_MAX=64)[0]
        assert one == _reference_plan(prog, n, 1, HP_ONE_MAX=64)
        assert one.split()[0] == ("rn_hp_one_kernel" if n <= 64 else "rn_hp_kernel")
        for ch in (2, 3):
            assert prog([f"plan:{n},256,1,{ch}"], HP_ONE_MAX=64)[0].split()[0] == "rn_hp_one_kernel"


def test_channel_count_sits_beside_the_row_pitch():
    """RnGroupDev::pcm_chan follows pcm_pitch, and the step is the only writer of either, in one place (b->g never carries them)"""
    csrc = os.path.join(ROOT, "rnnoise_amd", "csrc")
    src = open(os.path.join(csrc, "rn_dev.h")).read()
    assert re.search(r"int pcm_pitch;\n(\s*//[^\n]*\n)+\s*int pcm_chan;", src)
    host = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".cpp")}
    writers = [f for f, text in host.items() for _ in re.findall(r"[.>]pcm_chan\s*=[^=]", text)]
    assert len(writers) == 1, writers
    step = host[writers[0]]  # the one writer is the step itself, handing on the call's count
    assert re.search(r"^int batch_process_device_impl\(", step, re.M) and "g.pcm_chan = pcm_chan;" in step
    for f, text in host.items():
        assert "b->g.pcm_chan" not in text, f
