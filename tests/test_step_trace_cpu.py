"""What the batch host code enqueues, call by call, without a GPU.

tests/csrc/step_trace.cpp links the batch host sources (the batch*.cpp of SRCS in rnnoise_amd/csrc/Makefile) against recording stubs
of the HIP runtime and of the kernel launchers, runs fixed sequences of API calls -- every call kind, schedule, network form and
configuration the frame step distinguishes, the split halves, the chunk calls and the staged forms -- and prints, per case, the
number of records and the SHA-256 of the trace.  tests/golden/step_trace.txt holds those lines as the commit named in its first line
produced them: the launches, their order, streams, events and arguments, and what every entry point returns, are that commit's.
The golden file is never regenerated from the code under test.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rnnoise_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "csrc", "step_trace.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_trace.txt")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def batch_sources(csrc=CSRC):
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    return [os.path.join(csrc, f) for f in srcs if f.startswith("batch") and f.endswith(".cpp")]


def build(out, csrc=CSRC):
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I", ROCM_INCLUDE, "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wno-unused-result", "-o", out, HARNESS] + batch_sources(csrc), check=True)
    return out


def _env():  # the dispatch switches are read from the environment: the cases run on their defaults
    return {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("step_trace") / "step_trace"))


def _golden():
    lines = open(GOLDEN).read().splitlines()
    assert lines[0].startswith("# recorded from commit "), lines[0]
    return [l.split() for l in lines[1:] if l and not l.startswith("#")]


def test_every_case_traces_as_recorded(harness, tmp_path):
    got = [l.split() for l in subprocess.run([harness], check=True, capture_output=True, text=True, env=_env()).stdout.splitlines()]
    want = _golden()
    assert [g[0] for g in got] == [w[0] for w in want]
    bad = []
    for g, w in zip(got, want):
        if g != w:
            path = tmp_path / (g[0] + ".trace")
            path.write_text(subprocess.run([harness, "--dump", g[0]], check=True, capture_output=True, text=True, env=_env()).stdout)
            bad.append("%s: %s records, recorded %s; the trace of this tree: %s" % (g[0], g[1], w[1], path))
    assert not bad, "\n".join(bad)


def test_the_cases_reach_what_they_are_for(harness):
    """The recorded traces hold the launches the cases were written to reach (a case that silently stops reaching them would still
    compare equal to a golden file recorded the same way)."""
    def dump(case):
        return subprocess.run([harness, "--dump", case], check=True, capture_output=True, text=True, env=_env()).stdout
    t = dump("frames_sched0")
    assert "hipStreamWaitEvent S2 E" in t and "hipStreamWaitEvent S1 E" in t  # (K0's and K1's streams wait)
    assert len(set(re.findall(r"rn_launch_hp (S\d+)", t))) == 3  # (the caller's, the null stream, the side stream)
    forms = {c: set(re.findall(r"rn_launch_nn_(\w+) ", dump(c))) for c in ("nn_one", "nn_vector", "nn_tiles", "nn_layers")}
    assert forms == {"nn_one": {"one"}, "nn_vector": {"vector"}, "nn_tiles": {"mfma"}, "nn_layers": {"layers", "requant"}}, forms
    assert dump("nn_layers").count("rn_launch_nn_requant") == 1  # (the first step alone)
    assert set(re.findall(r"rn_launch_nn_mfma .* form=(\d)", dump("nn_tiles"))) == {"2", "3"}
    assert "model=2" in dump("nn_layers_two_models")
    assert "hipMemsetD32Async" in dump("masked")
    assert re.search(r"rn_launch_nn_requant S\d+ list=U\+60000000 n=5", dump("list"))
    t = dump("split_sched0")
    assert t.count("hipMemcpyAsync D2D") == 3 * 3  # (T = 3, 6 and 9 keep the delayed spectra: X, P and E each)
    assert "mode=2" in t and "mode=3" in t
    assert "hook before_hp" in dump("host_fed_ring")
    t = dump("chunks")
    assert t.count("hipMalloc") == 1 + 1 + 2 and "kind=2" in t  # (arena, FIFOs, the staging buffer and its growth)
    assert "hipMemcpy2D H2D" in dump("staged") and "hipMemcpy2D D2H" in dump("staged")
    assert "feat+" in dump("staged_split") or "host" in dump("staged_split")
