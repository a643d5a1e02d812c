"""Which form of each kernel a frame step runs (rnnoise_amd/csrc/dispatch.h), pinned without a GPU.  Every form of a stage gives the
same bits, so the parity tests on the GPU would still pass if a threshold or a switch quietly sent every case to one form: the rules
are pinned here at each boundary, on both sides, with the switches set as the library reads them (the environment, once per
process).  bench.py keeps its own copy of the rules to name the kernel of a bench line (kernel_of); it is held to the library's here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rnnoise_amd", "csrc")
KNOBS = ("NN_LAYERS_MIN", "NN_ONE_MAX", "HP_ONE_MAX", "K1_SPW", "TILE_WAVES", "GRU_VARIANT", "PIPE")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dispatch") / "dispatch_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "csrc", "dispatch_test.cpp"), "-o", exe],
                   check=True)

    def run(cases, **knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("RNNOISE_AMD_")}
        env.update({f"RNNOISE_AMD_{k}": str(v) for k, v in knobs.items()})
        r = subprocess.run([exe] + list(cases), capture_output=True, text=True, check=True, env=env)
        return r.stdout.splitlines(), r.stderr
    return run


def plan(prog, n, whole=True, cus=256, path=0, pipelined=False, per_stream=False, low_rate=False, **knobs):
    """(K0, K1, K2, GRU, K3) kernel names of one step"""
    out, _ = prog([f"plan:{n},{int(whole)},{cus},{path},{int(pipelined)},{int(per_stream)},{int(low_rate)}"], **knobs)
    return tuple(out[0].split())


def k0(prog, n, **kw): return plan(prog, n, **kw)[0]
def k1(prog, n, **kw): return plan(prog, n, **kw)[1]
def k2(prog, n, **kw): return plan(prog, n, **kw)[2]
def gru(prog, n, **kw): return plan(prog, n, **kw)[3]
def k3(prog, n, **kw): return plan(prog, n, **kw)[4]


@pytest.mark.parametrize("pipelined", [False, True])
def test_k0_one_wave_per_stream_up_to_hp_one_max(prog, pipelined):
    assert k0(prog, 2048, pipelined=pipelined) == "rn_hp_one_kernel"
    assert k0(prog, 2049, pipelined=pipelined) == "rn_hp_kernel"
    assert k0(prog, 1, pipelined=pipelined, HP_ONE_MAX=0) == "rn_hp_kernel"      # 0: every 48 kHz size lane per stream
    assert k0(prog, 100, pipelined=pipelined, HP_ONE_MAX=100) == "rn_hp_one_kernel"
    assert k0(prog, 101, pipelined=pipelined, HP_ONE_MAX=100) == "rn_hp_kernel"
    assert k0(prog, 2049, pipelined=pipelined, HP_ONE_MAX=-3) == "rn_hp_kernel"  # (a negative value: the default)


def test_k0_low_rate_takes_one_wave_per_stream_at_every_size(prog):
    for n in (1, 2049, 65536):
        assert k0(prog, n, low_rate=True) == "rn_hp_one_kernel"
        assert k0(prog, n, low_rate=True, HP_ONE_MAX=0) == "rn_hp_one_kernel"


def test_k1_four_streams_per_workgroup_from_2560(prog):
    assert k1(prog, 2559) == "rn_analysis_single_kernel"
    assert k1(prog, 2560) == "rn_analysis_kernel"
    assert k1(prog, 2560, pipelined=True) == "rn_analysis_kernel"
    assert k1(prog, 65536, per_stream=True) == "rn_analysis_single_kernel"      # per-stream phase: always the single form
    assert k1(prog, 65536, K1_SPW=1) == "rn_analysis_single_kernel"
    for v in (4, 2, -1):                                                         # any other non-zero value: four at every size
        assert k1(prog, 1, K1_SPW=v) == "rn_analysis_kernel"
    assert k1(prog, 1, per_stream=True, K1_SPW=4) == "rn_analysis_single_kernel"


def test_k2_path0_latency_kernel_up_to_nn_one_max(prog):
    assert k2(prog, 512) == "rn_nn_one_kernel"
    assert k2(prog, 513) == "rn_nn_vector_kernel"
    assert k2(prog, 1, NN_ONE_MAX=0) == "rn_nn_vector_kernel"
    assert k2(prog, 65536, whole=True) == "rn_nn_vector_kernel"                  # path 0 never runs the layers
    # a one-stream view that is not the whole batch (drop-in frames do not take a plan: they run the row-list kernels, dropin.cpp)
    assert plan(prog, 1, whole=False) == ("rn_hp_one_kernel", "rn_analysis_single_kernel", "rn_nn_one_kernel", "rn_nn_gru_w8_kernel",
                                          "rn_synthesis_few_kernel")
    assert k2(prog, 1, whole=False, NN_ONE_MAX=0) == "rn_nn_vector_kernel"


def test_k2_path1_tiles_below_nn_layers_min_then_layers_on_whole_batches(prog):
    assert k2(prog, 10239, path=1, pipelined=True) == "rn_nn_mfma_kernel"
    assert k2(prog, 10240, path=1, pipelined=True) == "layers"
    assert k2(prog, 10240, path=1, whole=False, pipelined=True) == "rn_nn_mfma_kernel"
    assert k2(prog, 100, path=1, NN_LAYERS_MIN=100) == "layers"
    assert k2(prog, 99, path=1, NN_LAYERS_MIN=100) == "rn_nn_mfma16_kernel"
    assert k2(prog, 1, path=1, NN_LAYERS_MIN=0) == "layers"


def test_tile_kernel_sixteen_waves_alone_while_every_tile_has_a_cu(prog):
    # 256 CUs: 4,096 streams = 256 tiles
    assert k2(prog, 4096, path=1) == "rn_nn_mfma16_kernel"
    assert k2(prog, 4097, path=1) == "rn_nn_mfma_kernel"
    assert k2(prog, 4096, path=1, pipelined=True) == "rn_nn_mfma_kernel"
    assert k2(prog, 1600, path=1, cus=100) == "rn_nn_mfma16_kernel"
    assert k2(prog, 1601, path=1, cus=100) == "rn_nn_mfma_kernel"
    assert k2(prog, 8192, path=1, pipelined=True, TILE_WAVES=16) == "rn_nn_mfma16_kernel"
    assert k2(prog, 16, path=1, TILE_WAVES=8) == "rn_nn_mfma_kernel"
    for v in (0, 4, 12, 32):                                                     # any other value: by size
        assert k2(prog, 4096, path=1, TILE_WAVES=v) == "rn_nn_mfma16_kernel"
        assert k2(prog, 4097, path=1, TILE_WAVES=v) == "rn_nn_mfma_kernel"


def test_k2_path2_layers_on_whole_batches_tiles_on_parts(prog):
    assert k2(prog, 1, path=2) == "layers"
    assert k2(prog, 70, path=2, pipelined=True) == "layers"
    assert k2(prog, 1, path=2, whole=False) == "rn_nn_mfma16_kernel"             # a one-stream view is never whole
    assert k2(prog, 4097, path=2, whole=False) == "rn_nn_mfma_kernel"
    assert k2(prog, 64, path=2, whole=False, pipelined=True) == "rn_nn_mfma_kernel"


def test_gru_w8_while_every_group_has_a_cu(prog):
    assert gru(prog, 16384, path=2) == "rn_nn_gru_w8_kernel"
    assert gru(prog, 16385, path=2) == "rn_nn_gru_kernel"
    assert gru(prog, 6400, path=2, cus=100) == "rn_nn_gru_w8_kernel"
    assert gru(prog, 6401, path=2, cus=100) == "rn_nn_gru_kernel"
    assert gru(prog, 65536, path=2, GRU_VARIANT="w8") == "rn_nn_gru_w8_kernel"
    assert gru(prog, 1, path=2, GRU_VARIANT="w4") == "rn_nn_gru_kernel"
    assert gru(prog, 16385, path=2, GRU_VARIANT="") == "rn_nn_gru_kernel"       # empty: by size


def test_an_unknown_gru_form_is_reported_once_and_fails_the_layers(prog):
    out, err = prog(["plan:70,1,256,2,0,0,0", "plan:20000,1,256,1,1,0,0"], GRU_VARIANT="w16")
    assert [ln.split()[2:4] for ln in out] == [["layers", "unknown"]] * 2
    assert err.count("RNNOISE_AMD_GRU_VARIANT=w16") == 1


def test_k3_few_form_up_to_256(prog):
    assert k3(prog, 256) == "rn_synthesis_few_kernel"
    assert k3(prog, 257) == "rn_synthesis_kernel"
    assert k3(prog, 1, low_rate=True) == "rn_synthesis_few_kernel"


def test_a_new_batch_takes_the_mfma_path_above_nn_one_max_from_16_streams(prog):
    cases = ["path:512", "path:513", "path:1"]
    assert prog(cases)[0] == ["0", "1", "0"]
    assert prog(["path:15", "path:16"], NN_ONE_MAX=0)[0] == ["0", "1"]
    assert prog(["path:100000"], NN_ONE_MAX=100000)[0] == ["0"]


@pytest.mark.parametrize("pipe", [None, 0, 1, 2, 9])
def test_schedule(prog, pipe):
    knobs = {} if pipe is None else {"PIPE": pipe}
    cases = [f"sched:{f},{s}" for f in (0, 1, 2, 5) for s in (0, 1, 9)]
    out, _ = prog(cases, **knobs)
    got = dict(zip(cases, [tuple(int(x) for x in ln.split()) for ln in out]))
    for f in (0, 1, 2, 5):
        for s in (0, 1, 9):
            force = s or (pipe or 0)
            pipelined = f > 1 and force != 9
            assert got[f"sched:{f},{s}"] == (int(pipelined), int(pipelined and force != 1)), (f, s, pipe)


def test_bench_kernel_of_names_the_plans_kernels(prog, monkeypatch):
    """bench.py's copy of the rules (kernel_of) against the library's, for default switches, 256 CUs and 48 kHz lock-step calls"""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    for name, value in (("NN_LAYERS_MIN_STREAMS", 10240), ("NN_ONE_MAX_STREAMS", 512), ("HP_ONE_MAX_STREAMS", 2048),
                        ("K1_SPW_FORCE", 0), ("TILE_WAVES_FORCE", 0), ("N_CU", 256)):
        monkeypatch.setattr(bench, name, value)  # (bench reads the same switches from its own environment at import)
    sizes = [1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 2559, 2560, 2561, 4096, 4097, 8192, 10239, 10240, 12288,
             16384, 16385, 40037, 65536]
    shapes = [(n, nn, alone) for n in sizes for nn in ("mfma", "vector") for alone in (True, False)]
    out, _ = prog([f"plan:{n},1,256,{1 if nn == 'mfma' else 0},{int(not alone)},0,0" for n, nn, alone in shapes])
    for (n, nn, alone), line in zip(shapes, out):
        hp, an, net, g, syn = line.split()
        want = {"highpass": hp, "analysis": an, "network": g if net == "layers" else net, "synthesis": syn}
        for kind, kernel in want.items():
            assert bench.kernel_of(kind, n, nn, alone=alone) == kernel, (kind, n, nn, alone)


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_launchers_take_the_plan_and_drop_in_frames_the_row_kernels():
    for f in ("hp_kernel.hip", "dsp_kernels.hip", "nn_kernels.hip", "nn_mfma.hip", "nn_layers.hip", "nn_gru.h"):
        text = _src(f)
        assert "getenv" not in text and "hipGetDevice(" not in text, f
        for knob in KNOBS:
            assert f'"RNNOISE_AMD_{knob}"' not in text, (f, knob)
    # one plan per call, the schedule from the same module, the device's facts resolved once per batch
    step, batch = _src("batch_step.cpp"), _src("batch.cpp")  # (the step; create)
    assert "rn_plan(rn_knobs()" in step and "rn_schedule(rn_knobs()" in step and "rn_default_nn_path(rn_knobs()" in batch
    assert "hipDeviceAttributeMultiprocessorCount" in batch and "rn_nn_one_opt_in()" in batch and "rn_nn_gru_opt_in(" in batch
    # drop-in frames take no plan: every one of them is a launch group of the row-list kernels
    dropin = _src("dropin.cpp")
    assert "rn_plan(" not in dropin
    for launcher in ("rn_launch_hp_rows(", "rn_launch_analysis_rows(", "rn_launch_nn_rows(", "rn_launch_synthesis_rows("):
        assert dropin.count(launcher) == 1, launcher
    for launcher in ("rn_launch_hp(", "rn_launch_analysis(", "rn_launch_nn_one(", "rn_launch_nn_vector(", "rn_launch_synthesis("):
        assert launcher not in dropin, launcher
    for f in [f for f in os.listdir(CSRC) if f.startswith("batch")] + ["dropin.cpp", "host_io.cpp"]:
        for knob in KNOBS:
            assert f'"RNNOISE_AMD_{knob}"' not in _src(f), (f, knob)
