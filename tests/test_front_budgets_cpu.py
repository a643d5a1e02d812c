"""The compiled rn_nn_front_kernel keeps the budget its shape counts on (no GPU; read from the code object like
test_kernel_budgets_cpu.py): 64 streams per workgroup, eight waves, TWO workgroups per CU -- four waves per SIMD, so at most 128
VGPRs, and at most half of the CU's 160 KB of LDS each.  Measured when the shape was chosen: 118 VGPRs, 58,624 bytes of LDS."""
import os
import re
import subprocess
import tempfile

import pytest

from test_kernel_budgets_cpu import BUILD, LLVM, _code_object, _kernels

WORKGROUPS_PER_CU = 2
LDS_PER_CU = 160 * 1024
VGPRS_AT_FOUR_WAVES_PER_SIMD = 128  # 512 per lane and SIMD


@pytest.fixture(scope="module")
def front():
    obj = os.path.join(BUILD, "nn_mfma.o")
    if not os.path.exists(obj):
        pytest.skip("kernels not built (python -c 'import __graft_entry__ as g; g.build()')")
    meta, code = _kernels(obj)
    with tempfile.TemporaryDirectory() as td:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", _code_object(obj, td)], capture_output=True, text=True, check=True).stdout
    blk = next(b for b in notes.split("- .agpr_count:")[1:] if re.search(r"\.name:\s*rn_nn_front_kernel\s", b))
    lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", blk).group(1))
    agpr = int(re.match(r"\s*(\d+)", blk).group(1))
    threads = int(re.search(r"\.max_flat_workgroup_size:\s*(\d+)", blk).group(1))
    return dict(meta["rn_nn_front_kernel"], lds=lds, agpr=agpr, threads=threads, code=code["rn_nn_front_kernel"])


def test_no_spills_and_no_private_segment(front):
    assert front["vgpr_spill_count"] == 0 and front["private_segment_fixed_size"] == 0, front


def test_no_flat_or_scratch_memory_instructions(front):
    ins = front["code"]
    assert len(ins) > 200, len(ins)
    bad = [i for i in ins if i.startswith(("flat_", "scratch_"))]
    assert not bad, bad[:5]


def test_two_workgroups_fit_a_cu(front):
    assert front["threads"] == 512  # eight waves: two per SIMD and workgroup
    assert WORKGROUPS_PER_CU * front["lds"] <= LDS_PER_CU < (WORKGROUPS_PER_CU + 1) * front["lds"], front["lds"]
    assert front["lds"] <= 64 * 1024  # static LDS: no opt-in at launch
    assert front["vgpr_count"] + front["agpr"] <= VGPRS_AT_FOUR_WAVES_PER_SIMD, (front["vgpr_count"], front["agpr"])
