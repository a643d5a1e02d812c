"""What the CPU tests of every entry point of include/rnnoise_amd.h ask of the C boundary: declared once and listed in the binding,
exported by the libraries.  Each test module keeps its own list of names and its own further assertions."""
import os
import re
import subprocess

from conftest import ROOT
from rnnoise_amd import capi

HEADER = os.path.join(ROOT, "include", "rnnoise_amd.h")


def declared_once(names, ret="int"):
    """every name has exactly one RNNOISE_EXPORT prototype returning `ret` in the header and an entry in capi.EXPORTS; returns the
    header's text"""
    src = open(HEADER).read()
    for n in names:
        assert len(re.findall(rf"RNNOISE_EXPORT\s+{ret}\s+{n}\s*\(", src)) == 1, n
        assert n in capi.EXPORTS, n
    return src


def exported(so, names):
    """rnnoise_amd/<so> defines every name as a dynamic text symbol; returns all the names it defines"""
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "rnnoise_amd", so)], capture_output=True, text=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}\b", nm), (so, n)
    return [line.split()[-1] for line in nm.splitlines() if line.strip()]
