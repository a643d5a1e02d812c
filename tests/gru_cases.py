"""What the tests of the two GRU libraries share (test_gru_native_cpu.py, test_gru_stack_cpu.py, test_gru_native_gpu.py,
test_gru_stack_gpu.py): how a public header is read, and the small tools of the device tests."""
import ctypes as C
import os
import re

import numpy as np
import torch

import train_loss_ref as R

DEV = torch.device("cuda", 0)
FILL = 0x7A5A5A5A  # the guard word: a float no kernel here computes


# ---- the surface ----
def _declarations(header):
    """(return type, name, parameters) of every exported function of a header"""
    src = open(header).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return [(" ".join(ret.split()), name, " ".join(params.split()))
            for ret, name, params in re.findall(r"RNNOISE_EXPORT\s+([\w\s\*]+?)\b(rnnoise_\w+)\s*\(([^()]*)\)\s*;", src)]


def _fields(header, struct):
    """(name, ctypes type) of every field of a struct of a header; name[3] is an array of three"""
    src = open(header).read()
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", src, re.S)[1]
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        if decl.strip():
            kind = re.match(r"\s*(const float|float|long|int)\b", decl)[1]
            for f in decl.strip()[len(kind):].split(","):
                f = f.strip()
                base = C.c_void_p if f.startswith("*") else {"long": C.c_long, "int": C.c_int}[kind]
                name, count = re.match(r"\*?(\w+)(?:\[(\d+)\])?$", f).groups()
                fields.append((name, base * int(count) if count else base))
    return fields


def assert_shares_only_the_two_headers(pkg, unit, public_header):
    """the sources' side of "a library of its own": a gru unit's only quoted includes are its public header, the test shim (under its
    *_HOST switch) and the two shared headers; those hold no kernel, no exported call, no environment lookup and know no public gru
    header; both units are compiled under the one flags line, with -ffp-contract=off"""
    csrc = os.path.join(pkg, "csrc")
    text = open(os.path.join(csrc, unit)).read()
    quoted = re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M)
    assert sorted(quoted) == sorted([public_header, "gru_stack_shim.h", "../gru_cell.h", "../side_host.h"]), quoted
    assert re.search(r'^#ifdef RN_\w+_HOST\b[^\n]*\n#include "gru_stack_shim.h"\n#else\n', text, re.M)
    assert "getenv" not in text
    for shared in ("gru_cell.h", "side_host.h"):
        held = open(os.path.join(csrc, shared)).read()
        for word in ("__global__", 'extern "C"', "getenv", "rnnoise_amd_gru.h", "rnnoise_amd_gru_stack.h"):
            assert word not in held, (shared, word)
    mk = open(os.path.join(csrc, "Makefile")).read()
    name = os.path.splitext(os.path.basename(unit))[0]
    for var in ("SRCS", "ISRCS", "FLAGS", "HDRS", "SIDE_FLAGS"):
        assert name not in re.search(rf"^{var}\s*:?=\s*(.*)$", mk, re.M)[1], var
    assert "-ffp-contract=off" in re.search(r"^SIDE_FLAGS\s*:?=\s*(.*)$", mk, re.M)[1]
    rule = re.search(rf"^\$\(eval \$\(call SIDE_LIB,{os.path.dirname(unit)},{os.path.basename(unit)},{public_header},(.*)\)\)$", mk, re.M)
    assert rule and sorted(rule[1].split()) == ["gru_cell.h", "side_host.h"]  # the object depends on the shared headers it includes


def _injected_loss(gains, vad, records, gamma):
    return R.trainer_loss(gains, vad, records[:, 3:-1, R.FEATURES:R.FEATURES + R.BANDS], records[:, 3:-1, R.REC - 1:], gamma)


# ---- on the device ----
def u32(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def lay(t, frame_major):
    """a device copy of a [N, T, W] tensor: contiguous batch-first, or a transposed view of a [T, N, W] one"""
    t = t.to(DEV)
    return t.transpose(0, 1).contiguous().transpose(0, 1) if frame_major else t.contiguous()


def ratios(got, other, want, names):
    """per output: e_library / max(e_torch, 2^-23 max |X64|)"""
    out = {}
    for k in names:
        if want[k] is None or got[k] is None or other[k] is None:
            continue
        w = want[k]
        e_n = float((got[k].detach().cpu().double() - w).abs().max())
        e_t = float((other[k].detach().cpu().double() - w).abs().max())
        assert np.isfinite(e_n) and np.isfinite(e_t), k
        out[k] = e_n / max(e_t, 2.0 ** -23 * float(w.abs().max()), 1e-300)
    return out


def filled(n):
    return torch.full((n,), FILL, dtype=torch.int32, device=DEV).view(torch.float32)


def slot_mask(total, off, fs, rs, T, N, M):
    m = np.zeros(total, bool)
    for t in range(T):
        for s in range(N):
            m[off + t * fs + s * rs: off + t * fs + s * rs + M] = True
    return m


def net_outputs(net, x, A, B):
    gains, vad = net.forward_sequence(x)
    net.zero_grad()
    ((gains * A).sum() + (vad * B).sum()).backward()
    out = dict(gains=gains.detach(), vad=vad.detach())
    out.update({f"d {k}": v.grad.detach().clone() for k, v in net.named_parameters()})
    return out
