"""What the tests of the float-network runtime share (test_fnet_cpu.py, test_fnet_gpu.py): seeded networks and features, the float64
reference computed once per size, and the small tools of the device tests."""
import copy
import functools
import os
import subprocess

import numpy as np
import torch

from rnnoise_amd import float_net, fnet

DEV = torch.device("cuda", 0)
FILL = 0x7A5A5A5A  # the guard word: a float no kernel here computes
SIZES = ((16, 16), (32, 48), (128, 384))  # one unit tile; a quarter that is no whole chunk of 16; the real size
ROWS = (1, 15, 16, 17, 67)
FRAMES = (12, 35)
N_MAX, T_MAX = max(ROWS), max(FRAMES)


@functools.lru_cache(maxsize=None)
def net(cond, gru):
    """a FloatNet of that size as the trainer initialises it (torch's own initialisers), seeded, on the CPU, in eval mode"""
    torch.manual_seed(1000 * cond + gru)
    return float_net.FloatNet(cond, gru).eval()


@functools.lru_cache(maxsize=None)
def features(seed=0, n=N_MAX, t=T_MAX):
    """[n, t, 65] N(0, 1), float32, on the CPU: the cases take its first rows and frames"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, t, fnet.FEATURES), generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def x64(cond, gru, t):
    """FloatNet.forward in float64 on the CPU over the first t frames of all N_MAX rows -> (gains, vad): rows are independent, so a case
    of fewer rows takes the first of them"""
    n64 = copy.deepcopy(net(cond, gru)).double()
    n64.reset()
    with torch.no_grad():
        g, v = n64(features()[:, :t].double())
    return g, v


@functools.lru_cache(maxsize=None)
def seq64(cond, gru, t):
    """forward_sequence in float64 on the CPU: output k has seen frames k .. k + 4"""
    n64 = copy.deepcopy(net(cond, gru)).double()
    with torch.no_grad():
        return n64.forward_sequence(features()[:, :t].double())


@functools.lru_cache(maxsize=None)
def device_net(cond, gru):
    return copy.deepcopy(net(cond, gru)).to(DEV)


def runtime(cond, gru, max_frames=16):
    return fnet.FloatNetRuntime(net(cond, gru), device=0, max_frames=max_frames)


def u32(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def filled(n):
    return torch.full((n,), FILL, dtype=torch.int32, device=DEV).view(torch.float32)


def ratio(got, other, want):
    """e_got / max(e_other, 2^-23 max |want|) -> (ratio, e_got, the floor)"""
    w = want.double()
    e_g = float((got.detach().cpu().double() - w).abs().max())
    e_o = float((other.detach().cpu().double() - w).abs().max())
    assert np.isfinite(e_g) and np.isfinite(e_o)
    floor = max(e_o, 2.0 ** -23 * float(w.abs().max()), 1e-300)
    return e_g / floor, e_g, floor


def run_cuts(rt, x, cuts):
    """the frames of x through rt in calls of the given lengths -> gains, vad over all of them"""
    gs, vs, t = [], [], 0
    for c in cuts:
        g, v = rt(x[:, t:t + c])
        gs.append(g), vs.append(v)
        t += c
    assert t == x.shape[1]
    return torch.cat(gs, dim=1), torch.cat(vs, dim=1)


def build_c_example(out_dir):
    """tools/fnet_serve.c compiled as C against the two headers and linked against the two libraries -> the program's path"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg, exe = os.path.join(root, "rnnoise_amd"), os.path.join(out_dir, "fnet_serve")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", os.path.join(root, "tools", "fnet_serve.c"), "-I", os.path.join(root, "include"),
                    "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-L", pkg, "-lrnnoise_amd", "-lrnnoise_amd_fnet", "-L", "/opt/rocm/lib",
                    "-lamdhip64", "-lm", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe
