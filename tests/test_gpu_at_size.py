"""GPU suite, at BASELINE.json's full sizes: configs[2] (65,536 streams, the bench default; runs the >= 24,576-stream
build of the analysis kernel and 4096 MFMA tiles) and configs[3] (sparser blob, 32,768 streams).  An oracle run of
65,536 streams would take hours, so the checks are the size-independent ones: tiled replicas of a 32-stream block must
stay bit-identical to each other (no cross-talk, no dependence on the tile / CU / XCD a stream lands on), and the block
itself is checked bit for bit against the oracle, including a stream that starts silent inside a live MFMA tile.  The mixed
block of tests/stream_mix.py (389 streams of every kind, compared stream by stream) runs at batch sizes that reach every kernel
form, with NaN / Inf in copies of one of its streams, and through masked, stream-list and per-stream-phase lock-step calls with
NaN in every absent row; under linked gains with controls and two model slots (stream_mix.LINK_CASES), the same two ways; and
through the PCM front ends -- rate table, format table, strides, channels, int16 calls (stream_mix.DRESS_CASES) --, the same two ways,
against a chain on the CPU alone; and through the chunk calls -- full-size and list pushes of any count, in place on the staging
buffer, a reset with samples pending, a move with FIFO records (stream_mix.CHUNK_CASES) -- against the header's closed form on the CPU
alone; and through the feature calls -- the network alone on the block's features as training records, in cuts, layouts, two models,
with poisoned streams (stream_mix.FEATURE_CASES) -- against the oracle's compute_rnn and the float64 restatement of the trainer's loss.
Also here: the device-vs-host log10 sweep behind DESIGN.md's "known residuals", and two processes sharing one GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, load_blob
from oracle.binding import Oracle
import stream_mix
from rnnoise_amd import capi, synth
from test_gpu_parity import oracle_run

pytestmark = pytest.mark.gpu


def _tiled_check(blob, N, calls, silent_stream):
    """N streams = N/32 replicas of a 32-stream block, fed from HBM through rnnoise_batch_process_device in `calls` (frames per
    call) on the batch's DEFAULT schedule -- what bench.py times: multi-frame calls run the three-stream frame pipeline
    (high-pass two frames ahead, analysis(f+1) beside network + synthesis(f)), the 6-slot pitch ring and the 3 spectra slots
    wrap, call boundaries fall inside the ring, the network runs layer-wise from 10,240 streams up and the analysis kernel
    four streams per workgroup.  A one-frame call in the middle takes the unpipelined route through the same state."""
    import torch
    T = sum(calls)
    base = synth.batch_pcm(range(32), T)
    base[:3, silent_stream] = 0                       # silent for 3 frames, then live
    base[T - 5:T - 3, (silent_stream + 3) % 32] = 0   # another one goes silent across the last call boundary region
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(base).to(dev).repeat(1, N // 32, 1).contiguous()
    d_out = torch.empty_like(d_in)
    d_vad = torch.empty((T, N), device=dev)
    d_gains = torch.empty((T, N, 32), device=dev)
    m = capi.Model(blob)
    b = capi.Batch(m, N)
    assert b.set_nn_path(1) == 1                      # MFMA path is the default at this size
    st = torch.cuda.current_stream().cuda_stream
    f = 0
    for n in calls:
        b.process_device(d_out[f].data_ptr(), d_in[f].data_ptr(), d_vad[f].data_ptr(), d_gains[f].data_ptr(), n, st)
        f += n
    torch.cuda.synchronize()
    for name, t, w in (("pcm", d_out, 480), ("gains", d_gains, 32), ("vad", d_vad, 1)):
        r = t.view(torch.int32).reshape(T, N // 32, 32 * w)
        assert bool((r == r[:, :1]).all().item()), f"replicated streams diverged ({name})"
    out, gains, vad = d_out[:, :32].cpu().numpy(), d_gains[:, :32].cpu().numpy(), d_vad[:, :32].cpu().numpy()
    del d_in, d_out, d_gains, d_vad
    want = oracle_run(blob, base)
    assert want["silence"][:, silent_stream].any() and not want["silence"][:, 0].any()
    assert_bits_equal(out, want["out"], "pcm")
    assert_bits_equal(gains, want["gains"], "gains")
    assert_bits_equal(vad, want["vad"], "vad")
    for s_ in (0, 15, 16, silent_stream, 31):
        assert_bits_equal(b.export_state(N - 32 + s_), want["state"][s_], f"state of stream {N - 32 + s_}")
    # a stream from the middle of the batch as well (different XCD / tile than the first and the last block)
    mid = (N // 2 // 32) * 32
    assert_bits_equal(b.export_state(mid + 7), want["state"][7], f"state of stream {mid + 7}")
    b.close()
    m.close()


@pytest.mark.parametrize("rcp_profile", ["intel", "host"], indirect=True)
def test_65536_stream_batch_properties(blob_default, rcp_profile):
    """BASELINE configs[2] = the bench default: 14 frames as calls of 5 + 1 + 8 -- on the profile of the committed goldens and on
    "host", the profile a deployed process (and bench.py) runs on: the rcpps of this machine's CPU"""
    _tiled_check(blob_default, 65536, (5, 1, 8), silent_stream=21)


@pytest.mark.parametrize("rcp_profile", ["intel", "host"], indirect=True)
def test_sparser_model_32768(blob_little, rcp_profile):
    """BASELINE configs[3]: the sparser blob at 32,768 streams, 14 frames as calls of 5 + 1 + 8 -- on the goldens' profile and on
    the profile a deployed process runs on (this machine's rcpps)"""
    _tiled_check(blob_little, 32768, (5, 1, 8), silent_stream=9)


def _synth_block(T, silent_stream):
    """the 32-stream block of the synth recipe, with a stream silent for its first 3 frames and one silent across the last call boundary"""
    base = synth.batch_pcm(range(32), T)
    base[:3, silent_stream] = 0
    base[T - 5:T - 3, (silent_stream + 3) % 32] = 0
    return base


def _ragged_check(blob, N, calls, block, want=None, silent_stream=None, nn_path=1, state_streams=None, every_call=False, poisoned=(), ragged=True):
    """_tiled_check for a batch size that is NOT a multiple of anything: N = B q + r streams = q copies of a B-stream `block` and the
    first r streams of one more (stream i takes block stream i mod B).  Every kernel of the default schedule then has a partial unit at
    the end of its grid -- the lane = stream high-pass a partial wave, the four-stream analysis workgroups a partial workgroup, the front
    kernel a partial 16-stream tile, the four-wave GRU layer kernel and the dense kernel a partial 64-stream group -- whose surplus lanes
    work on clamped addresses and must store nothing.  Whole copies are compared among themselves, the ragged tail with the head of
    copy 0, and every stream's pcm / gains / vad with the oracle's run of its block stream (`want`), on the device; states are exported
    from `state_streams` (default: the tail and the middle).  every_call: after every call the features, silence flag and pitch of
    the call's last frame (debug_last) of all N streams against the oracle's frame.  poisoned: (frame, stream, sample, value) writes
    into the input -- those streams' own output is not checked, nor the copy comparisons.  ragged: N is a multiple of neither B nor
    4, 16, 64."""
    import torch
    T, B = sum(calls), block.shape[1]
    q, r = N // B, N % B
    assert not ragged or (r and N % 64 and N % 16 and N % 4)
    if want is None:
        want = oracle_run(blob, block)
    if silent_stream is not None:
        assert want["silence"][:, silent_stream].any() and not want["silence"][:, 0].any()
    dev = torch.device("cuda", 0)
    idx = torch.arange(N, device=dev) % B
    d_in = torch.from_numpy(np.ascontiguousarray(block, np.float32)).to(dev)[:, idx].contiguous()
    bad = sorted({s for _, s, _, _ in poisoned})
    for t, s, k, v in poisoned:
        d_in[t, s, k] = float(v)
    live = np.ones(N, bool)
    live[bad] = False
    d_out = torch.empty_like(d_in)
    d_vad = torch.empty((T, N), device=dev)
    d_gains = torch.empty((T, N, 32), device=dev)
    m = capi.Model(blob)
    b = capi.Batch(m, N)
    if nn_path is not None:
        old = b.set_nn_path(nn_path)
        assert old in (0, 1) and (N <= 512 or old == 1)   # the MFMA path is the default above 512 streams
    st = torch.cuda.current_stream().cuda_stream
    f = 0
    for n in calls:
        b.process_device(d_out[f].data_ptr(), d_in[f].data_ptr(), d_vad[f].data_ptr(), d_gains[f].data_ptr(), n, st)
        f += n
        if every_call:
            torch.cuda.synchronize()
            feats, sil, pitch = b.debug_last()
            at = idx.cpu().numpy()
            for name, got in (("features", feats), ("silence", sil), ("pitch", pitch)):
                assert_bits_equal(got[live], want[name][f - 1][at][live], f"{name} of frame {f - 1} (the last of a {n}-frame call)")
    torch.cuda.synchronize()
    d_live = torch.from_numpy(live).to(dev)
    for name, t, w in (("out", d_out, 480), ("gains", d_gains, 32), ("vad", d_vad, 1)):
        t = t.reshape(T, N, w).view(torch.int32)
        if not poisoned:
            whole = t[:, :B * q].reshape(T, q, B * w)
            assert bool((whole == whole[:, :1]).all().item()), f"replicated streams diverged ({name})"
            assert bool((t[:, B * q:] == t[:, :r]).all().item()), f"the ragged tail differs from the head of block 0 ({name})"
        ref = torch.from_numpy(np.ascontiguousarray(want[name], np.float32)).to(dev).reshape(T, B, w).view(torch.int32)[:, idx]
        ne = (t != ref).any(-1) & d_live
        if bool(ne.any().item()):
            where = ne.nonzero()[:5].tolist()
            raise AssertionError(f"{name}: {int(ne.sum().item())} of {T * int(d_live.sum().item())} stream-frames differ from the oracle, "
                                 f"first (frame, stream) {where}, block streams {[s_ % B for _, s_ in where]}")
        del ref, ne
    del d_in, d_out, d_gains, d_vad
    if state_streams is None:
        state_streams = (N - 1, N - r, N - r - 1, (N // 2 // B) * B + silent_stream)   # the last, the tail's first, the last whole copy's last
    for s_ in state_streams:
        assert_bits_equal(b.export_state(s_), want["state"][s_ % B], f"state of stream {s_} (block stream {s_ % B})")
    b.close()
    m.close()


@pytest.mark.rcp("host")
@pytest.mark.parametrize("which", ["default", "little"])
def test_ragged_40037_streams(blob_default, blob_little, which):
    """VERDICT r5 Weak #1: the kernels that are the at-size defaults -- the four-wave rn_nn_gru_kernel (more 64-stream groups than CUs:
    > 16,384 streams) and the lane-per-stream high-pass inside pipelined calls -- on a batch with a partial tile (40,037 = 16 x
    2,502 + 5), a partial group (64 x 625 + 37), a partial analysis workgroup and a partial high-pass wave; default and sparser blob,
    default schedule, 14 frames as calls of 5 + 1 + 8.  Arithmetic under test: src/nnet.c:65-94, src/denoise.c:409-419."""
    _ragged_check(blob_default if which == "default" else blob_little, 40037, (5, 1, 8), _synth_block(14, 3), silent_stream=3)


@pytest.mark.rcp("host")
def test_ragged_10277_streams_just_above_the_network_switch(blob_default):
    """The layer-wise network starts at 10,240 streams (rnnoise_amd/csrc/dispatch.h: RN_NN_LAYERS; 16,384 until round 6's last day): a
    ragged batch just above the switch -- 10,277 = 16 x 642 + 5 = 64 x 160 + 37, the eight-wave layer kernel (fewer 64-stream groups
    than CUs) with a partial tile and a partial group -- and, below, the largest batches of the tile kernel on both sides of 8,192
    streams (two tiles per CU, then three).  Arithmetic under test: src/nnet.c:65-94, src/rnn.c:44-60."""
    _ragged_check(blob_default, 10277, (4, 1, 3), _synth_block(8, 3), silent_stream=3)


_MIX = {}


def _mix(blob, profile):
    """tests/stream_mix.py's block and the oracle's run of it, once per module and rcpps profile"""
    if profile not in _MIX:
        pcm, _ = stream_mix.block()
        _MIX[profile] = pcm, stream_mix.oracle_block(blob, pcm)
    return _MIX[profile]


def _need_256_cus():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"{cus} CUs: the forms stream_mix.CASES reach are chosen for 256")


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path,calls", stream_mix.CASES, ids=[f"n{n}-path{p}" for n, p, _ in stream_mix.CASES])
def test_stream_mix_at_every_form(blob_default, rcp_profile, n, path, calls):
    """The mixed block of tests/stream_mix.py -- pitch from 60 to 767, silence that flips frame by frame and at call boundaries,
    extreme and edge signals, a stream of zeros, a permutation that puts different kinds of stream side by side -- copied over n
    streams and fed through the batch's default schedule in stream_mix.CALLS: with the network paths of CASES every form of every
    stage runs (tests/test_stream_mix_cpu.py: the forms on 256 CUs), among them the rows of one wave of rn_analysis_kernel's narrow
    phases, of one tile and of one layer-kernel group at different pitch, remove_doubling lengths and silence.  Every stream's pcm,
    gains and vad, and after every call the last frame's features, silence and pitch of every stream, against the oracle; then the
    state of every block position, each from a different copy."""
    _need_256_cus()
    pcm, want = _mix(blob_default, rcp_profile)
    B = pcm.shape[1]
    # block position p from copy (7 p) mod (the copies holding p)
    states = [p + (7 * p) % ((n - p + B - 1) // B) * B for p in range(min(B, n))]
    _ragged_check(blob_default, n, calls, pcm[:sum(calls)], want=want, nn_path=path, state_streams=states, every_call=True,
                  ragged=False)


_MASKED_MIX = {}
SENTINEL_OUT = 0x7FA0BEEF                 # (int32 bit patterns: signalling NaNs that no arithmetic produces)
SENTINEL_AUX = 0x7FB0CAFE


def _masked_mix(blob, profile):
    """the block and the oracle's run of it under stream_mix's presence schedule and resets, once per module and rcpps profile"""
    if profile not in _MASKED_MIX:
        pcm, _ = stream_mix.block()
        _MASKED_MIX[profile] = pcm, stream_mix.oracle_block(blob, pcm, presence=stream_mix.presence(), resets=stream_mix.RESET)
    return _MASKED_MIX[profile]


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path,calls", stream_mix.CASES, ids=[f"n{n}-path{p}" for n, p, _ in stream_mix.CASES])
def test_stream_mix_masked_and_listed_at_every_form(blob_default, rcp_profile, n, path, calls):
    """The mixed block through the serving API (include/rnnoise_amd.h): stream_mix.KINDS -- masked calls, stream-list calls with
    out-of-range entries and lock-step calls on a batch in per-stream frame phase, one-frame and pipelined -- with the presence
    schedule of stream_mix.presence() and a reset of stream_mix.RESET's copies before call RESET_BEFORE, on n copies of the block and
    the network paths of CASES: every form rn_plan chooses in per-stream phase and in list calls runs (tests/test_stream_mix_cpu.py),
    among them the lane-per-stream high-pass with the lanes of one wave at different ring slots.  Every absent input row is NaN (absent
    rows are not read), out is pre-filled with one sentinel and vad / gains with another: every present stream-frame matches the oracle
    run on that position's present frames bit for bit in pcm, vad and gains, every absent row keeps out's sentinel and reads vad 0 and
    32 zero gains.  After every call debug_last's defined entries against the oracle's frame; at the end the state of every block
    position (each from a different copy), of the reset copies, and of the position absent from every masked and list frame."""
    import torch
    _need_256_cus()
    assert calls == stream_mix.CALLS
    pcm, want = _masked_mix(blob_default, rcp_profile)
    B = pcm.shape[1]
    idx = np.arange(n) % B
    dev = torch.device("cuda", 0)
    blk = torch.from_numpy(pcm).to(dev)
    ref = {k: torch.from_numpy(np.ascontiguousarray(want[k], np.float32)).to(dev).view(torch.int32) for k in ("out", "vad", "gains")}
    m = capi.Model(blob_default)
    b = capi.Batch(m, n)
    if path is not None:
        b.set_nn_path(path)
    st = torch.cuda.current_stream().cuda_stream
    never = [s for s in range(n) if idx[s] == stream_mix.SPECIAL["never"]]
    never_state = {}
    for c, kind in enumerate(stream_mix.KINDS):
        plan = stream_mix.call_plan(n, c)
        fr = plan["frames"]
        k, R = len(fr), len(plan["src"])
        src = torch.from_numpy(plan["src"]).to(dev)
        present = torch.from_numpy(plan["present"]).to(dev)
        x = stream_mix.call_input(blk, fr, src, present).contiguous()
        out = torch.empty_like(x)
        out.view(torch.int32).fill_(SENTINEL_OUT)
        vad = torch.empty((k, R), device=dev)
        gains = torch.empty((k, R, 32), device=dev)
        vad.view(torch.int32).fill_(SENTINEL_AUX)
        gains.view(torch.int32).fill_(SENTINEL_AUX)
        ptrs = (out.data_ptr(), x.data_ptr(), vad.data_ptr(), gains.data_ptr())
        if kind == "lock":
            b.process_device(*ptrs, k, st)
        else:
            act = torch.from_numpy(plan["active"]).to(dev).contiguous()
            if kind == "masked":
                b.process_masked_device(*ptrs, act.data_ptr(), k, st)
            else:
                rows = torch.from_numpy(plan["rows"]).to(dev)
                b.process_list_device(*ptrs, rows.data_ptr(), R, act.data_ptr(), k, st)
        torch.cuda.synchronize()
        what = f"call {c} ({kind}, frames {fr.start}..{fr.stop - 1})"
        for name, got, w in (("out", out, 480), ("vad", vad, 1), ("gains", gains, 32)):
            r = ref[name][fr.start:fr.stop][:, src].reshape(k, R, w)
            r = torch.where(present[..., None], r, SENTINEL_OUT if name == "out" else 0)
            ne = (got.view(torch.int32).reshape(k, R, w) != r).any(-1)
            if bool(ne.any().item()):
                where = ne.nonzero()[:5].tolist()
                raise AssertionError(f"{what}: {name} of {int(ne.sum().item())} of {k * R} row-frames differs, first (frame, row) "
                                     f"{where}: present {[bool(plan['present'][f, i]) for f, i in where]}, list entry "
                                     f"{[None if plan['rows'] is None else int(plan['rows'][i]) for _, i in where]}, block position "
                                     f"{[int(plan['src'][i]) for _, i in where]}")
            del r, ne
        del x, out, vad, gains
        # debug_last: every stream after a masked or lock-step call (silence 2 where absent), the listed streams after a list call
        feats, sil, pitch = b.debug_last()
        last = fr.stop - 1
        streams = np.arange(n) if plan["rows"] is None else plan["rows"][(plan["rows"] >= 0) & (plan["rows"] < n)]
        here = stream_mix.presence()[last, streams % B] != 0
        assert (sil[streams[~here]] == 2).all(), f"{what}: silence of streams absent from frame {last}"
        on = streams[here]
        for name, got in (("features", feats), ("silence", sil), ("pitch", pitch)):
            assert_bits_equal(got[on], want[name][last][on % B], f"{what}: {name} of frame {last}")
        if c + 1 == stream_mix.RESET_BEFORE:
            b.reset_streams([s for s in range(n) if idx[s] in stream_mix.RESET])
        if kind == "lock":
            never_state = {s: b.export_state(s) for s in (never[0], never[-1])}
    torch.cuda.synchronize()
    # every block position from a different copy, as the lock-step test; the last copy of every reset position; the position that
    # missed every masked and list frame as it was after the last lock-step call
    states = [p + (7 * p) % ((n - p + B - 1) // B) * B for p in range(min(B, n))]
    states += [p + (n - 1 - p) // B * B for p in stream_mix.RESET if p < n]
    for s_ in states:
        assert_bits_equal(b.export_state(s_), want["state"][s_ % B], f"state of stream {s_} (block stream {s_ % B})")
    for s_, st_ in never_state.items():
        assert_bits_equal(b.export_state(s_), st_, f"state of stream {s_}, absent from every frame since the last lock-step call")
    b.close()
    m.close()


# ---- the block through the PCM front ends (stream_mix.DRESS_CASES): rate table, format table, strides, channels, int16 calls ----
_DRESSED = {}
SENTINEL_S16 = 0x5AA5                     # what `out` of an int16 call holds before it (bytes A5 5A)
PAD = 32                                  # samples behind the last slot of every PCM buffer: nothing may land there either


def _dressed(blob, profile, scheduled):
    """the CPU chain's run of the block (stream_mix.dress_expectation) under every variant, lock-step or under the presence schedule,
    once per module and rcpps profile.  No GPU takes part in it"""
    key = (profile, scheduled)
    if key not in _DRESSED:
        _DRESSED[key] = {v: stream_mix.dress_expectation(blob, v, scheduled) for v in stream_mix.VARIANTS}
    return _DRESSED[key]


def _dressed_run(blob, profile, case, scheduled):
    """One DRESS_CASES batch through lock-step CALLS or (scheduled) through KINDS with presence(), NaN / junk in everything of `in`
    that no present row owns and the reset before RESET_BEFORE.  After every call the whole allocation of `out` -- every present
    row's first M samples or bytes from the CPU chain, the sentinel everywhere else: the rest of the slot, the padding between rows
    and frames, absent rows, the channels of absent siblings --, vad and gains of every row (0 where absent), and `in` untouched; at
    the end the state of every block position from a different copy, the snapshots of 16 positions across all of their copies, and
    the tables."""
    import torch
    n, path, typ, C, layout = case
    s16 = typ == "int16"
    B, M = stream_mix.B, 480
    want = _dressed(blob, profile, scheduled)
    dev = torch.device("cuda", 0)
    kinds = ("float",) if not s16 else ("s16", "law")                         # the variants of this batch's rows: index = companded
    codes, Ms = stream_mix.rate_codes(), stream_mix.frame_lengths()
    comp_h = stream_mix.dress_companded(n, C, s16)
    table_h = stream_mix.dress_formats(n, C, s16)
    idx = np.arange(n) % B

    def bits(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.float32 else a).to(dev)

    x_in = {v: bits(stream_mix.dress_input(v)) for v in kinds}                # (T, B, 480) int32 bits | int16 | uint8
    ref_out = {v: bits(want[v]["out"]) for v in kinds}
    ref_vad = torch.cat([bits(want[v]["vad"]) for v in kinds], 1)             # (T, variants * B): row companded * B + position
    ref_gains = torch.cat([bits(want[v]["gains"]) for v in kinds], 1)
    comp = torch.from_numpy(comp_h).to(dev)
    Ms_d = torch.from_numpy(Ms).to(dev)
    lane = torch.arange(M, device=dev)
    el = torch.int16 if s16 else torch.int32
    junk, sentinel = (stream_mix.JUNK_S16, SENTINEL_S16) if s16 else (0x7FC00000, SENTINEL_OUT)

    m = capi.Model(blob)
    b = capi.Batch(m, n)
    if path is not None:
        b.set_nn_path(path)
    b.set_stream_rates(capi.code_rate(codes[idx]))
    b.set_stream_formats(table_h)
    if C > 1:
        assert b.set_pcm_channels(C) == 1
    st = torch.cuda.current_stream().cuda_stream
    for c in range(len(stream_mix.CALLS)):
        plan = stream_mix.dress_call_plan(n, C, c, scheduled)
        kind, fr = plan["kind"], plan["frames"]
        k, R = len(fr), len(plan["src"])
        G = R // C
        strides = stream_mix.dress_strides(layout, C, k, R)
        fs, rs = strides or (G * M * C, M * C)
        if strides:
            b.set_pcm_layout(fs, rs)
        size = (k - 1) * fs + (G - 1) * rs + M * C + PAD
        src = torch.from_numpy(plan["src"]).to(dev)
        present = torch.from_numpy(plan["present"]).to(dev)
        rcomp = comp[torch.from_numpy(plan["stream"]).to(dev)]                # (R,) the row holds bytes
        own = present[:, :, None] & (lane[None, None, :] < Ms_d[src][None, :, None])   # (k, R, 480): what a present row owns

        def slots(flat, as_bytes=False):
            """(k, G, M, C) view of the samples (bytes of companded groups) of a flat buffer: [f, g, i, ch] at f fs + g rs + i C + ch"""
            w = 2 if as_bytes else 1
            return (flat.view(torch.uint8) if as_bytes else flat).as_strided((k, G, M, C), (w * fs, w * rs, C, 1))

        def rows(a):
            return a.reshape(k, G, C, M).permute(0, 1, 3, 2)

        def put(flat, values, where, as_bytes=False):
            v = slots(flat, as_bytes)
            v.copy_(torch.where(rows(where), rows(values), v))

        def gather(t):
            return t[fr.start:fr.stop][:, src]

        d_in = torch.full((size,), junk, dtype=el, device=dev)
        d_exp = torch.full((size,), sentinel, dtype=el, device=dev)
        if s16:
            lin, law = own & ~rcomp[None, :, None], own & rcomp[None, :, None]
            put(d_in, gather(x_in["s16"]), lin)
            put(d_in, gather(x_in["law"]), law, as_bytes=True)
            put(d_exp, gather(ref_out["s16"]), lin)
            put(d_exp, gather(ref_out["law"]), law, as_bytes=True)
        else:
            put(d_in, gather(x_in["float"]), own)
            put(d_exp, gather(ref_out["float"]), own)
        d_in0 = d_in.clone()
        d_out = torch.full((size,), sentinel, dtype=el, device=dev)
        vad = torch.full((k, R), SENTINEL_AUX, dtype=torch.int32, device=dev)
        gains = torch.full((k, R, 32), SENTINEL_AUX, dtype=torch.int32, device=dev)
        ptrs = (d_out.data_ptr(), d_in.data_ptr(), vad.data_ptr(), gains.data_ptr())
        if kind == "lock":
            b.process_device(*ptrs, k, st, s16=s16)
        else:
            act = torch.from_numpy(plan["active"]).to(dev).contiguous()
            if kind == "masked":
                b.process_masked_device(*ptrs, act.data_ptr(), k, st, s16=s16)
            else:
                lst = torch.from_numpy(plan["rows"]).to(dev)
                b.process_list_device(*ptrs, lst.data_ptr(), R, act.data_ptr(), k, st, s16=s16)
        torch.cuda.synchronize()
        what = f"call {c} ({kind}, frames {fr.start}..{fr.stop - 1})"

        def where_rows(ne):
            w = ne.nonzero()[:5].tolist()
            return (f"first (frame, row) {w}: present {[bool(plan['present'][f, i]) for f, i in w]}, stream {[int(plan['stream'][i]) for _, i in w]}, "
                    f"block position {[int(plan['src'][i]) for _, i in w]}, rate code {[int(codes[plan['src'][i]]) for _, i in w]}, "
                    f"companded {[bool(comp_h[plan['stream'][i]]) for _, i in w]}")

        if not torch.equal(d_out, d_exp):
            # which rows: the samples (and, in an int16 call, the bytes) of every row's positions, present or not
            ne = (slots(d_out) != slots(d_exp)).permute(0, 1, 3, 2).reshape(k, R, M).any(-1)
            if s16:
                ne |= (slots(d_out, True) != slots(d_exp, True)).permute(0, 1, 3, 2).reshape(k, R, M).any(-1)
            at = int((d_out != d_exp).nonzero()[0])
            raise AssertionError(f"{what}: out differs in {int((d_out != d_exp).sum())} of {size} samples, the first at sample {at} "
                                 f"(frame stride {fs}, group stride {rs}, {C} channels); {int(ne.sum())} of {k * R} row-frames, " + where_rows(ne))
        assert torch.equal(d_in, d_in0), f"{what}: `in` was written"
        vidx = rcomp.long() * B + src
        for name, got, ref in (("vad", vad, ref_vad), ("gains", gains, ref_gains)):
            r = ref[fr.start:fr.stop][:, vidx].reshape(k, R, -1)
            r = torch.where(present[..., None], r, 0)
            ne = (got.reshape(k, R, -1) != r).any(-1)
            if bool(ne.any().item()):
                raise AssertionError(f"{what}: {name} of {int(ne.sum())} of {k * R} row-frames differs, " + where_rows(ne))
        del d_in, d_in0, d_out, d_exp, vad, gains
        if scheduled and c + 1 == stream_mix.RESET_BEFORE:
            b.reset_streams(np.flatnonzero(np.isin(idx, stream_mix.RESET)))
    del x_in, ref_out, ref_vad, ref_gains
    # every block position from a different copy
    streams = np.array([p + (7 * p) % ((n - p + B - 1) // B) * B for p in range(min(B, n))])
    if scheduled:
        streams = np.unique(np.concatenate([streams, [p + (n - 1 - p) // B * B for p in stream_mix.RESET if p < n]]))   # (a list names a stream once)
    snap = b.save_streams(streams)
    state = np.stack([want[kinds[int(comp_h[s_])]]["state"][s_ % B] for s_ in streams])
    bad = np.flatnonzero((snap[:, :capi.STATE_FLOATS].view(np.uint32) != state.view(np.uint32)).any(1))
    assert not len(bad), (f"state of {len(bad)} of {len(streams)} streams differs, first (stream, block position, companded) "
                          f"{[(int(streams[i]), int(streams[i]) % B, bool(comp_h[streams[i]])) for i in bad[:5]]}")
    # 16 positions, every copy: one record per variant (a resampler history that drifts between copies shows here)
    for p in range(3, min(B, n), 24)[:16]:
        copies = np.arange(p, n, B)
        snap = b.save_streams(copies).view(np.uint32)
        for v in (False, True):
            recs = snap[comp_h[copies] == v]
            assert (recs == recs[:1]).all(), f"snapshots of block position {p} differ between its {len(recs)} copies (companded: {v})"
    assert_bits_equal(b.stream_rates(), capi.code_rate(codes[idx]).astype(np.int32), "the rate table")
    assert_bits_equal(b.stream_formats(), table_h, "the format table")
    assert b.pcm_channels == C
    b.close()
    m.close()


@pytest.mark.rcp("host")
@pytest.mark.parametrize("case", stream_mix.DRESS_CASES, ids=stream_mix.DRESS_IDS)
def test_stream_mix_dressed_at_every_form(blob_default, rcp_profile, case):
    """The mixed block through the PCM front ends (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates, _set_stream_formats,
    _set_pcm_layout, _set_pcm_channels, the _s16 calls) at every kernel form: n copies of the block with stream_mix.rate_codes() and
    formats() on its positions -- 8 to 48 kHz, linear, mu-law and A-law side by side in every tile --, in lock-step calls of
    stream_mix.CALLS under the sample type, channel count and layout of DRESS_CASES.  The expectation is a chain on the CPU alone
    (stream_mix.dress_expectation: decode, resample.up, the oracle, resample.down, the truncating cast, encode), one run per block
    position and variant; every row of every copy is compared with it on the device, bit for bit, with everything a row does not own
    held to its sentinel (_dressed_run)."""
    _need_256_cus()
    _dressed_run(blob_default, rcp_profile, case, scheduled=False)


@pytest.mark.rcp("host")
@pytest.mark.parametrize("case", stream_mix.DRESS_CASES, ids=stream_mix.DRESS_IDS)
def test_stream_mix_dressed_masked_and_listed_at_every_form(blob_default, rcp_profile, case):
    """The same batches through the serving API: stream_mix.KINDS with presence() -- masked calls, list calls that list whole channel
    groups in a pseudo-random order with three entries that name no stream, lock-step calls in per-stream frame phase -- and a reset
    of RESET's copies before call RESET_BEFORE.  An absent frame advances neither a row's state nor its resampler histories, a reset
    zeroes both; absent float rows hold NaN, absent int16 rows junk; an absent channel's samples of a group slot keep the sentinel
    beside its siblings' output."""
    _need_256_cus()
    _dressed_run(blob_default, rcp_profile, case, scheduled=True)


# ---- the block through the chunk calls (stream_mix.CHUNK_CASES): in place on the staging buffer, a mask the device writes ----
_CHUNKED = {}


def _chunked(blob, profile, hz, typ):
    """the CPU chain's chunk expectation of the block (stream_mix.chunk_expectation), once per module, rcpps profile, rate and sample
    type; at 48 kHz float the plain positions take their frames from the lock-step run of _mix.  No GPU takes part in it"""
    key = (profile, hz, typ)
    if key not in _CHUNKED:
        lock = _mix(blob, profile)[1] if (hz, typ) == (48000, "float") else None
        _CHUNKED[key] = stream_mix.chunk_expectation(blob, hz, typ, lock=lock)
    return _CHUNKED[key]


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path,hz,typ", stream_mix.CHUNK_CASES, ids=stream_mix.CHUNK_IDS)
def test_stream_mix_chunked_at_every_form(blob_default, rcp_profile, n, path, hz, typ):
    """The mixed block through the chunk calls (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks[_list][_s16],
    rnnoise_batch_save / load_chunk_fifos_device) at every kernel form: n copies of the block, every position's signal as one row at
    the batch rate, handed over in the pushes of stream_mix.CHUNK_PUSHES -- full-size and list pushes, F = 1 to 7, every count from 0
    to max_count, so that the rows of one tile, wave and GRU group complete 0 .. F frames in the same call from FIFOs at every fill.
    The masked call inside runs in place on the batch's staging buffer, with rows M apart and a mask the scatter kernel wrote.  The
    expectation is the closed form y = 0^M ++ z on the CPU alone (stream_mix.chunk_expectation).  Every push: NaN / 31000 behind every
    row's count of `in`; the whole allocation of `out` -- the first count samples of every row from the expectation, the sentinel in
    everything else: the rest of the row, the rows of list entries that name no stream, the padding behind the buffer --, frames, vad
    and gains of every row (zeros from row k on), `in` untouched, and chunk_fill() of every stream; all as bit patterns, on the
    device.  Before push CHUNK_RESET_BEFORE RESET's copies are reset with samples pending; before push CHUNK_MOVE_BEFORE the whole
    batch moves to a fresh one through the device forms of snapshots and FIFO records and a shuffled list: the records of every stream
    against the CPU's, the portable state of every block position (each from a different copy) against the oracle's after its
    completed frames, and the destination's records the same bytes.  At the end the states as in the masked test, and empty FIFOs."""
    import torch
    _need_256_cus()
    B, T, s16 = stream_mix.B, stream_mix.T, typ == "int16"
    M = stream_mix.chunk_frame(hz)
    exp, s = _chunked(blob_default, rcp_profile, hz, typ), stream_mix.chunk_schedule(M)
    dev = torch.device("cuda", 0)
    el = torch.int16 if s16 else torch.int32
    junk, sentinel = (31000, SENTINEL_S16) if s16 else (0x7FC00000, SENTINEL_OUT)
    top, Fmax = int(s["max_count"].max()), int(s["F"].max())
    idx = np.arange(n) % B

    def padded(a, extra):
        """a (B, W, ...) as bit patterns on the device, with `extra` zero columns behind it: every gather below stays inside"""
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.float32 else a).to(dev)
        return torch.cat([t, torch.zeros((B, extra) + t.shape[2:], dtype=t.dtype, device=dev)], 1)

    x, y = padded(exp["x"], top), padded(exp["y"], top)
    ref_vad, ref_gains = padded(exp["vad"], Fmax), padded(exp["gains"], Fmax)
    cum, done, k_all = (torch.from_numpy(s[key].copy()).to(dev) for key in ("cum", "done", "k"))
    m = capi.Model(blob_default)

    def batch():
        b_ = capi.Batch(m, n)
        if path is not None:
            b_.set_nn_path(path)
        if hz != 48000:
            b_.set_pcm_rate(hz)
        assert b_.frame == M
        return b_

    b = batch()
    st = torch.cuda.current_stream().cuda_stream
    # every block position from a different copy, as the masked test
    one_each = np.array([p + (7 * p) % ((n - p + B - 1) // B) * B for p in range(min(B, n))])
    for q, push in enumerate(stream_mix.CHUNK_PUSHES):
        if q == stream_mix.CHUNK_RESET_BEFORE:
            hit = np.flatnonzero(np.isin(idx, stream_mix.RESET))
            assert b.chunk_fill()[hit].all()                                  # (something to drop on every one of them)
            b.reset_streams(hit)
            assert not b.chunk_fill()[hit].any()
        if q == stream_mix.CHUNK_MOVE_BEFORE:
            order = np.random.default_rng([n, 700]).permutation(n).astype(np.int32)
            d_list = torch.from_numpy(order).to(dev)
            d_snap = torch.empty((n, capi.SNAP_FLOATS), device=dev)
            d_rec = torch.full((n, capi.CHUNK_REC_FLOATS), 7.0, device=dev)
            b.save_streams_device(d_snap.data_ptr(), d_list.data_ptr(), n, st)
            b.save_chunk_fifos_device(d_rec.data_ptr(), d_list.data_ptr(), n, st)
            torch.cuda.synchronize()
            want_rec = torch.from_numpy(stream_mix.chunk_records(exp, M, q)).to(dev)[torch.from_numpy(order % B).to(dev)]
            ne = (d_rec.view(torch.int32) != want_rec).any(1)
            if bool(ne.any().item()):
                w = ne.nonzero()[:5, 0].tolist()
                raise AssertionError(f"the move before push {q}: the FIFO records of {int(ne.sum())} of {n} streams differ from the CPU's, first "
                                     f"(stream, block position, fill) {[(int(order[i]), int(order[i]) % B, int(s['fill'][q, order[i] % B])) for i in w]}")
            at = np.empty(n, np.int64)
            at[order] = np.arange(n)                                          # (where the list holds stream i)
            got = d_snap[torch.from_numpy(at[one_each]).to(dev), :capi.STATE_FLOATS].cpu().numpy()
            bad = np.flatnonzero((got.view(np.uint32) != exp["move_state"][one_each % B].view(np.uint32)).any(1))
            assert not len(bad), (f"the move before push {q}: the snapshots of {len(bad)} of {len(one_each)} block positions differ from the "
                                  f"oracle's state after their completed frames, first (stream, frames) "
                                  f"{[(int(one_each[i]), int(s['done'][q, one_each[i] % B])) for i in bad[:5]]}")
            fresh = batch()
            fresh.load_streams_device(d_snap.data_ptr(), d_list.data_ptr(), n, st)
            fresh.load_chunk_fifos_device(d_rec.data_ptr(), d_list.data_ptr(), n, st)
            torch.cuda.synchronize()
            b.close()
            b = fresh
            d_again = torch.full((n, capi.CHUNK_REC_FLOATS), 9.0, device=dev)
            b.save_chunk_fifos_device(d_again.data_ptr(), d_list.data_ptr(), n, st)
            torch.cuda.synchronize()
            assert torch.equal(d_again.view(torch.int32), d_rec.view(torch.int32)), "the destination's FIFO records, saved again, differ"
            assert_bits_equal(b.chunk_fill(), s["fill"][q][idx].astype(np.int32), "chunk_fill of the destination batch")
            del d_snap, d_rec, d_again, want_rec
        plan = stream_mix.chunk_push_plan(n, q, M)
        mc, F, R = int(s["max_count"][q]), int(s["F"][q]), len(plan["src"])
        src = torch.from_numpy(plan["src"]).to(dev)
        named = torch.from_numpy(plan["named"]).to(dev)
        cnt = torch.from_numpy(np.ascontiguousarray(plan["counts"], np.int32)).to(dev)
        at = cum[q][src][:, None] + torch.arange(mc, device=dev)[None]        # (R, mc): where the row's samples stand in x and y
        own = torch.arange(mc, device=dev)[None] < cnt[:, None]
        size = R * mc + PAD
        d_in = torch.full((size,), junk, dtype=el, device=dev)
        d_exp = torch.full((size,), sentinel, dtype=el, device=dev)
        d_in[:R * mc] = torch.where(own, x[src[:, None], at], junk).reshape(-1)
        d_exp[:R * mc] = torch.where(own & named[:, None], y[src[:, None], at], sentinel).reshape(-1)
        del at, own
        d_in0 = d_in.clone()
        d_out = torch.full((size,), sentinel, dtype=el, device=dev)
        vad = torch.full((F, R), SENTINEL_AUX, dtype=torch.int32, device=dev)
        gains = torch.full((F, R, 32), SENTINEL_AUX, dtype=torch.int32, device=dev)
        frames = torch.full((R,), SENTINEL_AUX, dtype=torch.int32, device=dev)
        if plan["rows"] is None:
            b.process_chunks_device(d_out.data_ptr(), d_in.data_ptr(), cnt.data_ptr(), mc, vad.data_ptr(), gains.data_ptr(),
                                    frames.data_ptr(), st, s16=s16)
        else:
            rows = torch.from_numpy(plan["rows"]).to(dev)
            b.process_chunks_list_device(d_out.data_ptr(), d_in.data_ptr(), cnt.data_ptr(), mc, rows.data_ptr(), R, vad.data_ptr(),
                                         gains.data_ptr(), frames.data_ptr(), st, s16=s16)
        torch.cuda.synchronize()
        what = f"push {q} ({push['form']}, max_count {mc}, F {F}, {R} rows)"
        k = torch.where(named, k_all[q][src], 0)

        def where_rows(ne):
            w = ne.nonzero()[:5, 0].tolist()
            return (f"first (push, row) {[(q, i) for i in w]}: list entry {[None if plan['rows'] is None else int(plan['rows'][i]) for i in w]}, "
                    f"block position {[int(plan['src'][i]) for i in w]}, count {[int(plan['counts'][i]) for i in w]}, fill before "
                    f"{[int(s['fill'][q, plan['src'][i]]) if plan['named'][i] else None for i in w]}, k {[int(k[i]) for i in w]}")

        if not torch.equal(d_out, d_exp):
            ne = (d_out[:R * mc].reshape(R, mc) != d_exp[:R * mc].reshape(R, mc)).any(1)
            raise AssertionError(f"{what}: out differs in {int((d_out != d_exp).sum())} of {size} samples, the first at sample "
                                 f"{int((d_out != d_exp).nonzero()[0])}; {int(ne.sum())} of {R} rows, " + where_rows(ne))
        assert torch.equal(d_in, d_in0), f"{what}: `in` was written"
        ne = frames != k
        if bool(ne.any().item()):
            raise AssertionError(f"{what}: frames of {int(ne.sum())} of {R} rows differ, " + where_rows(ne))
        j = torch.arange(F, device=dev)[:, None]
        live = j < k[None]                                                    # (F, R)
        fr = done[q][src][None] + j
        for name, got, ref in (("vad", vad, ref_vad), ("gains", gains, ref_gains)):
            r = ref[src[None].expand(F, R), fr].reshape(F, R, -1)
            r = torch.where(live[..., None], r, 0)
            ne = (got.reshape(F, R, -1) != r).any(-1).any(0)
            if bool(ne.any().item()):
                raise AssertionError(f"{what}: {name} of {int(ne.sum())} of {R} rows differs, " + where_rows(ne))
        del d_in, d_in0, d_out, d_exp, vad, gains, frames
        fill = b.chunk_fill()
        bad = np.flatnonzero(fill != s["fill_after"][q][idx])
        if len(bad):
            raise AssertionError(f"{what}: chunk_fill of {len(bad)} of {n} streams differs, first (stream, block position, listed, got, expected) "
                                 f"{[(int(i), int(i) % B, bool(s['listed'][q, i % B]), int(fill[i]), int(s['fill_after'][q, i % B])) for i in bad[:5]]}")
    del x, y, ref_vad, ref_gains
    assert not b.chunk_fill().any()
    # every block position from a different copy, the last copy of every reset position, every copy of the position no list push lists
    streams = np.unique(np.concatenate([one_each, [p + (n - 1 - p) // B * B for p in stream_mix.RESET if p < n],
                                        np.arange(stream_mix.SPECIAL["never"], n, B)]))
    for s_ in streams:
        assert_bits_equal(b.export_state(int(s_)), exp["state"][s_ % B], f"state of stream {s_} (block stream {s_ % B})")
    b.close()
    m.close()


# ---- the block under linked gains (stream_mix.LINK_CASES): controls, two model slots, group-wise list calls ----
_LINK_MIX = {}
_LINK_IDS = [f"n{n}-path{p}-k{K}" for n, p, K in stream_mix.LINK_CASES]


def _link_mix(blobs, K, profile, scheduled):
    """the block and the link oracle's run of the groups that occur for K -- lock-step, or under stream_mix's linked presence schedule
    and resets --, once per module, K and rcpps profile"""
    key = (K, profile, scheduled)
    if key not in _LINK_MIX:
        pcm, _ = stream_mix.block()
        kw = dict(presence=stream_mix.link_presence(K), resets=stream_mix.RESET) if scheduled else {}
        _LINK_MIX[key] = pcm, stream_mix.oracle_groups(blobs, pcm, K, stream_mix.controls(), stream_mix.slots(),
                                                       groups=stream_mix.link_groups(K), **kw)
    return _LINK_MIX[key]


def _linked_batch(blobs, n, path, K):
    """a batch of n copies of the block with the link dressing set before its first call: network path, slot 1 = the sparser model and
    the slot map, the control table, link count K"""
    idx = np.arange(n) % stream_mix.B
    models = [capi.Model(blob) for blob in blobs]
    b = capi.Batch(models[0], n)
    if path is not None:
        b.set_nn_path(path)
    assert b.add_model(models[1]) == 1
    b.set_stream_models(stream_mix.slots()[idx])
    b.set_stream_controls(stream_mix.controls()[idx])
    assert b.set_gain_link(K) == 1 and b.gain_link == K
    return b, models


def _device_refs(torch, want, dev):
    """out, vad and gains of oracle_groups as int32 bit patterns on the device, (T, B * K, width): row g0 * K + member"""
    T = want["vad"].shape[0]
    return {k: torch.from_numpy(np.ascontiguousarray(want[k], np.float32)).to(dev).reshape(T, -1, w).view(torch.int32)
            for k, w in (("out", 480), ("vad", 1), ("gains", 32))}


def _check_last_frame(b, want, frame, streams, gm, what):
    """debug_last's features, silence and pitch of `streams` against frame `frame` of oracle_groups' rows gm"""
    for name, got in zip(("features", "silence", "pitch"), b.debug_last()):
        ref = want[name][frame]
        assert_bits_equal(got[streams], ref.reshape((-1,) + ref.shape[2:])[gm].astype(got.dtype), f"{what}: {name} of frame {frame}")


def _check_linked_states(b, want, n, K):
    """save_streams of one copy per (g0, member), each from a different copy: the complete state, and the gate counter"""
    streams, gm = stream_mix.link_state_streams(n, K)
    snap = b.save_streams(streams)
    where = [(int(s_), int(x) // K, int(x) % K) for s_, x in zip(streams, gm)]
    state = want["state"].reshape(-1, capi.STATE_FLOATS)[gm]
    bad = np.flatnonzero((snap[:, :capi.STATE_FLOATS].view(np.uint32) != state.view(np.uint32)).any(1))
    assert not len(bad), f"state of {len(bad)} of {len(streams)} streams differs, first (stream, g0, member) {[where[i] for i in bad[:5]]}"
    gate = np.ascontiguousarray(snap[:, capi.SNAP_OFF_GATE]).view(np.int32)
    bad = np.flatnonzero(gate != want["gate"].reshape(-1)[gm])
    assert not len(bad), (f"gate counter of {len(bad)} of {len(streams)} streams differs, first (stream, g0, member) "
                          f"{[where[i] for i in bad[:5]]}: {gate[bad[:5]].tolist()} for {want['gate'].reshape(-1)[gm][bad[:5]].tolist()}")


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path,K", stream_mix.LINK_CASES, ids=_LINK_IDS)
def test_stream_mix_linked_at_every_form(blob_default, blob_little, rcp_profile, n, path, K):
    """Linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link) at every kernel form: n copies of the mixed block with link
    count K, stream_mix.controls() and slots() on its positions, in lock-step calls of stream_mix.CALLS on the default schedule.  The
    linked branch of the synthesis kernel reads its siblings' silence word, VAD and gains, which K1 and the network launch(es) of the
    same frame wrote: with the network paths of LINK_CASES every form of every stage writes them (tests/test_stream_mix_cpu.py), one
    launch per model slot, under the three-stream pipeline.  Every stream's pcm, vad and gains against the link oracle's run of its
    group (one per g0, stream_mix.oracle_groups) bit for bit, on the device; after every call debug_last; at the end the complete
    state and the gate counter of one copy per (g0, member)."""
    import torch
    _need_256_cus()
    blobs = (blob_default, blob_little)
    pcm, want = _link_mix(blobs, K, rcp_profile, False)
    T, B = sum(stream_mix.CALLS), stream_mix.B
    dev = torch.device("cuda", 0)
    gm_h = stream_mix.link_index(n, K)
    gm = torch.from_numpy(gm_h).to(dev)
    d_in = torch.from_numpy(pcm[:T]).to(dev)[:, torch.arange(n, device=dev) % B].contiguous()
    d_out = torch.empty_like(d_in)
    d_vad = torch.empty((T, n), device=dev)
    d_gains = torch.empty((T, n, 32), device=dev)
    b, models = _linked_batch(blobs, n, path, K)
    st = torch.cuda.current_stream().cuda_stream
    f = 0
    for c in stream_mix.CALLS:
        b.process_device(d_out[f].data_ptr(), d_in[f].data_ptr(), d_vad[f].data_ptr(), d_gains[f].data_ptr(), c, st)
        f += c
        torch.cuda.synchronize()
        _check_last_frame(b, want, f - 1, np.arange(n), gm_h, f"the {c}-frame call")
    ref = _device_refs(torch, want, dev)
    for name, t, w in (("out", d_out, 480), ("vad", d_vad, 1), ("gains", d_gains, 32)):
        ne = (t.reshape(T, n, w).view(torch.int32) != ref[name][:T][:, gm]).any(-1)
        if bool(ne.any().item()):
            where = ne.nonzero()[:5].tolist()
            raise AssertionError(f"{name}: {int(ne.sum().item())} of {T * n} stream-frames differ from the link oracle, first (frame, "
                                 f"stream) {where}, (g0, member) {[(int(gm_h[s_]) // K, s_ % K) for _, s_ in where]}")
        del ne
    del d_in, d_out, d_vad, d_gains, ref
    _check_linked_states(b, want, n, K)
    b.close()
    for m in models:
        m.close()


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path,K", stream_mix.LINK_CASES, ids=_LINK_IDS)
def test_stream_mix_linked_masked_and_listed_at_every_form(blob_default, blob_little, rcp_profile, n, path, K):
    """The same batches through the serving API: stream_mix.KINDS with the linked presence schedule (link_presence: masks by position,
    list calls that list whole groups by g0 in a pseudo-random group order, three entries that name no stream in place of a first, a
    middle and a last member, a hand-made group whose only present row is silent) and a reset of RESET's copies before call
    RESET_BEFORE.  In per-stream frame phase an absent sibling's words of an earlier frame must not be folded, in a list call the
    siblings are found through the list, and every slot's network launch stores only its own rows of the scratch planes.  NaN in
    every absent input row, the sentinels of test_stream_mix_masked_and_listed_at_every_form: every present row-frame matches the
    link oracle bit for bit in pcm, vad and gains, every absent row -- the replaced entries' among them -- keeps out's sentinel and
    reads vad 0 and 32 zero gains.  After every call debug_last's defined entries; at the end the complete state and the gate counter
    of one copy per (g0, member), and the copies of the position absent from every masked and list frame as the last lock-step call
    left them."""
    import torch
    _need_256_cus()
    blobs = (blob_default, blob_little)
    pcm, want = _link_mix(blobs, K, rcp_profile, True)
    B = stream_mix.B
    idx = np.arange(n) % B
    dev = torch.device("cuda", 0)
    blk = torch.from_numpy(pcm).to(dev)
    ref = _device_refs(torch, want, dev)
    b, models = _linked_batch(blobs, n, path, K)
    st = torch.cuda.current_stream().cuda_stream
    never = np.flatnonzero(idx == stream_mix.SPECIAL["never"])
    never_snap = None
    for c, kind in enumerate(stream_mix.KINDS):
        plan = stream_mix.link_call_plan(n, K, c)
        fr = plan["frames"]
        k, R = len(fr), len(plan["src"])
        src = torch.from_numpy(plan["src"]).to(dev)
        gm = torch.from_numpy(plan["gm"]).to(dev)
        present = torch.from_numpy(plan["present"]).to(dev)
        x = stream_mix.call_input(blk, fr, src, present).contiguous()
        out = torch.empty_like(x)
        out.view(torch.int32).fill_(SENTINEL_OUT)
        vad = torch.empty((k, R), device=dev)
        gains = torch.empty((k, R, 32), device=dev)
        vad.view(torch.int32).fill_(SENTINEL_AUX)
        gains.view(torch.int32).fill_(SENTINEL_AUX)
        ptrs = (out.data_ptr(), x.data_ptr(), vad.data_ptr(), gains.data_ptr())
        if kind == "lock":
            b.process_device(*ptrs, k, st)
        else:
            act = torch.from_numpy(plan["active"]).to(dev).contiguous()
            if kind == "masked":
                b.process_masked_device(*ptrs, act.data_ptr(), k, st)
            else:
                rows = torch.from_numpy(plan["rows"]).to(dev)
                b.process_list_device(*ptrs, rows.data_ptr(), R, act.data_ptr(), k, st)
        torch.cuda.synchronize()
        what = f"call {c} ({kind}, frames {fr.start}..{fr.stop - 1})"
        for name, got, w in (("out", out, 480), ("vad", vad, 1), ("gains", gains, 32)):
            r = torch.where(present[..., None], ref[name][fr.start:fr.stop][:, gm], SENTINEL_OUT if name == "out" else 0)
            ne = (got.view(torch.int32).reshape(k, R, w) != r).any(-1)
            if bool(ne.any().item()):
                where = ne.nonzero()[:5].tolist()
                raise AssertionError(f"{what}: {name} of {int(ne.sum().item())} of {k * R} row-frames differs, first (frame, row) "
                                     f"{where}: present {[bool(plan['present'][f, i]) for f, i in where]}, list entry "
                                     f"{[None if plan['rows'] is None else int(plan['rows'][i]) for _, i in where]}, (g0, member) "
                                     f"{[(int(plan['gm'][i]) // K, int(plan['gm'][i]) % K) for _, i in where]}")
            del r, ne
        del x, out, vad, gains
        # debug_last: every stream after a masked or lock-step call (silence 2 where absent), the listed streams after a list call
        named = np.ones(R, bool) if plan["rows"] is None else (plan["rows"] >= 0) & (plan["rows"] < n)
        streams = np.arange(n) if plan["rows"] is None else plan["rows"][named]
        here = plan["present"][-1][named]
        assert (b.debug_last()[1][streams[~here]] == 2).all(), f"{what}: silence of streams absent from frame {fr.stop - 1}"
        _check_last_frame(b, want, fr.stop - 1, streams[here], plan["gm"][named][here], what)
        if c + 1 == stream_mix.RESET_BEFORE:
            b.reset_streams(np.flatnonzero(np.isin(idx, stream_mix.RESET)))
        if kind == "lock":
            never_snap = b.save_streams(never)
    torch.cuda.synchronize()
    del blk, ref
    _check_linked_states(b, want, n, K)
    assert_bits_equal(b.save_streams(never), never_snap, "the streams absent from every frame since the last lock-step call")
    b.close()
    for m in models:
        m.close()


def _poison_places(n, B):
    """a block stream p and three of its copies: the first lane of an analysis quad, the last lane of a 64-stream wave (high-pass lanes,
    GRU group) and the middle of a 16-stream tile"""
    for p in range(B):
        copies = [p + c * B for c in range((n - p + B - 1) // B)]
        quad = [s for s in copies if s % 4 == 0]
        wave = [s for s in copies if s % 64 == 63 and s + 1 <= n - n % 64]
        tile = [s for s in copies if s % 16 in (7, 8) and s not in wave]
        if quad and wave and tile and len({quad[0], wave[0], tile[0]}) == 3:
            return p, (quad[0], wave[0], tile[0])
    raise AssertionError(f"no block stream has copies at all three places in {n} streams")


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n", [3001, 40037])
def test_poisoned_stream_in_every_at_size_unit(blob_default, rcp_profile, n):
    """NaN, +Inf and -Inf samples in three copies of one stream of the mixed block, placed at the first lane of a four-stream analysis
    workgroup, the last lane of a lane-per-stream high-pass wave and of a 64-stream GRU group, and the middle of a tile (rn_hp_kernel,
    rn_analysis_kernel, the tile kernels at 3,001 streams; the layer-wise network with rn_nn_gru_kernel at 40,037): every other stream
    still gets the oracle's bits"""
    _need_256_cus()
    pcm, want = _mix(blob_default, rcp_profile)
    B, calls = pcm.shape[1], stream_mix.CALLS
    p, places = _poison_places(n, B)
    poisoned = []
    for s in places:
        poisoned += [(2, s, 100, np.nan), (9, s, 7, np.inf), (16, s, 300, -np.inf), (23, s, 479, np.nan)]
    others = [s for s in range(n - 1, n - 1 - 3 * B, -7) if s not in places] + [places[0] + 1, places[1] - 1, places[2] + 1]
    _ragged_check(blob_default, n, calls, pcm, want=want, nn_path=None, state_streams=others, every_call=True,
                  poisoned=poisoned, ragged=False)


# ---- the block through the feature calls (stream_mix.FEATURE_CASES): the network alone on records, scored with the trainer's loss ----
_FEATURES = {}


def _feature_mix(blob, profile, little=None):
    """the records of the feature dressing, their compute_rnn-only expectation on the CPU (with `little`: under the two-model map of
    stream_mix.feature_slots()) and the canonical sums -- one 30-frame call of a B-stream batch on path 0 --, once per module, rcpps
    profile and model set; "worst": the largest relative difference of a position's canonical {gain, VAD} sums from the float64
    restatement (tests/eval_cases.py) over the expectation"""
    key = (profile, little is not None)
    if key not in _FEATURES:
        import eval_cases as ec
        import torch
        B, T = stream_mix.B, stream_mix.T
        rec = stream_mix.feature_records(_mix(blob, profile)[1])
        exp = stream_mix.feature_expectation(blob, rec, slot_blobs=None if little is None else (blob, little))
        dev = torch.device("cuda", 0)
        b, models = _feature_batch(blob, B, 0, little)
        d_rec = torch.from_numpy(rec).to(dev)
        d_sums = torch.zeros((B, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
        st = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        b.eval_records_device(d_sums.data_ptr(), 0, 0, d_rec.data_ptr(), 0, T, stream=st.cuda_stream)
        st.synchronize()
        canon = d_sums.cpu().numpy()
        b.close()
        for m in models:
            m.close()
        worst = [max(ec.rel_diff(canon[p, k], exp["sums"][p, k]) for p in range(B)) for k in (0, 1)]
        print(f"\n[feature calls] largest relative difference of a block position's sums against the float64 restatement: gain {worst[0]:.3e}, "
              f"vad {worst[1]:.3e} ({B} positions, {ec.frames_scored(0, T)} scored frames, {'two models' if little is not None else 'one model'})")
        _FEATURES[key] = dict(rec=rec, exp=exp, canon=canon, worst=worst)
    return _FEATURES[key]


def _feature_batch(blob, n, path, little=None):
    """a batch of n copies of the block for the feature calls: network path, and with `little` slot 1 = the sparser model under the map
    of stream_mix.feature_slots() by position"""
    models = [capi.Model(x) for x in ((blob,) if little is None else (blob, little))]
    b = capi.Batch(models[0], n)
    if path is not None:
        b.set_nn_path(path)
    if little is not None:
        assert b.add_model(models[1]) == 1
        b.set_stream_models(stream_mix.feature_slots()[np.arange(n) % stream_mix.B])
    return b, models


def _feature_rows(torch, r, layout):
    """r (T, n, w) on the device as the rows of a feature call under `layout` (stream_mix.FEATURE_LAYOUTS): (buffer, frame_stride,
    row_stride).  "frame": [T + 1][n][w] with the default strides; "stream": [n][T + 1][w], one sequence after the other; "pitch100":
    [T + 1][n][w + 2].  Record T -- behind every sequence's last record -- and the pad floats are NaN: nothing of them may reach a result"""
    T, n, w = r.shape
    if layout == "stream":
        buf = torch.full((n, T + 1, w), float("nan"), dtype=torch.float32, device=r.device)
        buf[:, :T] = r.transpose(0, 1)
        return buf, w, (T + 1) * w
    pitch = w + 2 if layout == "pitch100" else w
    buf = torch.full((T + 1, n, pitch), float("nan"), dtype=torch.float32, device=r.device)
    buf[:T, :, :w] = r
    return (buf, 0, 0) if layout == "frame" else (buf, n * pitch, pitch)


def _feature_differs(name, got, ref, idx, live, B, whole=True):
    """got (T, n, w) against ref (T, B, w) by block position, both int32 bit patterns on the device, on the streams `live` marks;
    whole: also the copies among themselves and the ragged tail against the head of copy 0"""
    T, n, w = got.shape
    q, r = n // B, n % B
    if whole:
        copies = got[:, :B * q].reshape(T, q, B * w)
        assert bool((copies == copies[:, :1]).all().item()), f"replicated streams diverged ({name})"
        assert bool((got[:, B * q:] == got[:, :r]).all().item()), f"the ragged tail differs from the head of copy 0 ({name})"
    ne = (got != ref[:, idx]).any(-1) & live
    if bool(ne.any().item()):
        where = ne.nonzero()[:5].tolist()
        raise AssertionError(f"{name}: {int(ne.sum().item())} of {T * int(live.sum().item())} stream-frames differ from the oracle's compute_rnn, "
                             f"first (frame, stream) {where}, block positions {[s_ % B for _, s_ in where]}")


def _poison_feature_rows(r, n, B):
    """NaN, +Inf and -Inf into the features, and one NaN into a target, of the copies _poison_places names -> those streams"""
    _, places = _poison_places(n, B)
    for s in places:
        r[2, s, 5] = float("nan")
        r[9, s, 40] = float("inf")
        r[16:, s, 0:65:7] = float("-inf")
        r[23, s, 64] = float("nan")
        r[6, s, 70] = float("nan")                            # a target, too
    return places


def _feature_run(blob, profile, n, path, layout, little=None, poisoned=False):
    """One batch of n copies of the block through the feature calls, device forms on a stream of the test's own.  eval_records_device
    in the cuts of stream_mix.FEATURE_CALLS on records under `layout`: gains and VAD of every stream-frame against the expectation bit
    for bit (the copies among themselves, the ragged tail against the head of copy 0), the frame behind the call's last keeps its
    sentinel, every stream's sums the same doubles as its position's canonical sums, frames scored exact.  Not poisoned: the exported
    state of every block position, each from a different copy, against the oracle's after its compute_rnn-only walk; then, after
    reset(), process_features_device in ONE 30-frame call on rows 65 floats apart gives the same bits again.  Poisoned: the copies
    _poison_places names carry NaN / Inf and are left out of every comparison"""
    import eval_cases as ec
    import torch
    mix = _feature_mix(blob, profile, little)
    exp, canon = mix["exp"], mix["canon"]
    T, B = stream_mix.T, stream_mix.B
    dev = torch.device("cuda", 0)
    idx = torch.arange(n, device=dev) % B
    r = torch.from_numpy(mix["rec"]).to(dev)[:, idx].contiguous()                 # (T, n, 98)
    live_h = np.ones(n, bool)
    if poisoned:
        live_h[list(_poison_feature_rows(r, n, B))] = False
    live = torch.from_numpy(live_h).to(dev)
    buf, fs, rs = _feature_rows(torch, r, layout)
    ref = {k: torch.from_numpy(np.ascontiguousarray(exp[k], np.float32)).to(dev).reshape(T, B, w).view(torch.int32)
           for k, w in (("gains", 32), ("vad", 1))}

    def outputs():
        return (torch.full((T + 1, n, 32), SENTINEL_AUX, dtype=torch.int32, device=dev),
                torch.full((T + 1, n), SENTINEL_AUX, dtype=torch.int32, device=dev))

    def check(gains, vad, what):
        assert bool((gains[T] == SENTINEL_AUX).all().item()) and bool((vad[T] == SENTINEL_AUX).all().item()), f"{what} wrote behind its last frame"
        _feature_differs(f"{what}: gains", gains[:T], ref["gains"], idx, live, B, whole=not poisoned)
        _feature_differs(f"{what}: vad", vad[:T].reshape(T, n, 1), ref["vad"], idx, live, B, whole=not poisoned)

    gains, vad = outputs()
    d_sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
    b, models = _feature_batch(blob, n, path, little)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    t = 0
    for k in stream_mix.FEATURE_CALLS:
        b.eval_records_device(d_sums.data_ptr(), gains.data_ptr() + t * n * 32 * 4, vad.data_ptr() + t * n * 4, buf.data_ptr(), t, k,
                              frame_stride=fs, row_stride=rs, stream=st.cuda_stream)
        t += k
    st.synchronize()
    assert t == T
    check(gains, vad, f"eval_records_device in calls of {stream_mix.FEATURE_CALLS}, layout {layout}")
    # the sums: the same doubles as the position's canonical sums
    d_canon = torch.from_numpy(canon).to(dev).view(torch.int64)[idx]
    ne = (d_sums.view(torch.int64) != d_canon).any(-1) & live
    if bool(ne.any().item()):
        where = ne.nonzero()[:5, 0].tolist()
        raise AssertionError(f"sums: {int(ne.sum().item())} of {int(live.sum().item())} streams differ from their position's canonical sums, first "
                             f"streams {where}, block positions {[s_ % B for s_ in where]}: {d_sums[where].tolist()} for {canon[[s_ % B for s_ in where]].tolist()}")
    assert bool(((d_sums[:, 2] == ec.frames_scored(0, T)) & (d_sums[:, 3] == 0))[live].all().item()), "frames scored"
    del buf, d_canon
    if not poisoned:
        # block position p from copy (7 p) mod (the copies holding p): nothing but the network state has moved
        for s_ in [p + (7 * p) % ((n - p + B - 1) // B) * B for p in range(min(B, n))]:
            assert_bits_equal(b.export_state(s_), exp["state"][s_ % B], f"state of stream {s_} (block position {s_ % B})")
        feats, _, _ = _feature_rows(torch, r[:, :, :65], "frame")
        gains2, vad2 = outputs()
        torch.cuda.synchronize()
        b.reset()
        b.process_features_device(gains2.data_ptr(), vad2.data_ptr(), feats.data_ptr(), T, stream=st.cuda_stream)
        st.synchronize()
        check(gains2, vad2, "process_features_device in one call after a reset")
        assert torch.equal(gains2, gains) and torch.equal(vad2, vad), "one 30-frame call after a reset against the seven eval calls"
    b.close()
    for m in models:
        m.close()
    return mix


def _assert_canonical_sums(mix):
    import eval_cases as ec
    canon, want = mix["canon"], mix["exp"]["sums"]
    assert (canon[:, 2] == ec.frames_scored(0, stream_mix.T)).all() and (canon[:, 3] == 0).all() and np.isfinite(canon).all()
    assert (want[:, 0] > 0).sum() > 300 and (want[:, 1] > 0).sum() > 150                    # (the sums are about something)
    for p in range(stream_mix.B):
        for k, name in ((0, "gain"), (1, "vad")):
            assert ec.rel_diff(canon[p, k], want[p, k]) <= 1e-10, (p, name, canon[p, k], want[p, k])


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path", stream_mix.FEATURE_CASES, ids=stream_mix.FEATURE_IDS)
def test_stream_mix_feature_calls_at_every_form(blob_default, rcp_profile, n, path):
    """The mixed block through the feature calls (include/rnnoise_amd.h: rnnoise_batch_eval_records_device,
    rnnoise_batch_process_features_device) at every form a feature call can take (tests/test_stream_mix_cpu.py): n copies of the
    records of stream_mix.feature_records() -- every position's 65 features of the lock-step oracle run, all exactly zero on its 304
    silent stream-frames at and across the call boundaries, beside live rows in the same tile and group, with targets of every kind
    the trainer's loss tells apart -- walked in the cuts of FEATURE_CALLS, the cases cycling through the three layouts.  The
    expectation is the oracle's compute_rnn alone, every frame, one walk per position (stream_mix.feature_expectation): a call that
    skipped the network on a zero row, as rnnoise_batch_process does, fails on 20 of the 22 partly silent positions.  See
    _feature_run for what is compared.  The canonical sums against the float64 restatement of the trainer's loss: relative difference
    at most 1e-10 -- a float32 step anywhere would show at 1e-8.
    Measured on MI355X: largest relative difference over the 389 positions 4.5e-16 (gain sums) and 1.5e-16 (VAD sums); with the
    sparser model on a third of the positions (the two-model test) 4.3e-16 and 1.5e-16.
    The block's counts behind this, recomputed in tests/test_stream_mix_cpu.py: 304 zero-feature stream-frames on 29 positions, 7 of
    them silent throughout and 22 partly, 9 to 20 positions in the first and the last frame of every call, 360 positions never
    silent; in a 4,099-stream batch 241 of the 256 whole tiles hold a zero row beside a live one in some frame."""
    _need_256_cus()
    layout = stream_mix.FEATURE_LAYOUTS[stream_mix.FEATURE_CASES.index((n, path)) % len(stream_mix.FEATURE_LAYOUTS)]
    _assert_canonical_sums(_feature_run(blob_default, rcp_profile, n, path, layout))


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path", [(4099, 1), (40037, None)], ids=["n4099-path1", "n40037-pathNone"])
def test_stream_mix_feature_calls_with_two_models(blob_default, blob_little, rcp_profile, n, path):
    """The same walk with the sparser model as slot 1 under the map of stream_mix.feature_slots(): the slots alternate within every
    tile and group, and one launch (layer-wise: one whole network) per slot owns its rows.  At 40,037 streams a slot's whole
    layer-wise network runs before the next slot's front inside a feature call with more groups than CUs; at 4,099 on path 1 the
    eight-wave tile kernel runs once per slot.  Predictions, sums and states against the two-model expectation"""
    _need_256_cus()
    layout = "stream" if n == 4099 else "pitch100"
    mix = _feature_run(blob_default, rcp_profile, n, path, layout, little=blob_little)
    _assert_canonical_sums(mix)
    one = _feature_mix(blob_default, rcp_profile)
    on = stream_mix.feature_slots() == 1
    assert (mix["canon"][~on] == one["canon"][~on]).all() and (mix["canon"][on, 0] != one["canon"][on, 0]).mean() > 0.8


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path", [(4099, 1), (40037, None)], ids=["n4099-path1", "n40037-pathNone"])
def test_feature_calls_keep_poisoned_streams_alone_at_size(blob_default, rcp_profile, n, path):
    """NaN, +Inf and -Inf in features, and a NaN in a target, of three copies of one block position -- the first lane of a quad, the
    last lane of a 64-stream GRU group and the middle of a tile (_poison_places) --: every other stream's predictions and sums are bit
    for bit what they are without the poison, on the eight-wave tile kernel and on the layer-wise network with rn_nn_gru_kernel"""
    _need_256_cus()
    _feature_run(blob_default, rcp_profile, n, path, "frame", poisoned=True)


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n,path", [(389, 1), (10277, None)], ids=["n389-path1", "n10277-pathNone"])
def test_feature_calls_report_their_network_time(blob_default, rcp_profile, n, path):
    """rnnoise_batch_kernel_ms after a 5-frame eval call with timing on: 5 launches and a positive ms[1] -- through the one-launch
    branch of the network step (the tile kernel) and the five-launch one (the layer-wise network) --, and ms[0], ms[2], ms[3] what a
    batch that ran no PCM call reports; the timed call's predictions are the expectation's all the same"""
    import torch
    _need_256_cus()
    mix = _feature_mix(blob_default, rcp_profile)
    B, k = stream_mix.B, 5
    dev = torch.device("cuda", 0)
    idx = torch.arange(n, device=dev) % B
    buf, fs, rs = _feature_rows(torch, torch.from_numpy(mix["rec"][:k]).to(dev)[:, idx].contiguous(), "frame")
    gains = torch.full((k + 1, n, 32), SENTINEL_AUX, dtype=torch.int32, device=dev)
    d_sums = torch.zeros((n, capi.EVAL_SUMS), dtype=torch.float64, device=dev)
    b, models = _feature_batch(blob_default, n, path)
    b.enable_timing()
    idle = b.kernel_ms()
    assert idle["launches"] == 0
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    b.eval_records_device(d_sums.data_ptr(), gains.data_ptr(), 0, buf.data_ptr(), 0, k, frame_stride=fs, row_stride=rs, stream=st.cuda_stream)
    st.synchronize()
    ms = b.kernel_ms()
    assert ms["launches"] == k and ms["network"] > 0, ms
    assert all(ms[key] == idle[key] for key in ("analysis", "synthesis", "highpass")), (ms, idle)
    assert b.kernel_ms()["launches"] == 0
    ref = torch.from_numpy(mix["exp"]["gains"][:k]).to(dev).view(torch.int32)
    _feature_differs("gains of the timed call", gains[:k], ref, idx, torch.ones(n, dtype=torch.bool, device=dev), B)
    assert bool((gains[k] == SENTINEL_AUX).all().item())
    b.close()
    for m in models:
        m.close()


@pytest.mark.rcp("host")
@pytest.mark.parametrize("n", [8192, 10208])
def test_the_tile_network_at_its_largest_batches(blob_default, n):
    _tiled_check(blob_default, n, (3, 1, 2), silent_stream=9)


@pytest.mark.rcp("host")
def test_16384_streams_on_the_host_profile(blob_default):
    """the largest batch on the eight-wave layer kernel (one 64-stream group per CU), on the profile a deployed process gets by
    default (this CPU's rcpps)"""
    _tiled_check(blob_default, 16384, (3, 4), silent_stream=5)


def _soak(blob, N, reps, cycles):
    """The pipelined schedule for a long time: `reps` runs from reset of `cycles` x 24 frames each, as calls of 8 + 5 + 1 + 8 + 2
    frames over a 24-frame input that repeats (what fits in HBM at 65,536 streams), N/32 replicas of a 32-stream block.  After
    EVERY call every replica's pcm / gains / vad is compared with replica 0 on the GPU; replica 0's block is collected and, at the
    end of a run, compared frame by frame with one oracle run of the whole sequence, as is the state of streams from three
    places of the batch.  This is the test that would have seen round 4's "one run in ten" corruption in the product's own
    configuration (profiles/r5_gru_race.txt): a wrong bit anywhere in ~10^8 stream-frames fails it."""
    import torch
    calls, P = (8, 5, 1, 8, 2), 24
    T = cycles * P
    base = synth.batch_pcm(range(32), P)
    base[:3, 9] = 0                                   # a stream that is silent whenever the input wraps ...
    base[P - 5:P - 3, 12] = 0                         # ... and one that goes silent inside a call
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(base).to(dev).repeat(1, N // 32, 1).contiguous()
    d_out = torch.empty_like(d_in)
    d_vad = torch.empty((P, N), device=dev)
    d_gains = torch.empty((P, N, 32), device=dev)
    m = capi.Model(blob)
    b = capi.Batch(m, N)
    assert b.set_nn_path(1) == 1
    st = torch.cuda.current_stream().cuda_stream
    want = oracle_run(blob, np.concatenate([base] * cycles))
    for rep in range(reps):
        b.reset()
        got = {"out": [], "gains": [], "vad": []}
        for c in range(cycles):
            f = 0
            for n in calls:
                b.process_device(d_out[f].data_ptr(), d_in[f].data_ptr(), d_vad[f].data_ptr(), d_gains[f].data_ptr(), n, st)
                for name, t, w in (("out", d_out, 480), ("gains", d_gains, 32), ("vad", d_vad, 1)):
                    r = t[f:f + n].view(torch.int32).reshape(n, N // 32, 32 * w)
                    assert bool((r == r[:, :1]).all().item()), f"run {rep}, frames {c * P + f}..{c * P + f + n - 1}: replicas diverged ({name})"
                    got[name].append(t[f:f + n, :32].cpu().numpy())
                f += n
        for name in got:
            assert_bits_equal(np.concatenate(got[name]), want[name], f"run {rep}: {name} of the first block, {T} frames")
        for s_ in (9, 31, (N // 2 // 32) * 32 + 12, N - 32 + 20):
            assert_bits_equal(b.export_state(s_), want["state"][s_ % 32], f"run {rep}: state of stream {s_} after {T} frames")
    b.close()
    m.close()


def test_soak_65536_streams(blob_default):
    """BASELINE configs[2]'s batch for 5 x 312 frames (10^8 stream-frames) on the default three-stream schedule"""
    _soak(blob_default, 65536, reps=5, cycles=13)


def test_soak_sparser_model_32768(blob_little):
    """the sparser blob at 32,768 streams (the configuration in which round 4 saw replicas diverge), 5 x 312 frames"""
    _soak(blob_little, 32768, reps=5, cycles=13)


@pytest.mark.parametrize("variant", [0, 1, 3])
def test_register_fft_bit_exact(variant):
    """F1 in isolation: the register-resident 960-point transform of the analysis / synthesis kernels (fft_reg.h; reference
    rnn_fft_c, src/kiss_fft.c:518-586) against the oracle's FFT on random, impulse, DC, alternating, tiny (denormal products)
    and huge inputs.  variant 0 = every exchange through ds_bpermute, 1 = DPP / swizzle forms, 3 = what the kernels use: as 1 with the
    lane ^ 32 level on v_permlane32_swap."""
    import ctypes as C
    rng = np.random.default_rng(960 + variant)
    cases = [(rng.standard_normal((960, 2)) * 3000).astype(np.float32) for _ in range(6)]
    imp = np.zeros((960, 2), np.float32); imp[0, 0] = 1; cases.append(imp)
    imp2 = np.zeros((960, 2), np.float32); imp2[517, 1] = -32768; cases.append(imp2)
    cases.append(np.full((960, 2), 12345.678, np.float32))                                   # DC
    alt = np.zeros((960, 2), np.float32); alt[::2, 0] = 1; alt[1::2, 0] = -1; cases.append(alt)  # Nyquist
    cases.append((rng.standard_normal((960, 2)) * 1e-38).astype(np.float32))                 # denormal inputs and products
    cases.append((rng.standard_normal((960, 2)) * 1e30).astype(np.float32))                  # no overflow at 1e30 / 960 * 960
    real = (rng.standard_normal((960, 2)) * 8000).astype(np.float32); real[:, 1] = 0; cases.append(real)  # what the kernels feed it
    cases.append(np.zeros((960, 2), np.float32))
    x = np.ascontiguousarray(np.stack(cases))
    y = np.empty_like(x)
    fp = C.POINTER(C.c_float)
    with capi.instrumented() as L:  # the probe kernels live in the instrumented library (include/rnnoise_amd_debug.h)
        rc = L.rnnoise_amd_debug_fft(0, variant, y.ctypes.data_as(fp), x.ctypes.data_as(fp), len(cases), 1, None, None)
    assert rc == 0
    for i, c in enumerate(cases):
        want = Oracle.fft(c.reshape(-1)).reshape(960, 2)
        assert_bits_equal(y[i], want, f"fft case {i} variant {variant}")


def test_log10_device_equals_host_libm_for_every_float():
    """(float)log10(1e-2 + (double)Ex), src/denoise.c:383 -- the one libm call on the path.  The kernels restate the host libm's
    algorithm (rnnoise_amd/csrc/log10_glibc.h); here the DEVICE code is swept against the host libm over every float Ex in
    [0, +Inf] (2,139,095,041 arguments: the device forms them from their bit patterns, the oracle side compares in C on all host
    threads).  Beside it, for the record, how often the device library's own log10 (round 4's implementation) rounds differently."""
    from concurrent.futures import ThreadPoolExecutor
    if not capi.log10_model().endswith("glibc-fma"):
        pytest.skip(f"log10 model {capi.log10_model()}: this host's libm is not the modelled one")
    CH, END = 1 << 26, 0x7f800001
    Oracle.lib()
    n_bad = {0: 0, 1: 0}
    first_bad = {}
    with capi.instrumented() as L, ThreadPoolExecutor(max(2, (os.cpu_count() or 4))) as pool:
        assert capi.log10_model().endswith("glibc-fma")
        for model in (0, 1):
            for lo in range(0, END, CH):
                n = min(CH, END - lo)
                got = np.empty(n, np.float32)
                assert L.rnnoise_amd_debug_log_energy_range(0, capi._fp(got), None, lo, n, model) == 0
                parts = [(lo + o, got[o:o + (1 << 22)]) for o in range(0, n, 1 << 22)]
                for (first, _), (bad, where) in zip(parts, pool.map(lambda p: Oracle.log_energy_range_diff(*p), parts)):
                    n_bad[model] += bad
                    if bad and model not in first_bad:
                        first_bad[model] = where
    print(f"log10, every float Ex in [0, Inf] ({END} arguments): the restated host algorithm differs from the host libm in {n_bad[0]}; "
          f"the device library's log10 in {n_bad[1]}" + (f" (first at Ex bits {first_bad[1]:#x})" if 1 in first_bad else ""))
    assert n_bad[0] == 0, f"{n_bad[0]} results differ, first at Ex bits {first_bad[0]:#x}"


_WORKER = r"""
import sys, lzma, zlib, numpy as np
sys.path.insert(0, {root!r})
from rnnoise_amd import capi, synth
blob = lzma.decompress(open({root!r} + "/tests/golden/default.blob.xz", "rb").read())
ids = list(range({first}, {first} + 48))
pcm = synth.batch_pcm(ids, 10, lead_silence=1)
m = capi.Model(blob); b = capi.Batch(m, 48, device=0); b.set_nn_path(1)
for rep in range(3):
    b.reset()
    out, vad, gains = b.process(pcm)
print("CRC", zlib.crc32(out.tobytes()), zlib.crc32(gains.tobytes()), zlib.crc32(vad.tobytes()), flush=True)
b.close(); m.close()
"""


def test_two_processes_share_one_gpu(blob_default):
    """replica independence: two processes, each with its own capi.Batch on device 0, run concurrently (what N ranks on N
    GPUs do, squeezed onto the one GPU this box has) and both produce the oracle's bits"""
    import zlib
    procs = [subprocess.Popen([sys.executable, "-c", _WORKER.format(root=ROOT, first=f)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for f in (0, 48)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]
    for first, (so, _) in zip((0, 48), outs):
        pcm = synth.batch_pcm(range(first, first + 48), 10, lead_silence=1)
        want = oracle_run(blob_default, pcm, collect_state=False)
        crc = [int(x) for x in so.split("CRC")[1].split()]
        assert crc == [zlib.crc32(want["out"].tobytes()), zlib.crc32(want["gains"].tobytes()),
                       zlib.crc32(want["vad"].tobytes())], f"process starting at stream {first}"


def test_bench_with_two_ranks_on_one_device():
    """bench.py's own multi-rank path on real kernels where only one GPU exists: two ranks of torch.distributed.run, both on
    device 0 (RNNOISE_AMD_BENCH_SHARE_DEVICE=1: gloo carries the reduction, RCCL refuses two ranks on one device) -- disjoint
    stream shards, whole-job aggregate over both ranks, rank-0-only line, parity leg green.  Not a scaling number."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT, RNNOISE_AMD_BENCH_SHARE_DEVICE="1", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--streams", "4096", "--steps", "4",
                        "--warmup", "2", "--repeats", "2", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["shared_device"] is True and d["scaling"] == "weak"
    assert d["config"]["streams_per_gpu"] == 4096 and d["config"]["frames_per_step"] == 8192
    assert d["config"]["stream_ids_by_rank"] == [[0, 4096], [4096, 8192]]
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / 8192 - 1) < 0.01
    assert d["parity"]["bit_identical"] is True and d["config"]["outputs_sane"] is True
    assert "cpu_baseline" not in d


def test_bench_falls_back_to_gloo_when_rccl_refuses():
    """The real RCCL in the failure path of bench.py's collectives (open_collectives): two ranks whose launcher shows each of them ONE
    device -- the same one (HIP_VISIBLE_DEVICES=0) -- both ask RCCL for a communicator, RCCL refuses ("Duplicate GPU detected"), every
    rank votes over the gloo control group, and the job runs to its line on gloo: "collective": "gloo-fallback" with the first error
    text, the aggregate over both ranks, parity green.  What the first multi-GPU run does if its communicator cannot be built."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="0", RNNOISE_AMD_BENCH_DATA_TIMEOUT="30", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RNNOISE_AMD_BENCH_SHARE_DEVICE", "RNNOISE_AMD_BENCH_DATA_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--streams", "4096", "--steps", "4",
                        "--warmup", "2", "--repeats", "2", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    if d["collective"] == "rccl":
        pytest.skip("this RCCL accepts two ranks on one device: nothing to fall back from")
    assert d["collective"] == "gloo-fallback" and d["collective_error"], d
    assert d["n_gpus"] == 2 and len(d["value_by_rank"]) == 2
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / 8192 - 1) < 0.01
    assert d["parity"]["bit_identical"] is True and d["config"]["outputs_sane"] is True


def test_bench_dump_outputs_are_the_last_timed_step(tmp_path):
    """bench.py --dump-outputs: what the last of the --steps timed steps returned to its caller (PCM, VAD, raw gains of every
    stream of a small batch) is written as float32 .npy; it is bit-identical to the oracle on the same input frames, and a
    second run with the same arguments writes the same bytes (the inputs depend on the arguments alone)"""
    import json

    import torch

    import bench
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    N, K, W = 40, 5, 2
    args = ["--streams", str(N), "--steps", str(K), "--warmup", str(W), "--repeats", "2", "--no-cpu-baseline", "--no-parity"]
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == K and d["steps_by_repeat"] == [3, 2]
        assert d["dump_outputs"]["frame"] == W + K - 1 and d["dump_outputs"]["streams"] == N and not d["dump_outputs"]["sampled"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["gains.npy", "pcm_out.npy", "stream_id.npy", "vad.npy"]
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.tobytes() == b.tobytes(), f
    out, vad, gains = (np.load(tmp_path / "a" / f) for f in ("pcm_out.npy", "vad.npy", "gains.npy"))
    assert out.shape == (N, 480) and vad.shape == (N,) and gains.shape == (N, 32)
    assert (np.load(tmp_path / "a" / "stream_id.npy") == np.arange(N)).all()
    # the bench's own input (W + K frames fit in its smallest input ring: no wrap), through the oracle up to the last timed step
    pcm = bench.synth_pcm_torch(torch, N, 8, torch.device("cuda", 0), 0)[:W + K].cpu().numpy()
    blob = load_blob("default")
    for s in (0, 17, N - 1):
        want = Oracle(blob).run(pcm[:, s])
        assert_bits_equal(out[s], want["out"][-1], f"stream {s} pcm")
        assert_bits_equal(vad[s], want["vad"][-1], f"stream {s} vad")
        assert_bits_equal(gains[s], want["gains"][-1], f"stream {s} gains")
