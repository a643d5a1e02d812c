"""Training data on the GPU: what the reference's src/dump_features.c does per sequence, in batches (include/rnnoise_amd.h:
RNNoiseTrainMix).  draw() makes the random choices of dump_features.c:367-406 and :454 / :460 on the host; generate() runs everything
from the int16 corpora to the 98-float records on the device, one sequence per stream of a batch and round:

    levels with the Viterbi VAD in the same launch (rnnoise_batch_train_levels_vad_device) ->
    mix (rnnoise_batch_train_mix_device) [-> RIR (rnnoise_batch_train_rir_device)] -> features (rnnoise_batch_train_features_device)

with nothing copied back and no synchronisation between the kernels -- or, on a host whose libm the device does not restate (vad="host"):

    levels (rnnoise_batch_train_levels_device) -> energies to the host -> Viterbi VAD (rnnoise_amd_train_vad) -> mix -> ...

For the same draws the records are bit for bit the reference's.  Its optional RIR filtering (-rir_list) is the bracketed step:
rir_spectra() transforms a list of room impulse responses once, draw_rir() makes the choices of dump_features.c:449-450, and
generate(..., rirs=(spectra, records)) filters between mix and clip.  draw() and draw_rir() follow the reference's distributions, not
glibc's rand() stream.

mix_rounds() stops in front of the features call and yields the audio itself -- clean, noisy and the VAD target of every round, on the
device -- for rnnoise_amd.evaluate.evaluate_audio, which denoises the noisy plane and scores the result against the clean one.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import capi

FRAME = capi.FRAME
FREQ_SIZE = 481
NB_BANDS = capi.NB_BANDS
REC = capi.NB_FEATURES + NB_BANDS + 1  # features | gain targets | vad
# the band edges in bins (src/denoise.c:63-65), as far as dump_features.c:401-406 looks
EBAND = (0, 2, 4, 6, 8, 10, 12, 15, 18, 21, 24, 28, 32, 36, 41, 47, 53, 60, 68, 77, 87, 98, 110, 124, 140, 157, 176, 198, 223, 251, 282, 317)

# draw() takes all its uniform numbers of a sequence from one row of rng.random((n, N_UNIFORM)); the columns:
U_POS = 0          # 3: the positions in the three corpora
U_START = 3        # 2: start_pos -- whether, and how far
U_GAIN = 5         # 6: speech, noise, foreground noise, two each
U_NO_NOISE = 11    # noise_gain = 0 with probability 1/8
U_FG = 12          # fgnoise_gain stays with probability 1/8
U_QUIET = 13       # both noise gains * 0.03 with probability 1/12
U_FILT = 14        # 6 filters (a_noise, b_noise, a_fgnoise, b_fgnoise, a_sig, b_sig), 4 each: branch, kind, two values
U_LOWPASS = 38
U_CLIP = 39
U_QUANT = 40
N_UNIFORM = 41


class Draws(NamedTuple):
    mix: np.ndarray        # (n,) capi.MIX_DTYPE
    start_pos: np.ndarray  # (n,) int32, samples: the VAD is cleared before it (dump_features.c:382-384, :437)
    lowpass: np.ndarray    # (n,) int32, first zeroed FFT bin (dump_features.c:400)
    band_lp: np.ndarray    # (n,) int32, last band with a valid gain target (dump_features.c:401-406)


def band_lp_of(lowpass: int, previous: int) -> int:
    """dump_features.c:401-406: the first band whose edge lies above `lowpass` -- and, as in the reference, the PREVIOUS sequence's
    value when no band does (band_lp is a global there, 32 before the first sequence)"""
    for i in range(NB_BANDS):
        if EBAND[i] > lowpass:
            return i
    return previous


def _rand_filt(u):
    """rand_filt (dump_features.c:159-178) from four uniform numbers per filter: u (n, 4) -> (n, 2) float32"""
    f32 = np.float32
    r = (f32(.7) * u[:, 2] * u[:, 2]).astype(f32)
    theta = (np.pi * u[:, 3] * u[:, 3]).astype(f32)
    pair = np.stack([-2 * r * np.cos(theta.astype(np.float64)), r.astype(np.float64) * r], 1)
    r0 = (1.4 * (u[:, 2] - .5)).astype(f32).astype(np.float64)
    r1 = (1.4 * (u[:, 3] - .5)).astype(f32).astype(np.float64)
    real = np.stack([-r0 - r1, r0 * r1], 1)
    out = np.where((u[:, 1] > .5)[:, None], pair, real)
    out[u[:, 0] >= 1 / 3] = 0  # rand() % 3 != 0
    return out.astype(f32)


def draw(rng: np.random.Generator, n: int, lens, n_frames: int, band_lp: int = NB_BANDS) -> Draws:
    """The draws of n sequences of n_frames frames from corpora of lens = (speech, noise, foreground noise) samples, in sequence
    order.  band_lp: the value carried in from the sequence before the first one (32 at the start of a run)."""
    f32 = np.float32
    span = FRAME * n_frames
    if min(lens) < span:
        raise ValueError(f"a corpus of {min(lens)} samples is shorter than a sequence of {span}")
    u = np.asarray(rng.random((n, N_UNIFORM)), np.float64)
    assert u.shape == (n, N_UNIFORM)
    mix = np.zeros(n, capi.MIX_DTYPE)
    for k, name in enumerate(("speech_pos", "noise_pos", "fgnoise_pos")):
        mix[name] = np.minimum((u[:, U_POS + k] * lens[k]).astype(np.int64), lens[k] - span)
    # start_pos = 0 three times out of four, else -(int)(1000 * log(uniform)), at most the sequence (:382-384)
    far = (-1000.0 * np.log(1.0 - u[:, U_START + 1])).astype(np.int64)
    start_pos = np.where(u[:, U_START] < .75, 0, np.minimum(far, span)).astype(np.int32)
    g = u[:, U_GAIN:U_GAIN + 6]
    speech = (10.0 ** ((-45 + 45 * g[:, 0] + 10 * g[:, 1]) / 20)).astype(f32)
    noise = (10.0 ** ((-30 + 40 * g[:, 2] + 15 * g[:, 3]) / 20)).astype(f32)
    fg = (10.0 ** ((-30 + 40 * g[:, 4] + 15 * g[:, 5]) / 20)).astype(f32)
    noise[u[:, U_NO_NOISE] < 1 / 8] = 0
    fg[u[:, U_FG] >= 1 / 8] = 0
    quiet = u[:, U_QUIET] < 1 / 12
    noise[quiet] = (noise[quiet] * 0.03).astype(f32)
    fg[quiet] = (fg[quiet] * 0.03).astype(f32)
    mix["speech_gain"], mix["noise_gain"], mix["fgnoise_gain"] = speech, noise * speech, fg * speech
    for k, name in enumerate(("a_noise", "b_noise", "a_fgnoise", "b_fgnoise", "a_sig", "b_sig")):
        mix[name] = _rand_filt(u[:, U_FILT + 4 * k:U_FILT + 4 * k + 4])
    lowpass = (FREQ_SIZE * 3000. / 24000. * 50.0 ** u[:, U_LOWPASS]).astype(np.int32)
    bands = np.empty(n, np.int32)
    for i in range(n):  # (in sequence order: the carry-over)
        band_lp = bands[i] = band_lp_of(int(lowpass[i]), band_lp)
    mix["clip"] = u[:, U_CLIP] < 1 / 4
    mix["quantize"] = u[:, U_QUANT] < 1 / 2
    return Draws(mix, start_pos, lowpass, bands)


def draw_rir(rng: np.random.Generator, n: int, n_rirs: int) -> np.ndarray:
    """dump_features.c:449-450 for n sequences: a room impulse response is applied with probability 1/2, and then it is one of the
    n_rirs of the list, each as likely -> (n,) capi.RIR_DTYPE with rir_id = -1 where none is applied.  The uniform numbers are this
    function's own rng.random((n, 2)); draw() takes none of them.  clip and quantize stay 0 here: generate() fills them in from
    the mix table of draw()."""
    if n_rirs < 1:
        raise ValueError("an empty RIR list")
    u = np.asarray(rng.random((n, 2)), np.float64)
    assert u.shape == (n, 2)
    rec = np.zeros(n, capi.RIR_DTYPE)
    rec["rir_id"] = np.where(u[:, 0] < .5, np.minimum((u[:, 1] * n_rirs).astype(np.int64), n_rirs - 1), -1)
    return rec


def rir_spectra(batch: capi.Batch, responses, device):
    """load_rir (dump_features.c:63-88) for a list of room impulse responses, 1-D float arrays of which the first 32768 samples count
    -> the (len(responses), 2, 65536, 2) float32 torch tensor on `device` that generate(rirs=...) takes: per response the spectrum of
    the whole one (for the noisy signal) and of its early part (for the clean signal)."""
    import torch
    rows = np.zeros((len(responses), capi.RIR_MAX), np.float32)
    lens = np.empty(len(responses), np.int32)
    for i, h in enumerate(responses):
        h = np.asarray(h, np.float32).ravel()[:capi.RIR_MAX]
        if len(h) < 1:
            raise ValueError(f"room impulse response {i} is empty")
        rows[i, :len(h)], lens[i] = h, len(h)
    d_rows = torch.from_numpy(rows).to(device)
    spectra = torch.empty((len(responses), 2, capi.RIR_FFT, 2), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        batch.train_rir_load_device(spectra.data_ptr(), d_rows.data_ptr(), lens, torch.cuda.current_stream(device).cuda_stream)
        torch.cuda.current_stream(device).synchronize()  # (d_rows dies here)
    return spectra


def _pad(a, n):
    """a round's table for a batch of n streams: the streams behind the last sequence repeat it (their records are dropped)"""
    return a if len(a) == n else np.concatenate([a, np.repeat(a[-1:], n - len(a), 0)])


def _mix_rounds(batch: capi.Batch, speech, noise, fgnoise, draws: Draws, n_frames: int, rirs, rir_work_bytes: int, vad: str):
    """the front of a round, shared by generate_rounds and mix_rounds: levels (+ VAD) -> mix [-> RIR] for sequences [r * N, (r + 1) * N)
    of `draws`, r = 0, 1, ...  Yields (first, k, clean, noisy, vad_target, noise_free, stream): the round's first sequence, how many
    of its N streams carry one, the device tensors the calls filled -- reused by the next round -- and the stream they ran on."""
    import torch
    if vad not in ("auto", "device", "host"):
        raise ValueError(f"vad={vad!r}: auto | device | host")
    on_device = vad == "device" or (vad == "auto" and capi.train_vad_device_available())
    N = batch.n
    corpora = (speech, noise, fgnoise)
    for c in corpora:
        assert c.dtype == torch.int16 and c.dim() == 1 and c.is_cuda and c.is_contiguous(), (c.dtype, c.shape, c.device)
    dev = speech.device
    ptrs, lens = [c.data_ptr() for c in corpora], [c.numel() for c in corpora]
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    energy, rms = new((N, n_frames)), new((N, 3))
    clean, noisy = new((n_frames, N, FRAME)), new((n_frames, N, FRAME))
    vad_target, noise_free = new((n_frames, N)), new((N,), torch.int32)
    d_vad = new((N, n_frames), torch.uint8) if on_device else None
    count = len(draws.mix)
    if rirs is not None:
        spectra, rir_rec = rirs
        assert spectra.dtype == torch.float32 and spectra.is_cuda and spectra.is_contiguous() and spectra.shape[1:] == (2, capi.RIR_FFT, 2)
        assert len(rir_rec) == count, (len(rir_rec), count)
        rir_rec = np.array(rir_rec, capi.RIR_DTYPE)
        rir_rec["clip"], rir_rec["quantize"] = draws.mix["clip"], draws.mix["quantize"]
        work = new((rir_work_bytes,), torch.uint8)
    for first in range(0, count, N):
        k = min(N, count - first)
        rows = slice(first, first + k)
        mix = _pad(draws.mix[rows], N)
        if rirs is not None:
            mix = mix.copy()
            mix["clip"] = mix["quantize"] = 0
        st = torch.cuda.current_stream(dev).cuda_stream
        if on_device:
            batch.train_levels_vad_device(energy.data_ptr(), rms.data_ptr(), d_vad.data_ptr(), ptrs, lens, mix,
                                          _pad(draws.start_pos[rows], N), n_frames, st)
        else:
            batch.train_levels_device(energy.data_ptr(), rms.data_ptr(), ptrs, lens, mix, n_frames, st)
            d_vad = torch.from_numpy(capi.train_vad(energy.cpu().numpy(), _pad(draws.start_pos[rows], N))).to(dev)
        batch.train_mix_device(clean.data_ptr(), noisy.data_ptr(), vad_target.data_ptr(), noise_free.data_ptr(), ptrs, lens, mix,
                               rms.data_ptr(), d_vad.data_ptr(), n_frames, st)
        if rirs is not None:
            batch.train_rir_device(clean.data_ptr(), noisy.data_ptr(), spectra.data_ptr(), len(spectra), _pad(rir_rec[rows], N),
                                   work.data_ptr(), rir_work_bytes, n_frames, st)
        yield first, k, clean, noisy, vad_target, noise_free, st


def mix_rounds(batch: capi.Batch, speech, noise, fgnoise, draws: Draws, n_frames: int, rirs=None, vad: str = "auto",
               rir_work_bytes: int = 256 << 20):
    """The sequences of `draws` as AUDIO, round by round: what generate_rounds runs in front of its features call -- levels (+ VAD)
    -> mix -> optional RIR -- and nothing behind it.  Yields (k, clean, noisy, vad_target) per round: clean and noisy
    (n_frames, N, 480) float32 and vad_target (n_frames, N) float32 tensors on the batch's device, of which streams 0 .. k - 1
    carry sequences [r * N, r * N + k) of round r (a partial last round repeats its last sequence on the others).  The tensors are
    the generator's own and valid until the next iteration; the work is enqueued on torch's current stream.  The calls read and
    write nothing of the batch's per-stream denoiser state (they use its device, its size and its upload buffers), so the same
    batch may denoise `noisy` in between.  Arguments as in generate_rounds."""
    for _first, k, clean, noisy, vad_target, _noise_free, _st in _mix_rounds(batch, speech, noise, fgnoise, draws, n_frames, rirs,
                                                                             rir_work_bytes, vad):
        yield k, clean, noisy, vad_target


def generate_rounds(batch: capi.Batch, speech, noise, fgnoise, draws: Draws, n_frames: int, rirs=None, rir_work_bytes: int = 256 << 20,
                    vad: str = "auto"):
    """Yields the records of sequences [r * N, (r + 1) * N) of `draws`, r = 0, 1, ..., each a (sequences, n_frames, 98) float32 array:
    sequence i runs on stream i % N of `batch` (N streams) in round i // N, and the batch's per-stream analysis state carries from one
    sequence of a stream to the next, as the reference's two DenoiseStates carry across its loop.  speech, noise, fgnoise: the corpora
    as 1-D int16 torch tensors on the batch's device.  Everything is enqueued on torch's current stream.  vad: where the Viterbi VAD of the
    frame energies runs -- "device": in the levels launch, a round then copies nothing back and does not synchronise between its
    kernels (RuntimeError on a host whose libm the device does not restate, capi.train_vad_device_available()); "host": the energies
    go to the host, rnnoise_amd_train_vad decodes them on one thread, the bytes go back; "auto" (the default): "device" where
    available, else "host".  The records are the same to the byte.  When the last round is partial, the streams behind the last sequence run that
    sequence again (records dropped), so their analysis state advances too: a later call on the same batch starts those streams from
    a state that no sequence of the file order left.  Reset the batch, or use a sequence count that is a multiple of N, where that
    matters; one run of the command line is not affected.
    rirs = (spectra, records): the tensor of rir_spectra() and draw_rir()'s records, one per sequence of `draws`.  The mix then runs
    without clipping and quantisation, and the RIR call filters the sequences the records name and applies the flags of `draws` to
    all (dump_features.c:449-465), in a workspace of rir_work_bytes (at least capi.train_rir_work_bytes(1)).  Without rirs nothing
    changes."""
    for k, rec in generate_rounds_device(batch, speech, noise, fgnoise, draws, n_frames, rirs, rir_work_bytes, vad):
        yield rec.permute(1, 0, 2)[:k].contiguous().cpu().numpy()  # sequence-major: the reference's file order


def generate_rounds_device(batch: capi.Batch, speech, noise, fgnoise, draws: Draws, n_frames: int, rirs=None,
                           rir_work_bytes: int = 256 << 20, vad: str = "auto"):
    """generate_rounds with the records left where the features call wrote them: yields (k, rec) per round, rec the
    (n_frames, N, 98) float32 tensor on the batch's device -- record t of stream s at rec[t, s]: strides (N * 98, 98) in the words
    of the score and loss calls -- of which streams 0 .. k - 1 carry sequences [r * N, r * N + k) of round r.  The tensor is the
    generator's own, reused by the next round and valid until the next iteration; the work is enqueued on torch's current stream and
    nothing is copied back or waited for (with the VAD on the device).  This is the online data of rnnoise_amd.train.  Arguments,
    carried state and the partial last round as in generate_rounds, which yields the bytes of these tensors."""
    import torch
    rec = None
    for first, k, clean, noisy, vad_target, noise_free, st in _mix_rounds(batch, speech, noise, fgnoise, draws, n_frames, rirs,
                                                                          rir_work_bytes, vad):
        N, dev = batch.n, clean.device
        if rec is None:
            rec = torch.empty((n_frames, N, REC), dtype=torch.float32, device=dev)
        rows = slice(first, first + k)
        d_lowpass = torch.from_numpy(_pad(draws.lowpass[rows], N).astype(np.int32)).to(dev)
        d_band_lp = torch.from_numpy(_pad(draws.band_lp[rows], N).astype(np.int32)).to(dev)
        batch.train_features_device(rec.data_ptr(), clean.data_ptr(), noisy.data_ptr(), vad_target.data_ptr(), d_lowpass.data_ptr(),
                                    d_band_lp.data_ptr(), noise_free.data_ptr(), n_frames, st)
        yield k, rec


def generate(batch: capi.Batch, speech, noise, fgnoise, draws: Draws, n_frames: int, rirs=None, rir_work_bytes: int = 256 << 20,
             vad: str = "auto") -> np.ndarray:
    """all records of `draws`, (sequences, n_frames, 98) float32 in sequence order (generate_rounds)"""
    return np.concatenate(list(generate_rounds(batch, speech, noise, fgnoise, draws, n_frames, rirs, rir_work_bytes, vad)))
