"""The ORDER of include/rnnoise_amd_score.h restated in numpy float64 -- what rn_audio_score_kernel is held to bit for bit: the lane
mapping, eight chains per lane from 0.0, the butterfly over lane ^ m, frame after frame, ADD into the sums.  Every operation below
is one elementwise IEEE double operation of numpy (no np.sum, no dot, no fused multiply-add), so the order is the text's."""
import numpy as np

FRAME, SLOTS, WAVE, DELAY = 480, 8, 64, 960
# lane l, step j -> the output sample it takes: granule l (j < 4), then granule l + 64 (j >= 4; lanes 56..63 have none)
LANE = np.arange(WAVE)[:, None]
STEP = np.arange(8)[None, :]
SAMPLE = 4 * LANE + 256 * (STEP >> 2) + (STEP & 3)      # (64, 8)
VALID = SAMPLE < FRAME                                   # lanes 56..63 x steps 4..7: no sample
SAMPLE = np.where(VALID, SAMPLE, 0)


def rows_view(plane, frame_stride, row_stride, n_rows, T):
    """a flat float32 plane as (n_rows, T, 480): sample i of frame t of row s at t * frame_stride + s * row_stride + i"""
    plane = np.asarray(plane)
    assert plane.dtype == np.float32 and plane.ndim == 1
    assert T == 0 or (T - 1) * frame_stride + (n_rows - 1) * row_stride + FRAME <= plane.size
    return np.lib.stride_tricks.as_strided(plane, (n_rows, T, FRAME), (4 * row_stride, 4 * frame_stride, 4), writeable=False)


def sequences(plane, frame_stride, row_stride, n_rows, T):
    """... as (n_rows, T * 480) float64, a copy: sample n of a row"""
    return rows_view(plane, frame_stride, row_stride, n_rows, T).astype(np.float64).reshape(n_rows, T * FRAME)


def terms(r, x, y):
    """the eight terms of samples r, x, y (float64 arrays of one shape) -> shape + (8,)"""
    with np.errstate(all="ignore"):
        xr, yr = x - r, y - r
        return np.stack([r * r, x * x, y * y, x * r, y * r, xr * xr, yr * yr, np.ones_like(r)], -1)


def frame_record(r, x, y):
    """r, x, y: (rows, 480) float64, the delayed ref / in and the out samples of ONE output frame -> (rows, 8), the frame record"""
    tm = terms(r[:, SAMPLE], x[:, SAMPLE], y[:, SAMPLE])          # (rows, 64, 8 steps, 8 slots)
    acc = np.zeros((r.shape[0], WAVE, SLOTS))
    with np.errstate(all="ignore"):
        for j in range(8):
            # (a lane without step j keeps its accumulator: no operation, as in the kernel)
            acc = np.where(VALID[None, :, j, None], acc + tm[:, :, j], acc)
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, np.arange(WAVE) ^ m]
    assert all(np.array_equal(acc[:, 0], acc[:, l], equal_nan=True) for l in (1, 31, 32, 63))
    return acc[:, 0]


def score(ref, inp, out, n_rows, t0, n_frames, first, delay, sums, frame_terms=None):
    """ref, inp, out: (plane, frame_stride, row_stride) with flat float32 planes holding the sequences from frame 0.  ADDS to
    sums (n_rows, 8) in place and writes the records of the scored frames into frame_terms (n_rows, T, 8) where given."""
    assert first * FRAME >= delay >= 0
    T = t0 + n_frames
    r, x, y = (sequences(*p, n_rows, T) for p in (ref, inp, out))
    with np.errstate(all="ignore"):
        for t in range(max(t0, first), T):
            n0 = t * FRAME
            rec = frame_record(r[:, n0 - delay:n0 - delay + FRAME], x[:, n0 - delay:n0 - delay + FRAME], y[:, n0:n0 + FRAME])
            sums[:] = sums + rec
            if frame_terms is not None:
                frame_terms[:, t] = rec
    return sums


def planes(rng, n_rows, T, layout, special=True):
    """ref, in, out as (flat, frame_stride, row_stride) in `layout` ("frames": [T][N][480]; "streams": padded [N][T * 480 + 16]) --
    random floats in the int16 range, one all-zero frame per plane, and with `special` a row of +-3e38 (the last but one, where
    there are three) and a NaN in the last row's out (where there are two)"""
    fs, rs = (n_rows * FRAME, FRAME) if layout == "frames" else (FRAME, T * FRAME + 16)
    out = []
    for p in range(3):
        size = (T - 1) * fs + (n_rows - 1) * rs + 480 + (16 if layout == "streams" else 0)
        flat = np.full(size, 12345.0, np.float32)  # (the padding holds a value that would show in a sum)
        v = np.lib.stride_tricks.as_strided(flat, (n_rows, T, 480), (4 * rs, 4 * fs, 4))
        v[:] = rng.uniform(-32768, 32767, (n_rows, T, 480)).astype(np.float32)
        v[:, (p + 1) % T] = 0
        if special and n_rows >= 3:
            v[n_rows - 2] = np.where(rng.random((T, 480)) < .5, np.float32(3e38), np.float32(-3e38))
        out.append((flat, fs, rs))
    if special and n_rows >= 2:
        np.lib.stride_tricks.as_strided(out[2][0], (n_rows, T, 480), (4 * out[2][2], 4 * out[2][1], 4))[n_rows - 1, T - 1, 77] = np.nan
    return out
