"""ctypes binding of librnnoise_amd.so -- the C-ABI boundary of the product.

Python host-side mirror of the reference's plugin interface for this path: the names,
argument meaning and error behaviour are those of include/rnnoise.h (drop-in, reference
rnnoise.h:51-125) and include/rnnoise_amd.h (additive batched API).  There is no fallback:
if the HIP library is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RNNOISE_AMD_LIB", os.path.join(HERE, "librnnoise_amd.so"))  # env override: A/B builds
# the instrumented build of the same sources (-DRN_INSTRUMENT=1): stage taps + probe kernels + include/rnnoise_amd_debug.h
INSTR_LIB_PATH = os.path.join(HERE, "librnnoise_amd_instr.so")

FRAME = 480
NB_BANDS = 32
NB_FEATURES = 65
STATE_FLOATS = 6282
# the stream snapshot of rnnoise_batch_save_streams (include/rn_layout.h: RN_SNAP_*): the portable state, a header of int32 words, the
# resampler history
SNAP_OFF_MAGIC = STATE_FLOATS
SNAP_OFF_L = SNAP_OFF_MAGIC + 1
SNAP_OFF_GATE = SNAP_OFF_MAGIC + 2
SNAP_OFF_RESERVED = SNAP_OFF_MAGIC + 3
SNAP_OFF_OUT_L = SNAP_OFF_RESERVED  # RN_SNAP_OFF_OUT_L: the code of the down history under an out-rate table, 0 without one
SNAP_OFF_HIST = SNAP_OFF_MAGIC + 6
SNAP_HIST_FLOATS = 336
SNAP_FLOATS = SNAP_OFF_HIST + SNAP_HIST_FLOATS  # 6624
SNAP_MAGIC = 0x534E5201
SNAP_GATE_NONE = 65536
# the FIFO record of rnnoise_batch_save_chunk_fifos (include/rnnoise_amd.h): pending samples, output FIFO, then int32 r, M, magic, 0
CHUNK_FIFO_ROW = 480
CHUNK_OFF_FILL = 2 * CHUNK_FIFO_ROW
CHUNK_OFF_M = CHUNK_OFF_FILL + 1
CHUNK_OFF_MAGIC = CHUNK_OFF_FILL + 2
CHUNK_REC_FLOATS = CHUNK_OFF_FILL + 4  # 964
CHUNK_MAGIC = 0x464B4301

_lib = None
_product = None
_instr = None

# The prototypes of the C API: symbol -> (restype, argtypes), in the order of the headers.  _load applies them; tests/test_capi_cpu.py
# holds every entry to its declaration (parameter count and return class).  A new entry point gets one line here and nowhere else.
# Batch, model and state handles, device pointers, streams and struct pointers are plain addresses (_vp); host arrays are typed.
_int, _long, _ll, _uint, _vp, _cp = C.c_int, C.c_long, C.c_longlong, C.c_uint, C.c_void_p, C.c_char_p
_fp_t, _ip, _sp, _up, _dp, _lp = (C.POINTER(t) for t in (C.c_float, C.c_int, C.c_short, C.c_ubyte, C.c_double, C.c_long))
_PCM = object()  # stands for the PCM pointer of a host call in _twins: float * in the float call, short * in its "_s16" twin


def _twins(name, argtypes):
    """a call and its int16 twin, declared next to each other in the header"""
    return {name + sfx: (_int, tuple(pp if a is _PCM else a for a in argtypes)) for sfx, pp in (("", _fp_t), ("_s16", _sp))}


def _stream_table(name, tp):
    """the three calls of a per-stream table: host setter, device setter (table, stream), getter"""
    return {f"rnnoise_batch_set_stream_{name}": (_int, (_vp, tp)), f"rnnoise_batch_set_stream_{name}_device": (_int, (_vp, _vp, _vp)),
            f"rnnoise_batch_stream_{name}": (_int, (_vp, tp))}


PROTOTYPES = {
    # include/rnnoise.h
    "rnnoise_get_size": (_int, ()),
    "rnnoise_get_frame_size": (_int, ()),
    "rnnoise_init": (_int, (_vp, _vp)),
    "rnnoise_create": (_vp, (_vp,)),
    "rnnoise_destroy": (_int, (_vp,)),
    "rnnoise_process_frame": (C.c_float, (_vp, _fp_t, _fp_t)),
    "rnnoise_model_from_buffer": (_vp, (_cp, _int)),
    "rnnoise_model_from_file": (_vp, (_vp,)),
    "rnnoise_model_from_filename": (_vp, (_cp,)),
    "rnnoise_model_free": (_int, (_vp,)),
    # include/rnnoise_amd.h
    "rnnoise_amd_device_count": (_int, ()),
    "rnnoise_amd_set_rcp_profile": (_int, (_cp,)),
    "rnnoise_amd_rcp_profile": (_cp, ()),
    "rnnoise_amd_log10_model": (_cp, ()),
    "rnnoise_batch_create": (_vp, (_vp, _int, _int)),
    "rnnoise_batch_destroy": (_int, (_vp,)),
    "rnnoise_batch_size": (_int, (_vp,)),
    "rnnoise_batch_reset": (_int, (_vp,)),
    "rnnoise_batch_process": (_int, (_vp, _fp_t, _fp_t, _fp_t, _fp_t, _int)),
    "rnnoise_batch_process_device": (_int, (_vp,) * 5 + (_int, _vp)),
    "rnnoise_batch_process_s16": (_int, (_vp, _sp, _sp, _fp_t, _fp_t, _int)),
    "rnnoise_batch_process_device_s16": (_int, (_vp,) * 5 + (_int, _vp)),
    **_twins("rnnoise_batch_process_device_masked", (_vp,) * 6 + (_int, _vp)),
    **_twins("rnnoise_batch_process_masked", (_vp, _PCM, _PCM, _fp_t, _fp_t, _up, _int)),
    **_twins("rnnoise_batch_process_device_list", (_vp,) * 6 + (_int, _vp, _int, _vp)),
    **_twins("rnnoise_batch_process_list", (_vp, _PCM, _PCM, _fp_t, _fp_t, _ip, _int, _up, _int)),
    "rnnoise_batch_reset_streams": (_int, (_vp, _ip, _int)),
    "rnnoise_batch_reset_streams_device": (_int, (_vp, _vp, _int, _vp)),
    "rnnoise_batch_set_pcm_rate": (_int, (_vp, _int)),
    "rnnoise_batch_pcm_rate": (_int, (_vp,)),
    **_stream_table("rates", _up),
    **_stream_table("formats", _up),
    **_stream_table("out_rates", _up),
    **_stream_table("out_formats", _up),
    "rnnoise_batch_set_pcm_layout": (_int, (_vp, _long, _long)),
    "rnnoise_batch_pcm_layout": (_int, (_vp, _lp, _lp)),
    "rnnoise_amd_pcm_layout_fits": (_int, (_long, _long, _int, _int, _int)),
    "rnnoise_batch_set_pcm_channels": (_int, (_vp, _int)),
    "rnnoise_batch_pcm_channels": (_int, (_vp,)),
    "rnnoise_amd_pcm_channels_fit": (_int, (_long, _long, _int, _int, _int, _int)),
    "rnnoise_batch_set_gain_link": (_int, (_vp, _int)),
    "rnnoise_batch_gain_link": (_int, (_vp,)),
    "rnnoise_batch_add_model": (_int, (_vp, _vp)),
    **_stream_table("models", _up),
    **_stream_table("controls", _fp_t),
    "rnnoise_batch_export_state": (_int, (_vp, _int, _fp_t)),
    "rnnoise_batch_import_state": (_int, (_vp, _int, _fp_t)),
    "rnnoise_batch_save_streams_device": (_int, (_vp, _vp, _vp, _int, _vp)),
    "rnnoise_batch_load_streams_device": (_int, (_vp, _vp, _vp, _int, _vp)),
    "rnnoise_batch_save_streams": (_int, (_vp, _fp_t, _ip, _int)),
    "rnnoise_batch_load_streams": (_int, (_vp, _fp_t, _ip, _int)),
    "rnnoise_amd_chunk_frames": (_int, (_int, _int)),
    **_twins("rnnoise_batch_process_device_chunks", (_vp,) * 4 + (_int,) + (_vp,) * 4),
    **_twins("rnnoise_batch_process_chunks", (_vp, _PCM, _PCM, _ip, _int, _fp_t, _fp_t, _ip)),
    "rnnoise_batch_chunk_fill": (_int, (_vp, _ip)),
    **_twins("rnnoise_batch_process_device_chunks_list", (_vp,) * 4 + (_int, _vp, _int) + (_vp,) * 4),
    **_twins("rnnoise_batch_process_chunks_list", (_vp, _PCM, _PCM, _ip, _int, _ip, _int, _fp_t, _fp_t, _ip)),
    "rnnoise_batch_save_chunk_fifos_device": (_int, (_vp, _vp, _vp, _int, _vp)),
    "rnnoise_batch_load_chunk_fifos_device": (_int, (_vp, _vp, _vp, _int, _vp)),
    "rnnoise_batch_save_chunk_fifos": (_int, (_vp, _fp_t, _ip, _int)),
    "rnnoise_batch_load_chunk_fifos": (_int, (_vp, _fp_t, _ip, _int)),
    "rnnoise_batch_set_nn_path": (_int, (_vp, _int)),
    "rnnoise_batch_set_schedule": (_int, (_vp, _int)),
    "rnnoise_model_weight_bytes": (_long, (_vp,)),
    "rnnoise_amd_model_pack": (_long, (_vp, _vp, _long)),
    "rnnoise_batch_train_features": (_int, (_vp, _fp_t, _fp_t, _fp_t, _fp_t, _ip, _ip, _ip, _int)),
    "rnnoise_batch_train_features_device": (_int, (_vp,) * 8 + (_int, _vp)),
    "rnnoise_amd_train_mix_check": (_int, (_vp, _int, _ll, _ll, _ll, _int)),
    "rnnoise_batch_train_levels_device": (_int, (_vp,) * 6 + (_ll, _ll, _ll, _vp, _int, _vp)),
    "rnnoise_amd_train_vad": (_int, (_fp_t, _int, _int, _ip, _up)),
    "rnnoise_amd_train_vad_device_available": (_int, ()),
    "rnnoise_batch_train_levels_vad_device": (_int, (_vp,) * 7 + (_ll, _ll, _ll, _vp, _ip, _int, _vp)),
    "rnnoise_batch_train_mix_device": (_int, (_vp,) * 8 + (_ll, _ll, _ll, _vp, _vp, _vp, _int, _vp)),
    "rnnoise_amd_train_rir_check": (_int, (_vp, _int, _int)),
    "rnnoise_amd_train_rir_work_bytes": (_ll, (_ll,)),
    "rnnoise_batch_train_rir_load_device": (_int, (_vp, _vp, _vp, _ip, _int, _vp)),
    "rnnoise_batch_train_rir_device": (_int, (_vp, _vp, _vp, _vp, _int, _vp, _vp, _ll, _int, _vp)),
    "rnnoise_amd_eval_records_check": (_int, (_vp, _long, _long, _int, _int, _int, _int)),
    "rnnoise_batch_process_features_device": (_int, (_vp,) * 4 + (_long, _long, _int, _vp)),
    "rnnoise_batch_process_features": (_int, (_vp, _fp_t, _fp_t, _fp_t, _long, _long, _int)),
    "rnnoise_batch_eval_records_device": (_int, (_vp,) * 5 + (_long, _long, _int, _int, _vp, _vp)),
    "rnnoise_batch_eval_records": (_int, (_vp, _dp, _fp_t, _fp_t, _fp_t, _long, _long, _int, _int, _vp)),
    "rnnoise_amd_score_records_check": (_int, (_vp,) + (_long,) * 6 + (_int,) * 3),
    "rnnoise_batch_score_records_device": (_int, (_vp, _vp, _vp, _vp, _long, _long, _vp, _long, _long, _vp, _long, _long, _int, _int, _int,
                                                  _vp, _vp)),
    "rnnoise_batch_score_records": (_int, (_vp, _dp, _dp, _fp_t, _long, _long, _fp_t, _long, _long, _fp_t, _long, _long, _int, _int, _int,
                                           _vp)),
    "rnnoise_amd_split_frame_bytes": (_long, (_int,)),
    "rnnoise_amd_split_rows_check": (_int, (_vp, _int, _int, _int)),
    "rnnoise_batch_split_reserve": (_int, (_vp, _int)),
    "rnnoise_batch_split_pending": (_int, (_vp,)),
    **_twins("rnnoise_batch_analyze_device", (_vp,) * 5 + (_int, _vp)),
    **_twins("rnnoise_batch_analyze", (_vp, _fp_t, _vp, _ip, _PCM, _int)),
    **_twins("rnnoise_batch_synthesize_device", (_vp,) * 6 + (_int, _vp)),
    **_twins("rnnoise_batch_synthesize", (_vp, _PCM, _fp_t, _vp, _fp_t, _vp, _int)),
    "rnnoise_batch_debug_last": (_int, (_vp, _fp_t, _ip, _ip)),
    "rnnoise_batch_enable_timing": (_int, (_vp, _int)),
    "rnnoise_batch_kernel_ms": (_int, (_vp, _dp, _lp)),
}
# include/rnnoise_amd_debug.h: present in the instrumented library only
DEBUG_PROTOTYPES = {
    "rnnoise_batch_debug_pitch": (_int, (_vp, _fp_t)),
    "rnnoise_amd_debug_fft": (_int, (_int, _int, _fp_t, _fp_t, _int, _int, C.POINTER(C.c_ulonglong), _ip)),
    "rnnoise_amd_debug_log_energy": (_int, (_int, _fp_t, _fp_t, _int)),
    "rnnoise_amd_debug_log_energy_range": (_int, (_int, _fp_t, _fp_t, _uint, _uint, _int)),
    "rnnoise_amd_debug_train_vad_libm": (_int, (_int, _int, _uint, _uint, _uint, C.POINTER(C.c_ulonglong), C.POINTER(_uint))),
    "rnnoise_amd_debug_train_vad_selfcheck": (None, (_int,)),
}
EXPORTS = list(PROTOTYPES)  # every symbol declared in include/rnnoise.h and include/rnnoise_amd.h
DEBUG_EXPORTS = list(DEBUG_PROTOTYPES)


class TrainMix(C.Structure):
    """RNNoiseTrainMix (include/rnnoise_amd.h): one training sequence's draws.  np.dtype(TrainMix) is the record type of a table."""
    _fields_ = [("speech_pos", C.c_longlong), ("noise_pos", C.c_longlong), ("fgnoise_pos", C.c_longlong),
                ("speech_gain", C.c_float), ("noise_gain", C.c_float), ("fgnoise_gain", C.c_float),
                ("a_sig", C.c_float * 2), ("b_sig", C.c_float * 2), ("a_noise", C.c_float * 2), ("b_noise", C.c_float * 2),
                ("a_fgnoise", C.c_float * 2), ("b_fgnoise", C.c_float * 2), ("clip", C.c_int), ("quantize", C.c_int)]


MIX_DTYPE = np.dtype(TrainMix)


class EvalConfig(C.Structure):
    """RNNoiseEvalConfig (include/rnnoise_amd.h): the perceptual exponent and the first scored step of the eval-records calls"""
    _fields_ = [("gamma", C.c_float), ("first", C.c_int)]


class Rows(C.Structure):
    """RNNoiseRows (include/rnnoise_amd.h): where the rows of a split call's buffer lie, in elements -- frame t of stream s at
    t * frame_stride + s * row_stride; (0, 0), like None, is [frame][n_streams][row]"""
    _fields_ = [("frame_stride", C.c_long), ("row_stride", C.c_long)]


FEATURES = 65  # RNNOISE_AMD_FEATURES: floats of a feature row
EVAL_SUMS = 4  # RNNOISE_AMD_EVAL_SUMS: doubles per stream {sum of gain terms, sum of vad terms, frames scored, 0}
REC = 98       # floats of a training record: 65 features, 32 gain targets, 1 VAD target


class TrainRir(C.Structure):
    """RNNoiseTrainRir (include/rnnoise_amd.h): one sequence's room impulse response (-1: none) and its augmentation flags"""
    _fields_ = [("rir_id", C.c_int), ("clip", C.c_int), ("quantize", C.c_int)]


RIR_DTYPE = np.dtype(TrainRir)
RIR_MAX = 32768  # the samples of a room impulse response that count (RIR_MAX_DURATION); a row of d_rir
RIR_FFT = 65536  # complex points of a spectrum
MAX_CHANNELS = 8  # RNNOISE_AMD_MAX_CHANNELS: interleaved channels of a batch's PCM rows
MAX_MODELS = 8  # RNNOISE_AMD_MAX_MODELS: model slots of a batch
PCM_RATES = (48000, 24000, 16000, 8000)  # the rates that divide 48 kHz: code = divisor
PCM_RATES_ALL = (48000, 32000, 24000, 16000, 8000)  # every rate a batch takes
RATE_32K = 32  # RNNOISE_AMD_RATE_32K: the code of 32 kHz in rate tables and snapshot records


def rate_code(hz):
    """the rate code of include/rnnoise_amd.h for rates in Hz out of PCM_RATES_ALL (scalar or array): 48000 / hz, RATE_32K at 32 kHz"""
    hz = np.asarray(hz, np.int64)
    return np.where(hz == 32000, RATE_32K, 48000 // np.maximum(hz, 1))


def code_rate(code):
    """... and back: Hz of rate codes"""
    code = np.asarray(code, np.int64)
    return np.where(code == RATE_32K, 32000, 48000 // np.maximum(code, 1))
CTL_FLOATS = 3  # RNNOISE_AMD_CTL_FLOATS: {floor, thr, hold} per stream (rnnoise_batch_set_stream_controls)
CTL_HOLD_MAX = 65535


def floor_of_limit_db(limit_db):
    """the linear gain floor of an attenuation limit of `limit_db` dB (scalar or array; 0 dB = floor 1, +inf = no floor):
    float32(10 ** (-limit_db / 20)).  The C API takes the linear floor only."""
    return np.float32(10.0 ** (-np.asarray(limit_db, np.float64) / 20.0))


def controls_table(n_streams, limit_db=None, vad_threshold=0.0, hold_frames=0):
    """the (N, 3) float32 table of rnnoise_batch_set_stream_controls from an attenuation limit in dB (None / inf: no floor), a VAD gate
    threshold (0: no gate) and a hold in frames -- each a scalar or an (N,) array"""
    t = np.zeros((n_streams, CTL_FLOATS), np.float32)
    t[:, 0] = 0.0 if limit_db is None else floor_of_limit_db(limit_db)
    t[:, 1] = vad_threshold
    t[:, 2] = hold_frames
    return t


def limit_db_of_floor(floor):
    """the inverse: the attenuation limit in dB of a linear floor (0 = no limit: +inf)"""
    with np.errstate(divide="ignore"):
        return -20.0 * np.log10(np.asarray(floor, np.float64))


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the same as /opt/rocm's).  If our library were loaded first it would pull
    in the system runtime and a later `import torch` would bring a second one: streams and
    events could then not be shared.  Pre-loading the runtime torch will use makes our
    DT_NEEDED entry resolve to it, whichever import order the application picks."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec and spec.origin:
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    """the library every call of this module goes to: the product, or -- inside `with instrumented():` -- its instrumented twin"""
    global _lib, _product
    if _lib is None:
        if _product is None:
            _product = _load(LIB_PATH, debug=False)
        _lib = _product
    return _lib


class instrumented:
    """`with capi.instrumented():` -- models, batches and calls inside the block use librnnoise_amd_instr.so (taps compiled into
    the kernels, probe kernels, the rnnoise_amd_debug.h entry points).  Objects must not cross the boundary: the two libraries
    are separate images of the same code with separate state.  Tests and tools only; the product never loads it."""

    def __enter__(self):
        global _lib, _instr
        self.prev = lib()
        if _instr is None:
            _instr = _load(INSTR_LIB_PATH, debug=True)
        _lib = _instr
        if self.prev is not _instr:
            _instr.rnnoise_amd_set_rcp_profile(self.prev.rnnoise_amd_rcp_profile().split(b"=")[0])
        return _instr

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        return False


def _load(path, debug):
    _share_hip_runtime_with_torch()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(path)
    for table in (PROTOTYPES, DEBUG_PROTOTYPES) if debug else (PROTOTYPES,):
        for name, (restype, argtypes) in table.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    return L


def set_rcp_profile(name: str) -> None:
    """which CPU family's `rcpps` the activations reproduce: "host" (default) | "intel" | "amd-zen5" (include/rnnoise_amd.h)"""
    if lib().rnnoise_amd_set_rcp_profile(name.encode()) != 0:
        raise ValueError(f"unknown rcp profile {name!r}")


def rcp_profile() -> str:
    return lib().rnnoise_amd_rcp_profile().decode()


def log10_model() -> str:
    """which log10 the feature stage evaluates: "host=glibc-fma" (the host libm's algorithm restated on the device) | "glibc-fma" |
    "ocml" | "host=unknown:ocml" (include/rnnoise_amd.h; $RNNOISE_AMD_LOG10)"""
    return lib().rnnoise_amd_log10_model().decode()


def chunk_frames(frame_samples: int, max_count: int) -> int:
    """F, the frame rows of vad / gains a chunk call of at most max_count samples per stream can complete at a frame of
    frame_samples (rnnoise_amd_chunk_frames; host only).  ValueError for a bad argument."""
    f = lib().rnnoise_amd_chunk_frames(int(frame_samples), int(max_count))
    if f < 0:
        raise ValueError("rnnoise_amd_chunk_frames: frame_samples > 0 and max_count >= 0")
    return f


def pcm_channels_fit(frame_stride: int, row_stride: int, frame_samples: int, channels: int, n_rows: int, n_frames: int) -> bool:
    """whether the group slots of a call with `channels` interleaved channels are disjoint under a PCM layout
    (rnnoise_amd_pcm_channels_fit: n_frames x n_rows // channels slots of frame_samples * channels samples; host only)"""
    return bool(lib().rnnoise_amd_pcm_channels_fit(int(frame_stride), int(row_stride), int(frame_samples), int(channels), int(n_rows),
                                                   int(n_frames)))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _mix_table(mix):
    """a table of RNNoiseTrainMix records as one contiguous array of MIX_DTYPE"""
    mix = np.ascontiguousarray(mix, MIX_DTYPE)
    assert mix.ndim == 1, mix.shape
    return mix


def train_mix_check(mix, lens, n_frames: int) -> bool:
    """rnnoise_amd_train_mix_check: whether every sequence of the table lies inside its corpora (lens: the three corpus lengths in
    samples), every gain and coefficient is finite and the flags are 0 or 1.  Host only."""
    mix = _mix_table(mix)
    return bool(lib().rnnoise_amd_train_mix_check(mix.ctypes.data, len(mix), int(lens[0]), int(lens[1]), int(lens[2]), int(n_frames)))


def _eval_cfg(gamma, first):
    """the RNNoiseEvalConfig of the eval-records calls, or None (the trainer's defaults) when both are None"""
    if gamma is None and first is None:
        return None
    return EvalConfig(0.25 if gamma is None else float(gamma), 4 if first is None else int(first))


def eval_records_check(frame_stride: int, row_stride: int, row_floats: int, n_streams: int, t0: int, n_frames: int, gamma=None,
                       first=None) -> bool:
    """rnnoise_amd_eval_records_check: whether the feature calls accept these arguments -- a finite gamma > 0 and first >= 0 (both
    None: the defaults), t0 and n_frames >= 0, and disjoint slots of row_floats floats under the strides (0, 0: [frame][n][row]).
    Host only."""
    cfg = _eval_cfg(gamma, first)
    return bool(lib().rnnoise_amd_eval_records_check(C.byref(cfg) if cfg is not None else None, int(frame_stride), int(row_stride),
                                                     int(row_floats), int(n_streams), int(t0), int(n_frames)))


def score_records_check(n_rows: int, t0: int, n_frames: int, rec_strides=(0, 0), gain_strides=(0, 0), vad_strides=(0, 0), gamma=None,
                        first=None) -> bool:
    """rnnoise_amd_score_records_check: whether the score calls accept these arguments -- gamma / first as eval_records_check has
    them, n_rows >= 1, t0 and n_frames >= 0, and for each buffer a (frame_stride, row_stride) pair that keeps its slots disjoint
    ((0, 0): [frame][n_rows][row]).  Host only."""
    cfg = _eval_cfg(gamma, first)
    return bool(lib().rnnoise_amd_score_records_check(C.byref(cfg) if cfg is not None else None, int(rec_strides[0]), int(rec_strides[1]),
                                                      int(gain_strides[0]), int(gain_strides[1]), int(vad_strides[0]),
                                                      int(vad_strides[1]), int(n_rows), int(t0), int(n_frames)))


def _rows_arg(rows):
    """the RNNoiseRows argument of a split call: None, a Rows, or a (frame_stride, row_stride) pair -> (keep-alive, pointer)"""
    if rows is None:
        return None, None
    r = rows if isinstance(rows, Rows) else Rows(int(rows[0]), int(rows[1]))
    return r, C.byref(r)


def split_frame_bytes(n_streams: int) -> int:
    """rnnoise_amd_split_frame_bytes: the device bytes one pending frame of the split calls costs a batch of n_streams (host only)"""
    v = lib().rnnoise_amd_split_frame_bytes(int(n_streams))
    if v < 0:
        raise ValueError("rnnoise_amd_split_frame_bytes: n_streams > 0")
    return v


def split_rows_check(rows, row_floats: int, n_streams: int, n_frames: int) -> bool:
    """rnnoise_amd_split_rows_check: whether the split calls accept `rows` (None, Rows or a pair of strides) for rows of row_floats
    floats of n_streams streams over n_frames frames: the default layout, or positive strides with disjoint rows.  Host only."""
    _keep, ptr = _rows_arg(rows)
    return bool(lib().rnnoise_amd_split_rows_check(ptr, int(row_floats), int(n_streams), int(n_frames)))


def eval_losses(sums):
    """the trainer's three means from sums (..., EVAL_SUMS) over all leading axes: dict(frames_scored, gain_loss, vad_loss, loss);
    nan where no frame was scored"""
    tot = np.asarray(sums, np.float64).reshape(-1, EVAL_SUMS).sum(0)
    frames = tot[2]
    gain = tot[0] / (NB_BANDS * frames) if frames else float("nan")
    vad = tot[1] / frames if frames else float("nan")
    return dict(frames_scored=int(frames), gain_loss=float(gain), vad_loss=float(vad), loss=float(gain + .001 * vad))


def train_vad_device_available() -> bool:
    """rnnoise_amd_train_vad_device_available: whether Batch.train_levels_vad_device exists on this host -- its log and pow are the
    ones the device restates"""
    return bool(lib().rnnoise_amd_train_vad_device_available())


def train_vad(energy, start_pos=None):
    """rnnoise_amd_train_vad: energy (n_seq, n_frames) float32 -> vad (n_seq, n_frames) uint8, the reference's Viterbi VAD per row with
    the first start_pos[s] // 480 frames cleared.  Host only."""
    energy = np.ascontiguousarray(energy, np.float32)
    n_seq, n_frames = energy.shape
    sp = None if start_pos is None else np.ascontiguousarray(start_pos, np.int32)
    assert sp is None or sp.shape == (n_seq,), sp.shape
    vad = np.empty((n_seq, n_frames), np.uint8)
    if lib().rnnoise_amd_train_vad(_fp(energy), n_seq, n_frames, sp.ctypes.data_as(C.POINTER(C.c_int)) if sp is not None else None,
                                   vad.ctypes.data_as(C.POINTER(C.c_ubyte))):
        raise ValueError("rnnoise_amd_train_vad failed")
    return vad


def _rir_table(rir):
    """a table of RNNoiseTrainRir records as one contiguous array of RIR_DTYPE"""
    rir = np.ascontiguousarray(rir, RIR_DTYPE)
    assert rir.ndim == 1, rir.shape
    return rir


def train_rir_check(rir, n_rirs: int) -> bool:
    """rnnoise_amd_train_rir_check: whether every rir_id of the table lies in [-1, n_rirs) and the flags are 0 or 1.  Host only."""
    rir = _rir_table(rir)
    return bool(lib().rnnoise_amd_train_rir_check(rir.ctypes.data, len(rir), int(n_rirs)))


def train_rir_work_bytes(n_units: int) -> int:
    """rnnoise_amd_train_rir_work_bytes: the workspace of train_rir_device for n_units transform pairs in flight.  Host only."""
    return int(lib().rnnoise_amd_train_rir_work_bytes(int(n_units)))


def _close_quietly(obj):
    """__del__ helper: at interpreter shutdown this module's globals (and possibly the HIP runtime the handle lives in)
    are already gone -- the process exit reclaims the rest; anywhere else a destructor must not raise."""
    try:
        import sys as _sys
        if _sys is None or _sys.is_finalizing():
            return
        obj.close()
    except Exception:
        pass


class Model:
    """RNNModel from a "DNNw" weight blob (reference: rnnoise_model_from_buffer, rnnoise.h:102)."""

    def __init__(self, blob: bytes):
        self._L = lib()  # the library image that owns this handle (capi.instrumented() swaps the global one)
        self._blob = bytes(blob)  # borrowed by the library for the model's lifetime
        self.h = self._L.rnnoise_model_from_buffer(self._blob, len(self._blob))
        if not self.h:
            raise ValueError("rnnoise_model_from_buffer failed")

    @property
    def weight_bytes(self) -> int:
        w = self._L.rnnoise_model_weight_bytes(self.h)
        if w < 0:
            raise ValueError("weight blob rejected")
        return int(w)

    def pack(self) -> bytes:
        """the model as a GPU-native "RNPK" pack (rnnoise_amd_model_pack); loadable wherever a blob is"""
        n = self._L.rnnoise_amd_model_pack(self.h, None, 0)
        if n <= 0:
            raise ValueError("weight blob rejected")
        buf = C.create_string_buffer(n)
        if self._L.rnnoise_amd_model_pack(self.h, buf, n) != n:
            raise RuntimeError("rnnoise_amd_model_pack failed")
        return buf.raw

    def close(self):
        if getattr(self, "h", None):
            self._L.rnnoise_model_free(self.h)
            self.h = None

    def __del__(self):
        try:
            _close_quietly(self)
        except Exception:  # (at interpreter shutdown the helper itself may already be gone)
            pass


def _encode_rates(b, hz):
    hz = np.asarray(hz).reshape(-1)
    assert hz.size == b.n
    if not np.isin(hz, PCM_RATES_ALL).all():
        raise ValueError(f"stream rate unsupported (each one of {PCM_RATES_ALL})")
    if hz.max(initial=0) > b.pcm_rate:
        raise ValueError(f"a stream rate above the batch's PCM rate {b.pcm_rate}: its frame would not fit its row")
    return np.ascontiguousarray(rate_code(hz), np.uint8)


def _encode_formats(b, formats):
    from . import g711
    if isinstance(formats, np.ndarray) and formats.dtype.kind in "iu":
        formats = formats.reshape(-1).tolist()
    codes = np.array([g711.code(f) for f in formats], np.uint8)
    assert codes.size == b.n
    return codes


def _encode_models(b, models):
    m = np.asarray(models).reshape(-1)
    assert m.size == b.n
    if m.min(initial=0) < 0 or m.max(initial=0) > 255:
        raise ValueError("model slot out of range")
    return np.ascontiguousarray(m, np.uint8)


def _encode_controls(b, ctl):
    c = np.ascontiguousarray(ctl, np.float32)
    assert c.shape == (b.n, CTL_FLOATS), c.shape
    return c


def _same(a):
    return a


def _decode_rates(codes):
    return code_rate(codes).astype(np.int32)


# The per-stream tables of a batch (rnnoise_batch_set_stream_<stem>, ..._device, rnnoise_batch_stream_<stem>): the element type and
# the trailing shape of a row, whether None drops the table, the caller's values -> the C table (encode(batch, values): validates, or
# raises) and back, and what a refusal of the host setter may mean
_StreamTable = collections.namedtuple("_StreamTable", "stem ctype row droppable encode decode why")
_RATES = _StreamTable("rates", C.c_ubyte, (), True, _encode_rates, _decode_rates, "")
_FORMATS = _StreamTable("formats", C.c_ubyte, (), True, _encode_formats, _same, "")
_OUT_RATES = _RATES._replace(stem="out_rates")
_OUT_FORMATS = _FORMATS._replace(stem="out_formats")
_MODELS = _StreamTable("models", C.c_ubyte, (), False, _encode_models, _same, " (an entry names no slot)")
_CONTROLS = _StreamTable("controls", C.c_float, (CTL_FLOATS,), True, _encode_controls, _same,
                         " (an entry is non-finite, out of range or has a fractional hold)")


class Batch:
    """N concurrent streams on one GPU (include/rnnoise_amd.h)."""

    def __init__(self, model: Model, n_streams: int, device: int = 0):
        self._L = lib()  # the library image that owns this handle (capi.instrumented() swaps the global one)
        self.model = model
        self.extra_models = []  # the models of slots 1.. (add_model): held so that they outlive the batch
        self.n = n_streams
        self.h = self._L.rnnoise_batch_create(model.h, n_streams, device)
        if not self.h:
            raise RuntimeError("rnnoise_batch_create failed (no GPU / bad model / out of memory)")

    def close(self):
        if getattr(self, "h", None):
            self._L.rnnoise_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            _close_quietly(self)
        except Exception:  # (at interpreter shutdown the helper itself may already be gone)
            pass

    def reset(self):
        if self._L.rnnoise_batch_reset(self.h):
            raise RuntimeError("reset failed")

    def set_nn_path(self, path: int) -> int:
        r = self._L.rnnoise_batch_set_nn_path(self.h, path)
        if r < 0:
            raise RuntimeError(f"network path {path} unsupported")
        return r

    def set_schedule(self, schedule: int) -> int:
        r = self._L.rnnoise_batch_set_schedule(self.h, schedule)
        if r < 0:
            raise RuntimeError(f"schedule {schedule} unsupported")
        return r

    def set_pcm_rate(self, hz: int) -> int:
        """PCM rate of the batch's calls (rnnoise_batch_set_pcm_rate): one of PCM_RATES_ALL; returns the previous one.
        At rate R the PCM arrays of every call are (T, N, 480 * R // 48000)."""
        r = self._L.rnnoise_batch_set_pcm_rate(self.h, int(hz))
        if r < 0:
            raise ValueError(f"PCM rate {hz} unsupported (one of {PCM_RATES_ALL})")
        return r

    @property
    def pcm_rate(self) -> int:
        return self._L.rnnoise_batch_pcm_rate(self.h)

    @property
    def frame(self) -> int:
        """samples per stream and frame at the batch's PCM rate (480 at 48 kHz): the row length of every PCM array, also with a
        rate table (set_stream_rates), under which a stream fills only the first 480 * rate // 48000 samples of its row"""
        return FRAME * self.pcm_rate // 48000

    def set_pcm_layout(self, frame_stride: int = 0, row_stride: int = 0):
        """where the frames of the PCM buffers of every call lie (rnnoise_batch_set_pcm_layout): frame f of row r starts at sample
        f * frame_stride + r * row_stride of `in` and of `out` -- (frame, T * frame) for (N, T * frame) stream-contiguous buffers.
        (0, 0): the default (T, N, frame) layout.  Both strides positive multiples of 4 samples, else ValueError and nothing changes.
        With a layout the host calls (process, process_s16, process_masked*, process_list*) take (T, rows, frame) arrays whose
        strides ARE the layout's -- views of the caller's buffers, pcm_array() makes one -- and read and write them in place."""
        if self._L.rnnoise_batch_set_pcm_layout(self.h, int(frame_stride), int(row_stride)):
            raise ValueError(f"PCM layout ({frame_stride}, {row_stride}) unsupported (both 0, or both positive multiples of 4 samples)")

    @property
    def pcm_layout(self):
        """(frame_stride, row_stride) in samples; (0, 0): the default layout"""
        f, r = C.c_long(0), C.c_long(0)
        if self._L.rnnoise_batch_pcm_layout(self.h, C.byref(f), C.byref(r)):
            raise RuntimeError("rnnoise_batch_pcm_layout failed")
        return int(f.value), int(r.value)

    def set_pcm_channels(self, channels: int = 1) -> int:
        """interleaved channels (rnnoise_batch_set_pcm_channels): with C = channels > 1 the rows of every call are taken C at a time,
        row C * g + c being channel c of group g, its sample i at i * C + c of the group's slot -- stereo LRLR... is C = 2.  Returns the
        previous count; ValueError (nothing changes) unless 1 <= channels <= MAX_CHANNELS and channels divides the batch's streams.
        With C > 1 the host calls take and return (T, rows // C, frame, C) arrays; vad / gains / active stay (T, rows[, 32])."""
        r = self._L.rnnoise_batch_set_pcm_channels(self.h, int(channels))
        if r < 0:
            raise ValueError(f"{channels} PCM channels unsupported (1 .. {MAX_CHANNELS}, a divisor of the batch's {self.n} streams)")
        return r

    @property
    def pcm_channels(self) -> int:
        return self._L.rnnoise_batch_pcm_channels(self.h)

    def set_gain_link(self, k: int = 1) -> int:
        """linked gains (rnnoise_batch_set_gain_link): with k > 1 the rows of every call are taken k at a time and each group gets one
        suppression per frame -- per band the smallest raw gain of its non-silent present rows, and their largest VAD for the gate of
        the controls.  vad / gains returned stay each row's own.  Returns the previous count; ValueError (nothing changes) unless
        1 <= k <= MAX_CHANNELS and k divides the batch's streams.  Independent of set_pcm_channels: a stereo file sets both to 2."""
        r = self._L.rnnoise_batch_set_gain_link(self.h, int(k))
        if r < 0:
            raise ValueError(f"link count {k} unsupported (1 .. {MAX_CHANNELS}, a divisor of the batch's {self.n} streams)")
        return r

    @property
    def gain_link(self) -> int:
        return self._L.rnnoise_batch_gain_link(self.h)

    def pcm_array(self, n_frames: int, dtype=np.float32, rows: int | None = None, fill=0):
        """a (n_frames, rows, frame) view, in the batch's PCM layout, of a fresh buffer that spans its frame slots and is filled with
        `fill` (rows: the batch's streams, or the rows of a list call); with a layout set `.base` is the flat buffer.  With C > 1
        interleaved channels (set_pcm_channels): a (n_frames, rows // C, frame, C) view"""
        rows = self.n if rows is None else rows
        fs, rs = self.pcm_layout
        ch = self.pcm_channels
        if ch > 1:
            assert rows % ch == 0
            g, it = rows // ch, np.dtype(dtype).itemsize
            if not rs:
                return np.full((n_frames, g, self.frame, ch), fill, dtype)
            flat = np.full(max(n_frames - 1, 0) * fs + max(g - 1, 0) * rs + self.frame * ch, fill, dtype)
            return np.ndarray((n_frames, g, self.frame, ch), flat.dtype, flat, 0, (fs * it, rs * it, ch * it, it))
        if not rs:
            return np.full((n_frames, rows, self.frame), fill, dtype)
        flat = np.full(max(n_frames - 1, 0) * fs + max(rows - 1, 0) * rs + self.frame, fill, dtype)
        it = flat.itemsize
        return np.ndarray((n_frames, rows, self.frame), flat.dtype, flat, 0, (fs * it, rs * it, it))

    @staticmethod
    def _pcm_dims(pcm):
        """(T, rows, frame) of a PCM array: (T, rows, frame), or (T, groups, frame, C) with interleaved channels"""
        if pcm.ndim == 4:
            return pcm.shape[0], pcm.shape[1] * pcm.shape[3], pcm.shape[2]
        return pcm.shape

    def _pcm_in(self, pcm, dtype):
        """the PCM argument of a host call: a C-contiguous (T, rows, frame) array in the default layout (copied if need be); with a
        layout set, the caller's array as it lies -- its strides must be the layout's"""
        fs, rs = self.pcm_layout
        ch = self.pcm_channels
        if ch > 1 and not (np.ndim(pcm) == 4 and np.shape(pcm)[3] == ch):
            raise ValueError(f"with {ch} interleaved channels the call takes a (T, rows // {ch}, frame, {ch}) array")
        if not rs:
            return np.ascontiguousarray(pcm, dtype)
        it = np.dtype(dtype).itemsize
        if not (isinstance(pcm, np.ndarray) and pcm.dtype == dtype and pcm.ndim == (4 if ch > 1 else 3)):
            raise ValueError(f"with a PCM layout set the call takes a {np.dtype(dtype).name} array in that layout")
        want = (fs * it, rs * it, ch * it, it) if ch > 1 else (fs * it, rs * it, it)
        if any(n > 1 and st != w for n, st, w in zip(pcm.shape, pcm.strides, want)):
            raise ValueError(f"array strides {pcm.strides} are not the batch's PCM layout {want} (bytes)")
        return pcm

    def _pcm_out(self, out, pcm, dtype, zero=False):
        """the output array of a host call: given (checked like the input), or fresh -- in the batch's layout"""
        if out is not None:
            if self.pcm_layout[1]:
                out = self._pcm_in(out, dtype)
            assert out.dtype == dtype and out.shape == pcm.shape and (self.pcm_layout[1] or out.flags.c_contiguous)
            return out
        if self.pcm_layout[1]:
            return self.pcm_array(pcm.shape[0], dtype, self._pcm_dims(pcm)[1])  # (rows, not the groups of a channel array)
        return np.zeros_like(pcm) if zero else np.empty_like(pcm)

    def _call(self, fn, *args, exc=RuntimeError, why=""):
        """one call of the library on this batch that answers 0, or `exc`"""
        if getattr(self._L, fn)(self.h, *args):
            raise exc(f"{fn} failed{why}")

    def _call_s16(self, fn, s16, *args, why=""):
        """... of `fn` or, with s16, of its int16 twin; the RuntimeError names `fn` either way"""
        if getattr(self._L, fn + "_s16" if s16 else fn)(self.h, *args):
            raise RuntimeError(f"{fn} failed{why}")

    def _table_set(self, t, table):
        """the host setter of a per-stream table: `table` through t.encode, or None to drop a table that can be dropped"""
        fn = f"rnnoise_batch_set_stream_{t.stem}"
        if table is None and t.droppable:
            return self._call(fn, None)
        self._call(fn, t.encode(self, table).ctypes.data_as(C.POINTER(t.ctype)), exc=ValueError, why=t.why)

    def _table_set_device(self, t, d_table, stream):
        self._call(f"rnnoise_batch_set_stream_{t.stem}_device", d_table or None, stream or None)

    def _table_get(self, t):
        a = np.empty((self.n,) + t.row, t.ctype)
        self._call(f"rnnoise_batch_stream_{t.stem}", a.ctypes.data_as(C.POINTER(t.ctype)))
        return t.decode(a)

    def set_stream_rates(self, hz):
        """the PCM rate of every stream in Hz (rnnoise_batch_set_stream_rates): (N,) values out of PCM_RATES_ALL, none above the batch's
        own rate, or None to drop the table.  Synchronous; ValueError (and nothing changes) on any other value.  The streams whose
        rate changes restart their resampling filters from zero; every stream keeps its DenoiseState."""
        self._table_set(_RATES, hz)

    def set_stream_rates_device(self, d_rates: int, stream: int = 0):
        """the same from N bytes of device memory holding the rate CODES (rate_code: the divisors 1, 2, 3, 6, and RATE_32K), a copy ordered on
        `stream`; any other byte, or a rate above the batch's, reads as the batch's rate.  Histories are not touched: reset or load the streams whose
        rate changed (reset_streams_device / load_streams_device) on the same stream before their next frame."""
        self._table_set_device(_RATES, d_rates, stream)

    def stream_rates(self) -> np.ndarray:
        """the PCM rate of every stream in Hz, (N,) int32 (synchronous; the batch's rate everywhere without a table)"""
        return self._table_get(_RATES)

    def set_stream_formats(self, formats):
        """the PCM format of every stream's rows in the int16 calls (rnnoise_batch_set_stream_formats): (N,) names out of "s16",
        "ulaw", "alaw" or codes 0, 1, 2 (rnnoise_amd.g711), or None to drop the table.  A companded stream's G.711 bytes fill the
        first 480 * rate // 48000 BYTES of its int16 row.  Synchronous; ValueError (and nothing changes) on anything else."""
        self._table_set(_FORMATS, formats)

    def set_stream_formats_device(self, d_formats: int, stream: int = 0):
        """the same from N bytes of device memory holding the CODES (0 s16, 1 ulaw, 2 alaw), a copy ordered on `stream`; any other
        byte reads as s16.  Nothing else changes: a stream that changes codec mid-run is the caller's to reset."""
        self._table_set_device(_FORMATS, d_formats, stream)

    def stream_formats(self) -> np.ndarray:
        """the format code of every stream as the kernels read it, (N,) uint8 (synchronous; zeros without a table)"""
        return self._table_get(_FORMATS)

    def set_stream_out_rates(self, hz):
        """the rate every stream's OUTPUT rows are written at, in Hz (rnnoise_batch_set_stream_out_rates): (N,) values out of
        PCM_RATES_ALL, none above the batch's own rate, or None to drop the table (every stream then leaves at the rate it came in
        at).  A stream reads the first 480 * rate_in // 48000 samples of its `in` row and writes the first 480 * rate_out // 48000 of
        its `out` row.  Synchronous; ValueError (and nothing changes) on any other value.  The streams whose output rate changes
        restart their down-resampling filter from zero; every stream keeps its DenoiseState and its up-resampling filter."""
        self._table_set(_OUT_RATES, hz)

    def set_stream_out_rates_device(self, d_rates: int, stream: int = 0):
        """the same from N bytes of device memory holding the rate CODES, a copy ordered on `stream`; any other byte, or a rate above
        the batch's, reads as the batch's rate.  Histories are not touched (set_stream_rates_device)."""
        self._table_set_device(_OUT_RATES, d_rates, stream)

    def stream_out_rates(self) -> np.ndarray:
        """the rate every stream's output is written at in Hz, (N,) int32 (synchronous; stream_rates() without an out table)"""
        return self._table_get(_OUT_RATES)

    def set_stream_out_formats(self, formats):
        """the PCM format of every stream's OUTPUT rows in the int16 calls (rnnoise_batch_set_stream_out_formats): as
        set_stream_formats, which then describes the `in` rows alone; None drops the table (output format = input format)."""
        self._table_set(_OUT_FORMATS, formats)

    def set_stream_out_formats_device(self, d_formats: int, stream: int = 0):
        """the same from N bytes of device memory holding the CODES (0 s16, 1 ulaw, 2 alaw), a copy ordered on `stream`; any other
        byte reads as s16"""
        self._table_set_device(_OUT_FORMATS, d_formats, stream)

    def stream_out_formats(self) -> np.ndarray:
        """the format code of every stream's output rows as K3 reads it, (N,) uint8 (synchronous; stream_formats() without an out table)"""
        return self._table_get(_OUT_FORMATS)

    def process(self, pcm: np.ndarray, want_gains: bool = True, out: np.ndarray | None = None):
        """pcm: (T, N, frame) float32 host array -> (out, vad[T,N], gains[T,N,32]).  With a PCM layout set (set_pcm_layout) pcm and
        out are arrays with the layout's strides, used in place; out may be pcm itself."""
        return self._process("process", np.float32, pcm, want_gains, out)

    def process_s16(self, pcm: np.ndarray, want_gains: bool = True, out: np.ndarray | None = None):
        """pcm: (T, N, 480) int16 host array -> (out int16, vad[T,N], gains[T,N,32]): rnnoise_batch_process_s16, the
        conversions of examples/rnnoise_demo.c:56,58 done on the device."""
        return self._process("process_s16", np.int16, pcm, want_gains, out)

    def process_into(self, out_ptr: int, in_ptr: int, vad_ptr: int, gains_ptr: int, n_frames: int, s16: bool = False):
        """rnnoise_batch_process[_s16] on raw HOST pointers (ints).  Pinned memory (hipHostMalloc / torch pin_memory) is read
        and written by DMA in place; pageable memory goes through the library's pinned bounce buffers."""
        fp = C.POINTER(C.c_float)
        pp = C.POINTER(C.c_short) if s16 else fp
        self._call_s16("rnnoise_batch_process", s16, C.cast(out_ptr, pp), C.cast(in_ptr, pp), C.cast(vad_ptr or None, fp),
                       C.cast(gains_ptr or None, fp), n_frames)

    def process_device(self, d_out: int, d_in: int, d_vad: int, d_gains: int, n_frames: int, stream: int = 0, s16: bool = False):
        """Raw device pointers (ints), asynchronous on `stream` (a hipStream_t handle); s16: the PCM buffers hold int16."""
        self._call_s16("rnnoise_batch_process_device", s16, d_out, d_in, d_vad or None, d_gains or None, n_frames, stream or None)

    def _process(self, name, dtype, pcm, want_gains, out, masked=False, active=None, streams=None):
        """the host process calls: rnnoise_batch_<name> on PCM of `dtype`.  masked: the call takes `active` and leaves absent rows of
        `out` alone; streams: a list call, whose arrays have one row per listed stream"""
        pcm = self._pcm_in(pcm, dtype)
        T, R, F = self._pcm_dims(pcm)
        if streams is None:
            assert R == self.n and F == self.frame
            rows, exc, why = [], RuntimeError, ""
        else:
            streams = np.ascontiguousarray(np.asarray(streams).reshape(-1), np.int32)
            assert streams.size == R and F == self.frame
            rows, exc, why = [streams.ctypes.data_as(C.POINTER(C.c_int)), R], ValueError, " (a stream out of range or listed twice?)"
        active = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
        assert active is None or active.shape == (T, R)
        out = self._pcm_out(out, pcm, dtype, zero=masked)
        vad = np.empty((T, R), np.float32)
        gains = np.empty((T, R, NB_BANDS), np.float32) if want_gains else None
        ptr = C.POINTER(C.c_short if dtype == np.int16 else C.c_float)
        mask = [active.ctypes.data_as(C.POINTER(C.c_ubyte)) if active is not None else None] if masked else []
        self._call("rnnoise_batch_" + name, out.ctypes.data_as(ptr), pcm.ctypes.data_as(ptr), _fp(vad), _fp(gains), *rows, *mask, T,
                   exc=exc, why=why)
        return out, vad, gains

    def process_masked(self, pcm: np.ndarray, active, want_gains: bool = True, out: np.ndarray | None = None):
        """pcm: (T, N, 480) float32, active: (T, N) (nonzero = the stream has this frame; None = all) -> (out, vad[T,N],
        gains[T,N,32]): rnnoise_batch_process_masked.  Absent rows of `out` are not written: they keep what `out` held (zeros
        when it is not given)."""
        return self._process("process_masked", np.float32, pcm, want_gains, out, masked=True, active=active)

    def process_masked_s16(self, pcm: np.ndarray, active, want_gains: bool = True, out: np.ndarray | None = None):
        """process_masked on int16 PCM (rnnoise_batch_process_masked_s16)"""
        return self._process("process_masked_s16", np.int16, pcm, want_gains, out, masked=True, active=active)

    def process_masked_device(self, d_out: int, d_in: int, d_vad: int, d_gains: int, d_active: int, n_frames: int, stream: int = 0,
                              s16: bool = False):
        """Raw device pointers (ints), asynchronous on `stream`; d_active: [n_frames][N] bytes, 0 = every stream present."""
        self._call_s16("rnnoise_batch_process_device_masked", s16, d_out, d_in, d_vad or None, d_gains or None, d_active or None, n_frames,
                       stream or None)

    def _process_chunks(self, name, dtype, pcm, counts, want_gains, out, streams=None):
        """the host chunk calls: rnnoise_batch_<name> on PCM of `dtype`, one row per stream; streams: a list call, whose arrays have one
        row per listed stream"""
        ip = C.POINTER(C.c_int)
        if streams is None:
            R, rows, shape, listed = self.n, [], "chunk PCM is (n_streams, max_count)", ""
            why = " (a count outside [0, max_count], or a batch with a rate / format table, a PCM layout, channels or a gain link?)"
        else:
            idx = np.ascontiguousarray(np.asarray(streams).reshape(-1), np.int32)
            R, shape, listed = int(idx.size), "list chunk PCM is (n_rows, max_count)", "listed "
            rows = [idx.ctypes.data_as(ip), R]
            why = (" (a stream out of range or listed twice, a count outside [0, max_count], more rows than streams, or a batch"
                   " with a rate / format table, a PCM layout, channels or a gain link?)")
        pcm = np.asarray(pcm)
        if pcm.ndim != 2 or pcm.shape[0] != R:
            raise ValueError(f"{shape}; got {pcm.shape} for {R} {listed}streams")
        pcm = np.ascontiguousarray(pcm, dtype)
        max_count = pcm.shape[1]
        counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), np.int32)
        if counts.size != R:
            raise ValueError(f"one count per {listed}stream")
        if out is None:
            out = np.zeros_like(pcm)
        elif out.dtype != dtype or out.shape != pcm.shape or not out.flags.c_contiguous:
            raise ValueError("out: a C-contiguous array of the PCM's shape and type")
        F = chunk_frames(self.frame, max_count)
        vad = np.zeros((F, R), np.float32)
        gains = np.zeros((F, R, 32), np.float32) if want_gains else None
        frames = np.zeros(R, np.int32)
        pp = C.POINTER(C.c_short if dtype == np.int16 else C.c_float)
        self._call(f"rnnoise_batch_{name}", out.ctypes.data_as(pp), pcm.ctypes.data_as(pp), counts.ctypes.data_as(ip),
                   int(max_count), *rows, _fp(vad), _fp(gains), frames.ctypes.data_as(ip), exc=ValueError, why=why)
        return out, vad, gains, frames

    def process_chunks(self, pcm: np.ndarray, counts, want_gains: bool = True, out: np.ndarray | None = None):
        """Any number of samples per stream: pcm (N, max_count) float32, stream s pushes its first counts[s] samples -> (out, vad[F,N],
        gains[F,N,32], frames[N]): rnnoise_batch_process_chunks.  out[s, :counts[s]] is the stream's output, one frame late; the rest of
        the row keeps what `out` held (zeros when it is not given).  frames[s] rows of vad / gains belong to stream s."""
        return self._process_chunks("process_chunks", np.float32, pcm, counts, want_gains, out)

    def process_chunks_s16(self, pcm: np.ndarray, counts, want_gains: bool = True, out: np.ndarray | None = None):
        """process_chunks on int16 PCM (rnnoise_batch_process_chunks_s16)"""
        return self._process_chunks("process_chunks_s16", np.int16, pcm, counts, want_gains, out)

    def process_chunks_device(self, d_out: int, d_in: int, d_counts: int, max_count: int, d_vad: int = 0, d_gains: int = 0,
                              d_frames: int = 0, stream: int = 0, s16: bool = False):
        """Raw device pointers (ints), asynchronous on `stream`: d_in / d_out [N][max_count] float32 (int16 with s16), d_counts [N]
        int32 (clamped into [0, max_count]), d_vad [F][N], d_gains [F][N][32], d_frames [N] int32 or 0."""
        self._call_s16("rnnoise_batch_process_device_chunks", s16, d_out or None, d_in or None, d_counts or None, int(max_count),
                       d_vad or None, d_gains or None, d_frames or None, stream or None)

    def process_chunks_list(self, pcm: np.ndarray, counts, streams, want_gains: bool = True, out: np.ndarray | None = None):
        """process_chunks for the listed streams only: pcm (R, max_count) float32, row i belongs to stream streams[i] and pushes its
        first counts[i] samples -> (out, vad[F,R], gains[F,R,32], frames[R]): rnnoise_batch_process_chunks_list.  Unlisted streams
        are not touched.  ValueError, and nothing changes, on a stream out of range or listed twice or a count out of range."""
        return self._process_chunks("process_chunks_list", np.float32, pcm, counts, want_gains, out, streams)

    def process_chunks_list_s16(self, pcm: np.ndarray, counts, streams, want_gains: bool = True, out: np.ndarray | None = None):
        """process_chunks_list on int16 PCM (rnnoise_batch_process_chunks_list_s16)"""
        return self._process_chunks("process_chunks_list_s16", np.int16, pcm, counts, want_gains, out, streams)

    def process_chunks_list_device(self, d_out: int, d_in: int, d_counts: int, max_count: int, d_streams: int, n_rows: int,
                                   d_vad: int = 0, d_gains: int = 0, d_frames: int = 0, stream: int = 0, s16: bool = False):
        """Raw device pointers (ints), asynchronous on `stream`: d_in / d_out [R][max_count] float32 (int16 with s16), d_counts [R]
        int32 (clamped into [0, max_count]), d_streams [R] int32 (an entry out of range: an absent row), d_vad [F][R],
        d_gains [F][R][32], d_frames [R] int32 or 0."""
        self._call_s16("rnnoise_batch_process_device_chunks_list", s16, d_out or None, d_in or None, d_counts or None, int(max_count),
                       d_streams or None, int(n_rows), d_vad or None, d_gains or None, d_frames or None, stream or None)

    def save_chunk_fifos(self, streams=None) -> np.ndarray:
        """the FIFO records of the listed streams (None: the whole batch), (n, CHUNK_REC_FLOATS) float32: pending samples, output FIFO,
        then r, M and the magic word (view as int32) -- rnnoise_batch_save_chunk_fifos.  Synchronous; the batch is unchanged."""
        return self._records("rnnoise_batch_save_chunk_fifos", CHUNK_REC_FLOATS, streams)

    def load_chunk_fifos(self, rec: np.ndarray, streams=None):
        """row i of rec (n, CHUNK_REC_FLOATS) becomes the FIFOs of stream streams[i]: rnnoise_batch_load_chunk_fifos -- AFTER
        load_streams, which restarts them.  Synchronous.  ValueError, and nothing changes, on an out-of-range or repeated stream or
        a record with another magic word, another frame length or a fill outside [0, M)."""
        self._records("rnnoise_batch_load_chunk_fifos", CHUNK_REC_FLOATS, streams, rec)

    def save_chunk_fifos_device(self, d_rec: int, d_streams: int, n: int, stream: int = 0):
        """Raw device pointers (ints), asynchronous on `stream`: d_rec [n][CHUNK_REC_FLOATS] float32, d_streams [n] int32 or 0 with
        n == N.  A row whose entry is out of range gets magic word 0."""
        self._call("rnnoise_batch_save_chunk_fifos_device", d_rec or None, d_streams or None, n, stream or None)

    def load_chunk_fifos_device(self, d_rec: int, d_streams: int, n: int, stream: int = 0):
        """the inverse, asynchronous on `stream`: rows that are not records of this frame length and out-of-range entries touch nothing"""
        self._call("rnnoise_batch_load_chunk_fifos_device", d_rec or None, d_streams or None, n, stream or None)

    def chunk_fill(self) -> np.ndarray:
        """the pending input samples r_s of every stream, (N,) int32 (rnnoise_batch_chunk_fill; synchronous)"""
        fill = np.zeros(self.n, np.int32)
        self._call("rnnoise_batch_chunk_fill", fill.ctypes.data_as(C.POINTER(C.c_int)))
        return fill

    def process_list(self, pcm: np.ndarray, streams, active=None, want_gains: bool = True, out: np.ndarray | None = None):
        """Advance only the listed streams: pcm (T, R, 480 / L) float32, row i of every frame belongs to stream streams[i]; active:
        (T, R) or None -> (out, vad[T,R], gains[T,R,32]): rnnoise_batch_process_list.  Absent rows of `out` keep what `out` held
        (zeros when it is not given).  ValueError on an out-of-range or repeated stream (nothing changes then)."""
        return self._process("process_list", np.float32, pcm, want_gains, out, masked=True, active=active, streams=streams)

    def process_list_s16(self, pcm: np.ndarray, streams, active=None, want_gains: bool = True, out: np.ndarray | None = None):
        """process_list on int16 PCM (rnnoise_batch_process_list_s16)"""
        return self._process("process_list_s16", np.int16, pcm, want_gains, out, masked=True, active=active, streams=streams)

    def process_list_device(self, d_out: int, d_in: int, d_vad: int, d_gains: int, d_streams: int, n_rows: int, d_active: int,
                            n_frames: int, stream: int = 0, s16: bool = False):
        """Raw device pointers (ints), asynchronous on `stream`: d_streams [n_rows] int32; buffers of n_rows rows per frame;
        d_active [n_frames][n_rows] bytes, 0 = every listed stream present.  Out-of-range entries are absent rows."""
        self._call_s16("rnnoise_batch_process_device_list", s16, d_out, d_in, d_vad or None, d_gains or None, d_streams or None, n_rows,
                       d_active or None, n_frames, stream or None)

    def reset_streams(self, indices):
        """the listed streams back to rnnoise_init()'s state (synchronous; ValueError on an index out of range)"""
        idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), np.int32)
        if self._L.rnnoise_batch_reset_streams(self.h, idx.ctypes.data_as(C.POINTER(C.c_int)), int(idx.size)):
            raise ValueError("rnnoise_batch_reset_streams failed (stream index out of range?)")

    def reset_streams_device(self, d_streams: int, n: int, stream: int = 0):
        """the same from an int32 device list, asynchronous on `stream` (out-of-range entries ignored)"""
        if self._L.rnnoise_batch_reset_streams_device(self.h, d_streams or None, n, stream or None):
            raise RuntimeError("rnnoise_batch_reset_streams_device failed")

    def add_model(self, model: Model) -> int:
        """puts `model` into the batch's next model slot (rnnoise_batch_add_model) and returns the slot (1 .. MAX_MODELS - 1); every
        stream stays where it is.  The batch keeps a reference: the model outlives it."""
        k = self._L.rnnoise_batch_add_model(self.h, model.h if model is not None else None)
        if k < 0:
            raise RuntimeError("rnnoise_batch_add_model failed (table full, or the model cannot go on this device)")
        self.extra_models.append(model)
        return k

    def set_stream_models(self, models):
        """the model slot of every stream: (N,) integers (synchronous; ValueError if an entry names no slot -- nothing changes then)"""
        self._table_set(_MODELS, models)

    def set_stream_models_device(self, d_models: int, stream: int = 0):
        """the same from N bytes of device memory, a copy ordered on `stream` (entries naming no slot read as slot 0)"""
        self._table_set_device(_MODELS, d_models, stream)

    def stream_models(self) -> np.ndarray:
        """the model slot of every stream, (N,) uint8 (synchronous)"""
        return self._table_get(_MODELS)

    def set_stream_controls(self, ctl):
        """per-stream suppression controls (rnnoise_batch_set_stream_controls): (N, 3) float32 rows {floor, thr, hold} -- floor a
        linear gain floor in [0, 1], thr a VAD gate threshold in [0, 1] (0: no gate), hold whole frames in [0, 65535] -- or None to
        drop the table.  Synchronous; ValueError (and nothing changes) on a non-finite, out-of-range or fractional entry."""
        self._table_set(_CONTROLS, ctl)

    def set_stream_controls_device(self, d_ctl: int, stream: int = 0):
        """the same from N x 3 floats of device memory, a copy ordered on `stream` (the kernel maps NaN to 0, clamps, truncates hold)"""
        self._table_set_device(_CONTROLS, d_ctl, stream)

    def stream_controls(self) -> np.ndarray:
        """the control table, (N, 3) float32 (zeros when there is none; synchronous)"""
        return self._table_get(_CONTROLS)

    def export_state(self, stream: int) -> np.ndarray:
        s = np.empty(STATE_FLOATS, np.float32)
        if self._L.rnnoise_batch_export_state(self.h, stream, _fp(s)):
            raise RuntimeError("export_state failed")
        return s

    def import_state(self, stream: int, state: np.ndarray):
        state = np.ascontiguousarray(state, np.float32)
        if self._L.rnnoise_batch_import_state(self.h, stream, _fp(state)):
            raise RuntimeError("import_state failed")

    def _records(self, fn, width, streams, rec=None):
        """save (rec None: a fresh array) or load of the (n, width) float32 records of the listed streams (None: the whole batch),
        through the host call `fn`"""
        idx, n = None, self.n
        if streams is not None:
            idx = np.ascontiguousarray(np.asarray(streams).reshape(-1), np.int32)
            n = int(idx.size)
        if rec is None:
            rec, why = np.empty((n, width), np.float32), " (a stream out of range, or too many rows?)"
        else:
            rec, why = np.ascontiguousarray(rec, np.float32), " (a stream out of range or listed twice, or a bad record?)"
            assert rec.shape == (n, width), rec.shape
        self._call(fn, _fp(rec), idx.ctypes.data_as(C.POINTER(C.c_int)) if idx is not None else None, n, exc=ValueError, why=why)
        return rec

    def save_streams(self, streams=None) -> np.ndarray:
        """complete snapshots of the listed streams (None: the whole batch, row i = stream i), (n, SNAP_FLOATS) float32:
        rnnoise_batch_save_streams.  Row i's first STATE_FLOATS words are export_state(streams[i]); then the header (view as int32)
        and the resampler history.  Synchronous; the batch is unchanged.  ValueError on an index out of range."""
        return self._records("rnnoise_batch_save_streams", SNAP_FLOATS, streams)

    def load_streams(self, snap: np.ndarray, streams=None):
        """row i of snap (n, SNAP_FLOATS) becomes the state of stream streams[i] (None: the whole batch): rnnoise_batch_load_streams.
        Synchronous.  ValueError, and nothing changes, on an out-of-range or repeated stream, a record without the magic word or one
        whose analysis_mem is not the tail of its pitch_buf."""
        self._records("rnnoise_batch_load_streams", SNAP_FLOATS, streams, snap)

    def save_streams_device(self, d_snap: int, d_streams: int, n: int, stream: int = 0):
        """Raw device pointers (ints), asynchronous on `stream`: d_snap [n][SNAP_FLOATS] float32 (16-byte aligned), d_streams [n] int32 or
        0 with n == N for the whole batch.  A row whose entry is out of range gets an empty record (magic word 0)."""
        self._call("rnnoise_batch_save_streams_device", d_snap or None, d_streams or None, n, stream or None)

    def load_streams_device(self, d_snap: int, d_streams: int, n: int, stream: int = 0):
        """the inverse, asynchronous on `stream`: rows without the magic word and out-of-range entries touch nothing"""
        self._call("rnnoise_batch_load_streams_device", d_snap or None, d_streams or None, n, stream or None)

    def debug_last(self):
        f = np.empty((self.n, NB_FEATURES), np.float32)
        s = np.empty(self.n, np.int32)
        p = np.empty(self.n, np.int32)
        ip = C.POINTER(C.c_int)
        if self._L.rnnoise_batch_debug_last(self.h, _fp(f), s.ctypes.data_as(ip), p.ctypes.data_as(ip)):
            raise RuntimeError("debug_last failed")
        return f, s, p

    def train_features(self, clean, noisy, vad, lowpass, band_lp, noise_free):
        """clean/noisy: (T, N, 480); vad: (T, N); lowpass/band_lp/noise_free: (N,) ints -> records (T, N, 98)."""
        clean = np.ascontiguousarray(clean, np.float32)
        noisy = np.ascontiguousarray(noisy, np.float32)
        vad = np.ascontiguousarray(vad, np.float32)
        T, N, _ = clean.shape
        ia = [np.ascontiguousarray(a, np.int32) for a in (lowpass, band_lp, noise_free)]
        rec = np.empty((T, N, 98), np.float32)
        ip = C.POINTER(C.c_int)
        if self._L.rnnoise_batch_train_features(self.h, _fp(rec), _fp(clean), _fp(noisy), _fp(vad),
                                              *[a.ctypes.data_as(ip) for a in ia], T):
            raise RuntimeError("rnnoise_batch_train_features failed")
        return rec

    def train_levels_device(self, d_energy: int, d_rms: int, d_corpora, lens, mix, n_frames: int, stream: int = 0):
        """Raw device pointers (ints), asynchronous on `stream`: d_energy [N][n_frames] and d_rms [N][3] float32 out; d_corpora: the
        speech, noise and foreground-noise corpora (int16), lens their lengths in samples; mix: a host table of N MIX_DTYPE records."""
        mix = _mix_table(mix)
        assert len(mix) == self.n, (len(mix), self.n)
        if self._L.rnnoise_batch_train_levels_device(self.h, d_energy or None, d_rms or None, *[p or None for p in d_corpora],
                                                     *[int(v) for v in lens], mix.ctypes.data, n_frames, stream or None):
            raise RuntimeError("rnnoise_batch_train_levels_device failed (a sequence outside its corpus, a non-finite gain?)")

    def train_levels_vad_device(self, d_energy: int, d_rms: int, d_vad: int, d_corpora, lens, mix, start_pos, n_frames: int,
                                stream: int = 0):
        """train_levels_device and, in the same launch, d_vad [N][n_frames] uint8 out: what train_vad(energy, start_pos) gives on
        those energies, byte for byte (rnnoise_batch_train_levels_vad_device).  start_pos: N ints on the host, or None.  Only where
        train_vad_device_available() says so."""
        mix = _mix_table(mix)
        assert len(mix) == self.n, (len(mix), self.n)
        sp = None
        if start_pos is not None:
            sp = np.ascontiguousarray(start_pos, np.int32)
            assert sp.shape == (self.n,), (sp.shape, self.n)
        if self._L.rnnoise_batch_train_levels_vad_device(self.h, d_energy or None, d_rms or None, d_vad or None,
                                                         *[p or None for p in d_corpora], *[int(v) for v in lens], mix.ctypes.data,
                                                         sp.ctypes.data_as(C.POINTER(C.c_int)) if sp is not None else None, n_frames,
                                                         stream or None):
            raise RuntimeError("rnnoise_batch_train_levels_vad_device failed (a sequence outside its corpus, a non-finite gain, a host "
                               "whose libm is not the restated one: train_vad_device_available()?)")

    def train_mix_device(self, d_clean: int, d_noisy: int, d_vad_target: int, d_noise_free: int, d_corpora, lens, mix, d_rms: int,
                         d_vad: int, n_frames: int, stream: int = 0):
        """Raw device pointers (ints), asynchronous on `stream`: d_clean, d_noisy [n_frames][N][480] float32, d_vad_target
        [n_frames][N] float32 and d_noise_free [N] int32 out -- the layouts rnnoise_batch_train_features_device takes; d_rms [N][3]
        from train_levels_device, d_vad [N][n_frames] uint8 from train_vad."""
        mix = _mix_table(mix)
        assert len(mix) == self.n, (len(mix), self.n)
        if self._L.rnnoise_batch_train_mix_device(self.h, d_clean or None, d_noisy or None, d_vad_target or None, d_noise_free or None,
                                                  *[p or None for p in d_corpora], *[int(v) for v in lens], mix.ctypes.data,
                                                  d_rms or None, d_vad or None, n_frames, stream or None):
            raise RuntimeError("rnnoise_batch_train_mix_device failed (a sequence outside its corpus, a non-finite gain?)")

    def train_rir_load_device(self, d_spectra: int, d_rir: int, lens, stream: int = 0):
        """Raw device pointers (ints), asynchronous on `stream`: d_rir [len(lens)][RIR_MAX] float32, of which the first lens[r] samples
        count -> d_spectra [len(lens)][2][RIR_FFT][2] float32, the whole and the early response of each (load_rir)."""
        lens = np.ascontiguousarray(lens, np.int32)
        assert lens.ndim == 1, lens.shape
        if self._L.rnnoise_batch_train_rir_load_device(self.h, d_spectra or None, d_rir or None, lens.ctypes.data_as(C.POINTER(C.c_int)),
                                                       len(lens), stream or None):
            raise RuntimeError("rnnoise_batch_train_rir_load_device failed (a length outside [1, 32768]?)")

    def train_rir_device(self, d_clean: int, d_noisy: int, d_spectra: int, n_rirs: int, rir, d_work: int, work_bytes: int,
                         n_frames: int, stream: int = 0):
        """Raw device pointers (ints), asynchronous on `stream`: filters d_clean and d_noisy [n_frames][N][480] float32 in place with
        the spectra train_rir_load_device made, then clips and quantises d_noisy; rir: a host table of N RIR_DTYPE records; d_work:
        work_bytes of scratch (train_rir_work_bytes)."""
        rir = _rir_table(rir)
        assert len(rir) == self.n, (len(rir), self.n)
        if self._L.rnnoise_batch_train_rir_device(self.h, d_clean or None, d_noisy or None, d_spectra or None, int(n_rirs),
                                                  rir.ctypes.data, d_work or None, int(work_bytes), n_frames, stream or None):
            raise RuntimeError("rnnoise_batch_train_rir_device failed (a rir_id outside the list, a workspace below one unit?)")

    def train_features_device(self, d_records: int, d_clean: int, d_noisy: int, d_vad: int, d_lowpass: int, d_band_lp: int,
                              d_noise_free: int, n_frames: int, stream: int = 0):
        """rnnoise_batch_train_features_device on raw device pointers (ints), asynchronous on `stream`"""
        if self._L.rnnoise_batch_train_features_device(self.h, d_records or None, d_clean or None, d_noisy or None, d_vad or None,
                                                       d_lowpass or None, d_band_lp or None, d_noise_free or None, n_frames,
                                                       stream or None):
            raise RuntimeError("rnnoise_batch_train_features_device failed")

    @staticmethod
    def _rows_in(rows, row_floats, layout):
        """a host array of rows for the feature calls -> (array, frame_stride, row_stride, n_frames): layout "frame" is (T, N, >=
        row_floats) and "stream" (N, T, >= row_floats), read where they lie -- the last axis may be longer than the row (records as
        features, a padded pitch)"""
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.ndim == 3 and rows.shape[2] >= row_floats and layout in ("frame", "stream"), (rows.shape, layout)
        a, bb, w = rows.shape
        return (rows, bb * w, w, a) if layout == "frame" else (rows, w, bb * w, bb)

    def process_features(self, features, want_gains: bool = True, layout: str = "frame"):
        """rnnoise_batch_process_features: the network alone on features (T, N, >= 65) (layout "stream": (N, T, >= 65)) ->
        (vad (T, N), gains (T, N, 32) or None)"""
        x, fs, rs, T = self._rows_in(features, NB_FEATURES, layout)
        assert x.shape[1 if layout == "frame" else 0] == self.n, (x.shape, self.n)
        vad = np.empty((T, self.n), np.float32)
        gains = np.empty((T, self.n, NB_BANDS), np.float32) if want_gains else None
        if self._L.rnnoise_batch_process_features(self.h, _fp(gains), _fp(vad), _fp(x), fs, rs, T):
            raise RuntimeError("rnnoise_batch_process_features failed")
        return vad, gains

    def process_features_device(self, d_gains: int, d_vad: int, d_features: int, n_frames: int, frame_stride: int = 0,
                                row_stride: int = 0, stream: int = 0):
        """rnnoise_batch_process_features_device on raw device pointers (ints), asynchronous on `stream`"""
        if self._L.rnnoise_batch_process_features_device(self.h, d_gains or None, d_vad or None, d_features or None, int(frame_stride),
                                                         int(row_stride), n_frames, stream or None):
            raise RuntimeError("rnnoise_batch_process_features_device failed (overlapping slots?)")

    # ---- split calls (include/rnnoise_amd.h: rnnoise_batch_analyze, rnnoise_batch_synthesize) ----
    @property
    def split_pending(self) -> int:
        """rnnoise_batch_split_pending: frames analysed and not yet synthesised"""
        return self._L.rnnoise_batch_split_pending(self.h)

    def split_reserve(self, max_frames: int):
        """rnnoise_batch_split_reserve: room for max_frames pending frames (split_frame_bytes(n) each); synchronous"""
        self._call("rnnoise_batch_split_reserve", int(max_frames), why=" (frames pending?)")

    def analyze(self, pcm, layout: str = "frame", s16: bool = False):
        """rnnoise_batch_analyze[_s16]: pcm as Batch.process[_s16] takes it -> (features, silence (T, N) int32); features is
        (T, N, 65), or with layout "stream" the trainer's batch-first (N, T, 65).  The T frames stay pending until synthesize."""
        dtype = np.int16 if s16 else np.float32
        pcm = self._pcm_in(pcm, dtype)
        T, R, F = self._pcm_dims(pcm)
        assert R == self.n and F == self.frame and layout in ("frame", "stream"), (pcm.shape, layout)
        feats = np.empty((T, R, FEATURES) if layout == "frame" else (R, T, FEATURES), np.float32)
        _keep, rows = _rows_arg(None if layout == "frame" else (FEATURES, T * FEATURES))
        sil = np.empty((T, R), np.int32)
        ptr = C.POINTER(C.c_short if s16 else C.c_float)
        self._call("rnnoise_batch_analyze_s16" if s16 else "rnnoise_batch_analyze", _fp(feats), rows,
                   sil.ctypes.data_as(C.POINTER(C.c_int)), pcm.ctypes.data_as(ptr), T, why=" (frames pending, or per-stream frame phase?)")
        return feats, sil

    def synthesize(self, gains, vad, layout: str = "frame", s16: bool = False, out: np.ndarray | None = None):
        """rnnoise_batch_synthesize[_s16]: gains (T, N, >= 32) and vad (T, N) or (T, N, >= 1) for the pending frames (layout "stream":
        (N, T, ...)), read where they lie -> out, the PCM as Batch.process[_s16] returns it"""
        dtype = np.int16 if s16 else np.float32
        g, gfs, grs, T = self._rows_in(gains, NB_BANDS, layout)
        v = np.ascontiguousarray(vad, np.float32)
        v, vfs, vrs, Tv = self._rows_in(v[..., None] if v.ndim == 2 else v, 1, layout)
        assert T == Tv and g.shape[1 if layout == "frame" else 0] == self.n and v.shape[:2] == g.shape[:2], (g.shape, v.shape)
        ch = self.pcm_channels
        shape = (T, self.n // ch, self.frame, ch) if ch > 1 else (T, self.n, self.frame)
        if out is None:
            out = self.pcm_array(T, dtype)
        elif self.pcm_layout[1]:
            out = self._pcm_in(out, dtype)
        assert out.dtype == dtype and out.shape == shape and (self.pcm_layout[1] or out.flags.c_contiguous), (out.shape, shape)
        kg, grows = _rows_arg((gfs, grs))
        kv, vrows = _rows_arg((vfs, vrs))
        ptr = C.POINTER(C.c_short if s16 else C.c_float)
        self._call("rnnoise_batch_synthesize_s16" if s16 else "rnnoise_batch_synthesize", out.ctypes.data_as(ptr), _fp(g), grows, _fp(v),
                   vrows, T, why=" (n_frames != split_pending, or overlapping rows?)")
        return out

    def analyze_device(self, d_features: int, d_silence: int, d_in: int, n_frames: int, feat_rows=None, stream: int = 0,
                       s16: bool = False):
        """rnnoise_batch_analyze_device[_s16] on raw device pointers (ints), asynchronous on `stream`; feat_rows: None, Rows or a
        (frame_stride, row_stride) pair"""
        _keep, rows = _rows_arg(feat_rows)
        self._call_s16("rnnoise_batch_analyze_device", s16, d_features or None, rows, d_silence or None, d_in or None, n_frames,
                       stream or None, why=" (frames pending, per-stream frame phase, overlapping rows?)")

    def synthesize_device(self, d_out: int, d_gains: int, d_vad: int, n_frames: int, gain_rows=None, vad_rows=None, stream: int = 0,
                          s16: bool = False):
        """rnnoise_batch_synthesize_device[_s16] on raw device pointers (ints), asynchronous on `stream`"""
        _kg, grows = _rows_arg(gain_rows)
        _kv, vrows = _rows_arg(vad_rows)
        self._call_s16("rnnoise_batch_synthesize_device", s16, d_out or None, d_gains or None, grows, d_vad or None, vrows, n_frames,
                       stream or None, why=" (n_frames != split_pending, overlapping rows?)")

    def eval_records(self, records, t0: int = 0, n_frames: int | None = None, sums=None, gamma=None, first=None,
                     want_gains: bool = True, want_vad: bool = True, layout: str = "frame"):
        """rnnoise_batch_eval_records: records (T, N, >= 98) from record 0 on (layout "stream": (N, T, >= 98)), frames t0 .. t0 +
        n_frames - 1 (default: to the end) -> (sums (N, EVAL_SUMS) float64, vad (n_frames, N) or None, gains (n_frames, N, 32) or
        None).  sums: an (N, EVAL_SUMS) float64 array that is added to in place, or None for a zeroed one."""
        x, fs, rs, T = self._rows_in(records, REC, layout)
        assert x.shape[1 if layout == "frame" else 0] == self.n, (x.shape, self.n)
        n_frames = T - t0 if n_frames is None else n_frames
        assert 0 <= t0 and 0 <= n_frames and t0 + n_frames <= T, (t0, n_frames, T)
        if sums is None:
            sums = np.zeros((self.n, EVAL_SUMS), np.float64)
        assert sums.dtype == np.float64 and sums.shape == (self.n, EVAL_SUMS) and sums.flags.c_contiguous
        vad = np.empty((n_frames, self.n), np.float32) if want_vad else None
        gains = np.empty((n_frames, self.n, NB_BANDS), np.float32) if want_gains else None
        cfg = _eval_cfg(gamma, first)
        if self._L.rnnoise_batch_eval_records(self.h, sums.ctypes.data_as(C.POINTER(C.c_double)), _fp(gains), _fp(vad), _fp(x), fs, rs,
                                              t0, n_frames, C.byref(cfg) if cfg is not None else None):
            raise RuntimeError("rnnoise_batch_eval_records failed (gamma, first, overlapping slots?)")
        return sums, vad, gains

    def eval_records_device(self, d_sums: int, d_gains: int, d_vad: int, d_records: int, t0: int, n_frames: int,
                            frame_stride: int = 0, row_stride: int = 0, gamma=None, first=None, stream: int = 0):
        """rnnoise_batch_eval_records_device on raw device pointers (ints), asynchronous on `stream`; d_sums [N][EVAL_SUMS] float64 is
        added to"""
        cfg = _eval_cfg(gamma, first)
        if self._L.rnnoise_batch_eval_records_device(self.h, d_sums or None, d_gains or None, d_vad or None, d_records or None,
                                                     int(frame_stride), int(row_stride), t0, n_frames,
                                                     C.byref(cfg) if cfg is not None else None, stream or None):
            raise RuntimeError("rnnoise_batch_eval_records_device failed (gamma, first, overlapping slots?)")

    def score_records(self, records, gains, vad, t0: int = 0, sums=None, band_sums=None, gamma=None, first=None,
                      want_bands: bool = True, layout: str = "frame"):
        """rnnoise_batch_score_records: the trainer's loss on predictions of the caller's.  records (T, R, >= 98) from record 0 on,
        gains (n_frames, R, >= 32) and vad (n_frames, R) or (n_frames, R, >= 1) for steps t0 .. t0 + n_frames - 1 (layout "stream":
        (R, T, ...) each), read where they lie; R is free of the batch's size -> (sums (R, EVAL_SUMS) float64, band_sums (R, 32)
        float64 or None).  sums / band_sums: arrays that are added to in place, or None for zeroed ones."""
        x, rfs, rrs, T = self._rows_in(records, REC, layout)
        g, gfs, grs, n_frames = self._rows_in(gains, NB_BANDS, layout)
        v = np.ascontiguousarray(vad, np.float32)
        v, vfs, vrs, Tv = self._rows_in(v[..., None] if v.ndim == 2 else v, 1, layout)
        R = x.shape[1 if layout == "frame" else 0]
        assert n_frames == Tv and g.shape[:2] == v.shape[:2] and g.shape[1 if layout == "frame" else 0] == R, (x.shape, g.shape, v.shape)
        assert 0 <= t0 and t0 + n_frames <= T, (t0, n_frames, T)
        if sums is None:
            sums = np.zeros((R, EVAL_SUMS), np.float64)
        if band_sums is None and want_bands:
            band_sums = np.zeros((R, NB_BANDS), np.float64)
        assert sums.dtype == np.float64 and sums.shape == (R, EVAL_SUMS) and sums.flags.c_contiguous
        assert band_sums is None or (band_sums.dtype == np.float64 and band_sums.shape == (R, NB_BANDS) and band_sums.flags.c_contiguous)
        cfg = _eval_cfg(gamma, first)
        dp = C.POINTER(C.c_double)
        if self._L.rnnoise_batch_score_records(self.h, sums.ctypes.data_as(dp), band_sums.ctypes.data_as(dp) if band_sums is not None else None,
                                               _fp(g), gfs, grs, _fp(v), vfs, vrs, _fp(x), rfs, rrs, R, t0, n_frames,
                                               C.byref(cfg) if cfg is not None else None):
            raise RuntimeError("rnnoise_batch_score_records failed (gamma, first, overlapping slots?)")
        return sums, band_sums

    def score_records_device(self, d_sums: int, d_band_sums: int, d_gains: int, d_vad: int, d_records: int, n_rows: int, t0: int,
                             n_frames: int, gain_strides=(0, 0), vad_strides=(0, 0), rec_strides=(0, 0), gamma=None, first=None,
                             stream: int = 0):
        """rnnoise_batch_score_records_device on raw device pointers (ints), asynchronous on `stream`, one launch; d_sums
        [n_rows][EVAL_SUMS] and d_band_sums [n_rows][32] (or 0) float64 are added to; strides are (frame_stride, row_stride) pairs"""
        cfg = _eval_cfg(gamma, first)
        if self._L.rnnoise_batch_score_records_device(self.h, d_sums or None, d_band_sums or None, d_gains or None, int(gain_strides[0]),
                                                      int(gain_strides[1]), d_vad or None, int(vad_strides[0]), int(vad_strides[1]),
                                                      d_records or None, int(rec_strides[0]), int(rec_strides[1]), int(n_rows), int(t0),
                                                      int(n_frames), C.byref(cfg) if cfg is not None else None, stream or None):
            raise RuntimeError("rnnoise_batch_score_records_device failed (gamma, first, overlapping slots?)")

    def debug_pitch(self, arm_only: bool = False):
        if arm_only:
            self._L.rnnoise_batch_debug_pitch(self.h, None)
            return None
        d = np.empty((self.n, 1400), np.float32)
        if self._L.rnnoise_batch_debug_pitch(self.h, _fp(d)):
            raise RuntimeError("debug_pitch failed")
        return d

    def enable_timing(self, on: bool = True):
        self._L.rnnoise_batch_enable_timing(self.h, int(on))

    def kernel_ms(self):
        ms = (C.c_double * 4)()
        n = C.c_long(0)
        if self._L.rnnoise_batch_kernel_ms(self.h, ms, C.byref(n)):
            raise RuntimeError("kernel_ms failed")
        return dict(analysis=ms[0], network=ms[1], synthesis=ms[2], highpass=ms[3], launches=n.value)


class DenoiseState:
    """The reference's one-stream object (rnnoise_create / process_frame / destroy)."""

    def __init__(self, model: Model):
        self._L = lib()  # the library image that owns this handle (capi.instrumented() swaps the global one)
        self.model = model
        self.h = self._L.rnnoise_create(model.h)
        if not self.h:
            raise RuntimeError("rnnoise_create failed")

    def process_frame(self, frame: np.ndarray):
        x = np.ascontiguousarray(frame, np.float32).copy()
        vad = self._L.rnnoise_process_frame(self.h, _fp(x), _fp(x))  # in place, like rnnoise_demo.c:57
        return x, vad

    def close(self):
        if getattr(self, "h", None):
            self._L.rnnoise_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            _close_quietly(self)
        except Exception:  # (at interpreter shutdown the helper itself may already be gone)
            pass
