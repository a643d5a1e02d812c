"""PyTorch-ROCm binding of the batched op: forward only, tensors in, tensors out,
on torch's current stream; plus an un-quantised float re-statement of the network built from the
same blob for sanity cross-checks (not bit parity: exact tanh/sigmoid, no 8-bit activations), the
role torch/rnnoise/rnnoise.py:86-109 plays in the reference's training stack.

torch is plumbing here (HBM buffers, streams); the arithmetic runs in librnnoise_amd.so.
"""
from __future__ import annotations

import weakref

import numpy as np

from . import blob as rblob
from . import capi


# handle -> RNNoiseOp: what torch.ops.rnnoise_amd.process resolves its integer argument to.  Weak: an op nobody holds any
# more is closed by its destructor (it owns a GPU arena and a model), not kept alive by this table.
_OPS = weakref.WeakValueDictionary()
_registered = False


def register_torch_op():
    """Registers `torch.ops.rnnoise_amd.process(pcm, state, handle) -> (out, vad, gains)` (torch.library custom op, forward
    only).  `handle` is RNNoiseOp.handle: the op is stateful per stream batch, like the C API it binds, and the stream state
    lives in the library, not in tensors.  So that tracing / functionalization / torch.compile cannot treat it as a pure
    function -- merge two calls with the same arguments, or drop one whose outputs are unused, and silently desynchronise the
    streams -- the op MUTATES its `state` argument (RNNoiseOp.state: the batch's frame counter, a one-element int64 tensor,
    advanced by the number of frames of every call).  A fake (meta) implementation gives shapes."""
    global _registered
    if _registered:
        return
    import torch

    def fake_outs(pcm, F, R, dtype=torch.float32, frames=False):
        """the outputs of a process op's fake: PCM like pcm, vad (F, R), gains (F, R, 32) and, in the chunk forms, frames (R,)"""
        res = torch.empty_like(pcm), pcm.new_empty((F, R), dtype=dtype), pcm.new_empty((F, R, capi.NB_BANDS), dtype=dtype)
        return res + (pcm.new_empty((R,), dtype=torch.int32),) if frames else res

    # (explicit schema: this module uses postponed annotations, which infer_schema cannot resolve for a local import)
    @torch.library.custom_op("rnnoise_amd::process", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)")
    def process(pcm, state, handle):
        res = _OPS[handle]._run(pcm)
        state.add_(pcm.shape[0])
        return res

    @process.register_fake
    def _(pcm, state, handle):
        return fake_outs(pcm, pcm.shape[0], pcm.shape[1], pcm.dtype)

    # the masked form (include/rnnoise_amd.h: rnnoise_batch_process_device_masked): active (T, N) bool / uint8, nonzero = the stream
    # has this frame.  Absent rows of the returned PCM are zeros, their vad 0 and gains zeros; absent frames leave a stream's state alone.
    @torch.library.custom_op("rnnoise_amd::process_masked", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)")
    def process_masked(pcm, active, state, handle):
        res = _OPS[handle]._run(pcm, active)
        state.add_(pcm.shape[0])
        return res

    @process_masked.register_fake
    def _(pcm, active, state, handle):
        return fake_outs(pcm, pcm.shape[0], pcm.shape[1], pcm.dtype)

    # the stream-list form (include/rnnoise_amd.h: rnnoise_batch_process_device_list): pcm (T, R, M), row i of every frame
    # belongs to stream idx[i] (int32 CUDA tensor); active (T, R) or None.  Only the listed streams advance; absent rows of the returned
    # PCM are zeros, their vad 0 and gains zeros.
    @torch.library.custom_op("rnnoise_amd::process_list", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor idx, Tensor? active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)")
    def process_list(pcm, idx, active, state, handle):
        res = _OPS[handle]._run_list(pcm, idx, active)
        state.add_(pcm.shape[0])
        return res

    @process_list.register_fake
    def _(pcm, idx, active, state, handle):
        return fake_outs(pcm, pcm.shape[0], pcm.shape[1], pcm.dtype)

    # the stream-contiguous form (include/rnnoise_amd.h: rnnoise_batch_set_pcm_layout): pcm (N, T * (M)) float32 or int16, one
    # contiguous run of samples per stream -- the [B, T] tensor a torch user holds, read and written where it lies, no transpose.
    # active (T, N) or None, as in process_masked.  Returns out (same shape and dtype as pcm), vad (T, N), gains (T, N, 32).
    @torch.library.custom_op("rnnoise_amd::process_streams", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor? active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)")
    def process_streams(pcm, active, state, handle):
        op = _OPS[handle]
        res = op._run_streams(pcm, active)
        state.add_(pcm.shape[1] // op.batch.frame)
        return res

    @process_streams.register_fake
    def _(pcm, active, state, handle):
        return fake_outs(pcm, pcm.shape[1] // _OPS[handle].batch.frame, pcm.shape[0])

    # the interleaved form (include/rnnoise_amd.h: rnnoise_batch_set_pcm_channels): pcm (G, T * (M), C) float32 or int16 with
    # G * C the batch's streams -- channel c of group g is stream g * C + c --, read and written where it lies, no de-interleave.
    # active (T, G * C) or None.  Returns out (same shape and dtype as pcm), vad (T, G * C), gains (T, G * C, 32).
    @torch.library.custom_op("rnnoise_amd::process_channels", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor? active, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor)")
    def process_channels(pcm, active, state, handle):
        op = _OPS[handle]
        res = op._run_channels(pcm, active)
        state.add_(pcm.shape[1] // op.batch.frame)
        return res

    @process_channels.register_fake
    def _(pcm, active, state, handle):
        return fake_outs(pcm, pcm.shape[1] // _OPS[handle].batch.frame, pcm.shape[0] * pcm.shape[2])

    # the chunk form (include/rnnoise_amd.h: rnnoise_batch_process_device_chunks): pcm (N, max_count) float32 or int16, stream s pushes
    # its first counts[s] samples (counts: (N,) int32 CUDA tensor, clamped into [0, max_count]) and gets as many back, one frame late.
    # Returns out (same shape and dtype as pcm, zeros beyond counts), vad (F, N), gains (F, N, 32) with F = capi.chunk_frames(M,
    # max_count), and frames (N,) int32: the rows of vad / gains each stream filled.  The frame counter advances by F.
    @torch.library.custom_op("rnnoise_amd::process_chunks", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor counts, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor, Tensor)")
    def process_chunks(pcm, counts, state, handle):
        op = _OPS[handle]
        res = op._run_chunks(pcm, counts)
        state.add_(capi.chunk_frames(op.batch.frame, pcm.shape[1]))
        return res

    @process_chunks.register_fake
    def _(pcm, counts, state, handle):
        return fake_outs(pcm, capi.chunk_frames(_OPS[handle].batch.frame, pcm.shape[1]), pcm.shape[0], frames=True)

    # ... and on a stream list (rnnoise_batch_process_device_chunks_list): pcm (R, max_count), counts (R,) int32 and idx (R,) int32 CUDA
    # tensors, row i belonging to stream idx[i]; every result has R rows in idx's order.  The frame counter advances by F.
    @torch.library.custom_op("rnnoise_amd::process_chunks_list", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor counts, Tensor idx, Tensor(a!) state, int handle) -> (Tensor, Tensor, Tensor, Tensor)")
    def process_chunks_list(pcm, counts, idx, state, handle):
        op = _OPS[handle]
        res = op._run_chunks(pcm, counts, idx)
        state.add_(capi.chunk_frames(op.batch.frame, pcm.shape[1]))
        return res

    @process_chunks_list.register_fake
    def _(pcm, counts, idx, state, handle):
        return fake_outs(pcm, capi.chunk_frames(_OPS[handle].batch.frame, pcm.shape[1]), pcm.shape[0], frames=True)

    # the split calls (include/rnnoise_amd.h: rnnoise_batch_analyze_device, rnnoise_batch_synthesize_device): the DSP around a network of
    # the caller's.  analyze: pcm (T, N, M) float32 or int16 -> features (N, T, 65), the trainer's batch-first tensor, and the silence
    # words (T, N) int32; the T frames stay pending in the batch.  synthesize: gains (N, T, 32) and vad (N, T, 1) or (N, T) for the
    # pending frames -> out (T, N, M) of `like`'s dtype (float32 or int16; only its dtype is read).  The frame counter advances in
    # synthesize, by T.
    @torch.library.custom_op("rnnoise_amd::analyze", mutates_args=("state",),
                             schema="(Tensor pcm, Tensor(a!) state, int handle) -> (Tensor, Tensor)")
    def analyze(pcm, state, handle):
        res = _OPS[handle]._run_analyze(pcm)
        state.add_(0)
        return res

    @analyze.register_fake
    def _(pcm, state, handle):
        T, N = pcm.shape[0], pcm.shape[1]
        return pcm.new_empty((N, T, capi.FEATURES), dtype=torch.float32), pcm.new_empty((T, N), dtype=torch.int32)

    @torch.library.custom_op("rnnoise_amd::synthesize", mutates_args=("state",),
                             schema="(Tensor gains, Tensor vad, Tensor like, Tensor(a!) state, int handle) -> Tensor")
    def synthesize(gains, vad, like, state, handle):
        out = _OPS[handle]._run_synthesize(gains, vad, like.dtype)
        state.add_(gains.shape[1])
        return out

    @synthesize.register_fake
    def _(gains, vad, like, state, handle):
        N, T = gains.shape[0], gains.shape[1]
        return gains.new_empty((T, N, _OPS[handle].batch.frame), dtype=like.dtype)

    _registered = True


class RNNoiseOp:
    """N concurrent streams; call with a (T, N, M) float32 CUDA tensor of int16-scaled PCM at `rate` (48000, 32000, 24000, 16000 or 8000:
    include/rnnoise_amd.h, rnnoise_batch_set_pcm_rate), M = 480 * rate // 48000 samples per frame (capi.Batch.frame).  The same object is reachable as the registered op:
    torch.ops.rnnoise_amd.process(pcm, op.state, op.handle).
    extra_models: more model blobs, put into model slots 1, 2, ... of the batch (rnnoise_batch_add_model); every stream starts on
    slot 0 (model_blob) and set_stream_models moves streams between slots."""

    def __init__(self, model_blob: bytes, n_streams: int, device: int = 0, nn_path: str = "mfma", rate: int = 48000,
                 extra_models=()):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.model = capi.Model(model_blob)
        self.batch = capi.Batch(self.model, n_streams, device=device)
        if nn_path == "mfma":
            self.batch.set_nn_path(1)
        if rate != 48000:
            self.batch.set_pcm_rate(rate)
        for blob in extra_models:
            self.batch.add_model(capi.Model(blob))
        self.n = n_streams
        register_torch_op()
        self.handle = id(self)
        self.state = torch.zeros(1, dtype=torch.int64, device=self.device)  # frames processed: the tensor the op mutates
        _OPS[self.handle] = self

    def close(self):
        _OPS.pop(getattr(self, "handle", None), None)
        if getattr(self, "batch", None) is not None:
            extra = self.batch.extra_models
            self.batch.close()
            self.model.close()
            for m in extra:
                m.close()
            self.batch = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, pcm):
        return self.torch.ops.rnnoise_amd.process(pcm, self.state, self.handle)

    def process_masked(self, pcm, active):
        """pcm (T, N, M) float32 CUDA tensor, active (T, N) bool / uint8 CUDA tensor: streams whose frame has not arrived skip it
        (torch.ops.rnnoise_amd.process_masked)"""
        return self.torch.ops.rnnoise_amd.process_masked(pcm, active, self.state, self.handle)

    def process_list(self, pcm, idx, active=None):
        """pcm (T, R, M) float32 CUDA tensor whose row i is stream idx[i] (an (R,) int32 CUDA tensor), active (T, R) bool / uint8
        CUDA tensor or None: only the listed streams advance, with compact buffers (torch.ops.rnnoise_amd.process_list)"""
        return self.torch.ops.rnnoise_amd.process_list(pcm, idx, active, self.state, self.handle)

    def process_streams(self, pcm, active=None):
        """pcm (N, T * (M)) float32 or int16 CUDA tensor, stream-contiguous: row s is T consecutive frames of stream s.  The
        batch reads it and writes the result of the same shape where they lie (rnnoise_batch_set_pcm_layout: no transpose to frame-
        major and back); active (T, N) bool / uint8 or None as in process_masked.  -> out (N, T * (M)), vad (T, N), gains
        (T, N, 32) (torch.ops.rnnoise_amd.process_streams).  The layout is set when it changes -- a synchronous call, so keep T and
        the entry point the same from call to call."""
        return self.torch.ops.rnnoise_amd.process_streams(pcm, active, self.state, self.handle)

    def process_channels(self, pcm, active=None, link=None):
        """pcm (G, T * (M), C) float32 or int16 CUDA tensor with G * C == n_streams: interleaved channels, channel c of group g
        being stream g * C + c.  The batch reads it and writes the result of the same shape where they lie
        (rnnoise_batch_set_pcm_channels + rnnoise_batch_set_pcm_layout: no de-interleave and no transpose); active (T, G * C) bool /
        uint8 or None as in process_masked.  -> out (G, T * (M), C), vad (T, G * C), gains (T, G * C, 32)
        (torch.ops.rnnoise_amd.process_channels).  Channel count and layout are set when they change -- synchronous calls, so keep
        T, C and the entry point the same from call to call.
        link: True gives the C channels of every group one suppression (set_gain_link(C): rnnoise_batch_set_gain_link), False
        none (set_gain_link(1)), None leaves the link count as it is.  vad and gains returned stay each channel's own."""
        if link is not None:
            self.set_gain_link(int(pcm.shape[2]) if link else 1)
        return self.torch.ops.rnnoise_amd.process_channels(pcm, active, self.state, self.handle)

    def process_chunks(self, pcm, counts):
        """pcm (N, max_count) float32 or int16 CUDA tensor, counts (N,) int32 CUDA tensor: stream s pushes the first counts[s] samples
        of its row, any number of them, through the batch's sample FIFOs on the device and gets as many output samples back, one
        frame late.  -> out (N, max_count), vad (F, N), gains (F, N, 32), frames (N,) int32 (torch.ops.rnnoise_amd.process_chunks)"""
        return self.torch.ops.rnnoise_amd.process_chunks(pcm, counts, self.state, self.handle)

    def process_chunks_list(self, pcm, counts, idx):
        """process_chunks for the listed streams only: pcm (R, max_count) float32 or int16, counts (R,) int32 and idx (R,) int32 CUDA
        tensors, row i belonging to stream idx[i].  Unlisted streams are not touched and the cost follows R.  -> out (R, max_count),
        vad (F, R), gains (F, R, 32), frames (R,) int32 (torch.ops.rnnoise_amd.process_chunks_list)"""
        return self.torch.ops.rnnoise_amd.process_chunks_list(pcm, counts, idx, self.state, self.handle)

    def analyze(self, pcm):
        """pcm (T, N, M) float32 or int16 CUDA tensor -> features (N, T, 65) float32, silence (T, N) int32; the T frames stay pending
        until synthesize (torch.ops.rnnoise_amd.analyze)"""
        return self.torch.ops.rnnoise_amd.analyze(pcm, self.state, self.handle)

    def synthesize(self, gains, vad, like=None):
        """gains (N, T, 32) and vad (N, T, 1) or (N, T) float32 CUDA tensors for the pending frames -> out (T, N, M), float32 or of
        `like`'s dtype (torch.ops.rnnoise_amd.synthesize).  On a silent frame the rows are not read."""
        like = gains if like is None else like
        return self.torch.ops.rnnoise_amd.synthesize(gains, vad, like, self.state, self.handle)

    def denoise_with(self, net, pcm):
        """pcm (T, N, M) through analyze -> net -> synthesize in one pair: net maps features (N, T, 65) to (gains (N, T, 32),
        vad (N, T, 1)) -- any torch module or function; a stateful one keeps its own state from call to call.  -> out (T, N, M)"""
        with self.torch.no_grad():  # (forward only, like every op of this module)
            feats, _silence = self.analyze(pcm)
            gains, vad = net(feats)
            return self.synthesize(gains.to(self.torch.float32), vad.to(self.torch.float32), like=pcm)

    def _run_analyze(self, pcm):
        torch = self.torch
        assert pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.shape[1:] == (self.n, self.batch.frame)
        self._layout(0, 0)
        pcm = pcm.contiguous()
        T = pcm.shape[0]
        feats = torch.empty((self.n, T, capi.FEATURES), device=pcm.device, dtype=torch.float32)
        sil = torch.empty((T, self.n), device=pcm.device, dtype=torch.int32)
        self.batch.analyze_device(feats.data_ptr(), sil.data_ptr(), pcm.data_ptr(), T, feat_rows=(capi.FEATURES, T * capi.FEATURES),
                                  stream=torch.cuda.current_stream(pcm.device).cuda_stream, s16=pcm.dtype == torch.int16)
        return feats, sil

    def _run_synthesize(self, gains, vad, dtype):
        torch = self.torch
        assert gains.is_cuda and gains.dtype == torch.float32 and gains.dim() == 3 and gains.shape[0] == self.n
        assert gains.shape[2] == capi.NB_BANDS and dtype in (torch.float32, torch.int16)
        T = gains.shape[1]
        assert vad.is_cuda and vad.dtype == torch.float32 and vad.numel() == self.n * T and vad.shape[:2] == (self.n, T)
        gains, vad = gains.contiguous(), vad.contiguous()
        out = torch.empty((T, self.n, self.batch.frame), device=gains.device, dtype=dtype)
        self.batch.synthesize_device(out.data_ptr(), gains.data_ptr(), vad.data_ptr(), T, gain_rows=(capi.NB_BANDS, T * capi.NB_BANDS),
                                     vad_rows=(1, T), stream=torch.cuda.current_stream(gains.device).cuda_stream, s16=dtype == torch.int16)
        return out

    def reset_streams(self, idx):
        """the listed streams (a sequence or a tensor of indices) back to rnnoise_init()'s state, on torch's current stream without
        a host synchronisation (rnnoise_batch_reset_streams_device: entries out of range are ignored)"""
        torch = self.torch
        idx = torch.as_tensor(idx).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        # (freeing idx afterwards is safe: torch's allocator hands the block out again only in this stream's order)
        self.batch.reset_streams_device(idx.data_ptr(), int(idx.numel()), torch.cuda.current_stream(self.device).cuda_stream)

    def _records(self, call, width, idx, rec=None):
        """save (rec None: a fresh tensor) or load of the (n, width) float32 records of the listed streams (a sequence or a tensor of
        indices; None: the whole batch) through the device call `call`, on torch's current stream"""
        torch = self.torch
        if idx is not None:
            idx = torch.as_tensor(idx).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        n = self.n if idx is None else int(idx.numel())
        if rec is None:
            rec = torch.empty((n, width), device=self.device, dtype=torch.float32)
        else:
            assert rec.is_cuda and rec.dtype == torch.float32 and tuple(rec.shape) == (n, width)
            rec = rec.to(self.device).contiguous()
        # (freeing idx or a temporary copy afterwards is safe: torch's allocator hands the block out again only in this stream's order)
        call(rec.data_ptr(), 0 if idx is None else idx.data_ptr(), n, torch.cuda.current_stream(self.device).cuda_stream)
        return rec

    def save_streams(self, idx=None):
        """complete snapshots of the listed streams (a sequence or a tensor of indices; None: the whole batch) as an (n, SNAP_FLOATS)
        float32 CUDA tensor, on torch's current stream without a host synchronisation (rnnoise_batch_save_streams_device: a row whose
        entry is out of range gets an empty record).  The batch is unchanged."""
        return self._records(self.batch.save_streams_device, capi.SNAP_FLOATS, idx)

    def load_streams(self, snap, idx=None):
        """row i of snap ((n, SNAP_FLOATS) float32 CUDA tensor) becomes the complete state of stream idx[i] (None: the whole batch), on
        torch's current stream without a host synchronisation (rnnoise_batch_load_streams_device: empty records and entries out of
        range touch nothing).  Model slots and controls are the caller's to set."""
        self._records(self.batch.load_streams_device, capi.SNAP_FLOATS, idx, snap)

    def save_chunk_fifos(self, idx=None):
        """the FIFO records of the listed streams (None: the whole batch) as an (n, CHUNK_REC_FLOATS) float32 CUDA tensor, on torch's
        current stream without a host synchronisation (rnnoise_batch_save_chunk_fifos_device): what save_streams leaves behind of a
        stream fed through process_chunks.  The batch is unchanged."""
        return self._records(self.batch.save_chunk_fifos_device, capi.CHUNK_REC_FLOATS, idx)

    def load_chunk_fifos(self, rec, idx=None):
        """row i of rec ((n, CHUNK_REC_FLOATS) float32 CUDA tensor) becomes the FIFOs of stream idx[i], on torch's current stream
        (rnnoise_batch_load_chunk_fifos_device: rows that are no records of the batch's frame length and entries out of range touch
        nothing).  Call it AFTER load_streams, which restarts the FIFOs of the streams it loads."""
        self._records(self.batch.load_chunk_fifos_device, capi.CHUNK_REC_FLOATS, idx, rec)

    def _set_table(self, call, table):
        """an (N,) uint8 CUDA tensor as a per-stream table, through the device setter `call` on torch's current stream"""
        torch = self.torch
        assert table.is_cuda and table.dtype == torch.uint8 and table.numel() == self.n
        table = table.to(self.device).contiguous()
        # (freeing a temporary copy afterwards is safe: torch's allocator hands the block out again only in this stream's order)
        call(table.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)

    def set_stream_models(self, slots):
        """the model slot of every stream: an (N,) uint8 CUDA tensor, copied on torch's current stream without a host synchronisation
        (rnnoise_batch_set_stream_models_device: entries naming no slot read as slot 0).  The frames of later calls run with it."""
        self._set_table(self.batch.set_stream_models_device, slots)

    def set_stream_rates(self, hz):
        """the PCM rate of every stream in Hz (include/rnnoise_amd.h: rnnoise_batch_set_stream_rates): a sequence / array of N values
        out of 48000, 32000, 24000, 16000, 8000, none above the op's `rate`, or None to drop the table.  Rows of the PCM tensors keep the
        op's frame length; stream s reads and writes the first 480 * hz[s] // 48000 samples of its row and leaves the rest alone.
        Synchronous; ValueError on any other value."""
        self.batch.set_stream_rates(hz)

    def set_stream_formats(self, formats):
        """the PCM format of every stream's rows in the batch's int16 calls: an (N,) uint8 CUDA tensor of codes (0 s16, 1 ulaw, 2 alaw:
        rnnoise_amd.g711), copied on torch's current stream without a host synchronisation (rnnoise_batch_set_stream_formats_device: any
        other byte reads as s16).  The op's own calls are float calls and ignore the table; it serves the int16 device calls made on
        `self.batch` with tensors of this process (capi.Batch.process_device_s16 and its masked and list forms)."""
        self._set_table(self.batch.set_stream_formats_device, formats)

    def set_stream_out_rates(self, hz):
        """the rate every stream's OUTPUT rows are written at in Hz (include/rnnoise_amd.h: rnnoise_batch_set_stream_out_rates): as
        set_stream_rates, which then describes the input rows alone; None drops the table.  Stream s writes the first
        480 * hz[s] // 48000 samples of its output row.  Synchronous; ValueError on any other value."""
        self.batch.set_stream_out_rates(hz)

    def set_stream_out_formats(self, formats):
        """the PCM format of every stream's OUTPUT rows in the batch's int16 calls: an (N,) uint8 CUDA tensor of codes, as
        set_stream_formats (rnnoise_batch_set_stream_out_formats_device), which then describes the input rows alone"""
        self._set_table(self.batch.set_stream_out_formats_device, formats)

    def set_stream_controls(self, limit_db=None, vad_threshold=0.0, hold_frames=0):
        """per-stream suppression controls (include/rnnoise_amd.h: rnnoise_batch_set_stream_controls): an attenuation limit in dB (a
        floor on the band gains; None / inf: none), a VAD gate threshold in [0, 1] (0: no gate) and the frames the gate stays open
        after the last voice frame -- each a scalar or a per-stream sequence / array of N.  Synchronous; ValueError on a value out of
        range.  clear_stream_controls() drops the table."""
        self.batch.set_stream_controls(capi.controls_table(self.n, limit_db, vad_threshold, hold_frames))

    def set_gain_link(self, k=1):
        """linked gains (include/rnnoise_amd.h: rnnoise_batch_set_gain_link): the rows of every call taken k at a time, each group with
        one set of band gains and one VAD for the gate per frame; 1: none.  Synchronous, and only when the count changes; ValueError
        unless 1 <= k <= 8 and k divides the op's streams.  Returns the previous count."""
        old = self.batch.gain_link
        return self.batch.set_gain_link(k) if old != k else old

    def clear_stream_controls(self):
        """no controls: every stream back to the reference's suppression (the table and the gate counters are dropped)"""
        self.batch.set_stream_controls(None)

    def _layout(self, frame_stride, row_stride, channels=1):
        # (the setters drain the device: called only when the layout or the channel count changes)
        if self.batch.pcm_channels != channels:
            self.batch.set_pcm_channels(channels)
        if self.batch.pcm_layout != (frame_stride, row_stride):
            self.batch.set_pcm_layout(frame_stride, row_stride)

    def _launch(self, pcm, active, T, frame_stride, row_stride, channels=1):
        """T frames of every stream from pcm, which lies as the strides say: sets that layout, allocates vad and gains and launches the
        device call on torch's current stream -- the masked one with `active` (T, N), whose absent rows of out are zeros"""
        torch = self.torch
        pcm = pcm.contiguous()  # (a [B, T] or [B, T, C] tensor as torch makes it is: no copy)
        self._layout(frame_stride, row_stride, channels)
        s16 = pcm.dtype == torch.int16
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        vad = torch.empty((T, self.n), device=pcm.device, dtype=torch.float32)
        gains = torch.empty((T, self.n, capi.NB_BANDS), device=pcm.device, dtype=torch.float32)
        if active is None:
            out = torch.empty_like(pcm)
            self.batch.process_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), T, stream, s16=s16)
        else:
            assert active.is_cuda and active.shape == (T, self.n)
            act = (active != 0).to(torch.uint8).contiguous()
            out = torch.zeros_like(pcm)
            self.batch.process_masked_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), act.data_ptr(), T, stream,
                                             s16=s16)
        return out, vad, gains

    def _run_channels(self, pcm, active=None):
        torch = self.torch
        M = self.batch.frame
        assert pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.dim() == 3
        G, C = pcm.shape[0], pcm.shape[2]
        assert G * C == self.n and 1 <= C <= capi.MAX_CHANNELS and pcm.shape[1] % M == 0 and pcm.shape[1] > 0
        T = pcm.shape[1] // M
        return self._launch(pcm, active, T, M * C, T * M * C, C)

    def _run_streams(self, pcm, active=None):
        torch = self.torch
        M = self.batch.frame
        assert pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.dim() == 2
        assert pcm.shape[0] == self.n and pcm.shape[1] % M == 0 and pcm.shape[1] > 0
        T = pcm.shape[1] // M
        return self._launch(pcm, active, T, M, T * M)

    def _run(self, pcm, active=None):
        assert pcm.is_cuda and pcm.dtype == self.torch.float32 and pcm.shape[1:] == (self.n, self.batch.frame)
        return self._launch(pcm, active, pcm.shape[0], 0, 0)

    def _run_chunks(self, pcm, counts, idx=None):
        """the chunk op, and with idx (R,) its list form, whose R rows belong to the listed streams"""
        torch = self.torch
        assert pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.dim() == 2
        R = pcm.shape[0]
        assert R == self.n if idx is None else R <= self.n
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.numel() == R
        assert idx is None or (idx.is_cuda and idx.dtype == torch.int32 and idx.numel() == R)
        self._layout(0, 0)
        pcm, counts, idx = pcm.contiguous(), counts.contiguous(), None if idx is None else idx.contiguous()
        F = capi.chunk_frames(self.batch.frame, pcm.shape[1])
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        new = torch.empty if idx is None else torch.zeros  # (the list form hands out zeroed vad and gains)
        vad = new((F, R), device=pcm.device, dtype=torch.float32)
        gains = new((F, R, capi.NB_BANDS), device=pcm.device, dtype=torch.float32)
        frames = torch.zeros((R,), device=pcm.device, dtype=torch.int32)
        out = torch.zeros_like(pcm)
        if pcm.shape[1] == 0 or R == 0:  # (nothing to push: the library's no-op, and an empty tensor has no address to hand it)
            return out, vad, gains, frames
        args = out.data_ptr(), pcm.data_ptr(), counts.data_ptr(), pcm.shape[1]
        rest = vad.data_ptr(), gains.data_ptr(), frames.data_ptr(), stream
        if idx is None:
            self.batch.process_chunks_device(*args, *rest, s16=pcm.dtype == torch.int16)
        else:
            self.batch.process_chunks_list_device(*args, idx.data_ptr(), R, *rest, s16=pcm.dtype == torch.int16)
        return out, vad, gains, frames

    def _run_list(self, pcm, idx, active=None):
        torch = self.torch
        assert pcm.is_cuda and pcm.dtype == torch.float32 and pcm.dim() == 3 and pcm.shape[2] == self.batch.frame
        assert idx.is_cuda and idx.dtype == torch.int32 and idx.numel() == pcm.shape[1]
        self._layout(0, 0)
        pcm, idx = pcm.contiguous(), idx.contiguous()
        T, R = pcm.shape[0], pcm.shape[1]
        stream = torch.cuda.current_stream(pcm.device).cuda_stream
        vad = torch.empty((T, R), device=pcm.device, dtype=torch.float32)
        gains = torch.empty((T, R, capi.NB_BANDS), device=pcm.device, dtype=torch.float32)
        out = torch.zeros_like(pcm)
        act = None
        if active is not None:
            assert active.is_cuda and active.shape == (T, R)
            act = (active != 0).to(torch.uint8).contiguous()
        self.batch.process_list_device(out.data_ptr(), pcm.data_ptr(), vad.data_ptr(), gains.data_ptr(), idx.data_ptr(), R,
                                       act.data_ptr() if act is not None else 0, T, stream)
        return out, vad, gains

    def reset(self):
        self.batch.reset()
        self.state.zero_()


class FloatNet:
    """Float32 forward of the network from a blob: int8 layers de-quantised (w_q * scale * 127), exact
    tanh/sigmoid, float activations.  State handling as src/rnn.c:44-60 / src/nnet.c:65-123."""

    def __init__(self, model_blob: bytes):
        r = rblob.read_blob(model_blob)
        f = lambda a: np.asarray(a, np.float64)  # noqa: E731
        self.c1w, self.c1b = f(r["conv1_weights_float"]).reshape(195, 128), f(r["conv1_bias"])
        q = f(r["conv2_weights_int8"]).reshape(48, 96, 8, 4).transpose(1, 3, 0, 2).reshape(384, 384)  # -> (in, out)
        self.c2w, self.c2b = q * f(r["conv2_scale"]) * 127, f(r["conv2_bias"])
        self.gru = []
        for k in (1, 2, 3):
            mats = []
            for side in ("input", "recurrent"):
                name = f"gru{k}_{side}"
                w = np.zeros((384, 1152))
                idx, blocks = r[name + "_weights_idx"], f(r[name + "_weights_int8"]).reshape(-1, 8, 4)
                p = b = 0
                for grp in range(144):
                    nb = idx[p]; p += 1
                    for _ in range(nb):
                        col = idx[p]; p += 1
                        w[col:col + 4, 8 * grp:8 * grp + 8] = blocks[b].T
                        b += 1
                w = w * f(r[name + "_scale"]) * 127
                if side == "recurrent":
                    d = f(r[name + "_weights_diag"])
                    for g in range(3):
                        w[np.arange(384), g * 384 + np.arange(384)] += d[g * 384:(g + 1) * 384]
                mats.append((w, f(r[name + "_bias"])))
            self.gru.append(mats)
        self.dw, self.db = f(r["dense_out_weights_float"]).reshape(1536, 32), f(r["dense_out_bias"])
        self.vw, self.vb = f(r["vad_dense_weights_float"]).reshape(1536, 1), f(r["vad_dense_bias"])
        self.reset()

    def reset(self):
        self.c1s, self.c2s, self.h = np.zeros(130), np.zeros(256), [np.zeros(384) for _ in range(3)]

    def step(self, features65):
        sig = lambda x: 1 / (1 + np.exp(-x))  # noqa: E731
        t1 = np.concatenate([self.c1s, features65])
        c1 = np.tanh(t1 @ self.c1w + self.c1b)
        self.c1s = t1[65:]
        t2 = np.concatenate([self.c2s, c1])
        x = np.tanh(t2 @ self.c2w + self.c2b)
        self.c2s = t2[128:]
        cat = [x]
        for k, ((wi, bi), (wr, br)) in enumerate(self.gru):
            a, b = x @ wi + bi, self.h[k] @ wr + br
            z, rr = sig(a[:384] + b[:384]), sig(a[384:768] + b[384:768])
            hh = np.tanh(a[768:] + b[768:] * rr)
            self.h[k] = z * self.h[k] + (1 - z) * hh
            x = self.h[k]
            cat.append(x)
        cat = np.concatenate(cat)
        return sig(cat @ self.dw + self.db), float(sig(cat @ self.vw + self.vb)[0])
