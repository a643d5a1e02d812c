// batch_step.h -- the frame step in pieces: what the whole step (batch_step.cpp: batch_process_device_impl) and the two halves of the
// split calls (batch_split.cpp) are driven from.  A Step is one process call, checked and planned; its members are the stages, each of
// which enqueues the launches of one frame on the stream the schedule gives it.  A driver is a loop over them.  Internal.
#pragma once
#include "shim.h"

#include <optional>

// What a driver launches, set when it builds its Step (the stages test nothing else about who drives them)
struct StepKind {
  bool side_k1;  // K1 may go to a side stream of its own (the analysis half keeps it on the caller's, with its export step behind it)
  bool k0;       // the call launches K0 and K1: it reads `in`, and may run them ahead on side streams (rn_schedule) -- the synthesis
                 // half has nothing to overlap
  bool k3;       // the call launches K3: it writes `out`, and under schedule 1 K0 of frame f starts behind K3 of frame f - 3
};

struct Step {
  RNNoiseBatch *b = nullptr;
  ProcessCall c;
  RnPlan plan{};
  bool listed = false, pipelined = false, side_k1 = false, k3 = true;
  hipStream_t st = nullptr, sb = nullptr, sc = nullptr;  // the caller's stream (network + synthesis), K1's, K0's
  size_t N = 0;      // rows of the caller's buffers
  size_t fstep = 0;  // bytes between the frames of the PCM buffers
  int pcm_pitch = 0, pcm_chan = 0, link = 1;  // the row pitch K0 / K3 get (0: the form's own constant), rn_dev.h: RnGroupDev::pcm_chan, ::link
  std::optional<DeviceGuard> guard;  // the batch's device, for as long as the Step lives
  Step() = default;
  Step(const Step &) = delete;
  // The one way a Step is made: the call's checks, the first masked call's phases, schedule and plan, the side streams and their
  // start behind the caller's stream.  0: run the stages; 1: the call has nothing to do and returns 0; -1: refused, nothing launched
  // or changed
  int begin(RNNoiseBatch *batch, const ProcessCall &call, StepKind kind);

  size_t buf(int f) const { return c.hooks ? (size_t)(f % c.hooks->ring) : (size_t)f; }  // frame f's place in the caller's buffers
  RnGroupDev call_group(int f) const;
  RnGroupDev frame_group(int f) const;
  int highpass(int f);                                       // K0 of frame f on stream sc
  int analysis(int f, RnGroupDev &g);                        // K1 of frame f on stream sb, on the frame's group
  int network(int f, RnGroupDev &g);                         // the network of frame f on the caller's stream
  int synthesis(int f, RnGroupDev &g, int cur, int prev);    // K3 of frame f on the caller's stream
  int finish();                                              // a list call's requant tail, and the batch's frame counters
};

// The host-buffer form of a call (batch_step.cpp: batch_process_staged; batch_split.cpp: the staged halves): its shape, and how its
// PCM travels between the caller's buffers and the default layout in one device allocation
struct StagedCall {
  RNNoiseBatch *b = nullptr;
  int n_frames = 0;
  size_t rows = 0, M = 0, esz = 0, C = 1;  // rows per frame, samples per row, bytes per sample, channels
  size_t fs = 0, pcm = 0;                  // rows of the call, bytes of one PCM buffer
  bool laid = false;
  int pcm_copy(void *dst, const void *src, bool up) const;
  // `out` goes up too where the device leaves parts of it alone: absent rows, the part of a row behind the frame of a stream of a
  // rate table or an out-rate table, or behind a companded stream's bytes, keep the caller's values
  int out_up(void *dst, const ProcessCall &c) const;
};
// -1: rows that fill no whole groups, or frame slots that overlap under the batch's layout
int staged_begin(StagedCall &s, RNNoiseBatch *b, const ProcessCall &c);
