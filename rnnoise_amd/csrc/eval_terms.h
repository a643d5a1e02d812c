// eval_terms.h -- one scored frame's terms of the reference trainer's loss (torch/rnnoise/train_rnnoise.py:149-155) in double, in
// the lane roles of a wave of 64: the body of the record step and of the score walk (dsp_kernels.hip) and of the loss-and-gradient
// kernel of librnnoise_amd_train.so (train/train_loss.hip).  Both units include this text, so the doubles the product's score calls
// add up and those the trainer's loss adds up are the same expressions compiled with the same flags: equal bit for bit by
// construction.  The including unit defines WAVE (64) and RN_NB_BANDS (32) and, on the device, has hip_runtime.h.
//   tg = max(g, 0) * tanh(8 max(g, 0))^2;  gain term (1 + 5 v) * min(g + 1, 1) * (p^gamma - tg^gamma)^2;
//   vad term |2 v - 1| * (-v log(.01 + q) - (1 - v) log(1.01 - q))
// NaN goes where torch's clamp sends it.
#pragma once

// one scored frame's terms from its four kinds of floats -- gt the record's gain target of band lane & 31, v its VAD target, p the
// predicted gain of that band, q the predicted VAD -- in the lane roles above: the body of the record step and of the score walk
struct EvalTerms {
  double band;     // lanes 0 .. 31: the band's gain term; lanes 32 .. 63: +0
  double term;     // the butterfly's sum of the 32 gain terms
  double lg, lg1;  // lane 0: log(.01 + q), log(1.01 - q)
  double pw, d;    // lanes 0 .. 31: p^gamma and p^gamma - tg^gamma, as the band's term has them (read by the gradient only)
};
__device__ __forceinline__ EvalTerms eval_frame_terms(float gt_f, float v_f, float p_f, float q_f, double gamma, int lane) {
  const double v = (double)v_f;
  // the f64 library calls are what this launch costs, so each runs once per wave: lane b raises band b's prediction
  // to gamma while lane 32 + b raises its shaped target, and lanes 0 and 1 take the two logs of the VAD term
  const double gt = (double)gt_f, p = (double)p_f;
  double tg = gt < 0.0 ? 0.0 : gt;
  const double th = tanh(8.0 * tg);
  tg = tg * (th * th);
  const double pw = pow(lane < RN_NB_BANDS ? p : tg, gamma);
  const double d = pw - __shfl_xor(pw, RN_NB_BANDS, WAVE);
  const double m = gt + 1.0 > 1.0 ? 1.0 : gt + 1.0;
  EvalTerms k;
  k.band = lane < RN_NB_BANDS ? ((1.0 + 5.0 * v) * m) * (d * d) : 0.0;
  k.term = k.band;
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) k.term += __shfl_xor(k.term, off, WAVE);
  const double q = (double)q_f;
  k.lg = log(lane == 0 ? .01 + q : 1.01 - q), k.lg1 = __shfl_xor(k.lg, 1, WAVE);
  k.pw = pw, k.d = d;
  return k;
}
// lane 0's VAD term of the frame
__device__ __forceinline__ double eval_vad_term(float v_f, const EvalTerms &k) {
  const double v = (double)v_f;
  return fabs(2.0 * v - 1.0) * (-v * k.lg - (1.0 - v) * k.lg1);
}
