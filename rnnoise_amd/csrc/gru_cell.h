// gru_cell.h -- the float GRU cell of librnnoise_amd_gru.so (gru/gru_seq.hip) and librnnoise_amd_gru_stack.so (gru_stack/gru_stack.hip):
// one workgroup's forward step and backward step of one layer, device code only.  The units keep their argument structs, their
// kernels (which pick the layer and call the cell) and their host loops; each library is still built from its own object.
//
// A workgroup of four waves owns 16 hidden units x 16 rows of one layer; wave w takes the w-th quarter of every sum with
// v_mfma_f32_16x16x4_f32 (exact float32: a k-ordered fmaf chain), A = weights, B = the rows' vectors, so a row is a column of B and
// of the result and never meets another row.  The quarters go through LDS and thread e of the 256 adds them up in wave order for
// unit e & 15 of row e >> 4, does the gate math and stores with ordinary vector-memory stores.
//
// Which k a lane feeds into an issue is free as long as A and B agree, so where a quarter holds 16 k or more, lane group q = lane >> 4
// loads the four consecutive k 16 c' + 4 q .. + 3 as one 16-byte read and issue c of the chunk takes element c of every group; what
// is left of a quarter (H = 16, 48: 4 and 12 k) goes one k per lane group and issue.
//
// Forward: K = H over y[t-1] and w_hh (HH), and for a layer that projects its own input (OWN_GI) another K = H over the layer
// below's y[t] and w_ih (IH), both written by an earlier launch; the reads of both halves of a block of chunks are issued together.
// The r and z sums of the two halves meet per wave (P^hh_w + P^ih_w); the n gate keeps hn and gi_n as sums of their own.
// Backward: K = 3H as H units x three gates, the wave's lanes compute the dgh they feed (element-wise on saved[t], dh, dy[t], y[t-1])
// instead of reading it, the workgroup of unit tile 0 also stores it (and dgi), and the result w_hh^T dgh + dh z goes to the OTHER dh
// buffer: every workgroup of a row tile reads all of dh while the others write their slices.  DX_IN: the layer above adds its dx to
// dy; DX_OUT: a second accumulator set, dx = w_ih^T dgi from the gate gradients a lane computes anyway.
//
// The single-layer kernels instantiate what layer 0 of the stack does forward (OWN_GI = false) and what a layer with DX_IN = DX_OUT =
// false does backward.  The argument type of a step is the unit's own (a template parameter): a field a flag rules out is not named.
#pragma once

#define RN_CELL_WAVE 64
#define RN_CELL_TILE 16  // hidden units, and rows, of a workgroup
#define RN_CELL_WAVES 4
#define RN_CELL_PAD 68  // floats of a register's row of partial sums: 64 lanes + 4, so the transposed read of the last stage hits 64 banks

// Chunks of 16 k whose reads a wave issues together before the first of their matrix instructions: a step is short and every read
// is a trip to L2 or HBM, so the reads of a quarter are put in flight at once instead of chunk after chunk.  Forward: 6 chunks of one
// half (H = 384: a wave's whole quarter) or 3 of both halves (24 reads of 16 bytes either way); backward, which reads seven vectors
// and twelve weights per chunk: 3, and 2 where the second weight matrix is read too.
#define RN_CELL_FWD_CH 6
#define RN_CELL_FWD2_CH 3
#define RN_CELL_BWD_CH 3
#define RN_CELL_BWD2_CH 2

#ifdef __HIPCC__  // (the units' host halves as plain C++ see the constants only)
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

static __device__ __forceinline__ float rn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// what a lane of the forward step reads: the row's vector and the three gates' weight rows of unit u0 + (lane & 15), from the
// wave's first k on
struct RnCellFwdHalf {
  const float *pb, *pa0, *pa1, *pa2;
};

// CH chunks of the forward sums from k offset kk on: every read first (both halves), then the issues in k order, each half a chain of
// its own (the order does not depend on CH)
template <int CH, bool HH, bool IH>
static __device__ __forceinline__ void rn_cell_fwd_chunks(const RnCellFwdHalf &h, const RnCellFwdHalf &x, int kk, bool live,
                                                          f32x4 (&hh)[3], f32x4 (&ih)[3]) {
  f32x4 hb[CH], h0[CH], h1[CH], h2[CH], xb[CH], x0[CH], x1[CH], x2[CH];
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int o = kk + 16 * i;
    if (HH) {
      hb[i] = *reinterpret_cast<const f32x4 *>(h.pb + o);
      h0[i] = *reinterpret_cast<const f32x4 *>(h.pa0 + o);
      h1[i] = *reinterpret_cast<const f32x4 *>(h.pa1 + o);
      h2[i] = *reinterpret_cast<const f32x4 *>(h.pa2 + o);
    }
    if (IH) {
      xb[i] = *reinterpret_cast<const f32x4 *>(x.pb + o);
      x0[i] = *reinterpret_cast<const f32x4 *>(x.pa0 + o);
      x1[i] = *reinterpret_cast<const f32x4 *>(x.pa1 + o);
      x2[i] = *reinterpret_cast<const f32x4 *>(x.pa2 + o);
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // the reads stay together above: left alone, the scheduler puts 8 in flight and interleaves the rest
#pragma unroll
  for (int i = 0; i < CH; i++) {
    if (!live) hb[i] = f32x4{0.f, 0.f, 0.f, 0.f}, xb[i] = f32x4{0.f, 0.f, 0.f, 0.f};  // rows beyond the last read as zeros (the read went to row 0)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (HH) {
        hh[0] = RN_MFMA(h0[i][c], hb[i][c], hh[0]);
        hh[1] = RN_MFMA(h1[i][c], hb[i][c], hh[1]);
        hh[2] = RN_MFMA(h2[i][c], hb[i][c], hh[2]);
      }
      if (IH) {
        ih[0] = RN_MFMA(x0[i][c], xb[i][c], ih[0]);
        ih[1] = RN_MFMA(x1[i][c], xb[i][c], ih[1]);
        ih[2] = RN_MFMA(x2[i][c], xb[i][c], ih[2]);
      }
    }
  }
}

// a wave's quarter of the forward sums: L k from the halves' first on
template <int CH, bool HH, bool IH>
static __device__ __forceinline__ void rn_cell_fwd_quarter(const RnCellFwdHalf &h, const RnCellFwdHalf &x, int L, int q, bool live,
                                                           f32x4 (&hh)[3], f32x4 (&ih)[3]) {
  int k = 0;
  for (; k + 16 * CH <= L; k += 16 * CH) rn_cell_fwd_chunks<CH, HH, IH>(h, x, k + 4 * q, live, hh, ih);
  for (; k + 16 <= L; k += 16) rn_cell_fwd_chunks<1, HH, IH>(h, x, k + 4 * q, live, hh, ih);
  for (; k < L; k += 4) {  // what is left of a quarter: one k per lane group and issue
    const int kk = k + q;
    if (HH) {
      const float b = live ? h.pb[kk] : 0.f;
      hh[0] = RN_MFMA(h.pa0[kk], b, hh[0]);
      hh[1] = RN_MFMA(h.pa1[kk], b, hh[1]);
      hh[2] = RN_MFMA(h.pa2[kk], b, hh[2]);
    }
    if (IH) {
      const float b = live ? x.pb[kk] : 0.f;
      ih[0] = RN_MFMA(x.pa0[kk], b, ih[0]);
      ih[1] = RN_MFMA(x.pa1[kk], b, ih[1]);
      ih[2] = RN_MFMA(x.pa2[kk], b, ih[2]);
    }
  }
}

// the partial sums of a forward step in LDS; sets: r, z, hn, and gi_n where the layer projects its own input
template <bool OWN_GI>
struct RnCellFwdLds {
  float part[RN_CELL_WAVES][OWN_GI ? 4 : 3][4][RN_CELL_PAD];
};

// one layer's forward step for units u0 .. u0 + 15 of the row tile blockIdx.y.  Step names gi, in_rs (the row stride of gi or of x),
// w_hh, b_hh, prev (y[t-1] of row 0, or NULL: zeros), prev_rs, y, y_rs, saved, and with OWN_GI x, w_ih, b_ih.  OWN_GI and
// p.prev != NULL are uniform over the workgroup.
template <bool OWN_GI, class Step>
static __device__ __forceinline__ void rn_cell_forward(const Step &p, int n_rows, int H, int u0, RnCellFwdLds<OWN_GI> &lds) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (RN_CELL_WAVE - 1), q = lane >> 4, m = lane & 15;
  const int s0 = (int)blockIdx.y * RN_CELL_TILE;
  const int L = H >> 2, k0 = wave * L;  // this wave's k: k0 .. k0 + L - 1
  // what the last stage needs of memory, asked for before the sum: unit fu of row frow (row 0 where the row does not exist)
  const int fi = tid & 15, fj = tid >> 4, frow = s0 + fj, fu = u0 + fi;
  const bool flive = frow < n_rows;
  const long long fr = flive ? frow : 0;
  float gi_r, gi_z, gi_n;
  if constexpr (OWN_GI) {
    gi_r = p.b_ih[fu], gi_z = p.b_ih[H + fu], gi_n = p.b_ih[2 * H + fu];
  } else {
    const float *const gi = p.gi + fr * p.in_rs;
    gi_r = gi[fu], gi_z = gi[H + fu], gi_n = gi[2 * H + fu];
  }
  const float b_r = p.b_hh[fu], b_z = p.b_hh[H + fu], b_n = p.b_hh[2 * H + fu];
  float hp = 0.f;
  f32x4 hh[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 ih[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  {
    const int row = s0 + m;
    const bool live = row < n_rows;
    const long long lrow = live ? row : 0, wo = (long long)(u0 + m) * H + k0, HH2 = (long long)H * H;
    RnCellFwdHalf h{}, x{};
    if constexpr (OWN_GI) x.pb = p.x + lrow * p.in_rs + k0, x.pa0 = p.w_ih + wo, x.pa1 = x.pa0 + HH2, x.pa2 = x.pa1 + HH2;
    if (p.prev != nullptr) {  // (uniform) zeros before: that half's sums stay zero, gh = b_hh
      hp = p.prev[fr * p.prev_rs + fu];
      h.pb = p.prev + lrow * p.prev_rs + k0, h.pa0 = p.w_hh + wo, h.pa1 = h.pa0 + HH2, h.pa2 = h.pa1 + HH2;
      if constexpr (OWN_GI)
        rn_cell_fwd_quarter<RN_CELL_FWD2_CH, true, true>(h, x, L, q, live, hh, ih);
      else
        rn_cell_fwd_quarter<RN_CELL_FWD_CH, true, false>(h, x, L, q, live, hh, ih);
    } else if constexpr (OWN_GI) {
      rn_cell_fwd_quarter<RN_CELL_FWD_CH, false, true>(h, x, L, q, live, hh, ih);
    }
  }
  // the result's map: lane holds row (column) lane & 15, units 4 (lane >> 4) + register
#pragma unroll
  for (int r = 0; r < 4; r++) {
    lds.part[wave][0][r][lane] = OWN_GI ? hh[0][r] + ih[0][r] : hh[0][r];
    lds.part[wave][1][r][lane] = OWN_GI ? hh[1][r] + ih[1][r] : hh[1][r];
    lds.part[wave][2][r][lane] = hh[2][r];
    if constexpr (OWN_GI) lds.part[wave][3][r][lane] = ih[2][r];
  }
  __syncthreads();
  if (!flive) return;  // rows that do not exist are not stored
  const int src = (fi >> 2) * 16 + fj, reg = fi & 3;
  float S[OWN_GI ? 4 : 3];
#pragma unroll
  for (int g = 0; g < (OWN_GI ? 4 : 3); g++)
    S[g] = ((lds.part[0][g][reg][src] + lds.part[1][g][reg][src]) + lds.part[2][g][reg][src]) + lds.part[3][g][reg][src];
  float r, z, n;
  const float hn = S[2] + b_n;
  if constexpr (OWN_GI) {
    r = rn_sigmoid(S[0] + (gi_r + b_r)), z = rn_sigmoid(S[1] + (gi_z + b_z));
    n = tanhf((S[3] + gi_n) + r * hn);
  } else {
    r = rn_sigmoid(gi_r + (S[0] + b_r)), z = rn_sigmoid(gi_z + (S[1] + b_z));
    n = tanhf(gi_n + r * hn);
  }
  p.y[(long long)frow * p.y_rs + fu] = (1.f - z) * n + z * hp;
  float *const sv = p.saved + (long long)frow * 4 * H + fu;
  sv[0] = r, sv[H] = z, sv[2 * H] = n, sv[3 * H] = hn;
}

// dgh of one unit of one row from what the forward step saved: -> a_r, a_z, a_n (dgi) and a_n r (dgh's third)
static __device__ __forceinline__ void rn_cell_gate_grads(float r, float z, float n, float hn, float dh, float hp, float &a_r, float &a_z,
                                                          float &a_n, float &b_n) {
  a_n = dh * (1.f - z) * (1.f - n * n);
  a_z = dh * (hp - n) * z * (1.f - z);
  a_r = a_n * hn * r * (1.f - r);
  b_n = a_n * r;
}

// what a lane of the backward step reads and writes of its row (row 0 where the row does not exist: read, zeroed, never stored)
struct RnCellGradLane {
  const float *sv, *dy, *dxi, *dhi, *hp;  // saved[t], dy[t], dx_{l+1}[t] (DX_IN), dh before (HAS_DH), y[t-1] (HAS_PREV) of the row
  float *dgi, *dgh;
  const float *pa0, *pa1, *pa2;  // w_hh's column c0 + (lane & 15) in the three gates' rows
  const float *pv0, *pv1, *pv2;  // w_ih's likewise (DX_OUT)
  bool live, store;
};

// CH chunks of 16 units of the backward sums from unit u on: every read first, then per chunk the gate gradients, their stores (unit
// tile 0 only) and the issues
template <bool HAS_DH, bool HAS_PREV, bool DX_IN, bool DX_OUT, int CH>
static __device__ __forceinline__ void rn_cell_bwd_chunks(const RnCellGradLane &p, int H, int u, f32x4 (&acc)[3], f32x4 (&acx)[3]) {
  f32x4 r[CH], z[CH], n[CH], hn[CH], dh[CH], dx[CH], di[CH], h[CH];
  float w0[CH][4], w1[CH][4], w2[CH][4], v0[CH][4], v1[CH][4], v2[CH][4];
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int v = u + 16 * i;
    r[i] = *reinterpret_cast<const f32x4 *>(p.sv + v), z[i] = *reinterpret_cast<const f32x4 *>(p.sv + H + v);
    n[i] = *reinterpret_cast<const f32x4 *>(p.sv + 2 * H + v), hn[i] = *reinterpret_cast<const f32x4 *>(p.sv + 3 * H + v);
    dh[i] = *reinterpret_cast<const f32x4 *>(p.dy + v);
    if (DX_IN) dx[i] = *reinterpret_cast<const f32x4 *>(p.dxi + v);
    if (HAS_DH) di[i] = *reinterpret_cast<const f32x4 *>(p.dhi + v);
    h[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (HAS_PREV) h[i] = *reinterpret_cast<const f32x4 *>(p.hp + v);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const long long o = (long long)(v + c) * H;
      w0[i][c] = p.pa0[o], w1[i][c] = p.pa1[o], w2[i][c] = p.pa2[o];
      if (DX_OUT) v0[i][c] = p.pv0[o], v1[i][c] = p.pv1[o], v2[i][c] = p.pv2[o];
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (as in the forward step)
#pragma unroll
  for (int i = 0; i < CH; i++) {
    const int v = u + 16 * i;
    if (DX_IN) dh[i] = dh[i] + dx[i];
    if (HAS_DH) dh[i] = di[i] + dh[i];
    f32x4 a_r, a_z, a_n, b_n;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float xr, xz, xn, xb;
      rn_cell_gate_grads(r[i][c], z[i][c], n[i][c], hn[i][c], dh[i][c], h[i][c], xr, xz, xn, xb);
      a_r[c] = p.live ? xr : 0.f, a_z[c] = p.live ? xz : 0.f, a_n[c] = p.live ? xn : 0.f, b_n[c] = p.live ? xb : 0.f;
    }
    if (p.store && p.live) {
      *reinterpret_cast<f32x4 *>(p.dgi + v) = a_r, *reinterpret_cast<f32x4 *>(p.dgi + H + v) = a_z;
      *reinterpret_cast<f32x4 *>(p.dgi + 2 * H + v) = a_n;
      *reinterpret_cast<f32x4 *>(p.dgh + v) = a_r, *reinterpret_cast<f32x4 *>(p.dgh + H + v) = a_z;
      *reinterpret_cast<f32x4 *>(p.dgh + 2 * H + v) = b_n;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      acc[0] = RN_MFMA(w0[i][c], a_r[c], acc[0]);
      acc[1] = RN_MFMA(w1[i][c], a_z[c], acc[1]);
      acc[2] = RN_MFMA(w2[i][c], b_n[c], acc[2]);
      if (DX_OUT) {
        acx[0] = RN_MFMA(v0[i][c], a_r[c], acx[0]);
        acx[1] = RN_MFMA(v1[i][c], a_z[c], acx[1]);
        acx[2] = RN_MFMA(v2[i][c], a_n[c], acx[2]);
      }
    }
  }
}

// the partial sums of a backward step in LDS; sets: w_hh^T dgh, and w_ih^T dgi where the layer leaves a dx
template <bool DX_OUT>
struct RnCellBwdLds {
  float part[RN_CELL_WAVES][DX_OUT ? 2 : 1][4][RN_CELL_PAD];
};

// one layer's backward step for units c0 .. c0 + 15 of the row tile blockIdx.y; HAS_DH: there is a dh from the step after (not at the
// last step of a call without dhT), HAS_PREV: there is a y[t-1] (not at step 0 of a call without h0), DX_IN: the layer above adds its
// dx to dy, DX_OUT: this layer leaves a dx -- uniform over the workgroup, so the reads of the usual step stand unconditionally.
// Step names saved, dy, dy_rs, prev, prev_rs, dh_in, w_hh, dgi, dgi_rs, dgh, dh_out, with DX_IN dx_in, with DX_OUT w_ih and dx_out.
template <bool HAS_DH, bool HAS_PREV, bool DX_IN, bool DX_OUT, class Step>
static __device__ __forceinline__ void rn_cell_grad_step(const Step &a, int n_rows, int H, int c0, RnCellBwdLds<DX_OUT> &lds) {
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & (RN_CELL_WAVE - 1), q = lane >> 4, m = lane & 15;
  const int s0 = (int)blockIdx.y * RN_CELL_TILE;
  const int L = H >> 2, ub = wave * L;  // this wave's units ub .. ub + L - 1, each with its three gates
  constexpr int CH = DX_OUT ? RN_CELL_BWD2_CH : RN_CELL_BWD_CH;
  // what the last stage needs of memory, asked for before the sum: unit fu of row frow (row 0 where the row does not exist)
  const int fi = tid & 15, fj = tid >> 4, frow = s0 + fj, fu = c0 + fi;
  const bool flive = frow < n_rows;
  const long long fr = flive ? frow : 0;
  float f_dh = a.dy[fr * a.dy_rs + fu];
  const float f_z = a.saved[fr * 4 * H + H + fu];
  if constexpr (DX_IN) f_dh = f_dh + a.dx_in[fr * H + fu];
  if (HAS_DH) f_dh = a.dh_in[fr * H + fu] + f_dh;
  f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  f32x4 acx[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  {
    const int row = s0 + m;
    RnCellGradLane p{};
    p.live = row < n_rows, p.store = c0 == 0;  // (store: uniform) one workgroup of a layer's row tile stores dgi and dgh
    const long long lrow = p.live ? row : 0, HH2 = (long long)H * H;
    p.sv = a.saved + lrow * 4 * H, p.dy = a.dy + lrow * a.dy_rs;
    if constexpr (DX_IN) p.dxi = a.dx_in + lrow * H;
    p.dhi = HAS_DH ? a.dh_in + lrow * H : nullptr;
    p.hp = HAS_PREV ? a.prev + lrow * a.prev_rs : nullptr;
    p.dgi = a.dgi + lrow * a.dgi_rs, p.dgh = a.dgh + lrow * 3 * H;
    // A[i][k] = w[gate row k][c0 + i]: lane reads column c0 + (lane & 15) of the gate rows it feeds
    p.pa0 = a.w_hh + c0 + m, p.pa1 = p.pa0 + HH2, p.pa2 = p.pa1 + HH2;
    if constexpr (DX_OUT) p.pv0 = a.w_ih + c0 + m, p.pv1 = p.pv0 + HH2, p.pv2 = p.pv1 + HH2;
    int k = 0;
    for (; k + 16 * CH <= L; k += 16 * CH) rn_cell_bwd_chunks<HAS_DH, HAS_PREV, DX_IN, DX_OUT, CH>(p, H, ub + k + 4 * q, acc, acx);
    for (; k + 16 <= L; k += 16) rn_cell_bwd_chunks<HAS_DH, HAS_PREV, DX_IN, DX_OUT, 1>(p, H, ub + k + 4 * q, acc, acx);
    for (; k < L; k += 4) {  // what is left of a quarter: one unit per lane group and issue
      const int u = ub + k + q;
      float dh = p.dy[u];
      if (DX_IN) dh = dh + p.dxi[u];
      if (HAS_DH) dh = p.dhi[u] + dh;
      float a_r, a_z, a_n, b_n;
      rn_cell_gate_grads(p.sv[u], p.sv[H + u], p.sv[2 * H + u], p.sv[3 * H + u], dh, HAS_PREV ? p.hp[u] : 0.f, a_r, a_z, a_n, b_n);
      if (!p.live) a_r = 0.f, a_z = 0.f, a_n = 0.f, b_n = 0.f;
      if (p.store && p.live) {
        p.dgi[u] = a_r, p.dgi[H + u] = a_z, p.dgi[2 * H + u] = a_n;
        p.dgh[u] = a_r, p.dgh[H + u] = a_z, p.dgh[2 * H + u] = b_n;
      }
      const long long o = (long long)u * H;
      acc[0] = RN_MFMA(p.pa0[o], a_r, acc[0]);
      acc[1] = RN_MFMA(p.pa1[o], a_z, acc[1]);
      acc[2] = RN_MFMA(p.pa2[o], b_n, acc[2]);
      if (DX_OUT) {
        acx[0] = RN_MFMA(p.pv0[o], a_r, acx[0]);
        acx[1] = RN_MFMA(p.pv1[o], a_z, acx[1]);
        acx[2] = RN_MFMA(p.pv2[o], a_n, acx[2]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    lds.part[wave][0][r][lane] = (acc[0][r] + acc[1][r]) + acc[2][r];
    if constexpr (DX_OUT) lds.part[wave][1][r][lane] = (acx[0][r] + acx[1][r]) + acx[2][r];
  }
  __syncthreads();
  if (!flive) return;
  const int src = (fi >> 2) * 16 + fj, reg = fi & 3;
  const float sum = ((lds.part[0][0][reg][src] + lds.part[1][0][reg][src]) + lds.part[2][0][reg][src]) + lds.part[3][0][reg][src];
  a.dh_out[(long long)frow * H + fu] = f_dh * f_z + sum;
  if constexpr (DX_OUT)
    a.dx_out[(long long)frow * H + fu] =
        ((lds.part[0][1][reg][src] + lds.part[1][1][reg][src]) + lds.part[2][1][reg][src]) + lds.part[3][1][reg][src];
}

// the backward step of a layer whose dh_in and prev may be NULL (zeros): both uniform over the launch
template <bool DX_IN, bool DX_OUT, class Step>
static __device__ __forceinline__ void rn_cell_backward(const Step &p, int n_rows, int H, int c0, RnCellBwdLds<DX_OUT> &lds) {
  if (p.dh_in != nullptr) {
    if (p.prev != nullptr)
      rn_cell_grad_step<true, true, DX_IN, DX_OUT>(p, n_rows, H, c0, lds);
    else
      rn_cell_grad_step<true, false, DX_IN, DX_OUT>(p, n_rows, H, c0, lds);
  } else {
    if (p.prev != nullptr)
      rn_cell_grad_step<false, true, DX_IN, DX_OUT>(p, n_rows, H, c0, lds);
    else
      rn_cell_grad_step<false, false, DX_IN, DX_OUT>(p, n_rows, H, c0, lds);
  }
}
#endif  // __HIPCC__
