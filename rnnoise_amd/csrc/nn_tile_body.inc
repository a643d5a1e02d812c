// nn_tile_body.inc -- body of the 16-stream tile kernels of nn_mfma.hip (the whole network for one tile), included once per kernel
// (a template or a shared __device__ function costs the fused kernel 30-80 VGPRs with this compiler: measured 118 -> 150 / 201).
//   RN_NN_LIST 0: tile row r is stream r;  1: tile row r is stream g.list[r] when a list is set (rn_dev.h: RnGroupDev::list), stream r
//   otherwise.  (Compiled once per value behind a uniform branch on g.list, the two bodies in one kernel spilled 29-49 registers.)
// The including kernel declares the LDS arena L (MfmaLds).
// NWAVES (8 | 16) is whatever the including file has it at: every loop over row / unit tiles strides by it, the one-per-wave roles
// (conv1's eight row tiles, the 512 producer threads of the dense phase, the three chain waves) stay on the first eight waves.
  // The tile is one long dependency chain and the analysis kernel of the next frame queues behind the LDS it
  // holds: let its waves win instruction arbitration against the co-resident analysis waves (4096 streams:
  // +2.4 % mean over 4 alternating A/B runs, run-to-run noise +-3 %; no effect at 65,536).
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, gq = lane >> 4;
  // Tile rows r = s0 .. s0 + 15: without a list row r is stream r; in a list call it is stream list[r] (rn_dev.h: RnGroupDev::list).
  // ROW_OK(r): row r has a stream -- only such rows get stores.  ROW_S(r): the stream to load from for row min(r, N - 1) (stream 0 for
  // a list entry naming none).
#if RN_NN_LIST
  const int N = g.list ? g.list_n : g.n_streams, s0 = blockIdx.x * TS;
#define ROW_OK(r) ((r) < N && (!g.list || (unsigned)g.list[(r)] < (unsigned)g.n_stride))
#define ROW_S(r) (g.list ? rn_list_stream_or0(g, min((r), N - 1)) : min((r), N - 1))
#else
  const int N = g.n_streams, s0 = blockIdx.x * TS;
#define ROW_OK(r) ((r) < N)
#define ROW_S(r) ((r) < N ? (r) : N - 1)
#endif
  const int sn = ROW_S(s0 + n);                              // this lane's stream (clamped for loads)
  const int sil_n = g.silence[sn];                           // (sn is clamped: loaded unconditionally, not behind the range test's branch)
  // model slots (rn_dev.h: RnGroupDev::model_of): bit q of ownm = this launch owns stream s0 + q.  Rows of another slot get no store
  // at all -- their slot's launch writes them -- and a tile without an owned row is left before any LDS or barrier (uniform: every
  // wave forms the same mask).
  uint32_t ownm = 0xffffu;
  if (g.model_of) {
    ownm = (uint32_t)__ballot(lane < TS && ROW_OK(s0 + lane) && rn_owns(g, ROW_S(s0 + lane)));
    if (!ownm) return;
  }
#define OWN(q) ((ownm >> (q)) & 1u)
  const bool live = ROW_OK(s0 + n) && !sil_n && OWN(n);        // silent streams keep state (src/denoise.c:474)
  const uint16_t *lut = L.lut;
#if RN_INSTRUMENT
  float *dbg = (g.debug && tid == 0) ? g.debug + (size_t)s0 * RN_DBG_FLOATS + RN_DBG_CLK2 : nullptr;
#else
  float *const dbg = nullptr;
#endif
  unsigned long long clk_prev = (RN_INSTRUMENT && g.debug) ? __builtin_amdgcn_s_memtime() : 0;
#define CLK_TAP(idx)                                           \
  do {                                                         \
    if (RN_INSTRUMENT && g.debug) {                            \
      unsigned long long now_ = __builtin_amdgcn_s_memtime();  \
      if (dbg) dbg[idx] = (float)(now_ - clk_prev);            \
      clk_prev = now_;                                         \
    }                                                          \
  } while (0)

  {  // (loads first, then stores: as a run-time loop every one of its four trips waited out its own L2 round trip)
    static_assert(2048 % NTHREADS == 0, "whole trips");
    uint32_t lw[2048 / NTHREADS];
#pragma unroll
    for (int j = 0; j < 2048 / NTHREADS; j++) lw[j] = reinterpret_cast<const uint32_t *>(tb.rcp16)[tid + j * NTHREADS];
#pragma unroll
    for (int j = 0; j < 2048 / NTHREADS; j++) reinterpret_cast<uint32_t *>(L.lut)[tid + j * NTHREADS] = lw[j];
  }
  {
    static_assert(RN_CAT % 512 == 0, "whole trips of the first eight waves");
    float vw_[RN_CAT / 512];
    if (NWAVES == 8 || tid < 512) {
#pragma unroll
      for (int j = 0; j < RN_CAT / 512; j++) vw_[j] = m.vad_dense.fw[tid + j * 512];
#pragma unroll
      for (int j = 0; j < RN_CAT / 512; j++) L.vadw[tid + j * 512] = vw_[j];
    }
  }
  // ---- conv1 input: [conv1_state(130) | features(65) | 0] per stream ----
  // (constant trip count, fully unrolled, loads before stores: all of a thread's loads are in flight together -- as a
  //  run-time loop each iteration waited out its own HBM trip: 21k of the front kernel's 66k cycles per tile)
  constexpr int NE1 = (TS * 196 + NTHREADS - 1) / NTHREADS;
  float t1v[NE1];
#pragma unroll
  for (int j = 0; j < NE1; j++) {
    const int e = tid + j * NTHREADS, q = e / 196, k = e - q * 196, s = ROW_S(s0 + q);
    float v = 0;
    if (e < TS * 196 && k < 130) v = g.conv1_state[(size_t)s * 130 + k];
    else if (e < TS * 196 && k < 195) v = g.features[(size_t)s * 68 + (k - 130)];
    t1v[j] = v;
  }
  constexpr int C1WD = 4;  // conv1 weight groups (of four chain steps) in flight
  const v4f *c1wq = reinterpret_cast<const v4f *>(m.conv1.fwm) + (size_t)(wave & 7) * 13 * 64 + lane;
  v4f c1w[C1WD];
#pragma unroll
  for (int u = 0; u < C1WD; u++) c1w[u] = c1wq[u * 64];
  // conv2 history: quantise old[0..255] into xq[0] (k = 0..255); keep old[128..255] to shift the state
  constexpr int HC = 1024 / NTHREADS;  // 16 streams x 64 chunks of 4 floats, spread over the workgroup
  v4f hist[HC];
  int hq_[HC], hk_[HC];
#pragma unroll
  for (int c = 0; c < HC; c++) {
    const int chunk = tid + c * NTHREADS, q = chunk >> 6, k = (chunk & 63) << 2;  // 16 streams x 64 chunks of 4
    const int s = ROW_S(s0 + q);
    hist[c] = *reinterpret_cast<const v4f *>(g.conv2_state + (size_t)s * 256 + k);
    hq_[c] = q;
    hk_[c] = k;
    *reinterpret_cast<int *>(L.xq[0] + frag_off(q, k)) = pack4(hist[c][0], hist[c][1], hist[c][2], hist[c][3]);
  }
#pragma unroll
  for (int j = 0; j < NE1; j++) {
    const int e = tid + j * NTHREADS, q = e / 196, k = e - q * 196;
    if (e < TS * 196) L.tmp1[q][k] = t1v[j];
  }
  __syncthreads();
  // state shifts (src/nnet.c:122): conv1 history <- tmp1[65..194]; conv2 history[0..127] <- old[128..255]
  constexpr int NE2 = (TS * 130 + NTHREADS - 1) / NTHREADS;
  int sil2[NE2];
#pragma unroll
  for (int j = 0; j < NE2; j++) {
    const int q = (tid + j * NTHREADS) / 130;
    sil2[j] = g.silence[ROW_S(s0 + q)];
  }
#pragma unroll
  for (int j = 0; j < NE2; j++) {
    const int e = tid + j * NTHREADS, q = e / 130, k = e - q * 130;
    if (e < TS * 130 && ROW_OK(s0 + q) && !sil2[j] && OWN(q)) g.conv1_state[(size_t)ROW_S(s0 + q) * 130 + k] = L.tmp1[q][65 + k];
  }
#pragma unroll
  for (int c = 0; c < HC; c++)
    if (hk_[c] >= 128 && ROW_OK(s0 + hq_[c]) && !g.silence[ROW_S(s0 + hq_[c])] && OWN(hq_[c]))
      *reinterpret_cast<v4f *>(g.conv2_state + (size_t)ROW_S(s0 + hq_[c]) * 256 + hk_[c] - 128) = hist[c];

  CLK_TAP(0);  // loads, history quantisation, state shifts
  // ---- conv1: f32 MFMA, 195(+1) -> 128 = 8 row tiles, one per wave ----
  // Weights in MFMA operand order (model.cpp: stage_linear): 16 bytes = this lane's operands of four steps, the first
  // C1WD groups requested before the loads of the prologue were waited for (c1w above), the rest C1WD groups ahead of their
  // MFMAs.  (Fetched element by element from the row-major matrix, every one of the 49 chain steps waited out an L2 trip:
  // 14 k of the front kernel's cycles per tile.)
  if (NWAVES == 8 || wave < 8) {  // one conv1 row tile per wave, eight of them
    const int rt = wave;
    v4f acc = {0, 0, 0, 0};
    const float *bx = &L.tmp1[n][gq];
#pragma unroll
    for (int u = 0; u < 12; u++) {  // steps 0..47
      const v4f a = c1w[u % C1WD];
      if (u + C1WD < 13) c1w[u % C1WD] = c1wq[(u + C1WD) * 64];
#pragma unroll
      for (int e = 0; e < 4; e++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bx[16 * u + 4 * e], acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(c1w[12 % C1WD][0], bx[192], acc, 0, 0, 0);  // step 48: inputs 192..194 (+ the zero pad)
    const int row0 = 16 * rt + 4 * gq;
    const v4f bs = *reinterpret_cast<const v4f *>(m.conv1.bias + row0);
    v4f c1;
#pragma unroll
    for (int r = 0; r < 4; r++) c1[r] = tanh_x86(acc[r] + bs[r], lut);
    *reinterpret_cast<int *>(L.xq[0] + frag_off(n, 256 + row0)) = pack4(c1[0], c1[1], c1[2], c1[3]);
    if (live) *reinterpret_cast<v4f *>(g.conv2_state + (size_t)sn * 256 + 128 + row0) = c1;
  }
  __syncthreads();

  CLK_TAP(1);  // conv1
  // ---- conv2: int8 dense 384 -> 384, tanh; wave w owns row tiles w, w+4, ... ----
  {
    for (int rt = wave; rt < 24; rt += NWAVES) {
      const int row0 = 16 * rt + 4 * gq;
      v4f o = int8_finish(m.conv2, row0, int8_tile(m.conv2.wmf, rt, lane, L.xq[0]));
#pragma unroll
      for (int r = 0; r < 4; r++) o[r] = tanh_x86(o[r], lut);
      if (ROW_OK(s0 + n)) *reinterpret_cast<v4f *>(g.nn_act + (size_t)sn * RN_GRU + row0) = o;  // f32 copy for dense_out
      *reinterpret_cast<int *>(L.xq[1] + frag_off(n, row0)) = pack4(o[0], o[1], o[2], o[3]);
    }
  }

  // ---- three GRUs (src/nnet.c:65-94); wave w owns hidden-unit tiles w, w+4, ... ----
  int cur = 1;
  CLK_TAP(2);  // conv2
  for (int k = 0; k < 3; k++) {
    float *st = g.gru_state + (size_t)k * g.n_stride * RN_GRU;
    for (int e = tid; e < TS * 96; e += NTHREADS) {  // quantise the old state into hq
      const int q = e / 96, c4 = (e - q * 96) << 2, s = ROW_S(s0 + q);
      const v4f h = *reinterpret_cast<const v4f *>(st + (size_t)s * RN_GRU + c4);
      *reinterpret_cast<int *>(L.hq + frag_off(q, c4)) = pack4(h[0], h[1], h[2], h[3]);
    }
    __syncthreads();
    const RnLinearDev &wi = m.gru_in[k], &wr = m.gru_rec[k];
    for (int u = wave; u < 24; u += NWAVES) {
      const int unit0 = 16 * u + 4 * gq;
      const v4f h_old = *reinterpret_cast<const v4f *>(st + (size_t)sn * RN_GRU + unit0);
      v4f gi[3], gr[3];
#pragma unroll
      for (int gate = 0; gate < 3; gate++) {
        gi[gate] = int8_finish(wi, gate * RN_GRU + unit0, int8_tile(wi.wmf, gate * 24 + u, lane, L.xq[cur]));
        gr[gate] = int8_finish(wr, gate * RN_GRU + unit0, int8_tile(wr.wmf, gate * 24 + u, lane, L.hq));
        const v4f dg = *reinterpret_cast<const v4f *>(wr.diag + gate * RN_GRU + unit0);
#pragma unroll
        for (int r = 0; r < 4; r++) gr[gate][r] += dg[r] * h_old[r];  // src/nnet_arch.h:153-161
      }
      v4f hn;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float z = sigmoid_x86(gi[0][r] + gr[0][r], lut);
        const float rg = sigmoid_x86(gi[1][r] + gr[1][r], lut);
        const float hh = tanh_x86(gi[2][r] + gr[2][r] * rg, lut);
        hn[r] = z * h_old[r] + (1 - z) * hh;
      }
      if (live) *reinterpret_cast<v4f *>(st + (size_t)sn * RN_GRU + unit0) = hn;
      *reinterpret_cast<int *>(L.xq[cur ^ 1] + frag_off(n, unit0)) = pack4(hn[0], hn[1], hn[2], hn[3]);
    }
    cur ^= 1;
    __syncthreads();
    CLK_TAP(3 + k);  // GRU k
  }

  // ---- dense_out (1536 -> 32, f32 MFMA chains, waves 0-1) and vad_dense (wave 2, lane = stream) ----
  // cat = [conv2 out | gru1 | gru2 | gru3] (src/rnn.c:53-55); silent streams are computed on
  // their unchanged state and discarded.
  // The chains are serial over the 1536 inputs.  Their activation operand is staged through LDS in
  // chunks of 128 inputs by the whole workgroup (one coalesced 16-byte load per thread and chunk, issued
  // a full chunk ahead and parked in a register), because fetched straight from the per-stream rows every
  // chain step costs 16 scattered L1 accesses -- and the vector L1 is what this kernel saturates first.
  // Measured with the phase taps at 65,536 streams: what paced this phase was the lane = stream VAD chain waiting for its
  // weights in L2 at every step (77k -> 54k clocks per tile with the weights in LDS), not the MFMA chain's weights.
  // Dead ends (this round): running the chains segment by segment inside the GRU phases (the tile loop then spills at
  // 128 VGPRs: K2 1.00 -> 1.14-1.28 ms); one 384-input chunk per barrier (172 VGPRs or spills: 1.13 ms).
  {
    const int pq = tid >> 5, pc = (tid & 31) << 2;              // producer role: stream pq, floats pc + 128 j .. +3 of a chunk, j = 0, 1
    const int ps = ROW_S(s0 + pq);
    auto chunk_src = [&](int c) {                                // chunk c = inputs 128c .. 128c+127 of cat
      // half-chunk h = 2c + j covers inputs 128 h .. 128 h + 127 of cat: segment h / 3, offset 128 (h % 3)
      return [=](int j) {
        const int h = 2 * c + j, seg = h / 3, k0 = (h - 3 * seg) * 128;
        return *reinterpret_cast<const v4f *>((seg == 0 ? g.nn_act : g.gru_state + (size_t)(seg - 1) * g.n_stride * RN_GRU) +
                                              (size_t)ps * RN_GRU + k0 + pc);
      };
    };
    constexpr int NCH = 4 * RN_GRU / CHUNK;  // 12
    const bool prod = NWAVES == 8 || tid < 512;  // (16 streams x 32 threads stage a chunk)
    v4f park[2] = {};
    if (prod) {
      park[0] = chunk_src(0)(0);
      park[1] = chunk_src(0)(1);
      *reinterpret_cast<v4f *>(&L.stage[0][pq][pc]) = park[0];  // xq / hq / tmp1 are dead: the last GRU barrier is behind us
      *reinterpret_cast<v4f *>(&L.stage[0][pq][pc + 128]) = park[1];
      park[0] = chunk_src(1)(0);
      park[1] = chunk_src(1)(1);
    }
    v4f dacc = {0, 0, 0, 0};
    float vacc = 0;
    // dense_out weights: the MFMA-ordered copy (model.cpp: stage_linear) -- 16 bytes = this lane's operands of four
    // consecutive steps, WDEPTH loads (4 x WDEPTH steps, > 1000 cycles of chain) in flight
    constexpr int WDEPTH = 8, NW4 = RN_CAT / 16;  // 96 groups of four steps
    static_assert((CHUNK / 16) % WDEPTH == 0, "a chunk is a whole number of weight-buffer rounds");
    const v4f *wq = reinterpret_cast<const v4f *>(m.dense_out.fwm) + (size_t)(wave & 1) * NW4 * 64 + lane;
    v4f wbuf[WDEPTH];
    if (wave < 2) {
#pragma unroll
      for (int u = 0; u < WDEPTH; u++) wbuf[u] = wq[u * 64];
    }
    __syncthreads();
    for (int c = 0; c < NCH; c++) {
      if (prod && c + 1 < NCH) {
        *reinterpret_cast<v4f *>(&L.stage[(c + 1) & 1][pq][pc]) = park[0];
        *reinterpret_cast<v4f *>(&L.stage[(c + 1) & 1][pq][pc + 128]) = park[1];
      }
      if (prod && c + 2 < NCH) {
        park[0] = chunk_src(c + 2)(0);
        park[1] = chunk_src(c + 2)(1);
      }
      const float(*sx)[CH_STRIDE] = L.stage[c & 1];
      if (wave < 2) {  // 64 MFMA steps: k = 256c + 16*t4 + 4e + gq
        const float *bx = &sx[n][gq];
#pragma unroll 8
        for (int t4 = 0; t4 < CHUNK / 16; t4++) {
          const int gidx = (CHUNK / 16) * c + t4;
          const v4f a = wbuf[t4 % WDEPTH];  // slot t4 % WDEPTH holds group gidx
          if (gidx + WDEPTH < NW4) wbuf[t4 % WDEPTH] = wq[(size_t)(gidx + WDEPTH) * 64];
#pragma unroll
          for (int e = 0; e < 4; e++) dacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bx[16 * t4 + 4 * e], dacc, 0, 0, 0);
        }
      } else if (wave == 2 && lane < TS) {  // unfused mul-then-add, src/vec_avx.h:732-736
        const v4f *w = reinterpret_cast<const v4f *>(L.vadw + CHUNK * c);
        const v4f *x = reinterpret_cast<const v4f *>(sx[lane]);
#pragma unroll 4
        for (int j = 0; j < CHUNK / 4; j++) {
          const v4f wj = w[j], xj = x[j];
#pragma unroll
          for (int e = 0; e < 4; e++) vacc = vacc + wj[e] * xj[e];
        }
      }
      __syncthreads();
    }
    if (wave < 2) {
      const int row0 = 16 * wave + 4 * gq;
      const v4f bs = *reinterpret_cast<const v4f *>(m.dense_out.bias + row0);
      v4f o;
#pragma unroll
      for (int r = 0; r < 4; r++) o[r] = live ? sigmoid_x86(dacc[r] + bs[r], lut) : 0.f;
      if (ROW_OK(s0 + n) && OWN(n)) *reinterpret_cast<v4f *>(g.gains + (size_t)sn * RN_NB_BANDS + row0) = o;
    } else if (wave == 2 && lane < TS) {
      const int q = s0 + lane, sq = ROW_S(q);
      const bool ok = ROW_OK(q), lv = ok && !g.silence[sq];
      if (ok && OWN(lane)) g.vad[sq] = lv ? sigmoid_x86(vacc + m.vad_dense.bias[0], lut) : 0.f;
    }
  }
  CLK_TAP(6);  // dense_out / vad (wave 0's view)
#undef CLK_TAP
#undef OWN
#undef ROW_OK
#undef ROW_S
