// gru_stack_main.cpp -- the host halves of rnnoise_amd/csrc/gru_stack/gru_stack.hip and rnnoise_amd/csrc/gru/gru_seq.hip as a plain
// C++ program (TEST INFRASTRUCTURE, built with the address and undefined-behaviour sanitizers by tests/test_gru_stack_cpu.py): the
// device calls of both run with every launch handed to a model of the memory instead of a device.  The model keeps, per float of every buffer, what was last written there
// (which layer, which step, which kind) and in which launch, and checks for every launch of the diagonal schedule that
//   - the grid and the layers of the launch are those of the header (launch s: layer l at step s - l; backward the mirror image),
//   - every float a layer's workgroups read holds exactly the value the formulas want (y_l[t-1], y_{l-1}[t], dh of step t + 1,
//     dx_{l+1}[t], saved[l][t], or an input) and was written by an EARLIER launch,
//   - no float is written twice in a launch, or read and written in the same launch (the kernel boundary is the only ordering),
//   - every address lies inside a buffer of the documented size (the work buffers are allocated at exactly the workspace call's),
// and after a call that everything it promises is written.  The single-layer calls run on the same shapes as a stack of one layer
// (layer 0): T launches each way of (H/16) x ceil(N/16) workgroups, step t reads the y[t-1] an earlier launch wrote, dh_out is never
// dh_in, the halves of the scratch alternate and the last step writes dh0.  Prints "ok <cases>" and exits 0, or the first violation
// and exits 1.
#define RN_STK_HOST 1
#define RN_GRU_HOST 1
#include "gru_stack.hip"
#undef RN_SIDE_LIB  // (each unit names itself for side_host.h's messages)
#include "gru_seq.hip"

#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

namespace {
enum Kind { NEVER = 0, INPUT, Y, SAVED, DGI, DGH, DH, DX };
const char *const KIND[] = {"never written", "input", "y", "saved", "dgi", "dgh", "dh", "dx"};

struct Cell {
  unsigned char kind = NEVER;
  signed char layer = -1;
  int step = -1, launch = -1;
};

struct Buf {
  std::string name;
  float *mem;
  std::vector<Cell> cell;
  Buf(const std::string &n, size_t floats, bool input) : name(n), cell(floats) {
    mem = static_cast<float *>(aligned_alloc(64, (floats * sizeof(float) + 63) / 64 * 64 + 64));
    if (input)
      for (Cell &c : cell) c.kind = INPUT;
  }
  Buf(const Buf &) = delete;
  ~Buf() { free(mem); }
};

std::vector<Buf *> g_bufs;
std::string g_case;
int g_launch = 0;        // counts the launches of both calls of a case
int g_call_launches = 0;  // ... of the call that runs

[[noreturn]] void fail(const std::string &what) {
  fprintf(stderr, "gru_stack_main: %s: launch %d: %s\n", g_case.c_str(), g_launch, what.c_str());
  exit(1);
}

Cell *cells(const float *p, long long n, const char *what) {
  for (Buf *b : g_bufs)
    if (p >= b->mem && p < b->mem + b->cell.size()) {
      if (p + n > b->mem + b->cell.size()) fail(std::string(what) + ": runs past the end of " + b->name);
      return b->cell.data() + (p - b->mem);
    }
  fail(std::string(what) + ": an address outside every buffer");
}

void writes(float *p, long long n, Kind kind, int layer, int step, const char *what) {
  Cell *c = cells(p, n, what);
  for (long long i = 0; i < n; i++) {
    if (c[i].launch == g_launch) fail(std::string(what) + ": written twice in one launch");
    if (c[i].kind == INPUT) fail(std::string(what) + ": writes an input");
    c[i].kind = kind, c[i].layer = (signed char)layer, c[i].step = step, c[i].launch = g_launch;
  }
}

void reads(const float *p, long long n, Kind kind, int layer, int step, const char *what) {
  const Cell *c = cells(p, n, what);
  for (long long i = 0; i < n; i++) {
    if (c[i].kind != kind || (kind != INPUT && (c[i].layer != layer || c[i].step != step)))
      fail(std::string(what) + ": wants " + KIND[kind] + " of layer " + std::to_string(layer) + " step " + std::to_string(step) + ", finds " +
           KIND[c[i].kind] + " of layer " + std::to_string(c[i].layer) + " step " + std::to_string(c[i].step));
    if (c[i].launch >= g_launch) fail(std::string(what) + ": read in the launch that writes it");
  }
}

void want(bool ok, const char *what) {
  if (!ok) fail(what);
}

const RNNoiseGruStack *g_fwd = nullptr;
const RNNoiseGruStackGrad *g_bwd = nullptr;
const float *g_saved = nullptr;
const RNNoiseGruSeq *g_seq_fwd = nullptr;
const RNNoiseGruSeqGrad *g_seq_bwd = nullptr;
const float *g_seq_scratch = nullptr, *g_seq_dh = nullptr;  // the scratch, and what the launch before left as dh
}  // namespace

static void check_grid(dim3 grid, dim3 block, int layers, int N, int H) {
  want(layers >= 1 && grid.x == (unsigned)(layers * (H / 16)) && grid.y == (unsigned)((N + 15) / 16) && grid.z == 1, "the grid");
  want(block.x == 256 && block.y == 1 && block.z == 1, "the block");
}

static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t, const RnStackStep &a) {
  const RNNoiseGruStack &c = *g_fwd;
  const int s = g_call_launches, T = c.n_frames, N = c.n_rows, H = c.hidden;
  want(s < T + 2, "more than T + 2 launches");
  want(a.n_rows == N && a.H == H && a.tiles == H / 16, "the sizes");
  int lo = 3, hi = -1;
  for (int l = 0; l < 3; l++)
    if (s - l >= 0 && s - l < T) lo = l < lo ? l : lo, hi = l;
  check_grid(grid, block, hi - lo + 1, N, H);
  for (int pass = 0; pass < 2; pass++)  // all the writes of the launch, then all its reads
    for (int l = lo; l <= hi; l++) {
      const RnStackLayerStep &p = a.L[l - lo];
      const int t = s - l;
      if (pass == 0) {
        want(p.y == c.y[l] + (long long)t * c.y_frame_stride[l] && p.y_rs == c.y_row_stride[l], "y is not the layer's slot");
        want(p.w_hh == c.w_hh[l] && p.b_hh == c.b_hh[l], "the recurrent weights are not the layer's");
        for (int r = 0; r < N; r++) {
          writes(p.y + r * p.y_rs, H, Y, l, t, "y");
          writes(p.saved + (long long)r * 4 * H, 4 * H, SAVED, l, t, "saved");
        }
        want(p.saved == g_saved + ((long long)l * T + t) * N * 4 * H, "saved is not [l][t]");
        continue;
      }
      if (l == 0) {
        want(p.gi != nullptr && p.x == nullptr, "layer 0 reads gi0");
        for (int r = 0; r < N; r++) reads(p.gi + r * p.in_rs, 3 * H, INPUT, 0, 0, "gi0");
      } else {
        want(p.gi == nullptr && p.w_ih == c.w_ih[l] && p.b_ih == c.b_ih[l], "layers 1, 2 project their own input");
        for (int r = 0; r < N; r++) reads(p.x + r * p.in_rs, H, Y, l - 1, t, "the layer below's output");
      }
      if (t == 0) {
        want(p.prev == c.h0[l], "step 0 reads h0");
        if (p.prev)
          for (int r = 0; r < N; r++) reads(p.prev + r * p.prev_rs, H, INPUT, 0, 0, "h0");
      } else {
        for (int r = 0; r < N; r++) reads(p.prev + r * p.prev_rs, H, Y, l, t - 1, "y[t-1]");
      }
    }
  g_call_launches++, g_launch++;
}

static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t, const RnStackGradStep &a) {
  const RNNoiseGruStackGrad &c = *g_bwd;
  const int s = g_call_launches, T = c.n_frames, N = c.n_rows, H = c.hidden;
  want(s < T + 2, "more than T + 2 launches");
  want(a.n_rows == N && a.H == H && a.tiles == H / 16, "the sizes");
  int lo = 3, hi = -1;
  for (int l = 0; l < 3; l++) {
    const int t = T - 1 - s + (2 - l);
    if (t >= 0 && t < T) lo = l < lo ? l : lo, hi = l;
  }
  check_grid(grid, block, hi - lo + 1, N, H);
  for (int pass = 0; pass < 2; pass++)
    for (int l = lo; l <= hi; l++) {
      const RnStackLayerGrad &p = a.L[l - lo];
      const int t = T - 1 - s + (2 - l);
      if (pass == 0) {
        want(p.dh_out != nullptr && (t != 0 || p.dh_out == c.dh0[l]), "the last step writes dh0");
        want((p.dx_out != nullptr) == (l > 0), "layers 1, 2 leave a dx, layer 0 none");
        want(p.dgh == c.dgh[l] + (long long)t * N * 3 * H, "dgh is not [t]");
        if (l == 0)
          want(p.dgi == c.dgi[0] + (long long)t * c.dgi0_frame_stride && p.dgi_rs == c.dgi0_row_stride, "dgi[0] is not the slot");
        else
          want(p.dgi == c.dgi[l] + (long long)t * N * 3 * H && p.dgi_rs == 3 * H, "dgi[l] is not [t]");
        for (int r = 0; r < N; r++) {
          writes(p.dgi + r * p.dgi_rs, 3 * H, DGI, l, t, "dgi");
          writes(p.dgh + (long long)r * 3 * H, 3 * H, DGH, l, t, "dgh");
          writes(p.dh_out + (long long)r * H, H, DH, l, t, "dh");
          if (l > 0) writes(p.dx_out + (long long)r * H, H, DX, l, t, "dx");
        }
        continue;
      }
      want(p.w_hh == c.w_hh[l] && p.w_ih == (l > 0 ? c.w_ih[l] : nullptr), "the weights are not the layer's");
      want((p.dx_in != nullptr) == (l < 2), "layers 0, 1 read a dx, layer 2 none");
      for (int r = 0; r < N; r++) {
        reads(p.saved + (long long)r * 4 * H, 4 * H, SAVED, l, t, "saved");
        reads(p.dy + r * p.dy_rs, H, INPUT, 0, 0, "dy");
        if (l < 2) reads(p.dx_in + (long long)r * H, H, DX, l + 1, t, "dx of the layer above");
      }
      want(p.dy == c.dy[l] + (long long)t * c.dy_frame_stride[l] && p.dy_rs == c.dy_row_stride[l], "dy is not the layer's slot");
      if (t == T - 1) {
        want(p.dh_in == c.dhT[l], "the first step reads dhT");
        if (p.dh_in)
          for (int r = 0; r < N; r++) reads(p.dh_in + (long long)r * H, H, INPUT, 0, 0, "dhT");
      } else {
        for (int r = 0; r < N; r++) reads(p.dh_in + (long long)r * H, H, DH, l, t + 1, "dh of the step after");
      }
      if (t == 0) {
        want(p.prev == c.h0[l], "step 0 reads h0");
        if (p.prev)
          for (int r = 0; r < N; r++) reads(p.prev + r * p.prev_rs, H, INPUT, 0, 0, "h0");
      } else {
        for (int r = 0; r < N; r++) reads(p.prev + r * p.prev_rs, H, Y, l, t - 1, "y[t-1]");
      }
    }
  g_call_launches++, g_launch++;
}

// the step's y[t-1] (h0 at step 0) of a single layer
static void reads_prev(const float *prev, long long prev_rs, const float *h0, int t, int N, int H) {
  if (t == 0) {
    want(prev == h0, "step 0 reads h0");
    if (prev)
      for (int r = 0; r < N; r++) reads(prev + r * prev_rs, H, INPUT, 0, 0, "h0");
  } else {
    for (int r = 0; r < N; r++) reads(prev + r * prev_rs, H, Y, 0, t - 1, "y[t-1]");
  }
}

static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t, const RnGruStep &a) {
  const RNNoiseGruSeq &c = *g_seq_fwd;
  const int t = g_call_launches, T = c.n_frames, N = c.n_rows, H = c.hidden;
  want(t < T, "more than T launches");
  want(a.n_rows == N && a.H == H, "the sizes");
  check_grid(grid, block, 1, N, H);
  want(a.y == c.y + (long long)t * c.y_frame_stride && a.y_rs == c.y_row_stride, "y is not the step's slot");
  want(a.w_hh == c.w_hh && a.b_hh == c.b_hh, "the recurrent weights are not the call's");
  want(a.saved == g_saved + (long long)t * N * 4 * H, "saved is not [t]");
  for (int r = 0; r < N; r++) {
    writes(a.y + r * a.y_rs, H, Y, 0, t, "y");
    writes(a.saved + (long long)r * 4 * H, 4 * H, SAVED, 0, t, "saved");
  }
  want(a.gi == c.gi + (long long)t * c.gi_frame_stride && a.in_rs == c.gi_row_stride, "gi is not the step's slot");
  for (int r = 0; r < N; r++) reads(a.gi + r * a.in_rs, 3 * H, INPUT, 0, 0, "gi");
  reads_prev(a.prev, a.prev_rs, c.h0, t, N, H);
  g_call_launches++, g_launch++;
}

static void rn_stk_host_launch(dim3 grid, dim3 block, hipStream_t, const RnGruGradStep &a) {
  const RNNoiseGruSeqGrad &c = *g_seq_bwd;
  const int s = g_call_launches, T = c.n_frames, N = c.n_rows, H = c.hidden, t = T - 1 - s;
  want(s < T, "more than T launches");
  want(a.n_rows == N && a.H == H, "the sizes");
  check_grid(grid, block, 1, N, H);
  want(a.dh_out != nullptr && a.dh_out != a.dh_in, "dh_out is never dh_in");
  if (t == 0)
    want(a.dh_out == c.dh0, "the last step writes dh0");
  else
    want(a.dh_out == g_seq_scratch + (long long)(s & 1) * N * H, "the halves of the scratch alternate");
  want(a.dgh == c.dgh + (long long)t * N * 3 * H, "dgh is not [t]");
  want(a.dgi == c.dgi + (long long)t * c.dgi_frame_stride && a.dgi_rs == c.dgi_row_stride, "dgi is not the step's slot");
  for (int r = 0; r < N; r++) {
    writes(a.dgi + r * a.dgi_rs, 3 * H, DGI, 0, t, "dgi");
    writes(a.dgh + (long long)r * 3 * H, 3 * H, DGH, 0, t, "dgh");
    writes(a.dh_out + (long long)r * H, H, DH, 0, t, "dh");
  }
  want(a.w_hh == c.w_hh, "the weights are not the call's");
  want(a.saved == g_saved + (long long)t * N * 4 * H, "saved is not [t]");
  want(a.dy == c.dy + (long long)t * c.dy_frame_stride && a.dy_rs == c.dy_row_stride, "dy is not the step's slot");
  for (int r = 0; r < N; r++) {
    reads(a.saved + (long long)r * 4 * H, 4 * H, SAVED, 0, t, "saved");
    reads(a.dy + r * a.dy_rs, H, INPUT, 0, 0, "dy");
  }
  want(a.dh_in == g_seq_dh, "dh_in is what the launch before wrote (dhT at the first step)");
  if (t == T - 1) {
    if (a.dh_in)
      for (int r = 0; r < N; r++) reads(a.dh_in + (long long)r * H, H, INPUT, 0, 0, "dhT");
  } else {
    for (int r = 0; r < N; r++) reads(a.dh_in + (long long)r * H, H, DH, 0, t + 1, "dh of the step after");
  }
  reads_prev(a.prev, a.prev_rs, c.h0, t, N, H);
  g_seq_dh = a.dh_out;
  g_call_launches++, g_launch++;
}

namespace {
void all_written(const float *p, long fs, long rs, int T, int N, long M, Kind kind, int layer, const char *what) {
  for (int t = 0; t < T; t++)
    for (int r = 0; r < N; r++) {
      const Cell *c = cells(p + t * fs + r * rs, M, what);
      for (long i = 0; i < M; i++)
        if (c[i].kind != kind || c[i].layer != layer || c[i].step != t) fail(std::string(what) + ": not all written after the call");
    }
}

int run_case(int N, int T, int H, bool states, bool batch_first) {
  g_case = "N " + std::to_string(N) + " T " + std::to_string(T) + " H " + std::to_string(H) + (states ? ", states" : ", no states") +
           (batch_first ? ", slices of a batch-first concatenation" : ", frame-major buffers");
  g_launch = 0;
  const long NH = (long)N * H, Tn = T ? T : 1;
  size_t n_saved = 0, n_scratch = 0;
  RNNoiseGruStack f{};
  f.n_rows = N, f.n_frames = T, f.hidden = H;
  want(rnnoise_amd_gru_stack_workspace(&f, &n_saved, &n_scratch) == 0, "the workspace call");
  want(n_saved == (size_t)3 * T * N * 4 * H && n_scratch == (size_t)10 * N * H, "the workspace formulas");
  std::vector<Buf *> own;
  auto buf = [&](const char *name, size_t floats, bool input) {
    own.push_back(new Buf(name, floats ? floats : 4, input));
    g_bufs.push_back(own.back());
    return own.back()->mem;
  };
  float *gi0 = buf("gi0", Tn * NH * 3, true), *saved = buf("saved", n_saved, false), *scratch = buf("scratch", n_scratch, false);
  float *cat = buf("y (concatenation)", batch_first ? Tn * NH * 4 : 4, false), *dcat = buf("dy (concatenation)", batch_first ? Tn * NH * 4 : 4, true);
  f.gi0 = gi0, f.gi0_frame_stride = batch_first ? 3 * H : 3 * NH, f.gi0_row_stride = batch_first ? (long)Tn * 3 * H : 3 * H;
  RNNoiseGruStackGrad g{};
  g.n_rows = N, g.n_frames = T, g.hidden = H;
  for (int l = 0; l < 3; l++) {
    f.w_hh[l] = buf("w_hh", 3L * H * H, true), f.b_hh[l] = buf("b_hh", 3 * H, true);
    if (l) f.w_ih[l] = buf("w_ih", 3L * H * H, true), f.b_ih[l] = buf("b_ih", 3 * H, true);
    if (states) f.h0[l] = buf("h0", NH, true), g.dhT[l] = buf("dhT", NH, true);
    if (batch_first) {
      f.y[l] = cat + (l + 1) * H, f.y_frame_stride[l] = 4 * H, f.y_row_stride[l] = (long)Tn * 4 * H;
      g.dy[l] = dcat + (l + 1) * H;
    } else {
      f.y[l] = buf("y", Tn * NH, false), f.y_frame_stride[l] = NH, f.y_row_stride[l] = H;
      g.dy[l] = buf("dy", Tn * NH, true);
    }
    g.dy_frame_stride[l] = g.y_frame_stride[l] = f.y_frame_stride[l], g.dy_row_stride[l] = g.y_row_stride[l] = f.y_row_stride[l];
    g.y[l] = f.y[l], g.w_hh[l] = f.w_hh[l], g.w_ih[l] = f.w_ih[l], g.h0[l] = f.h0[l];
    g.dgi[l] = buf("dgi", Tn * NH * 3, false), g.dgh[l] = buf("dgh", Tn * NH * 3, false), g.dh0[l] = buf("dh0", NH, false);
  }
  g.dgi0_frame_stride = f.gi0_frame_stride, g.dgi0_row_stride = f.gi0_row_stride;
  want(rnnoise_amd_gru_stack_check(&f) == 0 && rnnoise_amd_gru_stack_grad_check(&g) == 0, "the checks accept the case");

  g_fwd = &f, g_saved = saved, g_call_launches = 0;
  want(rnnoise_amd_gru_stack_forward_device(1, &f, saved, nullptr) == 0, "the forward call");
  want(g_call_launches == (T ? T + 2 : 0), "forward: T + 2 launches");
  want(g_shim_device == 0, "the device is restored");
  for (int l = 0; l < 3; l++) {
    all_written(f.y[l], f.y_frame_stride[l], f.y_row_stride[l], T, N, H, Y, l, "y");
    all_written(saved + (long)l * T * NH * 4, NH * 4, 4 * H, T, N, 4 * H, SAVED, l, "saved");
  }
  g_bwd = &g, g_call_launches = 0;
  want(rnnoise_amd_gru_stack_backward_device(1, &g, saved, scratch, nullptr) == 0, "the backward call");
  want(g_call_launches == (T ? T + 2 : 0), "backward: T + 2 launches");
  for (int l = 0; l < 3; l++) {
    all_written(g.dgi[l], l ? NH * 3 : g.dgi0_frame_stride, l ? 3 * H : g.dgi0_row_stride, T, N, 3 * H, DGI, l, "dgi");
    all_written(g.dgh[l], NH * 3, 3 * H, T, N, 3 * H, DGH, l, "dgh");
    if (T) all_written(g.dh0[l], 0, H, 1, N, H, DH, l, "dh0");
  }
  // refused and unreachable: nothing is launched
  g_call_launches = 0;
  want(rnnoise_amd_gru_stack_forward_device(2, &f, saved, nullptr) == (T ? -1 : 0), "a device that cannot be selected");
  RNNoiseGruStack bad = f;
  bad.hidden = H + 8;
  want(rnnoise_amd_gru_stack_forward_device(0, &bad, saved, nullptr) == -1 && g_call_launches == 0, "a refused call launches nothing");
  if (T && batch_first) {  // two layers' outputs on one another
    bad = f, bad.y[2] = f.y[1];
    want(rnnoise_amd_gru_stack_check(&bad) == -1, "overlapping outputs are refused");
  }
  g_bufs.clear();
  for (Buf *b : own) delete b;
  return 1;
}

// the single-layer library on the same shapes
int run_seq_case(int N, int T, int H, bool states, bool batch_first) {
  g_case = "single layer, N " + std::to_string(N) + " T " + std::to_string(T) + " H " + std::to_string(H) + (states ? ", states" : ", no states") +
           (batch_first ? ", a slice of a batch-first concatenation" : ", frame-major buffers");
  g_launch = 0;
  const long NH = (long)N * H, Tn = T ? T : 1;
  size_t n_saved = 0, n_scratch = 0;
  RNNoiseGruSeq f{};
  f.n_rows = N, f.n_frames = T, f.hidden = H;
  want(rnnoise_amd_gru_workspace(&f, &n_saved, &n_scratch) == 0, "the workspace call");
  want(n_saved == (size_t)T * N * 4 * H && n_scratch == (size_t)2 * N * H, "the workspace formulas");
  std::vector<Buf *> own;
  auto buf = [&](const char *name, size_t floats, bool input) {
    own.push_back(new Buf(name, floats ? floats : 4, input));
    g_bufs.push_back(own.back());
    return own.back()->mem;
  };
  float *saved = buf("saved", n_saved, false), *scratch = buf("scratch", n_scratch, false);
  f.gi = buf("gi", Tn * NH * 3, true), f.gi_frame_stride = batch_first ? 3 * H : 3 * NH, f.gi_row_stride = batch_first ? (long)Tn * 3 * H : 3 * H;
  f.w_hh = buf("w_hh", 3L * H * H, true), f.b_hh = buf("b_hh", 3 * H, true);
  RNNoiseGruSeqGrad g{};
  g.n_rows = N, g.n_frames = T, g.hidden = H;
  if (states) f.h0 = buf("h0", NH, true), g.dhT = buf("dhT", NH, true);
  if (batch_first) {  // slice 1 of a [N][T][4H] concatenation
    f.y = buf("y (concatenation)", Tn * NH * 4, false) + H, f.y_frame_stride = 4 * H, f.y_row_stride = (long)Tn * 4 * H;
    g.dy = buf("dy (concatenation)", Tn * NH * 4, true) + H;
  } else {
    f.y = buf("y", Tn * NH, false), f.y_frame_stride = NH, f.y_row_stride = H;
    g.dy = buf("dy", Tn * NH, true);
  }
  g.dy_frame_stride = g.y_frame_stride = f.y_frame_stride, g.dy_row_stride = g.y_row_stride = f.y_row_stride;
  g.y = f.y, g.w_hh = f.w_hh, g.h0 = f.h0;
  g.dgi = buf("dgi", Tn * NH * 3, false), g.dgi_frame_stride = f.gi_frame_stride, g.dgi_row_stride = f.gi_row_stride;
  g.dgh = buf("dgh", Tn * NH * 3, false), g.dh0 = buf("dh0", NH, false);
  want(rnnoise_amd_gru_check(&f) == 0 && rnnoise_amd_gru_grad_check(&g) == 0, "the checks accept the case");

  g_seq_fwd = &f, g_saved = saved, g_call_launches = 0;
  want(rnnoise_amd_gru_forward_device(1, &f, saved, nullptr) == 0, "the forward call");
  want(g_call_launches == T, "forward: T launches");
  want(g_shim_device == 0, "the device is restored");
  all_written(f.y, f.y_frame_stride, f.y_row_stride, T, N, H, Y, 0, "y");
  all_written(saved, NH * 4, 4 * H, T, N, 4 * H, SAVED, 0, "saved");
  g_seq_bwd = &g, g_seq_scratch = scratch, g_seq_dh = g.dhT, g_call_launches = 0;
  want(rnnoise_amd_gru_backward_device(1, &g, saved, scratch, nullptr) == 0, "the backward call");
  want(g_call_launches == T, "backward: T launches");
  all_written(g.dgi, g.dgi_frame_stride, g.dgi_row_stride, T, N, 3 * H, DGI, 0, "dgi");
  all_written(g.dgh, NH * 3, 3 * H, T, N, 3 * H, DGH, 0, "dgh");
  if (T) all_written(g.dh0, 0, H, 1, N, H, DH, 0, "dh0");
  // refused and unreachable: nothing is launched
  g_call_launches = 0;
  want(rnnoise_amd_gru_forward_device(2, &f, saved, nullptr) == (T ? -1 : 0), "a device that cannot be selected");
  RNNoiseGruSeq bad = f;
  bad.hidden = H + 8;
  want(rnnoise_amd_gru_forward_device(0, &bad, saved, nullptr) == -1 && g_call_launches == 0, "a refused call launches nothing");
  if (states) {
    RNNoiseGruSeqGrad on = g;
    on.dhT = g.dh0;
    want(rnnoise_amd_gru_grad_check(&on) == -1, "dh0 on dhT is refused");
  }
  g_bufs.clear();
  for (Buf *b : own) delete b;
  return 1;
}
}  // namespace

int main() {
  int cases = 0;
  for (int H : {16, 32})
    for (int N : {1, 17})
      for (int T : {0, 1, 2, 3, 4, 7})
        for (int states = 0; states < 2; states++)
          for (int batch_first = 0; batch_first < 2; batch_first++) {
            cases += run_case(N, T, H, states != 0, batch_first != 0);
            cases += run_seq_case(N, T, H, states != 0, batch_first != 0);
          }
  printf("ok %d\n", cases);
  return 0;
}
