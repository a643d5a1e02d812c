// tests/test_out_tables_cpu.py: the plan of a step of a batch with output tables (rnnoise_amd/csrc/dispatch.h: RnStepShape::split),
// without a GPU.  A stand-alone program that checks itself over the shape sweep of the other dispatch harnesses, under every knob
// set they use; it prints one line per failure and a summary, and exits 0 when there is none.
//   1. a shape without output tables plans as before there were any: parent_plan below is the rule as it stood, restated, and every
//      field it gives must be the field rn_plan gives; the new field, k3_rs, is that shape's low_rate;
//   2. an out-only shape (output tables, 48 kHz linear inputs) keeps every form of the same shape without tables -- the lane = stream
//      K0 above hp_one_max among them -- and sets K3's epilogue;
//   3. an input-only description (no output tables) plans as today whatever the output members hold, and with output tables the
//      high-pass form follows the input side alone and K3's epilogue the output side alone.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../rnnoise_amd/csrc/dispatch.h"

struct ParentPlan {
  RnHpForm hp;
  RnK1Form k1;
  RnNnForm nn;
  RnGruForm gru;
  RnK3Form k3;
};

// the rule before output tables: it reads the members a shape had then, and nothing else
static ParentPlan parent_plan(const RnKnobs &k, const RnStepShape &s) {
  ParentPlan p;
  p.hp = s.listed || s.low_rate || s.companded || s.channels > 1 || s.n <= k.hp_one_max ? RN_HP_ONE_WAVE : RN_HP_LANES;
  p.k1 = s.listed || s.per_stream || k.k1_spw == 1 || (k.k1_spw == 0 && s.n < 2560) ? RN_K1_SINGLE : RN_K1_FOUR;
  const int tiles = (s.n + 15) / 16;
  const RnNnForm tile = k.tile_waves == 16 || (k.tile_waves != 8 && !s.pipelined && tiles <= s.cus) ? RN_NN_TILE16 : RN_NN_TILE8;
  if (s.listed) p.nn = s.nn_path == 0 ? RN_NN_ONE : tile;
  else if (s.whole && (s.nn_path == 2 || (s.nn_path == 1 && s.n >= k.nn_layers_min))) p.nn = RN_NN_LAYERS;
  else if (s.nn_path >= 1) p.nn = tile;
  else p.nn = s.n <= k.nn_one_max ? RN_NN_ONE : RN_NN_VECTOR;
  const int groups = (tiles + 3) / 4;
  p.gru = k.gru == 4 ? RN_GRU_W4 : k.gru == 8 ? RN_GRU_W8 : k.gru ? RN_GRU_UNKNOWN : groups > s.cus ? RN_GRU_W4 : RN_GRU_W8;
  p.k3 = s.n <= 256 ? RN_K3_FEW : RN_K3_WIDE;
  return p;
}

static int failures = 0;
static void fail(const char *what, const RnStepShape &s, int knobs) {
  if (failures++ < 20)
    fprintf(stderr, "FAIL %s: n=%d whole=%d cus=%d path=%d pipelined=%d per_stream=%d low_rate=%d listed=%d companded=%d channels=%d knobs=%d\n",
            what, s.n, s.whole, s.cus, s.nn_path, s.pipelined, s.per_stream, s.low_rate, s.listed, s.companded, s.channels, knobs);
}
static bool same_forms(const RnPlan &a, const ParentPlan &b) {
  return a.hp == b.hp && a.k1 == b.k1 && a.nn == b.nn && a.gru == b.gru && a.k3 == b.k3;
}
static bool same_forms(const RnPlan &a, const RnPlan &b) {
  return a.hp == b.hp && a.k1 == b.k1 && a.nn == b.nn && a.gru == b.gru && a.k3 == b.k3;
}

int main() {
  // the sizes tests/test_dispatch_cpu.py pins a boundary at, both sides of each (tests/test_stream_formats_cpu.py: SIZES)
  static const int sizes[] = {1,    15,   16,   17,   99,   100,  101,  255,   256,   257,   511,   512,   513,   1600,  1601, 2047, 2048,
                              2049, 2559, 2560, 2561, 4096, 4097, 6400, 6401,  8192,  10239, 10240, 12288, 16384, 16385, 40037, 65536};
  // the knob sets of the other harnesses: the defaults, two high-pass switches, and everything else forced
  RnKnobs base{};
  base.nn_layers_min = 10240, base.nn_one_max = 512, base.hp_one_max = 2048, base.k1_spw = 0, base.tile_waves = 0, base.gru = 0, base.pipe = 0;
  std::vector<RnKnobs> knobs(4, base);
  knobs[1].hp_one_max = 0;
  knobs[2].hp_one_max = 100;
  knobs[3].k1_spw = 4, knobs[3].tile_waves = 8, knobs[3].nn_layers_min = 100, knobs[3].nn_one_max = 0;
  long shapes = 0, lanes_kept = 0;
  for (size_t ki = 0; ki < knobs.size(); ki++) {
    const RnKnobs &k = knobs[ki];
    for (int n : sizes)
      for (int whole = 0; whole < 2; whole++)
        for (int cus : {256, 100})
          for (int path = 0; path < 3; path++)
            for (int pipelined = 0; pipelined < 2; pipelined++)
              for (int per_stream = 0; per_stream < 2; per_stream++)
                for (int low_rate = 0; low_rate < 2; low_rate++)
                  for (int listed = 0; listed <= per_stream; listed++)  // (a list call is always in per-stream phase)
                    for (int companded = 0; companded < 2; companded++)
                      for (int channels : {1, 2}) {
                        RnStepShape s{n, whole != 0, cus, path, pipelined != 0, per_stream != 0, low_rate != 0};
                        s.listed = listed != 0;
                        s.companded = companded != 0;
                        s.channels = channels;
                        shapes++;
                        // 1. no output tables: the parent's plan, whatever the output members hold
                        const ParentPlan want = parent_plan(k, s);
                        for (int junk = 0; junk < 4; junk++) {
                          RnStepShape t = s;
                          t.out_low_rate = junk & 1;
                          t.out_companded = (junk & 2) != 0;
                          const RnPlan p = rn_plan(k, t);
                          if (!same_forms(p, want)) fail("a shape without output tables plans as before", s, (int)ki);
                          if (p.k3_rs != s.low_rate) fail("without output tables K3's epilogue is the one description's low_rate", s, (int)ki);
                        }
                        // 2. / 3. output tables: the forms of the same shape without them, the high-pass by the input side alone,
                        // the epilogue by the output side alone
                        for (int out_low = 0; out_low < 2; out_low++)
                          for (int out_comp = 0; out_comp < 2; out_comp++) {
                            RnStepShape t = s;
                            t.split = true;
                            t.out_low_rate = out_low != 0;
                            t.out_companded = out_comp != 0;
                            const RnPlan p = rn_plan(k, t);
                            if (!same_forms(p, want)) fail("output tables move no form", s, (int)ki);
                            if (p.k3_rs != (out_low != 0)) fail("K3's epilogue comes from the output side", s, (int)ki);
                          }
                        // the out-only batch: 48 kHz linear inputs, tables on the way out -- the plan of the plain batch, with the epilogue
                        if (!low_rate && !companded) {
                          RnStepShape t = s;
                          t.split = true;
                          t.out_low_rate = true;
                          const RnPlan p = rn_plan(k, t), plain = rn_plan(k, s);
                          if (!same_forms(p, plain) || !p.k3_rs || plain.k3_rs) fail("an out-only shape is the plain shape with the epilogue", s, (int)ki);
                          const bool lanes = !listed && channels == 1 && n > k.hp_one_max;
                          if ((p.hp == RN_HP_LANES) != lanes) fail("an out-only shape keeps the lane high-pass above hp_one_max", s, (int)ki);
                          lanes_kept += p.hp == RN_HP_LANES;
                          // ... where the same tables on the input side force the one-wave form
                          RnStepShape u = s;
                          u.low_rate = true;
                          if (rn_plan(k, u).hp != RN_HP_ONE_WAVE) fail("an input-side table forces the one-wave high-pass", s, (int)ki);
                        }
                      }
  }
  // the two sizes the issue names, on the default knobs
  {
    RnStepShape s{2049, true, 256, 1, false, false, false};
    s.split = true;
    s.out_low_rate = true;
    const RnPlan p = rn_plan(base, s);
    if (p.hp != RN_HP_LANES || !p.k3_rs) fail("2,049 out-only streams: lanes and the epilogue", s, 0);
    s.n = 2048;
    if (rn_plan(base, s).hp != RN_HP_ONE_WAVE) fail("2,048 out-only streams: one wave per stream, as without tables", s, 0);
  }
  printf("%ld shapes, %ld out-only plans with the lane high-pass, %d failures\n", shapes, lanes_kept, failures);
  return failures ? 1 : 0;
}
