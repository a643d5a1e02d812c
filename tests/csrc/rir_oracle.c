/* rir_oracle.c -- TEST INFRASTRUCTURE: the RIR filtering of the reference's feature dumper (src/dump_features.c:51-144, :449-465)
 * restated in plain C, for any number of frames: what the GPU tests compare rnnoise_batch_train_rir_* against, itself compared with the
 * reference where its sources are (tests/test_train_rir_cpu.py).  Compile with -O2 -ffp-contract=off.
 *
 * The transform is kiss_fft at 65,536 points: eight radix-4 stages over an array in base-4 digit-reversed order, the first one in
 * the twiddle-free form, whose sums come in another order than the general form's would with a twiddle of 1. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define N 65536
#define HALF (N / 2)
#define FRAME 480

typedef struct {
  float r, i;
} cpx;

static cpx tw[N];
static int rev[N];
static int ready;

static void init(void) {
  if (ready) return;
  for (int i = 0; i < N; i++) {
    const double pi = 3.14159265358979323846264338327;
    double phase = (-2 * pi / N) * i;
    tw[i].r = (float)cos(phase);
    tw[i].i = (float)sin(phase);
    int v = i, r = 0;
    for (int d = 0; d < 8; d++) {
      r = r << 2 | (v & 3);
      v >>= 2;
    }
    rev[i] = r;
  }
  ready = 1;
}

static cpx mul(cpx a, cpx b) {
  cpx m;
  m.r = a.r * b.r - a.i * b.i;
  m.i = a.r * b.i + a.i * b.r;
  return m;
}

/* the stages on f[], already in digit-reversed order */
static void stages(cpx *f) {
  for (int m = 1; m < N; m *= 4) {
    int stride = N / (4 * m);
    for (int g = 0; g < N; g += 4 * m)
      for (int j = 0; j < m; j++) {
        cpx *a = f + g + j, *b = a + m, *c = a + 2 * m, *d = a + 3 * m;
        cpx s0 = *b, s1 = *c, s2 = *d, s3, s4, s5;
        if (m > 1) {
          s0 = mul(s0, tw[j * stride]);
          s1 = mul(s1, tw[2 * j * stride]);
          s2 = mul(s2, tw[3 * j * stride]);
        }
        s5.r = a->r - s1.r;
        s5.i = a->i - s1.i;
        a->r += s1.r;
        a->i += s1.i;
        s3.r = s0.r + s2.r;
        s3.i = s0.i + s2.i;
        s4.r = s0.r - s2.r;
        s4.i = s0.i - s2.i;
        c->r = a->r - s3.r;
        c->i = a->i - s3.i;
        a->r += s3.r;
        a->i += s3.i;
        b->r = s5.r + s4.i;
        b->i = s5.i - s4.r;
        d->r = s5.r - s4.i;
        d->i = s5.i + s4.r;
      }
  }
}

static void fft(const cpx *in, cpx *out) {
  const float scale = 1.f / N;
  for (int i = 0; i < N; i++) {
    out[rev[i]].r = scale * in[i].r;
    out[rev[i]].i = scale * in[i].i;
  }
  stages(out);
}

static void ifft(const cpx *in, cpx *out) {
  for (int i = 0; i < N; i++) {
    out[rev[i]].r = in[i].r;
    out[rev[i]].i = -in[i].i;
  }
  stages(out);
  for (int i = 0; i < N; i++) out[i].i = -out[i].i;
}

void riro_twiddles(float *out) {
  init();
  memcpy(out, tw, sizeof(tw));
}

void riro_bitrev(int *out) {
  init();
  memcpy(out, rev, sizeof(rev));
}

void riro_fft(const float *in, float *out, int inverse) {
  init();
  if (inverse) ifft((const cpx *)in, (cpx *)out);
  else fft((const cpx *)in, (cpx *)out);
}

/* load_rir (:63-88) from memory: the first len <= 32768 samples of rir[] -> spec[65536][2] */
void riro_load(const float *rir, int len, int early, float *spec) {
  init();
  cpx *x = calloc(N, sizeof(*x));
  for (int i = 0; i < len; i++) {
    float v = rir[i];
    if (early && i >= 480 && i < 720) v *= (1 - (i - 480) / 240.f);
    if (early && i >= 720) v = 0;
    x[i].r = v;
  }
  fft(x, (cpx *)spec);
  free(x);
}

/* rir_filter_sequence (:119-144) on audio[480 * n_frames], in place */
void riro_filter(float *audio, int n_frames, const float *spec) {
  init();
  const cpx *Y = (const cpx *)spec;
  const long total = (long)FRAME * n_frames;
  cpx *x = calloc(N, sizeof(*x)), *X = calloc(N, sizeof(*X)), *y = calloc(N, sizeof(*y));
  for (long at = 0; at < total; at += HALF) {
    long have = total - at < HALF ? total - at : HALF;
    memcpy(x, x + HALF, HALF * sizeof(*x));
    for (long j = 0; j < HALF; j++) x[HALF + j].r = j < have ? audio[at + j] : 0;
    fft(x, X);
    for (int j = 0; j < N; j++) {
      cpx t = mul(X[j], Y[j]);
      X[j].r = t.r * N / 2;
      X[j].i = t.i * N / 2;
    }
    ifft(X, y);
    for (long j = 0; j < have; j++) audio[at + j] = y[HALF + j].r;
  }
  free(x);
  free(X);
  free(y);
}

/* :457 and :463 */
void riro_clip_quantize(float *x, long n, int clip, int quantize) {
  for (long j = 0; j < n; j++) {
    float t = x[j];
    if (clip) {
      t = -32767.f > t ? -32767.f : t;
      t = 32767.f < t ? 32767.f : t;
    }
    if (quantize) t = floor(.5f + t);
    x[j] = t;
  }
}
