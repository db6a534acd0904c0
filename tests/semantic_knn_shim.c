/* test shim: host restatement of the KNN back-projection's arithmetic specification (semantic_suma_amd/csrc/
 * k_semantic_knn.hip header), built with gcc -ffp-contract=off against include/suma_detmath.h.  It follows the
 * specification's own form -- a sort of the window by its keys and an array of vote counts -- not the kernel's sweeps
 * and bit-sliced counters.  The GPU tests compare the kernels with it bit for bit; tests/test_semantic_knn_host.py pins
 * it with known answers and an independent numpy restatement. */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../include/suma_detmath.h"
#include "../include/suma_hip.h" /* suma_semantic_params, suma_semantic_knn */

#define KNN_MAX 81
#define NONE (-1)

/* 0 = valid, else the number of the rule broken: 1 search, 2 k, 3 sigma, 4 cutoff */
int knn_check(const suma_semantic_knn* kp) {
  if (kp->search < 1 || kp->search > 9 || kp->search % 2 == 0) return 1;
  if (kp->k < 1 || kp->k > kp->search * kp->search) return 2;
  if (!(kp->sigma > 0.0f) || !isfinite(kp->sigma)) return 3;
  if (!isfinite(kp->cutoff)) return 4;
  return 0;
}

/* rule 4: w[S * S] */
void knn_weights(uint32_t S, float sigma, float* w) {
  const int R = (int)(S - 1) / 2;
  double e[KNN_MAX], sum = 0.0;
  for (uint32_t t = 0; t < S * S; ++t) {
    const int dy = (int)(t / S) - R, dx = (int)(t % S) - R;
    e[t] = exp(-(double)(dx * dx + dy * dy) / (2.0 * (double)sigma * (double)sigma));
    sum += e[t];
  }
  for (uint32_t t = 0; t < S * S; ++t) w[t] = (float)(1.0 - e[t] / sum);
}

static float depth_of(const float* pt) {
  return sdm_sqrt(__builtin_fmaf(pt[2], pt[2], __builtin_fmaf(pt[1], pt[1], pt[0] * pt[0])));
}

/* rules 1 and 2 per pixel: range[P], cls[P] (-1 = none), prob[P] */
void knn_pixels(const suma_semantic_params* sp, const float* points, uint32_t n, const float* scores, int logits,
                const int32_t* proj_idx, float* range, int32_t* cls, float* prob) {
  const uint32_t P = sp->width * sp->height, C = sp->n_classes;
  for (uint32_t p = 0; p < P; ++p) {
    const int32_t idx = proj_idx[p];
    range[p] = (idx >= 0 && (uint32_t)idx < n) ? depth_of(points + 4 * (size_t)idx) : INFINITY;
    float s[SUMA_SEM_MAX_CLASSES];
    for (uint32_t j = 0; j < C; ++j) s[j] = scores[(size_t)j * P + p];
    if (logits) {
      float m = -INFINITY;
      for (uint32_t j = 0; j < C; ++j) m = (s[j] > m) ? s[j] : m;
      float sum = 0.0f;
      for (uint32_t j = 0; j < C; ++j) {
        s[j] = sdm_exp(s[j] - m);
        sum = sum + s[j];
      }
      for (uint32_t j = 0; j < C; ++j) s[j] = s[j] / sum;
    }
    int32_t c = NONE;
    float pr = 0.0f;
    for (uint32_t j = 0; j < C; ++j)
      if (pr <= s[j]) {
        c = (int32_t)j;
        pr = s[j];
      }
    cls[p] = c;
    prob[p] = pr;
  }
}

/* a before b in the key (d, t != t_c, t) */
static int key_less(float da, int ta, float db, int tb, int tc) {
  if (da != db) return da < db;
  if ((ta != tc) != (tb != tc)) return ta == tc;
  return ta < tb;
}

/* prob order of rule 8: -0 below +0 */
static int prob_greater(float a, float b) { return a > b || (a == b && signbit(b) && !signbit(a)); }

void sem_unproject_knn(const suma_semantic_params* sp, const suma_semantic_knn* kp, const float* points,
                       const float* scores, int logits, const int32_t* pixel, const int32_t* proj_idx, uint32_t n,
                       float* labels, float* probs, float* range, int32_t* cls, float* prob) {
  const int32_t W = (int32_t)sp->width, H = (int32_t)sp->height;
  const uint32_t P = sp->width * sp->height;
  const int S = (int)kp->search, R = (S - 1) / 2, S2 = S * S, tc = (S2 - 1) / 2, K = (int)kp->k;
  float w[KNN_MAX];
  knn_weights(kp->search, kp->sigma, w);
  knn_pixels(sp, points, n, scores, logits, proj_idx, range, cls, prob);
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t pix = pixel[i];
    labels[i] = 0.0f;
    probs[i] = 0.0f;
    if (pix < 0 || (uint32_t)pix >= P) continue;
    const float ri = depth_of(points + 4 * (size_t)i);
    if (!(ri > 0.0f && ri <= FLT_MAX)) continue; /* rule 3: not a point the projection gives a pixel */
    const int32_t v = pix / W, u = pix % W;
    float d[KNN_MAX], pr[KNN_MAX];
    int32_t c[KNN_MAX];
    int order[KNN_MAX];
    for (int t = 0; t < S2; ++t) {
      const int32_t yy = v + t / S - R, xx = u + t % S - R;
      float rt = 0.0f;
      c[t] = NONE;
      pr[t] = 0.0f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        rt = range[yy * W + xx];
        c[t] = cls[yy * W + xx];
        pr[t] = prob[yy * W + xx];
      }
      d[t] = (t == tc) ? 0.0f : fabsf(rt - ri) * w[t];
      order[t] = t;
    }
    /* insertion sort of the window by key */
    for (int a = 1; a < S2; ++a)
      for (int b = a; b > 0 && key_less(d[order[b]], order[b], d[order[b - 1]], order[b - 1], tc); --b) {
        const int x = order[b];
        order[b] = order[b - 1];
        order[b - 1] = x;
      }
    int votes[SUMA_SEM_MAX_CLASSES] = {0};
    int any = 0;
    for (int q = 0; q < K; ++q) {
      const int t = order[q];
      if (c[t] != NONE && c[t] != 0 && (kp->cutoff <= 0.0f || d[t] <= kp->cutoff)) {
        votes[c[t]] += 1;
        any = 1;
      }
    }
    if (!any) continue;
    int win = 0;
    for (int j = 1; j < SUMA_SEM_MAX_CLASSES; ++j)
      if (votes[j] > votes[win]) win = j;
    int have = 0;
    float best = 0.0f;
    for (int q = 0; q < K; ++q) {
      const int t = order[q];
      if (c[t] == win && (kp->cutoff <= 0.0f || d[t] <= kp->cutoff) && (!have || prob_greater(pr[t], best))) {
        best = pr[t];
        have = 1;
      }
    }
    labels[i] = (float)sp->label_map[win];
    probs[i] = best;
  }
}

void knn_layout(uint64_t* out) {
  out[0] = sizeof(suma_semantic_knn);
  out[1] = offsetof(suma_semantic_knn, search);
  out[2] = offsetof(suma_semantic_knn, k);
  out[3] = offsetof(suma_semantic_knn, sigma);
  out[4] = offsetof(suma_semantic_knn, cutoff);
}
