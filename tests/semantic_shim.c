/* test shim: host restatement of the semantic front end's arithmetic specification (semantic_suma_amd/csrc/k_semantic.hip
 * header), built with gcc -ffp-contract=off against include/suma_detmath.h.  The GPU tests compare the kernels with it
 * bit for bit; tests/test_semantic_host.py pins it with known answers. */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../include/suma_detmath.h"
#include "../include/suma_hip.h" /* suma_semantic_params */

/* points: n x 4 floats; input: 5 x H x W; pixel: n; proj_idx: H x W */
void sem_project(const suma_semantic_params* sp, const float* points, uint32_t n, float* input, int32_t* pixel,
                 int32_t* proj_idx) {
  const int32_t W = (int32_t)sp->width, H = (int32_t)sp->height;
  const uint32_t P = sp->width * sp->height;
  const float Wf = (float)sp->width, Hf = (float)sp->height, pi = (float)M_PI;
  const float fdown = (float)(fabs((double)sp->fov_down) * M_PI / 180.0);
  const float fov = (float)((fabs((double)sp->fov_up) + fabs((double)sp->fov_down)) * M_PI / 180.0);
  float inv_std[SUMA_SEM_CHANNELS];
  for (int c = 0; c < SUMA_SEM_CHANNELS; ++c) inv_std[c] = (float)(1.0 / (double)sp->stds[c]);
  for (uint32_t p = 0; p < P; ++p) proj_idx[p] = -1;
  float* best = input; /* plane 0 holds the winning depth until the resolve below */
  for (uint32_t i = 0; i < n; ++i) {
    const float x = points[4 * i], y = points[4 * i + 1], z = points[4 * i + 2];
    const float depth = sdm_sqrt(__builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
    int32_t pix = -1;
    if (depth > 0.0f && depth <= FLT_MAX) {
      const float yaw = -sdm_atan2(y, x);
      const float pitch = sdm_asin(z / depth);
      float fu = sdm_floor((0.5f * (yaw / pi + 1.0f)) * Wf);
      float fv = sdm_floor((1.0f - (pitch + fdown) / fov) * Hf);
      fu = (fu >= 0.0f) ? fu : 0.0f;
      fv = (fv >= 0.0f) ? fv : 0.0f;
      const int32_t u = (fu < Wf) ? (int32_t)fu : W - 1;
      const int32_t v = (fv < Hf) ? (int32_t)fv : H - 1;
      pix = v * W + u;
      /* in point order, strictly nearer replaces: equal ranges keep the lower index */
      if (proj_idx[pix] < 0 || depth < best[pix]) {
        proj_idx[pix] = (int32_t)i;
        best[pix] = depth;
      }
    }
    pixel[i] = pix;
  }
  for (uint32_t p = 0; p < P; ++p) {
    float o[SUMA_SEM_CHANNELS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (proj_idx[p] >= 0) {
      const float* pt = points + 4 * (size_t)proj_idx[p];
      const float v[SUMA_SEM_CHANNELS] = {best[p], pt[0], pt[1], pt[2], pt[3]};
      for (int c = 0; c < SUMA_SEM_CHANNELS; ++c) o[c] = (v[c] - sp->means[c]) * inv_std[c];
    }
    for (int c = 0; c < SUMA_SEM_CHANNELS; ++c) input[(size_t)c * P + p] = o[c];
  }
}

/* scores: C x H x W planar */
void sem_unproject(const suma_semantic_params* sp, const float* scores, int logits, const int32_t* pixel, uint32_t n,
                   float* labels, float* probs) {
  const uint32_t P = sp->width * sp->height, C = sp->n_classes;
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t pix = pixel[i];
    float label = 0.0f, prob = 0.0f;
    if (pix >= 0 && (uint32_t)pix < P) {
      float s[SUMA_SEM_MAX_CLASSES];
      for (uint32_t j = 0; j < C; ++j) s[j] = scores[(size_t)j * P + (uint32_t)pix];
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
      for (uint32_t j = 0; j < C; ++j)
        if (prob <= s[j]) {
          label = (float)sp->label_map[j];
          prob = s[j];
        }
    }
    labels[i] = label;
    probs[i] = prob;
  }
}

/* layout of suma_semantic_params as the C compiler sees it: size, then the offsets of its fields in order */
void sem_layout(uint64_t* out) {
  out[0] = sizeof(suma_semantic_params);
  out[1] = offsetof(suma_semantic_params, width);
  out[2] = offsetof(suma_semantic_params, height);
  out[3] = offsetof(suma_semantic_params, fov_up);
  out[4] = offsetof(suma_semantic_params, fov_down);
  out[5] = offsetof(suma_semantic_params, means);
  out[6] = offsetof(suma_semantic_params, stds);
  out[7] = offsetof(suma_semantic_params, n_classes);
  out[8] = offsetof(suma_semantic_params, label_map);
}
