/*
 * place_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_place.hip restated on the host, sequentially:
 * the descriptor of a vertex map, the column norms, the distance of two descriptors under every shift, the top-K with
 * the exclusion window, the yaw of a shift and the pose hypothesis of a match.  Compiled by the tests with
 * gcc -O2 -ffp-contract=off; the library's cells, norms, distances, shifts and matches must equal it to the bit.  It
 * shares no code with the library: the structures are declared again here, and the only header is the public fp32 math
 * specification (include/suma_detmath.h: sdm_atan2, sdm_cos_d, sdm_sin_d).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "suma_detmath.h"

typedef struct {
  float x, y, z, w;
} float4_t;

typedef struct {
  uint32_t index, id;
  float distance;
  int32_t shift;
  float yaw;
} match_t;

#define TWO_PI (2.0f * SUMA_PI_F)

static uint32_t label_of(float r) {
  const float t = r * 255.0f + 0.5f;
  return (t >= 0.0f && t < 260.0f) ? (uint32_t)t : 0u;
}

/* cells: S x R floats, sector-major */
void place_shim_describe(const float4_t* vertex, const float4_t* semantic, uint32_t n_texels, int R, int S, float max_range,
                         float height_offset, const uint8_t* keep_label, float* cells) {
  for (int i = 0; i < S * R; ++i) cells[i] = 0.0f;
  for (uint32_t t = 0; t < n_texels; ++t) {
    const float x = vertex[t].x, y = vertex[t].y, z = vertex[t].z;
    if (!(vertex[t].w > 0.0f)) continue;
    if (!keep_label[label_of(semantic[t].x)]) continue;
    const float d = sqrtf(x * x + y * y);
    if (!(d > 0.0f && d < max_range)) continue;
    int ring = (int)(d * ((float)R / max_range));
    if (ring > R - 1) ring = R - 1;
    float a = sdm_atan2(y, x);
    if (a < 0.0f) a = a + TWO_PI;
    int sector = (int)(a * ((float)S / TWO_PI));
    if (sector > S - 1) sector = S - 1;
    const float h = z + height_offset;
    if (!(h > 0.0f && h <= 1000.0f)) continue;
    if (h > cells[sector * R + ring]) cells[sector * R + ring] = h;
  }
}

void place_shim_norms(const float* cells, int S, int R, float* norms) {
  for (int j = 0; j < S; ++j) {
    float sum = 0.0f;
    for (int r = 0; r < R; ++r) {
      const float v = cells[j * R + r];
      sum = sum + v * v;
    }
    norms[j] = sqrtf(sum);
  }
}

/* the least distance over the shifts; *shift = the smallest shift that reaches it */
float place_shim_distance(const float* qc, const float* qn, const float* cc, const float* cn, int S, int R, int32_t* shift) {
  float best = 0.0f;
  int32_t best_s = 0;
  for (int s = 0; s < S; ++s) {
    float sum = 0.0f;
    uint32_t cnt = 0;
    for (int j = 0; j < S; ++j) {
      const int jq = (j + s) % S;
      if (qn[jq] > 0.0f && cn[j] > 0.0f) {
        float dot = 0.0f;
        for (int r = 0; r < R; ++r) dot = dot + qc[jq * R + r] * cc[j * R + r];
        sum = sum + dot / (qn[jq] * cn[j]);
        cnt += 1;
      }
    }
    const float dist = cnt ? 1.0f - sum / (float)cnt : 1.0f;
    if (s == 0 || dist < best) best = dist, best_s = s;
  }
  *shift = best_s;
  return best;
}

void place_shim_search(const float* cells, const float* norms, uint32_t n, const float* qc, const float* qn, int S, int R,
                       float* dist, int32_t* shift) {
  for (uint32_t e = 0; e < n; ++e)
    dist[e] = place_shim_distance(qc, qn, cells + (size_t)e * S * R, norms + (size_t)e * S, S, R, &shift[e]);
}

float place_shim_yaw(int32_t shift, int S) {
  const float D = TWO_PI / (float)S;
  return shift <= S / 2 ? -(float)shift * D : (float)(S - shift) * D;
}

/* the K best by (dist ascending, entry index ascending) among the entries whose id is outside [lo, hi]; returns how many */
uint32_t place_shim_topk(const float* dist, const int32_t* shift, const uint32_t* ids, uint32_t n, uint32_t lo, uint32_t hi,
                         uint32_t K, int S, match_t* out) {
  uint32_t m = 0;
  for (uint32_t e = 0; e < n; ++e) {
    if (lo <= hi && ids[e] >= lo && ids[e] <= hi) continue;
    /* insertion behind every kept match that is not worse: ascending e keeps the index order among equals */
    uint32_t at = m;
    while (at > 0 && dist[e] < out[at - 1].distance) --at;
    if (at >= K) continue;
    const uint32_t last = m < K ? m : K - 1;
    for (uint32_t k = last; k > at; --k) out[k] = out[k - 1];
    out[at].index = e, out[at].id = ids[e], out[at].distance = dist[e], out[at].shift = shift[e];
    out[at].yaw = place_shim_yaw(shift[e], S);
    if (m < K) ++m;
  }
  return m;
}

/* T * Rz(yaw), column-major doubles, every product ((a0 b0 + a1 b1) + a2 b2) + a3 b3 */
void place_shim_hypothesis(const double* T, float yaw, double* out) {
  double Rz[16];
  for (int i = 0; i < 16; ++i) Rz[i] = (i % 5 == 0) ? 1.0 : 0.0;
  const double cy = sdm_cos_d((double)yaw), sy = sdm_sin_d((double)yaw);
  Rz[0] = cy, Rz[1] = sy, Rz[4] = -sy, Rz[5] = cy;
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      out[4 * c + r] = ((T[r] * Rz[4 * c] + T[4 + r] * Rz[4 * c + 1]) + T[8 + r] * Rz[4 * c + 2]) + T[12 + r] * Rz[4 * c + 3];
}
