/*
 * object_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_objects.hip restated on the host, one texel
 * after the other: members, links, components by a flood fill from each unvisited member in ascending texel order (the
 * library labels by union-find with atomics and reduces by atomics; this walks a stack and sums in a loop), the records,
 * the id image and the counts.  Compiled by the tests with gcc -O2 -ffp-contract=off; the library's records, ids and
 * counts must equal it byte for byte.  It shares no code with the library; the structures are declared again here.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  float link_base, link_slope;
  uint32_t min_texels, max_objects;
} oparams_t;

typedef struct {
  uint32_t root, n_texels, label;
  float prob;
  uint32_t n_dynamic;
  float min[3], max[3], centroid[3];
  float r_min;
  uint32_t scan_id;
} object_t;

typedef struct {
  uint32_t n_texels, n_members, n_components, n_small, n_objects, stored;
} ocounts_t;

typedef struct {
  float x, y, z;
} v3;

static v3 mk3(float x, float y, float z) {
  v3 r = {x, y, z};
  return r;
}
static float dot3(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static float len3(v3 a) { return sqrtf(dot3(a, a)); }
static v3 sub3(v3 a, v3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 m4_point(const float* m, v3 p) {
  return mk3(fmaf(m[8], p.z, fmaf(m[4], p.y, m[0] * p.x)) + m[12], fmaf(m[9], p.z, fmaf(m[5], p.y, m[1] * p.x)) + m[13],
             fmaf(m[10], p.z, fmaf(m[6], p.y, m[2] * p.x)) + m[14]);
}
static float fmin_(float a, float b) { return (b < a) ? b : a; }
static float fclampf(float x, float lo, float hi) {
  const float t = (x < lo) ? lo : x;
  return (t > hi) ? hi : t;
}
static uint32_t world_label(float r) {
  const float t = r * 255.0f + 0.5f;
  return (t >= 0.0f && t < 260.0f) ? (uint32_t)t : 0u;
}
static int is_dynamic_label(float l) {
  return l == 10.0f || l == 11.0f || l == 13.0f || l == 15.0f || l == 18.0f || l == 20.0f || l == 30.0f || l == 31.0f ||
         l == 32.0f;
}
static uint32_t vote_weight(float w) {
  const float c = (w > 0.0f) ? ((w < 1.0f) ? w : 1.0f) : 0.0f;
  return (uint32_t)rintf(c * 65535.0f);
}
/* a below b, where -0 is below +0; neither is a NaN */
static int below(float a, float b) { return a < b || (a == b && signbit(a) && !signbit(b)); }

static v3 vertex(const float* V, uint32_t t) { return mk3(V[4 * (size_t)t], V[4 * (size_t)t + 1], V[4 * (size_t)t + 2]); }

static int linked(const float* V, uint32_t a, uint32_t b, const oparams_t* op) {
  const uint32_t lo = a < b ? a : b, hi = a < b ? b : a; /* the lower texel index first */
  const v3 ma = vertex(V, lo), mb = vertex(V, hi);
  return len3(sub3(ma, mb)) <= op->link_base + op->link_slope * fmin_(len3(ma), len3(mb));
}

/* V, S: height x width x 4 floats; flag: height x width bytes; T: the sensor pose, column-major; out: room for
 * op->max_objects records; ids: height x width words */
void object_shim_segment(const float* V, const float* S, const uint8_t* flag, int32_t W, int32_t H, const double* T,
                         const oparams_t* op, uint32_t scan_id, object_t* out, uint32_t* ids, ocounts_t* counts) {
  const uint32_t P = (uint32_t)W * (uint32_t)H;
  float Pf[16];
  for (int k = 0; k < 16; ++k) Pf[k] = (float)T[k];
  uint8_t* state = (uint8_t*)calloc((size_t)P + 1, 1); /* 1: member, not yet visited; 2: visited */
  uint32_t* stack = (uint32_t*)malloc(((size_t)P + 1) * sizeof(uint32_t));
  uint32_t* mem = (uint32_t*)malloc(((size_t)P + 1) * sizeof(uint32_t));
  uint64_t* sums = (uint64_t*)malloc(260 * sizeof(uint64_t));
  memset(counts, 0, sizeof(*counts));
  counts->n_texels = P;
  for (uint32_t t = 0; t < P; ++t) {
    ids[t] = 0xffffffffu;
    const float* dv = V + 4 * (size_t)t;
    const v3 m = mk3(dv[0], dv[1], dv[2]);
    const v3 w = m4_point(Pf, m);
    if (flag[t] != 0 && dv[3] > 0.5f && isfinite(m.x) && isfinite(m.y) && isfinite(m.z) && isfinite(w.x) && isfinite(w.y) &&
        isfinite(w.z)) {
      state[t] = 1;
      counts->n_members += 1;
    }
  }
  for (uint32_t root = 0; root < P; ++root) {
    if (state[root] != 1) continue;
    /* the component of `root`: every member reached from here has a greater index, or it would have been visited */
    uint32_t top = 0, n = 0;
    stack[top++] = root;
    state[root] = 2;
    while (top) {
      const uint32_t t = stack[--top];
      mem[n++] = t;
      const int32_t tx = (int32_t)(t % (uint32_t)W), ty = (int32_t)(t / (uint32_t)W);
      for (int32_t dy = -1; dy <= 1; ++dy)
        for (int32_t dx = -1; dx <= 1; ++dx) {
          const int32_t y = ty + dy, x = ((tx + dx) % W + W) % W;
          if (y < 0 || y >= H) continue;
          const uint32_t u = (uint32_t)y * (uint32_t)W + (uint32_t)x;
          if (u == t || state[u] != 1) continue; /* itself, no member, or taken already */
          if (!linked(V, t, u, op)) continue;
          state[u] = 2;
          stack[top++] = u;
        }
    }
    counts->n_components += 1;
    if (n < op->min_texels) {
      counts->n_small += 1;
      continue;
    }
    const uint32_t number = counts->n_objects;
    counts->n_objects += 1;
    if (number >= op->max_objects) continue;
    counts->stored += 1;
    object_t* o = &out[number];
    memset(o, 0, sizeof(*o));
    memset(sums, 0, 260 * sizeof(uint64_t));
    int64_t S3[3] = {0, 0, 0};
    uint64_t sum_all = 0;
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t t = mem[k];
      ids[t] = number;
      const float* ds = S + 4 * (size_t)t;
      const v3 m = vertex(V, t);
      const v3 w = m4_point(Pf, m);
      const float rm = len3(m), wk[3] = {w.x, w.y, w.z};
      for (int a = 0; a < 3; ++a) {
        if (k == 0 || below(wk[a], o->min[a])) o->min[a] = wk[a];
        if (k == 0 || below(o->max[a], wk[a])) o->max[a] = wk[a];
        S3[a] += llrintf(fclampf(wk[a] * 1024.0f, -1099511627776.0f, 1099511627776.0f));
      }
      if (k == 0 || rm < o->r_min) o->r_min = rm;
      if (is_dynamic_label(ds[0] * 255.0f)) o->n_dynamic += 1;
      const uint32_t wl = world_label(ds[0]), L = wl < 260u ? wl : 0u, q = vote_weight(ds[3]);
      sums[L] += q;
      sum_all += q;
    }
    uint32_t best = 0;
    for (uint32_t L = 1; L < 260; ++L)
      if (sums[L] > sums[best]) best = L;
    if (sum_all != 0) {
      o->label = best;
      o->prob = (float)sums[best] / (float)sum_all;
    } else {
      const uint32_t wl = world_label(S[4 * (size_t)root]);
      o->label = wl < 260u ? wl : 0u;
      o->prob = 0.0f;
    }
    o->root = root;
    o->n_texels = n;
    for (int a = 0; a < 3; ++a) o->centroid[a] = (float)((double)S3[a] / ((double)n * 1024.0));
    o->scan_id = scan_id;
  }
  free(sums), free(mem), free(stack), free(state);
}
