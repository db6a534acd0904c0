/*
 * world_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_world.hip restated on the host, sequentially:
 * transform, filter, then (voxel mode) a stable sort by key and a walk over each voxel with a table of 260 vote sums.
 * Compiled by the tests with gcc -O2 -ffp-contract=off; suma_map_export_world must equal it byte for byte.
 * It shares no code with the library: the structures are declared again here.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define N_LABELS 260

typedef struct {
  float x, y, z, radius;
  float nx, ny, nz, confidence;
  uint32_t timestamp;
  float color, weight, count;
  float r, g, b, w;
} surfel_t;

typedef struct {
  float x, y, z, radius;
  float nx, ny, nz, confidence;
  uint32_t label;
  float prob;
  uint32_t timestamp;
  uint32_t support;
} world_t;

typedef struct {
  float voxel_size;
  float min_confidence;
  uint8_t keep_label[N_LABELS];
} params_t;

typedef struct {
  uint32_t n_active, n_tiles, n_parked, n_passed, n_dropped, n_out;
} stats_t;

typedef struct {
  uint64_t key;
  uint32_t src;
} member_t;

uint32_t world_shim_label(float r) {
  const float t = r * 255.0f + 0.5f;
  return (t >= 0.0f && t < 260.0f) ? (uint32_t)t : 0u;
}

uint32_t world_shim_weight(float w) {
  float c = 0.0f;
  if (w > 0.0f) c = (w < 1.0f) ? w : 1.0f;
  return (uint32_t)rintf(c * 65535.0f);
}

/* M column-major; each row fma(m3, v.w, fma(m2, v.z, fma(m1, v.y, m0 * v.x))) */
static void mat_vec(const float* m, const float v[4], float out[4]) {
  for (int r = 0; r < 4; ++r) out[r] = fmaf(m[12 + r], v[3], fmaf(m[8 + r], v[2], fmaf(m[4 + r], v[1], m[r] * v[0])));
}

static void transform(const surfel_t* s, const float* poses, uint32_t n_poses, float p[4], float n[4]) {
  uint32_t k = 0;
  if (s->count >= 0.0f) k = (s->count < (float)n_poses) ? (uint32_t)(int32_t)s->count : n_poses - 1u;
  const float v[4] = {s->x, s->y, s->z, 1.0f}, w[4] = {s->nx, s->ny, s->nz, 0.0f};
  mat_vec(poses + 16 * (size_t)k, v, p);
  mat_vec(poses + 16 * (size_t)k, w, n);
}

/* the world-frame position and normal of every source record (for the tests that check the transform alone) */
void world_shim_transform(const surfel_t* src, uint32_t n, const float* poses, uint32_t n_poses, float* p4, float* n4) {
  for (uint32_t s = 0; s < n; ++s) transform(src + s, poses, n_poses, p4 + 4 * (size_t)s, n4 + 4 * (size_t)s);
}

static int by_key_then_source(const void* a, const void* b) {
  const member_t *x = (const member_t*)a, *y = (const member_t*)b;
  if (x->key != y->key) return x->key < y->key ? -1 : 1;
  return x->src < y->src ? -1 : (x->src > y->src ? 1 : 0);
}

/* keys (optional): the voxel key of every output record.  stats: n_passed, n_dropped, n_out are written.
 * Returns 0, or -1 when memory runs out. */
int world_shim(const surfel_t* src, uint32_t n, const float* poses, uint32_t n_poses, const params_t* wp, world_t* out,
               uint32_t capacity, stats_t* stats, uint64_t* keys) {
  const int voxel = wp->voxel_size > 0.0f;
  member_t* mem = (member_t*)malloc(sizeof(member_t) * (n ? n : 1));
  if (!mem) return -1;
  uint32_t passed = 0, dropped = 0, m = 0, n_out = 0;
  for (uint32_t s = 0; s < n; ++s) {
    const surfel_t* q = src + s;
    const uint32_t L = world_shim_label(q->r);
    if (!(q->confidence > wp->min_confidence) || !wp->keep_label[L]) continue;
    ++passed;
    float p[4], nn[4];
    transform(q, poses, n_poses, p, nn);
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
      ++dropped;
      continue;
    }
    uint64_t key = 0;
    if (voxel) {
      const float f[3] = {floorf(p[0] / wp->voxel_size), floorf(p[1] / wp->voxel_size), floorf(p[2] / wp->voxel_size)};
      if (!(fabsf(f[0]) < 1048576.0f && fabsf(f[1]) < 1048576.0f && fabsf(f[2]) < 1048576.0f)) {
        ++dropped;
        continue;
      }
      key = ((uint64_t)((int32_t)f[0] + 1048576) << 42) | ((uint64_t)((int32_t)f[1] + 1048576) << 21) |
            (uint64_t)((int32_t)f[2] + 1048576);
    }
    mem[m].key = key;
    mem[m].src = s;
    ++m;
    if (!voxel) {
      if (n_out < capacity) {
        world_t* o = out + n_out;
        o->x = p[0], o->y = p[1], o->z = p[2], o->radius = q->radius;
        o->nx = nn[0], o->ny = nn[1], o->nz = nn[2], o->confidence = q->confidence;
        o->label = L, o->prob = q->w, o->timestamp = q->timestamp, o->support = 1;
        if (keys) keys[n_out] = 0;
      }
      ++n_out;
    }
  }
  if (voxel) {
    qsort(mem, m, sizeof(member_t), by_key_then_source);
    for (uint32_t a = 0; a < m;) {
      uint32_t b = a;
      uint64_t sums[N_LABELS], all = 0;
      memset(sums, 0, sizeof(sums));
      uint32_t rep = mem[a].src, stamp = 0;
      for (; b < m && mem[b].key == mem[a].key; ++b) { /* ascending source index */
        const surfel_t* q = src + mem[b].src;
        const uint32_t w = world_shim_weight(q->w);
        sums[world_shim_label(q->r)] += w;
        all += w;
        if (q->confidence > src[rep].confidence) rep = mem[b].src; /* a tie keeps the smaller source index */
        if (q->timestamp > stamp) stamp = q->timestamp;
      }
      if (n_out < capacity) {
        const surfel_t* q = src + rep;
        uint32_t best = 0;
        for (uint32_t l = 1; l < N_LABELS; ++l)
          if (sums[l] > sums[best]) best = l; /* a tie keeps the smaller id */
        float p[4], nn[4];
        transform(q, poses, n_poses, p, nn);
        world_t* o = out + n_out;
        o->x = p[0], o->y = p[1], o->z = p[2], o->radius = q->radius;
        o->nx = nn[0], o->ny = nn[1], o->nz = nn[2], o->confidence = q->confidence;
        if (all != 0) {
          o->label = best;
          o->prob = (float)sums[best] / (float)all;
        } else {
          o->label = world_shim_label(q->r);
          o->prob = 0.0f;
        }
        o->timestamp = stamp;
        o->support = b - a;
        if (keys) keys[n_out] = mem[a].key;
      }
      ++n_out;
      a = b;
    }
  }
  free(mem);
  stats->n_passed = passed;
  stats->n_dropped = dropped;
  stats->n_out = n_out;
  return 0;
}
