/*
 * localize_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_localize.hip restated on the host,
 * sequentially: cell index, binning (a stable sort by key), the tile directory, the window order, the conversion of a
 * world record to a surfel, and the re-centring rule.  Compiled by the tests with gcc -O2 -ffp-contract=off; the
 * localiser's window must equal it byte for byte.  It shares no code with the library: the structures are declared
 * again here.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

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
  uint64_t key;
  uint32_t start, count;
} tile_t;

typedef struct {
  uint64_t key;
  uint32_t src;
} member_t;

#define GRID 1048576 /* 2^20 */

/* 1: the cell of (x, y); 0: the record is dropped */
int loc_shim_cell(float e, float x, float y, float z, int32_t* i, int32_t* j) {
  if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return 0;
  const float w = 2.0f * e;
  const float fi = floorf((x + e) / w), fj = floorf((y + e) / w);
  if (!(fabsf(fi) < (float)GRID) || !(fabsf(fj) < (float)GRID)) return 0;
  *i = (int32_t)fi;
  *j = (int32_t)fj;
  return 1;
}

uint64_t loc_shim_key(int32_t i, int32_t j) { return ((uint64_t)(i + GRID) << 21) | (uint64_t)(j + GRID); }

static int by_key_then_source(const void* a, const void* b) {
  const member_t *p = (const member_t*)a, *q = (const member_t*)b;
  if (p->key != q->key) return p->key < q->key ? -1 : 1;
  return p->src < q->src ? -1 : (p->src > q->src ? 1 : 0);
}

/* order: the kept records' source indices by (key, source index); dir: one entry per occupied tile, ascending by key.
 * Both hold up to n entries.  Returns 0, or -1 without memory. */
int loc_shim_bin(const world_t* rec, uint32_t n, float extent, uint32_t* order, tile_t* dir, uint32_t* n_kept,
                 uint32_t* n_dropped, uint32_t* n_tiles) {
  *n_kept = *n_dropped = *n_tiles = 0;
  if (n == 0) return 0;
  member_t* m = (member_t*)malloc((size_t)n * sizeof(member_t));
  if (!m) return -1;
  uint32_t kept = 0;
  for (uint32_t s = 0; s < n; ++s) {
    int32_t i, j;
    if (!loc_shim_cell(extent, rec[s].x, rec[s].y, rec[s].z, &i, &j)) continue;
    m[kept].key = loc_shim_key(i, j);
    m[kept].src = s;
    ++kept;
  }
  qsort(m, kept, sizeof(member_t), by_key_then_source);
  uint32_t tiles = 0;
  for (uint32_t k = 0; k < kept; ++k) {
    order[k] = m[k].src;
    if (k == 0 || m[k].key != m[k - 1].key) {
      dir[tiles].key = m[k].key;
      dir[tiles].start = k;
      dir[tiles].count = 0;
      ++tiles;
    }
    dir[tiles - 1].count += 1;
  }
  free(m);
  *n_kept = kept;
  *n_dropped = n - kept;
  *n_tiles = tiles;
  return 0;
}

void loc_shim_convert(const world_t* s, surfel_t* o) {
  o->x = s->x, o->y = s->y, o->z = s->z, o->radius = s->radius;
  o->nx = s->nx, o->ny = s->ny, o->nz = s->nz, o->confidence = s->confidence;
  o->timestamp = 0;
  o->color = 0.0f, o->weight = 0.0f, o->count = 0.0f;
  o->r = o->g = o->b = (float)s->label / 255.0f;
  o->w = s->prob;
}

/* the window around (oi, oj): tiles ascending by (i, then j), each in ascending source index.  Returns the number of
 * records the window holds; the first min(that, capacity) are written. */
uint64_t loc_shim_window(const world_t* rec, const uint32_t* order, const tile_t* dir, uint32_t n_tiles, int32_t oi,
                         int32_t oj, int32_t dim, surfel_t* out, uint32_t capacity) {
  uint64_t at = 0;
  for (int64_t i = (int64_t)oi - dim; i <= (int64_t)oi + dim; ++i)
    for (int64_t j = (int64_t)oj - dim; j <= (int64_t)oj + dim; ++j) {
      if (i <= -GRID || i >= GRID || j <= -GRID || j >= GRID) continue;
      const uint64_t key = loc_shim_key((int32_t)i, (int32_t)j);
      for (uint32_t t = 0; t < n_tiles; ++t) {
        if (dir[t].key != key) continue;
        for (uint32_t k = 0; k < dir[t].count; ++k, ++at)
          if (at < capacity) loc_shim_convert(&rec[order[dir[t].start + k]], &out[at]);
      }
    }
  return at;
}

/* updateActiveSubmaps' rule on the predicted position: 1 if the origin moved */
int loc_shim_recentre(float e, float x, float y, int32_t* oi, int32_t* oj) {
  const float cx = (float)(2.0 * *oi * e), cy = (float)(2.0 * *oj * e);
  const float changex = x - cx, changey = y - cy;
  const float factor = 1.1f;
  int moved = 0;
  if (fabsf(changex) > factor * e) *oi += (changex < 0) ? -1 : 1, moved = 1;
  if (fabsf(changey) > factor * e) *oj += (changey < 0) ? -1 : 1, moved = 1;
  return moved;
}
