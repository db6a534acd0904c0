/*
 * grid_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_grid.hip restated on the host, sequentially:
 * a list of members per cell in source order, a table of 260 vote sums, then a pass over the raster.
 * Compiled by the tests with gcc -O2 -ffp-contract=off; suma_world_grid must equal it byte for byte.
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
  uint32_t label;
  float prob;
  uint32_t timestamp;
  uint32_t support;
} world_t;

typedef struct {
  float cell_size, origin_x, origin_y;
  uint32_t width, height;
  uint8_t ground_label[N_LABELS];
  float min_normal_z, step_height, clearance;
  uint32_t fill_radius;
} params_t;

typedef struct {
  float ground_z, ground_rough, z_min, z_max;
  float obstacle_z, prob;
  uint32_t label, support;
  uint32_t n_ground, n_obstacle, n_overhang;
  uint8_t state, ground_source, pad[2];
} cell_t;

typedef struct {
  uint32_t n_records, n_dropped, n_outside, n_binned, n_occupied, n_free, n_obstacle, n_no_ground, n_filled;
} stats_t;

static float quiet_nan(void) {
  const uint32_t u = 0x7fc00000u;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

uint32_t grid_shim_weight(float w) {
  float c = 0.0f;
  if (w > 0.0f) c = (w < 1.0f) ? w : 1.0f;
  return (uint32_t)rintf(c * 65535.0f);
}

/* the cell of a record: -2 dropped, -1 outside */
int64_t grid_shim_cell(const params_t* gp, float x, float y, float z) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return -2;
  const float fx = floorf((x - gp->origin_x) / gp->cell_size), fy = floorf((y - gp->origin_y) / gp->cell_size);
  if (!(fx >= 0.0f && fx < (float)gp->width && fy >= 0.0f && fy < (float)gp->height)) return -1;
  return (int64_t)((uint32_t)fy * gp->width + (uint32_t)fx);
}

/* is member a (source index sa) more confident than b (sb)?  a number beats a NaN, the greater number the smaller; equal
 * numbers or two NaNs: the smaller source index */
static int more_confident(float a, uint32_t sa, float b, uint32_t sb) {
  if (isnan(a) || isnan(b)) {
    if (isnan(a) && isnan(b)) return sa < sb;
    return isnan(b);
  }
  if (a > b) return 1;
  if (a < b) return 0;
  return sa < sb;
}

/* -0 is below +0 */
static int below(float a, float b) { return a < b || (a == b && signbit(a) && !signbit(b)); }

/* cells: width * height; returns 0, or -1 when memory runs out */
int grid_shim(const params_t* gp, const world_t* rec, uint32_t n, cell_t* cells, stats_t* stats) {
  const uint32_t n_cells = gp->width * gp->height;
  const float nan = quiet_nan();
  /* members per cell in source order: a linked list through next[], built back to front */
  int64_t* head = (int64_t*)malloc(sizeof(int64_t) * n_cells);
  int64_t* next = (int64_t*)malloc(sizeof(int64_t) * (n ? n : 1));
  if (!head || !next) {
    free(head), free(next);
    return -1;
  }
  memset(stats, 0, sizeof(*stats));
  stats->n_records = n;
  for (uint32_t c = 0; c < n_cells; ++c) head[c] = -1;
  for (int64_t s = (int64_t)n - 1; s >= 0; --s) {
    const int64_t c = grid_shim_cell(gp, rec[s].x, rec[s].y, rec[s].z);
    if (c == -2) ++stats->n_dropped;
    else if (c == -1) ++stats->n_outside;
    else next[s] = head[c], head[c] = s, ++stats->n_binned;
  }
  /* stage A */
  for (uint32_t c = 0; c < n_cells; ++c) {
    cell_t* o = cells + c;
    memset(o, 0, sizeof(*o));
    o->ground_z = o->ground_rough = o->z_min = o->z_max = o->obstacle_z = nan;
    if (head[c] < 0) continue;
    ++stats->n_occupied;
    uint64_t sums[N_LABELS], all = 0;
    memset(sums, 0, sizeof(sums));
    int64_t rep = -1, grep = -1;
    float g_min = 0.0f, g_max = 0.0f;
    for (int64_t s = head[c]; s >= 0; s = next[s]) {
      const world_t* q = rec + s;
      const uint32_t L = q->label < N_LABELS ? q->label : 0u, w = grid_shim_weight(q->prob);
      sums[L] += w, all += w;
      if (rep < 0 || more_confident(q->confidence, (uint32_t)s, rec[rep].confidence, (uint32_t)rep)) rep = s;
      if (o->support == 0 || below(q->z, o->z_min)) o->z_min = q->z;
      if (o->support == 0 || below(o->z_max, q->z)) o->z_max = q->z;
      ++o->support;
      if (gp->ground_label[L] != 0 && fabsf(q->nz) >= gp->min_normal_z) {
        if (grep < 0 || more_confident(q->confidence, (uint32_t)s, rec[grep].confidence, (uint32_t)grep)) grep = s;
        if (o->n_ground == 0 || below(q->z, g_min)) g_min = q->z;
        if (o->n_ground == 0 || below(g_max, q->z)) g_max = q->z;
        ++o->n_ground;
      }
    }
    if (all != 0) {
      uint32_t best = 0;
      for (uint32_t l = 1; l < N_LABELS; ++l)
        if (sums[l] > sums[best]) best = l; /* a tie keeps the smaller id */
      o->label = best;
      o->prob = (float)sums[best] / (float)all;
    } else {
      o->label = rec[rep].label < N_LABELS ? rec[rep].label : 0u;
      o->prob = 0.0f;
    }
    if (o->n_ground) o->ground_z = rec[grep].z, o->ground_rough = g_max - g_min;
  }
  /* stage B: the fill reads the stage-A heights only (own ground), so a filled cell never feeds another */
  float* own = (float*)malloc(sizeof(float) * n_cells);
  if (!own) {
    free(head), free(next);
    return -1;
  }
  for (uint32_t c = 0; c < n_cells; ++c) own[c] = cells[c].ground_z;
  const int32_t R = (int32_t)gp->fill_radius, W = (int32_t)gp->width, H = (int32_t)gp->height;
  for (uint32_t c = 0; c < n_cells; ++c) {
    cell_t* o = cells + c;
    float g = nan;
    if (o->n_ground) {
      g = o->ground_z, o->ground_source = 1;
    } else {
      const int32_t ix = (int32_t)(c % gp->width), iy = (int32_t)(c / gp->width);
      int32_t best_d = -1, best_dy = 0, best_dx = 0;
      for (int32_t dx = R; dx >= -R; --dx)      /* any order: the comparison below decides */
        for (int32_t dy = R; dy >= -R; --dy) {
          const int32_t x = ix + dx, y = iy + dy, d = dx * dx + dy * dy;
          if (x < 0 || x >= W || y < 0 || y >= H || cells[(uint32_t)y * gp->width + (uint32_t)x].n_ground == 0) continue;
          if (best_d < 0 || d < best_d || (d == best_d && (dy < best_dy || (dy == best_dy && dx < best_dx))))
            best_d = d, best_dy = dy, best_dx = dx;
        }
      if (best_d >= 0) {
        g = own[(uint32_t)(iy + best_dy) * gp->width + (uint32_t)(ix + best_dx)];
        o->ground_z = g, o->ground_rough = nan, o->ground_source = 2;
        ++stats->n_filled;
      }
    }
    if (o->ground_source)
      for (int64_t s = head[c]; s >= 0; s = next[s]) {
        const float z = rec[s].z, h = z - g;
        if (h > gp->clearance) {
          ++o->n_overhang;
        } else if (h > gp->step_height) {
          if (o->n_obstacle == 0 || below(o->obstacle_z, z)) o->obstacle_z = z;
          ++o->n_obstacle;
        }
      }
    if (o->support == 0) o->state = 0;
    else if (!o->ground_source) o->state = 3, ++stats->n_no_ground;
    else if (o->n_obstacle) o->state = 2, ++stats->n_obstacle;
    else o->state = 1, ++stats->n_free;
  }
  free(own), free(head), free(next);
  return 0;
}
