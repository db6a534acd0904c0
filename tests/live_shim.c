/*
 * live_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_live.hip restated on the host, one texel and one
 * cell after the other: the hits in texel order (the library sends one atomic a hit and lets the lane that finds an older
 * stamp keep the count; this compares and counts in a loop), the rays in texel order, live / pending and the composed
 * cells.  Compiled by the tests with gcc -O2 -ffp-contract=off; the library's state, counts, composed cells, mask and
 * stats must equal it byte for byte.  It shares no code with the library; the structures are declared again here.
 * With -DLIVE_SHIM_MAIN it is a program of its own that runs a small sequence, for the sanitizers.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  uint32_t hold_scans, min_hits;
  float carve_range, carve_margin;
} lparams_t;

typedef struct {
  uint64_t hit;
  uint32_t clear, hits;
} lcell_t;

typedef struct {
  uint32_t n_texels, n_members, n_outside, n_no_ground, n_low, n_high, n_hit_texels, n_hit_cells, n_rays, n_cleared;
} lcounts_t;

typedef struct {
  uint32_t n_live, n_pending, n_expired, n_carved;
} lstats_t;

/* the fields of the static grid the layer reads */
typedef struct {
  float cell_size, origin_x, origin_y;
  uint32_t width, height;
  float step_height, clearance;
} lgrid_t;

/* suma_grid_cell, 48 bytes */
typedef struct {
  float ground_z, ground_rough, z_min, z_max, obstacle_z, prob;
  uint32_t label, support, n_ground, n_obstacle, n_overhang;
  uint8_t state, ground_source, pad[2];
} gcell_t;

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

static uint32_t bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
static float unbits(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint32_t ordered(float f) {
  const uint32_t b = bits(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static float unordered(uint32_t o) { return unbits((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

#define NONE 0xffffffffu

static uint32_t cell_of(const lgrid_t* g, float x, float y) {
  const float fx = floorf((x - g->origin_x) / g->cell_size), fy = floorf((y - g->origin_y) / g->cell_size);
  if (!(fx >= 0.0f && fx < (float)g->width && fy >= 0.0f && fy < (float)g->height)) return NONE;
  return (uint32_t)fy * g->width + (uint32_t)fx;
}

static int has_return(const float* dv, const float* Pf, v3* w) {
  const v3 m = mk3(dv[0], dv[1], dv[2]);
  *w = m4_point(Pf, m);
  return dv[3] > 0.5f && isfinite(m.x) && isfinite(m.y) && isfinite(m.z) && isfinite(w->x) && isfinite(w->y) && isfinite(w->z);
}

/* V: height x width x 4 floats; flag: height x width bytes; ids: height x width words, or NULL (objects off); T: the sensor
 * pose, column-major; cells: the static grid; state: width * height cells, updated in place; s: the update's stamp */
void live_shim_update(const float* V, const uint8_t* flag, const uint32_t* ids, int32_t W, int32_t H, const double* T,
                      const lgrid_t* g, const gcell_t* cells, const lparams_t* lp, uint32_t s, lcell_t* state,
                      lcounts_t* counts) {
  const uint32_t P = (uint32_t)W * (uint32_t)H;
  float Pf[16];
  for (int k = 0; k < 16; ++k) Pf[k] = (float)T[k];
  memset(counts, 0, sizeof(*counts));
  counts->n_texels = P;
  for (uint32_t t = 0; t < P; ++t) {
    v3 w;
    if (!has_return(V + 4 * (size_t)t, Pf, &w) || flag[t] == 0) continue;
    if (ids && ids[t] == NONE) continue;
    counts->n_members += 1;
    const uint32_t c = cell_of(g, w.x, w.y);
    if (c == NONE) {
      counts->n_outside += 1;
      continue;
    }
    const float gz = cells[c].ground_z;
    if (isnan(gz)) {
      counts->n_no_ground += 1;
      continue;
    }
    const float h = w.z - gz;
    if (h <= g->step_height) {
      counts->n_low += 1;
      continue;
    }
    if (h > g->clearance) {
      counts->n_high += 1;
      continue;
    }
    counts->n_hit_texels += 1;
    lcell_t* st = &state[c];
    const uint32_t old = (uint32_t)(st->hit >> 32);
    if (old < s) { /* the cell's first hit of this update */
      st->hits = (old != 0 && old > st->clear && s - old <= lp->hold_scans) ? (st->hits + 1 < 65535u ? st->hits + 1 : 65535u) : 1u;
      counts->n_hit_cells += 1;
    }
    const uint64_t v = ((uint64_t)s << 32) | ordered(w.z);
    if (v > st->hit) st->hit = v;
  }
  if (lp->carve_range == 0.0f) return;
  /* the rays see the hits of the whole scan: a second pass */
  const v3 o = mk3(Pf[12], Pf[13], Pf[14]);
  const float step = 0.5f * g->cell_size;
  for (uint32_t t = 0; t < P; ++t) {
    v3 w;
    if (!has_return(V + 4 * (size_t)t, Pf, &w)) continue;
    counts->n_rays += 1;
    const v3 u = sub3(w, o);
    const float r = len3(u), lim = r - lp->carve_margin;
    uint32_t prev = NONE;
    for (uint32_t k = 1; k <= 4096u; ++k) {
      const float tk = (float)k * step;
      if (!(tk < lim && tk <= lp->carve_range)) break;
      const float q = tk / r;
      const float px = o.x + u.x * q, py = o.y + u.y * q, pz = o.z + u.z * q;
      const uint32_t c = cell_of(g, px, py);
      if (c == prev) continue;
      prev = c;
      if (c == NONE) continue;
      const uint32_t Hs = (uint32_t)(state[c].hit >> 32);
      if (!(Hs > 0 && Hs < s)) continue;
      if (!(pz <= unordered((uint32_t)state[c].hit))) continue;
      if (!(pz - cells[c].ground_z > g->step_height)) continue;
      if (state[c].clear < s) {
        state[c].clear = s;
        counts->n_cleared += 1;
      }
    }
  }
}

/* out: width * height cells; mask: one byte a cell, or NULL; now: the last update's stamp */
void live_shim_compose(const lgrid_t* g, const gcell_t* cells, const lparams_t* lp, const lcell_t* state, uint32_t now,
                       gcell_t* out, uint8_t* mask, lstats_t* stats) {
  const uint32_t n = g->width * g->height;
  memset(stats, 0, sizeof(*stats));
  for (uint32_t c = 0; c < n; ++c) {
    const uint32_t Hs = (uint32_t)(state[c].hit >> 32);
    uint8_t m = 0;
    out[c] = cells[c];
    if (Hs != 0) {
      if (!(Hs > state[c].clear)) stats->n_carved += 1;
      else if (!(now - Hs < lp->hold_scans)) stats->n_expired += 1;
      else if (state[c].hits >= lp->min_hits) {
        const float top = unordered((uint32_t)state[c].hit), oz = cells[c].obstacle_z;
        stats->n_live += 1;
        m = 1;
        out[c].state = 2; /* SUMA_GRID_OBSTACLE */
        if (isnan(oz) || oz < top || (oz == top && signbit(oz) && !signbit(top))) out[c].obstacle_z = top;
      } else {
        stats->n_pending += 1;
        m = 2;
      }
    }
    if (mask) mask[c] = m;
  }
}

#ifdef LIVE_SHIM_MAIN
#include <stdio.h>
/* a ring of returns around the sensor on a 9 x 7 raster, some of them on a box that is there for four scans and gone
 * afterwards; NaN and infinite points among them */
int main(void) {
  enum { W = 37, H = 3, GW = 9, GH = 7 };
  const lgrid_t g = {1.0f, -4.5f, -3.5f, GW, GH, 0.25f, 2.0f};
  const lparams_t lp = {3, 2, 20.0f, 0.5f};
  gcell_t* cells = (gcell_t*)calloc(GW * GH, sizeof(gcell_t));
  gcell_t* out = (gcell_t*)calloc(GW * GH, sizeof(gcell_t));
  uint8_t* mask = (uint8_t*)calloc(GW * GH, 1);
  lcell_t* state = (lcell_t*)calloc(GW * GH, sizeof(lcell_t));
  float* V = (float*)calloc((size_t)W * H * 4, sizeof(float));
  uint8_t* flag = (uint8_t*)calloc((size_t)W * H, 1);
  uint32_t* ids = (uint32_t*)calloc((size_t)W * H, sizeof(uint32_t));
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.25, -0.25, 0.5, 1};
  uint32_t live_total = 0;
  for (int c = 0; c < GW * GH; ++c) cells[c].ground_z = (c % 11 == 5) ? NAN : -1.0f, cells[c].obstacle_z = NAN, cells[c].state = 1;
  for (uint32_t s = 1; s <= 9; ++s) {
    for (int t = 0; t < W * H; ++t) {
      const float a = 6.2831853f * (float)(t % W) / (float)W, rr = (s <= 4 && t % W < 9) ? 2.0f : 6.0f;
      V[4 * t] = rr * cosf(a), V[4 * t + 1] = rr * sinf(a), V[4 * t + 2] = 0.5f * (float)(t / W) - 0.75f, V[4 * t + 3] = 1.0f;
      if (t % 17 == 3) V[4 * t + (t % 3)] = (t % 2) ? NAN : INFINITY;
      if (t % 23 == 7) V[4 * t + 3] = 0.0f;
      flag[t] = (uint8_t)(rr == 2.0f || t % 5 == 0);
      ids[t] = (t % 7 == 6) ? NONE : 0u;
    }
    lcounts_t cnt;
    lstats_t st;
    live_shim_update(V, flag, (s % 2) ? ids : NULL, W, H, T, &g, cells, &lp, s, state, &cnt);
    live_shim_compose(&g, cells, &lp, state, s, out, mask, &st);
    printf("%u: members %u hits %u cells %u rays %u cleared %u | live %u pending %u expired %u carved %u\n", s, cnt.n_members,
           cnt.n_hit_texels, cnt.n_hit_cells, cnt.n_rays, cnt.n_cleared, st.n_live, st.n_pending, st.n_expired, st.n_carved);
    live_total += st.n_live;
  }
  free(ids), free(flag), free(V), free(state), free(mask), free(out), free(cells);
  return live_total ? 0 : 1;
}
#endif
