/*
 * change_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_change.hip restated on the host, one window
 * record after the other: the observation of a frame at a pose (evidence and the nine totals) and the prune rule.
 * Compiled by the tests with gcc -O2 -ffp-contract=off; the library's evidence must equal it byte for byte.  It shares
 * no code with the library besides the transcendentals of include/suma_detmath.h, which are part of the specification
 * (draw_shim.c is the precedent); the structures are declared again here.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../include/suma_detmath.h"

typedef struct {
  float x, y, z, radius;
  float nx, ny, nz, confidence;
  uint32_t label;
  float prob;
  uint32_t timestamp;
  uint32_t support;
} world_t;

typedef struct {
  uint32_t hits, misses, occluded, label_changes;
} evidence_t;

typedef struct {
  uint32_t n_window, unseen, no_return, occluded, misses, grazing, hits, near_, label_changes;
} counts_t;

typedef struct {
  float free_margin, min_view_cos, max_range;
  int32_t tracked_only;
} params_t;

typedef struct {
  uint32_t min_misses;
  float miss_ratio;
} rule_t;

/* the data image (suma_params: data_fov_up / _down, min_depth, max_depth, data_width, data_height) and K9's literals */
typedef struct {
  float fov_up, fov_down, min_depth, max_depth;
  int32_t width, height;
  float map_max_distance, map_max_angle;
} image_t;

/* what the classification saw of one record (for the tests that craft boundary cases) */
typedef struct {
  float r, c, rm, distance, angle;
  int32_t in_tex, tx, ty, category; /* category: 1 unseen .. 7 near, the order of counts_t */
} probe_t;

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
static v3 neg3(v3 a) { return mk3(-a.x, -a.y, -a.z); }
static v3 divs3(v3 a, float s) {
  const float r = 1.0f / s;
  return mk3(a.x * r, a.y * r, a.z * r);
}
static v3 normalize3(v3 a) { return divs3(a, len3(a)); }
static v3 cross3(v3 a, v3 b) {
  return mk3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
static v3 m4_point(const float* m, v3 p) {
  return mk3(fmaf(m[8], p.z, fmaf(m[4], p.y, m[0] * p.x)) + m[12], fmaf(m[9], p.z, fmaf(m[5], p.y, m[1] * p.x)) + m[13],
             fmaf(m[10], p.z, fmaf(m[6], p.y, m[2] * p.x)) + m[14]);
}
static v3 m4_dir(const float* m, v3 d) {
  return mk3(fmaf(m[8], d.z, fmaf(m[4], d.y, m[0] * d.x)), fmaf(m[9], d.z, fmaf(m[5], d.y, m[1] * d.x)),
             fmaf(m[10], d.z, fmaf(m[6], d.y, m[2] * d.x)));
}

static uint32_t world_label(float r) {
  const float t = r * 255.0f + 0.5f;
  return (t >= 0.0f && t < 260.0f) ? (uint32_t)t : 0u;
}

/* SurfelMap.cpp:407: std::sin(Radians(float)) */
float change_shim_angle_thresh(float map_max_angle) { return sinf(((float)M_PI / 180.f) * map_max_angle); }

/* P = float(T), Pinv = float(rigid inverse of T in fp64) */
static void poses(const double* T, float* P, float* Pinv) {
  double inv[16];
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) inv[4 * c + r] = T[4 * r + c];
  for (int r = 0; r < 3; ++r) inv[12 + r] = -((T[4 * r] * T[12] + T[4 * r + 1] * T[13]) + T[4 * r + 2] * T[14]);
  inv[3] = inv[7] = inv[11] = 0.0;
  inv[15] = 1.0;
  for (int k = 0; k < 16; ++k) P[k] = (float)T[k], Pinv[k] = (float)inv[k];
}

/* one record; returns the category (1 .. 7) and adds to *e */
static int classify(const world_t* s, const float* V, const float* N, const float* S, const image_t* im, const float* P,
                    const float* Pinv, const params_t* cp, evidence_t* e, int* relabel, probe_t* pb) {
  const float fov_up = fabsf(im->fov_up), fov = fabsf(fabsf(im->fov_up)) + fabsf(fabsf(im->fov_down));
  const float width = (float)im->width, height = (float)im->height;
  const float angle_thresh = change_shim_angle_thresh(im->map_max_angle);
  const v3 p = mk3(s->x, s->y, s->z), n = mk3(s->nx, s->ny, s->nz);
  *relabel = 0;
  /* 1 */
  const v3 v = m4_point(Pinv, p);
  const float r = len3(v);
  if (pb) memset(pb, 0, sizeof(*pb)), pb->r = r, pb->tx = pb->ty = -1;
  if (!(r > 0.0f && r < cp->max_range)) return 1;
  /* 2 */
  const v3 ns = normalize3(m4_dir(Pinv, n));
  const float c = dot3(ns, divs3(neg3(v), r));
  if (pb) pb->c = c;
  /* 3: project01 */
  const float depth = len3(v);
  const float yaw = sdm_atan2(v.y, v.x);
  const float pitch = -sdm_asin(v.z / depth);
  const float x01 = 0.5f * ((-yaw * SUMA_INV_PI_F) + 1.0f);
  const float y01 = 1.0f - ((pitch * SUMA_RAD2DEG_F) + fov_up) / fov;
  const float imx = sdm_floor(x01 * width) + 0.5f, imy = sdm_floor(y01 * height) + 0.5f;
  const int in_tex = (imx >= 0.0f && imx < width && imy >= 0.0f && imy < height);
  if (!in_tex) return 1;
  const int32_t tx = (int32_t)sdm_floor(imx), ty = (int32_t)sdm_floor(imy);
  if (pb) pb->in_tex = 1, pb->tx = tx, pb->ty = ty;
  /* 4 */
  const size_t pix = 4 * ((size_t)ty * (size_t)im->width + (size_t)tx);
  const float *dv = V + pix, *dn = N + pix, *ds = S + pix;
  if (!(dv[3] > 0.5f)) return 2;
  /* 5 */
  const v3 m = mk3(dv[0], dv[1], dv[2]);
  const float rm = len3(m);
  if (pb) pb->rm = rm;
  if (rm + cp->free_margin < r) {
    e->occluded += 1;
    return 3;
  }
  if (rm > r + cp->free_margin) {
    if (c > cp->min_view_cos) {
      e->misses += 1;
      return 4;
    }
    return 5;
  }
  if (dn[3] > 0.5f && c > 0.0f) {
    const v3 mw = m4_point(P, m);
    const v3 nw = normalize3(m4_dir(P, mk3(dn[0], dn[1], dn[2])));
    const float distance = fabsf(dot3(n, sub3(mw, p)));
    const float angle = len3(cross3(nw, n));
    if (pb) pb->distance = distance, pb->angle = angle;
    if (distance < im->map_max_distance && angle < angle_thresh) {
      e->hits += 1;
      if (world_label(ds[0]) != s->label) e->label_changes += 1, *relabel = 1;
      return 6;
    }
  }
  return 7;
}

/* One observation.  rec: the map's records in source order; win: the source indices of the window's records, in window
 * order; V, N, S: the frame's maps (height x width x 4 floats); T: the sensor pose, column-major; ev: one entry per
 * record in source order, added to; counts: the totals of this observation; probes (optional): one per window record. */
void change_shim_observe(const world_t* rec, const uint32_t* win, uint32_t n_window, const float* V, const float* N,
                         const float* S, const image_t* im, const double* T, const params_t* cp, evidence_t* ev,
                         counts_t* counts, probe_t* probes) {
  float P[16], Pinv[16];
  poses(T, P, Pinv);
  uint32_t* cnt = (uint32_t*)counts;
  memset(counts, 0, sizeof(*counts));
  counts->n_window = n_window;
  for (uint32_t o = 0; o < n_window; ++o) {
    int relabel = 0;
    const int cat = classify(&rec[win[o]], V, N, S, im, P, Pinv, cp, &ev[win[o]], &relabel, probes ? &probes[o] : 0);
    if (probes) probes[o].category = cat;
    cnt[cat] += 1;
    counts->label_changes += (uint32_t)relabel;
  }
}

void change_shim_prune(const evidence_t* ev, uint32_t n, const rule_t* rule, uint8_t* keep, uint32_t* n_removed) {
  uint32_t removed = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const int gone = ev[k].misses >= rule->min_misses && (float)ev[k].misses > rule->miss_ratio * (float)ev[k].hits;
    keep[k] = gone ? 0 : 1;
    removed += (uint32_t)gone;
  }
  *n_removed = removed;
}
