/*
 * novel_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_novel.hip restated on the host, one record and
 * one texel after the other: the mark image, the collection (candidates, counts, capacity) and the fusion.  Compiled by
 * the tests with gcc -O2 -ffp-contract=off; the library's marks, candidates, counts and fused records must equal it byte
 * for byte.  It shares no code with the library besides the transcendentals of include/suma_detmath.h, which are part of
 * the specification (change_shim.c is the precedent); the structures are declared again here.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
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
  uint32_t n_texels, no_return, out_of_range, grazing, explained, novel, stored;
} counts_t;

typedef struct {
  float agree_margin, max_range;
  int32_t tracked_only;
  uint32_t max_candidates;
} params_t;

/* the data image and the map constants a collection reads (suma_params: data_fov_up / _down, data_width, data_height,
 * max_angle, p_prior, min_radius, max_radius) */
typedef struct {
  float fov_up, fov_down;
  int32_t width, height;
  float max_angle, p_prior, min_radius, max_radius;
} image_t;

typedef struct {
  float x, y, z;
} v3;

static v3 mk3(float x, float y, float z) {
  v3 r = {x, y, z};
  return r;
}
static float dot3(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static float len3(v3 a) { return sqrtf(dot3(a, a)); }
static v3 neg3(v3 a) { return mk3(-a.x, -a.y, -a.z); }
static v3 divs3(v3 a, float s) {
  const float r = 1.0f / s;
  return mk3(a.x * r, a.y * r, a.z * r);
}
static v3 normalize3(v3 a) { return divs3(a, len3(a)); }
static v3 m4_point(const float* m, v3 p) {
  return mk3(fmaf(m[8], p.z, fmaf(m[4], p.y, m[0] * p.x)) + m[12], fmaf(m[9], p.z, fmaf(m[5], p.y, m[1] * p.x)) + m[13],
             fmaf(m[10], p.z, fmaf(m[6], p.y, m[2] * p.x)) + m[14]);
}
static v3 m4_dir(const float* m, v3 d) {
  return mk3(fmaf(m[8], d.z, fmaf(m[4], d.y, m[0] * d.x)), fmaf(m[9], d.z, fmaf(m[5], d.y, m[1] * d.x)),
             fmaf(m[10], d.z, fmaf(m[6], d.y, m[2] * d.x)));
}
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
static int finite_f(float x) { return isfinite(x) ? 1 : 0; }

/* the constants as the library derives them from suma_params (the reference's setParameters) */
float novel_shim_angle_thresh(float max_angle) { return (float)cos((double)(float)((double)max_angle * M_PI / 180.0)); }
float novel_shim_log_prior(float p_prior) { return (float)log((double)p_prior / (1.0 - (double)p_prior)); }
float novel_shim_pixel_size(const image_t* im) {
  const float vfov = fabsf(im->fov_up) + fabsf(im->fov_down), hfov = 360.0f;
  const float vpix = (float)tan(0.5 * ((double)vfov * M_PI / 180.0) / (double)(uint32_t)im->height);
  const float hpix = (float)tan(0.5 * ((double)hfov * M_PI / 180.0) / (double)(uint32_t)im->width);
  return vpix < hpix ? hpix : vpix;
}

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

/* Step 1.  rec: the map's records in source order; win: the source indices of the window's records; V: the frame's
 * vertex map (height x width x 4 floats); T: the sensor pose, column-major; mark: height x width bytes, zeroed here */
void novel_shim_mark(const world_t* rec, const uint32_t* win, uint32_t n_window, const float* V, const image_t* im,
                     const double* T, const params_t* np, uint8_t* mark) {
  float P[16], Pinv[16];
  poses(T, P, Pinv);
  const float fov_up = fabsf(im->fov_up), fov = fabsf(fabsf(im->fov_up)) + fabsf(fabsf(im->fov_down));
  const float width = (float)im->width, height = (float)im->height;
  memset(mark, 0, (size_t)im->width * (size_t)im->height);
  for (uint32_t o = 0; o < n_window; ++o) {
    const world_t* s = &rec[win[o]];
    const v3 v = m4_point(Pinv, mk3(s->x, s->y, s->z));
    const float r = len3(v);
    if (!(r > 0.0f && r < np->max_range)) continue;
    const float yaw = sdm_atan2(v.y, v.x);
    const float pitch = -sdm_asin(v.z / r);
    const float x01 = 0.5f * ((-yaw * SUMA_INV_PI_F) + 1.0f);
    const float y01 = 1.0f - ((pitch * SUMA_RAD2DEG_F) + fov_up) / fov;
    const float imx = sdm_floor(x01 * width) + 0.5f, imy = sdm_floor(y01 * height) + 0.5f;
    if (!(imx >= 0.0f && imx < width && imy >= 0.0f && imy < height)) continue;
    const int32_t tx = (int32_t)sdm_floor(imx), ty = (int32_t)sdm_floor(imy);
    const size_t pix = (size_t)ty * (size_t)im->width + (size_t)tx;
    const float* dv = V + 4 * pix;
    if (!(dv[3] > 0.5f)) continue;
    const float rm = len3(mk3(dv[0], dv[1], dv[2]));
    if (rm + np->agree_margin < r) continue;
    if (rm > r + np->agree_margin) continue;
    mark[pix] = 1;
  }
}

/* Steps 2-4.  cand: the buffer of np->max_candidates records, *held of them in use; category (optional): one byte per
 * texel, 1 no return .. 5 novel, the order of counts_t */
void novel_shim_collect(const float* V, const float* N, const float* S, const image_t* im, const double* T,
                        const params_t* np, const uint8_t* mark, uint32_t scan_id, world_t* cand, uint32_t* held,
                        uint32_t* n_overflow, counts_t* counts, uint8_t* category) {
  float P[16], Pinv[16];
  poses(T, P, Pinv);
  const int32_t W = im->width, H = im->height;
  const float angle_thresh = novel_shim_angle_thresh(im->max_angle), pixel_size = novel_shim_pixel_size(im);
  const float log_prior = novel_shim_log_prior(im->p_prior);
  uint32_t* cnt = (uint32_t*)counts;
  memset(counts, 0, sizeof(*counts));
  counts->n_texels = (uint32_t)W * (uint32_t)H;
  for (int32_t ty = 0; ty < H; ++ty)
    for (int32_t tx = 0; tx < W; ++tx) {
      const size_t pix = (size_t)ty * (size_t)W + (size_t)tx;
      const float *dv = V + 4 * pix, *dn = N + 4 * pix, *ds = S + 4 * pix;
      int cat;
      const v3 m = mk3(dv[0], dv[1], dv[2]), nn = mk3(dn[0], dn[1], dn[2]);
      const float rm = len3(m);
      const v3 w = m4_point(P, m);
      if (!(dv[3] > 0.5f && dn[3] > 0.5f)) {
        cat = 1;
      } else if (!(rm > 0.0f && rm + np->agree_margin < np->max_range) || !(finite_f(w.x) && finite_f(w.y) && finite_f(w.z))) {
        cat = 2;
      } else if (!(dot3(nn, divs3(neg3(m), rm)) > angle_thresh)) {
        cat = 3;
      } else {
        int marked = 0;
        for (int32_t dy = -1; dy <= 1; ++dy)
          for (int32_t dx = -1; dx <= 1; ++dx) {
            const int32_t y = ty + dy, x = ((tx + dx) % W + W) % W;
            if (y >= 0 && y < H && mark[(size_t)y * (size_t)W + (size_t)x]) marked = 1;
          }
        cat = marked ? 4 : 5;
      }
      cnt[cat] += 1;
      if (category) category[pix] = (uint8_t)cat;
      if (cat != 5) continue;
      if (*held >= np->max_candidates) {
        *n_overflow += 1;
        continue;
      }
      world_t* c = &cand[*held];
      const v3 nw = normalize3(m4_dir(P, nn));
      float radius = ((1.41f * rm) * pixel_size) / fclampf(dot3(nn, divs3(neg3(m), rm)), 0.5f, 1.0f);
      radius = (radius < im->min_radius) ? im->min_radius : radius; /* fmax_ */
      radius = (im->max_radius < radius) ? im->max_radius : radius; /* fmin_ */
      c->x = w.x, c->y = w.y, c->z = w.z, c->radius = radius;
      c->nx = nw.x, c->ny = nw.y, c->nz = nw.z;
      c->confidence = is_dynamic_label(ds[0] * 255.0f) ? log_prior - 0.5f : log_prior;
      c->label = world_label(ds[0]);
      c->prob = ds[3];
      c->timestamp = scan_id;
      c->support = 1u;
      *held += 1;
      counts->stored += 1;
    }
}

/* Step 5 */
typedef struct {
  uint64_t key;
  uint32_t idx;
} keyed_t;

static int by_key_then_index(const void* a, const void* b) {
  const keyed_t *p = (const keyed_t*)a, *q = (const keyed_t*)b;
  if (p->key != q->key) return p->key < q->key ? -1 : 1;
  return p->idx < q->idx ? -1 : (p->idx > q->idx ? 1 : 0);
}

static uint32_t vote_weight(float w) {
  const float c = (w > 0.0f) ? ((w < 1.0f) ? w : 1.0f) : 0.0f;
  return (uint32_t)rintf(c * 65535.0f);
}

/* out / views: room for n records; stats: n_dropped, n_voxels, n_out */
void novel_shim_fuse(const world_t* cand, uint32_t n, float voxel_size, uint32_t min_views, float confidence, world_t* out,
                     uint32_t* views, uint32_t* stats) {
  keyed_t* k = (keyed_t*)malloc(((size_t)n + 1) * sizeof(keyed_t));
  uint32_t m = 0;
  stats[0] = stats[1] = stats[2] = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const float fx = sdm_floor(cand[i].x / voxel_size), fy = sdm_floor(cand[i].y / voxel_size),
                fz = sdm_floor(cand[i].z / voxel_size);
    if (!(fabsf(fx) < 1048576.0f && fabsf(fy) < 1048576.0f && fabsf(fz) < 1048576.0f)) {
      stats[0] += 1;
      continue;
    }
    const uint64_t ix = (uint64_t)((int32_t)fx + 1048576), iy = (uint64_t)((int32_t)fy + 1048576),
                   iz = (uint64_t)((int32_t)fz + 1048576);
    k[m].key = (ix << 42) | (iy << 21) | iz;
    k[m].idx = i;
    ++m;
  }
  qsort(k, m, sizeof(keyed_t), by_key_then_index);
  uint64_t* sums = (uint64_t*)malloc(260 * sizeof(uint64_t));
  for (uint32_t a = 0; a < m;) {
    uint32_t b = a;
    while (b < m && k[b].key == k[a].key) ++b;
    stats[1] += 1;
    /* distinct timestamps: a member counts when no earlier member of the run carries its timestamp */
    uint32_t nv = 0, stamp = 0, rep = k[a].idx;
    float rad_best = 0.0f;
    uint64_t sum_all = 0;
    memset(sums, 0, 260 * sizeof(uint64_t));
    for (uint32_t j = a; j < b; ++j) {
      const world_t* c = &cand[k[j].idx];
      int seen = 0;
      for (uint32_t e = a; e < j && !seen; ++e) seen = cand[k[e].idx].timestamp == c->timestamp;
      nv += seen ? 0u : 1u;
      stamp = c->timestamp > stamp ? c->timestamp : stamp;
      const float rad = (c->radius == c->radius) ? c->radius : INFINITY;
      if (j == a || rad < rad_best) rad_best = rad, rep = k[j].idx; /* ascending index: the first of a tie stays */
      const uint32_t L = c->label < 260u ? c->label : 0u, q = vote_weight(c->prob);
      sums[L] += q;
      sum_all += q;
    }
    const uint32_t members = b - a;
    a = b;
    if (nv < min_views) continue;
    const world_t* r = &cand[rep];
    world_t* o = &out[stats[2]];
    uint32_t lab_best = 0;
    for (uint32_t L = 1; L < 260; ++L)
      if (sums[L] > sums[lab_best]) lab_best = L;
    *o = *r;
    o->confidence = confidence;
    if (sum_all != 0) {
      o->label = lab_best;
      o->prob = (float)sums[lab_best] / (float)sum_all;
    } else {
      o->label = r->label < 260u ? r->label : 0u;
      o->prob = 0.0f;
    }
    o->timestamp = stamp;
    o->support = members;
    views[stats[2]] = nv;
    stats[2] += 1;
  }
  free(sums);
  free(k);
}
