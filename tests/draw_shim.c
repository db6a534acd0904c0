/*
 * draw_shim.c -- TEST INFRASTRUCTURE: the arithmetic specification of csrc/k_draw.hip (SurfelMap::draw as a compute
 * rasteriser) restated on the host, one surfel after the other, in index order.  Built by the tests with
 * gcc -ffp-contract=off; the GPU tests compare the kernels with it bit for bit (RGBA8 and ids).  Every step below is
 * the one the kernel file's header states, in the same fp32 operation order.
 *
 *   int draw_shim(dp, surfels, n, poses, n_poses, rgba, ids)
 *     rgba: width * height uint32 (bytes R, G, B, A), row 0 = bottom; ids: width * height int32 (may be NULL)
 *   returns 0, or -1 for parameters suma_map_draw rejects
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/suma_detmath.h"
#include "../include/suma_hip.h"

#define EMPTY_KEY (~0ull)
#define MAXV 16 /* vertices of a clipped polygon (a convex one has at most 3 + 6) */

typedef struct {
  float x, y, z;
} v3;
typedef struct {
  float x, y, z, w;
} v4;
typedef struct {
  float c[6]; /* x, y, z, w, tu, tv */
} cvtx;
typedef struct {
  int32_t X, Y;
  float z, iw, su, sv;
} rvtx;

static v3 mk3(float x, float y, float z) {
  v3 r = {x, y, z};
  return r;
}
static float dot3(v3 a, v3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static v3 sub3(v3 a, v3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 scale3(float s, v3 a) { return mk3(s * a.x, s * a.y, s * a.z); }
static v3 normalize3(v3 a) {
  const float r = 1.0f / sqrtf(dot3(a, a));
  return mk3(a.x * r, a.y * r, a.z * r);
}
static v3 cross3(v3 a, v3 b) {
  return mk3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
/* column-major M * v: fma(m3, v.w, fma(m2, v.z, fma(m1, v.y, m0 * v.x))) per row */
static v4 mat_vec(const float* m, v4 v) {
  float o[4];
  for (int r = 0; r < 4; ++r) o[r] = fmaf(m[12 + r], v.w, fmaf(m[8 + r], v.z, fmaf(m[4 + r], v.y, m[r] * v.x)));
  v4 res = {o[0], o[1], o[2], o[3]};
  return res;
}
static float fclamp(float x, float lo, float hi) {
  float t = (x < lo) ? lo : x;
  return (t > hi) ? hi : t;
}
static int finite_f(float x) { return (sdm_f2u(x) & 0x7f800000u) != 0x7f800000u; }
static uint32_t unorm8(float x) {
  x = (x > 0.0f) ? x : 0.0f;
  x = (x < 1.0f) ? x : 1.0f;
  return (uint32_t)rintf(x * 255.0f);
}

/* vertex stage: world position and rotated normal through poses[int(count)] */
static void vertex_stage(const suma_surfel* s, const float* poses, uint32_t n_poses, v4* p, v4* n) {
  const float cnt = s->count;
  const uint32_t k = (cnt >= 0.0f) ? ((cnt < (float)n_poses) ? (uint32_t)(int32_t)cnt : n_poses - 1u) : 0u;
  const float* M = poses + 16 * (size_t)k;
  v4 a = {s->x, s->y, s->z, 1.0f}, b = {s->nx, s->ny, s->nz, 0.0f};
  *p = mat_vec(M, a);
  *n = mat_vec(M, b);
}

/* geometry stage up to the four clip-space corners: 0 = the surfel emits nothing */
static int quad_setup(const suma_draw_params* dp, const suma_surfel* s, const float* poses, uint32_t n_poses,
                      cvtx cv[4]) {
  v4 p, n;
  vertex_stage(s, poses, n_poses, &p, &n);
  const int mode = dp->color_mode;
  const float c = s->confidence;
  float radius = s->radius, alpha = 1.0f;
  int valid = (c > dp->conf_threshold) || !dp->use_stability;
  const v3 pp = mk3(p.x, p.y, p.z), nn = mk3(n.x, n.y, n.z);
  const v3 view_dir = normalize3(sub3(mk3(dp->view_pos[0], dp->view_pos[1], dp->view_pos[2]), pp));
  if (mode == 3) valid = 1;
  else if (mode == 5) {
    if (!(s->r != 0.0f)) valid = 0;
  } else if (mode == 0) {
    alpha = dp->mat_alpha;
  } else if (mode == 4) {
    valid = 1;
    alpha = 1.0f - fclamp(dp->conf_threshold - c, 0.1f, 1.0f);
    radius = radius / 1.41421356f;
  }
  valid = valid && (!dp->backface_culling || dot3(view_dir, nn) > 0.0f);
  if (!valid || alpha < 0.5f) return 0;
  const v3 u = normalize3(mk3(n.y - n.z, -n.x, n.x));
  const v3 v = normalize3(cross3(nn, u));
  const v3 ru = scale3(radius, u), rv = scale3(radius, v);
  static const float su[4] = {-1.0f, 1.0f, -1.0f, 1.0f}, sv[4] = {-1.0f, -1.0f, 1.0f, 1.0f};
  for (int k = 0; k < 4; ++k) {
    v4 q;
    q.x = (su[k] < 0.0f ? p.x - ru.x : p.x + ru.x);
    q.y = (su[k] < 0.0f ? p.y - ru.y : p.y + ru.y);
    q.z = (su[k] < 0.0f ? p.z - ru.z : p.z + ru.z);
    q.x = (sv[k] < 0.0f ? q.x - rv.x : q.x + rv.x);
    q.y = (sv[k] < 0.0f ? q.y - rv.y : q.y + rv.y);
    q.z = (sv[k] < 0.0f ? q.z - rv.z : q.z + rv.z);
    q.w = p.w;
    const v4 o = mat_vec(dp->mvp, q);
    cv[k].c[0] = o.x;
    cv[k].c[1] = o.y;
    cv[k].c[2] = o.z;
    cv[k].c[3] = o.w;
    cv[k].c[4] = su[k];
    cv[k].c[5] = sv[k];
    for (int j = 0; j < 4; ++j)
      if (!finite_f(cv[k].c[j])) return 0;
  }
  return 1;
}

/* signed distance to clip plane k: near z + w, far w - z, then x / y against the guard band |x|, |y| <= 2 w */
static float plane_dist(const cvtx* v, int k) {
  const float x = v->c[0], y = v->c[1], z = v->c[2], w = v->c[3], w2 = w + w;
  switch (k) {
    case 0: return z + w;
    case 1: return w - z;
    case 2: return w2 + x;
    case 3: return w2 - x;
    case 4: return w2 + y;
    default: return w2 - y;
  }
}
/* the point where the edge from the inside vertex a to the outside vertex b leaves the half space */
static cvtx isect(const cvtx* a, const cvtx* b, float da, float db) {
  const float t = da / (da - db);
  cvtx r;
  for (int j = 0; j < 6; ++j) r.c[j] = a->c[j] + t * (b->c[j] - a->c[j]);
  return r;
}
/* Sutherland-Hodgman against the six planes in order; returns the vertex count (0: nothing left or overflow) */
static int clip_poly(cvtx* poly, int n) {
  cvtx tmp[MAXV];
  for (int k = 0; k < 6 && n > 0; ++k) {
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const cvtx* cur = &poly[i];
      const cvtx* prev = &poly[(i + n - 1) % n];
      const float dc = plane_dist(cur, k), dpv = plane_dist(prev, k);
      if (dc >= 0.0f) {
        if (dpv < 0.0f) {
          if (m >= MAXV) return 0;
          tmp[m++] = isect(cur, prev, dc, dpv);
        }
        if (m >= MAXV) return 0;
        tmp[m++] = *cur;
      } else if (dpv >= 0.0f) {
        if (m >= MAXV) return 0;
        tmp[m++] = isect(prev, cur, dpv, dc);
      }
    }
    memcpy(poly, tmp, sizeof(cvtx) * (size_t)m);
    n = m;
  }
  return n;
}
/* perspective divide, viewport transform, snap to 1/256 pixel: 0 = the vertex is unusable */
static int project_vtx(const cvtx* v, float hw, float hh, rvtx* r) {
  const float w = v->c[3];
  if (!(w > 0.0f)) return 0;
  const float xd = v->c[0] / w, yd = v->c[1] / w, zd = v->c[2] / w;
  if (!(fabsf(xd) <= 4.0f && fabsf(yd) <= 4.0f && fabsf(zd) <= 4.0f)) return 0;
  const float xw = xd * hw + hw, yw = yd * hh + hh;
  r->X = (int32_t)sdm_floor(xw * 256.0f + 0.5f);
  r->Y = (int32_t)sdm_floor(yw * 256.0f + 0.5f);
  r->z = 0.5f * zd + 0.5f;
  r->iw = 1.0f / w;
  r->su = v->c[4] * r->iw;
  r->sv = v->c[5] * r->iw;
  return 1;
}

static double edge_fn(const rvtx* a, const rvtx* b, int32_t px, int32_t py) {
  const double ux = (double)(b->X - a->X), uy = (double)(b->Y - a->Y), vx = (double)(px - a->X),
               vy = (double)(py - a->Y);
  return fma(ux, vy, -(uy * vx));
}
static float edge_to_float(double w) { return (float)(w + 0.0); }
static int owns_edge(const rvtx* s, const rvtx* t) {
  const int32_t dx = t->X - s->X, dy = t->Y - s->Y;
  return dy > 0 || (dy == 0 && dx < 0);
}
static uint64_t draw_key(rvtx A, rvtx B, rvtx C, int32_t i, int32_t j, uint32_t id) {
  double area = edge_fn(&A, &B, C.X, C.Y);
  if (area < 0) {
    rvtx t = B;
    B = C;
    C = t;
    area = -area;
  }
  const int32_t px = 256 * i + 128, py = 256 * j + 128;
  const double w0 = edge_fn(&B, &C, px, py), w1 = edge_fn(&C, &A, px, py), w2 = edge_fn(&A, &B, px, py);
  const int covered = (area != 0) && (w0 > 0 || (w0 == 0 && owns_edge(&B, &C))) &&
                      (w1 > 0 || (w1 == 0 && owns_edge(&C, &A))) && (w2 > 0 || (w2 == 0 && owns_edge(&A, &B)));
  if (!covered) return EMPTY_KEY;
  const float fa = (float)area;
  const float b0 = edge_to_float(w0) / fa, b1 = edge_to_float(w1) / fa, b2 = edge_to_float(w2) / fa;
  const float z = (b0 * A.z + b1 * B.z) + b2 * C.z;
  const float den = (b0 * A.iw + b1 * B.iw) + b2 * C.iw;
  const float tu = ((b0 * A.su + b1 * B.su) + b2 * C.su) / den;
  const float tv = ((b0 * A.sv + b1 * B.sv) + b2 * C.sv) / den;
  if ((tu * tu + tv * tv) > 1.0f || sdm_isnan(z)) return EMPTY_KEY;
  const float zc = fclamp(z, 0.0f, 1.0f);
  return ((uint64_t)(uint32_t)rintf(zc * 16777215.0f) << 32) | id;
}
static void raster_tri(const rvtx* A, const rvtx* B, const rvtx* C, int32_t W, int32_t H, uint32_t id, uint64_t* zbuf) {
  const int32_t minX = A->X < B->X ? (A->X < C->X ? A->X : C->X) : (B->X < C->X ? B->X : C->X);
  const int32_t maxX = A->X > B->X ? (A->X > C->X ? A->X : C->X) : (B->X > C->X ? B->X : C->X);
  const int32_t minY = A->Y < B->Y ? (A->Y < C->Y ? A->Y : C->Y) : (B->Y < C->Y ? B->Y : C->Y);
  const int32_t maxY = A->Y > B->Y ? (A->Y > C->Y ? A->Y : C->Y) : (B->Y > C->Y ? B->Y : C->Y);
  int32_t i0 = (minX - 128 + 255) >> 8, i1 = (maxX - 128) >> 8, j0 = (minY - 128 + 255) >> 8, j1 = (maxY - 128) >> 8;
  if (i0 < 0) i0 = 0;
  if (j0 < 0) j0 = 0;
  if (i1 > W - 1) i1 = W - 1;
  if (j1 > H - 1) j1 = H - 1;
  for (int32_t j = j0; j <= j1; ++j)
    for (int32_t i = i0; i <= i1; ++i) {
      const uint64_t key = draw_key(*A, *B, *C, i, j, id);
      uint64_t* z = &zbuf[(size_t)j * (size_t)W + (size_t)i];
      if (key < *z) *z = key;
    }
}

/* fragment colour of the winning surfel (draw_surfels.geom:84-147), RGBA in [0, 1] before the unorm conversion */
static void shade(const suma_draw_params* dp, const suma_surfel* s, const float* poses, uint32_t n_poses, float out[4],
                  int* direct, uint8_t bytes[3]) {
  v4 p, n;
  vertex_stage(s, poses, n_poses, &p, &n);
  const int mode = dp->color_mode;
  const float c = s->confidence;
  const v3 pp = mk3(p.x, p.y, p.z), nn = mk3(n.x, n.y, n.z);
  *direct = 0;
  out[3] = 1.0f;
  if (mode == 1) {
    const float a = 0.5f * fabsf(dot3(nn, mk3(1.0f, 1.0f, 1.0f))) + 0.1f;
    out[0] = out[1] = out[2] = a;
  } else if (mode == 2) {
    out[0] = fabsf(n.x);
    out[1] = fabsf(n.y);
    out[2] = fabsf(n.z);
  } else if (mode == 3) {
    static const float R[4] = {2.90912735f, -2.14404531f, 0.04439198f, 0.29390206f};
    static const float G[4] = {-0.17293242f, -0.16906214f, 1.24131122f, 0.01871256f};
    static const float B[4] = {0.17848859f, -1.72405244f, 1.23042564f, 0.34479632f};
    const float t = 1.0f - 1.0f / (1.0f + sdm_exp(c));
    const float t2 = t * t, t3 = t2 * t;
    const float* tab[3] = {R, G, B};
    for (int k = 0; k < 3; ++k) out[k] = fmaf(1.0f, tab[k][3], fmaf(t, tab[k][2], fmaf(t2, tab[k][1], t3 * tab[k][0])));
  } else if (mode == 5) {
    const float sx = (s->r * 255.0f) / 259.0f;
    const float fi = sdm_floor(sx * 260.0f);
    *direct = 1;
    if (fi >= 0.0f && fi < 260.0f) {
      const int idx = (int)fi;
      bytes[0] = dp->color_map[idx][0];
      bytes[1] = dp->color_map[idx][1];
      bytes[2] = dp->color_map[idx][2];
    } else {
      bytes[0] = bytes[1] = bytes[2] = 0;
    }
  } else {
    const v3 norm = normalize3(nn);
    const v3 view_dir = normalize3(sub3(mk3(dp->view_pos[0], dp->view_pos[1], dp->view_pos[2]), pp));
    v3 sc = mk3(dp->mat_diffuse[0], dp->mat_diffuse[1], dp->mat_diffuse[2]);
    float alpha = dp->mat_alpha;
    if (mode == 4) {
      const float col = s->color;
      const int32_t ci = (col >= 0.0f && col < 2147483648.0f) ? (int32_t)col : 0;
      sc = mk3((float)((ci >> 16) & 0xFF) / 255.0f, (float)((ci >> 8) & 0xFF) / 255.0f, (float)(ci & 0xFF) / 255.0f);
      alpha = 1.0f - fclamp(dp->conf_threshold - c, 0.1f, 1.0f);
    }
    v3 res = mk3(0.0f, 0.0f, 0.0f);
    for (uint32_t i = 0; i < dp->num_lights; ++i) {
      const suma_draw_light* L = &dp->lights[i];
      const v3 lp = mk3(L->position[0], L->position[1], L->position[2]);
      const v3 ld = (L->position[3] < 0.0001f) ? normalize3(mk3(-lp.x, -lp.y, -lp.z)) : normalize3(sub3(lp, pp));
      const float diff = fabsf(dot3(norm, ld));
      const v3 I = mk3(-ld.x, -ld.y, -ld.z);
      const float t = 2.0f * dot3(norm, I);
      const v3 refl = mk3(I.x - t * norm.x, I.y - t * norm.y, I.z - t * norm.z);
      float sd = dot3(view_dir, refl);
      sd = (sd < 0.0f) ? 0.0f : sd;
      const float spec = (sd > 0.0f) ? sdm_exp(dp->mat_shininess * sdm_log(sd)) : 0.0f;
      const float scv[3] = {sc.x, sc.y, sc.z};
      float* r3[3] = {&res.x, &res.y, &res.z};
      for (int k = 0; k < 3; ++k) {
        const float amb = L->ambient[k] * dp->mat_ambient[k];
        const float dif = L->diffuse[k] * (diff * scv[k]);
        const float spc = L->specular[k] * (spec * dp->mat_specular[k]);
        *r3[k] = *r3[k] + (((amb + dif) + spc) + dp->mat_emission[k]);
      }
    }
    out[0] = res.x;
    out[1] = res.y;
    out[2] = res.z;
    out[3] = alpha;
  }
}

int draw_check(const suma_draw_params* dp) {
  if (!dp || dp->width < 1 || dp->width > SUMA_DRAW_MAX_SIZE || dp->height < 1 || dp->height > SUMA_DRAW_MAX_SIZE ||
      dp->color_mode < 0 || dp->color_mode > 5 || dp->num_lights > SUMA_DRAW_MAX_LIGHTS)
    return -1;
  return 0;
}

/* the clip-space corners of one surfel, for the known-answer tests: 1 = emitted */
int draw_shim_corners(const suma_draw_params* dp, const suma_surfel* s, const float* poses, uint32_t n_poses,
                      float* out24) {
  cvtx cv[4];
  if (!quad_setup(dp, s, poses, n_poses, cv)) return 0;
  for (int k = 0; k < 4; ++k) memcpy(out24 + 6 * k, cv[k].c, sizeof(cv[k].c));
  return 1;
}

/* the pixels of one surfel, bit for bit the z-buffer keys the kernels' raster pass sends (EMPTY_KEY elsewhere) */
void draw_shim_raster(const suma_draw_params* dp, const suma_surfel* s, uint32_t n, const float* poses,
                      uint32_t n_poses, uint64_t* zbuf) {
  const int32_t W = (int32_t)dp->width, H = (int32_t)dp->height;
  const float hw = 0.5f * (float)dp->width, hh = 0.5f * (float)dp->height;
  static const int tri[2][3] = {{0, 1, 2}, {2, 1, 3}};
  for (uint32_t id = 0; id < n; ++id) {
    cvtx cv[4];
    if (!quad_setup(dp, &s[id], poses, n_poses, cv)) continue;
    for (int t = 0; t < 2; ++t) {
      cvtx poly[MAXV];
      for (int k = 0; k < 3; ++k) poly[k] = cv[tri[t][k]];
      const int m = clip_poly(poly, 3);
      if (m < 3) continue;
      rvtx r[MAXV];
      int ok = 1;
      for (int k = 0; k < m && ok; ++k) ok = project_vtx(&poly[k], hw, hh, &r[k]);
      if (!ok) continue;
      for (int k = 1; k + 1 < m; ++k) raster_tri(&r[0], &r[k], &r[k + 1], W, H, id, zbuf);
    }
  }
}

int draw_shim(const suma_draw_params* dp, const suma_surfel* s, uint32_t n, const float* poses, uint32_t n_poses,
              uint32_t* rgba, int32_t* ids) {
  if (draw_check(dp) || n_poses == 0) return -1;
  const size_t P = (size_t)dp->width * dp->height;
  uint64_t* zbuf = (uint64_t*)malloc(P * sizeof(uint64_t));
  if (!zbuf) return -2;
  for (size_t k = 0; k < P; ++k) zbuf[k] = EMPTY_KEY;
  draw_shim_raster(dp, s, n, poses, n_poses, zbuf);
  const uint32_t clear = unorm8(dp->clear_color[0]) | (unorm8(dp->clear_color[1]) << 8) |
                         (unorm8(dp->clear_color[2]) << 16) | (unorm8(dp->clear_color[3]) << 24);
  for (size_t k = 0; k < P; ++k) {
    const uint64_t key = zbuf[k];
    if (key == EMPTY_KEY) {
      rgba[k] = clear;
      if (ids) ids[k] = -1;
      continue;
    }
    const uint32_t id = (uint32_t)(key & 0xffffffffull);
    float col[4];
    int direct;
    uint8_t b[3];
    shade(dp, &s[id], poses, n_poses, col, &direct, b);
    rgba[k] = direct ? ((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | (255u << 24))
                     : (unorm8(col[0]) | (unorm8(col[1]) << 8) | (unorm8(col[2]) << 16) | (unorm8(col[3]) << 24));
    if (ids) ids[k] = (int32_t)id;
  }
  free(zbuf);
  return 0;
}
