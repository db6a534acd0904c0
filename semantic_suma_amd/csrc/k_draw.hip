/*
 * k_draw.hip -- SurfelMap::draw without a graphics pipeline: the viewer's picture of the active map (a compute
 * rasteriser, like K4 in k_render.hip, but with a perspective camera and clipping).
 *
 * Replaces (reference, citations relative to the reference tree):
 *   src/core/SurfelMap.cpp:1167-1230  SurfelMap::draw (GL_LESS depth test, glDrawArrays(GL_POINTS) over surfels_)
 *   src/shader/draw_surfels.vert      surfel -> map frame through the creation pose, colour unpack (color.glsl:40-47)
 *   src/shader/draw_surfels.geom      validity, the six colour modes, the quad p +- r u +- r v as a 4-vertex strip
 *   src/shader/draw_surfels.frag      alpha < 0.5 and dot(tc, tc) > 1 discard
 *   with the uniforms SurfelMap's constructor leaves (SurfelMap.cpp:187-229: use_stability never set = false,
 *   num_lights = 1) and the colour map texture of setColorMap (SurfelMap.cpp:1238-1256, NEAREST / CLAMP_TO_BORDER).
 *
 * Kernels (VGPRs: tools/isa_stats.py k_draw.hip; none uses scratch):
 *   kd_raster   lane per surfel: vertex + geometry stage, quads that need no clipping and cover at most
 *               DRAW_LANE_TESTS pixel tests are rasterised by the lane; the others go to the large-quad queue.  77 VGPRs.
 *   kd_big      block per queued quad: two lanes clip the two triangles, the block runs their pixel tests.   60 VGPRs.
 *   kd_resolve  lane per pixel: deferred shading of the winner, RGBA8 + id, re-arms the z-buffer.           42 VGPRs.
 * The z-buffer (W x H keys) and the queue (max_surfels ids + a counter) belong to the ctx; both are left cleared.
 *
 * ARITHMETIC SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; dot / cross / mat * vec
 * are the fma chains of dev_math.h; normalize(v) = v * (1 / sqrt(dot(v, v))); `/` and sqrt correctly rounded;
 * transcendentals from include/suma_detmath.h).  tests/draw_shim.c restates it on the host, bit for bit.
 *
 * Vertex stage, surfel s: k = int(count) clamped to [0, max_poses - 1]; M = poses[k] (column-major);
 *   p = M * (x, y, z, 1), n = M * (nx, ny, nz, 0), each row fma(m3, v.w, fma(m2, v.z, fma(m1, v.y, m0 * v.x))).
 * Geometry stage:
 *   valid = c > conf_threshold || !use_stability;  view_dir = normalize(view_pos - p.xyz);  radius = s.radius
 *   mode 3: valid = true;  mode 5: valid = false if s.r == 0 (label 0);  mode 0: alpha = mat_alpha;
 *   mode 4: valid = true, alpha = 1 - clamp(conf_threshold - c, 0.1, 1), radius = radius / 1.41421356f;  else alpha = 1
 *   valid = valid && (!backface_culling || dot(view_dir, n.xyz) > 0);  nothing is drawn unless valid && !(alpha < 0.5)
 *   (draw_surfels.frag discards every fragment of a surfel with alpha < 0.5 before the depth test).
 *   u = normalize(n.y - n.z, -n.x, n.x), v = normalize(cross(n.xyz, u)) -- K4's construction.  DEGENERATE NORMALS
 *   (n.x = 0 and n.y = n.z, u of length 0): 1 / sqrt(0) = inf, 0 * inf = NaN, so the corners are NaN and the rule below
 *   drops the surfel: it draws nothing (GL leaves normalize(0) undefined).
 *   corners (p - ru) - rv, (p + ru) - rv, (p - ru) + rv, (p + ru) + rv (ru = radius * u, w = p.w), tc (+-1, +-1);
 *   clip_k = mvp * corner_k.  A surfel with a non-finite clip coordinate draws nothing.
 * Primitive assembly: triangles (v0, v1, v2) and (v2, v1, v3), no face culling (GL_CULL_FACE is never enabled).
 * Clipping, per triangle, Sutherland-Hodgman against near z + w >= 0, far w - z >= 0 and the guard band
 *   (w + w) +- x >= 0, (w + w) +- y >= 0, in that order; an edge leaving a plane is cut at t = d_in / (d_in - d_out),
 *   v = a + t * (b - a) for (x, y, z, w, tu, tv), always from the INSIDE vertex a (so both triangles of the shared
 *   edge get the same point).  A triangle inside every plane comes out unchanged; the polygon is drawn as the fan
 *   (P0, Pk, Pk+1).  (More than 16 vertices -- impossible for a convex polygon -- drops the triangle.)
 * Projection of a polygon vertex: w > 0 or the polygon is dropped; xd = x / w, yd = y / w, zd = z / w, each |.| <= 4
 *   or dropped; X = int(floor((xd * hw + hw) * 256 + 0.5)), Y alike with hh (hw = 0.5 * W, hh = 0.5 * H: window
 *   coordinates in 1/256 pixel, below 2^22 in magnitude); zw = 0.5 * zd + 0.5; iw = 1 / w; su = tu * iw; sv = tv * iw.
 * Pixel (i, j), centre (256 i + 128, 256 j + 128): K4's integer edge functions (in binary64, exact) and antisymmetric
 *   tie rule, triangle turned to positive area; b_k = float(e_k) / float(area);
 *   z = (b0 z0 + b1 z1) + b2 z2 (linear in window space);  den = (b0 iw0 + b1 iw1) + b2 iw2;
 *   tu = ((b0 su0 + b1 su1) + b2 su2) / den, tv alike (perspective-correct);  discard if tu tu + tv tv > 1 or z is NaN;
 *   key = rint(clamp(z, 0, 1) * 16777215) << 32 | surfel index; the smallest key wins (GL_LESS, in order).
 * Resolve (the winner's colour; depends on the surfel and view_pos only), channels clamped to [0, 1] (NaN -> 0),
 *   byte = rint(c * 255) (GL's unorm conversion), the clear colour alike:
 *   mode 1: 0.5 * |dot(n, (1, 1, 1))| + 0.1;  mode 2: |n|;  mode 3: t = 1 - 1 / (1 + exp(c)), (t^2 = t t, t^3 = t^2 t)
 *   viridis: fma(1, k3, fma(t, k2, fma(t^2, k1, t^3 k0))) per channel;  mode 5: texel floor(((r * 255) / 259) * 260)
 *   of the colour map, black outside 0 .. 259 (border), bytes as stored, alpha 255;
 *   modes 0 / 4 (Phong): norm = normalize(n); diffuse colour mat_diffuse, or in mode 4 unpack(color) =
 *   ((int(color) >> 16) & 255) / 255 ...; per light in order: light_dir = normalize(-pos.xyz) if pos.w < 0.0001,
 *   else normalize(pos.xyz - p.xyz); diff = |dot(norm, light_dir)|; I = -light_dir, r = I - (2 dot(norm, I)) norm;
 *   sd = max(dot(view_dir, r), 0); spec = sd > 0 ? exp(shininess * log(sd)) : 0;
 *   result += ((La * Ma + Ld * (diff * colour)) + Ls * (spec * Ms)) + Me;  alpha as above.
 * Output rows are in glReadPixels order: row 0 is the bottom (window y = 0).
 */
#include <cstring>

#include "suma_internal.h"
#include "draw_vertex.h"

#define DRAW_THREADS 256
#define DRAW_LANE_TESTS 64 /* a quad with more pixel tests than this goes to the block-cooperative queue */
#define DRAW_MAXV 16
#define DRAW_BIG_BLOCKS 1024u

struct DrawLight {
  float pos[4], amb[3], dif[3], spe[3];
};
struct DrawArgs {
  const suma_surfel* surfels;
  const DevState* ds;
  const float* poses;
  uint32_t n_poses;
  int32_t W, H;
  float hw, hh;
  int32_t mode, backface, use_stability;
  float conf;
  float view[3];
  float mvp[16];
  unsigned long long* zbuf;
  uint32_t* queue; /* qcap ids, then the counter */
  uint32_t qcap;
};
struct ShadeArgs {
  uint32_t num_lights;
  DrawLight lights[SUMA_DRAW_MAX_LIGHTS];
  float mamb[3], mdif[3], mspe[3], memi[3], shin, alpha;
  uint32_t clear;
  uint32_t cmap[SUMA_DRAW_COLORS]; /* RGB bytes, alpha 255 */
};

struct cvtx {
  float c[6]; /* x, y, z, w, tu, tv */
};
struct dvtx {
  int32_t X, Y;
  float z, iw, su, sv;
};

SDEV v3 nrm3(v3 a) { return divs3(a, len3(a)); }
SDEV uint32_t unorm8(float x) {
  x = (x > 0.0f) ? x : 0.0f;
  x = (x < 1.0f) ? x : 1.0f;
  return (uint32_t)__builtin_rintf(x * 255.0f);
}

/* draw_surfels.geom up to the four clip-space corners; false: the surfel emits nothing */
SDEV bool quad_setup(const DrawArgs& a, uint32_t id, cvtx cv[4]) {
  const float4* sf = reinterpret_cast<const float4*>(a.surfels) + 4 * (size_t)id;
  const float4 s0 = sf[0], s1 = sf[1], s2 = sf[2], s3 = sf[3];
  float4 p, n;
  draw_vertex(a.poses, a.n_poses, s0, s1, s2.w, &p, &n);
  const float c = s1.w;
  float radius = s0.w, alpha = 1.0f;
  bool valid = (c > a.conf) || !a.use_stability;
  const v3 pp = mk3(p.x, p.y, p.z), nn = mk3(n.x, n.y, n.z);
  const v3 view_dir = nrm3(sub3(mk3(a.view[0], a.view[1], a.view[2]), pp));
  if (a.mode == 3) {
    valid = true;
  } else if (a.mode == 5) {
    if (!(s3.x != 0.0f)) valid = false;
  } else if (a.mode == 4) {
    valid = true;
    alpha = 1.0f - fclamp(a.conf - c, 0.1f, 1.0f);
    radius = radius / 1.41421356f;
  }
  valid = valid && (!a.backface || dot3(view_dir, nn) > 0.0f);
  if (!valid || alpha < 0.5f) return false; /* mode 0's material alpha is checked on the host (kernel-uniform) */
  const v3 u = nrm3(mk3(n.y - n.z, -n.x, n.x));
  const v3 v = nrm3(cross3(nn, u));
  const v3 ru = scale3(radius, u), rv = scale3(radius, v);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool pu = (k & 1) != 0, pv = (k & 2) != 0;
    float4 q;
    q.x = pu ? p.x + ru.x : p.x - ru.x;
    q.y = pu ? p.y + ru.y : p.y - ru.y;
    q.z = pu ? p.z + ru.z : p.z - ru.z;
    q.x = pv ? q.x + rv.x : q.x - rv.x;
    q.y = pv ? q.y + rv.y : q.y - rv.y;
    q.z = pv ? q.z + rv.z : q.z - rv.z;
    q.w = p.w;
    const float4 o = mat_vec(a.mvp, q);
    cv[k].c[0] = o.x;
    cv[k].c[1] = o.y;
    cv[k].c[2] = o.z;
    cv[k].c[3] = o.w;
    cv[k].c[4] = pu ? 1.0f : -1.0f;
    cv[k].c[5] = pv ? 1.0f : -1.0f;
    ok = ok && finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(o.w);
  }
  return ok;
}

SDEV float plane_dist(const float* c, int k) {
  const float x = c[0], y = c[1], z = c[2], w = c[3], w2 = w + w;
  switch (k) {
    case 0: return z + w;
    case 1: return w - z;
    case 2: return w2 + x;
    case 3: return w2 - x;
    case 4: return w2 + y;
    default: return w2 - y;
  }
}
SDEV bool project_vtx(const float* c, float hw, float hh, dvtx* r) {
  const float w = c[3];
  if (!(w > 0.0f)) return false;
  const float xd = c[0] / w, yd = c[1] / w, zd = c[2] / w;
  if (!(fabsf(xd) <= 4.0f && fabsf(yd) <= 4.0f && fabsf(zd) <= 4.0f)) return false;
  const float xw = xd * hw + hw, yw = yd * hh + hh;
  r->X = (int32_t)sdm_floor(xw * 256.0f + 0.5f);
  r->Y = (int32_t)sdm_floor(yw * 256.0f + 0.5f);
  r->z = 0.5f * zd + 0.5f;
  r->iw = 1.0f / w;
  r->su = c[4] * r->iw;
  r->sv = c[5] * r->iw;
  return true;
}

/* K4's edge function: exact in binary64 (all four differences are below 2^23) */
SDEV double dedge(const dvtx& a, const dvtx& b, int32_t px, int32_t py) {
  const double ux = (double)(b.X - a.X), uy = (double)(b.Y - a.Y), vx = (double)(px - a.X), vy = (double)(py - a.Y);
  return __builtin_fma(ux, vy, -(uy * vx));
}
SDEV bool downs(const dvtx& s, const dvtx& t) {
  const int32_t dx = t.X - s.X, dy = t.Y - s.Y;
  return dy > 0 || (dy == 0 && dx < 0);
}
/* a triangle turned to positive area (the per-pixel part below depends on nothing else) */
struct DrawTri {
  dvtx A, B, C;
  double area;
};
SDEV DrawTri tri_setup(const dvtx& A, const dvtx& B, const dvtx& C) {
  DrawTri t;
  t.A = A;
  t.B = B;
  t.C = C;
  t.area = dedge(A, B, C.X, C.Y);
  if (t.area < 0) {
    t.B = C;
    t.C = B;
    t.area = -t.area;
  }
  return t;
}
SDEV unsigned long long draw_key(const DrawTri& T, int32_t i, int32_t j, uint32_t id) {
  const int32_t px = 256 * i + 128, py = 256 * j + 128;
  const double w0 = dedge(T.B, T.C, px, py), w1 = dedge(T.C, T.A, px, py), w2 = dedge(T.A, T.B, px, py);
  const bool covered = (T.area != 0) && (w0 > 0 || (w0 == 0 && downs(T.B, T.C))) &&
                       (w1 > 0 || (w1 == 0 && downs(T.C, T.A))) && (w2 > 0 || (w2 == 0 && downs(T.A, T.B)));
  if (!covered) return SUMA_EMPTY_KEY;
  const float fa = (float)T.area;
  const float b0 = (float)(w0 + 0.0) / fa, b1 = (float)(w1 + 0.0) / fa, b2 = (float)(w2 + 0.0) / fa;
  const float z = (b0 * T.A.z + b1 * T.B.z) + b2 * T.C.z;
  const float den = (b0 * T.A.iw + b1 * T.B.iw) + b2 * T.C.iw;
  const float tu = ((b0 * T.A.su + b1 * T.B.su) + b2 * T.C.su) / den;
  const float tv = ((b0 * T.A.sv + b1 * T.B.sv) + b2 * T.C.sv) / den;
  if ((tu * tu + tv * tv) > 1.0f || sdm_isnan(z)) return SUMA_EMPTY_KEY;
  return ((unsigned long long)depth24(fclamp(z, 0.0f, 1.0f)) << 32) | id;
}

struct DrawBox {
  int32_t i0, j0, w, h;
};
SDEV DrawBox tri_box(const dvtx& A, const dvtx& B, const dvtx& C, int32_t W, int32_t H) {
  const int32_t minX = min(min(A.X, B.X), C.X), maxX = max(max(A.X, B.X), C.X);
  const int32_t minY = min(min(A.Y, B.Y), C.Y), maxY = max(max(A.Y, B.Y), C.Y);
  const int32_t i0 = max((minX - 128 + 255) >> 8, 0), i1 = min((maxX - 128) >> 8, W - 1);
  const int32_t j0 = max((minY - 128 + 255) >> 8, 0), j1 = min((maxY - 128) >> 8, H - 1);
  DrawBox b;
  b.i0 = i0;
  b.j0 = j0;
  b.w = i1 >= i0 ? i1 - i0 + 1 : 0;
  b.h = j1 >= j0 ? j1 - j0 + 1 : 0;
  return b;
}

SDEV void push_big(const DrawArgs& a, uint32_t id) {
  const uint32_t slot = atomicAdd(&a.queue[a.qcap], 1u);
  if (slot < a.qcap) a.queue[slot] = id; /* qcap = max_surfels >= the map size: never full */
}

/* one lane per surfel over the map's capacity (the size is read from HBM): no loop keeps the arguments alive */
__global__ void __launch_bounds__(DRAW_THREADS) kd_raster(DrawArgs a) {
  const uint32_t id = blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (id >= a.ds->n_surfels) return;
  {
    cvtx cv[4];
    if (!quad_setup(a, id, cv)) return;
    /* inside flags: bit 6 v + k for plane k of vertex v (the distances of plane_dist, written out) */
    uint32_t in_mask = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float x = cv[v].c[0], y = cv[v].c[1], z = cv[v].c[2], w = cv[v].c[3], w2 = w + w;
      in_mask |= ((z + w >= 0.0f) ? 1u : 0u) << (6 * v);
      in_mask |= ((w - z >= 0.0f) ? 2u : 0u) << (6 * v);
      in_mask |= ((w2 + x >= 0.0f) ? 4u : 0u) << (6 * v);
      in_mask |= ((w2 - x >= 0.0f) ? 8u : 0u) << (6 * v);
      in_mask |= ((w2 + y >= 0.0f) ? 16u : 0u) << (6 * v);
      in_mask |= ((w2 - y >= 0.0f) ? 32u : 0u) << (6 * v);
    }
    const uint32_t any_in = (in_mask | (in_mask >> 6) | (in_mask >> 12) | (in_mask >> 18)) & 63u;
    const bool out = any_in != 63u; /* every vertex outside one plane: every triangle clips to nothing */
    const bool all_in = in_mask == 0xffffffu;
    if (out) return;
    dvtx r[4];
    bool ok = all_in;
#pragma unroll
    for (int k = 0; k < 4; ++k) ok = ok && project_vtx(cv[k].c, a.hw, a.hh, &r[k]);
    if (!ok) {
      push_big(a, id); /* clipping needed */
      return;
    }
    const int32_t minX = min(min(r[0].X, r[1].X), min(r[2].X, r[3].X)), maxX = max(max(r[0].X, r[1].X), max(r[2].X, r[3].X));
    const int32_t minY = min(min(r[0].Y, r[1].Y), min(r[2].Y, r[3].Y)), maxY = max(max(r[0].Y, r[1].Y), max(r[2].Y, r[3].Y));
    const int32_t i0 = max((minX - 128 + 255) >> 8, 0), i1 = min((maxX - 128) >> 8, a.W - 1);
    const int32_t j0 = max((minY - 128 + 255) >> 8, 0), j1 = min((maxY - 128) >> 8, a.H - 1);
    if (i1 < i0 || j1 < j0) return;
    if ((int64_t)(i1 - i0 + 1) * (j1 - j0 + 1) > DRAW_LANE_TESTS) {
      push_big(a, id);
      return;
    }
    /* (v0, v1, v2), then (v2, v1, v3): the box of the quad holds both */
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const DrawTri T = tri_setup(r[2 * t], r[1], r[2 + t]);
      for (int32_t j = j0; j <= j1; ++j)
        for (int32_t i = i0; i <= i1; ++i) {
          const unsigned long long key = draw_key(T, i, j, id);
          if (key != SUMA_EMPTY_KEY) atomicMin(&a.zbuf[(size_t)j * (size_t)a.W + (size_t)i], key);
        }
    }
  }
}

/* one block per queued quad: lanes 0 / 1 clip triangle 0 / 1 in LDS and lay out its fan, then all lanes run the
 * pixel tests of every fan triangle */
__global__ void __launch_bounds__(DRAW_THREADS) kd_big(DrawArgs a) {
  __shared__ float s_poly[2][2][DRAW_MAXV][6];
  __shared__ dvtx s_v[2][DRAW_MAXV];
  __shared__ int32_t s_n[2];
  const uint32_t nq = min(a.queue[a.qcap], a.qcap);
  for (uint32_t e = blockIdx.x; e < nq; e += gridDim.x) {
    const uint32_t id = a.queue[e];
    if (threadIdx.x < 2) {
      const int t = threadIdx.x;
      cvtx cv[4];
      int32_t n = 0;
      if (quad_setup(a, id, cv)) {
        /* triangle 0: (v0, v1, v2), triangle 1: (v2, v1, v3) */
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          s_poly[t][0][0][j] = t == 0 ? cv[0].c[j] : cv[2].c[j];
          s_poly[t][0][1][j] = cv[1].c[j];
          s_poly[t][0][2][j] = t == 0 ? cv[2].c[j] : cv[3].c[j];
        }
        n = 3;
        int src = 0;
        for (int k = 0; k < 6 && n > 0; ++k) {
          float(*in)[6] = s_poly[t][src];
          float(*outp)[6] = s_poly[t][src ^ 1];
          int32_t m = 0;
          for (int32_t i = 0; i < n && m >= 0; ++i) {
            const float* cur = in[i];
            const float* prev = in[(i + n - 1) % n];
            const float dc = plane_dist(cur, k), dp = plane_dist(prev, k);
            const bool need_x = (dc >= 0.0f) ? (dp < 0.0f) : (dp >= 0.0f);
            const bool keep = dc >= 0.0f;
            if (m + (need_x ? 1 : 0) + (keep ? 1 : 0) > DRAW_MAXV) {
              m = -1;
              break;
            }
            if (need_x) {
              const float* ai = keep ? cur : prev; /* from the inside vertex */
              const float* bo = keep ? prev : cur;
              const float da = keep ? dc : dp, db = keep ? dp : dc;
              const float tt = da / (da - db);
#pragma unroll
              for (int j = 0; j < 6; ++j) outp[m][j] = ai[j] + tt * (bo[j] - ai[j]);
              ++m;
            }
            if (keep) {
#pragma unroll
              for (int j = 0; j < 6; ++j) outp[m][j] = cur[j];
              ++m;
            }
          }
          n = m < 0 ? 0 : m;
          src ^= 1;
        }
        if (n >= 3) {
          for (int32_t k = 0; k < n; ++k)
            if (!project_vtx(s_poly[t][src][k], a.hw, a.hh, &s_v[t][k])) n = 0;
        } else {
          n = 0;
        }
      }
      s_n[t] = n;
    }
    __syncthreads();
    for (int t = 0; t < 2; ++t) {
      const int32_t n = s_n[t];
      for (int32_t f = 1; f + 1 < n; ++f) {
        const DrawTri T = tri_setup(s_v[t][0], s_v[t][f], s_v[t][f + 1]);
        const DrawBox b = tri_box(T.A, T.B, T.C, a.W, a.H);
        const int32_t tests = b.w * b.h;
        for (int32_t q = threadIdx.x; q < tests; q += DRAW_THREADS) {
          const int32_t j = b.j0 + q / b.w, i = b.i0 + q % b.w;
          const unsigned long long key = draw_key(T, i, j, id);
          if (key != SUMA_EMPTY_KEY) atomicMin(&a.zbuf[(size_t)j * (size_t)a.W + (size_t)i], key);
        }
      }
    }
    __syncthreads();
  }
}

/* the winner's colour (draw_surfels.geom:84-147), as RGBA8 */
SDEV uint32_t draw_shade(const DrawArgs& a, const ShadeArgs& sh, uint32_t id) {
  const float4* sf = reinterpret_cast<const float4*>(a.surfels) + 4 * (size_t)id;
  const float4 s0 = sf[0], s1 = sf[1], s2 = sf[2], s3 = sf[3];
  float4 p, n;
  draw_vertex(a.poses, a.n_poses, s0, s1, s2.w, &p, &n);
  const float c = s1.w;
  const v3 pp = mk3(p.x, p.y, p.z), nn = mk3(n.x, n.y, n.z);
  if (a.mode == 1) {
    const uint32_t g = unorm8(0.5f * fabsf(dot3(nn, mk3(1.0f, 1.0f, 1.0f))) + 0.1f);
    return g | (g << 8) | (g << 16) | (255u << 24);
  }
  if (a.mode == 2) return unorm8(fabsf(n.x)) | (unorm8(fabsf(n.y)) << 8) | (unorm8(fabsf(n.z)) << 16) | (255u << 24);
  if (a.mode == 3) {
    const float t = 1.0f - 1.0f / (1.0f + sdm_exp(c));
    const float t2 = t * t, t3 = t2 * t;
    const float r = SDEV_FMA(1.0f, 0.29390206f, SDEV_FMA(t, 0.04439198f, SDEV_FMA(t2, -2.14404531f, t3 * 2.90912735f)));
    const float g = SDEV_FMA(1.0f, 0.01871256f, SDEV_FMA(t, 1.24131122f, SDEV_FMA(t2, -0.16906214f, t3 * -0.17293242f)));
    const float b = SDEV_FMA(1.0f, 0.34479632f, SDEV_FMA(t, 1.23042564f, SDEV_FMA(t2, -1.72405244f, t3 * 0.17848859f)));
    return unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | (255u << 24);
  }
  if (a.mode == 5) {
    const float fi = sdm_floor(((s3.x * 255.0f) / 259.0f) * 260.0f);
    return (fi >= 0.0f && fi < 260.0f) ? sh.cmap[(int32_t)fi] : (255u << 24);
  }
  /* Phong (modes 0 and 4) */
  const v3 norm = nrm3(nn);
  const v3 view_dir = nrm3(sub3(mk3(a.view[0], a.view[1], a.view[2]), pp));
  v3 sc = mk3(sh.mdif[0], sh.mdif[1], sh.mdif[2]);
  float alpha = sh.alpha;
  if (a.mode == 4) {
    const float col = s2.y;
    const int32_t ci = (col >= 0.0f && col < 2147483648.0f) ? (int32_t)col : 0;
    sc = mk3((float)((ci >> 16) & 0xFF) / 255.0f, (float)((ci >> 8) & 0xFF) / 255.0f, (float)(ci & 0xFF) / 255.0f);
    alpha = 1.0f - fclamp(a.conf - c, 0.1f, 1.0f);
  }
  float res[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t l = 0; l < sh.num_lights; ++l) {
    const DrawLight& L = sh.lights[l];
    const v3 lp = mk3(L.pos[0], L.pos[1], L.pos[2]);
    const v3 ld = (L.pos[3] < 0.0001f) ? nrm3(neg3(lp)) : nrm3(sub3(lp, pp));
    const float diff = fabsf(dot3(norm, ld));
    const v3 I = neg3(ld);
    const float t = 2.0f * dot3(norm, I);
    const v3 refl = mk3(I.x - t * norm.x, I.y - t * norm.y, I.z - t * norm.z);
    float sd = dot3(view_dir, refl);
    sd = (sd < 0.0f) ? 0.0f : sd;
    const float spec = (sd > 0.0f) ? sdm_exp(sh.shin * sdm_log(sd)) : 0.0f;
    const float scv[3] = {sc.x, sc.y, sc.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float amb = L.amb[k] * sh.mamb[k];
      const float dif = L.dif[k] * (diff * scv[k]);
      const float spc = L.spe[k] * (spec * sh.mspe[k]);
      res[k] = res[k] + (((amb + dif) + spc) + sh.memi[k]);
    }
  }
  return unorm8(res[0]) | (unorm8(res[1]) << 8) | (unorm8(res[2]) << 16) | (unorm8(alpha) << 24);
}

__global__ void __launch_bounds__(DRAW_THREADS)
    kd_resolve(DrawArgs a, ShadeArgs sh, uint32_t* __restrict__ rgba, int32_t* __restrict__ ids) {
  const uint32_t P = (uint32_t)a.W * (uint32_t)a.H;
  const uint32_t p = blockIdx.x * DRAW_THREADS + threadIdx.x;
  if (p == 0) a.queue[a.qcap] = 0u; /* the large-quad pass of this draw has finished: re-arm the queue */
  if (p >= P) return;
  const unsigned long long key = a.zbuf[p];
  uint32_t col = sh.clear;
  int32_t id = -1;
  if (key != SUMA_EMPTY_KEY) {
    a.zbuf[p] = SUMA_EMPTY_KEY;
    id = (int32_t)(uint32_t)(key & 0xffffffffull);
    col = draw_shade(a, sh, (uint32_t)id);
  }
  rgba[p] = col;
  if (ids) ids[p] = id;
}

/* ---- host side ---- */
extern "C" void suma_draw_params_default(suma_draw_params* d) {
  static const float dirs[4][4] = {{1, -1, 1, 0}, {-1, -1, 1, 0}, {1, -1, -1, 0}, {-1, -1, -1, 0}};
  if (!d) return;
  std::memset(d, 0, sizeof(*d));
  d->color_mode = 5;
  d->conf_threshold = 10.0f;
  for (int k = 0; k < 4; ++k) d->clear_color[k] = 1.0f;
  d->num_lights = 1;
  const float pos0[4] = {0.0f, -1.0f, -1.0f, 0.0f}, dif0[3] = {0.6f, 0.52944f, 0.4566f};
  for (int k = 0; k < 4; ++k) d->lights[0].position[k] = pos0[k];
  for (int k = 0; k < 3; ++k) {
    d->lights[0].ambient[k] = 0.4f;
    d->lights[0].diffuse[k] = dif0[k];
    d->lights[0].specular[k] = 0.3f;
  }
  for (int i = 1; i < 5; ++i)
    for (int k = 0; k < 4; ++k) {
      d->lights[i].position[k] = dirs[i - 1][k];
      if (k < 3) d->lights[i].ambient[k] = d->lights[i].diffuse[k] = d->lights[i].specular[k] = 0.1f;
    }
  const float amb[3] = {0.75f, 0.65f, 0.5f}, dif[3] = {1.0f, 0.9f, 0.7f};
  for (int k = 0; k < 3; ++k) {
    d->mat_ambient[k] = amb[k];
    d->mat_diffuse[k] = dif[k];
    d->mat_specular[k] = 1.0f;
  }
  d->mat_shininess = 16.0f;
  d->mat_alpha = 1.0f;
}

extern "C" int suma_map_draw(suma_ctx* c, const suma_draw_params* dp, void* d_rgba8, int32_t* d_ids) {
  if (!c) return SUMA_ERR_INVALID;
  if (!dp) return fail(c, SUMA_ERR_INVALID, "suma_map_draw: NULL parameters");
  if (!d_rgba8) return fail(c, SUMA_ERR_INVALID, "suma_map_draw: NULL colour buffer");
  if (dp->width < 1 || dp->width > SUMA_DRAW_MAX_SIZE || dp->height < 1 || dp->height > SUMA_DRAW_MAX_SIZE)
    return fail(c, SUMA_ERR_INVALID, "suma_map_draw: width x height = " + std::to_string(dp->width) + " x " +
                                     std::to_string(dp->height) + " (each must be 1 .. " +
                                     std::to_string(SUMA_DRAW_MAX_SIZE) + ")");
  if (dp->color_mode < 0 || dp->color_mode > 5)
    return fail(c, SUMA_ERR_INVALID,
                "suma_map_draw: color_mode = " + std::to_string(dp->color_mode) + " (must be 0 .. 5)");
  if (dp->num_lights > SUMA_DRAW_MAX_LIGHTS)
    return fail(c, SUMA_ERR_INVALID, "suma_map_draw: num_lights = " + std::to_string(dp->num_lights) + " (at most " +
                                     std::to_string(SUMA_DRAW_MAX_LIGHTS) + ")");
  const size_t P = (size_t)dp->width * dp->height;
  int r = grow(c, c->draw_zbuf, P, {c->stream});
  if (r < 0) return r;
  if (r) HIP_TRY(c, hipMemsetAsync(c->draw_zbuf, 0xFF, P * 8, c->stream)); /* left cleared by every resolve */
  r = grow(c, c->draw_queue, (size_t)c->p.max_surfels + 1, {});
  if (r < 0) return r;
  if (r) HIP_TRY(c, hipMemsetAsync(c->draw_queue + c->p.max_surfels, 0, sizeof(uint32_t), c->stream));
  DrawArgs a;
  a.surfels = c->surfels[c->cur];
  a.ds = c->ds;
  a.poses = c->poses;
  a.n_poses = c->p.max_poses;
  a.W = (int32_t)dp->width;
  a.H = (int32_t)dp->height;
  a.hw = 0.5f * (float)dp->width;
  a.hh = 0.5f * (float)dp->height;
  a.mode = dp->color_mode;
  a.backface = dp->backface_culling ? 1 : 0;
  a.use_stability = dp->use_stability ? 1 : 0;
  a.conf = dp->conf_threshold;
  for (int k = 0; k < 3; ++k) a.view[k] = dp->view_pos[k];
  for (int k = 0; k < 16; ++k) a.mvp[k] = dp->mvp[k];
  a.zbuf = c->draw_zbuf;
  a.queue = c->draw_queue;
  a.qcap = c->p.max_surfels;

  ShadeArgs sh;
  sh.num_lights = dp->num_lights;
  for (uint32_t l = 0; l < SUMA_DRAW_MAX_LIGHTS; ++l) {
    const suma_draw_light& L = dp->lights[l];
    for (int k = 0; k < 4; ++k) sh.lights[l].pos[k] = L.position[k];
    for (int k = 0; k < 3; ++k) {
      sh.lights[l].amb[k] = L.ambient[k];
      sh.lights[l].dif[k] = L.diffuse[k];
      sh.lights[l].spe[k] = L.specular[k];
    }
  }
  for (int k = 0; k < 3; ++k) {
    sh.mamb[k] = dp->mat_ambient[k];
    sh.mdif[k] = dp->mat_diffuse[k];
    sh.mspe[k] = dp->mat_specular[k];
    sh.memi[k] = dp->mat_emission[k];
  }
  sh.shin = dp->mat_shininess;
  sh.alpha = dp->mat_alpha;
  sh.clear = 0;
  for (int k = 0; k < 4; ++k) {
    float x = dp->clear_color[k];
    x = (x > 0.0f) ? x : 0.0f;
    x = (x < 1.0f) ? x : 1.0f;
    sh.clear |= (uint32_t)std::rint(x * 255.0f) << (8 * k);
  }
  for (int t = 0; t < SUMA_DRAW_COLORS; ++t)
    sh.cmap[t] = (uint32_t)dp->color_map[t][0] | ((uint32_t)dp->color_map[t][1] << 8) |
                 ((uint32_t)dp->color_map[t][2] << 16) | (255u << 24);

  /* mode 0 draws nothing when the material's alpha is below 0.5 (draw_surfels.frag:17): uniform over the map */
  const bool nothing = (dp->color_mode == 0) && (dp->mat_alpha < 0.5f);
  {
    ProfScope ps(c, "draw_raster", 64.0 * c->known_surfels);
    if (!nothing && c->p.max_surfels)
      kd_raster<<<(c->p.max_surfels + DRAW_THREADS - 1) / DRAW_THREADS, DRAW_THREADS, 0, c->stream>>>(a);
  }
  {
    ProfScope ps(c, "draw_big", 0.0);
    if (!nothing) kd_big<<<DRAW_BIG_BLOCKS, DRAW_THREADS, 0, c->stream>>>(a);
  }
  {
    ProfScope ps(c, "draw_resolve", 16.0 * (double)P);
    kd_resolve<<<(unsigned)((P + DRAW_THREADS - 1) / DRAW_THREADS), DRAW_THREADS, 0, c->stream>>>(
        a, sh, reinterpret_cast<uint32_t*>(d_rgba8), d_ids);
  }
  HIP_TRY(c, hipGetLastError());
  return SUMA_OK;
}
