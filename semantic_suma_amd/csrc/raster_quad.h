/*
 * raster_quad.h -- the pixel test of k_render.hip's rasteriser (K4, phase 2), device and host.
 *
 * A surfel is drawn as the triangle strip (v0,v1,v2), (v2,v1,v3) of its projected quad.  raster_key() is the
 * SPECIFICATION of one triangle at one pixel centre.  quad_setup() + quad_test() compute min(raster_key(T1),
 * raster_key(T2)) to the bit, with everything that depends on the quad alone -- signed areas, orientation, the float area
 * and its refined reciprocal, the edge-ownership decisions -- done once per quad instead of once per pixel test and
 * triangle, and the diagonal both triangles share evaluated once.  tests/cpp/raster_quad_driver.cpp holds the two
 * against each other on the host (this file compiles there without HIP: SDEV is then a plain inline function).
 *
 * fp32 / fp64, every operation as written (-ffp-contract=off): these bodies are specification.
 */
#ifndef SUMA_RASTER_QUAD_H_
#define SUMA_RASTER_QUAD_H_

#include <stdint.h>

#ifdef SDEV /* device: behind dev_math.h */
#define RQ_RCP(x) __builtin_amdgcn_rcpf(x)
#else /* host: nothing of HIP; exact_div.h is correctly rounded for ANY reciprocal within 1 ulp, 1 / x is one */
#define SDEV static inline
#define RQ_RCP(x) (1.0f / (x))
#define SUMA_EMPTY_KEY (~0ull)
SDEV uint32_t depth24(float zw) { return (uint32_t)__builtin_rintf(zw * 16777215.0f); } /* as dev_math.h */
#endif
#define EXDIV_FN SDEV
#include "exact_div.h"

enum { TIE_LOW_INDEX = 0, TIE_HIGH_INDEX_OLD = 1, TIE_HIGH_INDEX_NEW = 2 };

struct rvtx {
  int32_t X, Y; /* window coordinates in 1/256 pixel (|X| < 2^21: 20 bits of image + seam unwrap) */
  float z, tu, tv;
};

/* Edge function of the directed edge a->b at point (px, py): an exact integer below 2^47 in magnitude (the four
 * differences are below 2^23).  Formed in binary64: each product of two such integers is exact (46 bits), and the fused
 * multiply-add delivers their exact difference (representable, so its one rounding rounds nothing) -- the same integer
 * the 64-bit form (b.X - a.X) * (py - a.Y) - (b.Y - a.Y) * (px - a.X) computes, as a double.  Why: the 64-bit form costs
 * two 32 x 32 -> 64-bit multiplies, add-with-carry pairs and 64-bit compares per edge, and its conversion to float is a
 * dozen instructions (count leading zeros, shifts, rounding) where v_cvt_f32_f64 is one; binary64 issues at the ordinary
 * VALU rate on gfx950 (profiles/r05_instr_rate_gfx950.txt).  Per pair of pixel tests 831 -> 684 VALU instructions; the
 * pass is 5 % faster where it is issue-bound (50 M surfels) and unchanged at the steady 1 M map
 * (profiles/r05_second_session_experiments.txt).  The one value the integer form cannot produce is -0 (two zero products
 * of unlike sign): comparisons do not see it, and edge_to_float() turns it into the +0 an integer 0 converts to. */
SDEV double edge_fn(const rvtx& a, const rvtx& b, int32_t px, int32_t py) {
  const double ux = (double)(b.X - a.X), uy = (double)(b.Y - a.Y), vx = (double)(px - a.X), vy = (double)(py - a.Y);
  return __builtin_fma(ux, vy, -(uy * vx));
}
SDEV float edge_to_float(double w) { return (float)(w + 0.0); } /* (float)(long long): -0 -> +0 */
/* ownership of a pixel centre exactly on an edge: antisymmetric in the edge direction, so a
 * pixel on the diagonal shared by the two strip triangles is produced exactly once */
SDEV bool owns_edge(const rvtx& s, const rvtx& t) {
  int32_t dx = t.X - s.X, dy = t.Y - s.Y;
  return dy > 0 || (dy == 0 && dx < 0);
}

SDEV unsigned long long render_key(uint32_t z24, uint32_t id, int tie) {
  /* GL_LESS, in order: equal depth keeps the earlier primitive (lower id).  GL_LEQUAL
   * (render_composed, SurfelMap.cpp:1126): equal depth takes the later primitive, and the "new"
   * pass is drawn after the "old" pass into the same depth buffer. */
  if (tie == TIE_LOW_INDEX) return ((unsigned long long)z24 << 32) | id;
  unsigned long long pass = (tie == TIE_HIGH_INDEX_OLD) ? 1u : 0u;
  return ((unsigned long long)z24 << 33) | (pass << 32) | (unsigned long long)(0xffffffffu - id);
}

/* One triangle at one pixel centre: coverage (top-left style ownership rule), affine interpolation
 * of depth and disc coordinates, disc + near/far tests.  Returns the z-buffer key of the fragment or
 * SUMA_EMPTY_KEY if the triangle produces none.  Every quantity is a function of the triangle and the
 * pixel only, so the work can be distributed freely over lanes. */
SDEV unsigned long long raster_key(rvtx A, rvtx B, rvtx C, int32_t i, int32_t j, uint32_t id, int tie) {
  double area = edge_fn(A, B, C.X, C.Y);
  if (area < 0) {
    rvtx t = B;
    B = C;
    C = t;
    area = -area;
  }
  const int32_t px = 256 * i + 128, py = 256 * j + 128;
  const double w0 = edge_fn(B, C, px, py), w1 = edge_fn(C, A, px, py), w2 = edge_fn(A, B, px, py);
  const bool covered = (area != 0) && (w0 > 0 || (w0 == 0 && owns_edge(B, C))) &&
                       (w1 > 0 || (w1 == 0 && owns_edge(C, A))) && (w2 > 0 || (w2 == 0 && owns_edge(A, B)));
  unsigned long long key = SUMA_EMPTY_KEY;
  if (covered) {
    const float fa = (float)area;
#ifdef SUMA_BARY_PLAIN_DIV
    float b0 = edge_to_float(w0) / fa, b1 = edge_to_float(w1) / fa, b2 = edge_to_float(w2) / fa;
#else
    /* three quotients by one denominator; the operands are integers in [0, 2^46] over a positive integer area (X, Y
     * below 2^21, so every edge function is below 2^45 in magnitude), and a zero numerator gives an exact 0: the short
     * sequence of exact_div.h is correctly rounded there (tools/div_study.c) -- 18 instead of 33 instructions, the
     * same bits as the three `/` (the parity suite is the check) */
    const float fr = exdiv_refine(fa, RQ_RCP(fa));
    float b0 = exdiv_quot(edge_to_float(w0), fa, fr), b1 = exdiv_quot(edge_to_float(w1), fa, fr),
          b2 = exdiv_quot(edge_to_float(w2), fa, fr);
#endif
    float tu = (b0 * A.tu + b1 * B.tu) + b2 * C.tu;
    float tv = (b0 * A.tv + b1 * B.tv) + b2 * C.tv;
    float z = (b0 * A.z + b1 * B.z) + b2 * C.z;
    /* render_surfels.frag:22 disc test; near / far clipping */
    if (!((tu * tu + tv * tv) > 1.0f) && (z >= 0.0f && z <= 1.0f)) key = render_key(depth24(z), id, tie);
  }
  return key;
}

/* ---- the same keys with the quad's own work done once ----
 *
 * Write E(s,t;p) for edge_fn(s, t, p).  It is the exact integer (t - s) x (p - s), so
 *   E(t,s;p) = -E(s,t;p)                       (what raster_key's swap of B and C does to every edge), and
 *   E(s,t;p) = (p - s) x (p - t)               (t - s = (p - s) - (p - t), and (p - s) x (p - s) = 0):
 * five edges of one pixel need the four differences p - v_k and nothing else of the quad.  The differences are below
 * 2^23 in magnitude, so the products and their difference are exact in binary64 as in edge_fn.  A -0 where edge_fn
 * gives +0 (or the reverse) is harmless for the reason given there.
 *
 * A triangle (A,B,C) has the raw edge values e0 = E(B,C;p), e1 = E(C,A;p), e2 = E(A,B;p) and the raw area a = E(A,B;C).
 * raster_key works on (w0, w1, w2) = (e0, e1, e2) over the vertices (A, B, C) when a >= 0, and on (-e0, -e2, -e1) over
 * (A, C, B) when a < 0.  So with g_k = e_k or -e_k:
 *   - coverage is the same conjunction over k either way: g_k > 0, or g_k == 0 on an edge the ORIENTED triangle owns;
 *   - in a covered triangle every g_k >= 0, i.e. g_k = |e_k|, and edge_to_float(g_k) = (float)|e_k| (|-0| = +0);
 *   - the quotient |e_k| / |a| multiplies the same vertex either way (e0: A, e1: B, e2: C); only the ORDER of the last
 *     two terms of each interpolation sum follows the swap.
 * Ownership of the oriented edges: owns_edge(t, s) = !owns_edge(s, t) unless s and t coincide, and then the triangle
 * has no area and produces nothing whatever the bits say.
 *
 * What the set-up keeps per triangle is therefore, for each raw edge value, the SIGN CLASSES that count as covered:
 * positive (a > 0) or negative (a < 0), and zero where the oriented triangle owns the edge; none at all when a == 0.
 * They are kept as the class mask of v_cmp_class_f64 (bit 3: negative normal, bits 5 and 6: -0 and +0, bit 8: positive
 * normal), so that one instruction decides an edge.  The instruction reads ten mask bits.  An edge value is a finite
 * integer: it is zero or normal, and the mask bits of the other classes (NaN, infinity, denormal: bits 0-2, 4, 7, 9) are
 * never looked at -- the masks of the three edges overlap there, and the orientation bit sits there. */
enum {
  QC_NEG = 1 << 3,
  QC_ZERO = (1 << 5) | (1 << 6),
  QC_POS = 1 << 8,
  QS_NEG = 1,      /* bit 0 of a triangle's word: a < 0, raster_key swaps B and C.  Bits 1 and 2 are not read here (k_render
                      keeps a record's slot mask there) */
  QS_EDGE_SHIFT = 6 /* word >> 6 k: the class mask of e_k in bits 3-8 */
};
struct QuadSetup {
  float fa[2]; /* (float)|a| per triangle */
#ifndef SUMA_BARY_PLAIN_DIV
  float fr[2]; /* its refined reciprocal (exact_div.h) */
#endif
  uint32_t tri[2];
};

/* the word of triangle (A,B,C); flip2: the caller will test -e2 = E(B,A;p) in place of e2 (the strip's diagonal) */
SDEV uint32_t tri_setup(const rvtx& A, const rvtx& B, const rvtx& C, bool flip2, float* fa) {
  const double a = edge_fn(A, B, C.X, C.Y);
  const bool neg = a < 0;
  *fa = (float)__builtin_fabs(a);
  if (a == 0) return 0u;
  const uint32_t in = neg ? (uint32_t)QC_NEG : (uint32_t)QC_POS, in2 = (neg != flip2) ? (uint32_t)QC_NEG : (uint32_t)QC_POS;
  const uint32_t m0 = in | ((owns_edge(B, C) != neg) ? (uint32_t)QC_ZERO : 0u),
                 m1 = in | ((owns_edge(C, A) != neg) ? (uint32_t)QC_ZERO : 0u),
                 m2 = in2 | ((owns_edge(A, B) != neg) ? (uint32_t)QC_ZERO : 0u);
  return (neg ? (uint32_t)QS_NEG : 0u) | m0 | (m1 << QS_EDGE_SHIFT) | (m2 << (2 * QS_EDGE_SHIFT));
}
SDEV QuadSetup quad_setup(const rvtx& v0, const rvtx& v1, const rvtx& v2, const rvtx& v3) {
  QuadSetup s;
  s.tri[0] = tri_setup(v0, v1, v2, false, &s.fa[0]);
  s.tri[1] = tri_setup(v2, v1, v3, true, &s.fa[1]);
#ifndef SUMA_BARY_PLAIN_DIV
  s.fr[0] = exdiv_refine(s.fa[0], RQ_RCP(s.fa[0])); /* a degenerate triangle's is never read */
  s.fr[1] = exdiv_refine(s.fa[1], RQ_RCP(s.fa[1]));
#endif
  return s;
}

/* is the sign class of the edge value e in the mask?  (e is zero or normal) */
SDEV bool edge_covers(double e, uint32_t mask) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_class(e, (int)mask);
#else
  return (mask & (e < 0 ? (uint32_t)QC_NEG : e > 0 ? (uint32_t)QC_POS : (uint32_t)QC_ZERO)) != 0;
#endif
}
SDEV bool tri_covers(uint32_t word, double e0, double e1, double e2) {
  return edge_covers(e0, word) && edge_covers(e1, word >> QS_EDGE_SHIFT) && edge_covers(e2, word >> (2 * QS_EDGE_SHIFT));
}

/* a covered triangle from the float numerators (float)|e_k|: raster_key from `fa` on */
SDEV unsigned long long tri_key(bool neg, float fa, float fr, float nA, float nB, float nC, const rvtx& A, const rvtx& B,
                                const rvtx& C, uint32_t id, int tie) {
#ifdef SUMA_BARY_PLAIN_DIV
  (void)fr;
  const float bA = nA / fa, bB = nB / fa, bC = nC / fa;
#else
  const float bA = exdiv_quot(nA, fa, fr), bB = exdiv_quot(nB, fa, fr), bC = exdiv_quot(nC, fa, fr);
#endif
  /* (b0 * A'.f + b1 * B'.f) + b2 * C'.f over the oriented vertices: B's term first unless they were swapped */
  const float uB = bB * B.tu, uC = bC * C.tu, vB = bB * B.tv, vC = bC * C.tv, zB = bB * B.z, zC = bC * C.z;
  const float tu = (bA * A.tu + (neg ? uC : uB)) + (neg ? uB : uC);
  const float tv = (bA * A.tv + (neg ? vC : vB)) + (neg ? vB : vC);
  const float z = (bA * A.z + (neg ? zC : zB)) + (neg ? zB : zC);
  /* render_surfels.frag:22 disc test; near / far clipping */
  if (!((tu * tu + tv * tv) > 1.0f) && (z >= 0.0f && z <= 1.0f)) return render_key(depth24(z), id, tie);
  return SUMA_EMPTY_KEY;
}

/* min(raster_key(v0,v1,v2), raster_key(v2,v1,v3)) at pixel (i, j): five edge values from four differences; the strip's
 * diagonal is T1's e0 = E(v1,v2;p) and, negated, T2's e2 = E(v2,v1;p) -- T2's word holds that edge's classes mirrored.
 * The coverage decisions and the float numerators are formed before either triangle is interpolated, so that no binary64
 * value lives any longer. */
SDEV unsigned long long quad_test(const QuadSetup& s, const rvtx& v0, const rvtx& v1, const rvtx& v2, const rvtx& v3,
                                  int32_t i, int32_t j, uint32_t id, int tie) {
  const int32_t px = 256 * i + 128, py = 256 * j + 128;
  const double x0 = (double)(px - v0.X), y0 = (double)(py - v0.Y), x1 = (double)(px - v1.X), y1 = (double)(py - v1.Y),
               x2 = (double)(px - v2.X), y2 = (double)(py - v2.Y), x3 = (double)(px - v3.X), y3 = (double)(py - v3.Y);
  const double e12 = __builtin_fma(x1, y2, -(y1 * x2)), e20 = __builtin_fma(x2, y0, -(y2 * x0)),
               e01 = __builtin_fma(x0, y1, -(y0 * x1)), e13 = __builtin_fma(x1, y3, -(y1 * x3)),
               e32 = __builtin_fma(x3, y2, -(y3 * x2));
  const bool c1 = tri_covers(s.tri[0], e12, e20, e01), c2 = tri_covers(s.tri[1], e13, e32, e12);
  const float n12 = (float)__builtin_fabs(e12), n20 = (float)__builtin_fabs(e20), n01 = (float)__builtin_fabs(e01),
              n13 = (float)__builtin_fabs(e13), n32 = (float)__builtin_fabs(e32);
#ifdef SUMA_BARY_PLAIN_DIV
  const float fr0 = 0.0f, fr1 = 0.0f;
#else
  const float fr0 = s.fr[0], fr1 = s.fr[1];
#endif
  unsigned long long key = SUMA_EMPTY_KEY;
  if (c1) key = tri_key((s.tri[0] & QS_NEG) != 0, s.fa[0], fr0, n12, n20, n01, v0, v1, v2, id, tie);
  if (c2) {
    const unsigned long long kb = tri_key((s.tri[1] & QS_NEG) != 0, s.fa[1], fr1, n13, n32, n12, v2, v1, v3, id, tie);
    key = kb < key ? kb : key;
  }
  return key;
}

#endif
