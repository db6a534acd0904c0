/*
 * k_posegraph.hip -- the pose-graph optimiser behind suma_posegraph_* (include/suma_hip.h): the reference's Posegraph
 * (src/core/Posegraph.cpp), i.e. gtsam's PriorFactor / BetweenFactor<Pose3> graph optimised by Levenberg-Marquardt,
 * in fp64 on the device.  The mathematics is DESIGN.md "Pose graph"; tests/posegraph_host.py restates it on the host.
 *
 * Per LM iteration (the system never leaves the device; the host reads one small status record per damped solve):
 *   k_pg_factor (lin)   one lane per factor: e = Log(Z^-1 Xi^-1 Xj), Ji, Jj, and the blocks Ji'W Ji, Ji'W Jj,
 *                       Jj'W Jj, Ji'W e, Jj'W e of the factor (W = information)
 *   k_pg_nodes          one lane per node: its diagonal block and gradient, summed over its factors in factor order
 *                       (CSR built once per structure change) -- no atomics, bit-reproducible
 *   k_pg_pairs          one lane per distinct node pair (i < j): the off-diagonal block, its factors summed in insertion
 *                       order; |i - j| = 1 goes to the dense band U[i], the rest to the off-band list O
 * then per damped solve (lambda):
 *   k_pg_solve          ONE workgroup: preconditioned CG on (H + lambda I) delta = -g, preconditioned by an exact
 *                       block-cyclic-reduction solve of the block-tridiagonal part (diagonal + band); the linearised
 *                       cost change of the step is written to the status record
 *   k_pg_retract        X_new = X Exp(delta) per node
 *   k_pg_factor (eval)  per-factor energy at X_new,  k_pg_energy: their sum in a fixed order
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "suma_internal.h"

#define PG_SOLVE_THREADS 256
#define PG_BLOCK 256
#define PG_LIN 120 /* per factor: Hii 36 | Hij 36 | Hjj 36 | gi 6 | gj 6 (row-major) */
#define PG_SERIES_THETA 0.5

/* ---- SE(3) in fp64, tangent [omega, v] (the same formulas as tests/posegraph_host.py) ---------------------------- */

__device__ inline double pg_horner7(double t2, double c0, double c1, double c2, double c3, double c4, double c5,
                                    double c6) {
  return c0 + t2 * (c1 + t2 * (c2 + t2 * (c3 + t2 * (c4 + t2 * (c5 + t2 * c6)))));
}

/* A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3, D = 1/t^2 - cot(t/2) / (2t),
 * qb = (t^2 + 2 cos t - 2) / (2 t^4), qc = (2t - 3 sin t + t cos t) / (2 t^5); Taylor series below 0.5 */
struct PgCoef {
  double A, B, C, D, qb, qc;
};

__device__ inline PgCoef pg_coef(double th) {
  PgCoef k;
  if (th < PG_SERIES_THETA) {
    const double t2 = th * th;
    k.A = pg_horner7(t2, 1.0, -1.0 / 6, 1.0 / 120, -1.0 / 5040, 1.0 / 362880, -1.0 / 39916800, 1.0 / 6227020800);
    k.B = pg_horner7(t2, 1.0 / 2, -1.0 / 24, 1.0 / 720, -1.0 / 40320, 1.0 / 3628800, -1.0 / 479001600,
                     1.0 / 87178291200);
    k.C = pg_horner7(t2, 1.0 / 6, -1.0 / 120, 1.0 / 5040, -1.0 / 362880, 1.0 / 39916800, -1.0 / 6227020800,
                     1.0 / 1307674368000);
    k.D = pg_horner7(t2, 1.0 / 12, 1.0 / 720, 1.0 / 30240, 1.0 / 1209600, 1.0 / 47900160, 691.0 / 1307674368000,
                     7.0 / 523069747200);
    k.qb = pg_horner7(t2, 1.0 / 24, -1.0 / 720, 1.0 / 40320, -1.0 / 3628800, 1.0 / 479001600, -1.0 / 87178291200,
                      1.0 / 20922789888000);
    k.qc = pg_horner7(t2, 1.0 / 120, -1.0 / 2520, 1.0 / 120960, -1.0 / 9979200, 1.0 / 1245404160,
                      -1.0 / 217945728000, 1.0 / 50812489728000);
  } else {
    const double s = sin(th), c = cos(th), t2 = th * th;
    k.A = s / th;
    k.B = (1 - c) / t2;
    k.C = (th - s) / (t2 * th);
    k.D = 1 / t2 - cos(th / 2) / sin(th / 2) / (2 * th);
    k.qb = (t2 + 2 * c - 2) / (2 * (t2 * t2));
    k.qc = (2 * th - 3 * s + th * c) / (2 * (t2 * t2 * th));
  }
  return k;
}

__device__ inline void pg_hat(const double w[3], double H[9]) {
  H[0] = 0, H[1] = -w[2], H[2] = w[1];
  H[3] = w[2], H[4] = 0, H[5] = -w[0];
  H[6] = -w[1], H[7] = w[0], H[8] = 0;
}

__device__ inline void pg_mm3(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
}

__device__ inline void pg_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

/* pose = R (row-major 3x3) | t: 12 doubles */
__device__ inline void pg_load(const double* p, double R[9], double t[3]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = p[k];
  t[0] = p[9], t[1] = p[10], t[2] = p[11];
}

/* (A^-1 B) for rigid A, B */
__device__ inline void pg_between(const double Ra[9], const double ta[3], const double Rb[9], const double tb[3],
                                  double R[9], double t[3]) {
  const double d[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = Ra[0 * 3 + i] * Rb[0 * 3 + j] + Ra[1 * 3 + i] * Rb[1 * 3 + j] + Ra[2 * 3 + i] * Rb[2 * 3 + j];
    t[i] = Ra[0 * 3 + i] * d[0] + Ra[1 * 3 + i] * d[1] + Ra[2 * 3 + i] * d[2];
  }
}

__device__ inline void pg_so3_log(const double R[9], double om[3]) {
  const double w[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double s = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double th = atan2(s, c);
  if (c < -0.5) { /* near pi the skew part loses the axis: take it from the symmetric part */
    double B[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) B[i * 3 + j] = 0.5 * (R[i * 3 + j] + R[j * 3 + i]) - (i == j ? c : 0.0);
    int k = 0;
    if (B[4] > B[0]) k = 1;
    if (B[8] > B[k * 4]) k = 2;
    double a[3] = {B[0 * 3 + k], B[1 * 3 + k], B[2 * 3 + k]};
    const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    a[0] /= na, a[1] /= na, a[2] /= na;
    const double sg = (a[0] * w[0] + a[1] * w[1] + a[2] * w[2]) < 0 ? -th : th;
    om[0] = sg * a[0], om[1] = sg * a[1], om[2] = sg * a[2];
  } else {
    const double f = s > 0 ? th / s : 1.0;
    om[0] = f * w[0], om[1] = f * w[1], om[2] = f * w[2];
  }
}

__device__ inline void pg_se3_log(const double R[9], const double t[3], double xi[6]) {
  pg_so3_log(R, xi);
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  const double D = pg_coef(th).D;
  double wt[3], wwt[3];
  pg_cross(xi, t, wt);
  pg_cross(xi, wt, wwt);
#pragma unroll
  for (int i = 0; i < 3; ++i) xi[3 + i] = t[i] - 0.5 * wt[i] + D * wwt[i];
}

__device__ inline void pg_se3_exp(const double xi[6], double R[9], double t[3]) {
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  const PgCoef k = pg_coef(th);
  double W[9], W2[9];
  pg_hat(xi, W);
  pg_mm3(W, W, W2);
  double V[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double I = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = I + k.A * W[i] + k.B * W2[i];
    V[i] = I + k.B * W[i] + k.C * W2[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = V[i * 3 + 0] * xi[3] + V[i * 3 + 1] * xi[4] + V[i * 3 + 2] * xi[5];
}

/* right Jacobian inverse of SE(3) at xi: [[Ji, 0], [-Ji Q Ji, Ji]] (row-major 6x6) */
__device__ inline void pg_jr_inv(const double xi[6], double J[36]) {
  const double th = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
  const PgCoef k = pg_coef(th);
  double W[9], V[9], WW[9], WV[9], VW[9], WVW[9], WWV[9], VWW[9], WVWW[9], WWVW[9];
  pg_hat(xi, W);
  pg_hat(xi + 3, V);
  pg_mm3(W, W, WW);
  pg_mm3(W, V, WV);
  pg_mm3(V, W, VW);
  pg_mm3(WV, W, WVW);
  pg_mm3(W, WV, WWV);
  pg_mm3(VW, W, VWW);
  pg_mm3(WVW, W, WVWW);
  pg_mm3(W, WVW, WWVW);
  double Ji[9], Q[9], T[9], M[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    Ji[i] = ((i % 4 == 0) ? 1.0 : 0.0) + 0.5 * W[i] + k.D * WW[i];
    Q[i] = -0.5 * V[i] + k.C * (WV[i] + VW[i] - WVW[i]) - k.qb * (WWV[i] + VWW[i] - 3 * WVW[i]) +
           k.qc * (WVWW[i] + WWVW[i]);
  }
  pg_mm3(Ji, Q, T);
  pg_mm3(T, Ji, M);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      J[i * 6 + j] = Ji[i * 3 + j];
      J[i * 6 + 3 + j] = 0.0;
      J[(3 + i) * 6 + j] = -M[i * 3 + j];
      J[(3 + i) * 6 + 3 + j] = Ji[i * 3 + j];
    }
}

/* ---- 6x6 helpers (row-major) ---------------------------------------------------------------------------------- */

__device__ inline void pg_mv6(const double* A, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s += A[i * 6 + j] * x[j];
    y[i] = s;
  }
}

__device__ inline void pg_mtv6(const double* A, const double* x, double* y) { /* A^T x */
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s += A[j * 6 + i] * x[j];
    y[i] = s;
  }
}

__device__ inline void pg_mm6(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = 0;
#pragma unroll
      for (int l = 0; l < 6; ++l) s += A[i * 6 + l] * B[l * 6 + j];
      C[i * 6 + j] = s;
    }
}

__device__ inline void pg_mtm6(const double* A, const double* B, double* C) { /* A^T B */
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = 0;
#pragma unroll
      for (int l = 0; l < 6; ++l) s += A[l * 6 + i] * B[l * 6 + j];
      C[i * 6 + j] = s;
    }
}

/* Cholesky factor A = L L^T of a symmetric positive-definite 6x6 (only A's lower triangle is read).  F holds L's strict
 * lower triangle and 1 / L_ii on the diagonal (the solves multiply by it); its upper triangle is zero.  F may be A.
 * An explicit inverse in its place costs the cyclic reduction a factor cond(A) in accuracy: with blocks of condition
 * 1e9 the solve was wrong by 5e-7 where this one is at the system's own conditioning (test_gpu_posegraph_solve.py) */
__device__ inline void pg_chol6(const double* A, double* F) {
  double l[36];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= l[j * 6 + k] * l[j * 6 + k];
    const double r = 1.0 / sqrt(d);
    l[j * 6 + j] = r;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= l[i * 6 + k] * l[j * 6 + k];
      l[i * 6 + j] = s * r;
      l[j * 6 + i] = 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) F[i] = l[i];
}

/* x = A^-1 b with A's factor F of pg_chol6: L y = b, L^T x = y.  x may be b */
__device__ inline void pg_chol_solve6(const double* F, const double* b, double* x) {
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= F[i * 6 + k] * y[k];
    y[i] = s * F[i * 6 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= F[k * 6 + i] * y[k];
    y[i] = s * F[i * 6 + i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = y[i];
}

/* C = A^-1 B (6x6, row-major) with A's factor F, column by column */
__device__ inline void pg_chol_solve6m(const double* F, const double* B, double* C) {
  double f[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) f[i] = F[i];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = B[i * 6 + c];
    pg_chol_solve6(f, v, v);
#pragma unroll
    for (int i = 0; i < 6; ++i) C[i * 6 + c] = v[i];
  }
}

/* ---- kernels -------------------------------------------------------------------------------------------------- */

/* one lane per factor.  fr < 0: the prior on node `to` (Z is then the prior's mean).  lin == nullptr: energy only */
__global__ __launch_bounds__(PG_BLOCK) void k_pg_factor(uint32_t m, const int32_t* __restrict__ fr,
                                                        const int32_t* __restrict__ to, const double* __restrict__ Z,
                                                        const double* __restrict__ Om, const double* __restrict__ X,
                                                        double* __restrict__ lin, double* __restrict__ err6,
                                                        double* __restrict__ energy) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int a = fr[f], b = to[f];
  double Rj[9], tj[3], Rij[9], tij[3];
  pg_load(X + (size_t)b * 12, Rj, tj);
  if (a >= 0) {
    double Ri[9], ti[3];
    pg_load(X + (size_t)a * 12, Ri, ti);
    pg_between(Ri, ti, Rj, tj, Rij, tij);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) Rij[k] = Rj[k];
    tij[0] = tj[0], tij[1] = tj[1], tij[2] = tj[2];
  }
  double Rz[9], tz[3], RE[9], tE[3], e[6];
  pg_load(Z + (size_t)f * 12, Rz, tz);
  pg_between(Rz, tz, Rij, tij, RE, tE);
  pg_se3_log(RE, tE, e);
  const double* W = Om + (size_t)f * 36;
  double We[6];
  pg_mv6(W, e, We);
  double en = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) en += e[i] * We[i];
  energy[f] = 0.5 * en;
  if (err6)
#pragma unroll
    for (int i = 0; i < 6; ++i) err6[(size_t)f * 6 + i] = e[i];
  if (!lin) return;
  double* L = lin + (size_t)f * PG_LIN;
  double Jj[36], WJj[36], H[36], gv[6];
  pg_jr_inv(e, Jj);
  pg_mm6(W, Jj, WJj);
  pg_mtm6(Jj, WJj, H);
#pragma unroll
  for (int i = 0; i < 36; ++i) L[72 + i] = H[i];
  pg_mtv6(Jj, We, gv);
#pragma unroll
  for (int i = 0; i < 6; ++i) L[114 + i] = gv[i];
  if (a < 0) return;
  /* Ji = -Jj Ad(Tij^-1), Ad(T) = [[R, 0], [t^ R, R]] with T^-1 = (Rij^T, -Rij^T tij) */
  double Ri[9], ti[3], tR[9], Ad[36], Ji[36];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Ri[i * 3 + j] = Rij[j * 3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) ti[i] = -(Ri[i * 3 + 0] * tij[0] + Ri[i * 3 + 1] * tij[1] + Ri[i * 3 + 2] * tij[2]);
  double th[9];
  pg_hat(ti, th);
  pg_mm3(th, Ri, tR);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ad[i * 6 + j] = Ri[i * 3 + j];
      Ad[i * 6 + 3 + j] = 0.0;
      Ad[(3 + i) * 6 + j] = tR[i * 3 + j];
      Ad[(3 + i) * 6 + 3 + j] = Ri[i * 3 + j];
    }
  pg_mm6(Jj, Ad, Ji);
#pragma unroll
  for (int i = 0; i < 36; ++i) Ji[i] = -Ji[i];
  pg_mtm6(Ji, WJj, H);
#pragma unroll
  for (int i = 0; i < 36; ++i) L[36 + i] = H[i];
  pg_mm6(W, Ji, WJj);
  pg_mtm6(Ji, WJj, H);
#pragma unroll
  for (int i = 0; i < 36; ++i) L[i] = H[i];
  pg_mtv6(Ji, We, gv);
#pragma unroll
  for (int i = 0; i < 6; ++i) L[108 + i] = gv[i];
}

/* one lane per node: diagonal block and gradient, summed over the node's factors in factor order.
 * nfac entry = factor << 1 | side (0: the node is the factor's `from`, 1: its `to`) */
__global__ __launch_bounds__(PG_BLOCK) void k_pg_nodes(uint32_t n, const uint32_t* __restrict__ nptr,
                                                       const uint32_t* __restrict__ nfac,
                                                       const double* __restrict__ lin, double* __restrict__ D,
                                                       double* __restrict__ g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double H[36], v[6];
#pragma unroll
  for (int k = 0; k < 36; ++k) H[k] = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = 0;
  for (uint32_t q = nptr[i]; q < nptr[i + 1]; ++q) {
    const uint32_t w = nfac[q];
    const double* L = lin + (size_t)(w >> 1) * PG_LIN;
    const double* Hb = L + ((w & 1) ? 72 : 0);
    const double* gb = L + ((w & 1) ? 114 : 108);
#pragma unroll
    for (int k = 0; k < 36; ++k) H[k] += Hb[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += gb[k];
  }
#pragma unroll
  for (int k = 0; k < 36; ++k) D[(size_t)i * 36 + k] = H[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) g[(size_t)i * 6 + k] = v[k];
}

/* one lane per distinct pair (pa < pb): block (pa, pb) summed over its factors in insertion order.
 * pfac entry = factor << 1 | flip (flip: the factor runs pb -> pa, its Hij is block (pb, pa) and enters transposed).
 * pdst >= 0: index into the off-band list O; pdst < 0: band pair, written to U[pa] */
__global__ __launch_bounds__(PG_BLOCK) void k_pg_pairs(uint32_t np, const int32_t* __restrict__ pa,
                                                       const uint32_t* __restrict__ pptr,
                                                       const uint32_t* __restrict__ pfac,
                                                       const int32_t* __restrict__ pdst,
                                                       const double* __restrict__ lin, double* __restrict__ U,
                                                       double* __restrict__ O) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= np) return;
  double H[36];
#pragma unroll
  for (int q = 0; q < 36; ++q) H[q] = 0;
  for (uint32_t q = pptr[k]; q < pptr[k + 1]; ++q) {
    const uint32_t w = pfac[q];
    const double* Hb = lin + (size_t)(w >> 1) * PG_LIN + 36;
    if (w & 1) {
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) H[r * 6 + c] += Hb[c * 6 + r];
    } else {
#pragma unroll
      for (int r = 0; r < 36; ++r) H[r] += Hb[r];
    }
  }
  double* out = pdst[k] >= 0 ? O + (size_t)pdst[k] * 36 : U + (size_t)pa[k] * 36;
#pragma unroll
  for (int q = 0; q < 36; ++q) out[q] = H[q];
}

struct PgStatus {
  double energy;     /* k_pg_energy */
  double lin_change; /* k_pg_solve: -(g.d + d.H d / 2) */
  double rz0, rz;    /* preconditioned residual norms^2, first and last */
  uint32_t cg_iterations;
  uint32_t pad[3];
};

/* the sum of a block's per-thread values, the same tree every time; every thread gets the result */
__device__ inline double pg_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = PG_SOLVE_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(PG_SOLVE_THREADS) void k_pg_energy(uint32_t m, const double* __restrict__ energy,
                                                                PgStatus* st) {
  __shared__ double red[PG_SOLVE_THREADS];
  double s = 0;
  for (uint32_t f = threadIdx.x; f < m; f += PG_SOLVE_THREADS) s += energy[f];
  s = pg_block_sum(s, red);
  if (threadIdx.x == 0) st->energy = s;
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_retract(uint32_t n, const double* __restrict__ X,
                                                         const double* __restrict__ delta, double* __restrict__ Xn) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double R[9], t[3], dR[9], dt[3], Rn[9];
  pg_load(X + (size_t)i * 12, R, t);
  pg_se3_exp(delta + (size_t)i * 6, dR, dt);
  pg_mm3(R, dR, Rn);
  double* o = Xn + (size_t)i * 12;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = Rn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) o[9 + k] = R[k * 3 + 0] * dt[0] + R[k * 3 + 1] * dt[1] + R[k * 3 + 2] * dt[2] + t[k];
}

struct PgSystem {
  uint32_t n;
  const double *D, *U, *O, *g;
  const int32_t *oa, *ob;         /* off-band pair k = (oa[k], ob[k]), oa < ob */
  const uint32_t *optr, *oadj;    /* per node: off-band pairs it is in, k << 1 | (node is ob) */
  double *Bf, *Cr, *Lb;           /* block cyclic reduction: per node, at its elimination level */
  double *x, *r, *z, *p, *q;      /* 6n each */
};

/* q = (H + lambda I) v */
__device__ void pg_spmv(const PgSystem& S, double lambda, const double* v, double* q) {
  for (uint32_t i = threadIdx.x; i < S.n; i += PG_SOLVE_THREADS) {
    double y[6], t[6];
    pg_mv6(S.D + (size_t)i * 36, v + (size_t)i * 6, y);
#pragma unroll
    for (int k = 0; k < 6; ++k) y[k] += lambda * v[(size_t)i * 6 + k];
    if (i + 1 < S.n) {
      pg_mv6(S.U + (size_t)i * 36, v + (size_t)(i + 1) * 6, t);
#pragma unroll
      for (int k = 0; k < 6; ++k) y[k] += t[k];
    }
    if (i > 0) {
      pg_mtv6(S.U + (size_t)(i - 1) * 36, v + (size_t)(i - 1) * 6, t);
#pragma unroll
      for (int k = 0; k < 6; ++k) y[k] += t[k];
    }
    for (uint32_t a = S.optr[i]; a < S.optr[i + 1]; ++a) {
      const uint32_t w = S.oadj[a], k = w >> 1;
      if (w & 1)
        pg_mtv6(S.O + (size_t)k * 36, v + (size_t)S.oa[k] * 6, t);
      else
        pg_mv6(S.O + (size_t)k * 36, v + (size_t)S.ob[k] * 6, t);
#pragma unroll
      for (int c = 0; c < 6; ++c) y[c] += t[c];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) q[(size_t)i * 6 + k] = y[k];
  }
  __syncthreads();
}

/* Block cyclic reduction of the block-tridiagonal part T (diagonal D + lambda I, band U).  At stride s the nodes
 * e = s-1 + 2sk are eliminated (lowest set bit of e+1 is s); their neighbours e -+ s survive to stride 2s.  Per node:
 * Bf = Cholesky factor of its reduced diagonal block (pg_chol6; the reduced block itself until the node is eliminated),
 * Cr = its coupling to the right neighbour at its level (Rb), Lb = its coupling to the left neighbour at its level. */
__device__ void pg_bcr_factor(const PgSystem& S, double lambda) {
  const uint32_t n = S.n;
  for (uint32_t i = threadIdx.x; i < n; i += PG_SOLVE_THREADS)
    for (int k = 0; k < 36; ++k) {
      S.Bf[(size_t)i * 36 + k] = S.D[(size_t)i * 36 + k] + (k % 7 == 0 ? lambda : 0.0);
      S.Cr[(size_t)i * 36 + k] = i + 1 < n ? S.U[(size_t)i * 36 + k] : 0.0;
    }
  __syncthreads();
  for (uint32_t s = 1; s <= n; s <<= 1) {
    for (size_t e = s - 1 + (size_t)2 * s * threadIdx.x; e < n; e += (size_t)2 * s * PG_SOLVE_THREADS) {
      pg_chol6(S.Bf + (size_t)e * 36, S.Bf + (size_t)e * 36);
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c)
          S.Lb[(size_t)e * 36 + r * 6 + c] = e >= s ? S.Cr[(size_t)(e - s) * 36 + c * 6 + r] : 0.0;
    }
    __syncthreads();
    for (size_t k = (size_t)2 * s - 1 + (size_t)2 * s * threadIdx.x; k < n; k += (size_t)2 * s * PG_SOLVE_THREADS) {
      double T1[36], T2[36];
      double* Bk = S.Bf + (size_t)k * 36;
      const double* Rl = S.Cr + (size_t)(k - s) * 36; /* block (k-s, k) */
      pg_chol_solve6m(S.Bf + (size_t)(k - s) * 36, Rl, T1);
      pg_mtm6(Rl, T1, T2);
      for (int q = 0; q < 36; ++q) Bk[q] -= T2[q];
      if (k + s < n) {
        const double* Lr = S.Lb + (size_t)(k + s) * 36; /* block (k+s, k) */
        const double* Bi = S.Bf + (size_t)(k + s) * 36;
        pg_chol_solve6m(Bi, Lr, T1);
        pg_mtm6(Lr, T1, T2);
        for (int q = 0; q < 36; ++q) Bk[q] -= T2[q];
        if (k + 2 * s < n) {
          pg_chol_solve6m(Bi, S.Cr + (size_t)(k + s) * 36, T1);
          pg_mtm6(Lr, T1, T2);
          for (int q = 0; q < 36; ++q) S.Cr[(size_t)k * 36 + q] = -T2[q];
        } else {
          for (int q = 0; q < 36; ++q) S.Cr[(size_t)k * 36 + q] = 0.0;
        }
      } else {
        for (int q = 0; q < 36; ++q) S.Cr[(size_t)k * 36 + q] = 0.0;
      }
    }
    __syncthreads();
  }
}

/* z = T^-1 r with the factorisation of pg_bcr_factor */
__device__ void pg_bcr_apply(const PgSystem& S, const double* r, double* z) {
  const uint32_t n = S.n;
  for (uint32_t i = threadIdx.x; i < 6 * n; i += PG_SOLVE_THREADS) z[i] = r[i];
  __syncthreads();
  uint32_t top = 1;
  for (uint32_t s = 1; s <= n; s <<= 1) {
    top = s;
    for (size_t k = (size_t)2 * s - 1 + (size_t)2 * s * threadIdx.x; k < n; k += (size_t)2 * s * PG_SOLVE_THREADS) {
      double y[6], t[6];
      pg_chol_solve6(S.Bf + (size_t)(k - s) * 36, z + (size_t)(k - s) * 6, y);
      pg_mtv6(S.Cr + (size_t)(k - s) * 36, y, t);
      for (int c = 0; c < 6; ++c) z[(size_t)k * 6 + c] -= t[c];
      if (k + s < n) {
        pg_chol_solve6(S.Bf + (size_t)(k + s) * 36, z + (size_t)(k + s) * 6, y);
        pg_mtv6(S.Lb + (size_t)(k + s) * 36, y, t);
        for (int c = 0; c < 6; ++c) z[(size_t)k * 6 + c] -= t[c];
      }
    }
    __syncthreads();
  }
  for (uint32_t s = top; s >= 1; s >>= 1) {
    for (size_t e = s - 1 + (size_t)2 * s * threadIdx.x; e < n; e += (size_t)2 * s * PG_SOLVE_THREADS) {
      double y[6], t[6];
      for (int c = 0; c < 6; ++c) y[c] = z[(size_t)e * 6 + c];
      if (e >= s) {
        pg_mv6(S.Lb + (size_t)e * 36, z + (size_t)(e - s) * 6, t);
        for (int c = 0; c < 6; ++c) y[c] -= t[c];
      }
      if (e + s < n) {
        pg_mv6(S.Cr + (size_t)e * 36, z + (size_t)(e + s) * 6, t);
        for (int c = 0; c < 6; ++c) y[c] -= t[c];
      }
      pg_chol_solve6(S.Bf + (size_t)e * 36, y, t);
      for (int c = 0; c < 6; ++c) z[(size_t)e * 6 + c] = t[c];
    }
    __syncthreads();
  }
}

__device__ double pg_dot(const double* a, const double* b, uint32_t len, double* red) {
  double s = 0;
  for (uint32_t i = threadIdx.x; i < len; i += PG_SOLVE_THREADS) s += a[i] * b[i];
  return pg_block_sum(s, red);
}

/* preconditioned CG on (H + lambda I) x = -g, in one workgroup (no grid-wide barrier, no host round trip); stops when
 * sqrt(r'z / r0'z0) <= tol or after max_it iterations.  Writes x and the linearised cost change of x. */
__global__ __launch_bounds__(PG_SOLVE_THREADS) void k_pg_solve(PgSystem S, double lambda, double tol, uint32_t max_it,
                                                               PgStatus* st) {
  __shared__ double red[PG_SOLVE_THREADS];
  const uint32_t N = 6 * S.n;
  pg_bcr_factor(S, lambda);
  for (uint32_t i = threadIdx.x; i < N; i += PG_SOLVE_THREADS) S.x[i] = 0.0, S.r[i] = -S.g[i];
  __syncthreads();
  pg_bcr_apply(S, S.r, S.z);
  for (uint32_t i = threadIdx.x; i < N; i += PG_SOLVE_THREADS) S.p[i] = S.z[i];
  double rz = pg_dot(S.r, S.z, N, red);
  const double rz0 = rz;
  uint32_t it = 0;
  if (rz0 > 0) {
    while (it < max_it) {
      pg_spmv(S, lambda, S.p, S.q);
      const double pq = pg_dot(S.p, S.q, N, red);
      if (!(pq > 0)) break;
      const double alpha = rz / pq;
      for (uint32_t i = threadIdx.x; i < N; i += PG_SOLVE_THREADS) S.x[i] += alpha * S.p[i], S.r[i] -= alpha * S.q[i];
      __syncthreads();
      ++it;
      pg_bcr_apply(S, S.r, S.z);
      const double rzn = pg_dot(S.r, S.z, N, red);
      if (!(rzn > tol * tol * rz0)) {
        rz = rzn;
        break;
      }
      const double beta = rzn / rz;
      for (uint32_t i = threadIdx.x; i < N; i += PG_SOLVE_THREADS) S.p[i] = S.z[i] + beta * S.p[i];
      __syncthreads();
      rz = rzn;
    }
  }
  /* linearised cost change of x on the undamped system: -(g'x + x'(H x) / 2), H x = (H + lambda I) x - lambda x */
  pg_spmv(S, lambda, S.x, S.q);
  double s = 0;
  for (uint32_t i = threadIdx.x; i < N; i += PG_SOLVE_THREADS)
    s += S.g[i] * S.x[i] + 0.5 * S.x[i] * (S.q[i] - lambda * S.x[i]);
  s = pg_block_sum(s, red);
  if (threadIdx.x == 0) {
    st->lin_change = -s;
    st->rz0 = rz0;
    st->rz = rz;
    st->cg_iterations = it;
  }
}

/* ---- host side ------------------------------------------------------------------------------------------------ */

struct suma_posegraph {
  int device = 0;
  hipStream_t stream = nullptr;
  mutable std::string err; /* also set by the const entries that fail */
  uint32_t node_cap = 0, edge_cap = 0;
  /* host record of the graph (Posegraph::initial_ / result_ / edges_): poses as rigid R | t, 12 doubles */
  std::vector<double> initial, result;
  std::vector<int32_t> efrom, eto;
  std::vector<double> eZ, eOm; /* 12 / 36 (row-major, symmetrised) per edge */
  bool structure_dirty = true;
  /* device: factors (prior + edges), structure, system, solver */
  uint32_t n_dev = 0, m_dev = 0, np_dev = 0, no_dev = 0;
  DevBuf<double> X, Xn, Z, Om, lin, energy, err6, D, U, O, g, Bf, Cr, Lb, work;
  DevBuf<int32_t> fr, to, pa, pdst, oa, ob;
  DevBuf<uint32_t> nptr, nfac, pptr, pfac, optr, oadj;
  DevBuf<PgStatus> dst;
  PinnedBuf<PgStatus> hst;
};

namespace {

thread_local std::string g_pg_create_error; /* per thread: concurrent failed creates do not race */

int pg_fail(const suma_posegraph* g, int code, const std::string& msg) {
  if (g) g->err = msg;
  return code;
}

#define PG_HIP(g, expr)                                                              \
  do {                                                                               \
    hipError_t e__ = (expr);                                                         \
    if (e__ != hipSuccess) return pg_fail(g, SUMA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
  } while (0)

/* A first allocation is exact (a clone is prepared once, at its final size); a block that has to grow doubles, so a
 * graph that gains a node and an edge between two preparations -- the scan pipeline's -- allocates and frees nothing in
 * all but O(log n) of them.  hipFree waits for the whole device, the optimiser's stream included. */
template <class T>
hipError_t pg_grow(DevBuf<T>& b, size_t n) {
  n = std::max<size_t>(n, 1);
  return n <= b.cap ? hipSuccess : b.alloc(std::max(n, 2 * b.cap));
}

bool finite_n(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

/* column-major 4x4 -> R (row-major) | t */
void to_rigid(const double T[16], double* o) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[i * 3 + j] = T[j * 4 + i];
  o[9] = T[12], o[10] = T[13], o[11] = T[14];
}

void from_rigid(const double* o, double T[16]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[j * 4 + i] = o[i * 3 + j];
    T[12 + i] = o[9 + i];
    T[i * 4 + 3] = 0.0;
  }
  T[15] = 1.0;
}

uint32_t grid(uint32_t n) { return (n + PG_BLOCK - 1) / PG_BLOCK; }

/* uploads the factors and builds the adjacency (CSR) of the current structure; uploads the current result as X */
int pg_prepare(suma_posegraph* G) {
  const uint32_t n = (uint32_t)(G->result.size() / 12), ne = (uint32_t)G->efrom.size(), m = ne + 1;
  PG_HIP(G, hipSetDevice(G->device));
  if (G->structure_dirty || n != G->n_dev) {
    std::vector<int32_t> fr(m), to(m);
    std::vector<double> Z(12 * (size_t)m, 0.0), Om(36 * (size_t)m, 0.0);
    fr[0] = -1, to[0] = 0; /* Posegraph.cpp:39-45: PriorFactor(first id, Pose3(), variances 1e-6) */
    Z[0] = Z[4] = Z[8] = 1.0;
    for (int k = 0; k < 6; ++k) Om[k * 7] = 1e6;
    for (uint32_t e = 0; e < ne; ++e) {
      fr[e + 1] = G->efrom[e], to[e + 1] = G->eto[e];
      std::copy(G->eZ.begin() + 12 * e, G->eZ.begin() + 12 * (e + 1), Z.begin() + 12 * (e + 1));
      std::copy(G->eOm.begin() + 36 * e, G->eOm.begin() + 36 * (e + 1), Om.begin() + 36 * (e + 1));
    }
    /* node -> factors, in factor order */
    std::vector<uint32_t> nptr(n + 1, 0), nfac;
    for (uint32_t f = 0; f < m; ++f) {
      if (fr[f] >= 0) ++nptr[fr[f] + 1];
      ++nptr[to[f] + 1];
    }
    for (uint32_t i = 0; i < n; ++i) nptr[i + 1] += nptr[i];
    nfac.resize(std::max<uint32_t>(nptr[n], 1));
    {
      std::vector<uint32_t> fill(nptr.begin(), nptr.end() - 1);
      for (uint32_t f = 0; f < m; ++f) {
        if (fr[f] >= 0) nfac[fill[fr[f]]++] = f << 1;
        nfac[fill[to[f]]++] = f << 1 | 1u;
      }
    }
    /* distinct pairs (a < b) in order of first appearance, each with its factors in insertion order */
    std::map<std::pair<int32_t, int32_t>, uint32_t> pid;
    std::vector<std::vector<uint32_t>> plist;
    std::vector<int32_t> pa, pb;
    for (uint32_t f = 1; f < m; ++f) {
      const int32_t a = std::min(fr[f], to[f]), b = std::max(fr[f], to[f]);
      auto it = pid.find({a, b});
      uint32_t k;
      if (it == pid.end()) {
        k = (uint32_t)plist.size();
        pid[{a, b}] = k;
        plist.emplace_back();
        pa.push_back(a), pb.push_back(b);
      } else {
        k = it->second;
      }
      plist[k].push_back(f << 1 | (fr[f] == b ? 1u : 0u));
    }
    const uint32_t np = (uint32_t)plist.size();
    std::vector<uint32_t> pptr(np + 1, 0), pfac;
    std::vector<int32_t> pdst(np), oa, ob;
    for (uint32_t k = 0; k < np; ++k) {
      pptr[k + 1] = pptr[k] + (uint32_t)plist[k].size();
      pfac.insert(pfac.end(), plist[k].begin(), plist[k].end());
      if (pb[k] == pa[k] + 1) {
        pdst[k] = -1;
      } else {
        pdst[k] = (int32_t)oa.size();
        oa.push_back(pa[k]), ob.push_back(pb[k]);
      }
    }
    const uint32_t no = (uint32_t)oa.size();
    std::vector<uint32_t> optr(n + 1, 0), oadj(std::max<uint32_t>(2 * no, 1));
    for (uint32_t k = 0; k < no; ++k) ++optr[oa[k] + 1], ++optr[ob[k] + 1];
    for (uint32_t i = 0; i < n; ++i) optr[i + 1] += optr[i];
    {
      std::vector<uint32_t> fill(optr.begin(), optr.end() - 1);
      for (uint32_t k = 0; k < no; ++k) oadj[fill[oa[k]]++] = k << 1, oadj[fill[ob[k]]++] = k << 1 | 1u;
    }
    if (pfac.empty()) pfac.push_back(0);
    PG_HIP(G, hipStreamSynchronize(G->stream)); /* grown blocks may still be read by earlier work */
    PG_HIP(G, pg_grow(G->fr, m));
    PG_HIP(G, pg_grow(G->to, m));
    PG_HIP(G, pg_grow(G->Z, 12 * (size_t)m));
    PG_HIP(G, pg_grow(G->Om, 36 * (size_t)m));
    PG_HIP(G, pg_grow(G->lin, (size_t)PG_LIN * m));
    PG_HIP(G, pg_grow(G->energy, m));
    PG_HIP(G, pg_grow(G->err6, 6 * (size_t)m));
    PG_HIP(G, pg_grow(G->nptr, n + 1));
    PG_HIP(G, pg_grow(G->nfac, nfac.size()));
    PG_HIP(G, pg_grow(G->pa, np));
    PG_HIP(G, pg_grow(G->pdst, np));
    PG_HIP(G, pg_grow(G->pptr, np + 1));
    PG_HIP(G, pg_grow(G->pfac, pfac.size()));
    PG_HIP(G, pg_grow(G->oa, no));
    PG_HIP(G, pg_grow(G->ob, no));
    PG_HIP(G, pg_grow(G->optr, n + 1));
    PG_HIP(G, pg_grow(G->oadj, oadj.size()));
    PG_HIP(G, pg_grow(G->O, 36 * (size_t)no));
    for (DevBuf<double>* b : {&G->D, &G->U, &G->Bf, &G->Cr, &G->Lb}) PG_HIP(G, pg_grow(*b, 36 * (size_t)n));
    PG_HIP(G, pg_grow(G->g, 6 * (size_t)n));
    PG_HIP(G, pg_grow(G->work, 30 * (size_t)n)); /* x r z p q */
    PG_HIP(G, pg_grow(G->X, 12 * (size_t)n));
    PG_HIP(G, pg_grow(G->Xn, 12 * (size_t)n));
    auto up = [&](void* d, const void* h, size_t bytes) {
      return bytes ? hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, G->stream) : hipSuccess;
    };
    PG_HIP(G, up(G->fr, fr.data(), 4 * fr.size()));
    PG_HIP(G, up(G->to, to.data(), 4 * to.size()));
    PG_HIP(G, up(G->Z, Z.data(), 8 * Z.size()));
    PG_HIP(G, up(G->Om, Om.data(), 8 * Om.size()));
    PG_HIP(G, up(G->nptr, nptr.data(), 4 * nptr.size()));
    PG_HIP(G, up(G->nfac, nfac.data(), 4 * nfac.size()));
    PG_HIP(G, up(G->pa, pa.data(), 4 * pa.size()));
    PG_HIP(G, up(G->pdst, pdst.data(), 4 * pdst.size()));
    PG_HIP(G, up(G->pptr, pptr.data(), 4 * pptr.size()));
    PG_HIP(G, up(G->pfac, pfac.data(), 4 * pfac.size()));
    PG_HIP(G, up(G->oa, oa.data(), 4 * oa.size()));
    PG_HIP(G, up(G->ob, ob.data(), 4 * ob.size()));
    PG_HIP(G, up(G->optr, optr.data(), 4 * optr.size()));
    PG_HIP(G, up(G->oadj, oadj.data(), 4 * oadj.size()));
    /* band blocks without a factor stay zero */
    PG_HIP(G, hipMemsetAsync(G->U, 0, 36 * sizeof(double) * n, G->stream));
    G->n_dev = n, G->m_dev = m, G->np_dev = np, G->no_dev = no;
    G->structure_dirty = false;
  }
  PG_HIP(G, hipMemcpyAsync(G->X, G->result.data(), 8 * G->result.size(), hipMemcpyHostToDevice, G->stream));
  return SUMA_OK;
}

/* energy of the poses in `Xd` -> *e (one status read) */
int pg_eval(suma_posegraph* G, const double* Xd, double* e) {
  hipLaunchKernelGGL(k_pg_factor, dim3(grid(G->m_dev)), dim3(PG_BLOCK), 0, G->stream, G->m_dev, G->fr.p, G->to.p,
                     G->Z.p, G->Om.p, Xd, (double*)nullptr, (double*)nullptr, G->energy.p);
  hipLaunchKernelGGL(k_pg_energy, dim3(1), dim3(PG_SOLVE_THREADS), 0, G->stream, G->m_dev, G->energy.p, G->dst.p);
  PG_HIP(G, hipGetLastError());
  PG_HIP(G, hipMemcpyAsync(G->hst.p, G->dst.p, sizeof(PgStatus), hipMemcpyDeviceToHost, G->stream));
  PG_HIP(G, hipStreamSynchronize(G->stream));
  *e = G->hst->energy;
  return SUMA_OK;
}

/* the system at the poses in X */
int pg_linearize(suma_posegraph* G) {
  const uint32_t n = G->n_dev, m = G->m_dev;
  hipLaunchKernelGGL(k_pg_factor, dim3(grid(m)), dim3(PG_BLOCK), 0, G->stream, m, G->fr.p, G->to.p, G->Z.p, G->Om.p,
                     G->X.p, G->lin.p, G->err6.p, G->energy.p);
  hipLaunchKernelGGL(k_pg_nodes, dim3(grid(n)), dim3(PG_BLOCK), 0, G->stream, n, G->nptr.p, G->nfac.p, G->lin.p,
                     G->D.p, G->g.p);
  if (G->np_dev)
    hipLaunchKernelGGL(k_pg_pairs, dim3(grid(G->np_dev)), dim3(PG_BLOCK), 0, G->stream, G->np_dev, G->pa.p,
                       G->pptr.p, G->pfac.p, G->pdst.p, G->lin.p, G->U.p, G->O.p);
  PG_HIP(G, hipGetLastError());
  return SUMA_OK;
}

PgSystem pg_system(suma_posegraph* G) {
  const size_t n6 = 6 * (size_t)G->n_dev;
  PgSystem S;
  S.n = G->n_dev;
  S.D = G->D, S.U = G->U, S.O = G->O, S.g = G->g;
  S.oa = G->oa, S.ob = G->ob, S.optr = G->optr, S.oadj = G->oadj;
  S.Bf = G->Bf, S.Cr = G->Cr, S.Lb = G->Lb;
  S.x = G->work, S.r = G->work + n6, S.z = G->work + 2 * n6, S.p = G->work + 3 * n6, S.q = G->work + 4 * n6;
  return S;
}

int pg_check_params(const suma_posegraph_params* p) {
  const double v[] = {p->lambda_initial, p->lambda_factor, p->lambda_upper_bound, p->lambda_lower_bound,
                      p->min_model_fidelity, p->relative_error_tol, p->absolute_error_tol, p->error_tol,
                      p->cg_tolerance};
  if (!finite_n(v, 9)) return 0;
  return p->lambda_initial > 0 && p->lambda_factor > 1 && p->lambda_lower_bound >= 0 && p->cg_tolerance >= 0 &&
         p->cg_max_iterations > 0;
}

}  // namespace

extern "C" {

void suma_posegraph_default_params(suma_posegraph_params* p) {
  if (!p) return;
  *p = suma_posegraph_params{};
  p->lambda_initial = 1e-5;
  p->lambda_factor = 10.0;
  p->lambda_upper_bound = 1e5;
  p->lambda_lower_bound = 0.0;
  p->min_model_fidelity = 1e-3;
  p->relative_error_tol = 1e-5;
  p->absolute_error_tol = 1e-5;
  p->error_tol = 0.0;
  p->cg_tolerance = 1e-10;
  p->cg_max_iterations = 1000;
}

const char* suma_posegraph_last_error(const suma_posegraph* g) {
  return g ? g->err.c_str() : g_pg_create_error.c_str();
}

int suma_posegraph_create(int hip_device, uint32_t node_capacity, uint32_t edge_capacity, suma_posegraph** out) {
  if (!out || node_capacity == 0 || node_capacity > (1u << 30) || edge_capacity > (1u << 29)) {
    g_pg_create_error = "suma_posegraph_create: bad argument";
    return SUMA_ERR_INVALID;
  }
  *out = nullptr;
  suma_posegraph* G = new (std::nothrow) suma_posegraph();
  if (!G) {
    g_pg_create_error = "out of host memory";
    return SUMA_ERR_NOMEM;
  }
  G->device = hip_device, G->node_cap = node_capacity, G->edge_cap = edge_capacity;
  hipError_t e = hipSetDevice(hip_device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&G->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = G->dst.alloc(1);
  if (e == hipSuccess) e = G->hst.alloc(1);
  if (e != hipSuccess) {
    g_pg_create_error = std::string("suma_posegraph_create: ") + hipGetErrorString(e);
    if (G->stream) (void)hipStreamDestroy(G->stream);
    delete G;
    return SUMA_ERR_HIP;
  }
  *out = G;
  return SUMA_OK;
}

void suma_posegraph_destroy(suma_posegraph* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  hipStream_t st = g->stream;
  delete g; /* the device blocks go before their stream */
  if (st) (void)hipStreamDestroy(st);
}

int suma_posegraph_clear(suma_posegraph* g) {
  if (!g) return SUMA_ERR_INVALID;
  g->initial.clear(), g->result.clear(), g->efrom.clear(), g->eto.clear(), g->eZ.clear(), g->eOm.clear();
  g->structure_dirty = true;
  return SUMA_OK;
}

int suma_posegraph_clone(const suma_posegraph* g, suma_posegraph** out) {
  if (!g || !out) return SUMA_ERR_INVALID;
  int rc = suma_posegraph_create(g->device, g->node_cap, g->edge_cap, out);
  if (rc != SUMA_OK) return rc;
  suma_posegraph* c = *out;
  c->initial = g->initial, c->result = g->result, c->efrom = g->efrom, c->eto = g->eto, c->eZ = g->eZ, c->eOm = g->eOm;
  return SUMA_OK;
}

int suma_posegraph_set_initial(suma_posegraph* g, int32_t id, const double T[16]) {
  if (!g) return SUMA_ERR_INVALID;
  const uint32_t n = (uint32_t)(g->result.size() / 12);
  if (!T || id < 0 || (uint32_t)id > n) return pg_fail(g, SUMA_ERR_INVALID, "set_initial: id must be < size (update) or == size (append)");
  if (!finite_n(T, 16)) return pg_fail(g, SUMA_ERR_INVALID, "set_initial: non-finite pose");
  double r[12];
  to_rigid(T, r);
  if ((uint32_t)id == n) {
    if (n >= g->node_cap) return pg_fail(g, SUMA_ERR_CAPACITY, "set_initial: node capacity exceeded");
    g->initial.insert(g->initial.end(), r, r + 12);
    g->result.insert(g->result.end(), r, r + 12);
    g->structure_dirty = true;
  } else {
    std::copy(r, r + 12, g->initial.begin() + 12 * (size_t)id);
    std::copy(r, r + 12, g->result.begin() + 12 * (size_t)id);
  }
  return SUMA_OK;
}

int suma_posegraph_add_edge(suma_posegraph* g, int32_t from, int32_t to, const double Z[16], const double info[36]) {
  if (!g) return SUMA_ERR_INVALID;
  const int32_t n = (int32_t)(g->result.size() / 12);
  if (!Z || !info || from < 0 || to < 0 || from >= n || to >= n || from == to)
    return pg_fail(g, SUMA_ERR_INVALID, "add_edge: from and to must be distinct ids < size");
  if (!finite_n(Z, 16) || !finite_n(info, 36)) return pg_fail(g, SUMA_ERR_INVALID, "add_edge: non-finite input");
  if (g->efrom.size() >= g->edge_cap) return pg_fail(g, SUMA_ERR_CAPACITY, "add_edge: edge capacity exceeded");
  double r[12], W[36];
  to_rigid(Z, r);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) W[i * 6 + j] = 0.5 * (info[j * 6 + i] + info[i * 6 + j]);
  g->efrom.push_back(from), g->eto.push_back(to);
  g->eZ.insert(g->eZ.end(), r, r + 12);
  g->eOm.insert(g->eOm.end(), W, W + 36);
  g->structure_dirty = true;
  return SUMA_OK;
}

int32_t suma_posegraph_size(const suma_posegraph* g) { return g ? (int32_t)(g->result.size() / 12) : 0; }

uint32_t suma_posegraph_edge_count(const suma_posegraph* g) { return g ? (uint32_t)g->efrom.size() : 0; }

int suma_posegraph_pose(const suma_posegraph* g, int32_t id, double T[16]) {
  if (!g) return SUMA_ERR_INVALID;
  if (!T || id < 0 || (size_t)id >= g->result.size() / 12) return pg_fail(g, SUMA_ERR_INVALID, "pose: id must be < size");
  from_rigid(g->result.data() + 12 * (size_t)id, T);
  return SUMA_OK;
}

int suma_posegraph_poses(const suma_posegraph* g, double* out, uint32_t capacity, uint32_t* n) {
  if (!g) return SUMA_ERR_INVALID;
  const uint32_t sz = (uint32_t)(g->result.size() / 12);
  if (n) *n = sz;
  if (sz > capacity) return pg_fail(g, SUMA_ERR_CAPACITY, "poses: capacity < size");
  if (sz && !out) return pg_fail(g, SUMA_ERR_INVALID, "poses: no output buffer");
  for (uint32_t i = 0; i < sz; ++i) from_rigid(g->result.data() + 12 * (size_t)i, out + 16 * (size_t)i);
  return SUMA_OK;
}

int suma_posegraph_reserve(suma_posegraph* g, uint32_t node_capacity, uint32_t edge_capacity) {
  if (!g) return SUMA_ERR_INVALID;
  if (node_capacity > (1u << 30) || edge_capacity > (1u << 29)) return pg_fail(g, SUMA_ERR_INVALID, "reserve: bad argument");
  g->node_cap = std::max(g->node_cap, node_capacity);
  g->edge_cap = std::max(g->edge_cap, edge_capacity);
  return SUMA_OK;
}

int suma_posegraph_edge(const suma_posegraph* g, uint32_t index, int32_t* from, int32_t* to, double Z[16],
                        double information[36]) {
  if (!g) return SUMA_ERR_INVALID;
  if (index >= g->efrom.size()) return pg_fail(g, SUMA_ERR_INVALID, "edge: index must be < edge count");
  if (from) *from = g->efrom[index];
  if (to) *to = g->eto[index];
  if (Z) from_rigid(g->eZ.data() + 12 * (size_t)index, Z);
  if (information) std::copy(g->eOm.begin() + 36 * (size_t)index, g->eOm.begin() + 36 * (size_t)(index + 1), information);
  return SUMA_OK;
}

int suma_posegraph_reinitialize(suma_posegraph* g) {
  if (!g) return SUMA_ERR_INVALID;
  g->result = g->initial;
  return SUMA_OK;
}

int suma_posegraph_error(suma_posegraph* g, double* error) {
  if (!g || !error) return SUMA_ERR_INVALID;
  *error = 0.0;
  if (g->result.empty()) return SUMA_OK;
  int rc = pg_prepare(g);
  if (rc != SUMA_OK) return rc;
  return pg_eval(g, g->X, error);
}

int suma_posegraph_linearize(suma_posegraph* g, double* factor_errors, double* gradient, double* diag_blocks,
                             double* band_blocks, double* off_blocks, int32_t* off_pairs, uint32_t off_capacity,
                             uint32_t* n_off) {
  if (!g) return SUMA_ERR_INVALID;
  const uint32_t n = (uint32_t)(g->result.size() / 12);
  if (n == 0) return pg_fail(g, SUMA_ERR_INVALID, "linearize: empty graph");
  int rc = pg_prepare(g);
  if (rc != SUMA_OK) return rc;
  rc = pg_linearize(g);
  if (rc != SUMA_OK) return rc;
  if (n_off) *n_off = g->no_dev;
  if (off_blocks && g->no_dev > off_capacity) return pg_fail(g, SUMA_ERR_CAPACITY, "linearize: off_capacity");
  std::vector<double> D(36 * (size_t)n), U(36 * (size_t)n), O(36 * (size_t)g->no_dev), gr(6 * (size_t)n),
      e6(6 * (size_t)g->m_dev);
  std::vector<int32_t> oa(g->no_dev), ob(g->no_dev);
  auto down = [&](void* h, const void* d, size_t bytes) {
    return bytes ? hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, g->stream) : hipSuccess;
  };
  PG_HIP(g, down(D.data(), g->D, 8 * D.size()));
  PG_HIP(g, down(U.data(), g->U, 8 * U.size()));
  PG_HIP(g, down(O.data(), g->O, 8 * O.size()));
  PG_HIP(g, down(gr.data(), g->g, 8 * gr.size()));
  PG_HIP(g, down(e6.data(), g->err6, 8 * e6.size()));
  PG_HIP(g, down(oa.data(), g->oa, 4 * oa.size()));
  PG_HIP(g, down(ob.data(), g->ob, 4 * ob.size()));
  PG_HIP(g, hipStreamSynchronize(g->stream));
  auto cm = [](const double* rm, double* out) { /* row-major 6x6 -> column-major */
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) out[j * 6 + i] = rm[i * 6 + j];
  };
  if (factor_errors) std::copy(e6.begin(), e6.end(), factor_errors);
  if (gradient) std::copy(gr.begin(), gr.end(), gradient);
  for (uint32_t i = 0; i < n; ++i) {
    if (diag_blocks) cm(D.data() + 36 * (size_t)i, diag_blocks + 36 * (size_t)i);
    if (band_blocks && i + 1 < n) cm(U.data() + 36 * (size_t)i, band_blocks + 36 * (size_t)i);
  }
  for (uint32_t k = 0; k < g->no_dev; ++k) {
    if (off_blocks) cm(O.data() + 36 * (size_t)k, off_blocks + 36 * (size_t)k);
    if (off_pairs && off_blocks) off_pairs[2 * k] = oa[k], off_pairs[2 * k + 1] = ob[k];
  }
  return SUMA_OK;
}

int suma_posegraph_optimize(suma_posegraph* g, uint32_t max_iterations, const suma_posegraph_params* params,
                            suma_posegraph_stats* stats) {
  if (!g) return SUMA_ERR_INVALID;
  suma_posegraph_params p;
  suma_posegraph_default_params(&p);
  if (params) p = *params;
  if (!pg_check_params(&p)) return pg_fail(g, SUMA_ERR_INVALID, "optimize: bad parameters");
  suma_posegraph_stats st{};
  st.termination = SUMA_PG_MAX_ITERATIONS;
  st.lambda = p.lambda_initial;
  if (stats) *stats = st;
  if (g->result.empty()) return SUMA_OK;
  int rc = pg_prepare(g);
  if (rc != SUMA_OK) return rc;
  double err;
  if ((rc = pg_eval(g, g->X, &err)) != SUMA_OK) return rc;
  st.initial_error = st.final_error = err;
  double lam = p.lambda_initial;
  const uint32_t n = g->n_dev;
  const PgSystem S = pg_system(g);
  if (max_iterations > 0 && err <= p.error_tol) st.termination = SUMA_PG_ERROR_TOL;
  uint32_t it = 0;
  bool changed = false;
  while (max_iterations > 0 && !(err <= p.error_tol)) {
    if ((rc = pg_linearize(g)) != SUMA_OK) return rc;
    ++it;
    const double prev = err;
    bool accepted = false, stop = false, bound = false;
    for (;;) {
      ++st.linear_solves;
      accepted = stop = false;
      hipLaunchKernelGGL(k_pg_solve, dim3(1), dim3(PG_SOLVE_THREADS), 0, g->stream, S, lam, p.cg_tolerance,
                         p.cg_max_iterations, g->dst.p);
      hipLaunchKernelGGL(k_pg_retract, dim3(grid(n)), dim3(PG_BLOCK), 0, g->stream, n, g->X.p, S.x, g->Xn.p);
      double en;
      if ((rc = pg_eval(g, g->Xn, &en)) != SUMA_OK) return rc;
      const double lin = g->hst->lin_change;
      st.cg_iterations += g->hst->cg_iterations;
      if (lin >= 0) {
        const double change = err - en;
        accepted = (lin > 1e-20 ? change / lin > p.min_model_fidelity : true) && std::isfinite(en);
        stop = accepted || std::fabs(change) < p.relative_error_tol * err;
      }
      if (accepted) {
        std::swap(g->X, g->Xn);
        err = en;
        changed = true;
        lam = std::max(p.lambda_lower_bound, lam / p.lambda_factor);
        break;
      }
      if (stop) break;
      lam *= p.lambda_factor;
      if (lam >= p.lambda_upper_bound) {
        bound = true;
        break;
      }
    }
    st.iterations = it, st.final_error = err, st.lambda = lam;
    if (bound) {
      st.termination = SUMA_PG_LAMBDA_BOUND;
      break;
    }
    if (it >= max_iterations) {
      st.termination = SUMA_PG_MAX_ITERATIONS;
      break;
    }
    if (err <= p.error_tol) {
      st.termination = SUMA_PG_ERROR_TOL;
      break;
    }
    const double dec = prev - err;
    if (dec <= p.absolute_error_tol || dec / prev <= p.relative_error_tol) {
      st.termination = SUMA_PG_CONVERGED;
      break;
    }
  }
  st.lambda = lam;
  if (changed) {
    std::vector<double> X(12 * (size_t)n);
    PG_HIP(g, hipMemcpyAsync(X.data(), g->X, 8 * X.size(), hipMemcpyDeviceToHost, g->stream));
    PG_HIP(g, hipStreamSynchronize(g->stream));
    if (!finite_n(X.data(), X.size())) return pg_fail(g, SUMA_ERR_HIP, "optimize: non-finite poses (not stored)");
    g->result.swap(X);
  }
  if (stats) *stats = st;
  return SUMA_OK;
}

}  // extern "C"

/* for the scan pipeline's loop closing (suma_loop.hip): the poses where they lie, rigid R (row-major) | t, 12 doubles a
 * node.  device: the optimiser's result buffer, valid behind a suma_posegraph_optimize of a non-empty graph (its
 * stream has been synchronised when that returns). */
const double* posegraph_host_poses(const suma_posegraph* g, uint32_t* n) {
  *n = (uint32_t)(g->result.size() / 12);
  return g->result.data();
}
const double* posegraph_device_poses(const suma_posegraph* g, uint32_t* n) {
  *n = g->n_dev;
  return g->X.p;
}
const double* posegraph_host_initial(const suma_posegraph* g, uint32_t* n) {
  *n = (uint32_t)(g->initial.size() / 12);
  return g->initial.data();
}
/* for a restored checkpoint (suma_loop.hip): the nodes as they were saved.  to_device: the graph is prepared and its
 * stream synchronised, so that X holds `result` as it does behind suma_posegraph_optimize */
int posegraph_install_nodes(suma_posegraph* g, const double* initial12, const double* result12, uint32_t n, bool to_device) {
  if (!g || (n && (!initial12 || !result12))) return SUMA_ERR_INVALID;
  if (n > g->node_cap) return pg_fail(g, SUMA_ERR_CAPACITY, "install_nodes: node capacity exceeded");
  if (!finite_n(initial12, 12 * (size_t)n) || !finite_n(result12, 12 * (size_t)n))
    return pg_fail(g, SUMA_ERR_INVALID, "install_nodes: non-finite pose");
  g->initial.assign(initial12, initial12 + 12 * (size_t)n);
  g->result.assign(result12, result12 + 12 * (size_t)n);
  g->structure_dirty = true;
  if (!to_device || n == 0) return SUMA_OK;
  const int rc = pg_prepare(g);
  if (rc != SUMA_OK) return rc;
  PG_HIP(g, hipStreamSynchronize(g->stream));
  return SUMA_OK;
}
