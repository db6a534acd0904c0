/*
 * k_loop.hip -- integrateLoopClosures on the device (SurfelMapping.cpp:215-233): the optimised trajectory goes from the
 * pose-graph optimiser's fp64 result buffer to the map's float pose table (and its inverse table) in one launch,
 * without a host round trip for the table.
 *
 *   row i < n_opt                  poses[i] = float(opt[i])                          (:219-222)
 *   row n_opt <= i < n_opt + n_tail  poses[i] = float(difference * tail[i - n_opt])    (:227-231)
 *
 * opt: the optimiser's layout, 12 doubles a node, R row-major | t (k_posegraph.hip).  tail: the nodes the main graph
 * gained while the optimiser ran, column-major 4x4 doubles.  The product is mat4_mul's (suma_internal.h),
 * ((a0 b0 + a1 b1) + a2 b2) + a3 b3 without contraction (-ffp-contract=off), so the floats written here are the casts of
 * the doubles the host gives the main graph through setInitial, bit for bit.
 */
#include "suma_internal.h"

struct LoopDiff {
  double m[16];
};

__global__ void __launch_bounds__(256) k_loop_integrate(float* __restrict__ poses, float* __restrict__ poses_inv,
                                                        const double* __restrict__ opt, uint32_t n_opt,
                                                        const double* __restrict__ tail, uint32_t n_rows,
                                                        const LoopDiff D) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_rows) return;
  float m[16], inv[16];
  if (k < n_opt) {
    const double* o = opt + 12 * (size_t)k;
    for (int c = 0; c < 3; ++c) {
      for (int r = 0; r < 3; ++r) m[4 * c + r] = (float)o[3 * r + c];
      m[4 * c + 3] = 0.0f;
    }
    for (int r = 0; r < 3; ++r) m[12 + r] = (float)o[9 + r];
    m[15] = 1.0f;
  } else {
    const double* B = tail + 16 * (size_t)(k - n_opt);
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 4; ++r)
        m[4 * c + r] = (float)(((D.m[r] * B[4 * c] + D.m[4 + r] * B[4 * c + 1]) + D.m[8 + r] * B[4 * c + 2]) +
                               D.m[12 + r] * B[4 * c + 3]);
  }
  rigid_inverse_dev(m, inv);
  for (int i = 0; i < 16; ++i) {
    poses[16 * (size_t)k + i] = m[i];
    poses_inv[16 * (size_t)k + i] = inv[i];
  }
}

hipError_t launch_loop_integrate(suma_ctx* c, const double* d_opt12, uint32_t n_opt, const double* d_tail16,
                                 uint32_t n_tail, const double difference[16]) {
  /* the table holds max_poses rows (SurfelMap.h:205): rows beyond it are not written, as suma_map_update_poses */
  const uint32_t cap = c->p.max_poses;
  if (n_opt > cap) n_opt = cap;
  uint32_t n_rows = n_opt + n_tail;
  if (n_rows > cap || n_rows < n_opt) n_rows = cap;
  if (n_rows == 0) return hipSuccess;
  LoopDiff D;
  for (int i = 0; i < 16; ++i) D.m[i] = difference[i];
  k_loop_integrate<<<(n_rows + 255) / 256, 256, 0, c->ls>>>(c->poses, c->poses_inv, d_opt12, n_opt, d_tail16, n_rows, D);
  return hipGetLastError();
}
