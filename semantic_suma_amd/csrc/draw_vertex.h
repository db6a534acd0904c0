/*
 * draw_vertex.h -- the vertex stage of draw_surfels.vert as k_draw.hip specifies it (ARITHMETIC SPECIFICATION, "Vertex
 * stage"): a surfel's position and normal taken to the map frame through the pose of its creation scan.  Shared by the
 * rasteriser (k_draw.hip) and the world-frame export (k_world.hip), so that both place a surfel at the same bits.
 */
#ifndef SUMA_DRAW_VERTEX_H_
#define SUMA_DRAW_VERTEX_H_

#include "dev_math.h"

SDEV bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
SDEV float4 mat_vec(const float* m, float4 v) {
  return f4(SDEV_FMA(m[12], v.w, SDEV_FMA(m[8], v.z, SDEV_FMA(m[4], v.y, m[0] * v.x))),
            SDEV_FMA(m[13], v.w, SDEV_FMA(m[9], v.z, SDEV_FMA(m[5], v.y, m[1] * v.x))),
            SDEV_FMA(m[14], v.w, SDEV_FMA(m[10], v.z, SDEV_FMA(m[6], v.y, m[2] * v.x))),
            SDEV_FMA(m[15], v.w, SDEV_FMA(m[11], v.z, SDEV_FMA(m[7], v.y, m[3] * v.x))));
}

/* draw_surfels.vert: p = M * (x, y, z, 1), n = M * (n, 0) with M = poses[int(count)] */
SDEV void draw_vertex(const float* poses, uint32_t n_poses, const float4& s0, const float4& s1, float count, float4* p, float4* n) {
  const uint32_t k = (count >= 0.0f) ? ((count < (float)n_poses) ? (uint32_t)(int32_t)count : n_poses - 1u) : 0u;
  const float4* src = reinterpret_cast<const float4*>(poses + 16 * (size_t)k);
  float M[16];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float4 col = src[c];
    M[4 * c] = col.x;
    M[4 * c + 1] = col.y;
    M[4 * c + 2] = col.z;
    M[4 * c + 3] = col.w;
  }
  *p = mat_vec(M, f4(s0.x, s0.y, s0.z, 1.0f));
  *n = mat_vec(M, f4(s1.x, s1.y, s1.z, 0.0f));
}

#endif
