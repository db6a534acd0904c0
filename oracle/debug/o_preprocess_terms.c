/*
 * oracle/debug/o_preprocess_terms.c -- TEST INFRASTRUCTURE (CPU oracle), stage export for
 * tests/test_preprocess_crafted_host.py.
 *
 * The fp32 intermediates that K1 .. K3 (o_preprocess.c) compare, formed with the oracle's own helpers in the oracle's
 * operation order: per point the texel coordinates before the floor and the window depth before the 24-bit rounding;
 * per texel of a vertex map the length of the cross product that K2 holds against 1e-7 and the range that K3's test
 * compares.  It reads the context's parameters and changes nothing; like o_update_terms.c it lives beside the oracle
 * proper, so that the arithmetic specification (the .c and .h files of oracle/ itself) stays as recorded.  The host test
 * pins these terms to what ora_preprocess itself decided: the floor of the coordinates names the texel in which the
 * point's coordinates turn up, and the sign of len - 1e-7 is the normal's w.
 */
#include "../o_ctx.h"

static inline int32_t t_wrap(int32_t x, int32_t w) {
  while (x >= w) x -= w;
  while (x < 0) x += w;
  return x;
}

/* terms: n x 3 = (0.5 (x + 1)) W, (0.5 (y + 1)) H, zw */
void ora_debug_preprocess_point_terms(const ora_ctx* c, const suma_float4* pts, uint32_t n, float* terms) {
  const suma_params* p = &c->p;
  const float width = (float)(int32_t)p->data_width, height = (float)(int32_t)p->data_height;
  const float fov_up = fabsf(p->data_fov_up), fov_down = fabsf(p->data_fov_down);
  const float fov = fabsf(fov_up) + fabsf(fov_down);
  const float min_depth = p->min_depth, max_depth = p->max_depth;
  for (uint32_t i = 0; i < n; ++i) {
    ov3 pos = ov3_make(pts[i].x, pts[i].y, pts[i].z);
    float depth = ov3_len(pos);
    float yaw = sdm_atan2(pos.y, pos.x);
    float pitch = -sdm_asin(pos.z / depth);
    float x = (-yaw * SUMA_INV_PI_F);
    float y = (1.0f - (2.0f * ((pitch * SUMA_RAD2DEG_F) + fov_up)) / fov);
    float z = 2.0f * ((depth - min_depth) / (max_depth - min_depth)) - 1.0f;
    terms[3 * (size_t)i + 0] = (0.5f * (x + 1.0f)) * width;
    terms[3 * (size_t)i + 1] = (0.5f * (y + 1.0f)) * height;
    terms[3 * (size_t)i + 2] = 0.5f * z + 0.5f;
  }
}

/* terms: P x 2 = |un x vn| of K2 at the texel (whatever the validity rules say), |xyz| of K3 */
void ora_debug_preprocess_map_terms(const ora_ctx* c, const suma_float4* V, float* terms) {
  const int32_t W = (int32_t)c->p.data_width, H = (int32_t)c->p.data_height;
  for (int32_t y = 0; y < H; ++y)
    for (int32_t x = 0; x < W; ++x) {
      const size_t pix = (size_t)y * W + x;
      const suma_float4 p = V[pix];
      const suma_float4 u = o_texel(V, W, H, t_wrap(x + 1, W), y), v = o_texel(V, W, H, x, y + 1);
      const ov3 pp = ov3_make(p.x, p.y, p.z);
      const ov3 un = ov3_normalize(ov3_sub(ov3_make(u.x, u.y, u.z), pp));
      const ov3 vn = ov3_normalize(ov3_sub(ov3_make(v.x, v.y, v.z), pp));
      terms[2 * pix + 0] = ov3_len(ov3_cross(un, vn));
      terms[2 * pix + 1] = ov3_len(pp);
    }
}
