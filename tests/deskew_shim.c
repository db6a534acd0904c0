/*
 * deskew_shim.c -- host restatement of the motion compensation csrc/k_deskew.hip specifies, written from the
 * specification at the top of that file (parts A and B) and sharing only include/suma_detmath.h with the library.
 * The library must equal it to the byte (tests/test_gpu_deskew.py).  Compile with -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../include/suma_detmath.h"

typedef struct {
  int32_t time_source, clockwise;
  float start_azimuth, t_ref, scale;
} shim_deskew_params;

typedef struct {
  float v[3], a[3], b[3], c[3];
  float theta, inv_theta;
} shim_twist;

static void cross_d(const double* u, const double* w, double* o) {
  o[0] = u[1] * w[2] - u[2] * w[1];
  o[1] = u[2] * w[0] - u[0] * w[2];
  o[2] = u[0] * w[1] - u[1] * w[0];
}

/* part A */
void deskew_shim_twist(const double* M, float scale_f, shim_twist* o) {
  const double t[3] = {M[12], M[13], M[14]};
  const double q[3] = {0.5 * (M[6] - M[9]), 0.5 * (M[8] - M[2]), 0.5 * (M[1] - M[4])};
  const double sn = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  const double cs = 0.5 * (((M[0] + M[5]) + M[10]) - 1.0);
  const double theta0 = atan2(sn, cs);
  double a[3] = {0.0, 0.0, 1.0}, v0[3] = {t[0], t[1], t[2]};
  int rot = 0;
  if (sn > 0.0)
    for (int j = 0; j < 3; ++j) a[j] = q[j] / sn;
  if (!(theta0 < 1e-6)) {
    const double h = 0.5 * theta0;
    const double k = 1.0 - (h * sdm_cos_d(h)) / sdm_sin_d(h);
    double b0[3], c0[3];
    cross_d(a, t, b0);
    cross_d(a, b0, c0);
    for (int j = 0; j < 3; ++j) v0[j] = (t[j] - h * b0[j]) + k * c0[j];
    rot = 1;
  }
  const double scale = (double)scale_f;
  const double v[3] = {scale * v0[0], scale * v0[1], scale * v0[2]};
  const double theta = scale * theta0;
  if ((float)theta == 0.0f) rot = 0;
  double b[3], c[3];
  cross_d(a, v, b);
  cross_d(a, b, c);
  for (int j = 0; j < 3; ++j) {
    o->v[j] = (float)v[j];
    o->a[j] = (float)a[j];
    o->b[j] = (float)b[j];
    o->c[j] = (float)c[j];
  }
  o->theta = rot ? (float)theta : 0.0f;
  o->inv_theta = rot ? (float)(1.0 / theta) : 0.0f;
}

static int finite_f(float f) { return (sdm_f2u(f) & 0x7fffffffu) < 0x7f800000u; }

/* parts A and B: n points (x, y, z, w) -> out (may be in); times may be NULL for the azimuth source */
void deskew_shim_points(const shim_deskew_params* dp, const float* in, const float* times, uint32_t n, const double* M,
                        float* out) {
  double I[16];
  for (int k = 0; k < 16; ++k) I[k] = (k % 5 == 0) ? 1.0 : 0.0;
  if (memcmp(M, I, sizeof(I)) == 0) {
    if (out != in) memmove(out, in, (size_t)n * 16);
    return;
  }
  shim_twist w;
  deskew_shim_twist(M, dp->scale, &w);
  const int use_times = dp->time_source == 1;
  for (uint32_t i = 0; i < n; ++i) {
    float p[4];
    memcpy(p, in + 4 * (size_t)i, 16);
    const float tm = use_times ? times[i] : 0.0f;
    if (!(finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]) && finite_f(tm))) {
      memmove(out + 4 * (size_t)i, p, 16);
      continue;
    }
    float s;
    if (use_times) {
      s = tm;
    } else {
      float u = (sdm_atan2(p[1], p[0]) - dp->start_azimuth) / 6.28318530717958647692f;
      u = u - sdm_floor(u);
      s = dp->clockwise ? 1.0f - u : u;
    }
    const float d = s - dp->t_ref;
    const float phi = d * w.theta;
    const float sn = sdm_sin(phi);
    const float hs = sdm_sin(0.5f * phi);
    const float omc = (2.0f * hs) * hs;
    const float ap[3] = {w.a[1] * p[2] - w.a[2] * p[1], w.a[2] * p[0] - w.a[0] * p[2], w.a[0] * p[1] - w.a[1] * p[0]};
    const float aap[3] = {w.a[1] * ap[2] - w.a[2] * ap[1], w.a[2] * ap[0] - w.a[0] * ap[2], w.a[0] * ap[1] - w.a[1] * ap[0]};
    const float k1 = omc * w.inv_theta, k2 = (phi - sn) * w.inv_theta;
    float o[4];
    for (int j = 0; j < 3; ++j) {
      const float r = (p[j] + sn * ap[j]) + omc * aap[j];
      const float t = (d * w.v[j] + k1 * w.b[j]) + k2 * w.c[j];
      o[j] = r + t;
    }
    memcpy(&o[3], &p[3], 4);
    memcpy(out + 4 * (size_t)i, o, 16);
  }
}
