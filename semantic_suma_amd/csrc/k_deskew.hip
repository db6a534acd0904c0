/*
 * k_deskew.hip -- motion compensation of one sweep.  A rotating lidar on a moving platform measures every column of a
 * sweep from another pose; K1 and everything behind it treat a scan as a snapshot from one pose.  kd_deskew moves every
 * point from the sensor frame of the instant it was measured into the sensor frame at one reference instant of the
 * sweep, given the sensor's rigid motion over the sweep.  Nothing in the reference does this: the KITTI odometry scans
 * it is run on are compensated already.
 *
 * Kernel (VGPRs: tools/isa_stats.py k_deskew.hip; no scratch, no LDS, no atomics):
 *   kd_deskew  lane per point, blocks of 256: one 16-byte load, the optional 4-byte time, one 16-byte store.  The twist
 *              arrives by value in the argument struct (DeskewArgs, suma_internal.h), so a launch depends on nothing a
 *              later call could change.  in == out is allowed: a lane reads and writes its own point only.
 *
 * SPECIFICATION (tests/deskew_shim.c restates it on the host, byte for byte).
 *
 * The operation: a point p measured at sweep fraction s becomes  p' = Exp((s - t_ref) * xi) * p,  xi = scale * Log(motion),
 * motion = pose_prev^-1 * pose, the sensor's motion over one scan interval, column-major double[16].
 *
 * A. Host, fp64, once per call (deskew_twist below; every operation as written, no contraction; sin and cos are
 *    sdm_sin_d / sdm_cos_d, sqrt is the IEEE one, atan2 is the C library's):
 *      R(r, c) = motion[4 c + r], t = (motion[12], motion[13], motion[14]).
 *      q = 0.5 * (R(2,1) - R(1,2), R(0,2) - R(2,0), R(1,0) - R(0,1))                       (sin(theta0) * axis)
 *      sn = sqrt((q0 q0 + q1 q1) + q2 q2),  cs = 0.5 * (((R(0,0) + R(1,1)) + R(2,2)) - 1.0),  theta0 = atan2(sn, cs)
 *      a = q / sn if sn > 0, else (0, 0, 1).
 *      SMALL ANGLE: theta0 < SUMA_DESKEW_SMALL_THETA (1e-6 rad) is a pure translation: v0 = t, rot = false.  Else
 *        h = 0.5 * theta0, k = 1.0 - (h * cos(h)) / sin(h), b0 = a x t, c0 = a x b0, v0 = (t - h * b0) + k * c0
 *        (V^-1 t of SE(3): I - W / 2 + k [a]x^2), rot = true.  Rotations near pi (theta0 > 3) are outside what a sweep
 *        does; the axis loses its digits there.
 *      v = scale * v0, theta = scale * theta0; rot also needs (float)theta != 0.
 *      b = a x v, c = a x b  (cross(u, w) = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0)).
 *      The kernel receives, each rounded to fp32: v, a, b, c, theta and inv_theta = 1.0 / theta (both 0 unless rot),
 *      t_ref, start_azimuth, and the two switches.
 *    IDENTITY: a motion whose 16 doubles are bitwise those of the identity launches nothing; every output bit is the
 *      input's (in != out: a copy).  n = 0 launches nothing.
 * B. Device, fp32, per point (x, y, z, w), every operation as written, -ffp-contract=off, no FMA:
 *      PASS-THROUGH: if x, y or z is not finite, or the time source is `times` and times[i] is not finite, the output
 *        is the input's 16 bytes.
 *      TIME.  times: s = times[i], as given, not clamped (|(s - t_ref) * theta| > 8192 leaves sdm_sin's domain: NaN).
 *        azimuth: u = (sdm_atan2(y, x) - start_azimuth) / 6.28318530717958647692f;  u = u - sdm_floor(u);
 *          s = clockwise ? 1.0f - u : u.
 *          u lies in [0, 1]; a point exactly on the start azimuth has u == 0: the START of the sweep (s = 0) for a
 *          counter-clockwise sensor, its END (s = 1) for a clockwise one.  The far end u == 1.0f only arises by rounding
 *          of a tiny negative quotient.  x == y == 0 has azimuth 0 (sdm_atan2).
 *      d = s - t_ref, phi = d * theta, sn = sdm_sin(phi), hs = sdm_sin(0.5f * phi), omc = (2.0f * hs) * hs
 *        (1 - cos phi by the half angle: no cancellation at small angles).
 *      ROTATION (Rodrigues about the unit axis a): ap = a x p, aap = a x ap,
 *        r_i = (p_i + sn * ap_i) + omc * aap_i.
 *      TRANSLATION (the V matrix of SE(3) applied to d * v, with phi = d * theta divided out):
 *        k1 = omc * inv_theta, k2 = (phi - sn) * inv_theta,  t_i = (d * v_i + k1 * b_i) + k2 * c_i.
 *      p'_i = r_i + t_i;  w is copied bit for bit.
 *      With rot false (theta = inv_theta = 0) the same expressions are evaluated: phi = 0, sn = hs = omc = k1 = k2 = 0.
 */
#include <string.h>

#include "suma_internal.h"

#define DSK_THREADS 256

__device__ __forceinline__ bool dsk_finite(float f) { return (__float_as_uint(f) & 0x7fffffffu) < 0x7f800000u; }

__global__ void __launch_bounds__(DSK_THREADS)
    kd_deskew(const float4* in, const float* times, uint32_t n, DeskewArgs a, float4* out) {
  const uint32_t i = blockIdx.x * DSK_THREADS + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  const float tm = a.use_times ? times[i] : 0.0f;
  float4 o = p;
  if (dsk_finite(p.x) && dsk_finite(p.y) && dsk_finite(p.z) && dsk_finite(tm)) {
    float s;
    if (a.use_times) {
      s = tm;
    } else {
      float u = (sdm_atan2(p.y, p.x) - a.start_azimuth) / 6.28318530717958647692f;
      u = u - sdm_floor(u);
      s = a.clockwise ? 1.0f - u : u;
    }
    const float d = s - a.t_ref;
    const float phi = d * a.theta;
    const float sn = sdm_sin(phi);
    const float hs = sdm_sin(0.5f * phi);
    const float omc = (2.0f * hs) * hs;
    const float apx = a.a[1] * p.z - a.a[2] * p.y, apy = a.a[2] * p.x - a.a[0] * p.z, apz = a.a[0] * p.y - a.a[1] * p.x;
    const float aapx = a.a[1] * apz - a.a[2] * apy, aapy = a.a[2] * apx - a.a[0] * apz, aapz = a.a[0] * apy - a.a[1] * apx;
    const float rx = (p.x + sn * apx) + omc * aapx;
    const float ry = (p.y + sn * apy) + omc * aapy;
    const float rz = (p.z + sn * apz) + omc * aapz;
    const float k1 = omc * a.inv_theta, k2 = (phi - sn) * a.inv_theta;
    const float tx = (d * a.v[0] + k1 * a.b[0]) + k2 * a.c[0];
    const float ty = (d * a.v[1] + k1 * a.b[1]) + k2 * a.c[1];
    const float tz = (d * a.v[2] + k1 * a.b[2]) + k2 * a.c[2];
    o.x = rx + tx;
    o.y = ry + ty;
    o.z = rz + tz;
  }
  out[i] = o;
}

/* ---- host side ---- */
bool deskew_is_identity(const double motion[16]) {
  double I[16];
  mat4_eye(I);
  return memcmp(motion, I, sizeof(I)) == 0;
}

/* part A of the specification */
void deskew_twist(const suma_deskew_params& dp, const double M[16], DeskewArgs* out) {
  const double t[3] = {M[12], M[13], M[14]};
  const double q[3] = {0.5 * (M[6] - M[9]), 0.5 * (M[8] - M[2]), 0.5 * (M[1] - M[4])};
  const double sn = sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  const double cs = 0.5 * (((M[0] + M[5]) + M[10]) - 1.0);
  const double theta0 = atan2(sn, cs);
  double a[3] = {0.0, 0.0, 1.0};
  if (sn > 0.0)
    for (int k = 0; k < 3; ++k) a[k] = q[k] / sn;
  double v0[3] = {t[0], t[1], t[2]};
  bool rot = false;
  if (!(theta0 < SUMA_DESKEW_SMALL_THETA)) {
    const double h = 0.5 * theta0;
    const double k = 1.0 - (h * sdm_cos_d(h)) / sdm_sin_d(h);
    const double b0[3] = {a[1] * t[2] - a[2] * t[1], a[2] * t[0] - a[0] * t[2], a[0] * t[1] - a[1] * t[0]};
    const double c0[3] = {a[1] * b0[2] - a[2] * b0[1], a[2] * b0[0] - a[0] * b0[2], a[0] * b0[1] - a[1] * b0[0]};
    for (int j = 0; j < 3; ++j) v0[j] = (t[j] - h * b0[j]) + k * c0[j];
    rot = true;
  }
  const double scale = (double)dp.scale;
  const double v[3] = {scale * v0[0], scale * v0[1], scale * v0[2]};
  const double theta = scale * theta0;
  if ((float)theta == 0.0f) rot = false;
  const double b[3] = {a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]};
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  for (int j = 0; j < 3; ++j) {
    out->v[j] = (float)v[j];
    out->a[j] = (float)a[j];
    out->b[j] = (float)b[j];
    out->c[j] = (float)c[j];
  }
  out->theta = rot ? (float)theta : 0.0f;
  out->inv_theta = rot ? (float)(1.0 / theta) : 0.0f;
  out->t_ref = dp.t_ref;
  out->start_azimuth = dp.start_azimuth;
  out->clockwise = dp.clockwise ? 1 : 0;
  out->use_times = dp.time_source == SUMA_DESKEW_TIME_TIMES ? 1 : 0;
}

hipError_t launch_kd_deskew(hipStream_t st, const float4* in, const float* times, uint32_t n, const DeskewArgs& a,
                            float4* out) {
  if (n == 0) return hipSuccess;
  kd_deskew<<<(n + DSK_THREADS - 1) / DSK_THREADS, DSK_THREADS, 0, st>>>(in, times, n, a, out);
  return hipGetLastError();
}
