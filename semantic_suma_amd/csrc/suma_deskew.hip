/*
 * suma_deskew.hip -- motion compensation of raw sweeps (include/suma_hip.h, suma_deskew_* and suma_pipeline_*deskew*).
 * Host code: the parameter checks, the primitive on host and device points, and the state a pipeline keeps while the
 * correction is enabled.  k_deskew.hip states the operation and holds the kernel; the localiser's entries are in
 * suma_localize.hip and use deskew_scan below.
 */
#include <string.h>

#include <cmath>
#include <new>

#include "suma_internal.h"

extern "C" void suma_deskew_params_default(suma_deskew_params* dp) {
  if (!dp) return;
  dp->time_source = SUMA_DESKEW_TIME_AZIMUTH;
  dp->clockwise = 0;
  dp->start_azimuth = 0.0f;
  dp->t_ref = 0.5f;
  dp->scale = 1.0f;
}

static const char* deskew_params_why(const suma_deskew_params& q, bool for_scans) {
  if (q.time_source != SUMA_DESKEW_TIME_AZIMUTH && q.time_source != SUMA_DESKEW_TIME_TIMES) return "unknown time_source";
  if (for_scans && q.time_source == SUMA_DESKEW_TIME_TIMES)
    return "the scan entries carry no per-point times: correct such scans with suma_deskew_points first";
  if (q.clockwise != 0 && q.clockwise != 1) return "clockwise must be 0 or 1";
  if (!(std::isfinite(q.start_azimuth) && std::fabs(q.start_azimuth) <= 6.2831855f)) return "start_azimuth must lie in [-2 pi, 2 pi]";
  if (!(q.t_ref >= 0.0f && q.t_ref <= 1.0f)) return "t_ref must lie in [0, 1]";
  if (!std::isfinite(q.scale)) return "scale must be finite";
  return nullptr;
}

int deskew_params_check(suma_ctx* c, const suma_deskew_params* dp, bool for_scans, const char* who) {
  suma_deskew_params q;
  suma_deskew_params_default(&q);
  if (dp) q = *dp;
  const char* why = deskew_params_why(q, for_scans);
  return why ? fail(c, SUMA_ERR_INVALID, std::string(who) + ": " + why) : SUMA_OK;
}

static bool motion_finite(const double* T) {
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(T[k])) return false;
  return true;
}

/* host only: what suma_deskew_points would refuse about its parameters, before any device is touched */
extern "C" int suma_deskew_check(const suma_deskew_params* dp, int have_times, const double motion[16]) {
  suma_deskew_params q;
  suma_deskew_params_default(&q);
  if (dp) q = *dp;
  const char* why = deskew_params_why(q, false);
  if (!why && !motion) why = "NULL motion";
  if (!why && !motion_finite(motion)) why = "non-finite motion";
  if (!why && q.time_source == SUMA_DESKEW_TIME_TIMES && !have_times) why = "time source `times` without times";
  return why ? fail_without_ctx(SUMA_ERR_INVALID, std::string("suma_deskew_points: ") + why) : SUMA_OK;
}

static int deskew_check_call(suma_ctx* c, const suma_deskew_params* dp, const void* points, const float* times, uint32_t n,
                             const double* motion, const void* out, suma_deskew_params* q) {
  if (!c) return SUMA_ERR_INVALID;
  suma_deskew_params_default(q);
  if (dp) *q = *dp;
  if (suma_deskew_check(dp, times != nullptr || n == 0, motion) != SUMA_OK) /* n = 0 reads no times */ return fail(c, SUMA_ERR_INVALID, suma_last_error(nullptr));
  if (n && (!points || !out)) return fail(c, SUMA_ERR_INVALID, "suma_deskew_points: NULL points with n > 0");
  return SUMA_OK;
}

extern "C" int suma_deskew_points_device(suma_ctx* c, const suma_deskew_params* dp, const suma_float4* d_points,
                                         const float* d_times, uint32_t n, const double motion[16], suma_float4* d_out) {
  suma_deskew_params q;
  int r = deskew_check_call(c, dp, d_points, d_times, n, motion, d_out, &q);
  if (r || n == 0) return r;
  if (((uintptr_t)d_points | (uintptr_t)d_out) & 15u) return fail(c, SUMA_ERR_INVALID, "suma_deskew_points_device: points must be 16-byte aligned");
  if (deskew_is_identity(motion)) {
    if (d_out != d_points)
      HIP_TRY(c, hipMemcpyAsync(d_out, d_points, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    return SUMA_OK;
  }
  DeskewArgs a;
  deskew_twist(q, motion, &a);
  ProfScope ps(c, "kd_deskew", (32.0 + (a.use_times ? 4.0 : 0.0)) * (double)n);
  HIP_TRY(c, launch_kd_deskew(c->stream, (const float4*)d_points, d_times, n, a, (float4*)d_out));
  return SUMA_OK;
}

extern "C" int suma_deskew_points(suma_ctx* c, const suma_deskew_params* dp, const suma_float4* points, const float* times,
                                  uint32_t n, const double motion[16], suma_float4* out) {
  suma_deskew_params q;
  int r = deskew_check_call(c, dp, points, times, n, motion, out, &q);
  if (r || n == 0) return r;
  if (deskew_is_identity(motion)) {
    if (out != points) memmove(out, points, (size_t)n * sizeof(suma_float4));
    return SUMA_OK;
  }
  const bool use_times = q.time_source == SUMA_DESKEW_TIME_TIMES;
  DevBuf<float4> d_pts; /* given back when the call returns: this entry is a convenience, not the scan path */
  DevBuf<float> d_times;
  HIP_TRY(c, d_pts.alloc(n));
  HIP_TRY(c, hipMemcpyAsync(d_pts, points, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  if (use_times) {
    HIP_TRY(c, d_times.alloc(n));
    HIP_TRY(c, hipMemcpyAsync(d_times, times, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  r = suma_deskew_points_device(c, &q, (const suma_float4*)d_pts.p, use_times ? d_times.p : nullptr, n, motion,
                                (suma_float4*)d_pts.p);
  if (r == SUMA_OK) {
    const hipError_t e = hipMemcpyAsync(out, d_pts, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) r = fail(c, SUMA_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  const hipError_t es = hipStreamSynchronize(c->stream); /* nothing uses the two blocks behind this */
  if (r == SUMA_OK && es != hipSuccess) r = fail(c, SUMA_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(es));
  return r;
}

int deskew_scan(suma_ctx* c, Deskew& dk, const double increment[16], hipStream_t st, const suma_float4* d_in, uint32_t n,
                const suma_float4** d_out) {
  const double* motion = dk.have_override ? dk.override_motion : increment;
  dk.last_source = dk.have_override ? SUMA_DESKEW_MOTION_OVERRIDE : SUMA_DESKEW_MOTION_INCREMENT;
  memcpy(dk.last_motion, motion, sizeof(dk.last_motion));
  dk.have_override = false;
  *d_out = d_in;
  if (n == 0 || deskew_is_identity(dk.last_motion)) return SUMA_OK;
  if (!motion_finite(dk.last_motion)) return fail(c, SUMA_ERR_INVALID, "motion compensation: the motion of the sweep is not finite");
  if ((uintptr_t)d_in & 15u) return fail(c, SUMA_ERR_INVALID, "motion compensation: points must be 16-byte aligned");
  const int g = grow(c, dk.points, n, {c->stream, c->side_stream}, (size_t)n + n / 4 + 1024);
  if (g < 0) return g;
  DeskewArgs a;
  deskew_twist(dk.dp, dk.last_motion, &a);
  HIP_TRY(c, launch_kd_deskew(st, (const float4*)d_in, nullptr, n, a, dk.points));
  *d_out = (const suma_float4*)dk.points.p;
  return SUMA_OK;
}

/* ---- the pipeline's switch ---- */
extern "C" int suma_pipeline_enable_deskew(suma_pipeline* s, const suma_deskew_params* dp) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  int r = deskew_params_check(c, dp, true, "suma_pipeline_enable_deskew");
  if (r) return r;
  if (s->phase != 0) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_enable_deskew: only between scans");
  if (ingest_pending(c)) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_enable_deskew: scans staged with suma_pipeline_prefetch_scan are pending");
  if (!s->deskew) {
    s->deskew = new (std::nothrow) Deskew();
    if (!s->deskew) return fail(c, SUMA_ERR_NOMEM, "out of host memory");
    mat4_eye(s->deskew->last_motion);
  }
  suma_deskew_params_default(&s->deskew->dp);
  if (dp) s->deskew->dp = *dp;
  s->deskew->on = true;
  return SUMA_OK;
}

extern "C" int suma_pipeline_disable_deskew(suma_pipeline* s) {
  if (!s) return SUMA_ERR_INVALID;
  if (s->deskew) {
    s->deskew->on = false;
    s->deskew->have_override = false;
  }
  return SUMA_OK;
}

extern "C" int suma_pipeline_set_deskew_motion(suma_pipeline* s, const double motion[16]) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  if (!s->deskew || !s->deskew->on) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_set_deskew_motion: motion compensation is not enabled");
  if (!motion) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_set_deskew_motion: NULL motion");
  if (!motion_finite(motion)) return fail(c, SUMA_ERR_INVALID, "suma_pipeline_set_deskew_motion: non-finite motion");
  memcpy(s->deskew->override_motion, motion, 16 * sizeof(double));
  s->deskew->have_override = true;
  return SUMA_OK;
}

extern "C" int suma_pipeline_deskew_motion(const suma_pipeline* s, double motion[16], int32_t* source) {
  if (!s || !motion) return SUMA_ERR_INVALID;
  if (s->deskew) {
    memcpy(motion, s->deskew->last_motion, 16 * sizeof(double));
    if (source) *source = s->deskew->last_source;
  } else {
    mat4_eye(motion);
    if (source) *source = SUMA_DESKEW_MOTION_NONE;
  }
  return SUMA_OK;
}

void deskew_destroy(suma_pipeline* s) {
  if (!s || !s->deskew) return;
  delete s->deskew;
  s->deskew = nullptr;
}
