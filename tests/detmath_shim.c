/* test shim: exposes include/suma_detmath.h (the shared math specification) to Python, and is the gcc-built host side
 * of tests/detmath_device.hip: dm_* evaluate the inputs of tests/detmath_inputs.h with the specification as the CPU
 * oracle compiles it (oracle/o_math.h) and compare them with the device's bits. */
#include "../oracle/o_math.h"
#include "detmath_inputs.h"
#define V1(name, fn) void name(const float* x, float* y, int n) { for (int i = 0; i < n; ++i) y[i] = fn(x[i]); }
V1(t_atan, sdm_atan) V1(t_asin, sdm_asin) V1(t_acos, sdm_acos) V1(t_sin, sdm_sin) V1(t_cos, sdm_cos)
V1(t_exp, sdm_exp) V1(t_log, sdm_log) V1(t_floor, sdm_floor) V1(t_round, sdm_round) V1(t_sqrt, sdm_sqrt)
void t_atan2(const float* y, const float* x, float* r, int n) { for (int i = 0; i < n; ++i) r[i] = sdm_atan2(y[i], x[i]); }
void t_sin_d(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = sdm_sin_d(x[i]); }
void t_cos_d(const double* x, double* y, int n) { for (int i = 0; i < n; ++i) y[i] = sdm_cos_d(x[i]); }

/* ---- host side of tests/test_gpu_detmath.py ---- */

/* the 32-bit input words of case i of test t; returns their number */
int dm_inputs(int t, uint64_t i, int log2n, uint32_t* in) {
  if (t <= T_I2F) {
    in[0] = di_unary(t, i, log2n);
    return 1;
  }
  if (t <= T_DIV) {
    di_binary(t, i, &in[0], &in[1]);
    return 2;
  }
  if (t == T_FMA) {
    di_ternary(i, &in[0], &in[1], &in[2]);
    return 3;
  }
  if (t <= T_COS_D) {
    const uint64_t u = di_double(i);
    in[0] = (uint32_t)u;
    in[1] = (uint32_t)(u >> 32);
    return 2;
  }
  if (t == T_PACK_RGB) {
    for (uint32_t k = 0; k < 3; ++k) in[k] = di_unit(i, k);
    return 3;
  }
  if (t == T_DEPTH24) {
    in[0] = (uint32_t)i;
    return 1;
  }
  const int n = (t == T_M4_POINT || t == T_M4_DIR) ? 19 : (t == T_M4_MUL) ? 32 : 6;
  for (int k = 0; k < n; ++k) in[k] = di_vcomp(i, (uint32_t)k);
  return n;
}

static void put3(uint32_t* o, ov3 v) {
  o[0] = sdm_f2u(v.x);
  o[1] = sdm_f2u(v.y);
  o[2] = sdm_f2u(v.z);
}

/* host result of case i of test t: di_nout(t) words */
void dm_eval(int t, uint64_t i, int log2n, uint32_t* o) {
  uint32_t in[32] = {0};
  dm_inputs(t, i, log2n, in);
  float f[32];
  memcpy(f, in, sizeof f);
  const float x = f[0];
  const ov3 a = ov3_make(f[0], f[1], f[2]), b = ov3_make(f[3], f[4], f[5]);
  double d;
  memcpy(&d, in, 8);
  uint64_t r64;
  switch (t) {
    case T_ATAN: o[0] = sdm_f2u(sdm_atan(x)); break;
    case T_ASIN: o[0] = sdm_f2u(sdm_asin(x)); break;
    case T_ACOS: o[0] = sdm_f2u(sdm_acos(x)); break;
    case T_SIN: o[0] = sdm_f2u(sdm_sin(x)); break;
    case T_COS: o[0] = sdm_f2u(sdm_cos(x)); break;
    case T_EXP: o[0] = sdm_f2u(sdm_exp(x)); break;
    case T_LOG: o[0] = sdm_f2u(sdm_log(x)); break;
    case T_FLOOR: o[0] = sdm_f2u(sdm_floor(x)); break;
    case T_ROUND: o[0] = sdm_f2u(sdm_round(x)); break;
    case T_SQRT: o[0] = sdm_f2u(sdm_sqrt(x)); break;
    case T_RINT: o[0] = sdm_f2u(__builtin_rintf(x)); break;
    /* the specification converts only inside guards (|x| < 2^23 in floor / round, |x| <= 10431 in sin / cos) */
    case T_F2I: o[0] = (sdm_abs(x) < 2147483648.0f) ? (uint32_t)(int32_t)x : 0xdeadbeefu; break;
    case T_I2F: o[0] = sdm_f2u((float)(int32_t)in[0]); break;
    case T_ATAN2: o[0] = sdm_f2u(sdm_atan2(f[0], f[1])); break;
    case T_DIV: o[0] = sdm_f2u(f[0] / f[1]); break;
    case T_FMA: o[0] = sdm_f2u(__builtin_fmaf(f[0], f[1], f[2])); break;
    case T_SIN_D:
    case T_COS_D:
      d = (t == T_SIN_D) ? sdm_sin_d(d) : sdm_cos_d(d);
      memcpy(&r64, &d, 8);
      o[0] = (uint32_t)r64;
      o[1] = (uint32_t)(r64 >> 32);
      break;
    case T_DOT3: o[0] = sdm_f2u(ov3_dot(a, b)); break;
    case T_LEN3: o[0] = sdm_f2u(ov3_len(a)); break;
    case T_NORMALIZE3: put3(o, ov3_normalize(a)); break;
    case T_CROSS3: put3(o, ov3_cross(a, b)); break;
    case T_DIVS3: put3(o, ov3_divs(a, f[3])); break;
    case T_M4_POINT: put3(o, om4_point(f + 3, a)); break;
    case T_M4_DIR: put3(o, om4_dir(f + 3, a)); break;
    case T_M4_MUL: {
      float c[16];
      om4_mul(f, f + 16, c);
      memcpy(o, c, sizeof c);
      break;
    }
    case T_PACK_RGB: o[0] = sdm_f2u(o_pack(f[0], f[1], f[2])); break;
    case T_DEPTH24: o[0] = o_depth24(x); break;
    default: o[0] = 0xffffffffu;
  }
}

static int word_is_nan(int t, const uint32_t* w, int k) {
  if (t == T_F2I || t == T_DEPTH24) return 0;
  if (t == T_SIN_D || t == T_COS_D) {
    const uint32_t hi = w[k | 1], lo = w[k & ~1];
    return (hi & 0x7fffffffu) > 0x7ff00000u || ((hi & 0x7fffffffu) == 0x7ff00000u && lo != 0);
  }
  return (w[k] & 0x7fffffffu) > 0x7f800000u;
}

#define DM_FIRST 4
/* Compare the device's words of cases [base, base + n) of test t with the host's.  Returns the number of cases whose
 * bits differ; *nonnan counts those among them where the two sides are not both NaN at every differing word.  first /
 * first_nonnan receive the smallest such case indices (up to DM_FIRST each, UINT64_MAX where there are fewer). */
uint64_t dm_check(int t, int log2n, uint64_t base, uint64_t n, const uint32_t* dev, uint64_t* nonnan, uint64_t* first,
                  uint64_t* first_nonnan) {
  const int nout = di_nout(t);
  uint64_t mism = 0, mism_nonnan = 0;
  for (int k = 0; k < DM_FIRST; ++k) first[k] = first_nonnan[k] = UINT64_MAX;
#pragma omp parallel reduction(+ : mism, mism_nonnan)
  {
    uint64_t f[DM_FIRST], fn[DM_FIRST];
    int nf = 0, nfn = 0;
#pragma omp for schedule(static)
    for (uint64_t j = 0; j < n; ++j) {
      uint32_t h[16];
      dm_eval(t, base + j, log2n, h);
      const uint32_t* d = dev + j * (uint64_t)nout;
      int differ = 0, value = 0;
      for (int k = 0; k < nout; ++k)
        if (h[k] != d[k]) {
          differ = 1;
          if (!(word_is_nan(t, h, k) && word_is_nan(t, d, k))) value = 1;
        }
      if (differ) {
        ++mism;
        if (nf < DM_FIRST) f[nf++] = base + j;
      }
      if (value) {
        ++mism_nonnan;
        if (nfn < DM_FIRST) fn[nfn++] = base + j;
      }
    }
#pragma omp critical
    {
      /* each thread's indices are ascending (static schedule): merge into the global smallest */
      for (int q = 0; q < nf; ++q)
        for (int k = 0; k < DM_FIRST; ++k)
          if (f[q] < first[k]) {
            for (int s = DM_FIRST - 1; s > k; --s) first[s] = first[s - 1];
            first[k] = f[q];
            break;
          }
      for (int q = 0; q < nfn; ++q)
        for (int k = 0; k < DM_FIRST; ++k)
          if (fn[q] < first_nonnan[k]) {
            for (int s = DM_FIRST - 1; s > k; --s) first_nonnan[s] = first_nonnan[s - 1];
            first_nonnan[k] = fn[q];
            break;
          }
    }
  }
  *nonnan = mism_nonnan;
  return mism;
}
