/*
 * detmath_inputs.h -- the input sets of tests/test_gpu_detmath.py, generated from an index.
 *
 * Included by tests/detmath_device.hip (device side: each thread makes its own inputs) and by tests/detmath_shim.c
 * (gcc side: the host oracle makes the same inputs).  Integer arithmetic only, plus one correctly rounded double
 * product per k*pi/4 centre, so both compilers produce the same bit patterns and nothing large crosses the bus.
 *
 * Every case is a flat index space [0, di_count(t)) per test t:
 *   unary fp32   strided bit patterns (i * DI_STRIDE: a permutation of all 2^32 patterns when 2^32 are taken), the
 *                edge set, +-4096-ulp windows around every branch threshold of include/suma_detmath.h, and for
 *                sin / cos +-4096-ulp windows around k*pi/4 for every k up to 8192 * 4/pi
 *   binary fp32  a 2^13 x 2^13 grid of strided bit patterns (atan2) or hashed random pairs, then edge set x edge set
 *   fma          hashed random triples, then edge set ^ 3
 *   fp64 sin/cos strided doubles over |x| <= 2^30, windows around k*pi/4, tiny arguments, the 2^30 cut-off, edges
 *   vector       dev_math.h helpers on hashed components that are normal, subnormal, huge (overflowing products),
 *                +0 or -0; depth24 on every pattern of [0, 1]
 */
#ifndef DETMATH_INPUTS_H_
#define DETMATH_INPUTS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define DI_HD __host__ __device__ static inline
#else
#define DI_HD static inline
#endif

enum {
  T_ATAN, T_ASIN, T_ACOS, T_SIN, T_COS, T_EXP, T_LOG, T_FLOOR, T_ROUND, T_SQRT, /* sdm_* unary fp32 */
  T_RINT, T_F2I, T_I2F,                                                        /* IEEE primitives, unary */
  T_ATAN2, T_DIV, T_FMA,                                                       /* binary / ternary fp32 */
  T_SIN_D, T_COS_D,                                                            /* fp64 */
  T_DOT3, T_LEN3, T_NORMALIZE3, T_CROSS3, T_DIVS3, T_M4_POINT, T_M4_DIR, T_M4_MUL, T_PACK_RGB, T_DEPTH24,
  T_COUNT
};

#define DI_STRIDE 0x9E3779B1u  /* odd: i * DI_STRIDE is a permutation of the 2^32 patterns */
#define DI_STRIDE2 0x85EBCA77u /* second odd stride for the x axis of the atan2 grid */
#define DI_WIN 4096u           /* half width of a threshold window, in ulps */
#define DI_WLEN (2u * DI_WIN + 1u)
#define DI_NEDGE 26u
#define DI_NTHR 13u
#define DI_KPI4 10430u /* floor(8192 * 4 / pi): the last k*pi/4 inside sdm_sin / sdm_cos' domain */
#define DI_GRID 8192u  /* atan2 grid side */
#define DI_NRAND (1u << 24) /* hashed random pairs / triples / vectors */

DI_HD uint32_t di_f2u(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
DI_HD uint64_t di_d2u(double f) {
  uint64_t u;
  __builtin_memcpy(&u, &f, 8);
  return u;
}

/* splitmix64 finaliser */
DI_HD uint64_t di_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

/* +-0, +-min subnormal, +-max subnormal, +-FLT_MIN, +-FLT_MAX, +-inf, quiet and signalling NaNs of either sign with
 * payloads, +-1, +-0.5, +-pi */
DI_HD uint32_t di_edge(uint32_t k) {
  const uint32_t e[DI_NEDGE] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu,
                                0x00800000u, 0x80800000u, 0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u,
                                0x7fc00000u, 0xffc00000u, 0x7fc12345u, 0xffd5aa55u, 0x7f800001u, 0xff812345u,
                                0x7fbfffffu, 0xffa00001u, 0x3f800000u, 0xbf800000u, 0x3f000000u, 0xbf000000u,
                                0x40490fdbu, 0xc0490fdbu};
  return e[k];
}

/* branch thresholds of include/suma_detmath.h (positive; both signs are windowed) */
DI_HD uint32_t di_threshold(uint32_t k) {
  const float t[DI_NTHR] = {
      1.0e-4f,               /* asin: identity below */
      0.5f,                  /* asin / acos: sqrt branch */
      1.0f,                  /* asin / acos: domain end */
      0.4142135623730950f,   /* atan: tan(pi/8) */
      2.414213562373095f,    /* atan: tan(3pi/8) */
      0.707106781186547524f, /* log: mantissa branch */
      88.72283905206835f,    /* exp: overflow */
      87.33654475f,          /* exp: -ln(FLT_MIN), subnormal results below -87.34 */
      103.278929903431851f,  /* exp: underflow to 0 */
      8192.0f,               /* sin / cos: domain end */
      8388608.0f,            /* floor / round: 2^23 */
      2147483648.0f,         /* float -> int32 range */
      1.17549435e-38f,       /* FLT_MIN: log's subnormal scale-up */
  };
  return di_f2u(t[k]);
}

/* number of strided patterns of a unary test: 2^log2n (32 = every pattern) */
DI_HD uint64_t di_nstride(int log2n) { return 1ull << log2n; }
DI_HD uint64_t di_nwindows(int t) {
  uint64_t n = 2ull * DI_NTHR * DI_WLEN;
  if (t == T_SIN || t == T_COS) n += 2ull * (DI_KPI4 + 1u) * DI_WLEN;
  return n;
}

/* unary fp32 input i of test t */
DI_HD uint32_t di_unary(int t, uint64_t i, int log2n) {
  const uint64_t ns = di_nstride(log2n);
  if (t == T_I2F || i < ns) return (uint32_t)i * DI_STRIDE; /* T_I2F: int32 patterns, strided only */
  i -= ns;
  if (i < DI_NEDGE) return di_edge((uint32_t)i);
  i -= DI_NEDGE;
  const uint32_t sign = (uint32_t)(i & 1u) << 31;
  i >>= 1;
  const uint32_t d = (uint32_t)(i % DI_WLEN);
  const uint64_t w = i / DI_WLEN;
  uint32_t c;
  if (w < DI_NTHR) {
    c = di_threshold((uint32_t)w);
  } else {
    const double kpi4 = (double)(w - DI_NTHR) * 0.78539816339744830962; /* one rounding, then one more to fp32 */
    c = di_f2u((float)kpi4);
  }
  if (c < DI_WIN) c = DI_WIN; /* k = 0: the window starts at +0 */
  return sign | (c - DI_WIN + d);
}
DI_HD uint64_t di_count_unary(int t, int log2n) {
  if (t == T_I2F) return di_nstride(log2n);
  return di_nstride(log2n) + DI_NEDGE + di_nwindows(t);
}

/* binary fp32 input pair i of test t (T_ATAN2: y, x; T_DIV: a, b) */
DI_HD void di_binary(int t, uint64_t i, uint32_t* a, uint32_t* b) {
  const uint64_t nmain = (t == T_ATAN2) ? (uint64_t)DI_GRID * DI_GRID : (uint64_t)DI_NRAND;
  if (i < nmain) {
    if (t == T_ATAN2) {
      *a = (uint32_t)(i / DI_GRID) * DI_STRIDE;
      *b = (uint32_t)(i % DI_GRID) * DI_STRIDE2;
    } else {
      const uint64_t h = di_mix(i);
      *a = (uint32_t)h;
      *b = (uint32_t)(h >> 32);
    }
    return;
  }
  i -= nmain;
  *a = di_edge((uint32_t)(i / DI_NEDGE));
  *b = di_edge((uint32_t)(i % DI_NEDGE));
}
DI_HD uint64_t di_count_binary(int t) {
  return ((t == T_ATAN2) ? (uint64_t)DI_GRID * DI_GRID : (uint64_t)DI_NRAND) + DI_NEDGE * DI_NEDGE;
}

DI_HD void di_ternary(uint64_t i, uint32_t* a, uint32_t* b, uint32_t* c) {
  if (i < DI_NRAND) {
    const uint64_t h = di_mix(i), g = di_mix(i ^ 0x5555555555555555ull);
    *a = (uint32_t)h;
    *b = (uint32_t)(h >> 32);
    *c = (uint32_t)g;
    return;
  }
  i -= DI_NRAND;
  *a = di_edge((uint32_t)(i / (DI_NEDGE * DI_NEDGE)));
  *b = di_edge((uint32_t)(i / DI_NEDGE % DI_NEDGE));
  *c = di_edge((uint32_t)(i % DI_NEDGE));
}
DI_HD uint64_t di_count_ternary(void) { return DI_NRAND + DI_NEDGE * DI_NEDGE * DI_NEDGE; }

/* fp64 sin / cos inputs */
#define DI_D_STRIDED (1ull << 24)
#define DI_D_KLOW 8192u   /* every k*pi/4 up to k = 8191 ... */
#define DI_D_KSTEP 166880u /* ... then 8192 k spread up to 2^30 * 4/pi */
#define DI_D_WIN 256u
#define DI_D_WLEN (2u * DI_D_WIN + 1u)
#define DI_D_TINY (1ull << 20)
#define DI_D_CUT 4096u
#define DI_D_NEDGE 10u
#define DI_D_TWO30 0x41D0000000000000ull
DI_HD uint64_t di_count_double(void) {
  return DI_D_STRIDED + 2ull * 2u * DI_D_KLOW * DI_D_WLEN + DI_D_TINY + 2ull * (2u * DI_D_CUT + 1u) + DI_D_NEDGE;
}
DI_HD uint64_t di_double(uint64_t i) {
  if (i < DI_D_STRIDED) { /* |x| <= 2^30, both signs */
    const uint64_t m = (i * 0x9E3779B97F4A7C15ull) % (DI_D_TWO30 + 1u);
    return ((i & 1u) << 63) | m;
  }
  i -= DI_D_STRIDED;
  if (i < 2ull * 2u * DI_D_KLOW * DI_D_WLEN) {
    const uint64_t sign = (i & 1u) << 63;
    i >>= 1;
    const uint64_t d = i % DI_D_WLEN, w = i / DI_D_WLEN;
    const uint64_t k = (w < DI_D_KLOW) ? w : DI_D_KLOW + (w - DI_D_KLOW) * DI_D_KSTEP;
    uint64_t c = di_d2u((double)k * 0.78539816339744830962);
    if (c < DI_D_WIN) c = DI_D_WIN;
    return sign | (c - DI_D_WIN + d);
  }
  i -= 2ull * 2u * DI_D_KLOW * DI_D_WLEN;
  if (i < DI_D_TINY) /* [0, 2^-20): subnormals and tiny normals, strided */
    return ((i & 1u) << 63) | ((i * 0x9E3779B97F4A7C15ull) % 0x3EB0000000000000ull);
  i -= DI_D_TINY;
  if (i < 2ull * (2u * DI_D_CUT + 1u)) return ((i & 1u) << 63) | (DI_D_TWO30 - DI_D_CUT + (i >> 1));
  i -= 2ull * (2u * DI_D_CUT + 1u);
  {
    const uint64_t e[DI_D_NEDGE] = {0x0ull,
                                    0x8000000000000000ull,
                                    0x1ull,
                                    0x8000000000000001ull,
                                    0x7fefffffffffffffull,
                                    0x7ff0000000000000ull,
                                    0xfff0000000000000ull,
                                    0x7ff8000000000000ull,
                                    0xfff8000000000123ull,
                                    0x7ff0000000000001ull};
    return e[i];
  }
}

/* one vector component: +0, -0, subnormal, huge (products overflow) or a normal in [2^-20, 2^20) of either sign */
DI_HD uint32_t di_vcomp(uint64_t i, uint32_t comp) {
  const uint64_t h = di_mix(i * 64u + comp);
  const uint32_t cls = (uint32_t)(h & 31u), sign = (uint32_t)(h >> 63) << 31, mant = (uint32_t)(h >> 8) & 0x7fffffu;
  if (cls == 0) return 0u;
  if (cls == 1) return 0x80000000u;
  if (cls == 2) return sign | (mant ? mant : 1u);
  if (cls == 3) return sign | ((200u + (uint32_t)(h >> 40) % 55u) << 23) | mant; /* 2^73 ... 2^127 */
  return sign | ((107u + (uint32_t)(h >> 40) % 40u) << 23) | mant;
}
/* a colour channel of pack_rgb: [0, 1] */
DI_HD uint32_t di_unit(uint64_t i, uint32_t comp) {
  return (uint32_t)(di_mix(i * 64u + comp) % 0x3f800001u);
}

/* inputs / outputs per vector test */
DI_HD int di_vec_nout(int t) {
  switch (t) {
    case T_DOT3: case T_LEN3: case T_PACK_RGB: case T_DEPTH24: return 1;
    case T_M4_MUL: return 16;
    default: return 3;
  }
}
DI_HD uint64_t di_count_vec(int t) { return (t == T_DEPTH24) ? 0x3f800001ull : (uint64_t)DI_NRAND; }

DI_HD uint64_t di_count(int t, int log2n) {
  if (t <= T_I2F) return di_count_unary(t, log2n);
  if (t <= T_DIV) return di_count_binary(t);
  if (t == T_FMA) return di_count_ternary();
  if (t <= T_COS_D) return di_count_double();
  return di_count_vec(t);
}
/* 32-bit output words per input */
DI_HD int di_nout(int t) {
  if (t <= T_FMA) return 1;
  if (t <= T_COS_D) return 2;
  return di_vec_nout(t);
}

#endif
