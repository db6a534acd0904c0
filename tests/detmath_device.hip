// tests/detmath_device.hip -- device side of tests/test_gpu_detmath.py.
//
// Evaluates include/suma_detmath.h, the IEEE primitives it relies on and the helpers of csrc/dev_math.h on the gfx950
// for the input sets of tests/detmath_inputs.h, and compares every output bit with the gcc-built host side
// (tests/detmath_shim.c, dm_check).  Built by the test with the library's own CXXFLAGS.  Prints one JSON line per
// function:  {"fn", "n", "mismatch", "mismatch_not_nan", "first": [[inputs..., host..., device...] as hex], "s"}.
//
//   detmath_device <log2 strided fp32 patterns per unary function> [function names...]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../semantic_suma_amd/csrc/dev_math.h"
#include "detmath_inputs.h"

extern "C" {
int dm_inputs(int t, uint64_t i, int log2n, uint32_t* in);
void dm_eval(int t, uint64_t i, int log2n, uint32_t* o);
uint64_t dm_check(int t, int log2n, uint64_t base, uint64_t n, const uint32_t* dev, uint64_t* nonnan, uint64_t* first,
                  uint64_t* first_nonnan);
}

static const char* const kNames[T_COUNT] = {
    "atan", "asin", "acos", "sin", "cos", "exp", "log", "floor", "round", "sqrt", "rint", "f2i", "i2f", "atan2", "div",
    "fma", "sin_d", "cos_d", "dot3", "len3", "normalize3", "cross3", "divs3", "m4_point", "m4_dir", "m4_mul",
    "pack_rgb", "depth24"};

#define CHECK(x)                                                                            \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) {                                                                 \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
      exit(2);                                                                              \
    }                                                                                       \
  } while (0)

__device__ __forceinline__ float fw(uint32_t u) { return sdm_u2f(u); }
__device__ __forceinline__ void put3(uint32_t* o, v3 v) {
  o[0] = sdm_f2u(v.x);
  o[1] = sdm_f2u(v.y);
  o[2] = sdm_f2u(v.z);
}

// the device restatement of dm_eval (tests/detmath_shim.c): same inputs, the kernels' own headers
__device__ void eval(int t, uint64_t i, int log2n, uint32_t* o) {
  if (t <= T_I2F) {
    const uint32_t u = di_unary(t, i, log2n);
    const float x = fw(u);
    float r = 0.0f;
    switch (t) {
      case T_ATAN: r = sdm_atan(x); break;
      case T_ASIN: r = sdm_asin(x); break;
      case T_ACOS: r = sdm_acos(x); break;
      case T_SIN: r = sdm_sin(x); break;
      case T_COS: r = sdm_cos(x); break;
      case T_EXP: r = sdm_exp(x); break;
      case T_LOG: r = sdm_log(x); break;
      case T_FLOOR: r = sdm_floor(x); break;
      case T_ROUND: r = sdm_round(x); break;
      case T_SQRT: r = sdm_sqrt(x); break;
      case T_RINT: r = __builtin_rintf(x); break;
      case T_F2I: o[0] = (sdm_abs(x) < 2147483648.0f) ? (uint32_t)(int32_t)x : 0xdeadbeefu; return;
      default: r = (float)(int32_t)u; break; /* T_I2F */
    }
    o[0] = sdm_f2u(r);
    return;
  }
  if (t <= T_DIV) {
    uint32_t a, b;
    di_binary(t, i, &a, &b);
    o[0] = sdm_f2u(t == T_ATAN2 ? sdm_atan2(fw(a), fw(b)) : fw(a) / fw(b));
    return;
  }
  if (t == T_FMA) {
    uint32_t a, b, c;
    di_ternary(i, &a, &b, &c);
    o[0] = sdm_f2u(__builtin_fmaf(fw(a), fw(b), fw(c)));
    return;
  }
  if (t <= T_COS_D) {
    const uint64_t u = di_double(i);
    double d;
    __builtin_memcpy(&d, &u, 8);
    d = (t == T_SIN_D) ? sdm_sin_d(d) : sdm_cos_d(d);
    uint64_t r;
    __builtin_memcpy(&r, &d, 8);
    o[0] = (uint32_t)r;
    o[1] = (uint32_t)(r >> 32);
    return;
  }
  if (t == T_PACK_RGB) {
    o[0] = sdm_f2u(pack_rgb(fw(di_unit(i, 0)), fw(di_unit(i, 1)), fw(di_unit(i, 2))));
    return;
  }
  if (t == T_DEPTH24) {
    o[0] = depth24(fw((uint32_t)i));
    return;
  }
  float f[32];
  const int n = (t == T_M4_POINT || t == T_M4_DIR) ? 19 : (t == T_M4_MUL) ? 32 : 6;
  for (int k = 0; k < n; ++k) f[k] = fw(di_vcomp(i, (uint32_t)k));
  const v3 a = mk3(f[0], f[1], f[2]), b = mk3(f[3], f[4], f[5]);
  switch (t) {
    case T_DOT3: o[0] = sdm_f2u(dot3(a, b)); break;
    case T_LEN3: o[0] = sdm_f2u(len3(a)); break;
    case T_NORMALIZE3: put3(o, normalize3(a)); break;
    case T_CROSS3: put3(o, cross3(a, b)); break;
    case T_DIVS3: put3(o, divs3(a, f[3])); break;
    case T_M4_POINT: put3(o, m4_point(f + 3, a)); break;
    case T_M4_DIR: put3(o, m4_dir(f + 3, a)); break;
    default: { /* T_M4_MUL */
      float c[16];
      m4_mul(f, f + 16, c);
      for (int k = 0; k < 16; ++k) o[k] = sdm_f2u(c[k]);
    }
  }
}

// cases [base, base + n) of test t; out holds nout words per case
__global__ void __launch_bounds__(256) k_eval(int t, int log2n, int nout, uint64_t base, uint32_t n, uint32_t* out) {
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
    uint32_t o[16];
    eval(t, base + j, log2n, o);
    for (int k = 0; k < nout; ++k) out[(size_t)j * nout + k] = o[k];
  }
}

static void hex_list(const uint32_t* w, int n, int words_per_value) {
  // a double is printed as one 16-digit value (high word first)
  for (int k = 0; k < n; k += words_per_value) {
    if (k) printf(", ");
    if (words_per_value == 2)
      printf("\"%08x%08x\"", w[k + 1], w[k]);
    else
      printf("\"%08x\"", w[k]);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s log2n [function ...]\n", argv[0]);
    return 2;
  }
  const int log2n = atoi(argv[1]);
  if (log2n < 10 || log2n > 32) {
    fprintf(stderr, "log2n must be in [10, 32]\n");
    return 2;
  }
  bool want[T_COUNT];
  for (int t = 0; t < T_COUNT; ++t) want[t] = (argc == 2);
  for (int a = 2; a < argc; ++a) {
    int t = 0;
    while (t < T_COUNT && strcmp(argv[a], kNames[t]) != 0) ++t;
    if (t == T_COUNT) {
      fprintf(stderr, "unknown function %s\n", argv[a]);
      return 2;
    }
    want[t] = true;
  }

  const size_t kWords = (size_t)1 << 25; /* per buffer: 128 MiB */
  uint32_t *dbuf[2], *hbuf[2];
  hipStream_t s;
  hipEvent_t done[2];
  CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    CHECK(hipMalloc(&dbuf[b], kWords * 4));
    CHECK(hipHostMalloc(&hbuf[b], kWords * 4, hipHostMallocDefault));
    CHECK(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
  }

  for (int t = 0; t < T_COUNT; ++t) {
    if (!want[t]) continue;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = di_count(t, log2n);
    const int nout = di_nout(t);
    const uint64_t chunk = kWords / (size_t)nout;
    const uint64_t nchunks = (n + chunk - 1) / chunk;
    uint64_t mism = 0, mism_nonnan = 0, first[4], first_nonnan[4], best[4], best_nonnan[4];
    for (int k = 0; k < 4; ++k) best[k] = best_nonnan[k] = UINT64_MAX;
    // chunk c runs on the device into buffer c & 1 while the host checks chunk c - 1
    for (uint64_t c = 0; c <= nchunks; ++c) {
      if (c < nchunks) {
        const int b = (int)(c & 1);
        const uint64_t base = c * chunk;
        const uint32_t m = (uint32_t)((n - base < chunk) ? n - base : chunk);
        const uint32_t blocks = (m + 255u) / 256u < 16384u ? (m + 255u) / 256u : 16384u;
        hipLaunchKernelGGL(k_eval, dim3(blocks), dim3(256), 0, s, t, log2n, nout, base, m, dbuf[b]);
        CHECK(hipGetLastError());
        CHECK(hipMemcpyAsync(hbuf[b], dbuf[b], (size_t)m * nout * 4, hipMemcpyDeviceToHost, s));
        CHECK(hipEventRecord(done[b], s));
      }
      if (c > 0) {
        const uint64_t p = c - 1;
        const int b = (int)(p & 1);
        const uint64_t base = p * chunk, m = (n - base < chunk) ? n - base : chunk;
        CHECK(hipEventSynchronize(done[b]));
        uint64_t nn = 0;
        mism += dm_check(t, log2n, base, m, hbuf[b], &nn, first, first_nonnan);
        mism_nonnan += nn;
        for (int k = 0; k < 4; ++k) { /* chunks are ascending: keep the earliest found */
          for (int q = 0; q < 4 && first[k] != UINT64_MAX; ++q)
            if (best[q] == UINT64_MAX) { best[q] = first[k]; break; }
          for (int q = 0; q < 4 && first_nonnan[k] != UINT64_MAX; ++q)
            if (best_nonnan[q] == UINT64_MAX) { best_nonnan[q] = first_nonnan[k]; break; }
        }
      }
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // the reported examples: value mismatches first, then NaN-payload-only ones
    uint64_t show[4];
    int nshow = 0;
    for (int k = 0; k < 4 && best_nonnan[k] != UINT64_MAX; ++k) show[nshow++] = best_nonnan[k];
    for (int k = 0; k < 4 && nshow < 4 && best[k] != UINT64_MAX; ++k) {
      bool seen = false;
      for (int q = 0; q < nshow; ++q) seen |= show[q] == best[k];
      if (!seen) show[nshow++] = best[k];
    }
    printf("{\"fn\": \"%s\", \"n\": %llu, \"mismatch\": %llu, \"mismatch_not_nan\": %llu, \"first\": [", kNames[t],
           (unsigned long long)n, (unsigned long long)mism, (unsigned long long)mism_nonnan);
    const int wpv = (t == T_SIN_D || t == T_COS_D) ? 2 : 1;
    for (int q = 0; q < nshow; ++q) {
      uint32_t in[32], h[16], d[16];
      const int nin = dm_inputs(t, show[q], log2n, in);
      dm_eval(t, show[q], log2n, h);
      uint32_t* dd;
      CHECK(hipMalloc(&dd, 16 * 4));
      hipLaunchKernelGGL(k_eval, dim3(1), dim3(256), 0, s, t, log2n, nout, show[q], 1u, dd);
      CHECK(hipGetLastError());
      CHECK(hipMemcpyAsync(d, dd, (size_t)nout * 4, hipMemcpyDeviceToHost, s));
      CHECK(hipStreamSynchronize(s));
      CHECK(hipFree(dd));
      printf("%s{\"in\": [", q ? ", " : "");
      hex_list(in, nin, wpv);
      printf("], \"host\": [");
      hex_list(h, nout, wpv);
      printf("], \"dev\": [");
      hex_list(d, nout, wpv);
      printf("]}");
    }
    printf("], \"s\": %.3f}\n", sec);
    fflush(stdout);
  }
  for (int b = 0; b < 2; ++b) {
    CHECK(hipFree(dbuf[b]));
    CHECK(hipHostFree(hbuf[b]));
    CHECK(hipEventDestroy(done[b]));
  }
  CHECK(hipStreamDestroy(s));
  return 0;
}
