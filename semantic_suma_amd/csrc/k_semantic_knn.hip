/*
 * k_semantic_knn.hip -- RangeNet++'s k-nearest-neighbour label post-processing (Milioto et al., IROS 2019, section
 * III-D) for the semantic front end: the back-projection of k_semantic.hip with a vote among the points nearest in
 * range inside a window of the range image, so that a point hidden behind a nearer one does not take its pixel's class
 * (the class of a pole "bleeding" onto the wall behind it).  Opt-in: suma_semantic_unproject and the plain *_scores
 * entries stay what they are.
 *
 * Two passes: a lane per pixel reads the C score planes (coalesced) once and writes a compact record {range, class,
 * prob}; a lane per point gathers the S x S records around its pixel, selects K and votes.  The record image (12 bytes
 * a pixel: 1.5 MB at 64 x 2048) stays in L2 between the passes.
 *
 * ARITHMETIC SPECIFICATION (fp32, the rules of k_semantic.hip: -ffp-contract=off, include/suma_detmath.h, `/` and sqrt
 * correctly rounded).  tests/semantic_knn_shim.c restates it on the host, bit for bit.  Parameters: S = search (odd,
 * 1 .. 9), K = k (1 .. S^2), sigma (finite, > 0), cutoff (finite); R = (S - 1) / 2.
 *
 *  1. Ranges.  r_i = sqrt(fma(z, z, fma(y, y, x * x))) of point i, exactly ks_scatter's depth.  A pixel's range is its
 *     winner's r (proj_idx[p]; a winner index outside [0, n) counts as empty), +inf for an empty pixel.
 *  2. Pixel class.  ks_unproject's rule on pixel p's scores, softmax included in logits mode, with the class index in
 *     place of the label: cls = none, prob = 0; for j in class order: if (prob <= s_j) { cls = j; prob = s_j; }.
 *     All-negative or NaN scores leave cls = none.  Empty pixels get a class too (the network scores every pixel).
 *  3. Window.  Point i with pixel[i] = v * W + u (pixel < 0 or >= H * W: output (0, 0), as the plain path; so is a
 *     point whose own range r_i is not in (0, FLT_MAX] -- ks_scatter gives such a point no pixel, so this only meets a
 *     pixel array that was not made from these points; without it d would be NaN or inf in every slot); offsets
 *     dy, dx in [-R, R], window index t = (dy + R) * S + (dx + R), neighbour (v + dy, u + dx).  Outside the image:
 *     range 0.0f, class none; columns do not wrap (the published zero padding).  The centre t_c = (S * S - 1) / 2 has
 *     range r_i, but the pixel's class and prob.
 *  4. Weights, on the host in double: e[t] = exp(-(dx^2 + dy^2) / (2 sigma^2)), w[t] = (float)(1.0 - e[t] / sum_t e[t])
 *     (sum in t order).  The Gaussian's 1 / (2 pi sigma^2) cancels in the ratio and is not computed.
 *  5. Distance.  d[t] = fabsf(range[t] - r_i) * w[t]; the centre's d is exactly 0.
 *  6. Selection.  The K candidates with the smallest key (d, t != t_c, t), lexicographic: the centre first, ties to the
 *     lower window index (the published topk(sorted = False) is not deterministic).
 *  7. Vote.  A selected candidate votes for its class iff the class is not none, not index 0 ("unlabeled", dropped as
 *     in the published vote), and cutoff <= 0 or d <= cutoff.  The winner is the class with the most votes, equal counts
 *     to the lowest index.
 *  8. Output.  label = (float)label_map[winner]; prob = the largest prob(p) among the winner's voters, -0 below +0 (a
 *     total order: the result does not depend on the order the voters are visited in).  No vote: (0, 0) -- where the
 *     published code reports class 1, an artefact of its argmax over an all-zero row.
 *  search = 1 or k = 1 is the plain back-projection for every point whose pixel class is >= 1.
 *
 * Device form of 6 -- 8: d >= 0 and never NaN (range >= 0 or +inf, r_i finite by rule 3, w > 0 off the centre), so
 * bits(d) orders as d does.  The centre is taken first; the k - 1 others are found by k - 1 sweeps over the window, each taking the
 * smallest (bits(d), t) above the previous one.  The votes go into bit-sliced counters (bit j of plane b = bit b of class
 * j's count), and the winner is found by narrowing the voted classes plane by plane from the top: no register array is
 * indexed at run time, so nothing goes to scratch.  kk_points<5, 5> is the published default with S and K at compile
 * time; kk_points<S, 0> takes k at run time for every S.
 */
#include <float.h>
#include <math.h>

#include "suma_internal.h"

#define KNN_MAX_SEARCH 9
#define KNN_NONE 0xffffffffu /* record class of "no class wins" */

struct KnnArgs {
  int32_t W, H;
  uint32_t P, n, k;
  float cutoff;
  float w[KNN_MAX_SEARCH * KNN_MAX_SEARCH];
  float label[SUMA_SEM_MAX_CLASSES];
};

/* one lane per pixel: rule 1 (winner's range) and rule 2 (class, prob) -> range[p], cp[p] = {class, bits(prob)} */
__global__ void __launch_bounds__(256)
    kk_pixels(const float* __restrict__ scores, const int32_t* __restrict__ proj_idx, const float4* __restrict__ pts,
              uint32_t n, uint32_t P, uint32_t C, int logits, float* __restrict__ range, uint2* __restrict__ cp) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float s[SUMA_SEM_MAX_CLASSES];
#pragma unroll
  for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
    if (j < C) s[j] = scores[(size_t)j * P + p];
  const int32_t idx = proj_idx[p];
  float r = INFINITY;
  if (idx >= 0 && (uint32_t)idx < n) {
    const float4 pt = pts[(uint32_t)idx];
    r = sdm_sqrt(__builtin_fmaf(pt.z, pt.z, __builtin_fmaf(pt.y, pt.y, pt.x * pt.x)));
  }
  if (logits) {
    float m = -INFINITY;
#pragma unroll
    for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
      if (j < C) m = (s[j] > m) ? s[j] : m;
    float sum = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
      if (j < C) {
        s[j] = sdm_exp(s[j] - m);
        sum = sum + s[j];
      }
#pragma unroll
    for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
      if (j < C) s[j] = s[j] / sum;
  }
  uint32_t cls = KNN_NONE;
  float prob = 0.0f;
#pragma unroll
  for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
    if (j < C && prob <= s[j]) {
      cls = j;
      prob = s[j];
    }
  range[p] = r;
  cp[p] = make_uint2(cls, sdm_f2u(prob));
}

template <int K>
struct KnnBits {
  static constexpr int value = K <= 1 ? 1 : 1 + KnnBits<K / 2>::value;
};

/* the record of window slot t (runtime t) of the point at (v, u), pixel pix: out of the image -> none */
template <int S>
__device__ __forceinline__ uint2 knn_record(const uint2* __restrict__ cp, const KnnArgs& a, int32_t v, int32_t u,
                                            int32_t pix, int t) {
  constexpr int R = (S - 1) / 2;
  const int32_t yy = v + t / S - R, xx = u + t % S - R;
  const bool in = (uint32_t)yy < (uint32_t)a.H && (uint32_t)xx < (uint32_t)a.W;
  const uint2 rec = cp[in ? yy * a.W + xx : pix]; /* always an in-image address */
  return in ? rec : make_uint2(KNN_NONE, 0u);
}

/* bit-sliced vote: count[j] += 1 */
template <int NB>
__device__ __forceinline__ void knn_vote(uint32_t (&plane)[NB], uint32_t& voted, uint32_t j) {
  uint32_t carry = 1u << j;
  voted |= carry;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const uint32_t x = plane[b] ^ carry;
    carry &= plane[b];
    plane[b] = x;
  }
}

/* the voted class with the most votes, the lowest index on equal counts (voted != 0) */
template <int NB>
__device__ __forceinline__ uint32_t knn_winner(const uint32_t (&plane)[NB], uint32_t voted) {
  uint32_t cand = voted;
#pragma unroll
  for (int b = NB - 1; b >= 0; --b) {
    const uint32_t x = cand & plane[b];
    cand = x ? x : cand;
  }
  return (uint32_t)__builtin_ctz(cand);
}

__device__ __forceinline__ bool knn_votes(uint32_t cls, float d, float cutoff) {
  return cls != KNN_NONE && cls != 0u && (cutoff <= 0.0f || d <= cutoff);
}

/* one lane per point: rules 3 - 8.  KC > 0: k = KC at compile time (the selected slots stay in registers); KC = 0: a.k */
template <int S, int KC>
__global__ void __launch_bounds__(256)
    kk_points(const float4* __restrict__ pts, const int32_t* __restrict__ pixel, const float* __restrict__ range,
              const uint2* __restrict__ cp, KnnArgs a, float* __restrict__ labels, float* __restrict__ probs) {
  constexpr int R = (S - 1) / 2, S2 = S * S, TC = (S2 - 1) / 2;
  constexpr int NB = KC > 0 ? KnnBits<KC>::value : KnnBits<S2>::value; /* bits of the largest count */
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int32_t pix = pixel[i];
  float label = 0.0f, prob = 0.0f;
  if (pix >= 0 && (uint32_t)pix < a.P) {
    const float4 pt = pts[i];
    const float ri = sdm_sqrt(__builtin_fmaf(pt.z, pt.z, __builtin_fmaf(pt.y, pt.y, pt.x * pt.x)));
    if (!(ri > 0.0f && ri <= FLT_MAX)) { /* rule 3: a pixel from another scan's projection; also keeps d free of NaN */
      labels[i] = 0.0f;
      probs[i] = 0.0f;
      return;
    }
    const int32_t v = pix / a.W, u = pix - v * a.W;
    uint32_t d[S2]; /* bits of d[t]; the centre's is never read */
#pragma unroll
    for (int t = 0; t < S2; ++t) {
      if (t == TC) continue;
      const int32_t yy = v + t / S - R, xx = u + t % S - R;
      const bool in = (uint32_t)yy < (uint32_t)a.H && (uint32_t)xx < (uint32_t)a.W;
      const float rt = range[in ? yy * a.W + xx : pix];
      d[t] = sdm_f2u(fabsf((in ? rt : 0.0f) - ri) * a.w[t]);
    }
    const uint2 centre = cp[pix];

    /* selection: after sweep q, (thr_d, thr_t) is the q-th smallest non-centre key */
    uint32_t thr_d = 0u;
    int thr_t = -1;
    auto sweep = [&]() {
      uint32_t bd = 0xffffffffu; /* above every bits(d) */
      int bt = S2;
#pragma unroll
      for (int t = 0; t < S2; ++t) {
        if (t == TC) continue;
        const bool above = d[t] > thr_d || (d[t] == thr_d && t > thr_t);
        if (above && d[t] < bd) { /* strictly: an equal d later in t order loses */
          bd = d[t];
          bt = t;
        }
      }
      thr_d = bd;
      thr_t = bt;
    };

    uint32_t plane[NB] = {};
    uint32_t voted = 0u;
    if constexpr (KC > 0) {
      int sel_t[KC];
      uint32_t sel_d[KC], cls[KC], pbits[KC];
      sel_d[0] = 0u;
#pragma unroll
      for (int q = 1; q < KC; ++q) {
        sweep();
        sel_t[q] = thr_t;
        sel_d[q] = thr_d;
      }
      cls[0] = centre.x;
      pbits[0] = centre.y;
#pragma unroll
      for (int q = 1; q < KC; ++q) {
        const uint2 rec = knn_record<S>(cp, a, v, u, pix, sel_t[q]);
        cls[q] = rec.x;
        pbits[q] = rec.y;
      }
#pragma unroll
      for (int q = 0; q < KC; ++q)
        if (knn_votes(cls[q], sdm_u2f(sel_d[q]), a.cutoff)) knn_vote<NB>(plane, voted, cls[q]);
      if (voted) {
        const uint32_t win = knn_winner<NB>(plane, voted);
        int32_t best = (int32_t)0x80000000u; /* -0.0f */
#pragma unroll
        for (int q = 0; q < KC; ++q)
          if (cls[q] == win && knn_votes(cls[q], sdm_u2f(sel_d[q]), a.cutoff) && (int32_t)pbits[q] > best)
            best = (int32_t)pbits[q];
        prob = sdm_u2f((uint32_t)best);
#pragma unroll
        for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
          if (j == win) label = a.label[j];
      }
    } else {
      /* run-time k: the selected set is the centre and every slot whose key is at most (thr_d, thr_t); its records are
       * read in window order, once to vote and once more for the winner's prob */
      for (uint32_t q = 1; q < a.k; ++q) sweep();
      if (knn_votes(centre.x, 0.0f, a.cutoff)) knn_vote<NB>(plane, voted, centre.x);
      uint32_t voters[(S2 + 31) / 32] = {}; /* bit t: slot t voted (kept in a VGPR, not as S2 lane masks) */
#pragma unroll
      for (int t = 0; t < S2; ++t) {
        if (t == TC) continue;
        if (d[t] < thr_d || (d[t] == thr_d && t <= thr_t)) {
          const uint2 rec = knn_record<S>(cp, a, v, u, pix, t);
          if (knn_votes(rec.x, sdm_u2f(d[t]), a.cutoff)) {
            knn_vote<NB>(plane, voted, rec.x);
            voters[t / 32] |= 1u << (t % 32);
          }
        }
      }
      if (voted) {
        const uint32_t win = knn_winner<NB>(plane, voted);
        int32_t best = (int32_t)0x80000000u;
        if (centre.x == win) best = (int32_t)centre.y; /* the centre's d is 0: it passes every cutoff */
#pragma unroll
        for (int t = 0; t < S2; ++t) {
          if (t == TC) continue;
          if (voters[t / 32] & (1u << (t % 32))) {
            const uint2 rec = knn_record<S>(cp, a, v, u, pix, t);
            if (rec.x == win && (int32_t)rec.y > best) best = (int32_t)rec.y;
          }
        }
        prob = sdm_u2f((uint32_t)best);
#pragma unroll
        for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
          if (j == win) label = a.label[j];
      }
    }
  }
  labels[i] = label;
  probs[i] = prob;
}

/* ---- host side ---- */
static int knn_check(suma_ctx* c, const suma_semantic_knn* kp) {
  if (!kp) return fail(c, SUMA_ERR_INVALID, "suma_semantic_knn: NULL");
  if (kp->search < 1 || kp->search > KNN_MAX_SEARCH || kp->search % 2 == 0)
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_knn: search = " + std::to_string(kp->search) +
                                     " (must be odd, 1 .. " + std::to_string(KNN_MAX_SEARCH) + ")");
  if (kp->k < 1 || kp->k > kp->search * kp->search)
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_knn: k = " + std::to_string(kp->k) + " (must be 1 .. search^2 = " +
                                     std::to_string(kp->search * kp->search) + ")");
  if (!(kp->sigma > 0.0f) || !std::isfinite(kp->sigma))
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_knn: sigma must be finite and > 0");
  if (!std::isfinite(kp->cutoff)) return fail(c, SUMA_ERR_INVALID, "suma_semantic_knn: cutoff must be finite");
  return SUMA_OK;
}

/* the record image of one stream's passes: cp (P x 8 bytes) then range (P x 4 bytes) in one block; every earlier pass
 * that used the block ran on st */
static int knn_reserve(suma_ctx* c, DevBuf<char>& sc, uint32_t P, hipStream_t st) {
  return grow(c, sc, (size_t)P * 12, {st}) < 0 ? SUMA_ERR_HIP : SUMA_OK;
}

static hipError_t launch_semantic_unproject_knn(suma_ctx* c, hipStream_t st, char* sc,
                                                const suma_semantic_params* sp, const suma_semantic_knn* kp,
                                                const suma_float4* d_points, const float* d_scores, int logits,
                                                const int32_t* d_pixel, const int32_t* d_proj_idx, uint32_t n,
                                                float* d_labels, float* d_probs) {
  const uint32_t P = sp->width * sp->height, C = sp->n_classes, S = kp->search;
  KnnArgs a;
  a.W = (int32_t)sp->width;
  a.H = (int32_t)sp->height;
  a.P = P;
  a.n = n;
  a.k = kp->k;
  a.cutoff = kp->cutoff;
  /* rule 4 */
  const int R = (int)(S - 1) / 2;
  const double sig = (double)kp->sigma;
  double e[KNN_MAX_SEARCH * KNN_MAX_SEARCH], sum = 0.0;
  for (uint32_t t = 0; t < S * S; ++t) {
    const int dy = (int)(t / S) - R, dx = (int)(t % S) - R;
    e[t] = std::exp(-(double)(dx * dx + dy * dy) / (2.0 * sig * sig));
    sum += e[t];
  }
  for (uint32_t t = 0; t < KNN_MAX_SEARCH * KNN_MAX_SEARCH; ++t) a.w[t] = t < S * S ? (float)(1.0 - e[t] / sum) : 0.0f;
  for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j) a.label[j] = j < C ? (float)sp->label_map[j] : 0.0f;
  if (n == 0) return hipGetLastError();
  uint2* cp = (uint2*)sc;
  float* range = (float*)(cp + P);
  {
    ProfScope ps(c, "semantic_knn_pixels", (16.0 + 4.0 * C) * P + 16.0 * n);
    kk_pixels<<<(P + 255) / 256, 256, 0, st>>>(d_scores, d_proj_idx, (const float4*)d_points, n, P, C, logits ? 1 : 0,
                                               range, cp);
  }
  ProfScope ps(c, "semantic_knn_points", (28.0 + 4.0 * (S * S - 1) + 8.0 * kp->k) * n);
  const dim3 grid((n + 255) / 256), block(256);
  const float4* pts = (const float4*)d_points;
  if (S == 5 && kp->k == 5)
    kk_points<5, 5><<<grid, block, 0, st>>>(pts, d_pixel, range, cp, a, d_labels, d_probs);
  else if (S == 1)
    kk_points<1, 0><<<grid, block, 0, st>>>(pts, d_pixel, range, cp, a, d_labels, d_probs);
  else if (S == 3)
    kk_points<3, 0><<<grid, block, 0, st>>>(pts, d_pixel, range, cp, a, d_labels, d_probs);
  else if (S == 5)
    kk_points<5, 0><<<grid, block, 0, st>>>(pts, d_pixel, range, cp, a, d_labels, d_probs);
  else if (S == 7)
    kk_points<7, 0><<<grid, block, 0, st>>>(pts, d_pixel, range, cp, a, d_labels, d_probs);
  else
    kk_points<9, 0><<<grid, block, 0, st>>>(pts, d_pixel, range, cp, a, d_labels, d_probs);
  return hipGetLastError();
}

static int knn_args_check(suma_ctx* c, const suma_semantic_params* sp, const suma_semantic_knn* kp, const char* who,
                          const void* d_points, const float* d_scores, const int32_t* d_pixel,
                          const int32_t* d_proj_idx, uint32_t n) {
  int r = semantic_check(c, sp);
  if (r) return r;
  r = knn_check(c, kp);
  if (r) return r;
  if (n > 0 && (!d_points || !d_scores || !d_pixel || !d_proj_idx))
    return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL buffer");
  return SUMA_OK;
}

/* scratch: this entry's record image (sem_knn[0]) is only used on the ctx stream, the pipeline's (sem_knn[1]) only on
 * the pipeline's input stream, so the two never wait for each other and each is reused in its own stream's order */
extern "C" int suma_semantic_unproject_knn(suma_ctx* c, const suma_semantic_params* sp, const suma_semantic_knn* knn,
                                           const suma_float4* d_points, const float* d_scores, int scores_are_logits,
                                           const int32_t* d_pixel, const int32_t* d_proj_idx, uint32_t n,
                                           float* d_labels, float* d_probs) {
  if (!c) return SUMA_ERR_INVALID;
  int r = knn_args_check(c, sp, knn, "suma_semantic_unproject_knn", d_points, d_scores, d_pixel, d_proj_idx, n);
  if (r) return r;
  if (n > 0 && (!d_labels || !d_probs)) return fail(c, SUMA_ERR_INVALID, "suma_semantic_unproject_knn: NULL buffer");
  if (n > 0) {
    r = knn_reserve(c, c->sem_knn[0], sp->width * sp->height, c->stream);
    if (r) return r;
  }
  HIP_TRY(c, launch_semantic_unproject_knn(c, c->stream, c->sem_knn[0], sp, knn, d_points, d_scores, scores_are_logits,
                                           d_pixel, d_proj_idx, n, d_labels, d_probs));
  return SUMA_OK;
}

/* suma_pipeline_begin_scan_scores with the KNN back-projection in front */
extern "C" int suma_pipeline_begin_scan_scores_knn(suma_pipeline* s, const suma_semantic_params* sp,
                                                   const suma_semantic_knn* knn, const suma_float4* d_points,
                                                   const float* d_scores, int scores_are_logits, const int32_t* d_pixel,
                                                   const int32_t* d_proj_idx, uint32_t n, void* producer_event) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  int r = knn_args_check(c, sp, knn, "suma_pipeline_begin_scan_scores_knn", d_points, d_scores, d_pixel, d_proj_idx, n);
  if (r) return r;
  hipStream_t st;
  r = semantic_scan_input(s, n, producer_event, &st);
  if (r) return r;
  if (n > 0) {
    r = knn_reserve(c, c->sem_knn[1], sp->width * sp->height, st);
    if (r) return r;
  }
  HIP_TRY(c, launch_semantic_unproject_knn(c, st, c->sem_knn[1], sp, knn, d_points, d_scores, scores_are_logits,
                                           d_pixel, d_proj_idx, n, c->sem_labels, c->sem_probs));
  /* K1-K3 follow on the same stream, exactly as suma_pipeline_begin_scan_device runs them */
  return pipeline_begin_scan_impl(s, d_points, c->sem_labels, c->sem_probs, n, nullptr);
}

extern "C" int suma_pipeline_process_scan_scores_knn(suma_pipeline* s, const suma_semantic_params* sp,
                                                     const suma_semantic_knn* knn, const suma_float4* d_points,
                                                     const float* d_scores, int scores_are_logits,
                                                     const int32_t* d_pixel, const int32_t* d_proj_idx, uint32_t n,
                                                     void* producer_event, int32_t fixed_iterations) {
  int r = suma_pipeline_begin_scan_scores_knn(s, sp, knn, d_points, d_scores, scores_are_logits, d_pixel, d_proj_idx, n,
                                              producer_event);
  return pipeline_finish_scan(s, r, fixed_iterations, false);
}
