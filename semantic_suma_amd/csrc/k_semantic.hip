/*
 * k_semantic.hip -- the semantic front end: range-image projection for a segmentation network and the back-projection
 * of its class scores to per-point labels, plus the scan-pipeline entry that takes the scores.
 *
 * Replaces (reference, citations relative to the reference tree):
 *   src/io/KITTIReader.cpp:172-200  RangenetAPI::infer (TensorRT: projection, network, un-projection) and the argmax
 *                                   over its N x 20 scores.  The network itself is the caller's (a PyTorch model on
 *                                   the same device); the two data-parallel stages around it are here.
 *
 * ARITHMETIC SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; transcendentals from
 * include/suma_detmath.h; `/` and sqrt correctly rounded).  tests/semantic_shim.c restates it on the host, bit for bit.
 *
 * Host constants, computed once in double and rounded once to float:
 *   pi_f = (float)pi, fdown = (float)(|fov_down| * pi / 180), fov = (float)((|fov_up| + |fov_down|) * pi / 180),
 *   inv_std_c = (float)(1.0 / std_c), Wf = (float)W, Hf = (float)H.
 *
 * Projection, point i = (x, y, z, r):
 *   depth = sqrt(fma(z, z, fma(y, y, x * x)))
 *   projected iff depth > 0 and depth <= FLT_MAX      (a NaN / inf coordinate or an overflowing range is not)
 *     The squares are fp32: with every |coordinate| below 2^-75 (about 2.6e-23) each square rounds to 0 and depth is 0;
 *     with one of 2^64 (about 1.8e19) or more its square is inf and so is depth.  Such a point is NOT projected although
 *     its true range is a finite fp32 number.  Between 2^-75 and 2^-60 the largest square is subnormal and depth carries
 *     few bits; between 2^60 and 2^64 the sum may overflow.  No lidar returns such coordinates; nothing rescales.
 *   yaw   = -sdm_atan2(y, x)
 *   pitch = sdm_asin(z / depth)
 *   fu = sdm_floor((0.5f * (yaw / pi_f + 1.0f)) * Wf)
 *   fv = sdm_floor((1.0f - (pitch + fdown) / fov) * Hf)
 *   clamp (RangeNet++ clamps, it does not clip): f = (f >= 0) ? f : 0;  u = (fu < Wf) ? (int)fu : W - 1, same for v
 *   pixel = v * W + u.  Row 0 is the TOP of the image (highest pitch): the OPPOSITE of the frames' vertex maps, whose
 *   row 0 is the lowest beam (k_preprocess.hip) -- the network's convention, not ours.
 *   z-buffer key = (bits(depth) << 32) | i; the smallest key wins (positive floats order as unsigned integers, so the
 *   nearest point wins and equal ranges go to the lower index).
 * Resolve, pixel p with winner i:  input[c][p] = (v_c - mean_c) * inv_std_c for v = (depth, x, y, z, r), depth the
 *   value of the key; an empty pixel is 0 in every channel.
 *
 * Back-projection, point i with pixel p (p < 0 or p >= H * W: not projected -> label 0, prob 0):
 *   s_j = scores[j * H * W + p], j = 0 .. C-1 (all C loads issued before any compare)
 *   logits: m = -inf; m = (s_j > m) ? s_j : m (class order);  e_j = sdm_exp(s_j - m);  sum = ((e_0 + e_1) + ...) + e_C-1
 *           (from 0.0f, class order);  s_j = e_j / sum
 *   label = 0, prob = 0; for j in class order: if (prob <= s_j) { label = (float)label_map[j]; prob = s_j; }
 *   (KITTIReader.cpp:189-200 literally: the last maximum wins, all-negative scores give (0, 0), a NaN never wins --
 *   and in logits mode one NaN logit makes every probability NaN, so such a point gets (0, 0) too).
 */
#include <float.h>
#include <math.h>

#include "suma_internal.h"

struct SemProj {
  int32_t W, H;
  uint32_t P;
  float Wf, Hf, pi, fdown, fov;
  float mean[SUMA_SEM_CHANNELS], inv_std[SUMA_SEM_CHANNELS];
};
struct SemMap {
  float label[SUMA_SEM_MAX_CLASSES];
};

__global__ void __launch_bounds__(256)
    ks_scatter(const float4* __restrict__ pts, uint32_t n, SemProj q, unsigned long long* __restrict__ zbuf,
               int32_t* __restrict__ pixel) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 pt = pts[i];
  const float depth = sdm_sqrt(__builtin_fmaf(pt.z, pt.z, __builtin_fmaf(pt.y, pt.y, pt.x * pt.x)));
  int32_t pix = -1;
  if (depth > 0.0f && depth <= FLT_MAX) {
    const float yaw = -sdm_atan2(pt.y, pt.x);
    const float pitch = sdm_asin(pt.z / depth);
    float fu = sdm_floor((0.5f * (yaw / q.pi + 1.0f)) * q.Wf);
    float fv = sdm_floor((1.0f - (pitch + q.fdown) / q.fov) * q.Hf);
    fu = (fu >= 0.0f) ? fu : 0.0f; /* also NaN -> 0 */
    fv = (fv >= 0.0f) ? fv : 0.0f;
    const int32_t u = (fu < q.Wf) ? (int32_t)fu : q.W - 1;
    const int32_t v = (fv < q.Hf) ? (int32_t)fv : q.H - 1;
    pix = v * q.W + u; /* W, H <= 2^24 and W * H < 2^31 (semantic_check) */
    const unsigned long long key = ((unsigned long long)sdm_f2u(depth) << 32) | (unsigned long long)i;
    atomicMin(&zbuf[pix], key);
  }
  if (pixel) pixel[i] = pix;
}

/* one thread per pixel: five planar fp32 stores (coalesced per plane), re-arms the z-buffer (no clear launch) */
__global__ void __launch_bounds__(256)
    ks_resolve(unsigned long long* __restrict__ zbuf, const float4* __restrict__ pts, SemProj q,
               float* __restrict__ input, int32_t* __restrict__ proj_idx) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= q.P) return;
  const unsigned long long key = zbuf[p];
  zbuf[p] = SUMA_EMPTY_KEY;
  float o[SUMA_SEM_CHANNELS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  int32_t idx = -1;
  if (key != SUMA_EMPTY_KEY) {
    idx = (int32_t)(uint32_t)(key & 0xffffffffull);
    const float4 pt = pts[(uint32_t)idx];
    const float v[SUMA_SEM_CHANNELS] = {sdm_u2f((uint32_t)(key >> 32)), pt.x, pt.y, pt.z, pt.w};
#pragma unroll
    for (int ch = 0; ch < SUMA_SEM_CHANNELS; ++ch) o[ch] = (v[ch] - q.mean[ch]) * q.inv_std[ch];
  }
#pragma unroll
  for (int ch = 0; ch < SUMA_SEM_CHANNELS; ++ch) input[(size_t)ch * q.P + p] = o[ch];
  if (proj_idx) proj_idx[p] = idx;
}

__global__ void __launch_bounds__(256)
    ks_unproject(const float* __restrict__ scores, const int32_t* __restrict__ pixel, uint32_t n, uint32_t P,
                 uint32_t C, int logits, SemMap lm, float* __restrict__ labels, float* __restrict__ probs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t pix = pixel[i];
  float label = 0.0f, prob = 0.0f;
  if (pix >= 0 && (uint32_t)pix < P) {
    float s[SUMA_SEM_MAX_CLASSES];
#pragma unroll
    for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
      if (j < C) s[j] = scores[(size_t)j * P + (uint32_t)pix];
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
#pragma unroll
    for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j)
      if (j < C && prob <= s[j]) { /* KITTIReader.cpp:194: labels_prob[i] <= color_mask[i*20+j] */
        label = lm.label[j];
        prob = s[j];
      }
  }
  labels[i] = label;
  probs[i] = prob;
}

/* ---- host side ---- */
int semantic_check(suma_ctx* c, const suma_semantic_params* sp) {
  if (!sp) return fail(c, SUMA_ERR_INVALID, "suma_semantic_params: NULL");
  if (sp->n_classes == 0 || sp->n_classes > SUMA_SEM_MAX_CLASSES)
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_params: n_classes = " + std::to_string(sp->n_classes) +
                                     " (must be 1 .. " + std::to_string(SUMA_SEM_MAX_CLASSES) + ")");
  if (sp->width == 0 || sp->height == 0 || sp->width > (1u << 24) || sp->height > (1u << 24) ||
      (uint64_t)sp->width * sp->height > (uint64_t)INT32_MAX)
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_params: width x height = " + std::to_string(sp->width) + " x " +
                                     std::to_string(sp->height) + " is empty or overflows the int32 pixel index");
  for (int ch = 0; ch < SUMA_SEM_CHANNELS; ++ch) {
    if (!(sp->stds[ch] != 0.0f) || !std::isfinite(sp->stds[ch]) || !std::isfinite(sp->means[ch]))
      return fail(c, SUMA_ERR_INVALID, "suma_semantic_params: channel " + std::to_string(ch) +
                                       " needs a finite mean and a finite, non-zero std");
  }
  const double fov = (std::fabs((double)sp->fov_up) + std::fabs((double)sp->fov_down)) * M_PI / 180.0;
  if (!(fov > 0.0) || !std::isfinite(fov) || !((float)fov > 0.0f))
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_params: |fov_up| + |fov_down| must be finite and > 0");
  return SUMA_OK;
}

static SemProj sem_proj(const suma_semantic_params* sp) {
  SemProj q;
  q.W = (int32_t)sp->width;
  q.H = (int32_t)sp->height;
  q.P = sp->width * sp->height;
  q.Wf = (float)sp->width;
  q.Hf = (float)sp->height;
  q.pi = (float)M_PI;
  q.fdown = (float)(std::fabs((double)sp->fov_down) * M_PI / 180.0);
  q.fov = (float)((std::fabs((double)sp->fov_up) + std::fabs((double)sp->fov_down)) * M_PI / 180.0);
  for (int ch = 0; ch < SUMA_SEM_CHANNELS; ++ch) {
    q.mean[ch] = sp->means[ch];
    q.inv_std[ch] = (float)(1.0 / (double)sp->stds[ch]);
  }
  return q;
}

static hipError_t launch_semantic_unproject(suma_ctx* c, const suma_semantic_params* sp, const float* d_scores,
                                            int logits, const int32_t* d_pixel, uint32_t n, float* d_labels,
                                            float* d_probs) {
  SemMap lm;
  for (uint32_t j = 0; j < SUMA_SEM_MAX_CLASSES; ++j) lm.label[j] = j < sp->n_classes ? (float)sp->label_map[j] : 0.0f;
  const uint32_t P = sp->width * sp->height;
  ProfScope ps(c, "semantic_unproject", (12.0 + 4.0 * sp->n_classes) * n);
  if (n > 0)
    ks_unproject<<<(n + 255) / 256, 256, 0, c->ls>>>(d_scores, d_pixel, n, P, sp->n_classes, logits ? 1 : 0, lm,
                                                      d_labels, d_probs);
  return hipGetLastError();
}

extern "C" int suma_semantic_project(suma_ctx* c, const suma_semantic_params* sp, const suma_float4* d_points,
                                     uint32_t n, float* d_input, int32_t* d_pixel, int32_t* d_proj_idx) {
  if (!c) return SUMA_ERR_INVALID;
  int r = semantic_check(c, sp);
  if (r) return r;
  if (!d_input || (n > 0 && !d_points)) return fail(c, SUMA_ERR_INVALID, "suma_semantic_project: NULL buffer");
  if (n == 0xffffffffu) return fail(c, SUMA_ERR_INVALID, "suma_semantic_project: too many points");
  const SemProj q = sem_proj(sp);
  r = grow(c, c->sem_zbuf, q.P, {c->stream});
  if (r < 0) return r;
  /* the z-buffer is left cleared by every resolve: only a new one needs a fill */
  if (r) HIP_TRY(c, hipMemsetAsync(c->sem_zbuf, 0xFF, (size_t)q.P * 8, c->stream));
  ProfScope ps(c, "semantic_project", 20.0 * n + 32.0 * q.P);
  if (n > 0)
    ks_scatter<<<(n + 255) / 256, 256, 0, c->stream>>>((const float4*)d_points, n, q, c->sem_zbuf, d_pixel);
  ks_resolve<<<(q.P + 255) / 256, 256, 0, c->stream>>>(c->sem_zbuf, (const float4*)d_points, q, d_input, d_proj_idx);
  HIP_TRY(c, hipGetLastError());
  return SUMA_OK;
}

extern "C" int suma_semantic_unproject(suma_ctx* c, const suma_semantic_params* sp, const float* d_scores,
                                       int scores_are_logits, const int32_t* d_pixel, uint32_t n, float* d_labels,
                                       float* d_probs) {
  if (!c) return SUMA_ERR_INVALID;
  int r = semantic_check(c, sp);
  if (r) return r;
  if (n > 0 && (!d_scores || !d_pixel || !d_labels || !d_probs))
    return fail(c, SUMA_ERR_INVALID, "suma_semantic_unproject: NULL buffer");
  HIP_TRY(c, launch_semantic_unproject(c, sp, d_scores, scores_are_logits, d_pixel, n, d_labels, d_probs));
  return SUMA_OK;
}

int semantic_scan_input(suma_pipeline* s, uint32_t n, void* producer_event, hipStream_t* st) {
  suma_ctx* c = s->c;
  SUMA_REFUSE_WHILE_DESKEW(s, "suma_pipeline_*_scan_scores*");
  if (s->phase != 0)
    return fail(c, SUMA_ERR_INVALID, "suma_pipeline_begin_scan: the previous scan has not been closed with suma_pipeline_update_map");
  *st = pipeline_input_stream(s);
  /* the previous scan's preprocessing may still read the old labels (input stream), its frame readers follow */
  const size_t cap = (size_t)n + n / 4 + 1024;
  if (grow(c, c->sem_labels, n, {*st, c->stream}, cap) < 0 || grow(c, c->sem_probs, n, {*st, c->stream}, cap) < 0)
    return SUMA_ERR_HIP;
  if (producer_event) HIP_TRY(c, hipStreamWaitEvent(*st, (hipEvent_t)producer_event, 0));
  return SUMA_OK;
}

/* begin_scan_device with the back-projection in front, both on the stream the pipeline preprocesses on */
extern "C" int suma_pipeline_begin_scan_scores(suma_pipeline* s, const suma_semantic_params* sp,
                                               const suma_float4* d_points, const float* d_scores,
                                               int scores_are_logits, const int32_t* d_pixel, uint32_t n,
                                               void* producer_event) {
  if (!s) return SUMA_ERR_INVALID;
  suma_ctx* c = s->c;
  int r = semantic_check(c, sp);
  if (r) return r;
  if (n > 0 && (!d_points || !d_scores || !d_pixel))
    return fail(c, SUMA_ERR_INVALID, "suma_pipeline_begin_scan_scores: NULL buffer");
  hipStream_t st;
  r = semantic_scan_input(s, n, producer_event, &st);
  if (r) return r;
  c->ls = st;
  hipError_t e = launch_semantic_unproject(c, sp, d_scores, scores_are_logits, d_pixel, n, c->sem_labels, c->sem_probs);
  c->ls = c->stream;
  HIP_TRY(c, e);
  /* K1-K3 follow on the same stream, exactly as suma_pipeline_begin_scan_device runs them */
  return pipeline_begin_scan_impl(s, d_points, c->sem_labels, c->sem_probs, n, nullptr);
}

extern "C" int suma_pipeline_process_scan_scores(suma_pipeline* s, const suma_semantic_params* sp,
                                                 const suma_float4* d_points, const float* d_scores,
                                                 int scores_are_logits, const int32_t* d_pixel, uint32_t n,
                                                 void* producer_event, int32_t fixed_iterations) {
  return pipeline_finish_scan(
      s, suma_pipeline_begin_scan_scores(s, sp, d_points, d_scores, scores_are_logits, d_pixel, n, producer_event),
      fixed_iterations, false);
}
