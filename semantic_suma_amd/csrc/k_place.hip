/*
 * k_place.hip -- place recognition: a compact, rotation-tolerant descriptor of a scan, made from the vertex map a frame
 * already holds, and a brute-force search over the descriptors of a whole mapping session that returns candidate places
 * with a yaw (include/suma_hip.h, suma_place_*; host side csrc/suma_place.hip).  Nothing in the reference does this.  The
 * descriptor is a polar height map about the sensor (sectors x rings, the highest point of each cell), compared column
 * by column under every cyclic shift of the sectors.
 *
 * Kernels (none uses scratch or inline assembly):
 *   kp_describe  grid-stride over the texels; 32-bit atomic max on the bit pattern of the (positive) heights, first in
 *                an LDS copy of the cells, then the non-empty cells into the entry.  The entry's cells are zero before.
 *   kp_norms     lane per (entry, sector): the column norm, summed in ring order.
 *   kp_search    the query's cells and norms in LDS (columns an odd stride apart: no bank conflicts between lanes that
 *                read neighbouring columns); one wave per entry, one lane per shift -- hence sectors <= 64; a lane runs
 *                the sector and ring loops sequentially, so the summation order is the specification's; the entry is
 *                read at wave-uniform addresses; a wave reduction over (dist, shift) follows.  Entries beyond the count
 *                are masked by the wave's own loop bound.
 *   kp_topk      one block, K rounds of argmin over the per-entry results: round k takes the least (dist, index) that
 *                lies behind round k - 1's.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; IEEE sqrtf and `/`; sdm_atan2 of
 * include/suma_detmath.h; tests/place_shim.c restates it on the host).  TWO_PI = 2.0f * SUMA_PI_F.
 *
 * Parameters (suma_place_params): rings R 1..64, sectors S 1..64, max_range finite > 0, height_offset finite,
 *   keep_label[SUMA_DRAW_COLORS].
 * Descriptor of a frame: every texel of SUMA_MAP_VERTEX with w > 0 is a point (x, y, z); its label is
 *   world_label(semantic.x) (k_world.hip: t = r * 255.0f + 0.5f; 0 <= t < 260 ? (uint32_t)t : 0); skipped unless
 *   keep_label[label].  Then
 *     d = sqrtf(x*x + y*y); skipped unless d > 0 && d < max_range (a NaN fails this)
 *     ring = min((int)(d * ((float)R / max_range)), R - 1)
 *     a = sdm_atan2(y, x); if (a < 0) a = a + TWO_PI
 *     sector = min((int)(a * ((float)S / TWO_PI)), S - 1)
 *     h = z + height_offset; skipped unless h > 0 && h <= 1000.0f
 *     cell[sector][ring] = max(cell, h); empty cells are 0.
 *   The result does not depend on the order of the texels.  norm[sector] = sqrtf(sum over ring of v*v), summed in ring
 *   order from 0.0f with plain multiply and add.  A stored entry is S*R cells (sector-major), then S norms, and a
 *   caller-chosen uint32 id.  The norms are always made on the device from the cells.
 * Distance of query q to entry c at shift s: for j = 0 .. S-1 in order, jq = (j + s) mod S: if q.norm[jq] > 0 &&
 *   c.norm[j] > 0: sum = sum + dot / (q.norm[jq] * c.norm[j]), cnt = cnt + 1, with dot the ring-order sum of
 *   q.cell[jq][r] * c.cell[j][r] from 0.0f.  dist(s) = cnt ? 1.0f - sum / (float)cnt : 1.0f.  The entry's result is the
 *   least dist as a float compare; on a tie the smallest s.
 * Yaw (made on the host, suma_place.hip): D = TWO_PI / (float)S; yaw = shift <= S/2 ? -(float)shift * D :
 *   (float)(S - shift) * D.  A query sensor turned by +theta about z against the entry's gives shift ~ S - theta / D; the
 *   pose hypothesis is T_entry * Rz(yaw).
 * Search: all entries are scored; those whose id lies in [exclude_lo, exclude_hi] are left out (lo > hi: none); the K
 *   best (K <= 32) ordered by (dist ascending, entry index ascending).
 * Limit: cells are 0 or in (0, 1000]; a product of two column norms that underflows to 0 is not defined (heights
 *   below 1e-18).
 */
#include "suma_internal.h"

#define KP_THREADS 256
#define KP_WAVES (KP_THREADS / 64)
#define KP_TWO_PI (2.0f * SUMA_PI_F)

/* k_world.hip's rule for a surfel's r */
SDEV uint32_t place_label(float r) {
  const float t = r * 255.0f + 0.5f;
  return (t >= 0.0f && t < 260.0f) ? (uint32_t)t : 0u;
}

__global__ void __launch_bounds__(KP_THREADS)
    kp_describe(const float4* __restrict__ vertex, const float4* __restrict__ semantic, uint32_t n_texels, PlaceArgs a,
                uint32_t* __restrict__ cells) {
  __shared__ uint32_t lds[SUMA_PLACE_MAX_DIM * SUMA_PLACE_MAX_DIM];
  const uint32_t nc = a.S * a.R;
  for (uint32_t i = threadIdx.x; i < nc; i += KP_THREADS) lds[i] = 0u;
  __syncthreads();
  for (uint32_t t = blockIdx.x * KP_THREADS + threadIdx.x; t < n_texels; t += gridDim.x * KP_THREADS) {
    const float4 v = vertex[t];
    if (!(v.w > 0.0f)) continue;
    const uint32_t L = place_label(semantic[t].x);
    if (!((a.keep[L >> 5] >> (L & 31u)) & 1u)) continue;
    const float d = sdm_sqrt(v.x * v.x + v.y * v.y);
    if (!(d > 0.0f && d < a.max_range)) continue;
    int ring = (int)(d * a.ring_scale);
    if (ring > (int)a.R - 1) ring = (int)a.R - 1;
    float ang = sdm_atan2(v.y, v.x);
    if (ang < 0.0f) ang = ang + KP_TWO_PI;
    int sector = (int)(ang * a.sector_scale);
    if (sector > (int)a.S - 1) sector = (int)a.S - 1;
    const float h = v.z + a.height_offset;
    if (!(h > 0.0f && h <= 1000.0f)) continue;
    if (ring < 0 || sector < 0) continue; /* cannot happen for the d and ang above; keeps the index in bounds */
    atomicMax(&lds[(uint32_t)sector * a.R + (uint32_t)ring], __float_as_uint(h)); /* positive floats order as their bits */
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nc; i += KP_THREADS)
    if (lds[i]) atomicMax(&cells[i], lds[i]);
}

__global__ void __launch_bounds__(KP_THREADS)
    kp_norms(float* __restrict__ entries, uint32_t stride, uint32_t n_entries, uint32_t S, uint32_t R) {
  const uint32_t t = blockIdx.x * KP_THREADS + threadIdx.x;
  if (t >= n_entries * S) return;
  const uint32_t e = t / S, j = t - e * S;
  float* c = entries + (size_t)e * stride;
  float sum = 0.0f;
  for (uint32_t r = 0; r < R; ++r) {
    const float v = c[j * R + r];
    sum = sum + v * v;
  }
  c[S * R + j] = sdm_sqrt(sum);
}

/* the lesser of two (dist, index) pairs: float compare, then the smaller index */
SDEV bool kp_less(float d2, uint32_t i2, float d, uint32_t i) { return d2 < d || (d2 == d && i2 < i); }

__global__ void __launch_bounds__(KP_THREADS)
    kp_search(const float* __restrict__ db, uint32_t stride, uint32_t n_entries, const float* __restrict__ q, uint32_t S,
              uint32_t R, float* __restrict__ dist, int32_t* __restrict__ shift) {
  __shared__ float qc[SUMA_PLACE_MAX_DIM * (SUMA_PLACE_MAX_DIM + 1)];
  __shared__ float qn[SUMA_PLACE_MAX_DIM];
  const uint32_t Rp = R | 1u; /* odd column stride */
  for (uint32_t i = threadIdx.x; i < S * R; i += KP_THREADS) qc[(i / R) * Rp + (i % R)] = q[i];
  for (uint32_t i = threadIdx.x; i < S; i += KP_THREADS) qn[i] = q[S * R + i];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (uint32_t e = blockIdx.x * KP_WAVES + wave; e < n_entries; e += gridDim.x * KP_WAVES) {
    const float* c = db + (size_t)e * stride;
    const float* cn = c + S * R;
    float d = __uint_as_float(0x7f800000u); /* lanes without a shift never win */
    uint32_t s = 0xffffffffu;
    if (lane < S) {
      float sum = 0.0f;
      uint32_t cnt = 0;
      for (uint32_t j = 0; j < S; ++j) {
        uint32_t jq = j + lane;
        if (jq >= S) jq -= S;
        const float a = qn[jq], b = cn[j];
        if (a > 0.0f && b > 0.0f) {
          float dot = 0.0f;
          for (uint32_t r = 0; r < R; ++r) dot = dot + qc[jq * Rp + r] * c[j * R + r];
          sum = sum + dot / (a * b);
          cnt += 1u;
        }
      }
      d = cnt ? 1.0f - sum / (float)cnt : 1.0f;
      s = lane;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const float d2 = __shfl_xor(d, m, 64);
      const uint32_t s2 = (uint32_t)__shfl_xor((int)s, m, 64);
      if (kp_less(d2, s2, d, s)) d = d2, s = s2;
    }
    if (lane == 0) {
      dist[e] = d;
      shift[e] = (int32_t)s;
    }
  }
}

__global__ void __launch_bounds__(KP_THREADS)
    kp_topk(const float* __restrict__ dist, const int32_t* __restrict__ shift, const uint32_t* __restrict__ ids,
            uint32_t n_entries, uint32_t lo, uint32_t hi, uint32_t K, suma_place_match* __restrict__ out,
            uint32_t* __restrict__ n_out) {
  __shared__ float wd[KP_WAVES];
  __shared__ uint32_t wi[KP_WAVES];
  __shared__ float pick_d;
  __shared__ uint32_t pick_i;
  const uint32_t none = 0xffffffffu;
  const float inf = __uint_as_float(0x7f800000u);
  float prev_d = 0.0f;
  uint32_t prev_i = none; /* none: no round has picked yet */
  uint32_t found = 0;
  for (uint32_t k = 0; k < K; ++k) {
    float bd = inf;
    uint32_t bi = none;
    for (uint32_t e = threadIdx.x; e < n_entries; e += KP_THREADS) {
      const uint32_t id = ids[e];
      if (lo <= hi && id >= lo && id <= hi) continue;
      const float d = dist[e];
      const bool behind = prev_i == none || d > prev_d || (d == prev_d && e > prev_i);
      if (behind && kp_less(d, e, bd, bi)) bd = d, bi = e;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const float d2 = __shfl_xor(bd, m, 64);
      const uint32_t i2 = (uint32_t)__shfl_xor((int)bi, m, 64);
      if (kp_less(d2, i2, bd, bi)) bd = d2, bi = i2;
    }
    if ((threadIdx.x & 63u) == 0) wd[threadIdx.x >> 6] = bd, wi[threadIdx.x >> 6] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
      float d = wd[0];
      uint32_t i = wi[0];
      for (uint32_t w = 1; w < KP_WAVES; ++w)
        if (kp_less(wd[w], wi[w], d, i)) d = wd[w], i = wi[w];
      pick_d = d, pick_i = i;
      if (i != none) {
        suma_place_match mt;
        mt.index = i, mt.id = ids[i], mt.distance = d, mt.shift = shift[i], mt.yaw = 0.0f;
        out[k] = mt;
      }
    }
    __syncthreads();
    prev_d = pick_d, prev_i = pick_i;
    __syncthreads(); /* pick_* and w* are rewritten by the next round */
    if (prev_i == none) break; /* block-uniform */
    found = k + 1u;
  }
  if (threadIdx.x == 0) *n_out = found;
}

/* ---- launchers ---- */
hipError_t launch_kp_describe(hipStream_t st, const suma_frame* f, const PlaceArgs& a, float* entry) {
  const uint32_t n = f->width * f->height;
  const size_t bytes = ((size_t)a.S * a.R + a.S) * sizeof(float);
  hipError_t e = hipMemsetAsync(entry, 0, bytes, st);
  if (e != hipSuccess) return e;
  uint32_t blocks = (n + 4u * KP_THREADS - 1u) / (4u * KP_THREADS);
  blocks = blocks < 1u ? 1u : (blocks > 256u ? 256u : blocks);
  kp_describe<<<blocks, KP_THREADS, 0, st>>>(f->map[SUMA_MAP_VERTEX], f->map[SUMA_MAP_SEMANTIC], n, a,
                                             reinterpret_cast<uint32_t*>(entry));
  kp_norms<<<1, KP_THREADS, 0, st>>>(entry, a.S * a.R + a.S, 1u, a.S, a.R);
  return hipGetLastError();
}

hipError_t launch_kp_norms(hipStream_t st, float* entries, uint32_t n_entries, uint32_t S, uint32_t R) {
  if (!n_entries) return hipSuccess;
  const uint64_t lanes = (uint64_t)n_entries * S;
  kp_norms<<<(unsigned)((lanes + KP_THREADS - 1) / KP_THREADS), KP_THREADS, 0, st>>>(entries, S * R + S, n_entries, S, R);
  return hipGetLastError();
}

hipError_t launch_kp_search(hipStream_t st, const float* db, uint32_t n_entries, const float* q, uint32_t S, uint32_t R,
                            float* dist, int32_t* shift) {
  if (!n_entries) return hipSuccess;
  uint32_t blocks = (n_entries + KP_WAVES - 1u) / KP_WAVES;
  if (blocks > 2048u) blocks = 2048u;
  kp_search<<<blocks, KP_THREADS, 0, st>>>(db, S * R + S, n_entries, q, S, R, dist, shift);
  return hipGetLastError();
}

hipError_t launch_kp_topk(hipStream_t st, const float* dist, const int32_t* shift, const uint32_t* ids, uint32_t n_entries,
                          uint32_t lo, uint32_t hi, uint32_t K, suma_place_match* out, uint32_t* n_out) {
  kp_topk<<<1, KP_THREADS, 0, st>>>(dist, shift, ids, n_entries, lo, hi, K, out, n_out);
  return hipGetLastError();
}
