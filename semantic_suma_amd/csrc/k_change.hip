/*
 * k_change.hip -- map maintenance, first step: while a localiser tracks (suma_localize.hip), every record of the world
 * map collects evidence -- confirmed (hit), seen through (miss) or hidden (occluded) -- from the scans that look at it.
 * The localiser never writes the map; the evidence is a second array beside the binned records, it comes
 * back in the caller's record order, and a rule (suma_change_prune_mask, host only) turns it into a pruned map.  Nothing
 * in the reference does this: its stability log-odds (K9) exist inside a mapping run only.
 *
 * Kernels (VGPRs: tools/isa_stats.py k_change.hip; none uses scratch):
 *   kc_observe  lane per window record, blocks of 256: finds its span by binary search (loc_window_record), loads the record's
 *               three 16-byte pieces and its 16-byte evidence word together, then -- the one dependent round trip -- the
 *               three texels of the frame the record projects to (K9's header, k_update.hip: the chain of dependent loads
 *               is the cost, so everything that does not depend on the projection is in flight before it).  The record
 *               is owned by this lane alone: no atomics on the evidence, one 16-byte store, only when it changed.  The
 *               nine totals are summed per block in LDS, then one global atomicAdd per non-zero total and block.
 *   kc_scatter  lane per sorted position: evidence from sorted order into source order, into a zeroed output.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; the helpers of dev_math.h with
 * their explicit FMAs and orders; every comparison is written so that a NaN counts nothing; tests/change_shim.c restates
 * it on the host, byte for byte).
 *
 * Parameters (suma_change_params): free_margin (0.5 m), min_view_cos (0.3), max_range (50 m), tracked_only (1).
 * Evidence (suma_change_evidence, 16 bytes): uint32 hits, misses, occluded, label_changes; one per record of the array
 *   suma_localizer_set_map was given, in that array's order; dropped records stay zero.
 * One observation of a frame F at a sensor pose T (double[16], world frame):
 *   P = T rounded to fp32 element by element; Pinv = mat4_rigid_inv(T) in fp64, then rounded to fp32; q = the data
 *   image's proj_t, as K9 receives it.  For every record of the current window, p = (x, y, z), n = (nx, ny, nz), label:
 *   1. v = m4_point(Pinv, p), r = len3(v).  UNSEEN unless r > 0.0f && r < max_range.
 *   2. ns = normalize3(m4_dir(Pinv, n)), c = dot3(ns, divs3(neg3(v), r))  (K9's `visible` expression).
 *   3. pr = project01(q, v); imx = sdm_floor(pr.x * q.width) + 0.5f, imy = sdm_floor(pr.y * q.height) + 0.5f,
 *      in_tex = imx >= 0 && imx < q.width && imy >= 0 && imy < q.height, tx = (int)sdm_floor(imx), ty likewise
 *      (k9_prepare, k_update.hip).  UNSEEN unless in_tex.
 *   4. dv, dn, ds = the vertex, normal and semantic texels of F at (tx, ty).  NO RETURN unless dv.w > 0.5f; no return is
 *      no evidence.
 *   5. m = xyz(dv), rm = len3(m).
 *      rm + free_margin < r:            occluded += 1.
 *      else rm > r + free_margin:       misses += 1 if c > min_view_cos, else GRAZING (nothing written).
 *      else (the ranges agree): if dn.w > 0.5f && c > 0.0f:
 *             mw = m4_point(P, m), nw = normalize3(m4_dir(P, xyz(dn))),
 *             distance = sdm_abs(dot3(n, sub3(mw, p))), angle = len3(cross3(nw, n));
 *             if distance < map_max_distance && angle < update_angle_thresh (the literals of K9):
 *               hits += 1, and label_changes += 1 when world_label(ds.x) != label  (k_world.hip's rule);
 *           anything else that reaches this branch is NEAR (nothing written).
 * Totals of one observation (suma_change_counts, uint32): n_window, unseen, no_return, occluded, misses, grazing, hits,
 *   near, label_changes -- integer sums, so independent of the order.
 * Prune rule (suma_change_rule {min_misses = 3, miss_ratio = 2.0f}): a record is removed iff
 *   misses >= min_misses && (float)misses > miss_ratio * (float)hits.  occluded and label_changes do not enter it.
 */
#include "suma_internal.h"
#include "group_by_key.h"

#define CHG_THREADS 256
enum { CHG_WINDOW = 0, CHG_UNSEEN, CHG_NO_RETURN, CHG_OCCLUDED, CHG_MISSES, CHG_GRAZING, CHG_HITS, CHG_NEAR, CHG_LABEL, CHG_TOTALS };

struct ChangeArgs {
  const float4* sorted;  /* 3 float4 a record */
  uint4* evidence;       /* one a sorted record */
  const LocSpan* spans;
  uint32_t n_spans, total;
  const float4 *V, *N, *Sem;
  proj_t q;
  m4 P, Pinv;
  float free_margin, min_view_cos, max_range;
  float map_max_distance, update_angle_thresh;
  uint32_t* totals; /* CHG_TOTALS words */
};

__global__ void __launch_bounds__(CHG_THREADS) kc_observe(ChangeArgs a) {
  __shared__ uint32_t tot[CHG_TOTALS];
  if (threadIdx.x < CHG_TOTALS) tot[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t o = blockIdx.x * CHG_THREADS + threadIdx.x;
  if (o < a.total) {
    const size_t k = loc_window_record(a.spans, a.n_spans, o);
    const float4* src = a.sorted + 3 * k;
    const float4 s0 = src[0], s1 = src[1], s2 = src[2];
    uint4 ev = a.evidence[k];

    const v3 p = xyz(s0), n = xyz(s1);
    const uint32_t label = __float_as_uint(s2.x);
    /* 1, 2 */
    const v3 v = m4_point(a.Pinv.m, p);
    const float r = len3(v);
    const v3 ns = normalize3(m4_dir(a.Pinv.m, n));
    const float c = dot3(ns, divs3(neg3(v), r));
    /* 3 */
    const v3 pr = project01(a.q, v);
    const float imx = sdm_floor(pr.x * a.q.width) + 0.5f, imy = sdm_floor(pr.y * a.q.height) + 0.5f;
    const bool in_tex = (imx >= 0.0f && imx < a.q.width && imy >= 0.0f && imy < a.q.height);
    const int32_t tx = in_tex ? (int32_t)sdm_floor(imx) : 0, ty = in_tex ? (int32_t)sdm_floor(imy) : 0;
    /* 4: the three texels from an always valid address, as one batch */
    const size_t pix = (size_t)ty * (size_t)a.q.W + (size_t)tx;
    const float4 dv = a.V[pix], dn = a.N[pix], ds = a.Sem[pix];

    /* 5, without branches: every lane of a wave takes another way through the cases, and a texel that is first read
     * inside a branch would be one more dependent round trip */
    const v3 m = xyz(dv);
    const float rm = len3(m);
    const v3 mw = m4_point(a.P.m, m);
    const v3 nw = normalize3(m4_dir(a.P.m, xyz(dn)));
    const float distance = sdm_abs(dot3(n, sub3(mw, p)));
    const float angle = len3(cross3(nw, n));
    const bool seen = (r > 0.0f && r < a.max_range) & in_tex;
    const bool ret = seen & (dv.w > 0.5f);
    const bool occluded = ret & (rm + a.free_margin < r);
    const bool behind = ret & !occluded & (rm > r + a.free_margin);
    const bool miss = behind & (c > a.min_view_cos);
    const bool agree = ret & !occluded & !behind;
    const bool hit = agree & (dn.w > 0.5f) & (c > 0.0f) & (distance < a.map_max_distance) & (angle < a.update_angle_thresh);
    const bool relabel = hit & (world_label(ds.x) != label);
    const uint32_t cat = !seen ? CHG_UNSEEN : !ret ? CHG_NO_RETURN : occluded ? CHG_OCCLUDED : miss ? CHG_MISSES
                         : behind ? CHG_GRAZING : hit ? CHG_HITS : CHG_NEAR;
    ev.x += hit ? 1u : 0u;
    ev.y += miss ? 1u : 0u;
    ev.z += occluded ? 1u : 0u;
    ev.w += relabel ? 1u : 0u;
    const bool changed = hit | miss | occluded;
    if (changed) a.evidence[k] = ev;
    atomicAdd(&tot[cat], 1u); /* LDS; integer sums do not depend on the order */
    if (relabel) atomicAdd(&tot[CHG_LABEL], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t first = blockIdx.x * CHG_THREADS;
    tot[CHG_WINDOW] = a.total > first ? min(a.total - first, (uint32_t)CHG_THREADS) : 0u;
  }
  __syncthreads();
  if (threadIdx.x < CHG_TOTALS && tot[threadIdx.x]) atomicAdd(&a.totals[threadIdx.x], tot[threadIdx.x]);
}

__global__ void __launch_bounds__(CHG_THREADS)
    kc_scatter(const uint4* __restrict__ evidence, const uint32_t* __restrict__ src_idx, uint32_t n_kept, uint32_t n,
               uint4* __restrict__ out) {
  const uint32_t k = blockIdx.x * CHG_THREADS + threadIdx.x;
  if (k >= n_kept) return;
  const uint32_t s = src_idx[k];
  if (s < n) out[s] = evidence[k];
}

/* ---- host side ---- */
hipError_t launch_kc_observe(suma_ctx* c, const LocMap& m, uint32_t n_spans, uint32_t total, const suma_frame* f,
                             const double T[16], const suma_change_params& cp, uint32_t* d_totals) {
  if (total == 0) return hipSuccess;
  ChangeArgs a;
  a.sorted = m.sorted;
  a.evidence = reinterpret_cast<uint4*>(m.evidence.p);
  a.spans = m.spans;
  a.n_spans = n_spans;
  a.total = total;
  a.V = f->map[SUMA_MAP_VERTEX];
  a.N = f->map[SUMA_MAP_NORMAL];
  a.Sem = f->map[SUMA_MAP_SEMANTIC];
  a.q = c->pd;
  double inv[16];
  mat4_rigid_inv(T, inv);
  mat4_cast_f(T, a.P.m);
  mat4_cast_f(inv, a.Pinv.m);
  a.free_margin = cp.free_margin;
  a.min_view_cos = cp.min_view_cos;
  a.max_range = cp.max_range;
  a.map_max_distance = c->p.map_max_distance;
  a.update_angle_thresh = c->mc.update_angle_thresh;
  a.totals = d_totals;
  kc_observe<<<(total + CHG_THREADS - 1) / CHG_THREADS, CHG_THREADS, 0, c->stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_kc_scatter(suma_ctx* c, const LocMap& m, suma_change_evidence* d_out) {
  if (m.n_kept == 0) return hipSuccess;
  kc_scatter<<<(m.n_kept + CHG_THREADS - 1) / CHG_THREADS, CHG_THREADS, 0, c->stream>>>(
      reinterpret_cast<const uint4*>(m.evidence.p), m.src_idx, m.n_kept, m.n_total, reinterpret_cast<uint4*>(d_out));
  return hipGetLastError();
}
