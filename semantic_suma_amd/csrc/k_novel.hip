/*
 * k_novel.hip -- map maintenance, second step: while a localiser tracks (suma_localize.hip), the texels of a scan that no
 * record of the world map explains are collected as world-frame candidate surfels on the device; on request they are
 * fused per voxel, kept where several scans agree, and handed back as suma_world_surfel records that concatenate with
 * the records the prune rule keeps (k_change.hip) into the updated map.  The localiser still never writes its map
 * (DESIGN.md 12): the candidates are a buffer beside it.  Nothing in the reference does this.
 *
 * Kernels (VGPRs by tools/isa_stats.py k_novel.hip; none spills or uses scratch):
 *   kn_mark     13 VGPRs  lane per window record, blocks of 256: span by binary search (loc_window_record), the record's
 *               position (16 bytes; the normal and the label are not needed), then -- the one dependent round trip -- the
 *               vertex texel it projects to; the classification is written without branches, the mark is a plain byte
 *               store (all writers store 1).
 *   kn_collect  44 VGPRs  lane per texel: the two texels, the nine mark bytes from clamped (always valid) addresses as
 *               one batch, the tests of step 2 without branches; a flag byte per texel and five counts per block.
 *   kn_emit     33 VGPRs  lane per texel: every block sums the counts of the blocks before it (P / 256 words: 512 at
 *               64 x 2048), ranks its flagged texels by wave ballots, and writes the records behind the device-side running
 *               count; the block that finishes last (a ticket, no spinning) advances the count, clamps it to the capacity
 *               and adds up the totals.  Chosen over a single pass with look-back because nothing here waits for another
 *               block, and over flags + rocPRIM's exclusive scan + emit because the scan brings launches of its own
 *               (P is 131 072 at 64 x 2048: launch count matters more than bandwidth): a collection is one memset and
 *               three launches.
 *   kn_key      22 VGPRs  fusion, lane per candidate: voxel key, vote label, timestamp, index.
 *   kn_heads    14 VGPRs  fusion, lane per sorted position: the lane at the head of a voxel's run walks it in
 *               (key, timestamp) order and counts the distinct timestamps.
 *   kn_reduce   32 VGPRs  fusion, lane per sorted position: the head of a kept run walks it in (key, label, index) order
 *               and writes the voxel's record.
 *   between them the sorts, the key gather and the scan of k_group.hip.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; the helpers of dev_math.h; every
 * comparison is written so that a NaN collects nothing; tests/novel_shim.c restates it on the host, byte for byte).
 *
 * Parameters (suma_novel_params): agree_margin (0.5 m), max_range (50 m), tracked_only (1), max_candidates (4 194 304).
 * One collection of a data-sized frame F at a sensor pose T (double[16], world frame) with a scan_id, over the current
 * window.  P, Pinv and q are k_change.hip's: P = T rounded to fp32, Pinv = mat4_rigid_inv(T) in fp64 rounded to fp32, q
 * the data image's proj_t.
 *   1. MARK.  The mark image (one byte a texel) is zeroed.  Every window record is projected by k_change.hip's steps 1
 *      and 3: v = m4_point(Pinv, p), r = len3(v), pr = project01(q, v), imx, imy, in_tex, tx, ty.  The record is SEEN iff
 *      r > 0.0f && r < max_range && in_tex.  It AGREES with its texel dv iff it is seen, dv.w > 0.5f,
 *      !(rm + agree_margin < r) and !(rm > r + agree_margin), rm = len3(xyz(dv)).  An agreeing record sets
 *      mark[ty * W + tx] = 1.  An OR: independent of the order.
 *   2. COLLECT.  Every texel (tx, ty) with dv, dn, ds, m = xyz(dv), rm = len3(m), nn = xyz(dn) falls into the first
 *      category whose test it fails, and is NOVEL when it fails none:
 *        NO RETURN     unless dv.w > 0.5f && dn.w > 0.5f;
 *        OUT OF RANGE  unless rm > 0.0f && rm + agree_margin < max_range (every record that could agree is then inside
 *                      max_range itself) and the three components of w = m4_point(P, m) are finite;
 *        GRAZING       unless dot3(nn, divs3(neg3(m), rm)) > radconf_angle_thresh (K8's validity, the ctx's constant);
 *        EXPLAINED     if a mark is set at (tx + dx mod W, ty + dy), dx, dy in -1 .. 1: columns wrap (the image is a full
 *                      turn), rows outside the image count as unmarked.
 *      Counts of one collection (suma_novel_counts, uint32): n_texels, no_return, out_of_range, grazing, explained, novel
 *      -- integer sums, the last five partition n_texels -- and stored.
 *   3. THE CANDIDATE of a novel texel (suma_world_surfel, 48 bytes): position = w; normal = normalize3(m4_dir(P, nn));
 *      radius = k8_pixel's ((1.41f * rm) * pixel_size) / fclamp(dot3(nn, divs3(neg3(m), rm)), 0.5f, 1.0f), clamped by
 *      fmin_(fmax_(radius, min_radius), max_radius); confidence = K10's log_prior, or log_prior - 0.5f when
 *      is_dynamic_label(ds.x * 255.0f); label = world_label(ds.x); prob = ds.w; timestamp = scan_id; support = 1.
 *   4. ORDER AND CAPACITY.  The candidates of a collection are appended behind those already held, in ascending texel
 *      index ty * W + tx.  The buffer holds max_candidates records: what does not fit is dropped from the end of the
 *      collection and added to n_overflow; stored counts what was written.  The running count lives on the device.
 *   5. FUSION, on request (suma_novel_fuse_params: voxel_size 0.2 m, min_views 2, confidence), over candidates 0 .. n - 1
 *      in creation order.  key = voxel_key (group_by_key.h) of the candidate's position: f_a = floorf(p_a / voxel_size), a
 *      candidate with any |f_a| >= 2^20 (NaN and infinite quotients included) is DROPPED (n_dropped),
 *      key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20).  Per distinct key, in ascending key order:
 *        views = the number of distinct timestamps among the members; the voxel is KEPT iff views >= min_views;
 *        representative = the member with the smallest radius (a NaN radius counts as +infinity), on a tie the smallest
 *          candidate index; x, y, z, radius, nx, ny, nz are the representative's; confidence = the parameter;
 *        vote (vote_weight and LabelVote, group_by_key.h): a member votes for L = its label if < 260, else 0, with the weight
 *          q = (uint32)rintf(clamp(prob, 0, 1) * 65535.0f) (NaN: 0), summed per label in uint64; label = the label with
 *          the greatest sum, on a tie the smallest id; prob = (float)sum_label / (float)sum_all; sum_all == 0: label =
 *          the representative's L, prob = 0;
 *        timestamp = the maximum over the members, support = the member count.
 *      A parallel uint32 array holds every output record's views.  n_voxels counts the distinct keys, n_out the kept.
 *      The result is a pure function of the candidates and the parameters.
 *
 * Decomposition of the fusion: two orders over the same sorted keys, each made by two stable radix sorts of (value, index)
 * (group_sort_by_value_then_key, k_group.hip) -- by timestamp (32 bits), then by key (64 bits: dropped candidates carry
 * VOXEL_NO_KEY and sort behind every voxel); and by label (9 bits), then by key.  The runs of both orders begin at the
 * same positions.  In the first a voxel's timestamps are ascending, so views is the number of changes plus one; in the
 * second its members come by label, then by index, so the vote needs one running sum (LabelVote).  No atomics on records,
 * no order that depends on a race.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"
#include "draw_vertex.h"
#include "group_by_key.h"

#define NOV_THREADS 256
/* per-block counts of kn_collect, NOV_BLOCK_WORDS words a block */
enum { NOV_NO_RETURN = 0, NOV_OUT_OF_RANGE, NOV_GRAZING, NOV_EXPLAINED, NOV_NOVEL, NOV_CATS, NOV_BLOCK_WORDS = 8 };

struct NovelArgs {
  const float4* sorted; /* 3 float4 a record */
  const LocSpan* spans;
  uint32_t n_spans, total;
  const float4 *V, *N, *Sem;
  proj_t q;
  m4 P, Pinv;
  float agree_margin, max_range;
  float angle_thresh, pixel_size, min_radius, max_radius, log_prior;
  uint32_t scan_id, capacity, n_blocks, n_texels;
  uint8_t *mark, *flag;
  uint32_t* block_counts;
  NovelState* state;
  float4* cand;
};

__global__ void __launch_bounds__(NOV_THREADS) kn_mark(NovelArgs a) {
  const uint32_t o = blockIdx.x * NOV_THREADS + threadIdx.x;
  if (o >= a.total) return;
  const v3 p = xyz(a.sorted[3 * loc_window_record(a.spans, a.n_spans, o)]);
  const v3 v = m4_point(a.Pinv.m, p);
  const float r = len3(v);
  const v3 pr = project01(a.q, v);
  const float imx = sdm_floor(pr.x * a.q.width) + 0.5f, imy = sdm_floor(pr.y * a.q.height) + 0.5f;
  const bool in_tex = (imx >= 0.0f && imx < a.q.width && imy >= 0.0f && imy < a.q.height);
  const int32_t tx = in_tex ? (int32_t)sdm_floor(imx) : 0, ty = in_tex ? (int32_t)sdm_floor(imy) : 0;
  const size_t pix = (size_t)ty * (size_t)a.q.W + (size_t)tx; /* always a valid address */
  const float4 dv = a.V[pix];
  const float rm = len3(xyz(dv));
  const bool seen = (r > 0.0f && r < a.max_range) & in_tex;
  const bool agree = seen & (dv.w > 0.5f) & !(rm + a.agree_margin < r) & !(rm > r + a.agree_margin);
  if (agree) a.mark[pix] = 1;
}

__global__ void __launch_bounds__(NOV_THREADS) kn_collect(NovelArgs a) {
  __shared__ uint32_t tot[NOV_CATS];
  if (threadIdx.x < NOV_CATS) tot[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t t = blockIdx.x * NOV_THREADS + threadIdx.x;
  if (t < a.n_texels) {
    const int32_t W = a.q.W, H = a.q.H;
    const int32_t tx = (int32_t)(t % (uint32_t)W), ty = (int32_t)(t / (uint32_t)W);
    const float4 dv = a.V[t], dn = a.N[t];
    uint32_t marks = 0;
#pragma unroll
    for (int32_t dy = -1; dy <= 1; ++dy) {
      const int32_t y = ty + dy;
      const bool inside = (y >= 0) & (y < H);
      const int32_t yc = min(max(y, 0), H - 1);
#pragma unroll
      for (int32_t dx = -1; dx <= 1; ++dx) {
        int32_t x = tx + dx;
        x = (x < 0) ? x + W : ((x >= W) ? x - W : x);
        const uint32_t b = a.mark[(size_t)yc * (size_t)W + (size_t)x];
        marks |= inside ? b : 0u;
      }
    }
    const v3 m = xyz(dv), nn = xyz(dn);
    const float rm = len3(m);
    const v3 w = m4_point(a.P.m, m);
    const float angle = dot3(nn, divs3(neg3(m), rm));
    const bool ret = (dv.w > 0.5f) & (dn.w > 0.5f);
    const bool fin = finite_f(w.x) && finite_f(w.y) && finite_f(w.z);
    const bool inr = (rm > 0.0f) & (rm + a.agree_margin < a.max_range) & fin;
    const bool steep = angle > a.angle_thresh;
    const uint32_t cat = !ret ? NOV_NO_RETURN : !inr ? NOV_OUT_OF_RANGE : !steep ? NOV_GRAZING
                         : marks ? NOV_EXPLAINED : NOV_NOVEL;
    a.flag[t] = (cat == NOV_NOVEL) ? 1 : 0;
    atomicAdd(&tot[cat], 1u); /* LDS; integer sums do not depend on the order */
  }
  __syncthreads();
  if (threadIdx.x < NOV_CATS) a.block_counts[(size_t)blockIdx.x * NOV_BLOCK_WORDS + threadIdx.x] = tot[threadIdx.x];
}

__global__ void __launch_bounds__(NOV_THREADS) kn_emit(NovelArgs a) {
  __shared__ uint32_t s_pre, s_tot, s_base, s_last, s_wave[NOV_THREADS / 64], s_sum[NOV_CATS];
  if (threadIdx.x == 0) s_pre = 0u, s_tot = 0u, s_base = a.state->count;
  if (threadIdx.x < NOV_CATS) s_sum[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
  for (uint32_t b = threadIdx.x; b < a.n_blocks; b += NOV_THREADS) {
    const uint32_t c = a.block_counts[(size_t)b * NOV_BLOCK_WORDS + NOV_NOVEL];
    tot += c;
    pre += (b < blockIdx.x) ? c : 0u;
  }
  if (pre) atomicAdd(&s_pre, pre);
  if (tot) atomicAdd(&s_tot, tot);
  const uint32_t t = blockIdx.x * NOV_THREADS + threadIdx.x;
  const bool f = (t < a.n_texels) && a.flag[t] != 0;
  const unsigned long long bal = __ballot(f);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t rank = s_pre + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
  for (uint32_t wv = 0; wv < wave; ++wv) rank += s_wave[wv];
  const uint32_t base = s_base;
  const uint32_t o = base + rank; /* capacity <= 2^30 and a collection < 2^31 texels: no wrap */
  if (f && o < a.capacity) {
    const float4 dv = a.V[t], dn = a.N[t], ds = a.Sem[t];
    const v3 m = xyz(dv), nn = xyz(dn);
    const float rm = len3(m);
    const v3 w = m4_point(a.P.m, m);
    const v3 nw = normalize3(m4_dir(a.P.m, nn));
    float radius = ((1.41f * rm) * a.pixel_size) / fclamp(dot3(nn, divs3(neg3(m), rm)), 0.5f, 1.0f);
    radius = fmin_(fmax_(radius, a.min_radius), a.max_radius);
    float conf = a.log_prior;
    if (is_dynamic_label(ds.x * 255.0f)) conf = a.log_prior - 0.5f;
    float4* dst = a.cand + 3 * (size_t)o;
    dst[0] = f4(w.x, w.y, w.z, radius);
    dst[1] = f4(nw.x, nw.y, nw.z, conf);
    dst[2] = f4(__uint_as_float(world_label(ds.x)), ds.w, __uint_as_float(a.scan_id), __uint_as_float(1u));
  }
  /* the block that finishes last advances the running count: every other block has read it by then */
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    s_last = (atomicAdd(&a.state->done, 1u) == gridDim.x - 1u) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  for (uint32_t b = threadIdx.x; b < a.n_blocks; b += NOV_THREADS)
#pragma unroll
    for (uint32_t k = 0; k < NOV_CATS; ++k) {
      const uint32_t c = a.block_counts[(size_t)b * NOV_BLOCK_WORDS + k];
      if (c) atomicAdd(&s_sum[k], c);
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t novel = s_tot, room = a.capacity - base; /* base <= capacity */
    const uint32_t stored = novel < room ? novel : room;
    NovelState* s = a.state;
    s->count = base + stored;
    s->n_overflow += novel - stored;
    s->done = 0u;
    s->counts[0] = a.n_texels;
    for (uint32_t k = 0; k < NOV_CATS; ++k) s->counts[1 + k] = s_sum[k];
    s->counts[6] = stored;
  }
}

/* ---- fusion ---- */
SDEV uint32_t novel_vote_label(uint32_t label) { return label < 260u ? label : 0u; }
enum { NOVF_DROPPED = 0, NOVF_VOXELS = 1, NOVF_OUT = 2, NOVF_COUNTERS = 4 };

__global__ void __launch_bounds__(NOV_THREADS)
    kn_key(uint32_t n, const float4* __restrict__ cand, float voxel_size, unsigned long long* __restrict__ key0,
           uint32_t* __restrict__ stamp, uint32_t* __restrict__ label, uint32_t* __restrict__ idx_a,
           uint32_t* __restrict__ idx_b, uint32_t* __restrict__ counters) {
  __shared__ uint32_t dropped;
  if (threadIdx.x == 0) dropped = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * NOV_THREADS + threadIdx.x;
  if (i < n) {
    const float4 c0 = cand[3 * (size_t)i], c2 = cand[3 * (size_t)i + 2];
    unsigned long long key = VOXEL_NO_KEY;
    if (!voxel_key(c0.x, c0.y, c0.z, voxel_size, &key)) atomicAdd(&dropped, 1u);
    key0[i] = key;
    stamp[i] = __float_as_uint(c2.z);
    label[i] = novel_vote_label(__float_as_uint(c2.x));
    idx_a[i] = i;
    idx_b[i] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0 && dropped) atomicAdd(&counters[NOVF_DROPPED], dropped);
}

/* keys: sorted; idx_a: the candidates by (key, timestamp, index) */
__global__ void __launch_bounds__(NOV_THREADS)
    kn_heads(uint32_t n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ idx_a,
             const float4* __restrict__ cand, uint32_t min_views, uint32_t* __restrict__ flag, uint32_t* __restrict__ views,
             uint32_t* __restrict__ counters) {
  __shared__ uint32_t voxels;
  if (threadIdx.x == 0) voxels = 0u;
  __syncthreads();
  const uint32_t j = blockIdx.x * NOV_THREADS + threadIdx.x;
  if (j < n) {
    const unsigned long long key = keys[j];
    uint32_t keep = 0, nv = 0;
    if (key != VOXEL_NO_KEY && (j == 0 || keys[j - 1] != key)) {
      uint32_t last = 0;
      for (uint32_t k = j; k < n && keys[k] == key; ++k) {
        const uint32_t ts = __float_as_uint(cand[3 * (size_t)idx_a[k] + 2].z);
        nv += (k == j || ts != last) ? 1u : 0u;
        last = ts;
      }
      keep = nv >= min_views ? 1u : 0u;
      atomicAdd(&voxels, 1u);
    }
    flag[j] = keep;
    views[j] = nv;
  }
  __syncthreads();
  if (threadIdx.x == 0 && voxels) atomicAdd(&counters[NOVF_VOXELS], voxels);
}

/* idx_b: the candidates by (key, label, index) */
__global__ void __launch_bounds__(NOV_THREADS)
    kn_reduce(uint32_t n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ idx_b,
              const float4* __restrict__ cand, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
              const uint32_t* __restrict__ views, float confidence, float4* __restrict__ out, uint32_t* __restrict__ views_out,
              uint32_t capacity, uint32_t* __restrict__ counters) {
  const uint32_t j = blockIdx.x * NOV_THREADS + threadIdx.x;
  if (j >= n) return;
  const uint32_t f = flag[j], o = pos[j];
  if (j == n - 1u) counters[NOVF_OUT] = o + f;
  if (!f || o >= capacity) return;
  const unsigned long long key = keys[j];
  LabelVote tally;
  uint32_t rep = 0, stamp = 0, support = 0;
  float rad_best = 0.0f;
  for (uint32_t k = j; k < n && keys[k] == key; ++k) {
    const uint32_t s = idx_b[k];
    const float4 c0 = cand[3 * (size_t)s], c2 = cand[3 * (size_t)s + 2];
    const uint32_t ts = __float_as_uint(c2.z);
    tally.add(novel_vote_label(__float_as_uint(c2.x)), vote_weight(c2.y));
    const float rad = (c0.w == c0.w) ? c0.w : INFINITY;
    if (support == 0 || rad < rad_best || (rad == rad_best && s < rep)) rad_best = rad, rep = s;
    stamp = (ts > stamp) ? ts : stamp;
    ++support;
  }
  const float4 r0 = cand[3 * (size_t)rep], r1 = cand[3 * (size_t)rep + 1], r2 = cand[3 * (size_t)rep + 2];
  uint32_t label;
  const float prob = tally.close(novel_vote_label(__float_as_uint(r2.x)), &label);
  float4* dst = out + 3 * (size_t)o;
  dst[0] = r0;
  dst[1] = f4(r1.x, r1.y, r1.z, confidence);
  dst[2] = f4(__uint_as_float(label), prob, __uint_as_float(stamp), __uint_as_float(support));
  views_out[o] = views[j];
}

/* ---- host side ---- */
int novel_collect(suma_ctx* c, Novel& nv, const LocMap& m, uint32_t n_spans, uint32_t total, const suma_frame* f,
                  const double T[16], uint32_t scan_id) {
  const uint32_t P = (uint32_t)f->width * (uint32_t)f->height;
  NovelArgs a;
  a.sorted = m.sorted;
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
  a.agree_margin = nv.np.agree_margin;
  a.max_range = nv.np.max_range;
  a.angle_thresh = c->mc.radconf_angle_thresh;
  a.pixel_size = c->mc.pixel_size;
  a.min_radius = c->p.min_radius;
  a.max_radius = c->p.max_radius;
  a.log_prior = c->mc.log_prior;
  a.scan_id = scan_id;
  a.capacity = nv.np.max_candidates;
  a.n_texels = P;
  a.n_blocks = (P + NOV_THREADS - 1) / NOV_THREADS;
  a.mark = nv.mark;
  a.flag = nv.flag;
  a.block_counts = nv.block_counts;
  a.state = nv.state;
  a.cand = nv.cand;
  HIP_TRY(c, hipMemsetAsync(nv.mark, 0, P, c->stream));
  if (total) {
    ProfScope ps(c, "novel_mark", 32.0 * total);
    kn_mark<<<(total + NOV_THREADS - 1) / NOV_THREADS, NOV_THREADS, 0, c->stream>>>(a);
  }
  {
    ProfScope ps(c, "novel_collect", 42.0 * P, 2);
    kn_collect<<<a.n_blocks, NOV_THREADS, 0, c->stream>>>(a);
    kn_emit<<<a.n_blocks, NOV_THREADS, 0, c->stream>>>(a);
  }
  HIP_TRY(c, hipGetLastError());
  return SUMA_OK;
}

int novel_fuse(suma_ctx* c, Novel& nv, uint32_t n, const suma_novel_fuse_params& fp, suma_world_surfel* d_out,
               uint32_t* d_views, uint32_t capacity, uint32_t* counters_h) {
  counters_h[0] = counters_h[1] = counters_h[2] = 0u;
  if (!n) return SUMA_OK;
  hipStream_t st = c->stream;
  int r;
  /* three key arrays 8 n each | seven word arrays 4 n each | counters */
  if ((r = grow(c, nv.scratch, (size_t)n * 52 + 64, {st})) < 0) return r;
  char* base = nv.scratch;
  unsigned long long* key0 = reinterpret_cast<unsigned long long*>(base);
  unsigned long long *keyA = key0 + n, *keyB = keyA + n;
  uint32_t* u0 = reinterpret_cast<uint32_t*>(keyB + n); /* values of a sort, then head flags */
  uint32_t *u1 = u0 + n /* values, then positions */, *u2 = u1 + n, *u3 = u2 + n /* the indices of a sort */;
  uint32_t *order_a = u3 + n /* the first order, kept */, *labels = order_a + n;
  uint32_t* views = labels + n; /* the identity for the second sort, then the views */
  uint32_t* counters = views + n;

  size_t tmp = 0;
  HIP_TRY(c, group_tmp_bytes(n, true, st, &tmp));
  if ((r = grow(c, nv.tmp, tmp, {st})) < 0) return r;
  const size_t bytes = nv.tmp.cap;

  const unsigned blocks = (n + NOV_THREADS - 1) / NOV_THREADS;
  const float4* cand = nv.cand;
  const size_t words = (size_t)n * sizeof(uint32_t);
  HIP_TRY(c, hipMemsetAsync(counters, 0, NOVF_COUNTERS * sizeof(uint32_t), st));
  ProfScope ps(c, "novel_fuse", 200.0 * n, 12);
  kn_key<<<blocks, NOV_THREADS, 0, st>>>(n, cand, fp.voxel_size, key0, u0, labels, u2, views, counters);
  { /* the first order: by timestamp, then by key */
    rocprim::double_buffer<uint32_t> val(u0, u1), idx(u2, u3);
    rocprim::double_buffer<unsigned long long> key(keyA, keyB);
    HIP_TRY(c, group_sort_by_value_then_key(nv.tmp, bytes, val, 32u, key0, key, 64u, idx, n, st));
    HIP_TRY(c, hipMemcpyAsync(order_a, idx.current(), words, hipMemcpyDeviceToDevice, st));
  }
  /* the second order: by label, then by key */
  HIP_TRY(c, hipMemcpyAsync(u0, labels, words, hipMemcpyDeviceToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(u2, views, words, hipMemcpyDeviceToDevice, st));
  rocprim::double_buffer<uint32_t> val(u0, u1), idx(u2, u3);
  rocprim::double_buffer<unsigned long long> key(keyA, keyB);
  HIP_TRY(c, group_sort_by_value_then_key(nv.tmp, bytes, val, 9u, key0, key, 64u, idx, n, st));
  /* the value pair is free now: head flags and positions */
  kn_heads<<<blocks, NOV_THREADS, 0, st>>>(n, key.current(), order_a, cand, fp.min_views, u0, views, counters);
  HIP_TRY(c, group_scan(nv.tmp, bytes, u0, u1, n, st));
  kn_reduce<<<blocks, NOV_THREADS, 0, st>>>(n, key.current(), idx.current(), cand, u0, u1, views, fp.confidence,
                                            reinterpret_cast<float4*>(d_out), d_views, capacity, counters);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(counters_h, counters, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return SUMA_OK;
}
