/*
 * k_objects.hip -- what stands in front of the robot that the map does not contain: while a localiser tracks with novelty
 * on (k_novel.hip), the texels of each scan that no record of the window explains are segmented into objects -- connected
 * components of the wrapped range image -- and each object is reduced to one 64-byte record (class, box, centroid,
 * nearest range).  The records of the last segmentation are what a planner, a tracker or a safety stop consumes; the
 * map, the candidates and every other output of the localiser stay bit-identical.  Nothing in the reference does this.
 *
 * Kernels (VGPRs by tools/isa_stats.py k_objects.hip; none spills, none uses scratch, LDS in bytes):
 *   kob_init     26 VGPRs, LDS 0    lane per texel: the member test of step 1; label = own index or none; a member's
 *                accumulator, the texel's two slots of the vote table and its id are put into their empty state, so a
 *                segmentation needs no memset.
 *   kob_merge    19 VGPRs, LDS 0    lane per member: the four forward neighbours (E, SW, S, SE; the other four are some
 *                other lane's forward ones), the link test of step 2, and a union by atomicMin on the current roots.
 *   kob_flatten  49 VGPRs, LDS 0    lane per member: label = its root; then the member's terms go into the root's
 *                accumulator by integer and ordered-integer atomics, and its vote into the table keyed by (root, label);
 *                a wave whose members share one root adds up in registers first and sends one set of atomics.
 *   kob_vote     14 VGPRs, LDS 16   lane per texel: the texel's two table slots go into their root's best (sum, label) by
 *                a 64-bit atomicMax; members, roots, small and kept roots are counted per block.
 *   kob_emit     36 VGPRs, LDS 36   lane per texel: every block sums the counts of the blocks before it, ranks its kept
 *                roots by wave ballots and writes their records; block 0 writes the counts.  kn_emit's form.
 *   kob_ids      6 VGPRs, LDS 0     lane per member: id = the object number its root was given.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; the helpers of dev_math.h; every
 * comparison is written so that a NaN joins nothing; tests/object_shim.c restates it sequentially, by flood fill, and
 * the library must equal it byte for byte).
 *
 * Parameters (suma_object_params): link_base (0.3 m; finite, >= 0), link_slope (0.03; finite, >= 0), min_texels (5;
 * >= 1), max_objects (4096; 1 .. 65 536).
 * One segmentation takes a data-sized frame (V, N, Sem; W x H texels, W * H <= 2^22), a flag image (one byte a texel),
 * the fp32 pose P of k_change.hip / k_novel.hip (P = T rounded to fp32) and a scan_id.  dv, ds are the texel's vertex and
 * semantic values.
 *   1. MEMBER.  Texel t = ty * W + tx is a member iff flag[t] != 0, dv.w > 0.5f, the three components of m = xyz(dv) are
 *      finite and the three components of w = m4_point(P, m) are finite.  rm = len3(m) (finite or +infinity, never NaN).
 *   2. LINK.  The neighbours of (tx, ty) are the texels (tx + dx mod W, ty + dy), dx, dy in -1 .. 1, not both 0: columns
 *      wrap (the image is a full turn), rows outside the image do not exist.  A texel is never its own neighbour and a
 *      neighbour reached by several (dx, dy) counts once (W = 1: only the texels above and below; W = 2: the other
 *      column's three texels).  Neighbouring members a < b (texel indices: the lower index first) are LINKED iff
 *        len3(sub3(m_a, m_b)) <= link_base + link_slope * fmin_(rm_a, rm_b).
 *      (A product 0 * infinity is a NaN and links nothing.)
 *   3. COMPONENT.  A connected component of the link graph; its root is its smallest texel index; components are ordered
 *      by ascending root.
 *   4. OBJECT.  A component with n_texels >= min_texels.  The objects of one segmentation are numbered 0, 1, ... in
 *      ascending root order; objects with a number >= max_objects are not stored, only counted.
 *   5. THE RECORD (suma_scan_object, 64 bytes): root, n_texels; label, prob: the vote of group_by_key.h over the members
 *      -- a member votes for L = world_label(ds.x) if < 260, else 0, with the weight q = vote_weight(ds.w), summed per
 *      label in uint64; label = the label with the greatest sum, on a tie the smallest id;
 *      prob = (float)sum_label / (float)sum_all; sum_all == 0: label = the root texel's L, prob = 0;
 *      n_dynamic = the members with is_dynamic_label(ds.x * 255.0f); min[3], max[3] = the componentwise fp32 minimum and
 *      maximum of w, where -0 is below +0 (k_grid.hip's order); centroid[a] = (float)((double)S_a / ((double)n_texels *
 *      1024.0)) with S_a = the int64 sum over the members of (int64)rintf(fclamp(w_a * 1024.0f, -2^40, 2^40)) -- the
 *      clamp bounds a term by 2^40 and the texel count bounds the sum by 2^62, so S cannot overflow; positions within
 *      2^30 m of the origin are not touched by it; an integer sum does not depend on the order; r_min = the smallest rm;
 *      scan_id.
 *   6. ID IMAGE.  One uint32 a texel: the object number of a member of a stored object, else 0xffffffff.
 *   7. COUNTS (suma_object_counts, uint32): n_texels = W * H, n_members, n_components, n_small (components below
 *      min_texels), n_objects, stored = min(n_objects, max_objects).  n_small + n_objects = n_components.
 * Open points, fixed here: H = 1 has no rows above or below, the neighbours are the two in the row.  W = 1 and W = 2 as
 * in step 2.  A flagged texel that is not a member belongs to nothing, links nothing and has id 0xffffffff.  min_texels
 * larger than the image: every component is small, no object.  A frame of more than 2^22 texels is refused.
 *
 * Decomposition.  Label-equivalence union-find on the texel grid: a label is the index of another member of the same
 * component, never greater than the texel's own.  A find follows strictly decreasing labels; a union attaches the greater
 * of two roots to the smaller by atomicMin and, when some other lane has attached it first, goes on from where that lane
 * attached it -- again strictly decreasing.  Every loop is bounded by the texel index it starts from; no lane or block
 * ever waits for another: no spinning, no cooperative launch, no grid barrier.  When kob_merge has ended, every edge has
 * been united, a tree's root is its smallest index, and so the labelling does not depend on the order of the atomics.
 * The reduction is by atomics per root rather than by the sorted walk of k_group.hip: an object is hundreds to thousands
 * of texels (a voxel of the fusion is a handful), and one lane walking such a run is a chain of dependent gathers; and
 * the two radix sorts and the scan of that path are some twenty launches of their own at a size (131 072 texels at
 * 64 x 2048) where a launch costs more than the bytes it moves.  All terms are integers, or floats mapped to integers in
 * their order, so atomics give the same bytes in any order.  The vote needs a sum per (root, label): an open-addressing
 * table of 2 P slots keyed by root * 512 + L + 1, a slot claimed by atomicCAS and probed linearly -- a probe that finds
 * a slot taken moves on, it does not wait; there are at most P distinct keys, so a free slot exists.  Six launches a
 * segmentation, each needed by a dependency that spans the grid: labels before unions, all unions before a root is final,
 * all sums before a maximum over them, all block counts before a rank, all ranks before an id.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"
#include "draw_vertex.h"
#include "group_by_key.h"

#define OB_THREADS 256
#define OB_NONE 0xffffffffu
enum { OB_MEMBERS = 0, OB_ROOTS, OB_SMALL, OB_KEPT, OB_BLOCK_WORDS = 4 };

struct ObjArgs {
  const float4 *V, *Sem;
  const uint8_t* flag;
  m4 P;
  int32_t W, H;
  uint32_t n_texels, n_blocks, table;
  float link_base, link_slope;
  uint32_t min_texels, max_objects, scan_id;
  uint32_t* label;
  ObjAcc* acc;
  uint32_t* hkey;
  unsigned long long* hsum;
  uint32_t* block_counts;
  uint32_t* state;
  float4* rec; /* 4 float4 a record */
  uint32_t* ids;
};

/* a float as an integer of the same order, -0 below +0 (grid_ordered_float inverts it) */
SDEV uint32_t ob_ordered(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SDEV float ob_unordered(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

SDEV uint32_t ob_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
/* labels only ever decrease: at most x steps */
SDEV uint32_t ob_find(const uint32_t* label, uint32_t x) {
  uint32_t p;
  while ((p = ob_load(label + x)) != x) x = p;
  return x;
}
/* max(a, b) decreases with every turn that does not return */
SDEV void ob_unite(uint32_t* label, uint32_t a, uint32_t b) {
  for (;;) {
    a = ob_find(label, a);
    b = ob_find(label, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t s = a;
      a = b, b = s;
    }
    const uint32_t old = atomicMin(label + a, b);
    if (old == a) return; /* a was a root and hangs below b now */
    a = old;              /* another lane has attached a below old < a: old and b remain to be united */
  }
}

SDEV bool ob_member(const ObjArgs& a, uint32_t t, float4 dv, v3* w) {
  const v3 m = xyz(dv);
  *w = m4_point(a.P.m, m);
  const bool fin = finite_f(m.x) && finite_f(m.y) && finite_f(m.z) && finite_f(w->x) && finite_f(w->y) && finite_f(w->z);
  return (a.flag[t] != 0) & (dv.w > 0.5f) & fin;
}

__global__ void __launch_bounds__(OB_THREADS) kob_init(ObjArgs a) {
  const uint32_t t = blockIdx.x * OB_THREADS + threadIdx.x;
  if (t >= a.n_texels) return;
  v3 w;
  const bool member = ob_member(a, t, a.V[t], &w);
  a.label[t] = member ? t : OB_NONE;
  a.ids[t] = OB_NONE;
  a.hkey[2 * (size_t)t] = 0u, a.hkey[2 * (size_t)t + 1] = 0u;
  a.hsum[2 * (size_t)t] = 0ull, a.hsum[2 * (size_t)t + 1] = 0ull;
  if (member) {
    ObjAcc z;
    z.n = 0u, z.n_dyn = 0u, z.obj = OB_NONE, z.rmin = 0xffffffffu;
    z.mn[0] = z.mn[1] = z.mn[2] = 0xffffffffu, z.pad0 = 0u;
    z.mx[0] = z.mx[1] = z.mx[2] = 0u, z.pad1 = 0u;
    z.S[0] = z.S[1] = z.S[2] = 0ull, z.sum_all = 0ull, z.best = 0ull, z.pad2 = 0ull;
    a.acc[t] = z;
  }
}

__global__ void __launch_bounds__(OB_THREADS) kob_merge(ObjArgs a) {
  const uint32_t t = blockIdx.x * OB_THREADS + threadIdx.x;
  if (t >= a.n_texels || ob_load(a.label + t) == OB_NONE) return;
  const int32_t W = a.W, H = a.H;
  const int32_t tx = (int32_t)(t % (uint32_t)W), ty = (int32_t)(t / (uint32_t)W);
  const v3 mt = xyz(a.V[t]);
  const float rt = len3(mt);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t dx = (k == 1) ? -1 : ((k == 2) ? 0 : 1), dy = (k == 0) ? 0 : 1;
    const int32_t y = ty + dy;
    if (y >= H) continue;
    int32_t x = tx + dx;
    x = (x < 0) ? x + W : ((x >= W) ? x - W : x);
    const uint32_t u = (uint32_t)y * (uint32_t)W + (uint32_t)x; /* < n_texels */
    if (u == t || ob_load(a.label + u) == OB_NONE) continue;
    const v3 mu = xyz(a.V[u]);
    const float ru = len3(mu);
    const bool t_first = t < u;
    const v3 ma = t_first ? mt : mu, mb = t_first ? mu : mt;
    const float ra = t_first ? rt : ru, rb = t_first ? ru : rt;
    if (len3(sub3(ma, mb)) <= a.link_base + a.link_slope * fmin_(ra, rb)) ob_unite(a.label, t, u);
  }
}

/* the sum / minimum / maximum over the 64 lanes of a wave: every lane takes part, with the identity where it has no term */
SDEV unsigned long long ob_wave_add(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
SDEV uint32_t ob_wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
SDEV uint32_t ob_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

/* q onto the sum of (root r, label L) in the vote table */
SDEV void ob_vote_add(const ObjArgs& a, uint32_t r, uint32_t L, unsigned long long q) {
  const uint32_t key = r * 512u + L + 1u; /* r < 2^22: below 2^31 + 512 */
  uint32_t s = (key * 2654435761u) % a.table;
  for (uint32_t probe = 0; probe < a.table; ++probe) {
    const uint32_t old = atomicCAS(a.hkey + s, 0u, key);
    if (old == 0u || old == key) {
      atomicAdd(a.hsum + s, q);
      return;
    }
    s = (s + 1u == a.table) ? 0u : s + 1u;
  }
}

/* A wave whose members all have one root -- 64 consecutive texels of a row inside one object, the common case -- adds
 * its terms up in registers first and sends one set of atomics instead of 64: many lanes on one 96-byte accumulator
 * serialise (measured: 17.2 ms for one component of 131 072 members without this).  Integer sums, minima and maxima:
 * the bytes are the same either way.  Every lane stays to the end of the wave's work, so the shuffles see all 64. */
__global__ void __launch_bounds__(OB_THREADS) kob_flatten(ObjArgs a) {
  const uint32_t t = blockIdx.x * OB_THREADS + threadIdx.x;
  const bool member = t < a.n_texels && ob_load(a.label + t) != OB_NONE;
  const unsigned long long act = __ballot(member);
  if (act == 0ull) return; /* the whole wave */
  uint32_t r = OB_NONE, dyn = 0u, omn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, omx[3] = {0u, 0u, 0u};
  uint32_t ormin = 0xffffffffu, L = 0u, q = 0u;
  unsigned long long S[3] = {0ull, 0ull, 0ull};
  if (member) {
    r = ob_find(a.label, t); /* final: every union has been made */
    __hip_atomic_store(a.label + t, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float4 dv = a.V[t], ds = a.Sem[t];
    const v3 m = xyz(dv);
    const v3 w = m4_point(a.P.m, m);
    const float wk[3] = {w.x, w.y, w.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      omn[k] = omx[k] = ob_ordered(wk[k]);
      S[k] = (unsigned long long)(long long)__builtin_rintf(fclamp(wk[k] * 1024.0f, -1099511627776.0f, 1099511627776.0f));
    }
    ormin = ob_ordered(len3(m));
    dyn = is_dynamic_label(ds.x * 255.0f) ? 1u : 0u;
    const uint32_t wl = world_label(ds.x);
    L = wl < 260u ? wl : 0u;
    q = vote_weight(ds.w);
  }
  const uint32_t lane = threadIdx.x & 63u, first = (uint32_t)__ffsll((long long)act) - 1u;
  const uint32_t r0 = (uint32_t)__shfl((int)r, (int)first, 64);
  if (__ballot(member && r != r0) == 0ull) { /* one root in this wave */
    const uint32_t n = (uint32_t)__popcll(act), nd = (uint32_t)__popcll(__ballot(dyn != 0u));
    const unsigned long long sum_all = ob_wave_add((unsigned long long)q);
#pragma unroll
    for (int k = 0; k < 3; ++k) omn[k] = ob_wave_min(omn[k]), omx[k] = ob_wave_max(omx[k]), S[k] = ob_wave_add(S[k]);
    ormin = ob_wave_min(ormin);
    if (lane == first) {
      ObjAcc* c = a.acc + r0;
      atomicAdd(&c->n, n);
      if (nd) atomicAdd(&c->n_dyn, nd);
#pragma unroll
      for (int k = 0; k < 3; ++k) atomicMin(&c->mn[k], omn[k]), atomicMax(&c->mx[k], omx[k]), atomicAdd(&c->S[k], S[k]);
      atomicMin(&c->rmin, ormin);
      if (sum_all) atomicAdd(&c->sum_all, sum_all);
    }
    /* the vote: one add per distinct label, for up to four labels; a wave with more sends the rest lane by lane */
    unsigned long long rest = __ballot(member && q != 0u); /* a weight of 0 adds to no sum */
    for (int it = 0; it < 4 && rest != 0ull; ++it) {
      const uint32_t l0 = (uint32_t)__shfl((int)L, __ffsll((long long)rest) - 1, 64);
      const bool in = ((rest >> lane) & 1ull) != 0ull && L == l0;
      const unsigned long long sum = ob_wave_add(in ? (unsigned long long)q : 0ull);
      if (lane == first) ob_vote_add(a, r0, l0, sum);
      rest &= ~__ballot(in);
    }
    if ((rest >> lane) & 1ull) ob_vote_add(a, r0, L, (unsigned long long)q);
    return;
  }
  if (!member) return;
  ObjAcc* c = a.acc + r;
  atomicAdd(&c->n, 1u);
  if (dyn) atomicAdd(&c->n_dyn, 1u);
#pragma unroll
  for (int k = 0; k < 3; ++k) atomicMin(&c->mn[k], omn[k]), atomicMax(&c->mx[k], omx[k]), atomicAdd(&c->S[k], S[k]);
  atomicMin(&c->rmin, ormin);
  if (q) {
    atomicAdd(&c->sum_all, (unsigned long long)q);
    ob_vote_add(a, r, L, (unsigned long long)q);
  }
}

__global__ void __launch_bounds__(OB_THREADS) kob_vote(ObjArgs a) {
  __shared__ uint32_t tot[OB_BLOCK_WORDS];
  if (threadIdx.x < OB_BLOCK_WORDS) tot[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t t = blockIdx.x * OB_THREADS + threadIdx.x;
  bool member = false, root = false, kept = false;
  if (t < a.n_texels) {
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      const size_t s = 2 * (size_t)t + k;
      const uint32_t key = a.hkey[s];
      if (key) { /* sum < 2^22 * 65535 < 2^38: the packed word orders by sum, then by the smaller label */
        const uint32_t r = (key - 1u) >> 9, L = (key - 1u) & 511u;
        atomicMax(&a.acc[r].best, (a.hsum[s] << 9) | (unsigned long long)(511u - L));
      }
    }
    const uint32_t lab = a.label[t];
    member = lab != OB_NONE;
    root = lab == t;
    kept = root && a.acc[t].n >= a.min_texels;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long bm = __ballot(member), br = __ballot(root), bk = __ballot(kept);
  if (lane == 0) {
    if (bm) atomicAdd(&tot[OB_MEMBERS], (uint32_t)__popcll(bm));
    if (br) atomicAdd(&tot[OB_ROOTS], (uint32_t)__popcll(br)), atomicAdd(&tot[OB_SMALL], (uint32_t)__popcll(br & ~bk));
    if (bk) atomicAdd(&tot[OB_KEPT], (uint32_t)__popcll(bk));
  }
  __syncthreads();
  if (threadIdx.x < OB_BLOCK_WORDS) a.block_counts[(size_t)blockIdx.x * OB_BLOCK_WORDS + threadIdx.x] = tot[threadIdx.x];
}

__global__ void __launch_bounds__(OB_THREADS) kob_emit(ObjArgs a) {
  __shared__ uint32_t s_pre, s_sum[OB_BLOCK_WORDS], s_wave[OB_THREADS / 64];
  if (threadIdx.x == 0) s_pre = 0u;
  if (threadIdx.x < OB_BLOCK_WORDS) s_sum[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t pre = 0, sum[OB_BLOCK_WORDS] = {0, 0, 0, 0};
  for (uint32_t b = threadIdx.x; b < a.n_blocks; b += OB_THREADS) {
#pragma unroll
    for (uint32_t k = 0; k < OB_BLOCK_WORDS; ++k) sum[k] += a.block_counts[(size_t)b * OB_BLOCK_WORDS + k];
    pre += (b < blockIdx.x) ? a.block_counts[(size_t)b * OB_BLOCK_WORDS + OB_KEPT] : 0u;
  }
  if (pre) atomicAdd(&s_pre, pre);
#pragma unroll
  for (uint32_t k = 0; k < OB_BLOCK_WORDS; ++k)
    if (sum[k]) atomicAdd(&s_sum[k], sum[k]);
  const uint32_t t = blockIdx.x * OB_THREADS + threadIdx.x;
  ObjAcc c;
  bool kept = false;
  if (t < a.n_texels && a.label[t] == t) {
    c = a.acc[t];
    kept = c.n >= a.min_texels;
  }
  const unsigned long long bal = __ballot(kept);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t o = s_pre + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
  for (uint32_t wv = 0; wv < wave; ++wv) o += s_wave[wv];
  if (kept && o < a.max_objects) {
    uint32_t label;
    float prob = 0.0f;
    if (c.sum_all != 0ull) {
      label = 511u - (uint32_t)(c.best & 511ull);
      prob = (float)(c.best >> 9) / (float)c.sum_all;
    } else {
      const uint32_t wl = world_label(a.Sem[t].x);
      label = wl < 260u ? wl : 0u;
    }
    float cen[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) cen[k] = (float)((double)(long long)c.S[k] / ((double)c.n * 1024.0));
    float4* dst = a.rec + 4 * (size_t)o;
    dst[0] = f4(__uint_as_float(t), __uint_as_float(c.n), __uint_as_float(label), prob);
    dst[1] = f4(__uint_as_float(c.n_dyn), ob_unordered(c.mn[0]), ob_unordered(c.mn[1]), ob_unordered(c.mn[2]));
    dst[2] = f4(ob_unordered(c.mx[0]), ob_unordered(c.mx[1]), ob_unordered(c.mx[2]), cen[0]);
    dst[3] = f4(cen[1], cen[2], ob_unordered(c.rmin), __uint_as_float(a.scan_id));
    a.acc[t].obj = o;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t n_objects = s_sum[OB_KEPT];
    a.state[0] = a.n_texels;
    a.state[1] = s_sum[OB_MEMBERS];
    a.state[2] = s_sum[OB_ROOTS];
    a.state[3] = s_sum[OB_SMALL];
    a.state[4] = n_objects;
    a.state[5] = n_objects < a.max_objects ? n_objects : a.max_objects;
  }
}

__global__ void __launch_bounds__(OB_THREADS) kob_ids(ObjArgs a) {
  const uint32_t t = blockIdx.x * OB_THREADS + threadIdx.x;
  if (t >= a.n_texels) return;
  const uint32_t r = a.label[t];
  if (r != OB_NONE) a.ids[t] = a.acc[r].obj;
}

/* ---- host side ---- */
int objects_alloc(suma_ctx* c, Objects& ob, const suma_object_params& op, uint32_t P) {
  const size_t blocks = ((size_t)P + OB_THREADS - 1) / OB_THREADS;
  Objects nw;
  hipError_t e = nw.label.alloc(P);
  if (e == hipSuccess) e = nw.acc.alloc(P);
  if (e == hipSuccess) e = nw.hkey.alloc(2 * (size_t)P);
  if (e == hipSuccess) e = nw.hsum.alloc(2 * (size_t)P);
  if (e == hipSuccess) e = nw.block_counts.alloc(OB_BLOCK_WORDS * blocks);
  if (e == hipSuccess) e = nw.state.alloc(8);
  if (e == hipSuccess) e = nw.rec.alloc(4 * (size_t)op.max_objects);
  if (e == hipSuccess) e = nw.ids.alloc(P);
  if (e == hipSuccess) e = nw.flags_in.alloc(P);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SUMA_ERR_NOMEM, "suma_localizer_enable_objects: no device memory for " + std::to_string(P) + " texels");
  }
  nw.n_texels = P;
  ob = std::move(nw);
  return SUMA_OK;
}

int objects_segment(suma_ctx* c, Objects& ob, const suma_frame* f, const uint8_t* d_flags, const double T[16],
                    uint32_t scan_id) {
  const uint32_t P = ob.n_texels;
  ObjArgs a;
  a.V = f->map[SUMA_MAP_VERTEX];
  a.Sem = f->map[SUMA_MAP_SEMANTIC];
  a.flag = d_flags;
  mat4_cast_f(T, a.P.m);
  a.W = f->width, a.H = f->height;
  a.n_texels = P;
  a.n_blocks = (P + OB_THREADS - 1) / OB_THREADS;
  a.table = 2u * P;
  a.link_base = ob.op.link_base, a.link_slope = ob.op.link_slope;
  a.min_texels = ob.op.min_texels, a.max_objects = ob.op.max_objects, a.scan_id = scan_id;
  a.label = ob.label;
  a.acc = ob.acc;
  a.hkey = ob.hkey;
  a.hsum = ob.hsum;
  a.block_counts = ob.block_counts;
  a.state = ob.state;
  a.rec = ob.rec;
  a.ids = ob.ids;
  {
    ProfScope ps(c, "objects_label", 150.0 * P, 3);
    kob_init<<<a.n_blocks, OB_THREADS, 0, c->stream>>>(a);
    kob_merge<<<a.n_blocks, OB_THREADS, 0, c->stream>>>(a);
    kob_flatten<<<a.n_blocks, OB_THREADS, 0, c->stream>>>(a);
  }
  {
    ProfScope ps(c, "objects_reduce", 40.0 * P, 3);
    kob_vote<<<a.n_blocks, OB_THREADS, 0, c->stream>>>(a);
    kob_emit<<<a.n_blocks, OB_THREADS, 0, c->stream>>>(a);
    kob_ids<<<a.n_blocks, OB_THREADS, 0, c->stream>>>(a);
  }
  HIP_TRY(c, hipGetLastError());
  return SUMA_OK;
}
