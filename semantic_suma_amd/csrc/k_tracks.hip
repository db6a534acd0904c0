/*
 * k_tracks.hip -- the objects of one scan tied to those of the scans before: with objects on (k_objects.hip), every
 * segmentation is followed by one tracker update that joins the scan's object records into detections, associates the
 * detections to the tracks, filters position and velocity, lets unmatched tracks coast and expire and founds new tracks.
 * It reads the segmentation's records, not texels, and writes nothing any other output of the localiser reads.  Nothing
 * in the reference does this.
 *
 * Kernels (VGPRs by tools/isa_stats.py k_tracks.hip; none spills, none uses scratch, LDS in bytes):
 *   ktr_init     20 VGPRs, LDS 0        lane per object: its union-find label = its own index, its accumulator into the
 *                empty state.
 *   ktr_join     26 VGPRs, LDS 8192     block per pair of tiles of 256 objects (the lower triangle, dealt round robin to
 *                a fixed grid): the column tile's boxes in LDS, a lane per row object, the join test of step 1, a union
 *                by atomicMin on the current roots (k_objects.hip's decreasing-label union-find).
 *   ktr_reduce   20 VGPRs, LDS 0        lane per object: label = its root; its terms into the root's accumulator by
 *                integer and ordered-integer atomics.
 *   ktr_track    72 VGPRs, LDS 123 000  ONE workgroup of 1024 lanes, the predicted positions, gates and picks of the
 *                table in LDS: numbers the detections (block scans), predicts, runs the rounds of step 3 over block
 *                barriers, updates the slots (a lane per slot), ranks the free slots and the unmatched detections (block
 *                scans), founds the new tracks, compacts the live tracks and writes the per-object ids and the counts.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; the helpers of dev_math.h;
 * tests/track_shim.c restates it sequentially and the library must equal it byte for byte).
 *
 * Parameters (suma_track_params): join_dist (2 m; not NaN, <= 1e6; negative: joining off), gate_base (1.5 m; 0 .. 1e6),
 * gate_speed (0.5 m a step; 0 .. 1e6), alpha (0.5; 0 .. 1), beta (0.2; 0 .. 2), confirm_hits (3; 1 .. 65 535),
 * max_missed (3; 0 .. 65 535), max_tracks (1024; 1 .. 4096), max_rounds (16; 1 .. 64).
 * State: max_tracks slots (suma_object_track, 112 bytes; state 0 = free), last_stamp (0 = no update yet), next_id (1).
 * One update takes n object records (suma_scan_object; the first min(n_objects, max_objects) of a segmentation, in their
 * order) and the stamp s = scan_id + 1 (uint32).  STAMP RULE: an update whose stamp is not above last_stamp is refused
 * in front of everything its call would launch (k_live.hip's rule).  dt = (float)(s - last_stamp).
 *   1. JOIN.  Objects a < b (indices) are JOINED iff label_a == label_b, the six box components of both are finite,
 *      join_dist is not negative and len3(g) <= join_dist with g[k] = fmax_(fmax_(0, a.min[k] - b.max[k]),
 *      b.min[k] - a.max[k]).  A DETECTION is a connected component of that graph; detections are numbered 0, 1, ... in
 *      ascending order of their smallest object index.  Its record: label; n_objects = the members; n_texels, n_dynamic
 *      = the members' sums, taken in uint64 and saturated at 2^32 - 1; min[3], max[3] = the componentwise minimum and
 *      maximum over the members in the order of the floats' bits mapped to ordered integers, -0 below +0 (k_grid.hip's
 *      order; a total order, so a NaN has a place in it too); r_min = the smallest in the same order;
 *      centroid[k] = (float)((double)S_k / ((double)W * 1024.0)), S_k = the int64 sum over the members of
 *      w * (int64)rintf(q), q = fclamp(centroid[k] * 1024.0f, -2^24, 2^24), a NaN q counting as 0,
 *      w = min(max(n_texels, 1), 2^22), W = the sum of w.  The clamp is chosen so that 65 536 members of weight 2^22
 *      stay below 2^16 * 2^22 * 2^24 = 2^62: the sum cannot overflow; positions within 2^14 m of the origin are not
 *      touched by it, and beyond that distance fp32 itself is coarser than 1/1024 m.  An integer sum does not depend on
 *      the order.  obj_det[i] = the detection of object i.
 *   2. PREDICT.  Every live slot t (state != 0): step = velocity * dt, p_pred = position + step (componentwise);
 *      gate_t = gate_base + gate_speed * (float)(s - last_matched_t).
 *   3. ASSOCIATE.  dist(t, d) = len3(sub3(c_d, p_pred_t)); the pair is GATED iff dist <= gate_t (a NaN is not).  Key of
 *      a pair: (bits of dist, t, d), compared lexicographically.  Round r = 0, 1, ...: every unmatched detection picks
 *      its smallest-key gated unmatched live slot, every unmatched live slot its smallest-key gated unmatched detection;
 *      c = the detections that have a pick.  If c == 0 or r == max_rounds: n_unresolved = c, rounds = r, the association
 *      ends.  Otherwise mutual picks are matched and the next round follows.  (The pair of the smallest key is always
 *      mutual: while c > 0 every round matches, and without the cap the result is greedy matching in ascending key
 *      order.)
 *   4. UPDATE.  A matched slot, with res = c_d - p_pred: hits == 1: position = c_d, velocity = res / dt (a division per
 *      component); otherwise position = p_pred + alpha * res, velocity = velocity + (beta / dt) * res (the quotient, then
 *      the product, then the sum).  hits += 1 up to 65 535, missed = 0, label, n_texels, n_dynamic, n_objects, min, max,
 *      r_min from the detection, last_matched = s, detection = d, state = confirmed once hits >= confirm_hits (and it
 *      stays).  An unmatched live slot: position = p_pred, missed += 1, detection = 0xffffffff; missed > max_missed: the
 *      slot becomes free, all of its 112 bytes zero.  Then the unmatched detections, in ascending order, take the free
 *      slots (those of this update's expiries included), in ascending order: all bytes zero, then id = next_id + rank,
 *      slot, position = origin = c_d, velocity = 0, hits = 1, missed = 0, first_stamp = last_matched = s, the detection's
 *      fields, detection = d, state = confirmed iff 1 >= confirm_hits, else tentative.  next_id += n_born.  Detections
 *      beyond the free slots are dropped and counted.  last_stamp = s.
 *   5. OUTPUTS.  The live slots in ascending slot order; obj_track[i] = the id of the track detection obj_det[i] matched
 *      or founded, 0 for a dropped one; the counts (suma_track_counts): n_objects = n, n_detections, n_joined =
 *      n - n_detections, n_tracks_before, n_matched, n_missed (unmatched live slots, the expired among them), n_expired,
 *      n_born, n_dropped, n_confirmed (confirmed tracks afterwards), n_unresolved, rounds.  n_detections = n_matched +
 *      n_born + n_dropped; n_tracks_before = n_matched + n_missed.
 * Open points, fixed here: the weights and saturations of step 1; an object with a non-finite box joins nothing but is a
 * detection of its own; `detection` of a new track is its founding detection; hits saturates at 65 535; ids are uint32
 * and would wrap after 2^32 - 1 births (not guarded); a free slot keeps whatever bytes an uploaded state gave it until it
 * is taken; n = 0 is an update like any other (every track is unmatched); the gate's terms are bounded by the parameter
 * ranges, so a track with a non-finite position or velocity has an infinite or NaN distance to everything, is never
 * matched and expires.
 *
 * Decomposition.  The join is k_objects.hip's label-equivalence union-find over object pairs instead of texel
 * neighbours: a find follows strictly decreasing labels, a union attaches the greater root below the smaller by
 * atomicMin and goes on from where another lane attached it first; no lane waits for another.  All n (n - 1) / 2 pairs
 * are tested; the object count is a device word the host never sees, so the grids are fixed and sized by max_objects,
 * and blocks without work end at once.  The rounds of the association depend on the data and the host may not look, so
 * they close inside one launch: one workgroup, block barriers, 112 KiB of LDS for the table's predictions (64), the
 * slots' picks (32) and matches (16) and 8 for the list of live slots.  A detection's pick is the minimum over the live
 * slots of a 64-bit word (bits of dist << 32 | slot); the same pass sends (bits of dist << 32 | detection) into the
 * slot's pick by an LDS atomicMin, so one pass over the gated pairs serves both sides, and a pick is mutual iff the slot's
 * word names the detection.  Minima and integer sums: the bytes do not depend on the order.  Everything one lane of
 * ktr_track writes to global memory for another lane of it to read goes through relaxed agent-scope atomics with a block
 * barrier between.  Four launches an update.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"
#include "draw_vertex.h"

#define TK_THREADS 256
#define TK_JOIN_BLOCKS 256
#define TK_BLOCK 1024
#define TK_MAX_TRACKS 4096
#define TK_NONE 0xffffffffu
#define TK_DEAD 0xfffffffeu
#define TK_DET_WORDS 16
enum { TD_LABEL = 0, TD_COUNT, TD_NTEX, TD_NDYN, TD_MIN, TD_MAX = 7, TD_CEN = 10, TD_RMIN = 13 };

struct TrkArgs {
  const uint32_t* rec; /* 16 words a record */
  const uint32_t* n_ptr;
  uint32_t max_objects, s, steps; /* steps = s - last_stamp */
  suma_track_params tp;
  uint32_t* parent;
  TrkAcc* acc;
  uint32_t* det; /* TK_DET_WORDS a detection */
  uint32_t *objdet, *objtrack, *detmatch, *dettrack;
  unsigned long long* detpick;
  suma_object_track *slots, *out;
  uint32_t* words;
};

SDEV uint32_t tk_ordered(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SDEV uint32_t tk_unordered(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o; }
SDEV uint32_t tk_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
SDEV void tk_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
SDEV uint32_t tk_count(const TrkArgs& a) {
  const uint32_t n = *a.n_ptr;
  return n < a.max_objects ? n : a.max_objects;
}
/* labels only ever decrease: at most x steps */
SDEV uint32_t tk_find(const uint32_t* parent, uint32_t x) {
  uint32_t p;
  while ((p = tk_ld(parent + x)) != x) x = p;
  return x;
}
/* max(a, b) decreases with every turn that does not return */
SDEV void tk_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = tk_find(parent, a);
    b = tk_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t s = a;
      a = b, b = s;
    }
    const uint32_t old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(TK_THREADS) ktr_init(TrkArgs a) {
  const uint32_t n = tk_count(a);
  for (uint32_t i = blockIdx.x * TK_THREADS + threadIdx.x; i < n; i += gridDim.x * TK_THREADS) {
    a.parent[i] = i;
    TrkAcc z;
    z.count = 0u, z.rmin = 0xffffffffu;
    z.mn[0] = z.mn[1] = z.mn[2] = 0xffffffffu;
    z.mx[0] = z.mx[1] = z.mx[2] = 0u;
    z.ntex = z.ndyn = z.W = 0ull;
    z.S[0] = z.S[1] = z.S[2] = 0ull;
    a.acc[i] = z;
  }
}

struct TkBox {
  float mn[3], mx[3];
  uint32_t label, ok;
};
SDEV TkBox tk_box(const uint32_t* rec, uint32_t i) {
  const uint32_t* r = rec + 16 * (size_t)i;
  TkBox b;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b.mn[k] = __uint_as_float(r[5 + k]), b.mx[k] = __uint_as_float(r[8 + k]);
    ok = ok && finite_f(b.mn[k]) && finite_f(b.mx[k]);
  }
  b.label = r[2];
  b.ok = ok ? 1u : 0u;
  return b;
}

__global__ void __launch_bounds__(TK_THREADS) ktr_join(TrkArgs a) {
  __shared__ TkBox tile[TK_THREADS];
  const uint32_t n = tk_count(a);
  if (a.tp.join_dist < 0.0f || n < 2u) return;
  const uint32_t R = (n + TK_THREADS - 1) / TK_THREADS;
  uint32_t u = 0, next = blockIdx.x;
  for (uint32_t ti = 0; ti < R; ++ti)
    for (uint32_t tj = 0; tj <= ti; ++tj, ++u) {
      if (u != next) continue; /* uniform over the block */
      next += gridDim.x;
      __syncthreads();
      const uint32_t jl = tj * TK_THREADS + threadIdx.x;
      if (jl < n) tile[threadIdx.x] = tk_box(a.rec, jl);
      __syncthreads();
      const uint32_t i = ti * TK_THREADS + threadIdx.x;
      if (i >= n) continue;
      const TkBox bi = tk_box(a.rec, i);
      if (!bi.ok) continue;
      for (uint32_t jj = 0; jj < TK_THREADS; ++jj) {
        const uint32_t j = tj * TK_THREADS + jj;
        if (j >= i) break; /* i < n: j < n too */
        const TkBox bj = tile[jj];
        if (!bj.ok || bj.label != bi.label) continue;
        /* a = the lower index j, b = i */
        v3 g;
        g.x = fmax_(fmax_(0.0f, bj.mn[0] - bi.mx[0]), bi.mn[0] - bj.mx[0]);
        g.y = fmax_(fmax_(0.0f, bj.mn[1] - bi.mx[1]), bi.mn[1] - bj.mx[1]);
        g.z = fmax_(fmax_(0.0f, bj.mn[2] - bi.mx[2]), bi.mn[2] - bj.mx[2]);
        if (len3(g) <= a.tp.join_dist) tk_unite(a.parent, i, j);
      }
    }
}

__global__ void __launch_bounds__(TK_THREADS) ktr_reduce(TrkArgs a) {
  const uint32_t n = tk_count(a);
  for (uint32_t i = blockIdx.x * TK_THREADS + threadIdx.x; i < n; i += gridDim.x * TK_THREADS) {
    const uint32_t r = tk_find(a.parent, i); /* final: every union has been made */
    tk_st(a.parent + i, r);
    const uint32_t* o = a.rec + 16 * (size_t)i;
    TrkAcc* c = a.acc + r;
    const uint32_t nt = o[1];
    const unsigned long long w = nt < 1u ? 1u : (nt > (1u << 22) ? (1u << 22) : nt);
    atomicAdd(&c->count, 1u);
    atomicAdd(&c->ntex, (unsigned long long)nt);
    atomicAdd(&c->ndyn, (unsigned long long)o[4]);
    atomicAdd(&c->W, w);
    atomicMin(&c->rmin, tk_ordered(__uint_as_float(o[14])));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(&c->mn[k], tk_ordered(__uint_as_float(o[5 + k])));
      atomicMax(&c->mx[k], tk_ordered(__uint_as_float(o[8 + k])));
      float q = fclamp(__uint_as_float(o[11 + k]) * 1024.0f, -16777216.0f, 16777216.0f);
      if (q != q) q = 0.0f;
      const long long term = (long long)w * (long long)__builtin_rintf(q);
      atomicAdd(&c->S[k], (unsigned long long)term);
    }
  }
}

/* the exclusive prefix of flag over the block's 1024 lanes in lane order, and the block's total; every lane calls it */
SDEV uint32_t tk_scan(uint32_t flag, uint32_t* s_wave, uint32_t* total) {
  const uint32_t incl = wave_inclusive_scan(flag);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 63u) s_wave[wave] = incl;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < TK_BLOCK / 64; ++w) {
    const uint32_t v = s_wave[w];
    tot += v;
    pre += (w < wave) ? v : 0u;
  }
  __syncthreads();
  *total = tot;
  return pre + incl - flag;
}

enum { TC_OBJECTS = 0, TC_DETECTIONS, TC_JOINED, TC_BEFORE, TC_MATCHED, TC_MISSED, TC_EXPIRED, TC_BORN, TC_DROPPED,
       TC_CONFIRMED, TC_UNRESOLVED, TC_ROUNDS };

SDEV uint32_t tk_detu(const uint32_t* det, uint32_t d, int word) { return tk_ld(det + TK_DET_WORDS * (size_t)d + word); }
SDEV float tk_detf(const uint32_t* det, uint32_t d, int word) { return __uint_as_float(tk_detu(det, d, word)); }
/* a slot as its 28 words in registers (every index a constant once the loops are unrolled), moved as seven uint4 */
enum { TW_ID = 0, TW_SLOT, TW_STATE, TW_LABEL, TW_NTEX, TW_NDYN, TW_NOBJ, TW_HITS, TW_MISSED, TW_FIRST, TW_LAST, TW_POS = 11,
       TW_VEL = 14, TW_ORG = 17, TW_MIN = 20, TW_MAX = 23, TW_RMIN = 26, TW_DET = 27, TW_WORDS = 28 };
static_assert(sizeof(suma_object_track) == 4 * TW_WORDS, "suma_object_track is 28 words");
struct TkSlot {
  uint32_t w[TW_WORDS];
};
SDEV TkSlot tk_slot_load(const suma_object_track* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  TkSlot k;
#pragma unroll
  for (int j = 0; j < TW_WORDS / 4; ++j) {
    const uint4 v = q[j];
    k.w[4 * j] = v.x, k.w[4 * j + 1] = v.y, k.w[4 * j + 2] = v.z, k.w[4 * j + 3] = v.w;
  }
  return k;
}
SDEV void tk_slot_store(suma_object_track* p, const TkSlot& k) {
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int j = 0; j < TW_WORDS / 4; ++j) q[j] = make_uint4(k.w[4 * j], k.w[4 * j + 1], k.w[4 * j + 2], k.w[4 * j + 3]);
}
SDEV TkSlot tk_slot_zero() {
  TkSlot k;
#pragma unroll
  for (int j = 0; j < TW_WORDS; ++j) k.w[j] = 0u;
  return k;
}
/* the detection's fields into a track record */
SDEV void tk_take(TkSlot& k, const uint32_t* det, uint32_t d) {
  k.w[TW_LABEL] = tk_detu(det, d, TD_LABEL), k.w[TW_NOBJ] = tk_detu(det, d, TD_COUNT);
  k.w[TW_NTEX] = tk_detu(det, d, TD_NTEX), k.w[TW_NDYN] = tk_detu(det, d, TD_NDYN);
#pragma unroll
  for (int x = 0; x < 3; ++x) k.w[TW_MIN + x] = tk_detu(det, d, TD_MIN + x), k.w[TW_MAX + x] = tk_detu(det, d, TD_MAX + x);
  k.w[TW_RMIN] = tk_detu(det, d, TD_RMIN);
}

__global__ void __launch_bounds__(TK_BLOCK) ktr_track(TrkArgs a) {
  __shared__ float4 s_pred[TK_MAX_TRACKS];              /* p_pred, gate */
  __shared__ unsigned long long s_best[TK_MAX_TRACKS];  /* a slot's pick: bits of dist << 32 | detection */
  __shared__ uint32_t s_match[TK_MAX_TRACKS];           /* TK_DEAD: no live slot; TK_NONE: unmatched; else the detection */
  __shared__ uint16_t s_list[TK_MAX_TRACKS];            /* the live slots, in any order */
  __shared__ uint32_t s_wave[TK_BLOCK / 64], s_cnt[12], s_nlist, s_cand;
  uint32_t* s_free = reinterpret_cast<uint32_t*>(s_best);    /* after the rounds: the free slots, ascending */
  uint32_t* s_birth = s_free + TK_MAX_TRACKS;                /* ... and per slot the detection that founds a track in it */
  const uint32_t tid = threadIdx.x, T = a.tp.max_tracks, s = a.s;
  const uint32_t n = tk_count(a);
  const uint32_t next_id = a.words[TRK_BORN_TOTAL] + 1u;
  const float dt = (float)a.steps;
  if (tid < 12u) s_cnt[tid] = 0u;
  if (tid == 0u) s_nlist = 0u;
  __syncthreads();

  /* the detections in ascending order of their smallest object */
  uint32_t D = 0;
  for (uint32_t base = 0; base < n; base += TK_BLOCK) {
    const uint32_t i = base + tid;
    const bool root = i < n && a.parent[i] == i;
    uint32_t total;
    const uint32_t k = D + tk_scan(root ? 1u : 0u, s_wave, &total);
    D += total;
    if (root) {
      const TrkAcc c = a.acc[i];
      uint32_t* dst = a.det + TK_DET_WORDS * (size_t)k;
      tk_st(dst + TD_LABEL, a.rec[16 * (size_t)i + 2]);
      tk_st(dst + TD_COUNT, c.count);
      tk_st(dst + TD_NTEX, c.ntex > 0xffffffffull ? 0xffffffffu : (uint32_t)c.ntex);
      tk_st(dst + TD_NDYN, c.ndyn > 0xffffffffull ? 0xffffffffu : (uint32_t)c.ndyn);
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        tk_st(dst + TD_MIN + x, tk_unordered(c.mn[x]));
        tk_st(dst + TD_MAX + x, tk_unordered(c.mx[x]));
        const float cen = (float)((double)(long long)c.S[x] / ((double)c.W * 1024.0));
        tk_st(dst + TD_CEN + x, __float_as_uint(cen));
      }
      tk_st(dst + TD_RMIN, tk_unordered(c.rmin));
      tk_st(a.objdet + i, k);
      tk_st(a.detmatch + k, TK_NONE);
    }
  }
  /* step 2 */
  for (uint32_t t = tid; t < T; t += TK_BLOCK) {
    const TkSlot k = tk_slot_load(a.slots + t);
    uint32_t m = TK_DEAD;
    if (k.w[TW_STATE] != 0u) {
      m = TK_NONE;
      float4 p;
      const float sx = __uint_as_float(k.w[TW_VEL]) * dt, sy = __uint_as_float(k.w[TW_VEL + 1]) * dt,
                  sz = __uint_as_float(k.w[TW_VEL + 2]) * dt;
      p.x = __uint_as_float(k.w[TW_POS]) + sx, p.y = __uint_as_float(k.w[TW_POS + 1]) + sy;
      p.z = __uint_as_float(k.w[TW_POS + 2]) + sz;
      const float age = a.tp.gate_speed * (float)(s - k.w[TW_LAST]);
      p.w = a.tp.gate_base + age;
      s_pred[t] = p;
      s_list[atomicAdd(&s_nlist, 1u)] = (uint16_t)t;
    }
    s_match[t] = m;
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += TK_BLOCK) {
    const uint32_t r = a.parent[i];
    if (r != i) tk_st(a.objdet + i, tk_ld(a.objdet + r));
  }
  const uint32_t n_live = s_nlist;

  /* step 3 */
  uint32_t round = 0;
  for (;; ++round) {
    for (uint32_t t = tid; t < T; t += TK_BLOCK) s_best[t] = ~0ull;
    if (tid == 0u) s_cand = 0u;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t d = tid; d < D; d += TK_BLOCK) {
      unsigned long long best = ~0ull;
      if (n_live != 0u && tk_ld(a.detmatch + d) == TK_NONE) {
        const v3 c = mk3(tk_detf(a.det, d, TD_CEN), tk_detf(a.det, d, TD_CEN + 1), tk_detf(a.det, d, TD_CEN + 2));
        /* the lanes of a wave start at different places of the list, so that they do not all send their atomics to one
         * slot at a time; a slot's pick only ever decreases, so a lane that reads a pick below its own word sends none */
        uint32_t q = tid % n_live;
        for (uint32_t it = 0; it < n_live; ++it, q = (q + 1u == n_live) ? 0u : q + 1u) {
          const uint32_t t = s_list[q];
          if (s_match[t] != TK_NONE) continue;
          const float4 p = s_pred[t];
          const float dist = len3(sub3(c, mk3(p.x, p.y, p.z)));
          if (!(dist <= p.w)) continue;
          const unsigned long long hi = (unsigned long long)__float_as_uint(dist) << 32;
          const unsigned long long key = hi | t;
          best = key < best ? key : best;
          if ((hi | d) < *(volatile unsigned long long*)&s_best[t]) atomicMin(&s_best[t], hi | d);
        }
      }
      a.detpick[d] = best; /* read back by this lane only */
      mine += best != ~0ull ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_cand, mine);
    __syncthreads();
    const uint32_t cand = s_cand;
    if (cand == 0u || round == a.tp.max_rounds) {
      if (tid == 0u) s_cnt[TC_UNRESOLVED] = cand;
      break;
    }
    for (uint32_t d = tid; d < D; d += TK_BLOCK) {
      const unsigned long long pick = a.detpick[d];
      if (pick == ~0ull) continue;
      const uint32_t t = (uint32_t)pick;
      if (s_best[t] == ((pick & 0xffffffff00000000ull) | d)) {
        tk_st(a.detmatch + d, t);
        s_match[t] = d; /* the one detection the slot picked: no other lane writes this word */
      }
    }
    __syncthreads();
  }
  __syncthreads();

  /* step 4: the slots that were alive */
  for (uint32_t t = tid; t < T; t += TK_BLOCK) {
    const uint32_t d = s_match[t];
    s_birth[t] = TK_NONE; /* s_best is no longer read */
    if (d == TK_DEAD) continue;
    TkSlot k = tk_slot_load(a.slots + t);
    const float4 p = s_pred[t];
    const float pp[3] = {p.x, p.y, p.z};
    atomicAdd(&s_cnt[TC_BEFORE], 1u);
    if (d != TK_NONE) {
      const float gain = a.tp.beta / dt;
      const bool second = k.w[TW_HITS] == 1u;
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const float c = tk_detf(a.det, d, TD_CEN + x);
        const float res = c - pp[x];
        const float dp = a.tp.alpha * res, dv = gain * res;
        const float pos = second ? c : pp[x] + dp;
        const float vel = second ? res / dt : __uint_as_float(k.w[TW_VEL + x]) + dv;
        k.w[TW_POS + x] = __float_as_uint(pos), k.w[TW_VEL + x] = __float_as_uint(vel);
      }
      if (k.w[TW_HITS] < 65535u) k.w[TW_HITS] += 1u;
      k.w[TW_MISSED] = 0u;
      tk_take(k, a.det, d);
      k.w[TW_LAST] = s;
      k.w[TW_DET] = d;
      if (k.w[TW_HITS] >= a.tp.confirm_hits) k.w[TW_STATE] = SUMA_TRACK_CONFIRMED;
      tk_st(a.dettrack + d, k.w[TW_ID]);
      atomicAdd(&s_cnt[TC_MATCHED], 1u);
    } else {
#pragma unroll
      for (int x = 0; x < 3; ++x) k.w[TW_POS + x] = __float_as_uint(pp[x]);
      k.w[TW_MISSED] += 1u;
      k.w[TW_DET] = TK_NONE;
      atomicAdd(&s_cnt[TC_MISSED], 1u);
      if (k.w[TW_MISSED] > a.tp.max_missed) {
        k = tk_slot_zero();
        s_match[t] = TK_DEAD;
        atomicAdd(&s_cnt[TC_EXPIRED], 1u);
      }
    }
    tk_slot_store(a.slots + t, k);
  }
  __syncthreads();
  /* the free slots and the unmatched detections, each ranked in ascending order */
  uint32_t n_free = 0;
  for (uint32_t base = 0; base < T; base += TK_BLOCK) {
    const uint32_t t = base + tid;
    const bool fr = t < T && s_match[t] == TK_DEAD;
    uint32_t total;
    const uint32_t k = n_free + tk_scan(fr ? 1u : 0u, s_wave, &total);
    n_free += total;
    if (fr) s_free[k] = t;
  }
  __syncthreads();
  uint32_t n_unmatched = 0;
  for (uint32_t base = 0; base < D; base += TK_BLOCK) {
    const uint32_t d = base + tid;
    const bool un = d < D && tk_ld(a.detmatch + d) == TK_NONE;
    uint32_t total;
    const uint32_t k = n_unmatched + tk_scan(un ? 1u : 0u, s_wave, &total);
    n_unmatched += total;
    if (un) {
      if (k < n_free) {
        const uint32_t f = s_free[k];
        s_birth[f] = d;
        s_match[f] = k; /* the rank, for the id */
      } else {
        tk_st(a.dettrack + d, 0u);
      }
    }
  }
  const uint32_t n_born = n_unmatched < n_free ? n_unmatched : n_free;
  __syncthreads();
  for (uint32_t t = tid; t < T; t += TK_BLOCK) {
    const uint32_t d = s_birth[t];
    if (d == TK_NONE) continue;
    TkSlot k = tk_slot_zero();
    k.w[TW_ID] = next_id + s_match[t];
    k.w[TW_SLOT] = t;
    k.w[TW_STATE] = (1u >= a.tp.confirm_hits) ? SUMA_TRACK_CONFIRMED : SUMA_TRACK_TENTATIVE;
    tk_take(k, a.det, d);
    k.w[TW_HITS] = 1u, k.w[TW_FIRST] = s, k.w[TW_LAST] = s;
#pragma unroll
    for (int x = 0; x < 3; ++x) k.w[TW_POS + x] = k.w[TW_ORG + x] = tk_detu(a.det, d, TD_CEN + x);
    k.w[TW_DET] = d;
    tk_slot_store(a.slots + t, k);
    tk_st(a.dettrack + d, k.w[TW_ID]);
  }
  __syncthreads();
  /* step 5 */
  uint32_t n_out = 0;
  for (uint32_t base = 0; base < T; base += TK_BLOCK) {
    const uint32_t t = base + tid;
    TkSlot k = tk_slot_zero();
    if (t < T) k = tk_slot_load(a.slots + t); /* this lane wrote it */
    const bool live = k.w[TW_STATE] != 0u;
    uint32_t total;
    const uint32_t o = n_out + tk_scan(live ? 1u : 0u, s_wave, &total);
    n_out += total;
    if (live) {
      tk_slot_store(a.out + o, k);
      if (k.w[TW_STATE] == SUMA_TRACK_CONFIRMED) atomicAdd(&s_cnt[TC_CONFIRMED], 1u);
    }
  }
  for (uint32_t i = tid; i < n; i += TK_BLOCK) a.objtrack[i] = tk_ld(a.dettrack + tk_ld(a.objdet + i));
  __syncthreads();
  if (tid == 0u) {
    s_cnt[TC_OBJECTS] = n, s_cnt[TC_DETECTIONS] = D, s_cnt[TC_JOINED] = n - D;
    s_cnt[TC_BORN] = n_born, s_cnt[TC_DROPPED] = n_unmatched - n_born, s_cnt[TC_ROUNDS] = round;
    for (uint32_t w = 0; w < 12u; ++w) a.words[w] = s_cnt[w];
    a.words[TRK_N_LIVE] = n_out;
    a.words[TRK_BORN_TOTAL] = next_id - 1u + n_born;
  }
}

/* ---- host side ---- */
int tracks_alloc(suma_ctx* c, Tracks& tk, const suma_track_params& tp, uint32_t max_objects) {
  Tracks nw;
  const size_t N = max_objects;
  hipError_t e = nw.parent.alloc(N);
  if (e == hipSuccess) e = nw.acc.alloc(N);
  if (e == hipSuccess) e = nw.det.alloc(TK_DET_WORDS * N);
  if (e == hipSuccess) e = nw.objdet.alloc(N);
  if (e == hipSuccess) e = nw.objtrack.alloc(N);
  if (e == hipSuccess) e = nw.detmatch.alloc(N);
  if (e == hipSuccess) e = nw.dettrack.alloc(N);
  if (e == hipSuccess) e = nw.detpick.alloc(N);
  if (e == hipSuccess) e = nw.rec_in.alloc(4 * N);
  if (e == hipSuccess) e = nw.slots.alloc(tp.max_tracks);
  if (e == hipSuccess) e = nw.out.alloc(tp.max_tracks);
  if (e == hipSuccess) e = nw.words.alloc(TRK_WORDS);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SUMA_ERR_NOMEM, "suma_localizer_enable_tracks: no device memory for " + std::to_string(max_objects) +
                                   " objects and " + std::to_string(tp.max_tracks) + " tracks");
  }
  nw.tp = tp;
  nw.max_objects = max_objects;
  tk = std::move(nw);
  return tracks_clear(c, tk);
}

int tracks_clear(suma_ctx* c, Tracks& tk) {
  HIP_TRY(c, hipMemsetAsync(tk.slots, 0, (size_t)tk.tp.max_tracks * sizeof(suma_object_track), c->stream));
  HIP_TRY(c, hipMemsetAsync(tk.words, 0, TRK_WORDS * sizeof(uint32_t), c->stream));
  tk.last_stamp = 0;
  tk.updated = 0;
  return SUMA_OK;
}

int tracks_update(suma_ctx* c, Tracks& tk, const float4* d_rec, const uint32_t* d_n, uint32_t s) {
  TrkArgs a;
  a.rec = reinterpret_cast<const uint32_t*>(d_rec);
  a.n_ptr = d_n;
  a.max_objects = tk.max_objects;
  a.s = s, a.steps = s - tk.last_stamp;
  a.tp = tk.tp;
  a.parent = tk.parent;
  a.acc = tk.acc;
  a.det = tk.det;
  a.objdet = tk.objdet, a.objtrack = tk.objtrack, a.detmatch = tk.detmatch, a.dettrack = tk.dettrack;
  a.detpick = tk.detpick;
  a.slots = tk.slots, a.out = tk.out;
  a.words = tk.words;
  const uint32_t blocks = (tk.max_objects + TK_THREADS - 1) / TK_THREADS;
  {
    ProfScope ps(c, "tracks_join", 200.0 * tk.max_objects, 3);
    ktr_init<<<blocks, TK_THREADS, 0, c->stream>>>(a);
    ktr_join<<<TK_JOIN_BLOCKS, TK_THREADS, 0, c->stream>>>(a);
    ktr_reduce<<<blocks, TK_THREADS, 0, c->stream>>>(a);
  }
  {
    ProfScope ps(c, "tracks_update", 250.0 * tk.tp.max_tracks, 1);
    ktr_track<<<1, TK_BLOCK, 0, c->stream>>>(a);
  }
  HIP_TRY(c, hipGetLastError());
  tk.last_stamp = s;
  tk.updated = 1;
  return SUMA_OK;
}
