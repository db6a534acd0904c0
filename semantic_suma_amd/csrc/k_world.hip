/*
 * k_world.hip -- the finished map handed to a user: every surfel of the active map and of the parked submap tiles in
 * ONE frame (the world frame of the pose table), filtered, optionally fused to one record per voxel with a label vote.
 * Nothing in the reference does this (its only global view is SurfelMap::draw's picture of the active map); the
 * transform is the one its draw_surfels.vert applies, which k_draw.hip specifies and draw_vertex.h implements.
 *
 * Kernels (VGPRs: tools/isa_stats.py k_world.hip; none uses scratch):
 *   kw_classify  lane per source record: label, filters, transform, voxel key; a keep flag (flat) or key / label / index /
 *                vote record (voxel mode); counts n_passed and n_dropped.
 *   kw_emit      flat mode, lane per source record: a kept record goes to the position the scan of the flags gives it.
 *   kw_reduce    voxel mode, lane per sorted position: the lane at the head of a run walks it and writes the voxel's record.
 *   between them the sorts, the key gather, the run heads and the scan of k_group.hip.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; `/` correctly rounded;
 * tests/world_shim.c restates it on the host, bit for bit).
 *
 * Source sequence: the active map [0, size) in buffer order, then every non-empty parked tile ascending by (i, j), each
 *   in its stored order -- getAllSurfels() ++ cached_tile(i, j) over suma_map_cached_tiles.  A record's position in it
 *   is its SOURCE INDEX.
 * Per source record s:
 *   1. Label: t = s.r * 255.0f + 0.5f; L = (uint32)t if 0 <= t < 260, else 0 (NaN and inf give 0).  This inverts
 *      float(l) / 255.0f for every l in 0 .. 259.  The record PASSES iff confidence > min_confidence && keep_label[L].
 *   2. Transform: k_draw.hip's vertex stage (draw_vertex.h): k = int(count) clamped to [0, max_poses - 1] (NaN: 0),
 *      p = M (x, y, z, 1), n = M (nx, ny, nz, 0), M = poses[k], rows fma(m3, v.w, fma(m2, v.z, fma(m1, v.y, m0 * v.x))).
 *      The normal is not re-normalised.  A passed record with a non-finite p.x / p.y / p.z is DROPPED (n_dropped).
 *   3. voxel_size == 0: the output is the stable compaction of the surviving records in source order;
 *      prob = s.w, support = 1, radius / confidence / timestamp copied.
 *   4. voxel_size > 0 (voxel_key, group_by_key.h): f_a = floorf(p_a / voxel_size) per axis; a record with any
 *      |f_a| >= 2^20 (an infinite quotient included) is DROPPED (n_dropped); i_a = (int)f_a;
 *      key = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20).
 *      One record per distinct key, in ascending key order:
 *      representative = the member with the greatest confidence, on a tie the smallest source index;
 *        x, y, z, radius, nx, ny, nz, confidence are the representative's.
 *      vote (vote_weight and LabelVote, group_by_key.h): a member votes for its L with the weight
 *        q = (uint32)rintf(clamp(s.w, 0, 1) * 65535.0f) (NaN: 0), summed per label in uint64 (exact, order-free);
 *        label = the label with the greatest sum, on a tie the smallest id;
 *        prob = (float)sum_label / (float)sum_all; sum_all == 0: label = the representative's L, prob = 0.
 *      timestamp = the maximum over the members, support = the member count.
 * The output is a pure function of the source sequence, the pose table and the parameters.
 *
 * Decomposition of the voxel mode: two stable radix sorts of (key, source index), in place in double buffers
 * (group_sort_by_value_then_key, k_group.hip) -- by label (9 bits), then by voxel key (64 bits: records that do not
 * survive carry VOXEL_NO_KEY and sort behind every voxel).  Inside a voxel's run the members are then ordered by label,
 * then by source index, so the vote needs one running sum and the best (sum, label) so far: no per-lane table of 260
 * sums, no atomics, and no order that depends on a race.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"
#include "draw_vertex.h"
#include "group_by_key.h"

#define WORLD_THREADS 256
#define WORLD_KEEP_WORDS ((SUMA_DRAW_COLORS + 31) / 32)

struct WorldArgs {
  const WorldSpan* spans;
  uint32_t n_spans;
  uint32_t n; /* source records */
  const float* poses;
  uint32_t n_poses;
  float voxel_size, min_confidence;
  uint32_t keep[WORLD_KEEP_WORDS];
};
/* counters (device): */
enum { WORLD_PASSED = 0, WORLD_DROPPED = 1, WORLD_OUT = 2, WORLD_COUNTERS = 4 };

SDEV const float4* world_source(const WorldArgs& a, uint32_t s) {
  const WorldSpan sp = world_span_find(a.spans, a.n_spans, s);
  return reinterpret_cast<const float4*>(sp.base + (s - sp.start));
}
/* world_label (step 1's rule) is in dev_math.h: k_change.hip reads labels by it too */
SDEV void world_store(suma_world_surfel* out, uint32_t o, const float4& p, float radius, const float4& n, float conf,
                      uint32_t label, float prob, uint32_t timestamp, uint32_t support) {
  float4* dst = reinterpret_cast<float4*>(out) + 3 * (size_t)o; /* 48-byte records: 16-byte aligned */
  dst[0] = f4(p.x, p.y, p.z, radius);
  dst[1] = f4(n.x, n.y, n.z, conf);
  dst[2] = f4(__uint_as_float(label), prob, __uint_as_float(timestamp), __uint_as_float(support));
}
/* steps 1, 2 and the key of step 4.  0: filtered, 1: passed but dropped, 2: survives */
SDEV int world_classify(const WorldArgs& a, const float4& s0, const float4& s1, const float4& s2, const float4& s3,
                        uint32_t* L, float4* p, float4* n, unsigned long long* key) {
  *L = world_label(s3.x);
  if (!(s1.w > a.min_confidence) || !((a.keep[*L >> 5] >> (*L & 31u)) & 1u)) return 0;
  draw_vertex(a.poses, a.n_poses, s0, s1, s2.w, p, n);
  if (!(finite_f(p->x) && finite_f(p->y) && finite_f(p->z))) return 1;
  if (a.voxel_size > 0.0f && !voxel_key(p->x, p->y, p->z, a.voxel_size, key)) return 1;
  return 2;
}

/* a block takes WORLD_CLASSIFY_ITEMS stretches of WORLD_THREADS records and adds its two counts to the global counters
 * once: one atomic per wave on one address was most of this kernel's time (3 M records: 556 us, of which the loads are
 * about 80) */
#define WORLD_CLASSIFY_ITEMS 8
__global__ void __launch_bounds__(WORLD_THREADS)
    kw_classify(WorldArgs a, uint32_t* __restrict__ u0 /* flat: keep flag; voxel mode: label */,
                unsigned long long* __restrict__ key0, uint32_t* __restrict__ idx0, uint4* __restrict__ vote,
                uint32_t* __restrict__ counters) {
  __shared__ uint32_t block_counts[2];
  if (threadIdx.x < 2) block_counts[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t np = 0, nd = 0; /* this lane's records that passed / were dropped */
  const unsigned long long first = (unsigned long long)blockIdx.x * (WORLD_THREADS * WORLD_CLASSIFY_ITEMS) + threadIdx.x;
#pragma unroll 2
  for (uint32_t it = 0; it < WORLD_CLASSIFY_ITEMS; ++it) {
    const unsigned long long s64 = first + (unsigned long long)it * WORLD_THREADS;
    if (s64 >= a.n) break;
    const uint32_t s = (uint32_t)s64;
    const float4* sf = world_source(a, s);
    const float4 s0 = sf[0], s1 = sf[1], s2 = sf[2], s3 = sf[3];
    uint32_t L;
    float4 p, n;
    unsigned long long key = VOXEL_NO_KEY;
    const int cls = world_classify(a, s0, s1, s2, s3, &L, &p, &n, &key);
    if (a.voxel_size > 0.0f) {
      key0[s] = (cls == 2) ? key : VOXEL_NO_KEY;
      u0[s] = L;
      idx0[s] = s;
      vote[s] = make_uint4(__float_as_uint(s1.w), (vote_weight(s3.w) << 16) | L, __float_as_uint(s2.x), 0u);
    } else {
      u0[s] = (cls == 2) ? 1u : 0u;
    }
    np += (cls >= 1) ? 1u : 0u;
    nd += (cls == 1) ? 1u : 0u;
  }
  if (np) atomicAdd(&block_counts[0], np); /* LDS; integer sums do not depend on the order */
  if (nd) atomicAdd(&block_counts[1], nd);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (block_counts[0]) atomicAdd(&counters[WORLD_PASSED], block_counts[0]);
    if (block_counts[1]) atomicAdd(&counters[WORLD_DROPPED], block_counts[1]);
  }
}

__global__ void __launch_bounds__(WORLD_THREADS)
    kw_emit(WorldArgs a, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
            suma_world_surfel* __restrict__ out, uint32_t capacity, uint32_t* __restrict__ counters) {
  const uint32_t s = blockIdx.x * WORLD_THREADS + threadIdx.x;
  if (s >= a.n) return;
  const uint32_t f = flag[s], o = pos[s];
  if (s == a.n - 1u) counters[WORLD_OUT] = o + f;
  if (!f || o >= capacity) return;
  const float4* sf = world_source(a, s);
  const float4 s0 = sf[0], s1 = sf[1], s2 = sf[2], s3 = sf[3];
  float4 p, n;
  draw_vertex(a.poses, a.n_poses, s0, s1, s2.w, &p, &n);
  world_store(out, o, p, s0.w, n, s1.w, world_label(s3.x), s3.w, __float_as_uint(s2.x), 1u);
}

__global__ void __launch_bounds__(WORLD_THREADS)
    kw_reduce(WorldArgs a, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ idx,
              const uint4* __restrict__ vote, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
              suma_world_surfel* __restrict__ out, uint32_t capacity, uint32_t* __restrict__ counters) {
  const uint32_t j = blockIdx.x * WORLD_THREADS + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t f = flag[j], o = pos[j];
  if (j == a.n - 1u) counters[WORLD_OUT] = o + f;
  if (!f || o >= capacity) return;
  const unsigned long long key = keys[j];
  /* members come by label, then by source index */
  LabelVote tally;
  uint32_t rep = 0, stamp = 0, support = 0;
  float conf_best = 0.0f;
  for (uint32_t k = j; k < a.n && keys[k] == key; ++k) {
    const uint32_t s = idx[k];
    const uint4 v = vote[s];
    const float conf = __uint_as_float(v.x);
    tally.add(v.y & 0xffffu, v.y >> 16);
    if (support == 0 || conf > conf_best || (conf == conf_best && s < rep)) conf_best = conf, rep = s;
    stamp = (v.z > stamp) ? v.z : stamp;
    ++support;
  }
  const float4* sf = world_source(a, rep);
  const float4 s0 = sf[0], s1 = sf[1], s2 = sf[2], s3 = sf[3];
  float4 p, n;
  draw_vertex(a.poses, a.n_poses, s0, s1, s2.w, &p, &n);
  uint32_t label;
  const float prob = tally.close(world_label(s3.x), &label);
  world_store(out, o, p, s0.w, n, s1.w, label, prob, stamp, support);
}

/* ---- host side ---- */
extern "C" void suma_world_params_default(suma_world_params* wp) {
  if (!wp) return;
  wp->voxel_size = 0.0f;
  wp->min_confidence = -INFINITY;
  std::memset(wp->keep_label, 1, sizeof(wp->keep_label));
}

/* the parked tiles that hold records, ascending by (i, j), with their slots as the device table has them now (one
 * synchronisation); ds: also the map's counters into c->h_ds (the staging record every read-back of them uses) */
static int world_tiles(suma_ctx* c, bool ds, std::vector<std::pair<int32_t, int32_t>>* ij, std::vector<CacheSlot>* live) {
  const uint32_t ns = (uint32_t)c->cache_index.size();
  std::vector<CacheSlot> slots(ns);
  if (ds) HIP_TRY(c, hipMemcpyAsync(c->h_ds, c->ds, sizeof(DevState), hipMemcpyDeviceToHost, c->stream));
  if (ns) HIP_TRY(c, hipMemcpyAsync(slots.data(), c->cache_slots, ns * sizeof(CacheSlot), hipMemcpyDeviceToHost, c->stream));
  if (ds || ns) HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (const auto& kv : c->cache_index) { /* std::map: ascending by (i, then j) */
    const CacheSlot q = slots[kv.second];
    if (q.count == 0) continue;
    if ((uint64_t)q.offset + q.count > c->cache_cap)
      return fail(c, SUMA_ERR_HIP, "submap cache slot outside the arena (internal error)");
    ij->push_back(kv.first);
    if (live) live->push_back(q);
  }
  return SUMA_OK;
}

extern "C" int suma_map_cached_tiles(suma_ctx* c, int32_t* ij, uint32_t capacity, uint32_t* n) {
  if (!c) return SUMA_ERR_INVALID;
  if (!n || (capacity && !ij)) return fail(c, SUMA_ERR_INVALID, "suma_map_cached_tiles: NULL argument");
  std::vector<std::pair<int32_t, int32_t>> tiles;
  const int r = world_tiles(c, false, &tiles, nullptr);
  if (r) return r;
  *n = (uint32_t)tiles.size();
  for (uint32_t k = 0; k < *n && k < capacity; ++k) ij[2 * k] = tiles[k].first, ij[2 * k + 1] = tiles[k].second;
  return SUMA_OK;
}

extern "C" int suma_map_export_world(suma_ctx* c, const suma_world_params* wp, suma_world_surfel* d_out, uint32_t capacity,
                                     suma_world_stats* stats) {
  if (!c) return SUMA_ERR_INVALID;
  if (!wp) return fail(c, SUMA_ERR_INVALID, "suma_map_export_world: NULL parameters");
  if (!stats) return fail(c, SUMA_ERR_INVALID, "suma_map_export_world: NULL stats");
  if (!(wp->voxel_size >= 0.0f) || std::isinf(wp->voxel_size))
    return fail(c, SUMA_ERR_INVALID, "suma_map_export_world: voxel_size = " + std::to_string(wp->voxel_size) +
                                     " (must be finite and >= 0)");
  if (std::isnan(wp->min_confidence)) return fail(c, SUMA_ERR_INVALID, "suma_map_export_world: min_confidence is NaN");
  if (capacity && !d_out) return fail(c, SUMA_ERR_INVALID, "suma_map_export_world: NULL output buffer with capacity > 0");

  /* the source sequence */
  std::vector<std::pair<int32_t, int32_t>> tiles;
  std::vector<CacheSlot> live;
  int r = world_tiles(c, true, &tiles, &live);
  if (r) return r;
  const uint32_t n_active = c->h_ds->n_surfels < c->p.max_surfels ? c->h_ds->n_surfels : c->p.max_surfels;
  std::vector<WorldSpan> spans;
  spans.push_back({c->surfels[c->cur], 0u, n_active});
  uint64_t total = n_active;
  for (const CacheSlot& q : live) {
    spans.push_back({c->cache_arena + q.offset, (uint32_t)total, q.count});
    total += q.count;
    if (total > 0xffffffffull) return fail(c, SUMA_ERR_CAPACITY, "suma_map_export_world: more than 2^32 - 1 source surfels");
  }
  const uint32_t N = (uint32_t)total;
  std::memset(stats, 0, sizeof(*stats));
  stats->n_active = n_active;
  stats->n_tiles = (uint32_t)live.size();
  stats->n_parked = N - n_active;

  const bool voxel = wp->voxel_size > 0.0f;
  if ((r = grow(c, c->world_counters, WORLD_COUNTERS, {})) < 0) return r;
  if ((r = grow(c, c->world_counters_h, WORLD_COUNTERS, {})) < 0) return r;
  if ((r = grow(c, c->world_spans, spans.size(), {c->stream}, spans.size() + spans.size() / 4 + 64)) < 0) return r;
  if ((r = grow(c, c->world_scratch, (size_t)N * (voxel ? 48 : 8), {c->stream})) < 0) return r;
  char* base = c->world_scratch;
  /* voxel mode: vote 16 N | two key arrays 8 N each | two label arrays, then two index arrays, 4 N each: the sorts
   * ping-pong inside each pair (rocprim::double_buffer), so their temporary storage is histograms only; the label pair
   * is free after the first sort and takes the head flags and positions.  Flat: keep flags and positions, 4 N each */
  uint4* vote = reinterpret_cast<uint4*>(base);
  unsigned long long* keyA = reinterpret_cast<unsigned long long*>(base + (voxel ? (size_t)16 * N : 0));
  unsigned long long* keyB = keyA + N;
  uint32_t* u0 = reinterpret_cast<uint32_t*>(base + (voxel ? (size_t)32 * N : 0)); /* labels, then head flags / keep flags */
  uint32_t *u1 = u0 + N /* sorted labels, then positions */, *u2 = u1 + N /* indices, then by voxel */, *u3 = u2 + N /* by label */;

  size_t tmp = 0;
  HIP_TRY(c, group_tmp_bytes(N, voxel, c->stream, &tmp));
  if ((r = grow(c, c->world_tmp, tmp, {c->stream})) < 0) return r;

  WorldArgs a;
  a.spans = c->world_spans;
  a.n_spans = (uint32_t)spans.size();
  a.n = N;
  a.poses = c->poses;
  a.n_poses = c->p.max_poses;
  a.voxel_size = wp->voxel_size;
  a.min_confidence = wp->min_confidence;
  std::memset(a.keep, 0, sizeof(a.keep));
  for (uint32_t l = 0; l < SUMA_DRAW_COLORS; ++l)
    if (wp->keep_label[l]) a.keep[l >> 5] |= 1u << (l & 31u);

  hipStream_t st = c->stream;
  /* pageable source: the copy has left `spans` when the call returns */
  HIP_TRY(c, hipMemcpyAsync(c->world_spans, spans.data(), spans.size() * sizeof(WorldSpan), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(c->world_counters, 0, WORLD_COUNTERS * sizeof(uint32_t), st));
  if (N) {
    const unsigned blocks = (N + WORLD_THREADS - 1) / WORLD_THREADS;
    const size_t bytes = c->world_tmp.cap;
    {
      ProfScope ps(c, "world_classify", 64.0 * N);
      const unsigned per_block = WORLD_THREADS * WORLD_CLASSIFY_ITEMS;
      kw_classify<<<(unsigned)(((size_t)N + per_block - 1) / per_block), WORLD_THREADS, 0, st>>>(a, u0, keyA, u2, vote,
                                                                                                 c->world_counters);
    }
    if (!voxel) {
      ProfScope ps(c, "world_emit", 72.0 * N);
      HIP_TRY(c, group_scan(c->world_tmp, bytes, u0, u1, N, st));
      kw_emit<<<blocks, WORLD_THREADS, 0, st>>>(a, u0, u1, d_out, capacity, c->world_counters);
    } else {
      rocprim::double_buffer<uint32_t> lab(u0, u1), idx(u2, u3); /* labels / source indices as kw_classify wrote them */
      rocprim::double_buffer<unsigned long long> key(keyB, keyA); /* keyB is filled from keyA, which is then dead */
      {
        ProfScope ps(c, "world_sort", 64.0 * N);
        HIP_TRY(c, group_sort_by_value_then_key(c->world_tmp, bytes, lab, 9u, keyA, key, 64u, idx, N, st));
      }
      ProfScope ps(c, "world_reduce", 40.0 * N);
      HIP_TRY(c, group_heads(c->world_tmp, bytes, key.current(), VOXEL_NO_KEY, u0, u1, N, st));
      kw_reduce<<<blocks, WORLD_THREADS, 0, st>>>(a, key.current(), idx.current(), vote, u0, u1, d_out, capacity,
                                                  c->world_counters);
    }
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipMemcpyAsync(c->world_counters_h, c->world_counters, WORLD_COUNTERS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  stats->n_passed = c->world_counters_h[WORLD_PASSED];
  stats->n_dropped = c->world_counters_h[WORLD_DROPPED];
  stats->n_out = c->world_counters_h[WORLD_OUT];
  return check_overflow(c); /* a map that an overflow has truncated is reported, as every download does */
}
