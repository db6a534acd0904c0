/*
 * k_localize.hip -- the finished map as a source of surfels: the world-frame records of suma_map_export_world (48 bytes,
 * suma_world_surfel) kept on the device, binned into the reference's submap tiles, and the tiles around the sensor
 * gathered into the active surfel buffer of a localiser's ctx (suma_localize.hip), where k_render's inactive render and
 * the Gauss-Newton chain use them as they use any map.  Nothing in the reference does this; the tiles, their centres
 * and the re-centring rule are SurfelMap::updateActiveSubmaps' (SurfelMap.cpp:704-706, :744-824).
 *
 * Kernels (VGPRs: tools/isa_stats.py k_localize.hip; none uses scratch):
 *   kl_keys     lane per record: tile key and source index; counts the dropped records.
 *   kl_dir      lane per sorted position: the lane at the head of a run writes the tile's key and start.
 *   kl_counts   lane per tile: count = the next tile's start (or the number of kept records) - start.
 *   kl_permute  lane per sorted position: the record moves to its sorted place (16-byte loads and stores).
 *   kl_gather   lane per window record: finds its span by binary search (loc_window_record, group_by_key.h), converts
 *               48 -> 64 bytes (16-byte loads and stores); lane 0 sets DevState.n_surfels.
 *   between kl_keys and kl_dir the sort, the run heads and the scan of k_group.hip.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; `/` correctly rounded;
 * tests/localize_shim.c restates it on the host, byte for byte).  SOURCE INDEX = position in the caller's array.
 *
 * Cell index: e = suma_params.submap_extent; i = floorf((x + e) / (2e)), j = floorf((y + e) / (2e)), 2e = 2.0f * e.
 *   Tile (i, j) is the one whose centre submap_center() puts at (2ie, 2je).  A record is DROPPED (counted in n_dropped)
 *   when x, y or z is non-finite or when |i| or |j| >= 2^20 (an infinite quotient included).
 *   key = (i + 2^20) << 21 | (j + 2^20): ascending by key is ascending by (i, then j).
 * Binning (once per map): a stable sort of (key, source index) by key; the dropped records carry the key 2^42 and sort
 *   behind every tile.  The directory holds {key, start, count} per occupied tile, ascending by key; it is read back to
 *   the host once (suma_localizer_set_map is blocking and off the scan path).
 * Window: the tiles (oi + a, oj + b) with |a|, |b| <= submap_dimension, ascending by (i, then j), each tile's records
 *   in ascending source index.  The host looks the tiles up in its copy of the directory -- no device read-back on the
 *   scan path -- and passes a span table of at most (2 dim + 1)^2 entries.
 * Conversion (suma_world_surfel -> suma_surfel): x, y, z, radius and nx, ny, nz, confidence are copied;
 *   timestamp = 0, color = 0, weight = 0, count = 0.0f; r = g = b = (float)label / 255.0f, w = prob.
 *   Row 0 of the localiser ctx's pose table is the identity and is never written, so the world frame is the surfels'
 *   creation frame.  The ctx's timestamp is the constant T_loc = active_timestamps + 10: at least 10, because K1 drops
 *   moving-class points while timestamp < 10, and -- with the active_timestamps >= 91 that suma_localizer_create asks
 *   for -- above 100, because the inactive render selects the creation stamps below timestamp - 100 (the reference's
 *   literal, SurfelMap.cpp:873), here stamp 0: every record of the window.
 * Re-centring (updateActiveSubmaps' rule, applied to the predicted pose before the render): with (cx, cy) =
 *   ((float)(2.0 * oi * e), (float)(2.0 * oj * e)) the window centre and (x, y) the fp32 translation of the guess:
 *   if |x - cx| > 1.1f * e, oi moves by -1 (x - cx < 0) or +1; then the same test for y against the unchanged cy.  At
 *   most one step per axis per scan.  The window is gathered again only if the origin moved.  suma_localizer_set_pose
 *   puts the origin on the pose's own cell and gathers.
 * Capacity: a window of more than max_surfels records is SUMA_ERR_CAPACITY, found on the host from the directory
 *   before anything is launched.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"
#include "group_by_key.h"

#define LOC_THREADS 256
#define LOC_GRID 1048576.0f /* 2^20 */
#define LOC_NO_KEY (1ull << 42)
#define LOC_KEY_BITS 43u
enum { LOC_DROPPED = 0, LOC_COUNTERS = 2 };

/* the cell of a position, on both sides of the bus */
static __host__ __device__ __forceinline__ bool loc_cell(float e, float x, float y, float z, int32_t* i, int32_t* j) {
  const uint32_t inf = 0x7f800000u;
  if ((sdm_f2u(x) & inf) == inf || (sdm_f2u(y) & inf) == inf || (sdm_f2u(z) & inf) == inf) return false;
  const float w = 2.0f * e;
  const float fi = sdm_floor((x + e) / w), fj = sdm_floor((y + e) / w);
  if (!(sdm_abs(fi) < LOC_GRID && sdm_abs(fj) < LOC_GRID)) return false;
  *i = (int32_t)fi;
  *j = (int32_t)fj;
  return true;
}
static __host__ __device__ __forceinline__ unsigned long long loc_key(int32_t i, int32_t j) {
  return ((unsigned long long)(uint32_t)(i + 1048576) << 21) | (unsigned long long)(uint32_t)(j + 1048576);
}

bool localize_cell(float extent, float x, float y, float z, int32_t* i, int32_t* j) { return loc_cell(extent, x, y, z, i, j); }

__global__ void __launch_bounds__(LOC_THREADS)
    kl_keys(const float4* __restrict__ rec, uint32_t n, float extent, unsigned long long* __restrict__ key,
            uint32_t* __restrict__ idx, uint32_t* __restrict__ counters) {
  __shared__ uint32_t block_dropped;
  if (threadIdx.x == 0) block_dropped = 0u;
  __syncthreads();
  const uint32_t s = blockIdx.x * LOC_THREADS + threadIdx.x;
  if (s < n) {
    const float4 p = rec[3 * (size_t)s];
    int32_t i, j;
    const bool kept = loc_cell(extent, p.x, p.y, p.z, &i, &j);
    key[s] = kept ? loc_key(i, j) : LOC_NO_KEY;
    idx[s] = s;
    if (!kept) atomicAdd(&block_dropped, 1u); /* LDS; integer sums do not depend on the order */
  }
  __syncthreads();
  if (threadIdx.x == 0 && block_dropped) atomicAdd(&counters[LOC_DROPPED], block_dropped);
}

__global__ void __launch_bounds__(LOC_THREADS)
    kl_dir(uint32_t n, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ flag,
           const uint32_t* __restrict__ pos, LocTile* __restrict__ dir, uint32_t n_tiles) {
  const uint32_t k = blockIdx.x * LOC_THREADS + threadIdx.x;
  if (k >= n || !flag[k]) return;
  const uint32_t t = pos[k];
  if (t >= n_tiles) return;
  dir[t].key = keys[k];
  dir[t].start = k;
}

__global__ void __launch_bounds__(LOC_THREADS) kl_counts(LocTile* __restrict__ dir, uint32_t n_tiles, uint32_t n_kept) {
  const uint32_t t = blockIdx.x * LOC_THREADS + threadIdx.x;
  if (t >= n_tiles) return;
  const uint32_t end = (t + 1u < n_tiles) ? dir[t + 1u].start : n_kept;
  dir[t].count = end - dir[t].start;
}

__global__ void __launch_bounds__(LOC_THREADS)
    kl_permute(const float4* __restrict__ rec, const uint32_t* __restrict__ idx, uint32_t n_kept,
               float4* __restrict__ sorted) {
  const uint32_t k = blockIdx.x * LOC_THREADS + threadIdx.x;
  if (k >= n_kept) return;
  const float4* src = rec + 3 * (size_t)idx[k];
  const float4 a = src[0], b = src[1], d = src[2];
  float4* dst = sorted + 3 * (size_t)k;
  dst[0] = a;
  dst[1] = b;
  dst[2] = d;
}

__global__ void __launch_bounds__(LOC_THREADS)
    kl_gather(const float4* __restrict__ sorted, const LocSpan* __restrict__ spans, uint32_t n_spans, uint32_t total,
              float4* __restrict__ out, uint32_t* __restrict__ n_surfels) {
  const uint32_t o = blockIdx.x * LOC_THREADS + threadIdx.x;
  if (o == 0) *n_surfels = total;
  if (o >= total) return;
  const float4* src = sorted + 3 * loc_window_record(spans, n_spans, o);
  const float4 s0 = src[0], s1 = src[1], s2 = src[2];
  const float L = (float)__float_as_uint(s2.x) / 255.0f;
  float4* dst = out + 4 * (size_t)o; /* 64-byte records */
  dst[0] = s0;
  dst[1] = s1;
  dst[2] = f4(0.0f, 0.0f, 0.0f, 0.0f); /* timestamp 0 (all-zero bits), color, weight, count */
  dst[3] = f4(L, L, L, s2.y);
}

/* ---- host side ---- */
int localize_bin(suma_ctx* c, const suma_world_surfel* d_records, uint32_t n, LocMap* m, bool keep_evidence) {
  LocMap nm;
  nm.has_evidence = keep_evidence;
  nm.n_total = n;
  if (n == 0) {
    nm.spans = std::move(m->spans);
    *m = std::move(nm);
    return SUMA_OK;
  }
  if (n > 0x80000000u) return fail(c, SUMA_ERR_CAPACITY, "suma_localizer_set_map: more than 2^31 records");
  hipStream_t st = c->stream;
  const float4* rec = reinterpret_cast<const float4*>(d_records);
  const unsigned blocks = (unsigned)(((size_t)n + LOC_THREADS - 1) / LOC_THREADS);
  /* scratch of the binning, given back when the call returns: two key arrays 8 n each, then two index arrays, head
   * flags and positions, 4 n each; the sort ping-pongs inside the pairs (rocprim::double_buffer) */
  DevBuf<char> scratch, tmp;
  DevBuf<uint32_t> counters;
  DevBuf<LocTile> d_dir;
  HIP_TRY(c, scratch.alloc((size_t)32 * n));
  HIP_TRY(c, counters.alloc(LOC_COUNTERS));
  unsigned long long* keyA = reinterpret_cast<unsigned long long*>(scratch.p);
  unsigned long long* keyB = keyA + n;
  uint32_t *idxA = reinterpret_cast<uint32_t*>(keyB + n), *idxB = idxA + n, *flag = idxB + n, *pos = flag + n;
  rocprim::double_buffer<unsigned long long> key(keyA, keyB);
  rocprim::double_buffer<uint32_t> idx(idxA, idxB);
  size_t need = 0;
  HIP_TRY(c, group_tmp_bytes(n, true, st, &need));
  HIP_TRY(c, tmp.alloc(need));

  uint32_t h_counters[LOC_COUNTERS] = {0, 0}, last[2] = {0, 0};
  {
    ProfScope ps(c, "loc_bin", 48.0 * n);
    HIP_TRY(c, hipMemsetAsync(counters, 0, LOC_COUNTERS * sizeof(uint32_t), st));
    kl_keys<<<blocks, LOC_THREADS, 0, st>>>(rec, n, c->p.submap_extent, keyA, idxA, counters);
    HIP_TRY(c, group_sort(tmp.p, tmp.cap, key, idx, n, LOC_KEY_BITS, st));
    HIP_TRY(c, group_heads(tmp.p, tmp.cap, key.current(), LOC_NO_KEY, flag, pos, n, st));
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&last[0], flag + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&last[1], pos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const uint32_t n_dropped = h_counters[LOC_DROPPED], n_tiles = last[0] + last[1];
  if (n_dropped > n || n_tiles > n - n_dropped)
    return fail(c, SUMA_ERR_HIP, "suma_localizer_set_map: inconsistent counters (internal error)");
  nm.n_dropped = n_dropped;
  nm.n_kept = n - n_dropped;
  if (nm.n_kept) {
    HIP_TRY(c, d_dir.alloc(n_tiles));
    HIP_TRY(c, nm.sorted.alloc(3 * (size_t)nm.n_kept));
    nm.dir.resize(n_tiles);
    ProfScope ps(c, "loc_bin", 112.0 * nm.n_kept);
    kl_dir<<<blocks, LOC_THREADS, 0, st>>>(n, key.current(), flag, pos, d_dir, n_tiles);
    kl_counts<<<(n_tiles + LOC_THREADS - 1) / LOC_THREADS, LOC_THREADS, 0, st>>>(d_dir, n_tiles, nm.n_kept);
    kl_permute<<<(nm.n_kept + LOC_THREADS - 1) / LOC_THREADS, LOC_THREADS, 0, st>>>(rec, idx.current(), nm.n_kept, nm.sorted);
    HIP_TRY(c, hipGetLastError());
    if (keep_evidence) { /* the sort's source index outlives the scratch, and the evidence starts at zero */
      HIP_TRY(c, nm.src_idx.alloc(nm.n_kept));
      HIP_TRY(c, nm.evidence.alloc(nm.n_kept));
      HIP_TRY(c, hipMemcpyAsync(nm.src_idx, idx.current(), (size_t)nm.n_kept * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      HIP_TRY(c, hipMemsetAsync(nm.evidence, 0, (size_t)nm.n_kept * sizeof(suma_change_evidence), st));
    }
    HIP_TRY(c, hipMemcpyAsync(nm.dir.data(), d_dir, n_tiles * sizeof(LocTile), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    /* what the window look-up relies on, checked once: ascending keys, runs that tile [0, n_kept) */
    uint64_t at = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
      const LocTile& q = nm.dir[t];
      if (q.start != at || q.count == 0 || q.key >= LOC_NO_KEY || (t && nm.dir[t - 1].key >= q.key))
        return fail(c, SUMA_ERR_HIP, "suma_localizer_set_map: malformed tile directory (internal error)");
      at += q.count;
    }
    if (at != nm.n_kept) return fail(c, SUMA_ERR_HIP, "suma_localizer_set_map: malformed tile directory (internal error)");
  }
  nm.spans = std::move(m->spans);
  *m = std::move(nm);
  return SUMA_OK;
}

void localize_window_spans(const LocMap& m, int32_t oi, int32_t oj, int32_t dim, std::vector<LocSpan>* spans,
                           uint64_t* total) {
  spans->clear();
  uint64_t at = 0;
  for (int64_t i = (int64_t)oi - dim; i <= (int64_t)oi + dim; ++i) {
    for (int64_t j = (int64_t)oj - dim; j <= (int64_t)oj + dim; ++j) {
      if (i <= -1048576 || i >= 1048576 || j <= -1048576 || j >= 1048576) continue;
      const unsigned long long key = loc_key((int32_t)i, (int32_t)j);
      size_t lo = 0, hi = m.dir.size(); /* the first tile with a key >= key */
      while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (m.dir[mid].key < key) lo = mid + 1; else hi = mid;
      }
      if (lo == m.dir.size() || m.dir[lo].key != key) continue;
      if (at <= 0xffffffffull) spans->push_back({m.dir[lo].start, (uint32_t)at, m.dir[lo].count, 0u});
      at += m.dir[lo].count;
    }
  }
  *total = at;
}

int localize_gather(suma_ctx* c, LocMap* m, const std::vector<LocSpan>& spans, uint32_t total) {
  if (total > c->p.max_surfels) return fail(c, SUMA_ERR_CAPACITY, "localiser window beyond max_surfels (internal error)");
  const size_t ns = spans.size();
  int r = grow(c, m->spans, ns ? ns : 1, {c->stream}, ns + ns / 4 + 32);
  if (r < 0) return r;
  hipStream_t st = c->stream;
  /* pageable source: the copy has left `spans` when the call returns */
  if (ns) HIP_TRY(c, hipMemcpyAsync(m->spans, spans.data(), ns * sizeof(LocSpan), hipMemcpyHostToDevice, st));
  {
    ProfScope ps(c, "loc_gather", 112.0 * total);
    const unsigned blocks = total ? (total + LOC_THREADS - 1) / LOC_THREADS : 1u;
    kl_gather<<<blocks, LOC_THREADS, 0, st>>>(m->sorted, m->spans, (uint32_t)ns, total,
                                             reinterpret_cast<float4*>(c->surfels[c->cur].p), &c->ds->n_surfels);
    HIP_TRY(c, hipGetLastError());
  }
  c->known_surfels = total;
  c->map_version++;
  return SUMA_OK;
}
