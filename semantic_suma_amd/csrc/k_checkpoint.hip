/*
 * k_checkpoint.hip -- the device side of a pipeline checkpoint (suma_pipeline_checkpoint_save / _load,
 * suma_checkpoint.hip; the container's structs and its host parser are checkpoint_format.h).
 *
 * THE IMAGE.  One self-describing byte image, little-endian, taken BETWEEN scans (phase 0, no prefetched scan pending).
 * It is canonical: a function of the pipeline's logical state only.  Arena layout, stale arena blocks, slot numbers, the
 * parity of the double buffers (cur), the de-duplication caches (rendered, k7, k7_spec, k8_fused_*), profiling and wall
 * clock time do not enter it; two pipelines in the same logical state give identical bytes.
 *
 *   header     magic "SUMAKCP1", format version (1), section count, total bytes; then the directory, one entry per
 *              section {id, 0, offset, payload bytes, record count, 64-bit digest of the payload}; then the digest of
 *              every byte before it.  Padded with zeros to 64 bytes.
 *   payloads   in ascending id order, back to back, each starting at a multiple of 64 and padded with zeros.
 *
 *   1 PARAMS    the suma_params the pipeline was created with, as the POD.  A load into a pipeline with other parameters
 *               is refused; the message names the first field that differs.
 *   2 PIPELINE  current_pose, last_pose, pose_old, pose_new, last_increment, last_pose_old (column-major fp64), timestamp,
 *               track_loss, the resolved stats and stats_mst (a pending statistics record is resolved by the save).
 *   3 MAP_STATE SurfelMap::timestamp_, origin_i, origin_j, n_active, the counters of the last update that the C-ABI
 *               shows (n_updated, n_kept_updated, n_data, n_kept_data), and the pending extraction stack in stack order.
 *   4 POSES     the first `timestamp` rows of the float pose table.  The inverse table is not stored: the load rebuilds it
 *               with the kernel that builds it for suma_map_update_poses (the same fp64 arithmetic as every other writer).
 *   5 ACTIVE    the active map's 64-byte records in buffer order (K7 breaks depth ties by index).
 *   6 FRAME     the three maps of current_frame: the fallback minimisation of the next scan reads it as last_frame.
 *               current_model is not stored: the load clears `rendered`, so the next begin_scan renders it again.
 *   7 TILE_DIR  {i, j, first, count} of every non-empty parked tile, ascending by (i, j) -- suma_map_cached_tiles' order.
 *   8 TILES     their records back to back, each tile in its stored order.  Stale arena blocks are not in the image.
 *   9 LOOP      (loop closing on) suma_loop_params, trajectory_distances, the unverified and verified candidates,
 *               already_verified, loop_count, time_without, result_old and the per-scan status of the last scan.
 *  10 GRAPH     (loop closing on) nodes: initial value and current estimate; edges in insertion order with their
 *               information as stored.  All fp64.
 *  11 OPT       (an optimisation started and not yet integrated; the save joins the worker) before_id,
 *               before_loop_count, started_at, before_pose, the worker's return code, the clone's optimised poses.  A
 *               restored pipeline integrates them at the scan the uninterrupted one does when optimize_wait = 1; with
 *               optimize_wait = 0 that scan depends on timing in an uninterrupted run already.
 *
 *   digest     of a payload read as n little-endian 64-bit words w[k] (a shorter tail zero-extended):
 *                sum over k of (w[k] + 0x9E3779B97F4A7C15) * (2 k + 1)  mod 2^64.
 *              An integer sum: the order of accumulation does not matter, so the block-parallel reduction below is
 *              deterministic.  k is the word's position in the PACKED section, not where the record lay in the arena.
 *
 * KERNELS (plain C++ and 16-byte vector memory operations; no inline assembly):
 *   kc_pack    one launch per device-resident section over a span table {base, start, count} (WorldSpan, in units of
 *              16 bytes): lane per 16-byte piece, global_load_dwordx4 -> global_store_dwordx4 into the packed image, and
 *              the section digest: per-lane partial sums, a wave reduction, one 64-bit atomicAdd per block.  POSES, ACTIVE
 *              and FRAME are one span each; TILES one span per tile.
 *   kc_verify  the same digest over a section of a staged image (contiguous, nothing stored); the load runs it over every
 *              section BEFORE anything of the pipeline is written.
 *   kc_unpack  TILES -> the cache arena, compactly from offset 0 in (i, j) order; the CacheSlot table (slot s = the s-th
 *              tile of TILE_DIR); DevState.n_surfels, cache_used and the stored counters.
 *
 * Block shape: 256 lanes x 8 pieces = 32 KiB of records per block iteration, grid capped at SUMA_STREAM_BLOCKS with a
 * grid stride: 16-byte accesses are the full-rate width of the memory pipeline, consecutive lanes touch consecutive
 * pieces, and the at most 2048 atomics of a launch on one word cost microseconds (a returning device-scope atomic on one
 * word saturates near 88 / us) against the hundreds of microseconds a large section streams for.
 */
#include "suma_internal.h"
#include "group_by_key.h"

#define KC_THREADS 256
#define KC_ITEMS 8
#define KC_GOLDEN 0x9E3779B97F4A7C15ull

/* spans == nullptr: one contiguous source at `single` */
template <bool STORE>
__device__ __forceinline__ void kc_stream(const WorldSpan* __restrict__ spans, uint32_t n_spans,
                                          const uint4* __restrict__ single, uint32_t n_quads, uint64_t n_words,
                                          uint4* __restrict__ dst, unsigned long long* __restrict__ digest) {
  __shared__ unsigned long long s_part[KC_THREADS / 64];
  unsigned long long sum = 0;
  WorldSpan sp;
  sp.base = reinterpret_cast<const suma_surfel*>(single);
  sp.start = 0;
  sp.count = spans ? 0u : n_quads;
  const uint64_t per_block = (uint64_t)KC_THREADS * KC_ITEMS;
  for (uint64_t chunk = (uint64_t)blockIdx.x * per_block; chunk < n_quads; chunk += (uint64_t)gridDim.x * per_block) {
    uint4 v[KC_ITEMS];
#pragma unroll
    for (int j = 0; j < KC_ITEMS; ++j) {
      const uint64_t q = chunk + (uint64_t)j * KC_THREADS + threadIdx.x;
      v[j] = make_uint4(0u, 0u, 0u, 0u);
      if (q < n_quads) {
        if (!((uint32_t)q >= sp.start && (uint32_t)q - sp.start < sp.count)) sp = world_span_find(spans, n_spans, (uint32_t)q);
        v[j] = reinterpret_cast<const uint4*>(sp.base)[(uint32_t)q - sp.start];
      }
    }
#pragma unroll
    for (int j = 0; j < KC_ITEMS; ++j) {
      const uint64_t q = chunk + (uint64_t)j * KC_THREADS + threadIdx.x;
      if (q < n_quads) {
        if (STORE) dst[q] = v[j];
        const unsigned long long w0 = (unsigned long long)v[j].x | ((unsigned long long)v[j].y << 32);
        const unsigned long long w1 = (unsigned long long)v[j].z | ((unsigned long long)v[j].w << 32);
        const unsigned long long k0 = 2ull * q;
        if (k0 < n_words) sum += (w0 + KC_GOLDEN) * (2ull * k0 + 1ull);
        if (k0 + 1ull < n_words) sum += (w1 + KC_GOLDEN) * (2ull * k0 + 3ull);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63u) == 0u) s_part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < KC_THREADS / 64; ++w) total += s_part[w];
    atomicAdd(digest, total);
  }
}

__global__ void __launch_bounds__(KC_THREADS)
    kc_pack(const WorldSpan* __restrict__ spans, uint32_t n_spans, uint32_t n_quads, uint4* __restrict__ dst,
            unsigned long long* __restrict__ digest) {
  kc_stream<true>(spans, n_spans, nullptr, n_quads, 2ull * n_quads, dst, digest);
}

__global__ void __launch_bounds__(KC_THREADS)
    kc_verify(const uint4* __restrict__ src, uint32_t n_quads, uint64_t n_words, unsigned long long* __restrict__ digest) {
  kc_stream<false>(nullptr, 0, src, n_quads, n_words, nullptr, digest);
}

struct KcCounters {
  uint32_t n_active, cache_used, n_updated, n_kept_updated, n_data, n_kept_data;
};

__global__ void __launch_bounds__(KC_THREADS)
    kc_unpack(const uint4* __restrict__ tiles, uint4* __restrict__ arena, uint32_t n_quads,
              const uint4* __restrict__ tile_dir, uint32_t n_tiles, CacheSlot* __restrict__ slots, DevState* ds,
              KcCounters in) {
  const uint64_t gid = (uint64_t)blockIdx.x * KC_THREADS + threadIdx.x, stride = (uint64_t)gridDim.x * KC_THREADS;
  for (uint64_t q = gid; q < n_quads; q += stride) arena[q] = tiles[q];
  for (uint64_t t = gid; t < n_tiles; t += stride) {
    const uint4 e = tile_dir[t]; /* {i, j, first, count} */
    CacheSlot cs;
    cs.offset = e.z, cs.count = e.w;
    slots[t] = cs;
  }
  if (gid == 0) {
    ds->n_surfels = in.n_active;
    ds->cache_used = in.cache_used;
    ds->n_updated = in.n_updated, ds->n_kept_updated = in.n_kept_updated;
    ds->n_data = in.n_data, ds->n_kept_data = in.n_kept_data;
  }
}

static unsigned kc_grid(uint64_t n_quads) {
  const uint64_t per_block = (uint64_t)KC_THREADS * KC_ITEMS;
  uint64_t b = (n_quads + per_block - 1) / per_block;
  if (b < 1) b = 1;
  return (unsigned)(b < SUMA_STREAM_BLOCKS ? b : SUMA_STREAM_BLOCKS);
}

hipError_t launch_kc_pack(suma_ctx* c, const WorldSpan* d_spans, uint32_t n_spans, uint32_t n_quads, void* d_dst,
                          unsigned long long* d_digest) {
  if (n_quads == 0 || n_spans == 0) return hipSuccess; /* the digest of an empty payload is 0: the word stays cleared */
  ProfScope ps(c, "kc_pack", 32.0 * n_quads);
  kc_pack<<<kc_grid(n_quads), KC_THREADS, 0, c->ls>>>(d_spans, n_spans, n_quads, static_cast<uint4*>(d_dst), d_digest);
  return hipGetLastError();
}

hipError_t launch_kc_verify(suma_ctx* c, const void* d_src, uint64_t bytes, unsigned long long* d_digest) {
  const uint64_t n_words = (bytes + 7) / 8, n_quads = (n_words + 1) / 2;
  if (n_quads == 0) return hipSuccess;
  if (n_quads > 0xffffffffull) return hipErrorInvalidValue;
  ProfScope ps(c, "kc_verify", 16.0 * n_quads);
  kc_verify<<<kc_grid(n_quads), KC_THREADS, 0, c->ls>>>(static_cast<const uint4*>(d_src), (uint32_t)n_quads, n_words,
                                                        d_digest);
  return hipGetLastError();
}

hipError_t launch_kc_unpack(suma_ctx* c, const void* d_tiles, uint32_t n_parked, const void* d_tile_dir, uint32_t n_tiles,
                            uint32_t n_active, const uint32_t counters[4]) {
  KcCounters in;
  in.n_active = n_active, in.cache_used = n_parked;
  in.n_updated = counters[0], in.n_kept_updated = counters[1], in.n_data = counters[2], in.n_kept_data = counters[3];
  const uint64_t n_quads = 4ull * n_parked;
  if (n_quads > 0xffffffffull) return hipErrorInvalidValue;
  ProfScope ps(c, "kc_unpack", 32.0 * n_quads);
  kc_unpack<<<kc_grid(n_quads), KC_THREADS, 0, c->ls>>>(static_cast<const uint4*>(d_tiles),
                                                        reinterpret_cast<uint4*>(c->cache_arena.p), (uint32_t)n_quads,
                                                        static_cast<const uint4*>(d_tile_dir), n_tiles, c->cache_slots,
                                                        c->ds, in);
  return hipGetLastError();
}
