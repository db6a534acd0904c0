/*
 * k_grid.hip -- a 2.5-D semantic traversability grid of world-frame records (suma_world_surfel: what the world export
 * writes), for a planner: per cell of an x / y raster the ground height, what stands on it within the robot's height, the
 * voted class and a state.  The world frame has z up (the first scan's sensor frame).  Nothing in the reference does
 * this.  The host entries (validation, scratch, stats) are suma_grid.hip.
 *
 * Kernels (VGPRs: tools/isa_stats.py k_grid.hip; none uses scratch):
 *   kgr_classify  lane per record: label, cell key (or no key), member record; counts n_dropped and n_outside.
 *   kgr_reduce    lane per sorted position: the lane at the head of a run walks it and writes stage A of the cell and the
 *                 cell's entry of the run table.
 *   kgr_finish    lane per raster cell: stage B -- the reference height (own, or the nearest neighbour's), a second walk
 *                 over the cell's run, the state; writes the whole cell; counts the cells by state.
 *   kgr_fit       grid-stride over the records: the extent of the finite ones, for suma_world_grid_fit.
 *   between classify and reduce the sorts, the key gather, the run heads and the scan of k_group.hip.
 * One lane walks a run, in kgr_reduce and again in kgr_finish: a very full cell serialises on its lane, as a very full
 * voxel does in kw_reduce (k_world.hip).
 *
 * SPECIFICATION of suma_world_grid (fp32, every operation as written, no contraction: -ffp-contract=off; `/` correctly
 * rounded; tests/grid_shim.c restates it on the host, bit for bit).  NaN below is the quiet NaN 0x7fc00000.
 *
 * Per record with source index s (its position in the input):
 *   L = label < 260 ? label : 0.
 *   fx = floorf((x - origin_x) / cell_size), fy = floorf((y - origin_y) / cell_size).
 *   A record with a non-finite x, y or z is DROPPED (n_dropped).  A finite record with
 *   !(fx >= 0 && fx < width && fy >= 0 && fy < height) is OUTSIDE (n_outside).  Every other record is BINNED into cell
 *   c = (uint)fy * width + (uint)fx.
 * "More confident" orders two members: a number beats a NaN, the greater number beats the smaller, and of two equal
 *   numbers or two NaNs the smaller s wins.
 * Stage A, per cell with members:
 *   support = the member count; z_min / z_max over all members.  For every min and max of z here, -0 is below +0.
 *   vote (vote_weight and LabelVote, group_by_key.h): a member votes for its L with q = (uint32)rintf(clamp(prob, 0, 1) *
 *     65535.0f) (NaN: 0), summed per label in uint64; label = the greatest sum, on a tie the smallest id; prob =
 *     (float)sum_label / (float)sum_all; sum_all == 0: label = the L of the most confident member, prob = 0.
 *   A GROUND MEMBER has ground_label[L] != 0 && fabsf(nz) >= min_normal_z (a NaN nz fails).  n_ground = their count;
 *     ground_z = the z of the most confident ground member; ground_rough = max - min of the ground members' z;
 *     n_ground == 0: both NaN.
 * Stage B, per raster cell (ix, iy):
 *   n_ground > 0: g = ground_z, ground_source = 1.
 *   else, over the cells (ix + dx, iy + dy) inside the raster with |dx|, |dy| <= fill_radius and n_ground > 0: the one
 *     with the smallest dx * dx + dy * dy, on a tie the smallest dy, then the smallest dx; g = its ground_z; this cell's
 *     ground_z = g, ground_rough = NaN, ground_source = 2.
 *   else g = NaN, ground_source = 0.
 *   With a g (it is finite: a binned z is), per member h = z - g: h > clearance: overhang (n_overhang); else
 *     h > step_height: obstacle (n_obstacle; obstacle_z = the max z of these); else surface.  Without one, or without an
 *     obstacle, obstacle_z = NaN and the counts are 0.
 *   state, first match: support == 0: UNKNOWN (a filled ground_z is still reported); g NaN: NO_GROUND; n_obstacle > 0:
 *     OBSTACLE; else FREE.
 *   A cell without members: z_min = z_max = ground_rough = obstacle_z = NaN, prob = 0, label = 0, every count 0.
 * The grid is a pure function of the records and the parameters.
 *
 * Decomposition: as k_world.hip's voxel mode -- two stable radix sorts of (key, source index) in double buffers
 * (group_sort_by_value_then_key): by label (9 bits), then by cell index.  The second sort takes only the bits
 * width * height needs: b with 2^b > width * height, so that the low b bits of the no-key value (all ones) exceed every
 * cell index and the records without a cell sort behind every cell.  Inside a run the members are ordered by label, then
 * by source index, so the vote needs one running sum.  kgr_finish reads its neighbours from the run table, which
 * kgr_reduce wrote and nothing writes after it, never from d_cells: no lane reads what another lane of the launch writes.
 */
#include <cmath>
#include <cstring>

#include <rocprim/types/double_buffer.hpp>

#include "suma_internal.h"
#include "draw_vertex.h"
#include "group_by_key.h"

#define GRID_THREADS 256
#define GRID_CLASSIFY_ITEMS 8
#define GRID_LABEL_WORDS ((SUMA_DRAW_COLORS + 31) / 32)
#define GRID_NAN 0x7fc00000u

struct GridArgs {
  const float4* rec; /* 3 float4 a record */
  uint32_t n;
  float cell_size, origin_x, origin_y;
  uint32_t width, height;
  float min_normal_z, step_height, clearance;
  int32_t fill_radius;
  uint32_t ground[GRID_LABEL_WORDS];
};

/* "more confident": (conf, s) against the best so far */
SDEV bool grid_better(float conf, uint32_t s, float best, uint32_t best_s) {
  const bool cn = conf != conf, bn = best != best;
  if (cn != bn) return bn;
  if (!cn && conf != best) return conf > best;
  return s < best_s;
}

/* z below / above the extreme so far; -0 counts as below +0, so that an extreme does not depend on the members' order */
SDEV bool grid_below(float z, float m) { return z < m || (z == m && __float_as_uint(z) > __float_as_uint(m)); }
SDEV bool grid_above(float z, float m) { return z > m || (z == m && __float_as_uint(z) < __float_as_uint(m)); }

/* a block's counts go to LDS first and to the global counters once (k_world.hip measured one atomic per wave on one
 * address as most of its classify kernel) */
__global__ void __launch_bounds__(GRID_THREADS)
    kgr_classify(GridArgs a, unsigned long long* __restrict__ key0, uint32_t* __restrict__ lab0, uint32_t* __restrict__ idx0,
                 uint4* __restrict__ member, uint32_t* __restrict__ counters) {
  __shared__ uint32_t block_counts[2];
  if (threadIdx.x < 2) block_counts[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t nd = 0, no = 0;
  const unsigned long long first = (unsigned long long)blockIdx.x * (GRID_THREADS * GRID_CLASSIFY_ITEMS) + threadIdx.x;
#pragma unroll 2
  for (uint32_t it = 0; it < GRID_CLASSIFY_ITEMS; ++it) {
    const unsigned long long s64 = first + (unsigned long long)it * GRID_THREADS;
    if (s64 >= a.n) break;
    const uint32_t s = (uint32_t)s64;
    const float4 r0 = a.rec[3 * (size_t)s], r1 = a.rec[3 * (size_t)s + 1], r2 = a.rec[3 * (size_t)s + 2];
    uint32_t L = __float_as_uint(r2.x);
    L = (L < (uint32_t)SUMA_DRAW_COLORS) ? L : 0u;
    unsigned long long key = VOXEL_NO_KEY;
    if (!(finite_f(r0.x) && finite_f(r0.y) && finite_f(r0.z))) {
      ++nd;
    } else {
      const float fx = sdm_floor((r0.x - a.origin_x) / a.cell_size), fy = sdm_floor((r0.y - a.origin_y) / a.cell_size);
      if (!(fx >= 0.0f && fx < (float)a.width && fy >= 0.0f && fy < (float)a.height)) ++no;
      else key = (unsigned long long)((uint32_t)fy * a.width + (uint32_t)fx);
    }
    const bool ground = ((a.ground[L >> 5] >> (L & 31u)) & 1u) && fabsf(r1.z) >= a.min_normal_z;
    key0[s] = key;
    lab0[s] = L;
    idx0[s] = s;
    member[s] = make_uint4(__float_as_uint(r0.z), __float_as_uint(r1.w), (vote_weight(r2.y) << 16) | L, ground ? 1u : 0u);
  }
  if (nd) atomicAdd(&block_counts[0], nd); /* LDS; integer sums do not depend on the order */
  if (no) atomicAdd(&block_counts[1], no);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (block_counts[0]) atomicAdd(&counters[GRID_DROPPED], block_counts[0]);
    if (block_counts[1]) atomicAdd(&counters[GRID_OUTSIDE], block_counts[1]);
  }
}

/* cell layout in float4s: {ground_z, ground_rough, z_min, z_max} {obstacle_z, prob, label, support}
 * {n_ground, n_obstacle, n_overhang, state | ground_source << 8} */
__global__ void __launch_bounds__(GRID_THREADS)
    kgr_reduce(uint32_t n, uint32_t n_cells, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ idx,
               const uint4* __restrict__ member, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
               uint4* __restrict__ runs, suma_grid_cell* __restrict__ cells, uint32_t* __restrict__ counters) {
  const uint32_t j = blockIdx.x * GRID_THREADS + threadIdx.x;
  if (j >= n) return;
  const uint32_t f = flag[j];
  if (j == n - 1u) counters[GRID_OCCUPIED] = pos[j] + f;
  if (!f) return;
  const unsigned long long key = keys[j];
  if (key >= n_cells) return; /* kgr_classify writes no such key */
  LabelVote tally;
  uint32_t support = 0, rep = 0, rep_label = 0, n_ground = 0, g_rep = 0;
  float rep_conf = 0.0f, z_min = 0.0f, z_max = 0.0f, g_conf = 0.0f, g_z = 0.0f, g_min = 0.0f, g_max = 0.0f;
  for (uint32_t k = j; k < n && keys[k] == key; ++k) {
    const uint32_t s = idx[k];
    const uint4 m = member[s];
    const float z = __uint_as_float(m.x), conf = __uint_as_float(m.y);
    const uint32_t L = m.z & 0xffffu;
    tally.add(L, m.z >> 16);
    if (support == 0 || grid_better(conf, s, rep_conf, rep)) rep_conf = conf, rep = s, rep_label = L;
    z_min = (support == 0 || grid_below(z, z_min)) ? z : z_min;
    z_max = (support == 0 || grid_above(z, z_max)) ? z : z_max;
    if (m.w) {
      if (n_ground == 0 || grid_better(conf, s, g_conf, g_rep)) g_conf = conf, g_rep = s, g_z = z;
      g_min = (n_ground == 0 || grid_below(z, g_min)) ? z : g_min;
      g_max = (n_ground == 0 || grid_above(z, g_max)) ? z : g_max;
      ++n_ground;
    }
    ++support;
  }
  uint32_t label;
  const float prob = tally.close(rep_label, &label);
  const float nan = __uint_as_float(GRID_NAN);
  const float ground_z = n_ground ? g_z : nan, rough = n_ground ? g_max - g_min : nan;
  float4* dst = reinterpret_cast<float4*>(cells) + 3 * (size_t)key;
  dst[0] = f4(ground_z, rough, z_min, z_max);
  dst[1] = f4(nan, prob, __uint_as_float(label), __uint_as_float(support));
  dst[2] = f4(__uint_as_float(n_ground), 0.0f, 0.0f, 0.0f);
  runs[key] = make_uint4(j, support, n_ground, __float_as_uint(ground_z));
}

__global__ void __launch_bounds__(GRID_THREADS)
    kgr_finish(GridArgs a, uint32_t n_cells, const uint32_t* __restrict__ idx, const uint4* __restrict__ member,
               const uint4* __restrict__ runs, suma_grid_cell* __restrict__ cells, uint32_t* __restrict__ counters) {
  __shared__ uint32_t block_counts[4]; /* free, obstacle, no ground, filled */
  if (threadIdx.x < 4) block_counts[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * GRID_THREADS + threadIdx.x;
  if (c < n_cells) {
    const float nan = __uint_as_float(GRID_NAN);
    const uint4 run = runs[c]; /* start, support, n_ground, ground_z */
    float4* dst = reinterpret_cast<float4*>(cells) + 3 * (size_t)c;
    float4 c0 = f4(nan, nan, nan, nan), c1 = f4(nan, 0.0f, 0.0f, 0.0f);
    if (run.y) c0 = dst[0], c1 = dst[1]; /* this lane's own cell, as kgr_reduce left it */
    float g = nan;
    uint32_t source = 0;
    if (run.z) {
      g = __uint_as_float(run.w), source = 1;
    } else if (a.fill_radius > 0) {
      const int32_t ix = (int32_t)(c % a.width), iy = (int32_t)(c / a.width);
      int32_t best = 0x7fffffff;
      for (int32_t dy = -a.fill_radius; dy <= a.fill_radius; ++dy) {
        const int32_t y = iy + dy;
        if (y < 0 || y >= (int32_t)a.height) continue;
        for (int32_t dx = -a.fill_radius; dx <= a.fill_radius; ++dx) {
          const int32_t x = ix + dx, d2 = dx * dx + dy * dy;
          if (x < 0 || x >= (int32_t)a.width || d2 >= best) continue; /* ascending dy, then dx: a tie keeps the first */
          const uint4 q = runs[(uint32_t)y * a.width + (uint32_t)x];
          if (q.z) best = d2, g = __uint_as_float(q.w), source = 2;
        }
      }
      if (source == 2) c0.x = g, c0.y = nan;
    }
    uint32_t n_obstacle = 0, n_overhang = 0;
    if (source && run.y) {
      float top = 0.0f;
      for (uint32_t k = run.x; k < run.x + run.y; ++k) {
        const float z = __uint_as_float(member[idx[k]].x), h = z - g;
        if (h > a.clearance) {
          ++n_overhang;
        } else if (h > a.step_height) {
          top = (n_obstacle == 0 || grid_above(z, top)) ? z : top;
          ++n_obstacle;
        }
      }
      if (n_obstacle) c1.x = top;
    }
    const uint32_t state = !run.y ? SUMA_GRID_UNKNOWN : (!source ? SUMA_GRID_NO_GROUND : (n_obstacle ? SUMA_GRID_OBSTACLE : SUMA_GRID_FREE));
    dst[0] = c0;
    dst[1] = c1;
    dst[2] = f4(__uint_as_float(run.z), __uint_as_float(n_obstacle), __uint_as_float(n_overhang),
                __uint_as_float(state | (source << 8)));
    if (state == SUMA_GRID_FREE) atomicAdd(&block_counts[0], 1u);
    if (state == SUMA_GRID_OBSTACLE) atomicAdd(&block_counts[1], 1u);
    if (state == SUMA_GRID_NO_GROUND) atomicAdd(&block_counts[2], 1u);
    if (source == 2) atomicAdd(&block_counts[3], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4 && block_counts[threadIdx.x]) atomicAdd(&counters[GRID_FREE + threadIdx.x], block_counts[threadIdx.x]);
}

/* floats as unsigned integers of the same order (finite values; -0 below +0) */
SDEV uint32_t grid_ordered(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
float grid_ordered_float(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  float v;
  memcpy(&v, &u, 4);
  return v;
}

/* min / max of x and y over the records whose x, y and z are finite: per lane, across the wave by shuffles, across the
 * block's waves through LDS, then one integer atomic min / max per block and quantity -- the result does not depend on
 * the order.  A block without a finite record sends nothing. */
#define GRID_FIT_BLOCKS 1024u
__global__ void __launch_bounds__(GRID_THREADS)
    kgr_fit(const float4* __restrict__ rec, uint32_t n, uint32_t* __restrict__ counters) {
  __shared__ float part[GRID_THREADS / 64][4];
  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  for (size_t s = (size_t)blockIdx.x * GRID_THREADS + threadIdx.x; s < n; s += (size_t)gridDim.x * GRID_THREADS) {
    const float4 r0 = rec[3 * s];
    if (!(finite_f(r0.x) && finite_f(r0.y) && finite_f(r0.z))) continue;
    lo_x = fmin_(lo_x, r0.x), hi_x = fmax_(hi_x, r0.x);
    lo_y = fmin_(lo_y, r0.y), hi_y = fmax_(hi_y, r0.y);
  }
  for (int off = 32; off > 0; off >>= 1) {
    lo_x = fmin_(lo_x, __shfl_xor(lo_x, off, 64)), hi_x = fmax_(hi_x, __shfl_xor(hi_x, off, 64));
    lo_y = fmin_(lo_y, __shfl_xor(lo_y, off, 64)), hi_y = fmax_(hi_y, __shfl_xor(hi_y, off, 64));
  }
  if ((threadIdx.x & 63u) == 0) {
    float* p = part[threadIdx.x >> 6];
    p[0] = lo_x, p[1] = lo_y, p[2] = hi_x, p[3] = hi_y;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GRID_THREADS / 64; ++w) {
      lo_x = fmin_(lo_x, part[w][0]), lo_y = fmin_(lo_y, part[w][1]);
      hi_x = fmax_(hi_x, part[w][2]), hi_y = fmax_(hi_y, part[w][3]);
    }
    if (lo_x <= hi_x) { /* at least one finite record */
      atomicMin(&counters[GRID_FIT_MIN_X], grid_ordered(lo_x));
      atomicMin(&counters[GRID_FIT_MIN_Y], grid_ordered(lo_y));
      atomicMax(&counters[GRID_FIT_MAX_X], grid_ordered(hi_x));
      atomicMax(&counters[GRID_FIT_MAX_Y], grid_ordered(hi_y));
    }
  }
}

hipError_t launch_grid_fit(suma_ctx* c, const suma_world_surfel* d_records, uint32_t n) {
  hipStream_t st = c->stream;
  uint32_t* counters = c->grid_counters;
  hipError_t e = hipMemsetAsync(counters, 0, GRID_COUNTERS * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(counters + GRID_FIT_MIN_X, 0xff, 2 * sizeof(uint32_t), st)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  ProfScope ps(c, "grid_fit", 16.0 * n);
  const size_t blocks = ((size_t)n + GRID_THREADS - 1) / GRID_THREADS;
  kgr_fit<<<(unsigned)(blocks < GRID_FIT_BLOCKS ? blocks : GRID_FIT_BLOCKS), GRID_THREADS, 0, st>>>(
      reinterpret_cast<const float4*>(d_records), n, counters);
  return hipGetLastError();
}

hipError_t launch_grid(suma_ctx* c, const suma_grid_params& gp, const suma_world_surfel* d_records, uint32_t n,
                       suma_grid_cell* d_cells) {
  hipStream_t st = c->stream;
  char* scratch = c->world_scratch;
  void* tmp = c->world_tmp;
  const size_t tmp_bytes = c->world_tmp.cap;
  uint4* runs = c->grid_runs;
  uint32_t* counters = c->grid_counters;
  GridArgs a;
  a.rec = reinterpret_cast<const float4*>(d_records);
  a.n = n;
  a.cell_size = gp.cell_size, a.origin_x = gp.origin_x, a.origin_y = gp.origin_y;
  a.width = gp.width, a.height = gp.height;
  a.min_normal_z = gp.min_normal_z, a.step_height = gp.step_height, a.clearance = gp.clearance;
  a.fill_radius = (int32_t)gp.fill_radius;
  memset(a.ground, 0, sizeof(a.ground));
  for (uint32_t l = 0; l < SUMA_DRAW_COLORS; ++l)
    if (gp.ground_label[l]) a.ground[l >> 5] |= 1u << (l & 31u);
  const uint32_t n_cells = gp.width * gp.height;
  unsigned key_bits = 1;
  while ((1ull << key_bits) <= n_cells) ++key_bits;
  const unsigned cell_blocks = (n_cells + GRID_THREADS - 1) / GRID_THREADS;

  hipError_t e = hipMemsetAsync(counters, 0, GRID_COUNTERS * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(runs, 0, (size_t)n_cells * sizeof(uint4), st)) != hipSuccess) return e; /* no run, no ground */
  const uint32_t* sorted_idx = nullptr;
  const uint4* member = nullptr;
  if (n) {
    /* member 16 n | two key arrays 8 n each | two label arrays, then two index arrays, 4 n each (k_world.hip's layout);
     * the label pair is free after the first sort and takes the head flags and ranks */
    uint4* mem = reinterpret_cast<uint4*>(scratch);
    unsigned long long* keyA = reinterpret_cast<unsigned long long*>(scratch + (size_t)16 * n);
    unsigned long long* keyB = keyA + n;
    uint32_t* u0 = reinterpret_cast<uint32_t*>(scratch + (size_t)32 * n);
    uint32_t *u1 = u0 + n, *u2 = u1 + n, *u3 = u2 + n;
    {
      ProfScope ps(c, "grid_classify", 80.0 * n);
      const unsigned per_block = GRID_THREADS * GRID_CLASSIFY_ITEMS;
      kgr_classify<<<(unsigned)(((size_t)n + per_block - 1) / per_block), GRID_THREADS, 0, st>>>(a, keyA, u0, u2, mem, counters);
    }
    rocprim::double_buffer<uint32_t> lab(u0, u1), idx(u2, u3);
    rocprim::double_buffer<unsigned long long> key(keyB, keyA); /* keyB is filled from keyA, which is then dead */
    {
      ProfScope ps(c, "grid_sort", 64.0 * n);
      if ((e = group_sort_by_value_then_key(tmp, tmp_bytes, lab, 9u, keyA, key, key_bits, idx, n, st)) != hipSuccess) return e;
    }
    {
      ProfScope ps(c, "grid_reduce", 40.0 * n);
      if ((e = group_heads(tmp, tmp_bytes, key.current(), VOXEL_NO_KEY, u0, u1, n, st)) != hipSuccess) return e;
      kgr_reduce<<<(unsigned)(((size_t)n + GRID_THREADS - 1) / GRID_THREADS), GRID_THREADS, 0, st>>>(
          n, n_cells, key.current(), idx.current(), mem, u0, u1, runs, d_cells, counters);
    }
    sorted_idx = idx.current(), member = mem;
  }
  ProfScope ps(c, "grid_finish", 64.0 * n_cells + 20.0 * n);
  kgr_finish<<<cell_blocks, GRID_THREADS, 0, st>>>(a, n_cells, sorted_idx, member, runs, d_cells, counters);
  return hipGetLastError();
}
