/*
 * k_plan.hip -- planning on the traversability grid (k_grid.hip): per raster cell the clearance to the nearest blocked
 * cell, whether a robot of a given radius may stand there, the cost-to-go to a set of goal cells and the direction of the
 * cheapest move; and paths read off that field.  Nothing in the reference does this.  The host entries (validation,
 * scratch, stats, the exchange of goals, starts and paths) are suma_plan.hip.
 *
 * SPECIFICATION of suma_grid_plan_field and suma_grid_plan_paths (tests/plan_shim.c restates it sequentially, byte for
 * byte).  Every quantity is an integer, or one fp32 comparison evaluated as written (-ffp-contract=off; sqrtf and `*`
 * correctly rounded).  Cells are (x, y) with index y * width + x; R = max_clear_cells; INF = 0xffffffff.
 * Directions k = 0..7 are E, NE, N, NW, W, SW, S, SE as (dx, dy) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1); the
 * row index grows with y.  k is diagonal iff odd.
 *
 * 1. Blocked.  L = label < 260 ? label : 0.  A cell is BLOCKED iff state is OBSTACLE or NO_GROUND; or state is UNKNOWN and
 *    unknown_blocked != 0; or label_cost[L] == 0; or max_rough is a number and ground_rough > max_rough (a NaN roughness
 *    never blocks).  Any other state value than the four of the grid counts as UNKNOWN.
 * 2. Clearance.  clear2(c) = min((R + 1)^2, min over blocked cells b of dx^2 + dy^2), dx and dy in whole cells: the exact
 *    squared Euclidean distance up to the cap.  A blocked cell has 0.  Cells outside the raster are not blocked.  (A
 *    blocked cell with d^2 < (R + 1)^2 has |dx|, |dy| <= R: a +-R window finds it.)
 * 3. Traversable.  !blocked && sqrtf((float)clear2) * cell_size >= robot_radius.
 * 4. Edges.  The move from c to its neighbour n in direction k is ALLOWED iff n is inside the raster; c and n are
 *    traversable; fabsf(ground_z(c) - ground_z(n)) <= max_step (a NaN on either side forbids it); and, for a diagonal k,
 *    the cells (x + dx, y) and (x, y + dy) are traversable.  Its cost is base * (w(c) + w(n)), base = 10 straight, 14
 *    diagonal, w(c) = label_cost[L] + soft_weight * max(0, soft_cells - s(c)), s(c) = the largest integer with s * s <=
 *    clear2(c).  Rule and cost are symmetric; every cost is >= 20.
 * 5. Field.  cost(g) = 0 for every goal g that is traversable; the others are ignored and counted (n_goals_ignored; n_goals
 *    is the number of entries given; a cell given twice counts twice).  Every other cell: the minimum over its allowed
 *    edges of cost(n) + edge(c, n), over the n with cost(n) != INF; INF without one.  Costs are uint32 and the entry
 *    refuses rasters on which one could wrap.  This is the unique fixed point of a min-plus equation with positive costs:
 *    it does not depend on the order of relaxation.
 * 6. Next.  8 where cost == 0 (the traversable goals: no other cell has cost 0); 255 where cost == INF; otherwise the
 *    smallest k whose allowed edge has cost(n_k) != INF and cost(n_k) + edge == cost(c).
 * 7. Output.  suma_plan_cell {cost, clear2, flags = blocked | traversable << 1 | (cost != INF) << 2, next}.  Stats:
 *    n_blocked, n_traversable, n_reached = cells with cost != INF, n_goals, n_goals_ignored, max_cost = the largest cost
 *    != INF (0 without one), n_rounds (diagnostic, not specified).
 * 8. Paths, per start s (a cell index, or "outside"), with path_capacity cells of room; the field is not trusted:
 *      outside: status START_OUTSIDE, length 0, cost INF.  Otherwise cost = field[s].cost;
 *      field[s].next == 255: UNREACHED, length 0.
 *      else c = s, length = 1, record c; repeat at most width * height times:
 *        k = field[c].next.  k == 8: OK, stop.  k > 7: BAD_FIELD, stop.  n = c moved by direction k; n outside the raster:
 *        BAD_FIELD, stop.  !(field[n].cost < field[c].cost): BAD_FIELD, stop.  c = n, length += 1, record c.
 *      The bound exhausted: BAD_FIELD.  OK with length > path_capacity: TRUNCATED.
 *    "record": the cell's index goes to position length - 1 of the start's row if that is below path_capacity.  Row entries
 *    that no record wrote are 0xffffffff.
 *
 * Kernels (VGPRs and LDS: DESIGN section 18, tools/isa_stats.py k_plan.hip; none uses scratch memory):
 *   kpl_classify   lane per cell: reads the 48-byte grid cell once, writes the 8-byte record {ground_z, blocked |
 *                  label_cost << 8}; counts the blocked per block.
 *   kpl_clear_row  64 x 4 cells a block, a row and +-R of halo as bytes in LDS: the distance along the row to the nearest
 *                  blocked cell within +-R (R + 1: none), one byte a cell.
 *   kpl_clear_col  64 x 16 cells a block, the row distances of +-R rows in LDS: clear2 = min over |dy| <= R of
 *                  d_row(x, y + dy)^2 + dy^2, rows taken outwards and left once dy^2 reaches the best; the traversable
 *                  bit and w; starts the caller's field cell.
 *   kpl_edges      lane per cell: the 8-bit mask of allowed moves, packed with w.
 *   kpl_seed       lane per goal: cost 0 on a traversable goal, else counted.
 *   kpl_relax      one relaxation round, a block per PLAN_TILE x PLAN_TILE tile (below).
 *   kpl_next       lane per cell: next, the flags, the whole field cell; counts reached / traversable, max cost.
 *   kpl_walk       a wave per start (below).
 *
 * Relaxation.  Two cost arrays; round r reads one and writes the other, so no lane reads what another block writes in the
 * same launch.  A block loads its tile with one cell of halo (cost, and w | edge mask) into LDS, relaxes the tile's own
 * cells there until none changes -- at most PLAN_TILE^2 sweeps, the most edges a shortest way inside the tile can have;
 * a sweep computes every new value from the old ones, a barrier, then stores -- and writes the tile.  The halo is fixed
 * during a launch.  A tile whose cells ended lower than they were loaded raises its byte of this round's tile flags and the
 * round's word.  Round r skips a tile none of whose 3 x 3 tile neighbourhood raised its flag in round r - 1: its input is
 * what it was a round ago, when it changed nothing, and both arrays hold its cells already.  The host enqueues
 * PLAN_ROUND_BATCH rounds and reads their words once; a round returns at once when the round before it in the batch
 * changed nothing.  The field is complete when a round changes nothing; width * height rounds are the hard bound.  No
 * kernel waits for another block, and every loop has a bound that follows from its shape.
 *
 * Walk.  `next` is stored, so a walk is a chain of dependent loads: every lane of the wave follows the same chain (the
 * loads are of one address, one transaction), lane i keeps the i-th cell of each run of 64, and the wave writes the run
 * in one coalesced store.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"

#define PLAN_THREADS 256
#define PLAN_INF 0xffffffffu
#define PLAN_ROW_W 64 /* columns of a clearance block */
#define PLAN_ROW_H 4  /* rows of a row-pass block */
#define PLAN_COL_H 16 /* rows of a column-pass block */
#define PLAN_R_MAX ((int)SUMA_PLAN_MAX_CLEAR_CELLS)
#define PLAN_HALO (PLAN_TILE + 2u)
/* the record kpl_clear_col leaves in rec.y, and what kpl_edges packs for the relaxation: w in the low 16 bits */
#define PLAN_NODE_TRAV (1u << 24)
#define PLAN_NODE_BLOCKED (1u << 25)

SDEV int plan_dx(uint32_t k) { return (int)((0x83u >> k) & 1u) - (int)((0x38u >> k) & 1u); }
SDEV int plan_dy(uint32_t k) { return (int)((0x0eu >> k) & 1u) - (int)((0xe0u >> k) & 1u); }

struct PlanArgs {
  uint32_t width, height, n_cells;
  float cell_size, robot_radius, max_step, max_rough;
  uint32_t unknown_blocked, R, soft_cells, soft_weight;
};
struct PlanLabelCost {
  uint32_t w[SUMA_DRAW_COLORS / 4]; /* label_cost, four to a word */
};

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_classify(PlanArgs a, PlanLabelCost lc, const float4* __restrict__ cells, uint2* __restrict__ rec,
                 uint32_t* __restrict__ counters) {
  __shared__ uint32_t block_count;
  if (threadIdx.x == 0) block_count = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (c < a.n_cells) {
    const float4 c0 = cells[3 * (size_t)c], c1 = cells[3 * (size_t)c + 1], c2 = cells[3 * (size_t)c + 2];
    uint32_t L = __float_as_uint(c1.z);
    L = (L < (uint32_t)SUMA_DRAW_COLORS) ? L : 0u;
    const uint32_t cost = (lc.w[L >> 2] >> (8u * (L & 3u))) & 0xffu;
    const uint32_t state = __float_as_uint(c2.w) & 0xffu;
    bool blocked = state == SUMA_GRID_OBSTACLE || state == SUMA_GRID_NO_GROUND;
    blocked = blocked || (state != SUMA_GRID_FREE && a.unknown_blocked);
    blocked = blocked || cost == 0u;
    blocked = blocked || (a.max_rough == a.max_rough && c0.y > a.max_rough);
    rec[c] = make_uint2(__float_as_uint(c0.x), (blocked ? 1u : 0u) | (cost << 8));
    if (blocked) atomicAdd(&block_count, 1u); /* LDS; integer sums do not depend on the order */
  }
  __syncthreads();
  if (threadIdx.x == 0 && block_count) atomicAdd(&counters[PLAN_BLOCKED], block_count);
}

/* blocks are numbered along x first: tile (b % tiles_x, b / tiles_x) */
__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_clear_row(PlanArgs a, uint32_t tiles_x, const uint2* __restrict__ rec, uint8_t* __restrict__ drow) {
  __shared__ uint8_t s[PLAN_ROW_H][PLAN_ROW_W + 2 * PLAN_R_MAX];
  const int R = (int)a.R, lane = (int)(threadIdx.x & 63u), row = (int)(threadIdx.x >> 6);
  const int x0 = (int)(blockIdx.x % tiles_x) * PLAN_ROW_W;
  const uint32_t y = (blockIdx.x / tiles_x) * PLAN_ROW_H + (uint32_t)row;
  for (int i = lane; i < PLAN_ROW_W + 2 * R; i += 64) {
    const int x = x0 - R + i;
    uint8_t b = 0;
    if (y < a.height && x >= 0 && x < (int)a.width) b = (uint8_t)(rec[(size_t)y * a.width + (uint32_t)x].y & 1u);
    s[row][i] = b;
  }
  __syncthreads();
  const int x = x0 + lane;
  if (y >= a.height || x >= (int)a.width) return;
  int d = 0;
  for (; d <= R; ++d)
    if (s[row][lane + R - d] | s[row][lane + R + d]) break;
  drow[(size_t)y * a.width + (uint32_t)x] = (uint8_t)d; /* R + 1: none within +-R */
}

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_clear_col(PlanArgs a, uint32_t tiles_x, const uint8_t* __restrict__ drow, uint2* __restrict__ rec,
                  uint2* __restrict__ field) {
  __shared__ uint8_t s[PLAN_COL_H + 2 * PLAN_R_MAX][PLAN_ROW_W];
  const int R = (int)a.R, lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int x = (int)(blockIdx.x % tiles_x) * PLAN_ROW_W + lane;
  const long long y0 = (long long)(blockIdx.x / tiles_x) * PLAN_COL_H;
  for (int i = wave; i < PLAN_COL_H + 2 * R; i += PLAN_THREADS / 64) {
    const long long y = y0 - R + i;
    uint8_t d = (uint8_t)(R + 1);
    if (y >= 0 && y < (long long)a.height && x < (int)a.width) d = drow[(size_t)y * a.width + (uint32_t)x];
    s[i][lane] = d;
  }
  __syncthreads();
  if (x >= (int)a.width) return;
  const uint32_t cap = (a.R + 1u) * (a.R + 1u);
  for (int j = wave; j < PLAN_COL_H; j += PLAN_THREADS / 64) {
    const long long y = y0 + j;
    if (y >= (long long)a.height) break;
    uint32_t best = cap;
    for (int dy = 0; dy <= R && (uint32_t)(dy * dy) < best; ++dy) {
      const uint32_t up = s[j + R + dy][lane], dn = s[j + R - dy][lane];
      const uint32_t d = up < dn ? up : dn; /* R + 1 (none) gives >= cap */
      const uint32_t d2 = d * d + (uint32_t)(dy * dy);
      best = d2 < best ? d2 : best;
    }
    const size_t c = (size_t)y * a.width + (uint32_t)x;
    const uint32_t r = rec[c].y; /* this lane's own cell, as kpl_classify left it */
    const bool blocked = r & 1u;
    const bool trav = !blocked && sdm_sqrt((float)best) * a.cell_size >= a.robot_radius;
    uint32_t sq = 0; /* min(s(c), soft_cells) */
    while (sq < a.soft_cells && (sq + 1u) * (sq + 1u) <= best) ++sq;
    const uint32_t w = (r >> 8) + a.soft_weight * (a.soft_cells - sq);
    rec[c].y = w | (trav ? PLAN_NODE_TRAV : 0u) | (blocked ? PLAN_NODE_BLOCKED : 0u);
    field[c] = make_uint2(PLAN_INF, best | ((blocked ? 1u : 0u) | (trav ? 2u : 0u)) << 16 | 255u << 24);
  }
}

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_edges(PlanArgs a, const uint2* __restrict__ rec, uint32_t* __restrict__ wm) {
  const uint32_t c = blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (c >= a.n_cells) return;
  const uint2 me = rec[c];
  uint32_t mask = 0;
  if (me.y & PLAN_NODE_TRAV) {
    const int x = (int)(c % a.width), y = (int)(c / a.width);
    const float gz = __uint_as_float(me.x);
    uint32_t trav = 0; /* bit k: the neighbour in direction k is inside and traversable */
    float nz[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      const int nx = x + plan_dx(k), ny = y + plan_dy(k);
      nz[k] = 0.0f;
      if (nx < 0 || ny < 0 || nx >= (int)a.width || ny >= (int)a.height) continue;
      const uint2 q = rec[(size_t)ny * a.width + (uint32_t)nx];
      nz[k] = __uint_as_float(q.x);
      if (q.y & PLAN_NODE_TRAV) trav |= 1u << k;
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      bool ok = ((trav >> k) & 1u) && fabsf(gz - nz[k]) <= a.max_step;
      if (k & 1u) ok = ok && ((trav >> ((k + 1u) & 7u)) & 1u) && ((trav >> (k - 1u)) & 1u); /* no corner cutting */
      if (ok) mask |= 1u << k;
    }
  }
  wm[c] = (me.y & 0xffffu) | (mask << 16);
}

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_seed(uint32_t n_goals, const uint32_t* __restrict__ goals, const uint2* __restrict__ rec, uint32_t* __restrict__ cost,
             uint32_t* __restrict__ counters) {
  const uint32_t i = blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (i >= n_goals) return;
  const uint32_t g = goals[i]; /* inside the raster: the entry's check */
  if (rec[g].y & PLAN_NODE_TRAV) cost[g] = 0u; /* a cell given twice is written twice, with the same value */
  else atomicAdd(&counters[PLAN_GOALS_IGNORED], 1u);
}

/* the cost of the move in direction k between cells of weights w and wn */
SDEV uint32_t plan_edge(uint32_t k, uint32_t w, uint32_t wn) { return ((k & 1u) ? 14u : 10u) * (w + wn); }

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_relax(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, int first, const uint32_t* __restrict__ wm,
              const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint8_t* __restrict__ tile_prev,
              uint8_t* __restrict__ tile_cur, const uint32_t* __restrict__ round_prev, uint32_t* __restrict__ round_cur) {
  __shared__ uint32_t s_cost[PLAN_HALO * PLAN_HALO], s_wm[PLAN_HALO * PLAN_HALO];
  if (round_prev && *round_prev == 0u) return; /* the round before changed nothing: the field is complete */
  const uint32_t tile = blockIdx.x;
  const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
  if (!first) {
    uint32_t active = 0;
    for (int j = -1; j <= 1; ++j)
      for (int i = -1; i <= 1; ++i) {
        const int qx = tx + i, qy = ty + j;
        if (qx >= 0 && qy >= 0 && qx < (int)tiles_x && qy < (int)tiles_y) active |= tile_prev[(size_t)qy * tiles_x + (uint32_t)qx];
      }
    if (!active) { /* uniform over the block */
      if (threadIdx.x == 0) tile_cur[tile] = 0;
      return;
    }
  }
  const long long gx0 = (long long)tx * PLAN_TILE - 1, gy0 = (long long)ty * PLAN_TILE - 1;
  for (uint32_t i = threadIdx.x; i < PLAN_HALO * PLAN_HALO; i += PLAN_THREADS) {
    const long long gx = gx0 + (i % PLAN_HALO), gy = gy0 + (i / PLAN_HALO);
    uint32_t cv = PLAN_INF, wv = 0u;
    if (gx >= 0 && gy >= 0 && gx < (long long)width && gy < (long long)height) {
      const size_t g = (size_t)gy * width + (size_t)gx;
      cv = src[g], wv = wm[g];
    }
    s_cost[i] = cv, s_wm[i] = wv;
  }
  __syncthreads();
  /* this lane's four cells: column lx, rows ly + 8 j */
  const uint32_t lx = threadIdx.x & (PLAN_TILE - 1u), ly = threadIdx.x / PLAN_TILE;
  constexpr uint32_t PER = PLAN_TILE * PLAN_TILE / PLAN_THREADS, STEP = PLAN_THREADS / PLAN_TILE;
  uint32_t loaded[PER], cur[PER], own[PER];
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const uint32_t at = (ly + STEP * j + 1u) * PLAN_HALO + lx + 1u;
    loaded[j] = cur[j] = s_cost[at];
    own[j] = s_wm[at];
  }
  for (uint32_t sweep = 0; sweep < PLAN_TILE * PLAN_TILE; ++sweep) {
    uint32_t nv[PER];
    bool lower = false;
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
      const int at = (int)((ly + STEP * j + 1u) * PLAN_HALO + lx + 1u);
      const uint32_t w = own[j] & 0xffffu, mask = own[j] >> 16;
      uint32_t best = cur[j];
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const int n = at + plan_dy(k) * (int)PLAN_HALO + plan_dx(k);
        const uint32_t cn = s_cost[n];
        if (cn == PLAN_INF) continue;
        const uint32_t cand = cn + plan_edge(k, w, s_wm[n] & 0xffffu);
        best = cand < best ? cand : best;
      }
      nv[j] = best;
      lower = lower || best < cur[j];
    }
    if (!__syncthreads_or(lower ? 1 : 0)) break; /* every read of the sweep is done */
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j)
      if (nv[j] < cur[j]) s_cost[(ly + STEP * j + 1u) * PLAN_HALO + lx + 1u] = cur[j] = nv[j];
    __syncthreads();
  }
  bool changed = false;
#pragma unroll
  for (uint32_t j = 0; j < PER; ++j) {
    const long long gx = gx0 + 1 + lx, gy = gy0 + 1 + ly + STEP * j;
    if (gx < (long long)width && gy < (long long)height) dst[(size_t)gy * width + (size_t)gx] = cur[j];
    changed = changed || cur[j] < loaded[j];
  }
  const int any = __syncthreads_or(changed ? 1 : 0);
  if (threadIdx.x == 0) {
    tile_cur[tile] = any ? 1 : 0;
    if (any) atomicOr(round_cur, 1u);
  }
}

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_next(uint32_t width, uint32_t height, uint32_t n_cells, const uint32_t* __restrict__ wm, const uint32_t* __restrict__ cost,
             uint2* __restrict__ field, uint32_t* __restrict__ counters) {
  __shared__ uint32_t block_counts[3]; /* traversable, reached, max cost */
  if (threadIdx.x < 3) block_counts[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * PLAN_THREADS + threadIdx.x;
  if (c < n_cells) {
    const uint32_t mine = cost[c], me = wm[c];
    uint32_t next = 255u;
    if (mine == 0u) {
      next = 8u;
    } else if (mine != PLAN_INF) {
      const int x = (int)(c % width), y = (int)(c / width);
#pragma unroll
      for (uint32_t k = 0; k < 8; ++k) {
        if (next != 255u || !((me >> (16u + k)) & 1u)) continue; /* an allowed move stays inside the raster */
        const size_t n = (size_t)(y + plan_dy(k)) * width + (size_t)(x + plan_dx(k));
        const uint32_t cn = cost[n];
        if (cn != PLAN_INF && cn + plan_edge(k, me & 0xffffu, wm[n] & 0xffffu) == mine) next = k;
      }
    }
    const uint32_t head = field[c].y & 0x00ffffffu; /* clear2 and the two bits kpl_clear_col wrote for this cell */
    const bool reached = mine != PLAN_INF;
    field[c] = make_uint2(mine, head | (reached ? 4u << 16 : 0u) | next << 24);
    if (head & (2u << 16)) atomicAdd(&block_counts[0], 1u);
    if (reached) atomicAdd(&block_counts[1], 1u), atomicMax(&block_counts[2], mine);
  }
  __syncthreads();
  if (threadIdx.x < 2 && block_counts[threadIdx.x]) atomicAdd(&counters[PLAN_TRAVERSABLE + threadIdx.x], block_counts[threadIdx.x]);
  if (threadIdx.x == 2 && block_counts[2]) atomicMax(&counters[PLAN_MAX_COST], block_counts[2]);
}

__global__ void __launch_bounds__(PLAN_THREADS)
    kpl_walk(uint32_t width, uint32_t height, const uint2* __restrict__ field, const uint32_t* __restrict__ starts,
             uint32_t n_starts, uint32_t capacity, uint4* __restrict__ results, uint32_t* __restrict__ cells) {
  const uint32_t s = blockIdx.x * (PLAN_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (s >= n_starts) return;
  const uint32_t n_cells = width * height;
  uint32_t* row = cells + (size_t)s * capacity;
  uint32_t c = starts[s], length = 0, status = SUMA_PATH_START_OUTSIDE, cost = PLAN_INF;
  if (c < n_cells) {
    uint2 fc = field[c];
    cost = fc.x;
    status = SUMA_PATH_UNREACHED;
    if ((fc.y >> 24) != 255u) {
      int x = (int)(c % width), y = (int)(c / width);
      uint32_t kept = c, base = 0; /* lane i keeps cell base + i of the path */
      length = 1;
      status = SUMA_PATH_BAD_FIELD;
      for (uint32_t step = 0; step < n_cells; ++step) { /* the same on every lane of the wave */
        const uint32_t k = fc.y >> 24;
        if (k == 8u) {
          status = SUMA_PATH_OK;
          break;
        }
        if (k > 7u) break;
        x += plan_dx(k), y += plan_dy(k);
        if (x < 0 || y < 0 || x >= (int)width || y >= (int)height) break;
        const uint32_t n = (uint32_t)y * width + (uint32_t)x;
        const uint2 fn = field[n];
        if (!(fn.x < fc.x)) break;
        c = n, fc = fn;
        if (length - base == 64u) {
          if (base + lane < capacity) row[base + lane] = kept;
          base += 64u;
        }
        if (lane == length - base) kept = c;
        ++length;
      }
      if (base + lane < length && base + lane < capacity) row[base + lane] = kept;
      if (status == SUMA_PATH_OK && length > capacity) status = SUMA_PATH_TRUNCATED;
    }
  }
  if (lane == 0) results[s] = make_uint4(length, status, cost, 0u);
}

size_t plan_scratch_bytes(uint32_t width, uint32_t height) {
  const size_t n = (((size_t)width * height + 15) / 16) * 16;
  const size_t tiles = (size_t)((width + PLAN_TILE - 1) / PLAN_TILE) * ((height + PLAN_TILE - 1) / PLAN_TILE);
  return n * PLAN_SCRATCH_PER_CELL + 2 * ((tiles + 15) / 16) * 16;
}

namespace {
/* the arrays of c->plan_scratch for a raster */
struct PlanScratch {
  uint2* rec;
  uint32_t *wm, *cost[2];
  uint8_t *drow, *tile[2];
  uint32_t tiles_x, tiles_y;
  PlanScratch(suma_ctx* c, uint32_t width, uint32_t height) {
    const size_t n = (((size_t)width * height + 15) / 16) * 16;
    tiles_x = (width + PLAN_TILE - 1) / PLAN_TILE, tiles_y = (height + PLAN_TILE - 1) / PLAN_TILE;
    char* p = c->plan_scratch;
    rec = reinterpret_cast<uint2*>(p), p += 8 * n;
    wm = reinterpret_cast<uint32_t*>(p), p += 4 * n;
    cost[0] = reinterpret_cast<uint32_t*>(p), p += 4 * n;
    cost[1] = reinterpret_cast<uint32_t*>(p), p += 4 * n;
    drow = reinterpret_cast<uint8_t*>(p), p += n;
    tile[0] = reinterpret_cast<uint8_t*>(p), p += (((size_t)tiles_x * tiles_y + 15) / 16) * 16;
    tile[1] = reinterpret_cast<uint8_t*>(p);
  }
};
}  // namespace

hipError_t launch_plan_prepare(suma_ctx* c, const suma_grid_params& gp, const suma_plan_params& pp, const suma_grid_cell* d_cells,
                               uint32_t n_goals, suma_plan_cell* d_field) {
  hipStream_t st = c->stream;
  const PlanScratch ps(c, gp.width, gp.height);
  uint32_t* counters = c->plan_counters;
  PlanArgs a;
  a.width = gp.width, a.height = gp.height, a.n_cells = gp.width * gp.height;
  a.cell_size = gp.cell_size, a.robot_radius = pp.robot_radius, a.max_step = pp.max_step, a.max_rough = pp.max_rough;
  a.unknown_blocked = pp.unknown_blocked, a.R = pp.max_clear_cells, a.soft_cells = pp.soft_cells, a.soft_weight = pp.soft_weight;
  PlanLabelCost lc;
  memcpy(lc.w, pp.label_cost, sizeof(lc.w));
  const unsigned cell_blocks = (a.n_cells + PLAN_THREADS - 1) / PLAN_THREADS;
  const uint32_t tiles_x = (gp.width + PLAN_ROW_W - 1) / PLAN_ROW_W;

  hipError_t e = hipMemsetAsync(counters, 0, PLAN_COUNTERS * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  {
    ProfScope p(c, "plan_classify", 56.0 * a.n_cells);
    kpl_classify<<<cell_blocks, PLAN_THREADS, 0, st>>>(a, lc, reinterpret_cast<const float4*>(d_cells), ps.rec, counters);
  }
  {
    ProfScope p(c, "plan_clearance", 30.0 * a.n_cells);
    kpl_clear_row<<<tiles_x * ((gp.height + PLAN_ROW_H - 1) / PLAN_ROW_H), PLAN_THREADS, 0, st>>>(a, tiles_x, ps.rec, ps.drow);
    kpl_clear_col<<<tiles_x * ((gp.height + PLAN_COL_H - 1) / PLAN_COL_H), PLAN_THREADS, 0, st>>>(
        a, tiles_x, ps.drow, ps.rec, reinterpret_cast<uint2*>(d_field));
    kpl_edges<<<cell_blocks, PLAN_THREADS, 0, st>>>(a, ps.rec, ps.wm);
  }
  if ((e = hipMemsetAsync(ps.cost[0], 0xff, (size_t)a.n_cells * sizeof(uint32_t), st)) != hipSuccess) return e;
  kpl_seed<<<(n_goals + PLAN_THREADS - 1) / PLAN_THREADS, PLAN_THREADS, 0, st>>>(n_goals, c->plan_io, ps.rec, ps.cost[0], counters);
  return hipGetLastError();
}

int launch_plan_relax(suma_ctx* c, const suma_grid_params& gp, uint32_t* n_rounds) {
  hipStream_t st = c->stream;
  const PlanScratch ps(c, gp.width, gp.height);
  uint32_t* flags = c->plan_counters + PLAN_ROUND_FLAGS;
  const uint64_t bound = (uint64_t)gp.width * gp.height;
  const uint32_t n_tiles = ps.tiles_x * ps.tiles_y;
  uint64_t rounds = 0;
  static_assert(PLAN_ROUND_BATCH % 2 == 0 && PLAN_ROUND_FLAGS + PLAN_ROUND_BATCH <= PLAN_COUNTERS, "the batch");
  ProfScope p(c, "plan_relax", 0.0);
  for (;;) {
    /* a batch starts reading cost[0]: an even number of rounds lies behind it */
    if (rounds) HIP_TRY(c, hipMemsetAsync(flags, 0, PLAN_ROUND_BATCH * sizeof(uint32_t), st));
    for (uint32_t i = 0; i < PLAN_ROUND_BATCH; ++i)
      kpl_relax<<<n_tiles, PLAN_THREADS, 0, st>>>(gp.width, gp.height, ps.tiles_x, ps.tiles_y, rounds == 0 && i == 0, ps.wm,
                                                  ps.cost[i & 1u], ps.cost[(i & 1u) ^ 1u], ps.tile[(i & 1u) ^ 1u], ps.tile[i & 1u],
                                                  i ? flags + i - 1 : nullptr, flags + i);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(c->plan_counters_h + PLAN_ROUND_FLAGS, flags, PLAN_ROUND_BATCH * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const uint32_t* h = c->plan_counters_h + PLAN_ROUND_FLAGS;
    for (uint32_t i = 0; i < PLAN_ROUND_BATCH; ++i) {
      ++rounds;
      if (!h[i]) { /* this round changed nothing: both cost arrays hold the field */
        *n_rounds = (uint32_t)rounds;
        return SUMA_OK;
      }
    }
    if (rounds >= bound + PLAN_ROUND_BATCH)
      return fail(c, SUMA_ERR_CAPACITY, "suma_grid_plan_field: the relaxation did not settle in width * height rounds");
  }
}

hipError_t launch_plan_next(suma_ctx* c, const suma_grid_params& gp, suma_plan_cell* d_field) {
  const PlanScratch ps(c, gp.width, gp.height);
  const uint32_t n_cells = gp.width * gp.height;
  ProfScope p(c, "plan_next", 24.0 * n_cells);
  kpl_next<<<(n_cells + PLAN_THREADS - 1) / PLAN_THREADS, PLAN_THREADS, 0, c->stream>>>(
      gp.width, gp.height, n_cells, ps.wm, ps.cost[0], reinterpret_cast<uint2*>(d_field), c->plan_counters);
  return hipGetLastError();
}

hipError_t launch_plan_walk(suma_ctx* c, const suma_grid_params& gp, const suma_plan_cell* d_field, uint32_t n_starts,
                            uint32_t capacity) {
  hipStream_t st = c->stream;
  uint32_t* io = c->plan_io;
  hipError_t e = hipMemsetAsync(io + 5 * (size_t)n_starts, 0xff, (size_t)n_starts * capacity * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  ProfScope p(c, "plan_walk", 0.0);
  const uint32_t per_block = PLAN_THREADS / 64;
  kpl_walk<<<(n_starts + per_block - 1) / per_block, PLAN_THREADS, 0, st>>>(
      gp.width, gp.height, reinterpret_cast<const uint2*>(d_field), io + 4 * (size_t)n_starts, n_starts, capacity,
      reinterpret_cast<uint4*>(io), io + 5 * (size_t)n_starts);
  return hipGetLastError();
}
