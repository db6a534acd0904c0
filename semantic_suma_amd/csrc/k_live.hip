/*
 * k_live.hip -- the live obstacle layer: what a localiser's scans see standing on the ground that yesterday's map does not
 * contain, kept per cell of a static traversability grid (k_grid.hip) and written into a copy of its cells, so that the
 * planner (k_plan.hip) goes round a car parked there this morning.  The layer takes the outputs of k_novel.hip (the flag
 * image) and, where objects are on, of k_objects.hip (the id image); the scan path, the candidates, the objects, the grid
 * and the planner keep their results bit for bit.  Nothing in the reference does this.  The host entries are in
 * suma_localize.hip.
 *
 * Kernels (VGPRs by tools/isa_stats.py k_live.hip; none spills, none uses scratch, LDS in bytes):
 *   klv_ground   4 VGPRs, LDS 0     lane per cell: the static cell's ground_z into the 4-byte array the rays read.
 *   klv_hit      11 VGPRs, LDS 28   lane per texel: the hit rule; one 64-bit atomicMax with return per hit; the lane that
 *                finds an older stamp keeps the cell's hits; counts per block in LDS, one global add per count and block.
 *   klv_carve    21 VGPRs, LDS 8    lane per texel: the ray walk (91 VALU and three IEEE divisions a sample: t_k / r and
 *                the two of the cell rule); one atomicMax per cleared sample.
 *   klv_compose  25 VGPRs, LDS 16   lane per cell: the composed cell, the mask byte, the stats.
 *
 * SPECIFICATION (fp32, every operation as written, no contraction: -ffp-contract=off; the helpers of dev_math.h; `/`
 * correctly rounded; a NaN passes no comparison; tests/live_shim.c restates it sequentially and the library must equal it
 * byte for byte).
 *
 * Parameters (suma_live_params): hold_scans (10; 1 .. 65 535), min_hits (2; 1 .. 65 535), carve_range (20 m; finite, >= 0;
 * 0 = no carving), carve_margin (0.5 m; finite, >= 0).  Of the static grid's suma_grid_params the layer reads cell_size,
 * origin_x, origin_y, width, height, step_height and clearance.
 * STATE per cell c (suma_live_cell, 16 bytes): hit = stamp << 32 | ordered(top_z) (uint64; ordered = k_objects.hip's
 * ob_ordered: a float as an integer of the same order, -0 below +0), clear (a uint32 stamp), hits (uint32).  The stamp of
 * an update is s = scan_id + 1; 0 means never.  An update needs s > the last update's stamp (s = 0, from scan_id =
 * 2^32 - 1, never is).  g(c) = the static cell's ground_z, its own or a filled one; a NaN g is "no ground".
 * One update takes a data-sized frame (V; W x H texels), a flag image (one byte a texel), with objects on that
 * segmentation's id image, the fp32 pose P (P = T rounded to fp32) and s.  dv is the texel's vertex value, m = xyz(dv),
 * w = m4_point(P, m).
 *   1. MEMBER.  k_objects.hip's step 1: flag[t] != 0, dv.w > 0.5f, the components of m and of w finite.  With objects on,
 *      also id[t] != 0xffffffff: a texel of a component below min_texels, or of an object beyond max_objects, is none.
 *   2. CELL of a position (x, y): fx = floorf((x - origin_x) / cell_size), fy likewise; inside the raster iff fx >= 0 &&
 *      fx < width && fy >= 0 && fy < height; c = (uint)fy * width + (uint)fx  (k_grid.hip's rule).
 *   3. HIT.  A member outside the raster: n_outside.  A member whose cell has no ground: n_no_ground.  Else h = w.z - g:
 *      h <= step_height: n_low; else h > clearance: n_high; else a hit (n_hit_texels):
 *      hit[c] = max(hit[c], s << 32 | ordered(w.z)).
 *      Per cell and update one hit finds a stamp below s in the value it replaces -- the first to arrive.  With old = that
 *      stamp and clear = clear[c] (no hit changes it): old != 0 && old > clear && s - old <= hold_scans:
 *      hits[c] = min(hits[c] + 1, 65 535); else hits[c] = 1.  n_hit_cells counts these cells.
 *      After the update the cell holds (s, the greatest w.z of its hits in this scan, hits) whatever the order.
 *   4. CARVE, behind all hits, only with carve_range != 0.  Every texel with a return casts a ray, flagged or not (n_rays):
 *      dv.w > 0.5f, m and w finite.  o = P's translation, u = sub3(w, o), r = len3(u).  Samples k = 1, 2, ... at
 *      t_k = (float)k * (0.5f * cell_size) while t_k < r - carve_margin && t_k <= carve_range && k <= 4096; the sample is
 *      p = o + u * (t_k / r), component by component (a product, then a sum).  A sample whose cell -- or whose "outside"
 *      -- is that of the sample before it is skipped.  At a cell c inside the raster, with H = the stamp of hit[c] and
 *      top_z its float: 0 < H && H < s && p.z <= top_z && p.z - g(c) > step_height:  clear[c] = max(clear[c], s).
 *      n_cleared counts the cells whose clear was below s before.  The rays read hit, which the carve does not write:
 *      a cell hit in this scan has H = s and is never cleared by it; a ray above the top of what was seen clears
 *      nothing; neither does a ray at or below step_height over the ground, or over a cell without ground.
 *   5. LIVE, with now = the last update's stamp: H != 0 && H > clear && now - H < hold_scans.  Such a cell is live with
 *      hits >= min_hits and pending with fewer.  Of the other cells with H != 0, one with H <= clear is carved, the rest
 *      are expired (suma_live_stats counts the four).
 *   6. COMPOSE.  The static cell; where live: state = SUMA_GRID_OBSTACLE, obstacle_z = top_z where it was NaN or below
 *      top_z (-0 below +0), every other field as it was.  Mask: 1 live, 2 pending, else 0.
 * Open points, fixed here: r = 0 or a NaN limit takes no sample.  An infinite u (a return further than fp32 spans) gives
 * NaN samples, which lie outside.  A sample that leaves the raster and comes back to the same cell is evaluated again;
 * max and the count by "was below s" make that harmless.  step_height and clearance are the static grid's; an infinite g
 * gives h = -+infinity, low or high.  The counts of an update that hits nothing are zero but n_texels, n_members and the
 * classes of step 3.
 *
 * Decomposition.  Three launches, none waits for another block.  klv_hit: the 64-bit atomicMax orders (stamp, height)
 * pairs, and the one lane per cell that is handed a value with an older stamp owns hits[c] for this launch: a plain load
 * and store, no second atomic.  klv_carve is a launch of its own because it must see every hit of the scan (H = s) before
 * it may clear: it reads hit and ground, written by earlier launches, and writes clear only by atomicMax.  Its early exit:
 * word LIVE_ANY_HIT is set by the first hit since the state was zeroed; while it is 0 no cell has H != 0, no sample can
 * clear, and the lanes only count their rays.  klv_compose reads everything and writes the caller's buffers.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"
#include "draw_vertex.h"

#define LV_THREADS 256
#define LV_NONE 0xffffffffu
#define LV_MAX_SAMPLES 4096u
enum { LV_MEMBERS = 0, LV_OUTSIDE, LV_NO_GROUND, LV_LOW, LV_HIGH, LV_HIT, LV_HIT_CELLS, LV_HIT_WORDS };

struct LiveArgs {
  const float4* V;
  const uint8_t* flag;
  const uint32_t* ids; /* NULL: objects off */
  m4 P;
  uint32_t n_texels, s;
  float cell_size, origin_x, origin_y;
  uint32_t width, height;
  float step_height, clearance;
  uint32_t hold_scans, min_hits;
  float carve_range, carve_margin;
  const float* ground;
  suma_live_cell* state;
  uint32_t* words;
};

/* k_objects.hip's order: a float as an integer of the same order, -0 below +0 */
SDEV uint32_t lv_ordered(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SDEV float lv_unordered(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

/* step 2: the cell of (x, y), or LV_NONE */
SDEV uint32_t lv_cell(const LiveArgs& a, float x, float y) {
  const float fx = sdm_floor((x - a.origin_x) / a.cell_size), fy = sdm_floor((y - a.origin_y) / a.cell_size);
  if (!(fx >= 0.0f && fx < (float)a.width && fy >= 0.0f && fy < (float)a.height)) return LV_NONE;
  return (uint32_t)fy * a.width + (uint32_t)fx; /* < width * height <= 2^26 */
}

/* dv.w > 0.5f, m and w finite: a return */
SDEV bool lv_return(const LiveArgs& a, float4 dv, v3* w) {
  const v3 m = xyz(dv);
  *w = m4_point(a.P.m, m);
  const bool fin = finite_f(m.x) && finite_f(m.y) && finite_f(m.z) && finite_f(w->x) && finite_f(w->y) && finite_f(w->z);
  return (dv.w > 0.5f) & fin;
}

__global__ void __launch_bounds__(LV_THREADS) klv_ground(const float4* __restrict__ cells, float* __restrict__ ground, uint32_t n) {
  const uint32_t c = blockIdx.x * LV_THREADS + threadIdx.x;
  if (c < n) ground[c] = cells[3 * (size_t)c].x;
}

__global__ void __launch_bounds__(LV_THREADS) klv_hit(LiveArgs a) {
  __shared__ uint32_t tot[LV_HIT_WORDS];
  if (threadIdx.x < LV_HIT_WORDS) tot[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t t = blockIdx.x * LV_THREADS + threadIdx.x;
  uint32_t kind = LV_HIT_WORDS; /* none */
  bool member = false, first = false;
  if (t < a.n_texels) {
    v3 w;
    member = lv_return(a, a.V[t], &w) && a.flag[t] != 0;
    if (member && a.ids) member = a.ids[t] != LV_NONE;
    if (member) {
      const uint32_t c = lv_cell(a, w.x, w.y);
      if (c == LV_NONE) {
        kind = LV_OUTSIDE;
      } else {
        const float g = a.ground[c];
        const float h = w.z - g;
        if (g != g) kind = LV_NO_GROUND;
        else if (h <= a.step_height) kind = LV_LOW;
        else if (h > a.clearance) kind = LV_HIGH;
        else {
          kind = LV_HIT;
          suma_live_cell* st = a.state + c;
          const unsigned long long v = ((unsigned long long)a.s << 32) | (unsigned long long)lv_ordered(w.z);
          const unsigned long long old = atomicMax(reinterpret_cast<unsigned long long*>(&st->hit), v);
          const uint32_t os = (uint32_t)(old >> 32);
          if (os < a.s) { /* the first hit of this update in c: this lane alone touches hits[c] in this launch */
            const uint32_t hits = st->hits, clear = st->clear;
            const bool run = os != 0u && os > clear && a.s - os <= a.hold_scans;
            st->hits = run ? (hits + 1u < 65535u ? hits + 1u : 65535u) : 1u;
            first = true;
          }
        }
      }
    }
  }
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long bm = __ballot(member), bf = __ballot(first);
  unsigned long long bk[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) bk[k] = __ballot(kind == LV_OUTSIDE + k);
  if (lane == 0) {
    if (bm) atomicAdd(&tot[LV_MEMBERS], (uint32_t)__popcll(bm));
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k)
      if (bk[k]) atomicAdd(&tot[LV_OUTSIDE + k], (uint32_t)__popcll(bk[k]));
    if (bf) atomicAdd(&tot[LV_HIT_CELLS], (uint32_t)__popcll(bf));
  }
  __syncthreads();
  if (threadIdx.x < LV_HIT_WORDS && tot[threadIdx.x]) atomicAdd(&a.words[1 + threadIdx.x], tot[threadIdx.x]);
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) atomicAdd(&a.words[0], a.n_texels);
    if (tot[LV_HIT]) atomicMax(&a.words[LIVE_ANY_HIT], 1u);
  }
}

__global__ void __launch_bounds__(LV_THREADS) klv_carve(LiveArgs a) {
  __shared__ uint32_t tot[2];
  if (threadIdx.x < 2) tot[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t t = blockIdx.x * LV_THREADS + threadIdx.x;
  const bool armed = a.words[LIVE_ANY_HIT] != 0u; /* written by earlier launches only */
  bool ray = false;
  uint32_t cleared = 0u;
  if (t < a.n_texels) {
    v3 w;
    ray = lv_return(a, a.V[t], &w);
    if (ray && armed) {
      const v3 o = mk3(a.P.m[12], a.P.m[13], a.P.m[14]);
      const v3 u = sub3(w, o);
      const float r = len3(u), step = 0.5f * a.cell_size, lim = r - a.carve_margin;
      uint32_t prev = LV_NONE;
      for (uint32_t k = 1; k <= LV_MAX_SAMPLES; ++k) {
        const float tk = (float)k * step;
        if (!(tk < lim && tk <= a.carve_range)) break;
        const float q = tk / r;
        const float px = o.x + u.x * q, py = o.y + u.y * q, pz = o.z + u.z * q;
        const uint32_t c = lv_cell(a, px, py);
        if (c == prev) continue;
        prev = c;
        if (c == LV_NONE) continue;
        const unsigned long long hit = a.state[c].hit; /* the hits are an earlier launch */
        const uint32_t H = (uint32_t)(hit >> 32);
        if (!(H > 0u && H < a.s)) continue;
        if (!(pz <= lv_unordered((uint32_t)hit))) continue;
        if (!(pz - a.ground[c] > a.step_height)) continue;
        if (atomicMax(&a.state[c].clear, a.s) < a.s) ++cleared;
      }
    }
  }
  const unsigned long long br = __ballot(ray);
  if ((threadIdx.x & 63u) == 0 && br) atomicAdd(&tot[0], (uint32_t)__popcll(br));
  if (cleared) atomicAdd(&tot[1], cleared);
  __syncthreads();
  if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&a.words[8 + threadIdx.x], tot[threadIdx.x]);
}

/* s = now */
__global__ void __launch_bounds__(LV_THREADS)
    klv_compose(LiveArgs a, const float4* __restrict__ cells, uint32_t n_cells, float4* __restrict__ out, uint8_t* __restrict__ mask) {
  __shared__ uint32_t tot[LIVE_STAT_WORDS];
  if (threadIdx.x < LIVE_STAT_WORDS) tot[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t c = blockIdx.x * LV_THREADS + threadIdx.x;
  uint32_t cls = LIVE_STAT_WORDS; /* 0 live, 1 pending, 2 expired, 3 carved */
  if (c < n_cells) {
    const suma_live_cell st = a.state[c];
    const uint32_t H = (uint32_t)(st.hit >> 32);
    float4 f0 = cells[3 * (size_t)c], f1 = cells[3 * (size_t)c + 1], f2 = cells[3 * (size_t)c + 2];
    if (H != 0u) {
      if (!(H > st.clear)) cls = 3u;
      else if (!(a.s - H < a.hold_scans)) cls = 2u;
      else cls = st.hits >= a.min_hits ? 0u : 1u;
    }
    if (cls == 0u) {
      const uint32_t top = (uint32_t)st.hit;
      if (f1.x != f1.x || lv_ordered(f1.x) < top) f1.x = lv_unordered(top);
      f2.w = __uint_as_float((__float_as_uint(f2.w) & 0xffffff00u) | (uint32_t)SUMA_GRID_OBSTACLE);
    }
    out[3 * (size_t)c] = f0, out[3 * (size_t)c + 1] = f1, out[3 * (size_t)c + 2] = f2;
    if (mask) mask[c] = cls == 0u ? 1 : (cls == 1u ? 2 : 0);
  }
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t k = 0; k < LIVE_STAT_WORDS; ++k) {
    const unsigned long long b = __ballot(cls == k);
    if (lane == 0 && b) atomicAdd(&tot[k], (uint32_t)__popcll(b));
  }
  __syncthreads();
  if (threadIdx.x < LIVE_STAT_WORDS && tot[threadIdx.x]) atomicAdd(&a.words[LIVE_STATS + threadIdx.x], tot[threadIdx.x]);
}

/* ---- host side ---- */
static void live_args(const Live& lv, LiveArgs* a) {
  memset(a, 0, sizeof(*a));
  a->cell_size = lv.gp.cell_size, a->origin_x = lv.gp.origin_x, a->origin_y = lv.gp.origin_y;
  a->width = lv.gp.width, a->height = lv.gp.height;
  a->step_height = lv.gp.step_height, a->clearance = lv.gp.clearance;
  a->hold_scans = lv.lp.hold_scans, a->min_hits = lv.lp.min_hits;
  a->carve_range = lv.lp.carve_range, a->carve_margin = lv.lp.carve_margin;
  a->ground = lv.ground;
  a->state = lv.state;
  a->words = lv.words;
}

int live_alloc(suma_ctx* c, Live& lv, const suma_grid_params& gp, const suma_grid_cell* d_cells) {
  const size_t n = (size_t)gp.width * gp.height;
  Live nw;
  hipError_t e = nw.cells.alloc(3 * n);
  if (e == hipSuccess) e = nw.ground.alloc(n);
  if (e == hipSuccess) e = nw.state.alloc(n);
  if (e == hipSuccess) e = nw.words.alloc(LIVE_WORDS);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SUMA_ERR_NOMEM, "suma_localizer_enable_live_grid: no device memory for " + std::to_string(n) + " cells");
  }
  nw.gp = gp;
  nw.n_cells = (uint32_t)n;
  HIP_TRY(c, hipMemcpyAsync(nw.cells, d_cells, n * sizeof(suma_grid_cell), hipMemcpyDeviceToDevice, c->stream));
  klv_ground<<<(unsigned)((n + LV_THREADS - 1) / LV_THREADS), LV_THREADS, 0, c->stream>>>(nw.cells, nw.ground, (uint32_t)n);
  HIP_TRY(c, hipGetLastError());
  int r = live_clear(c, nw);
  if (r) return r;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  lv = std::move(nw);
  return SUMA_OK;
}

int live_clear(suma_ctx* c, Live& lv) {
  HIP_TRY(c, hipMemsetAsync(lv.state, 0, (size_t)lv.n_cells * sizeof(suma_live_cell), c->stream));
  HIP_TRY(c, hipMemsetAsync(lv.words, 0, LIVE_WORDS * sizeof(uint32_t), c->stream));
  lv.last_stamp = 0;
  lv.updated = 0;
  return SUMA_OK;
}

int live_update(suma_ctx* c, Live& lv, const suma_frame* f, const uint8_t* d_flags, const uint32_t* d_ids, const double T[16],
                uint32_t s) {
  LiveArgs a;
  live_args(lv, &a);
  a.V = f->map[SUMA_MAP_VERTEX];
  a.flag = d_flags;
  a.ids = d_ids;
  mat4_cast_f(T, a.P.m);
  a.n_texels = (uint32_t)f->width * (uint32_t)f->height;
  a.s = s;
  const uint32_t blocks = (a.n_texels + LV_THREADS - 1) / LV_THREADS;
  HIP_TRY(c, hipMemsetAsync(lv.words, 0, LIVE_COUNT_WORDS * sizeof(uint32_t), c->stream));
  {
    ProfScope ps(c, "live_hit", 21.0 * a.n_texels);
    klv_hit<<<blocks, LV_THREADS, 0, c->stream>>>(a);
  }
  if (lv.lp.carve_range != 0.0f) {
    ProfScope ps(c, "live_carve", 16.0 * a.n_texels);
    klv_carve<<<blocks, LV_THREADS, 0, c->stream>>>(a);
  }
  HIP_TRY(c, hipGetLastError());
  lv.last_stamp = s;
  lv.updated = 1;
  return SUMA_OK;
}

int live_compose(suma_ctx* c, Live& lv, suma_grid_cell* d_out, uint8_t* d_mask) {
  LiveArgs a;
  live_args(lv, &a);
  a.s = lv.last_stamp;
  HIP_TRY(c, hipMemsetAsync(lv.words.p + LIVE_STATS, 0, LIVE_STAT_WORDS * sizeof(uint32_t), c->stream));
  {
    ProfScope ps(c, "live_compose", 113.0 * lv.n_cells);
    klv_compose<<<(lv.n_cells + LV_THREADS - 1) / LV_THREADS, LV_THREADS, 0, c->stream>>>(
        a, lv.cells, lv.n_cells, reinterpret_cast<float4*>(d_out), d_mask);
  }
  HIP_TRY(c, hipGetLastError());
  return SUMA_OK;
}
