/*
 * suma_grid.hip -- the traversability grid's entries (include/suma_hip.h, suma_grid_params_default, suma_world_grid_fit,
 * suma_world_grid).  Host code: the parameter checks, the scratch, the one blocking read of the counters.  k_grid.hip
 * states the specification and holds the kernels.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"

#define GRID_MAX_CELLS (1u << 26)

extern "C" void suma_grid_params_default(suma_grid_params* gp) {
  if (!gp) return;
  std::memset(gp, 0, sizeof(*gp));
  gp->cell_size = 0.2f;
  for (int l : {40, 44, 48, 49, 60, 72}) gp->ground_label[l] = 1;
  gp->min_normal_z = 0.7f;
  gp->step_height = 0.2f;
  gp->clearance = 2.0f;
  gp->fill_radius = 2;
}

static int grid_check_records(suma_ctx* c, const char* who, const suma_world_surfel* d_records, uint32_t n) {
  if (n && !d_records) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": NULL records with n > 0");
  if ((uintptr_t)d_records & 15u) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": records not 16-byte aligned");
  if (n >= (1u << 31)) return fail(c, SUMA_ERR_INVALID, std::string(who) + ": n = " + std::to_string(n) + " (must be < 2^31)");
  return SUMA_OK;
}

static int grid_check_cell_size(suma_ctx* c, const char* who, float cell_size) {
  if (!(std::isfinite(cell_size) && cell_size > 0.0f))
    return fail(c, SUMA_ERR_INVALID, std::string(who) + ": cell_size = " + std::to_string(cell_size) + " (must be finite and > 0)");
  return SUMA_OK;
}

/* the counters on the host, behind everything enqueued so far: the one wait of both entries */
static int grid_read_counters(suma_ctx* c) {
  HIP_TRY(c, hipMemcpyAsync(c->grid_counters_h, c->grid_counters, GRID_COUNTERS * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SUMA_OK;
}

extern "C" int suma_world_grid_fit(suma_ctx* c, const suma_world_surfel* d_records, uint32_t n, uint32_t margin_cells,
                                   suma_grid_params* gp) {
  if (!c) return SUMA_ERR_INVALID;
  const char* who = "suma_world_grid_fit";
  if (!gp) return fail(c, SUMA_ERR_INVALID, "suma_world_grid_fit: NULL parameters");
  int r = grid_check_records(c, who, d_records, n);
  if (r || (r = grid_check_cell_size(c, who, gp->cell_size))) return r;
  if (margin_cells > (1u << 20)) return fail(c, SUMA_ERR_INVALID, "suma_world_grid_fit: margin_cells above 2^20");
  if (!n) return fail(c, SUMA_ERR_INVALID, "suma_world_grid_fit: no finite record");
  if ((r = grow(c, c->grid_counters, GRID_COUNTERS, {c->stream})) < 0) return r;
  if ((r = grow(c, c->grid_counters_h, GRID_COUNTERS, {c->stream})) < 0) return r;
  HIP_TRY(c, launch_grid_fit(c, d_records, n));
  if ((r = grid_read_counters(c))) return r;
  const uint32_t* h = c->grid_counters_h;
  if (h[GRID_FIT_MIN_X] == 0xffffffffu) return fail(c, SUMA_ERR_INVALID, "suma_world_grid_fit: no finite record");
  const float cs = gp->cell_size, m = (float)margin_cells;
  const float lo_x = floorf(grid_ordered_float(h[GRID_FIT_MIN_X]) / cs), hi_x = floorf(grid_ordered_float(h[GRID_FIT_MAX_X]) / cs);
  const float lo_y = floorf(grid_ordered_float(h[GRID_FIT_MIN_Y]) / cs), hi_y = floorf(grid_ordered_float(h[GRID_FIT_MAX_Y]) / cs);
  const float span_x = hi_x - lo_x, span_y = hi_y - lo_y;
  /* the spans are whole numbers or infinite; beyond 2^26 no cast */
  const double w = (double)span_x + 1.0 + 2.0 * margin_cells, hgt = (double)span_y + 1.0 + 2.0 * margin_cells;
  if (!(w <= (double)GRID_MAX_CELLS && hgt <= (double)GRID_MAX_CELLS && w * hgt <= (double)GRID_MAX_CELLS))
    return fail(c, SUMA_ERR_CAPACITY, "suma_world_grid_fit: the records span " + std::to_string(w) + " x " + std::to_string(hgt) +
                                      " cells (width * height must be <= 2^26): choose a larger cell_size");
  const float ox = (lo_x - m) * cs + 0.0f, oy = (lo_y - m) * cs + 0.0f; /* + 0: never -0 */
  if (!(std::isfinite(ox) && std::isfinite(oy))) return fail(c, SUMA_ERR_CAPACITY, "suma_world_grid_fit: the origin is not finite");
  gp->origin_x = ox, gp->origin_y = oy;
  gp->width = (uint32_t)span_x + 1u + 2u * margin_cells;
  gp->height = (uint32_t)span_y + 1u + 2u * margin_cells;
  return SUMA_OK;
}

/* the ranges stated at suma_grid_params, cell_size included */
int grid_check_params(suma_ctx* c, const std::string& who, const suma_grid_params& gp) {
  int r = grid_check_cell_size(c, who.c_str(), gp.cell_size);
  if (r) return r;
  if (!(std::isfinite(gp.origin_x) && std::isfinite(gp.origin_y)))
    return fail(c, SUMA_ERR_INVALID, who + ": origin is not finite");
  if (gp.width < 1 || gp.height < 1 || (uint64_t)gp.width * gp.height > GRID_MAX_CELLS)
    return fail(c, SUMA_ERR_INVALID, who + ": width x height = " + std::to_string(gp.width) + " x " +
                                     std::to_string(gp.height) + " (each >= 1, width * height <= 2^26)");
  if (std::isnan(gp.min_normal_z)) return fail(c, SUMA_ERR_INVALID, who + ": min_normal_z is NaN");
  if (!std::isfinite(gp.step_height)) return fail(c, SUMA_ERR_INVALID, who + ": step_height is not finite");
  if (!(std::isfinite(gp.clearance) && gp.clearance > gp.step_height))
    return fail(c, SUMA_ERR_INVALID, who + ": clearance = " + std::to_string(gp.clearance) +
                                     " (must be finite and > step_height)");
  if (gp.fill_radius > 8) return fail(c, SUMA_ERR_INVALID, who + ": fill_radius = " + std::to_string(gp.fill_radius) +
                                                            " (0 .. 8)");
  return SUMA_OK;
}

extern "C" int suma_world_grid(suma_ctx* c, const suma_grid_params* gp, const suma_world_surfel* d_records, uint32_t n,
                               suma_grid_cell* d_cells, suma_grid_stats* stats) {
  if (!c) return SUMA_ERR_INVALID;
  const char* who = "suma_world_grid";
  if (!gp) return fail(c, SUMA_ERR_INVALID, "suma_world_grid: NULL parameters");
  if (!stats) return fail(c, SUMA_ERR_INVALID, "suma_world_grid: NULL stats");
  if (!d_cells) return fail(c, SUMA_ERR_INVALID, "suma_world_grid: NULL cells");
  if ((uintptr_t)d_cells & 15u) return fail(c, SUMA_ERR_INVALID, "suma_world_grid: cells not 16-byte aligned");
  int r = grid_check_records(c, who, d_records, n);
  if (r || (r = grid_check_params(c, who, *gp))) return r;

  const size_t n_cells = (size_t)gp->width * gp->height;
  size_t tmp = 0;
  HIP_TRY(c, group_tmp_bytes(n, true, c->stream, &tmp));
  if ((r = grow(c, c->grid_counters, GRID_COUNTERS, {c->stream})) < 0) return r;
  if ((r = grow(c, c->grid_counters_h, GRID_COUNTERS, {c->stream})) < 0) return r;
  if ((r = grow(c, c->grid_runs, n_cells, {c->stream})) < 0) return r;
  if ((r = grow(c, c->world_scratch, (size_t)n * GRID_SCRATCH_PER_RECORD, {c->stream})) < 0) return r;
  if ((r = grow(c, c->world_tmp, tmp, {c->stream})) < 0) return r;
  HIP_TRY(c, launch_grid(c, *gp, d_records, n, d_cells));
  if ((r = grid_read_counters(c))) return r;
  const uint32_t* h = c->grid_counters_h;
  std::memset(stats, 0, sizeof(*stats));
  stats->n_records = n;
  stats->n_dropped = h[GRID_DROPPED];
  stats->n_outside = h[GRID_OUTSIDE];
  stats->n_binned = n - h[GRID_DROPPED] - h[GRID_OUTSIDE];
  stats->n_occupied = h[GRID_OCCUPIED];
  stats->n_free = h[GRID_FREE];
  stats->n_obstacle = h[GRID_OBSTACLE];
  stats->n_no_ground = h[GRID_NO_GROUND];
  stats->n_filled = h[GRID_FILLED];
  return SUMA_OK;
}
