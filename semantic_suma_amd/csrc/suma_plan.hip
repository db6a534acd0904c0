/*
 * suma_plan.hip -- the entries of planning on the traversability grid (include/suma_hip.h: suma_plan_params_default,
 * suma_grid_cell_index, suma_grid_plan_field, suma_grid_plan_paths).  Host code: the parameter checks, the scratch, the
 * exchange of goals, starts and paths, the stats.  k_plan.hip states the specification and holds the kernels.
 */
#include <cmath>
#include <cstring>

#include "suma_internal.h"

#define PLAN_MAX_CELLS (1u << 26)
#define PLAN_MAX_PATH_CAPACITY (1u << 20)

extern "C" void suma_plan_params_default(suma_plan_params* pp) {
  if (!pp) return;
  std::memset(pp, 0, sizeof(*pp));
  pp->robot_radius = 0.4f;
  pp->max_step = 0.15f;
  pp->max_rough = NAN;
  pp->unknown_blocked = 1;
  pp->max_clear_cells = 16;
  pp->soft_cells = 3;
  pp->soft_weight = 2;
  std::memset(pp->label_cost, 1, sizeof(pp->label_cost));
}

extern "C" int64_t suma_grid_cell_index(const suma_grid_params* gp, float x, float y) {
  if (!gp || !(std::isfinite(x) && std::isfinite(y))) return -1;
  const float fx = sdm_floor((x - gp->origin_x) / gp->cell_size), fy = sdm_floor((y - gp->origin_y) / gp->cell_size);
  if (!(fx >= 0.0f && fx < (float)gp->width && fy >= 0.0f && fy < (float)gp->height)) return -1;
  return (int64_t)(uint32_t)fy * gp->width + (int64_t)(uint32_t)fx;
}

/* what both entries read of the grid's parameters */
static int plan_check_raster(suma_ctx* c, const std::string& who, const suma_grid_params* gp) {
  if (!gp) return fail(c, SUMA_ERR_INVALID, who + ": NULL grid parameters");
  if (!(std::isfinite(gp->cell_size) && gp->cell_size > 0.0f))
    return fail(c, SUMA_ERR_INVALID, who + ": cell_size = " + std::to_string(gp->cell_size) + " (must be finite and > 0)");
  if (gp->width < 1 || gp->height < 1 || (uint64_t)gp->width * gp->height > PLAN_MAX_CELLS)
    return fail(c, SUMA_ERR_INVALID, who + ": width x height = " + std::to_string(gp->width) + " x " + std::to_string(gp->height) +
                                         " (each >= 1, width * height <= 2^26)");
  return SUMA_OK;
}

extern "C" int suma_grid_plan_field(suma_ctx* c, const suma_grid_params* gp, const suma_plan_params* pp,
                                    const suma_grid_cell* d_cells, const int64_t* goals, uint32_t n_goals, suma_plan_cell* d_field,
                                    suma_plan_stats* stats) {
  if (!c) return SUMA_ERR_INVALID;
  const std::string who = "suma_grid_plan_field";
  int r = plan_check_raster(c, who, gp);
  if (r) return r;
  if (!pp) return fail(c, SUMA_ERR_INVALID, who + ": NULL plan parameters");
  if (!stats) return fail(c, SUMA_ERR_INVALID, who + ": NULL stats");
  if (!d_cells) return fail(c, SUMA_ERR_INVALID, who + ": NULL cells");
  if ((uintptr_t)d_cells & 15u) return fail(c, SUMA_ERR_INVALID, who + ": cells not 16-byte aligned");
  if (!d_field) return fail(c, SUMA_ERR_INVALID, who + ": NULL field");
  if ((uintptr_t)d_field & 7u) return fail(c, SUMA_ERR_INVALID, who + ": field not 8-byte aligned");
  if (!goals) return fail(c, SUMA_ERR_INVALID, who + ": NULL goals");
  if (n_goals < 1 || n_goals > SUMA_PLAN_MAX_GOALS)
    return fail(c, SUMA_ERR_INVALID, who + ": n_goals = " + std::to_string(n_goals) + " (1 .. 4096)");
  const uint32_t R = pp->max_clear_cells;
  if (R < 1 || R > SUMA_PLAN_MAX_CLEAR_CELLS)
    return fail(c, SUMA_ERR_INVALID, who + ": max_clear_cells = " + std::to_string(R) + " (1 .. 64)");
  if (pp->soft_cells > R + 1u)
    return fail(c, SUMA_ERR_INVALID, who + ": soft_cells = " + std::to_string(pp->soft_cells) + " (0 .. max_clear_cells + 1)");
  if (pp->soft_weight > 255u) return fail(c, SUMA_ERR_INVALID, who + ": soft_weight = " + std::to_string(pp->soft_weight) + " (0 .. 255)");
  if (pp->unknown_blocked > 1u)
    return fail(c, SUMA_ERR_INVALID, who + ": unknown_blocked = " + std::to_string(pp->unknown_blocked) + " (0 or 1)");
  if (std::isnan(pp->max_step)) return fail(c, SUMA_ERR_INVALID, who + ": max_step is NaN");
  if (!(std::isfinite(pp->robot_radius) && pp->robot_radius >= 0.0f && pp->robot_radius <= (float)R * gp->cell_size))
    return fail(c, SUMA_ERR_INVALID, who + ": robot_radius = " + std::to_string(pp->robot_radius) +
                                         " (must be finite, >= 0 and <= max_clear_cells * cell_size)");
  const uint64_t n_cells = (uint64_t)gp->width * gp->height;
  for (uint32_t i = 0; i < n_goals; ++i)
    if (goals[i] < 0 || (uint64_t)goals[i] >= n_cells)
      return fail(c, SUMA_ERR_INVALID, who + ": goal " + std::to_string(i) + " = " + std::to_string(goals[i]) + " is not a cell of the raster");
  const uint64_t w_max = 255u + (uint64_t)pp->soft_weight * pp->soft_cells;
  if (n_cells * 28u * w_max >= (1ull << 32))
    return fail(c, SUMA_ERR_CAPACITY, who + ": width * height * 28 * (255 + soft_weight * soft_cells) = " +
                                          std::to_string(n_cells * 28u * w_max) + " (must be < 2^32: a cost could wrap)");

  if ((r = grow(c, c->plan_counters, PLAN_COUNTERS, {c->stream})) < 0) return r;
  if ((r = grow(c, c->plan_counters_h, PLAN_COUNTERS, {c->stream})) < 0) return r;
  if ((r = grow(c, c->plan_scratch, plan_scratch_bytes(gp->width, gp->height), {c->stream})) < 0) return r;
  if ((r = grow(c, c->plan_io, n_goals, {c->stream})) < 0) return r;
  if ((r = grow(c, c->plan_io_h, n_goals, {c->stream})) < 0) return r;
  for (uint32_t i = 0; i < n_goals; ++i) c->plan_io_h[i] = (uint32_t)goals[i];
  HIP_TRY(c, hipMemcpyAsync(c->plan_io, c->plan_io_h, n_goals * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_plan_prepare(c, *gp, *pp, d_cells, n_goals, d_field));
  uint32_t n_rounds = 0;
  if ((r = launch_plan_relax(c, *gp, &n_rounds))) return r;
  HIP_TRY(c, launch_plan_next(c, *gp, d_field));
  HIP_TRY(c, hipMemcpyAsync(c->plan_counters_h, c->plan_counters, PLAN_ROUND_FLAGS * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t* h = c->plan_counters_h;
  std::memset(stats, 0, sizeof(*stats));
  stats->n_blocked = h[PLAN_BLOCKED];
  stats->n_traversable = h[PLAN_TRAVERSABLE];
  stats->n_reached = h[PLAN_REACHED];
  stats->n_goals = n_goals;
  stats->n_goals_ignored = h[PLAN_GOALS_IGNORED];
  stats->max_cost = h[PLAN_MAX_COST];
  stats->n_rounds = n_rounds;
  return SUMA_OK;
}

extern "C" int suma_grid_plan_paths(suma_ctx* c, const suma_grid_params* gp, const suma_plan_cell* d_field, const int64_t* starts,
                                    uint32_t n_starts, uint32_t path_capacity, uint32_t* path_cells, suma_plan_path* results) {
  if (!c) return SUMA_ERR_INVALID;
  const std::string who = "suma_grid_plan_paths";
  int r = plan_check_raster(c, who, gp);
  if (r) return r;
  if (!d_field) return fail(c, SUMA_ERR_INVALID, who + ": NULL field");
  if ((uintptr_t)d_field & 7u) return fail(c, SUMA_ERR_INVALID, who + ": field not 8-byte aligned");
  if (!starts) return fail(c, SUMA_ERR_INVALID, who + ": NULL starts");
  if (!path_cells) return fail(c, SUMA_ERR_INVALID, who + ": NULL path_cells");
  if (!results) return fail(c, SUMA_ERR_INVALID, who + ": NULL results");
  if (n_starts < 1 || n_starts > SUMA_PLAN_MAX_STARTS)
    return fail(c, SUMA_ERR_INVALID, who + ": n_starts = " + std::to_string(n_starts) + " (1 .. 4096)");
  if (path_capacity < 1 || path_capacity > PLAN_MAX_PATH_CAPACITY || (uint64_t)n_starts * path_capacity > PLAN_MAX_CELLS)
    return fail(c, SUMA_ERR_INVALID, who + ": path_capacity = " + std::to_string(path_capacity) +
                                         " (1 .. 2^20, n_starts * path_capacity <= 2^26)");
  const uint64_t n_cells = (uint64_t)gp->width * gp->height;
  const size_t words = (size_t)n_starts * (5u + (size_t)path_capacity); /* results, starts, path cells */
  if ((r = grow(c, c->plan_io, words, {c->stream})) < 0) return r;
  if ((r = grow(c, c->plan_io_h, n_starts, {c->stream})) < 0) return r;
  for (uint32_t i = 0; i < n_starts; ++i)
    c->plan_io_h[i] = (starts[i] < 0 || (uint64_t)starts[i] >= n_cells) ? 0xffffffffu : (uint32_t)starts[i];
  uint32_t* io = c->plan_io;
  HIP_TRY(c, hipMemcpyAsync(io + 4 * (size_t)n_starts, c->plan_io_h, n_starts * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, launch_plan_walk(c, *gp, d_field, n_starts, path_capacity));
  /* results and rows are one stretch of the scratch apart from the starts between them: two copies, one wait */
  HIP_TRY(c, hipMemcpyAsync(results, io, (size_t)n_starts * sizeof(suma_plan_path), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(path_cells, io + 5 * (size_t)n_starts, (size_t)n_starts * path_capacity * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SUMA_OK;
}
