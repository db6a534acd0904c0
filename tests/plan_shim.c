/*
 * plan_shim.c -- the specification at the top of semantic_suma_amd/csrc/k_plan.hip restated on the host, sequentially:
 * the clearance by a search of the +-R window, the field by Dijkstra with a binary heap from all goals at once, `next`
 * and the paths read off it.  Compiled by the tests with gcc -O2 -ffp-contract=off; suma_grid_plan_field and
 * suma_grid_plan_paths must equal it byte for byte (n_rounds apart, which it leaves 0).
 * It shares no code with the library: the structures are declared again here.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define N_LABELS 260
#define INF 0xffffffffu

typedef struct {
  float cell_size, origin_x, origin_y;
  uint32_t width, height;
  uint8_t ground_label[N_LABELS];
  float min_normal_z, step_height, clearance;
  uint32_t fill_radius;
} grid_params_t;

typedef struct {
  float ground_z, ground_rough, z_min, z_max;
  float obstacle_z, prob;
  uint32_t label, support;
  uint32_t n_ground, n_obstacle, n_overhang;
  uint8_t state, ground_source, pad[2];
} cell_t;

typedef struct {
  float robot_radius, max_step, max_rough;
  uint32_t unknown_blocked, max_clear_cells, soft_cells, soft_weight;
  uint8_t label_cost[N_LABELS];
} plan_params_t;

typedef struct {
  uint32_t cost;
  uint16_t clear2;
  uint8_t flags, next;
} plan_cell_t;

typedef struct {
  uint32_t n_blocked, n_traversable, n_reached, n_goals, n_goals_ignored, max_cost, n_rounds;
} plan_stats_t;

typedef struct {
  uint32_t length, status, cost, pad;
} plan_path_t;

enum { ST_UNKNOWN = 0, ST_FREE = 1, ST_OBSTACLE = 2, ST_NO_GROUND = 3 };
enum { PATH_OK = 0, PATH_UNREACHED = 1, PATH_START_OUTSIDE = 2, PATH_TRUNCATED = 3, PATH_BAD_FIELD = 4 };

static const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
static const int DY[8] = {0, 1, 1, 1, 0, -1, -1, -1};

typedef struct {
  uint32_t width, height;
  const cell_t* cells;
  const uint8_t* trav;
  const uint32_t* w;
  float max_step;
} graph_t;

static int inside(const graph_t* g, int64_t x, int64_t y) { return x >= 0 && y >= 0 && x < (int64_t)g->width && y < (int64_t)g->height; }

static int trav_at(const graph_t* g, int64_t x, int64_t y) { return inside(g, x, y) && g->trav[y * g->width + x]; }

/* the cost of the move from (x, y) in direction k, or 0 when it is not allowed (every allowed move costs >= 20) */
static uint32_t edge(const graph_t* g, int64_t x, int64_t y, int k) {
  const int64_t nx = x + DX[k], ny = y + DY[k];
  if (!trav_at(g, x, y) || !trav_at(g, nx, ny)) return 0;
  const float a = g->cells[y * g->width + x].ground_z, b = g->cells[ny * g->width + nx].ground_z;
  if (!(fabsf(a - b) <= g->max_step)) return 0;
  if ((k & 1) && !(trav_at(g, nx, y) && trav_at(g, x, ny))) return 0;
  return ((k & 1) ? 14u : 10u) * (g->w[y * g->width + x] + g->w[ny * g->width + nx]);
}

/* a binary min-heap of (cost, cell), lazy deletion */
typedef struct {
  uint32_t cost, cell;
} item_t;
typedef struct {
  item_t* a;
  size_t n, cap;
} heap_t;

static int heap_push(heap_t* h, uint32_t cost, uint32_t cell) {
  if (h->n == h->cap) {
    const size_t cap = h->cap ? 2 * h->cap : 1024;
    item_t* a = (item_t*)realloc(h->a, cap * sizeof(item_t));
    if (!a) return -1;
    h->a = a, h->cap = cap;
  }
  size_t i = h->n++;
  while (i > 0 && h->a[(i - 1) / 2].cost > cost) h->a[i] = h->a[(i - 1) / 2], i = (i - 1) / 2;
  h->a[i].cost = cost, h->a[i].cell = cell;
  return 0;
}

static item_t heap_pop(heap_t* h) {
  const item_t top = h->a[0], last = h->a[--h->n];
  size_t i = 0;
  for (;;) {
    size_t c = 2 * i + 1;
    if (c >= h->n) break;
    if (c + 1 < h->n && h->a[c + 1].cost < h->a[c].cost) ++c;
    if (h->a[c].cost >= last.cost) break;
    h->a[i] = h->a[c], i = c;
  }
  if (h->n) h->a[i] = last;
  return top;
}

/* 0, or -1 without memory.  The caller has checked the parameters as the entry does. */
int plan_shim_field(const grid_params_t* gp, const plan_params_t* pp, const cell_t* cells, const int64_t* goals, uint32_t n_goals,
                    plan_cell_t* field, plan_stats_t* stats) {
  const int64_t W = gp->width, H = gp->height, n = W * H, R = pp->max_clear_cells;
  const uint32_t cap = (uint32_t)((R + 1) * (R + 1));
  uint8_t* blocked = (uint8_t*)calloc((size_t)n, 1);
  uint8_t* trav = (uint8_t*)calloc((size_t)n, 1);
  uint32_t* w = (uint32_t*)calloc((size_t)n, sizeof(uint32_t));
  heap_t heap = {0, 0, 0};
  int rc = -1;
  if (!blocked || !trav || !w) goto out;
  memset(stats, 0, sizeof(*stats));
  memset(field, 0, (size_t)n * sizeof(plan_cell_t));
  stats->n_goals = n_goals;
  for (int64_t c = 0; c < n; ++c) {
    const uint32_t L = cells[c].label < N_LABELS ? cells[c].label : 0;
    int b = cells[c].state == ST_OBSTACLE || cells[c].state == ST_NO_GROUND;
    if (cells[c].state != ST_OBSTACLE && cells[c].state != ST_NO_GROUND && cells[c].state != ST_FREE && pp->unknown_blocked) b = 1;
    if (pp->label_cost[L] == 0) b = 1;
    if (!isnan(pp->max_rough) && cells[c].ground_rough > pp->max_rough) b = 1;
    blocked[c] = (uint8_t)b;
    stats->n_blocked += (uint32_t)b;
  }
  for (int64_t y = 0; y < H; ++y)
    for (int64_t x = 0; x < W; ++x) {
      const int64_t c = y * W + x;
      uint32_t clear2 = cap;
      for (int64_t dy = -R; dy <= R; ++dy)
        for (int64_t dx = -R; dx <= R; ++dx) {
          const int64_t qx = x + dx, qy = y + dy;
          if (qx < 0 || qy < 0 || qx >= W || qy >= H || !blocked[qy * W + qx]) continue;
          const uint32_t d2 = (uint32_t)(dx * dx + dy * dy);
          if (d2 < clear2) clear2 = d2;
        }
      const uint32_t L = cells[c].label < N_LABELS ? cells[c].label : 0;
      uint32_t s = 0;
      while ((s + 1) * (s + 1) <= clear2) ++s;
      w[c] = pp->label_cost[L] + pp->soft_weight * (s < pp->soft_cells ? pp->soft_cells - s : 0u);
      trav[c] = !blocked[c] && sqrtf((float)clear2) * gp->cell_size >= pp->robot_radius;
      field[c].cost = INF;
      field[c].clear2 = (uint16_t)clear2;
      field[c].flags = (uint8_t)(blocked[c] | (trav[c] << 1));
      field[c].next = 255;
      stats->n_traversable += trav[c];
    }
  {
    const graph_t g = {gp->width, gp->height, cells, trav, w, pp->max_step};
    for (uint32_t i = 0; i < n_goals; ++i) {
      if (!trav[goals[i]]) {
        ++stats->n_goals_ignored;
      } else if (field[goals[i]].cost != 0) {
        field[goals[i]].cost = 0;
        if (heap_push(&heap, 0, (uint32_t)goals[i])) goto out;
      }
    }
    while (heap.n) {
      const item_t it = heap_pop(&heap);
      if (it.cost != field[it.cell].cost) continue; /* a stale entry */
      const int64_t x = it.cell % W, y = it.cell / W;
      for (int k = 0; k < 8; ++k) {
        const uint32_t e = edge(&g, x, y, k);
        if (!e) continue;
        const int64_t nc = (y + DY[k]) * W + x + DX[k];
        if (it.cost + e < field[nc].cost) {
          field[nc].cost = it.cost + e;
          if (heap_push(&heap, it.cost + e, (uint32_t)nc)) goto out;
        }
      }
    }
    for (int64_t c = 0; c < n; ++c) {
      const uint32_t mine = field[c].cost;
      if (mine == INF) continue;
      field[c].flags |= 4;
      ++stats->n_reached;
      if (mine > stats->max_cost) stats->max_cost = mine;
      if (mine == 0) {
        field[c].next = 8;
        continue;
      }
      const int64_t x = c % W, y = c / W;
      for (int k = 0; k < 8; ++k) {
        const uint32_t e = edge(&g, x, y, k);
        if (!e) continue;
        const uint32_t cn = field[(y + DY[k]) * W + x + DX[k]].cost;
        if (cn != INF && cn + e == mine) {
          field[c].next = (uint8_t)k;
          break;
        }
      }
    }
  }
  rc = 0;
out:
  free(blocked), free(trav), free(w), free(heap.a);
  return rc;
}

void plan_shim_paths(const grid_params_t* gp, const plan_cell_t* field, const int64_t* starts, uint32_t n_starts, uint32_t capacity,
                     uint32_t* path_cells, plan_path_t* results) {
  const int64_t W = gp->width, H = gp->height, n = W * H;
  memset(path_cells, 0xff, (size_t)n_starts * capacity * sizeof(uint32_t));
  for (uint32_t s = 0; s < n_starts; ++s) {
    uint32_t* row = path_cells + (size_t)s * capacity;
    plan_path_t r = {0, PATH_START_OUTSIDE, INF, 0};
    int64_t c = starts[s];
    if (c >= 0 && c < n) {
      r.cost = field[c].cost;
      r.status = PATH_UNREACHED;
      if (field[c].next != 255) {
        int64_t x = c % W, y = c / W;
        r.length = 1, r.status = PATH_BAD_FIELD;
        row[0] = (uint32_t)c; /* capacity >= 1 */
        for (int64_t step = 0; step < n; ++step) {
          const uint32_t k = field[c].next;
          if (k == 8) {
            r.status = PATH_OK;
            break;
          }
          if (k > 7) break;
          x += DX[k], y += DY[k];
          if (x < 0 || y < 0 || x >= W || y >= H) break;
          const int64_t nc = y * W + x;
          if (!(field[nc].cost < field[c].cost)) break;
          c = nc;
          if (r.length < capacity) row[r.length] = (uint32_t)c;
          ++r.length;
        }
        if (r.status == PATH_OK && r.length > capacity) r.status = PATH_TRUNCATED;
      }
    }
    results[s] = r;
  }
}

/* sizes and offsets, for the layout test */
uint32_t plan_shim_sizeof(int which) {
  return which == 0 ? (uint32_t)sizeof(plan_params_t) : which == 1 ? (uint32_t)sizeof(plan_cell_t)
       : which == 2 ? (uint32_t)sizeof(plan_stats_t) : (uint32_t)sizeof(plan_path_t);
}
