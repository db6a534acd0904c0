"""The planner's specification on the host (tests/plan_shim.c, the yardstick of test_gpu_plan.py): the shim -- a window
search and Dijkstra with a heap -- against an independent numpy statement of every rule -- clearance over all blocked cells,
Bellman-Ford sweeps until nothing changes -- on crafted grids; the walk against plain python; the .npz round trip; the shim
under the address and undefined-behaviour sanitizers as a stand-alone program; and one semantic check end to end without a
GPU: a way round the cube of test_grid_host.py's synthetic street."""
import math
import os
import subprocess

import numpy as np
import pytest

import grid_common as gc
import plan_common as pc
import world_common as wc
from semantic_suma_amd import core, mapio, synth
from semantic_suma_amd.types import (GRID_FREE, GRID_NO_GROUND, GRID_OBSTACLE, PLAN_CELL_DTYPE, PLAN_DIRECTIONS, PlanParams,
                                     params_with_size)

INF = pc.INF
BIG = 1 << 40


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return pc.build_shim(tmp_path_factory.mktemp("plan_host"))


def shifted(a, k, fill):
    """a[y + dy, x + dx] at (y, x), `fill` outside"""
    dx, dy = PLAN_DIRECTIONS[k]
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def numpy_plan(cells, gp, pp, goals):
    """the specification stated with numpy: (field, stats without n_rounds)"""
    H, W, R = gp.height, gp.width, pp.max_clear_cells
    cells = cells.reshape(H, W)
    cost_of = np.array(list(pp.label_cost), dtype=np.int64)
    L = np.where(cells["label"] < 260, cells["label"], 0)
    state = cells["state"]
    blocked = (state == GRID_OBSTACLE) | (state == GRID_NO_GROUND) | (cost_of[L] == 0)
    if pp.unknown_blocked:
        blocked |= ~np.isin(state, (GRID_FREE, GRID_OBSTACLE, GRID_NO_GROUND))
    if not math.isnan(pp.max_rough):
        with np.errstate(invalid="ignore"):
            blocked |= cells["ground_rough"] > np.float32(pp.max_rough)
    clear2 = pc.numpy_clear2(blocked, R)
    trav = ~blocked & (np.sqrt(clear2.astype(np.float32)) * np.float32(gp.cell_size) >= np.float32(pp.robot_radius))
    s = np.array([math.isqrt(int(v)) for v in clear2.ravel()], dtype=np.int64).reshape(H, W)
    w = cost_of[L] + pp.soft_weight * np.maximum(0, pp.soft_cells - s)
    gz = cells["ground_z"].astype(np.float32)
    edge = []
    for k in range(8):
        with np.errstate(invalid="ignore"):
            ok = trav & shifted(trav, k, False) & (np.abs(gz - shifted(gz, k, np.float32(np.nan))) <= np.float32(pp.max_step))
        if k % 2:
            ok &= shifted(trav, (k + 1) % 8, False) & shifted(trav, k - 1, False)
        edge.append(np.where(ok, (14 if k % 2 else 10) * (w + shifted(w, k, 0)), 0))
    cost = np.full((H, W), BIG, dtype=np.int64)
    ignored = 0
    for g in goals:
        if trav.ravel()[g]:
            cost.ravel()[g] = 0
        else:
            ignored += 1
    for _ in range(W * H + 1):
        new = cost.copy()
        for k in range(8):
            new = np.minimum(new, np.where(edge[k] > 0, shifted(cost, k, BIG) + edge[k], BIG))
        if np.array_equal(new, cost):
            break
        cost = new
    reached = cost < BIG
    nxt = np.full((H, W), 255, dtype=np.int64)
    for k in reversed(range(8)):
        nxt = np.where(reached & (edge[k] > 0) & (shifted(cost, k, BIG) + edge[k] == cost), k, nxt)
    nxt = np.where(cost == 0, 8, nxt)
    field = np.zeros((H, W), dtype=PLAN_CELL_DTYPE)
    field["cost"] = np.where(reached, cost, INF)
    field["clear2"], field["next"] = clear2, nxt
    field["flags"] = blocked * 1 + trav * 2 + reached * 4
    stats = dict(n_blocked=int(blocked.sum()), n_traversable=int(trav.sum()), n_reached=int(reached.sum()), n_goals=len(goals),
                 n_goals_ignored=ignored, max_cost=int(cost[reached].max()) if reached.any() else 0, n_rounds=0)
    return field, stats


def same(shim, cells, gp, pp, goals, where=""):
    """the shim's field equals numpy's on (cells, gp, pp, goals): bytes and stats; returns (field, stats)"""
    assert pc.check_params(gp, pp) == 0
    got, st = pc.shim_field(shim, cells, gp, pp, goals)
    want, wst = numpy_plan(cells, gp, pp, goals)
    assert st == wst, (where, st, wst)
    if got.tobytes() != want.tobytes():
        bad = [f for f in PLAN_CELL_DTYPE.names if got[f].tobytes() != want[f].tobytes()]
        raise AssertionError((where, bad, int((got.view(np.uint8) != want.view(np.uint8)).sum())))
    return got, st


@pytest.mark.parametrize("density", [0.0, 0.05, 0.3, 1.0])
@pytest.mark.parametrize("size", [(1, 1), (1, 70), (65, 3), (47, 41)])
def test_shim_equals_numpy_on_random_grids(shim, size, density):
    W, H = size
    c = pc.random_grid(W, H, density)
    rng = np.random.default_rng(W + H)
    goals = rng.integers(0, W * H, 3)
    for pp in (PlanParams.defaults(robot_radius=0.3), pc.plain(), pc.plain(unknown_blocked=False, max_rough=0.0625, max_step=0.0625),
               PlanParams.defaults(robot_radius=0.0, max_clear_cells=5, soft_cells=6, soft_weight=7, label_cost={48: 4, 72: 0})):
        _, st = same(shim, c, pc.raster(W, H), pp, goals, (size, density))
        assert density < 1.0 or not pp.unknown_blocked or st["n_blocked"] == W * H


@pytest.mark.parametrize("corner", [False, True])
@pytest.mark.parametrize("R", [1, 2, 16, 64])
def test_clearance_probes(shim, R, corner):
    c, gp, pp, goals, (bx, by) = pc.probe_scene(R, corner)
    got, st = pc.shim_field(shim, c, gp, pp, goals)
    iy, ix = np.mgrid[0:gp.height, 0:gp.width]
    d2 = (ix - bx) ** 2 + (iy - by) ** 2
    cap = (R + 1) ** 2
    assert np.array_equal(got["clear2"], np.minimum(d2, cap)) and st["n_blocked"] == 1
    assert got["clear2"][by, bx + R] == R * R and got["clear2"][by + 1, bx + R] == R * R + 1 and got["clear2"][by, bx + R + 1] == cap
    assert got["clear2"][by + R, bx] == R * R and got["clear2"][by + R, bx + 1] == R * R + 1 and got["clear2"][by + R + 1, bx] == cap
    below = d2[d2 < cap].max()                       # the largest distance under the cap that two squares sum to
    assert below <= cap - 1 and (R not in (2, 16) or below == cap - 1)
    assert np.array_equal(got["clear2"][d2 == below], d2[d2 == below])


def test_three_four_five(shim):
    c = pc.free_grid(30, 30)
    pc.block(c, (10, 10))
    gp = pc.raster(30, 30, cell_size=0.2)
    r = np.float32(5.0) * np.float32(0.2)
    for radius, want in ((r, True), (np.nextafter(r, np.float32(np.inf)), False)):
        got, _ = same(shim, c, gp, PlanParams.defaults(robot_radius=float(radius)), [0])
        assert got["clear2"][14, 13] == 25 and bool(got["flags"][14, 13] & 2) == want
        assert bool(got["flags"][15, 13] & 2) and not got["flags"][13, 13] & 2


@pytest.mark.parametrize("case", pc.edge_cases(), ids=lambda c: c[0])
def test_edge_rules(shim, case):
    _, c, gp, pp, goals, expect = case
    got, _ = same(shim, c, gp, pp, goals)
    for (x, y), want in expect.items():
        assert (int(got[y, x]["cost"]), int(got[y, x]["next"]), int(got[y, x]["flags"])) == want, (x, y)


def test_serpentine(shim):
    c, gp, pp, goals = pc.serpentine()
    got, st = same(shim, c, gp, pp, goals)
    start = 32 * 65 + 64                                                  # the last corridor's far end (its gap is at x = 0)
    res, rows = pc.shim_paths(shim, got, gp, [start], 2000)
    n = int(res[0]["length"])
    assert res[0]["status"] == 0 and n > 1000 and rows[0, n - 1] == 0 and res[0]["cost"] == got[32, 64]["cost"] == 20 * (n - 1)
    assert set((rows[0, :n] // 65).tolist()) == set(range(33))            # every corridor and every gap
    assert st["n_reached"] == st["n_traversable"] == 17 * 65 + 16


def test_unreachable_islands_and_ignored_goals(shim):
    c = pc.free_grid(40, 20)
    pc.block(c, (slice(None), 20))                                        # a wall cuts the raster in two
    gp, pp = pc.raster(40, 20), pc.plain()
    got, st = same(shim, c, gp, pp, [5, 20, 20, 3 * 40 + 20])             # one goal on the left, three entries on the wall
    assert st["n_goals"] == 4 and st["n_goals_ignored"] == 3
    right = got[:, 21:]
    assert np.all(right["cost"] == INF) and np.all(right["next"] == 255) and np.all(right["flags"] == 2)
    assert np.all(got[:, :20]["flags"] == 6) and st["n_reached"] == 20 * 20
    got, st = same(shim, c, gp, pp, [20, 60])                             # every goal blocked: nothing is reached
    assert st["n_goals_ignored"] == 2 and st["n_reached"] == 0 and st["max_cost"] == 0 and np.all(got["cost"] == INF)
    assert np.all(got["next"] == 255) and not np.any(got["flags"] & 4)


def test_ties_take_the_smallest_direction(shim):
    c, gp = pc.free_grid(41, 41), pc.raster(41, 41)
    got, _ = same(shim, c, gp, pc.plain(), [20 * 41 + 20])
    # two cells west and one south of the goal: E then NE, or NE then E -- both 48; the smaller direction is E
    assert got[19, 18]["cost"] == 48 and got[19, 18]["next"] == 0
    assert got[20, 25]["next"] == 4 and got[25, 25]["next"] == 5 and got[15, 15]["next"] == 1 and got[20, 20]["next"] == 8


def test_soft_cost_centres_the_path(shim):
    start = 2 * 40 + 1
    c, gp, pp, goals = pc.soft_corridor(2)
    got, _ = same(shim, c, gp, pp, goals)
    res, rows = pc.shim_paths(shim, got, gp, [start], 100)
    path = rows[0, :res[0]["length"]]
    assert res[0]["status"] == 0 and np.all((path // 40)[path % 40 >= 4] == 4)
    c, gp, pp, goals = pc.soft_corridor(0)
    got0, _ = same(shim, c, gp, pp, goals)
    assert got0[2, 1]["cost"] == 2 * 28 + 35 * 20 < got[2, 1]["cost"]


def test_paths_against_python(shim):
    c = pc.random_grid(47, 41, 0.15, bumpy=False)
    gp = pc.raster(47, 41)
    field, _ = pc.shim_field(shim, c, gp, pc.plain(), [0, 46 * 41])
    starts = list(range(-2, 47 * 41 + 2, 7))
    for cap in (1, 5, 200):
        res, rows = pc.shim_paths(shim, field, gp, starts, cap)
        for s, r, row in zip(starts, res, rows):
            n, status, cost, cells = pc.python_walk(field, s, cap)
            assert (int(r["length"]), int(r["status"]), int(r["cost"]), int(r["pad"])) == (n, status, cost, 0), s
            assert row[:len(cells)].tolist() == cells and np.all(row[len(cells):] == INF)
    assert {0, 1, 2, 3} == set(pc.shim_paths(shim, field, gp, starts, 5)[0]["status"].tolist())
    # a field that lies: a two-cycle, a step off the raster, a cost that does not fall
    for name, edit in (("cycle", lambda f: f["next"].__setitem__((slice(3, 4), slice(3, 5)), [[0, 4]])),
                       ("leaves", lambda f: f["next"].__setitem__((0, 0), 4)),
                       ("cost", lambda f: f["cost"].__setitem__((4, 4), f["cost"][3, 3]))):
        bad = pc.free_grid(8, 8)
        f, _ = pc.shim_field(shim, bad, pc.raster(8, 8), pc.plain(), [63])
        f["next"][0, 0] = 1
        edit(f)
        start = 0 if name == "leaves" else 3 * 8 + 3
        res, rows = pc.shim_paths(shim, f, pc.raster(8, 8), [start], 20)
        assert res[0]["status"] == 4 and (int(res[0]["length"]), 4) == pc.python_walk(f, start, 20)[:2], name
        assert res[0]["length"] == (2 if name == "cycle" else 1)


def test_parameter_checks_as_the_header_states_them():
    gp = pc.raster(257, 129)
    assert pc.check_params(gp, PlanParams.defaults()) == 0
    assert pc.check_params(gp, PlanParams.defaults(max_clear_cells=64, soft_cells=65, soft_weight=255, robot_radius=0.0)) == -3
    assert pc.check_params(gp, PlanParams.defaults(robot_radius=16 * 0.25)) == 0
    assert pc.check_params(gp, PlanParams.defaults(robot_radius=4.01)) == -1


def test_plan_file_round_trip(tmp_path, shim):
    c, gp, pp, goals = pc.soft_corridor(2)
    field, _ = pc.shim_field(shim, c, gp, pp, goals)
    path = str(tmp_path / "map.plan.npz")
    mapio.write_plan(path, field, gp, pp)
    back, gp2, pp2 = mapio.read_plan(path)
    assert back.dtype == PLAN_CELL_DTYPE and back.shape == (9, 40) and back.tobytes() == field.tobytes()
    assert bytes(gp2) == bytes(gp) and bytes(pp2) == bytes(pp)
    with pytest.raises(ValueError):
        mapio.write_plan(path, field[:, :5], gp, pp)
    mapio.write_grid(path, c, gp)
    with pytest.raises(ValueError):
        mapio.read_plan(path)


SANITIZER_MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "plan_shim.c"
/* two crafted grids through the field and the walk: a wall with a gap at R = 64 on a raster smaller than the window, and
 * a raster of one row; every start from one before the raster to one behind it, with a capacity that truncates */
static int run(uint32_t W, uint32_t H, uint32_t R, uint32_t capacity) {
  grid_params_t gp;
  plan_params_t pp;
  memset(&gp, 0, sizeof gp), memset(&pp, 0, sizeof pp);
  gp.cell_size = 0.25f, gp.width = W, gp.height = H;
  pp.robot_radius = 0.25f, pp.max_step = 0.15f, pp.max_rough = NAN, pp.unknown_blocked = 1, pp.max_clear_cells = R;
  pp.soft_cells = R + 1, pp.soft_weight = 255;
  memset(pp.label_cost, 1, sizeof pp.label_cost);
  const uint32_t n = W * H;
  cell_t* cells = calloc(n, sizeof(cell_t));
  plan_cell_t* field = malloc(n * sizeof(plan_cell_t));
  int64_t* starts = malloc((n + 2) * sizeof(int64_t));
  uint32_t* rows = malloc((size_t)(n + 2) * capacity * sizeof(uint32_t));
  plan_path_t* res = malloc((n + 2) * sizeof(plan_path_t));
  for (uint32_t c = 0; c < n; ++c) {
    cells[c].state = (H > 2 && c / W == H / 2 && c % W != W - 1) ? ST_OBSTACLE : ST_FREE;
    cells[c].label = c % 7 == 0 ? 300 : 40;
  }
  const int64_t goals[3] = {0, (int64_t)n - 1, (int64_t)(H / 2) * W};
  plan_stats_t st;
  if (plan_shim_field(&gp, &pp, cells, goals, 3, field, &st)) return 1;
  for (uint32_t i = 0; i < n + 2; ++i) starts[i] = (int64_t)i - 1;
  plan_shim_paths(&gp, field, starts, n + 2, capacity, rows, res);
  uint32_t ok = 0;
  for (uint32_t i = 0; i < n + 2; ++i) ok += res[i].status == PATH_OK || res[i].status == PATH_TRUNCATED;
  printf("%u x %u: blocked %u traversable %u reached %u ignored %u max %u paths %u\n", W, H, st.n_blocked, st.n_traversable,
         st.n_reached, st.n_goals_ignored, st.max_cost, ok);
  free(cells), free(field), free(starts), free(rows), free(res);
  return st.n_reached == ok ? 0 : 1;
}
int main(void) { return run(23, 17, 64, 6) | run(70, 1, 3, 100); }
"""


def test_shim_under_sanitizers(tmp_path):
    """plan_shim.c with a main of its own, compiled with -fsanitize=address,undefined and run: host C only"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.call(["gcc"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0 or \
            subprocess.call([str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("the compiler cannot link the sanitizers")
    src = tmp_path / "san_main.c"
    src.write_text(SANITIZER_MAIN)
    exe = tmp_path / "san_main"
    subprocess.check_call(["gcc"] + pc.SHIM_FLAGS + flags + ["-I", pc.HERE, str(src), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0, out.stdout.decode()
    assert out.stdout.decode().count("\n") == 2


# ---- end to end on the CPU: synth -> oracle pipeline -> world shim -> grid shim -> plan shim, against the scene
import test_grid_host as tgh  # noqa: E402 -- its scene, its footprints


@pytest.fixture(scope="module")
def street(tmp_path_factory):
    """the grid test_grid_host.py makes of its synthetic street beside the static cube (cube 8 of synth.py)"""
    from oracle import pyoracle
    p = params_with_size(900, 64)
    op = pyoracle.OraclePipeline(p)
    for k in range(tgh.K0, tgh.K0 + tgh.SCANS):
        pts, lab, prob, _ = synth.generate_scan(k, n_azimuth=900)
        lab = np.where(lab == synth.LABEL_CAR, np.float32(99.0), lab)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    poses = op.ctx.map_poses().reshape(-1, 4, 4).transpose(0, 2, 1)
    tmp = tmp_path_factory.mktemp("plan_world")
    world, _, _ = wc.shim_export(wc.build_shim(tmp), op.ctx.map_surfels(), poses, p.max_poses)
    fit = gc.fit_of(world, tgh.CELL, 1)
    gp = gc.params(fit[2], fit[3], tgh.CELL, origin=fit[:2])
    cells, _ = gc.shim_grid(gc.build_shim(tmp), world, gp)
    return cells, gp, synth.trajectory_pose(tgh.K0)


def test_a_way_round_the_cube(shim, street):
    cells, gp, T0 = street
    pp = PlanParams.defaults()                                            # robot_radius 0.4 m, UNKNOWN blocked
    centre, half, _, _ = synth._boxes(tgh.K0)
    cube = T0[:2, :2].T @ (centre[8, :2] - T0[:2, 3])                     # the cube's centre in the map frame
    iy, ix = np.mgrid[0:gp.height, 0:gp.width]
    xy = np.stack([gp.origin_x + (ix + 0.5) * gp.cell_size, gp.origin_y + (iy + 0.5) * gp.cell_size], -1)

    def nearest_traversable(field, want):
        d = np.where(field["flags"] & 2, np.linalg.norm(xy - want, axis=-1), np.inf)
        c = int(np.argmin(d))
        assert d.ravel()[c] < 0.5, (want, d.ravel()[c])
        return c
    # on opposite sides of the cube, 2.4 m from its centre: the straight line between them runs through it
    probe, _ = pc.shim_field(shim, cells, gp, pp, [0])
    goal, start = nearest_traversable(probe, cube + [1.4, -2.0]), nearest_traversable(probe, cube + [-1.4, 2.0])
    middle = 0.5 * (xy.reshape(-1, 2)[goal] + xy.reshape(-1, 2)[start]) @ T0[:2, :2].T + T0[:2, 3]
    assert tgh.footprint_distance(middle[None], [tgh.K0], moving=False)[0] < -0.3
    field, st = pc.shim_field(shim, cells, gp, pp, [goal])
    res, rows = pc.shim_paths(shim, field, gp, [start], gp.width + gp.height)
    n = int(res[0]["length"])
    path = rows[0, :n]
    assert res[0]["status"] == 0 and path[0] == start and path[-1] == goal and n > 25          # the path exists
    flat, f = cells.reshape(-1), field.reshape(-1)
    assert np.all(flat["state"][path] == GRID_FREE)
    assert np.all(np.sqrt(f["clear2"][path].astype(np.float32)) * np.float32(gp.cell_size) >= np.float32(pp.robot_radius))
    scene_xy = xy.reshape(-1, 2)[path] @ T0[:2, :2].T + T0[:2, 3]
    d = tgh.footprint_distance(scene_xy, [tgh.K0], moving=False)
    print(f"path of {n} cells, cost {res[0]['cost']}, nearest to a static footprint {d.min():.3f} m")
    assert d.min() >= pp.robot_radius                                     # outside the footprint grown by the radius
    assert res[0]["cost"] == f["cost"][start] and res[0]["cost"] >= 20 * (n - 1)
    # and through the public classes the same way: world coordinates in, cell centres out (no GPU: the shim's field)
    assert core.grid_cell_index(gp, *xy.reshape(-1, 2)[start]) == start
