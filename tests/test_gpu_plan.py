"""suma_grid_plan_field / suma_grid_plan_paths on the MI355X (csrc/k_plan.hip, core.grid_plan, core.grid_paths,
core.GridPlanner): the field's bytes, every stat but n_rounds, the paths' bytes and results against the host restatement
(tests/plan_shim.c) -- rasters around the relaxation tile's edges, blocked densities from none to all, the clearance at its
cap and across block edges, every rule of the edges, a serpentine that crosses every tile edge, islands, ties, the soft cost,
the capacity bound, validation, the walk with lying fields, determinism, no side effects, and a real pipeline's grid."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import loop_scenario as ls
import plan_common as pc
from semantic_suma_amd import core
from semantic_suma_amd.types import (GRID_CELL_DTYPE, PLAN_CELL_DTYPE, PLAN_PATH_DTYPE, GridParams, PlanParams, PlanStats,
                                     params_with_size)

pytestmark = pytest.mark.gpu
INF, T = pc.INF, pc.TILE  # T = PLAN_TILE of csrc/suma_internal.h, the relaxation's tile (test_abi_plan.py compares them)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return pc.build_shim(tmp_path_factory.mktemp("plan_gpu"))


@pytest.fixture(scope="module")
def ctx():
    return core.Context(params_with_size(900, 64))


def check(shim, ctx, cells, gp, pp, goals, where=""):
    """the field of the device equals the shim's: bytes and every stat but n_rounds; returns (field, stats)"""
    got, st = core.grid_plan(ctx, cells, gp, goals, pp)
    want, wst = pc.shim_field(shim, cells, gp, pp, goals)
    assert got.dtype == PLAN_CELL_DTYPE and got.shape == (gp.height, gp.width)
    assert st["n_rounds"] >= 1 and dict(st, n_rounds=0) == wst, (where, st, wst)
    if got.tobytes() != want.tobytes():
        bad = [f for f in PLAN_CELL_DTYPE.names if got[f].tobytes() != want[f].tobytes()]
        raise AssertionError((where, bad, int((got.view(np.uint8) != want.view(np.uint8)).sum())))
    return got, st


def check_paths(shim, ctx, field, gp, starts, capacity):
    """the paths of the device equal the shim's: results and rows, bytes; returns them"""
    res, rows = core.grid_paths(ctx, field, gp, starts, capacity)
    wres, wrows = pc.shim_paths(shim, field, gp, starts, capacity)
    assert res.dtype == PLAN_PATH_DTYPE and rows.shape == (len(starts), capacity)
    assert res.tobytes() == wres.tobytes() and rows.tobytes() == wrows.tobytes()
    return res, rows


SIZES = [(1, 1), (1, 70), (65, 3), (257, 129)] + [(T + a, T + b) for a, b in ((-1, 1), (0, 0), (1, -1))] + \
        [(2 * T + a, 2 * T + b) for a, b in ((-1, 0), (0, 1), (1, -1))]


@pytest.mark.parametrize("density", [0.0, 0.02, 0.3, 1.0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rasters_and_densities(shim, ctx, size, density):
    W, H = size
    c, gp = pc.random_grid(W, H, density), pc.raster(W, H)
    goals = np.random.default_rng(W * H).integers(0, W * H, 4)
    for pp in (PlanParams.defaults(robot_radius=0.3), pc.plain(),
               PlanParams.defaults(robot_radius=0.0, max_clear_cells=5, soft_cells=6, soft_weight=7, unknown_blocked=False,
                                   max_rough=0.0625, label_cost={48: 4, 72: 0})):
        got, st = check(shim, ctx, c, gp, pp, goals, (size, density))
        assert density < 1.0 or not pp.unknown_blocked or (st["n_blocked"] == W * H and st["n_reached"] == 0)
        assert density > 0.0 or pp.label_cost[72] == 0 or st["n_blocked"] == 0
    starts = np.random.default_rng(7).integers(-1, W * H + 1, 50)
    check_paths(shim, ctx, got, gp, starts, W + H)


@pytest.mark.parametrize("corner", [False, True])
@pytest.mark.parametrize("R", [1, 2, 16, 64])
def test_clearance_probes(shim, ctx, R, corner):
    c, gp, pp, goals, (bx, by) = pc.probe_scene(R, corner)
    got, _ = check(shim, ctx, c, gp, pp, goals, (R, corner))
    cap = (R + 1) ** 2
    iy, ix = np.mgrid[0:gp.height, 0:gp.width]
    d2 = (ix - bx) ** 2 + (iy - by) ** 2
    assert np.array_equal(got["clear2"], np.minimum(d2, cap))
    assert got["clear2"][by, bx + R] == R * R and got["clear2"][by + 1, bx + R] == R * R + 1 and got["clear2"][by, bx + R + 1] == cap
    assert got["clear2"][by + R, bx] == R * R and got["clear2"][by + R, bx + 1] == R * R + 1 and got["clear2"][by + R + 1, bx] == cap
    below = d2[d2 < cap].max()                       # the largest distance under the cap that two squares sum to
    assert R not in (2, 16) or below == cap - 1
    assert np.array_equal(got["clear2"][d2 == below], d2[d2 == below])
    # many blocked cells at this R, in a raster of several clearance blocks
    c = pc.random_grid(140, 40, 0.004, bumpy=False)
    check(shim, ctx, c, pc.raster(140, 40), PlanParams.defaults(max_clear_cells=R, robot_radius=0.25 * min(R, 3), soft_cells=R + 1),
          [0, 77, 5599], R)


def test_three_four_five(shim, ctx):
    c = pc.free_grid(30, 30)
    pc.block(c, (10, 10))
    gp = pc.raster(30, 30, cell_size=0.2)
    r = np.float32(5.0) * np.float32(0.2)
    for radius, want in ((r, True), (np.nextafter(r, np.float32(np.inf)), False)):
        got, _ = check(shim, ctx, c, gp, PlanParams.defaults(robot_radius=float(radius)), [0])
        assert got["clear2"][14, 13] == 25 and bool(got["flags"][14, 13] & 2) == want
        assert bool(got["flags"][15, 13] & 2) and not got["flags"][13, 13] & 2


@pytest.mark.parametrize("case", pc.edge_cases(), ids=lambda c: c[0])
def test_edge_rules(shim, ctx, case):
    _, c, gp, pp, goals, expect = case
    got, _ = check(shim, ctx, c, gp, pp, goals)
    for (x, y), want in expect.items():
        assert (int(got[y, x]["cost"]), int(got[y, x]["next"]), int(got[y, x]["flags"])) == want, (x, y)


def test_serpentine_crosses_every_tile_edge(shim, ctx):
    c, gp, pp, goals = pc.serpentine()
    got, st = check(shim, ctx, c, gp, pp, goals)
    start = 32 * 65 + 64
    res, rows = check_paths(shim, ctx, got, gp, [start], 2000)
    n = int(res[0]["length"])
    assert res[0]["status"] == 0 and n > 1000 and rows[0, n - 1] == 0 and res[0]["cost"] == got[32, 64]["cost"] == 20 * (n - 1)
    assert set((rows[0, :n] // 65).tolist()) == set(range(33))            # every corridor and every gap
    assert st["n_rounds"] > 1 and st["n_reached"] == 17 * 65 + 16


def test_unreachable_islands_and_ignored_goals(shim, ctx):
    c = pc.free_grid(40, 20)
    pc.block(c, (slice(None), 20))
    gp, pp = pc.raster(40, 20), pc.plain()
    got, st = check(shim, ctx, c, gp, pp, [5, 20, 20, 3 * 40 + 20])
    assert st["n_goals"] == 4 and st["n_goals_ignored"] == 3
    right = got[:, 21:]
    assert np.all(right["cost"] == INF) and np.all(right["next"] == 255) and np.all(right["flags"] == 2)
    assert np.all(got[:, :20]["flags"] == 6) and st["n_reached"] == 20 * 20
    got, st = check(shim, ctx, c, gp, pp, [20, 60])                       # every goal blocked: SUMA_OK, nothing reached
    assert st["n_goals_ignored"] == 2 and st["n_reached"] == 0 and st["max_cost"] == 0 and np.all(got["cost"] == INF)
    assert np.all(got["next"] == 255) and not np.any(got["flags"] & 4)
    check(shim, ctx, c, gp, pp, np.arange(4096) % 800)                    # the most goals a call takes


def test_ties_take_the_smallest_direction(shim, ctx):
    c, gp = pc.free_grid(70, 70), pc.raster(70, 70)
    got, _ = check(shim, ctx, c, gp, pc.plain(), [33 * 70 + 33])
    assert got[32, 31]["cost"] == 48 and got[32, 31]["next"] == 0
    assert got[33, 60]["next"] == 4 and got[60, 60]["next"] == 5 and got[5, 5]["next"] == 1 and got[33, 33]["next"] == 8


def test_soft_cost_centres_the_path(shim, ctx):
    start = 2 * 40 + 1
    c, gp, pp, goals = pc.soft_corridor(2)
    got, _ = check(shim, ctx, c, gp, pp, goals)
    res, rows = check_paths(shim, ctx, got, gp, [start], 100)
    path = rows[0, :res[0]["length"]]
    assert res[0]["status"] == 0 and np.all((path // 40)[path % 40 >= 4] == 4)
    c, gp, pp, goals = pc.soft_corridor(0)
    got0, _ = check(shim, ctx, c, gp, pp, goals)
    assert got0[2, 1]["cost"] == 2 * 28 + 35 * 20 < got[2, 1]["cost"]


SENTINEL = 0x7fc00001


def raw_call(ctx, gp, pp, cells_t, goals, field_t, drop=None, n_goals=None, cells_off=0, field_off=0):
    """suma_grid_plan_field with raw arguments; `drop` names one to pass as NULL -> (rc, message, stats)"""
    st = PlanStats()
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.int64))
    args = dict(gp=C.byref(gp), pp=C.byref(pp), cells=C.c_void_p(cells_t.data_ptr() + cells_off), goals=g.ctypes.data_as(C.c_void_p),
                field=C.c_void_p(field_t.data_ptr() + field_off), stats=C.byref(st))
    if drop:
        args[drop] = None
    rc = ctx.L.suma_grid_plan_field(ctx.h, args["gp"], args["pp"], args["cells"], args["goals"], len(g) if n_goals is None else n_goals,
                                    args["field"], args["stats"])
    return rc, ctx.L.suma_last_error(ctx.h).decode(), st


BAD = [("pp", "max_clear_cells", 0, "max_clear_cells"), ("pp", "max_clear_cells", 65, "max_clear_cells"),
       ("pp", "soft_cells", 18, "soft_cells"), ("pp", "soft_weight", 256, "soft_weight"), ("pp", "unknown_blocked", 2, "unknown_blocked"),
       ("pp", "max_step", float("nan"), "max_step"), ("pp", "robot_radius", float("nan"), "robot_radius"),
       ("pp", "robot_radius", -0.1, "robot_radius"), ("pp", "robot_radius", float("inf"), "robot_radius"),
       ("pp", "robot_radius", float(np.nextafter(np.float32(4.0), np.float32(5.0))), "robot_radius"),
       ("gp", "cell_size", 0.0, "cell_size"), ("gp", "cell_size", float("nan"), "cell_size"), ("gp", "width", 0, "width"),
       ("gp", "height", 0, "width"), ("gp", "width", 1 << 25, "width"),
       ("drop", "gp", None, "grid parameters"), ("drop", "pp", None, "plan parameters"), ("drop", "cells", None, "cells"),
       ("drop", "goals", None, "goals"), ("drop", "field", None, "field"), ("drop", "stats", None, "stats"),
       ("n_goals", None, 0, "n_goals"), ("n_goals", None, 4097, "n_goals"), ("goal", None, -1, "goal 1"), ("goal", None, 16 * 8, "goal 1"),
       ("cells_off", None, 8, "aligned"), ("field_off", None, 4, "aligned")]


@pytest.mark.parametrize("kind,field,value,needle", BAD, ids=lambda v: str(v))
def test_invalid_calls_launch_nothing(shim, ctx, kind, field, value, needle):
    cells = pc.random_grid(16, 8, 0.1)
    gp, pp = pc.raster(16, 8), PlanParams.defaults()
    cells_t = torch.from_numpy(cells.view(np.int32).reshape(-1).copy()).cuda()
    field_t = torch.full((16 * 8 * 2 + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    goals, kw = [3, 5], {}
    if kind in ("pp", "gp"):
        setattr(pp if kind == "pp" else gp, field, value)
    elif kind == "drop":
        kw["drop"] = field
    elif kind == "n_goals":
        kw["n_goals"] = value
        goals = [3] * 4097
    elif kind == "goal":
        goals = [3, value]
    else:
        kw[kind] = value
    rc, msg, st = raw_call(ctx, gp, pp, cells_t, goals, field_t, **kw)
    assert rc == -1 and needle in msg, (rc, msg)
    ctx.synchronize()
    assert bool(torch.all(field_t == SENTINEL)), "an invalid call wrote the field"
    assert bytes(st) == bytes(PlanStats()) and cells_t.cpu().numpy().tobytes() == cells.tobytes()
    check(shim, ctx, cells, pc.raster(16, 8), PlanParams.defaults(), [3, 5])  # a valid call still works


def test_capacity_bound(shim, ctx):
    gp = pc.raster(257, 129)
    cells = pc.free_grid(257, 129)
    cells_t = torch.from_numpy(cells.view(np.int32).reshape(-1).copy()).cuda()
    field_t = torch.full((257 * 129 * 2,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pp = PlanParams.defaults(max_clear_cells=64, soft_cells=65, soft_weight=255, robot_radius=0.0)   # w_max = 16830
    assert pc.check_params(gp, pp) == -3
    rc, msg, _ = raw_call(ctx, gp, pp, cells_t, [0], field_t)
    assert rc == -3 and "2^32" in msg, (rc, msg)
    ctx.synchronize()
    assert bool(torch.all(field_t == SENTINEL))
    pp.soft_weight = 68                                                    # the smallest weight that trips the bound here
    assert 257 * 129 * 28 * (255 + 67 * 65) < 1 << 32 <= 257 * 129 * 28 * (255 + 68 * 65)
    rc, msg, _ = raw_call(ctx, gp, pp, cells_t, [0], field_t)
    assert rc == -3 and bool(torch.all(field_t == SENTINEL))
    pp.soft_weight = 67
    assert pc.check_params(gp, pp) == 0
    rc, msg, st = raw_call(ctx, gp, pp, cells_t, [0], field_t)
    assert rc == 0 and st.n_reached == 257 * 129


def test_paths(shim, ctx):
    c = pc.random_grid(47, 41, 0.15, bumpy=False)
    gp = pc.raster(47, 41)
    field, st = check(shim, ctx, c, gp, pc.plain(), [0, 46 * 41])
    f = field.reshape(-1)
    goal = 0 if f[0]["cost"] == 0 else 46 * 41
    assert f[goal]["cost"] == 0 and st["n_reached"] > 1000
    unreached = int(np.flatnonzero(f["cost"] == INF)[0])
    far = int(np.argmax(np.where(f["cost"] == INF, 0, f["cost"])))
    res, rows = check_paths(shim, ctx, field, gp, [-1, 47 * 41, unreached, goal, far], 200)
    assert res["status"].tolist() == [2, 2, 1, 0, 0] and res["length"][:4].tolist() == [0, 0, 0, 1] and rows[3, 0] == goal
    n = int(res[4]["length"])
    assert n > 20 and rows[4, 0] == far and rows[4, n - 1] in (0, 46 * 41) and res[4]["cost"] == f[far]["cost"]
    assert np.all(rows[4, n:] == INF) and np.all(rows[:3] == INF)
    # one cell of room too few: TRUNCATED, the full length, the first n - 1 cells
    res2, rows2 = check_paths(shim, ctx, field, gp, [far, goal], n - 1)
    assert res2["status"].tolist() == [3, 0] and res2["length"].tolist() == [n, 1]
    assert np.array_equal(rows2[0], rows[4, :n - 1])
    check_paths(shim, ctx, field, gp, [far], 1)
    # the walk against plain python, and 4096 starts in one call (a device field, nothing uploaded)
    d_field = torch.from_numpy(field.view(np.int32).reshape(-1).copy()).cuda()
    starts = np.arange(4096) % (47 * 41 + 3) - 1
    res, rows = core.grid_paths(ctx, d_field, gp, starts, 30)
    wres, wrows = pc.shim_paths(shim, field, gp, starts, 30)
    assert res.tobytes() == wres.tobytes() and rows.tobytes() == wrows.tobytes() and set(res["status"].tolist()) == {0, 1, 2, 3}
    for s in range(0, 4096, 97):
        n, status, cost, cells = pc.python_walk(field, int(starts[s]), 30)
        assert (int(res[s]["length"]), int(res[s]["status"]), int(res[s]["cost"])) == (n, status, cost)
        assert rows[s, :len(cells)].tolist() == cells
    # invalid calls write nothing
    out_rows, out_res = np.full((2, 5), 7, dtype=np.uint32), np.full(2, 7, dtype=PLAN_PATH_DTYPE)
    s64 = np.array([0, 1], dtype=np.int64)
    for n_starts, cap, ptrs, needle in ((0, 5, {}, "n_starts"), (4097, 5, {}, "n_starts"), (2, 0, {}, "path_capacity"),
                                        (2, (1 << 20) + 1, {}, "path_capacity"), (2, 5, dict(field=None), "field"),
                                        (2, 5, dict(starts=None), "starts"), (2, 5, dict(rows=None), "path_cells"),
                                        (2, 5, dict(res=None), "results"), (2, 5, dict(gp=None), "grid parameters"),
                                        (2, 5, dict(field=C.c_void_p(d_field.data_ptr() + 4)), "aligned")):
        a = dict(gp=C.byref(gp), field=C.c_void_p(d_field.data_ptr()), starts=s64.ctypes.data_as(C.c_void_p),
                 rows=out_rows.ctypes.data_as(C.c_void_p), res=out_res.ctypes.data_as(C.c_void_p))
        a.update(ptrs)
        rc = ctx.L.suma_grid_plan_paths(ctx.h, a["gp"], a["field"], a["starts"], n_starts, cap, a["rows"], a["res"])
        assert rc == -1 and needle in ctx.L.suma_last_error(ctx.h).decode(), (needle, rc, ctx.L.suma_last_error(ctx.h).decode())
        assert np.all(out_rows == 7) and np.all(out_res["length"] == 7)


@pytest.mark.parametrize("lie", ["cycle", "leaves", "cost", "next 9", "next 255 on the way"])
def test_a_lying_field_ends_the_walk(shim, ctx, lie):
    gp = pc.raster(8, 8)
    f, _ = check(shim, ctx, pc.free_grid(8, 8), gp, pc.plain(), [63])
    start = 3 * 8 + 3                                                     # on the diagonal: (3, 3) -> (4, 4) -> ... -> (7, 7)
    assert f[3, 3]["next"] == 1 and f[0, 0]["next"] == 1
    if lie == "cycle":
        f["next"][3, 3], f["next"][3, 4] = 0, 4                           # east, and back west
    elif lie == "leaves":
        f["next"][0, 0], start = 4, 0
    elif lie == "cost":
        f["cost"][4, 4] = f["cost"][3, 3]
    elif lie == "next 9":
        f["next"][4, 4] = 9
    else:
        f["next"][4, 4] = 255
    res, rows = check_paths(shim, ctx, f, gp, [start, 2 * 8 + 2], 20)
    want = {"cycle": 2, "leaves": 1, "cost": 1, "next 9": 2, "next 255 on the way": 2}[lie]
    assert res[0]["status"] == 4 and res[0]["length"] == want and np.all(rows[0, want:] == INF)
    assert res[1]["status"] == (0 if lie == "leaves" else 4)               # (2, 2) walks into the same lie
    assert (int(res[0]["length"]), 4) == pc.python_walk(f, start, 20)[:2]


def test_determinism_and_the_buffers(shim, ctx):
    W, H = 257, 129
    cells, gp, pp = pc.random_grid(W, H, 0.1), pc.raster(W, H), PlanParams.defaults(robot_radius=0.3)
    goals = np.array([5, W * H - 7, W * 64 + 128], dtype=np.int64)
    cells_t = torch.from_numpy(cells.view(np.int32).reshape(-1).copy()).cuda()
    a = torch.full((W * H * 2,), SENTINEL, dtype=torch.int32, device="cuda")
    b = torch.zeros((W * H * 2,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc1, _, st1 = raw_call(ctx, gp, pp, cells_t, goals, a)
    rc2, _, st2 = raw_call(ctx, gp, pp, cells_t, goals, b)
    assert rc1 == rc2 == 0 and bool(torch.equal(a, b)) and st1.as_dict() == st2.as_dict()   # every cell is written
    want, wst = pc.shim_field(shim, cells, gp, pp, goals)
    assert a.cpu().numpy().tobytes() == want.tobytes() and dict(st1.as_dict(), n_rounds=0) == wst
    assert cells_t.cpu().numpy().tobytes() == cells.tobytes()             # the grid is read only
    field, st = core.grid_plan(ctx, cells_t, gp, goals, pp)               # a torch tensor as the device address
    assert field.tobytes() == want.tobytes()
    # a smaller raster after a larger one reuses the scratch
    check(shim, ctx, pc.random_grid(33, 31, 0.1), pc.raster(33, 31), pp, [0, 500])


def test_grid_planner_in_world_coordinates(shim, ctx):
    c, _, pp, _ = pc.soft_corridor(2)
    gp = GridParams.defaults(cell_size=0.5, origin=(-3.0, 10.0), width=40, height=9)
    planner = core.GridPlanner(ctx, c, gp, pp)
    with pytest.raises(core.SumaError):
        planner.path((0.0, 12.0))
    goal_xy, start_xy = (-3.0 + 38.5 * 0.5, 10.0 + 4.5 * 0.5), (-3.0 + 1.2 * 0.5, 10.0 + 2.7 * 0.5)
    st = planner.set_goals([goal_xy])
    want, wst = pc.shim_field(shim, c, gp, pp, [4 * 40 + 38])
    assert planner.field().tobytes() == want.tobytes() and dict(st, n_rounds=0) == wst
    (xy, cost, status), (xy2, cost2, status2) = planner.paths([start_xy, (100.0, 0.0)])
    assert status == 0 and cost == want[2, 1]["cost"] and np.allclose(xy[0], (-3.0 + 1.5 * 0.5, 10.0 + 2.5 * 0.5))
    assert np.allclose(xy[-1], goal_xy) and np.all(np.abs(np.diff(xy, axis=0)) <= 0.5 + 1e-9)
    assert status2 == 2 and len(xy2) == 0 and cost2 == INF
    with pytest.raises(ValueError):
        planner.set_goals([(100.0, 0.0)])
    planner.close()


W_, H_ = 360, 32


def test_no_side_effects_on_a_pipeline(shim):
    p = params_with_size(W_, H_, submap_extent=4.0, submap_dimension=2)
    a, b = core.SurfelMapping(p), core.SurfelMapping(p)
    grid = None
    planned = 0
    for k in range(30):
        sc = ls.scan(k, W_, H_)
        a.processScan(*sc, fixed_iterations=6)
        b.processScan(*sc, fixed_iterations=6)
        if k % 5 == 4:
            cells, gp, _ = b.map.export_grid(cell_size=0.5)
            if grid is None:
                grid = (cells.copy(), gp, b.ctx.device_array(cells))      # a grid kept on the device through later scans
            d_cells = grid[2]
            free = np.flatnonzero(cells.reshape(-1)["state"] == 1)
            field, st = core.grid_plan(b.ctx, cells, gp, free[[len(free) // 3, len(free) // 2]], robot_radius=0.0, unknown_blocked=False)
            core.grid_plan(b.ctx, d_cells, grid[1], [0], robot_radius=0.0)
            res, _ = core.grid_paths(b.ctx, field, gp, np.arange(0, field.size, 11))
            planned += st["n_reached"] + int((res["status"] == 0).sum())
        assert np.array_equal(a.getCurrentPose(), b.getCurrentPose()), k
    assert planned > 60
    n = grid[0].nbytes
    assert b.ctx.device_download(grid[2], n).tobytes() == grid[0].tobytes()    # a grid made before is unchanged
    b.ctx.device_free(grid[2])
    assert a.map.getAllSurfels().tobytes() == b.map.getAllSurfels().tobytes()
    assert a.map.poses().tobytes() == b.map.poses().tobytes()
    assert a.map.counts() == b.map.counts() and a.map.cache_stats() == b.map.cache_stats()
    assert a.map.cached_tiles() == b.map.cached_tiles()
    for ij in a.map.cached_tiles():
        assert a.map.cached_tile(*ij).tobytes() == b.map.cached_tile(*ij).tobytes()


def test_plan_on_a_pipelines_grid_equals_the_shim(shim):
    p = params_with_size(W_, H_, submap_extent=4.0, submap_dimension=2)
    pipe = core.SurfelMapping(p)
    for k in range(12):
        pipe.processScan(*ls.scan(k, W_, H_), fixed_iterations=6)
    cells, gp, gst = pipe.map.export_grid(cell_size=0.25, fit_margin=1, fill_radius=3)
    assert cells.dtype == GRID_CELL_DTYPE and gst["n_free"] > 100
    free = np.flatnonzero(cells.reshape(-1)["state"] == 1)
    for pp in (PlanParams.defaults(robot_radius=0.25), PlanParams.defaults(robot_radius=0.0, unknown_blocked=False, max_step=0.05)):
        field, st = check(shim, pipe.ctx, cells, gp, pp, free[[0, len(free) // 2]])
        assert st["n_reached"] > 50
        check_paths(shim, pipe.ctx, field, gp, free[::17], gp.width + gp.height)


def test_plan_path_tool(tmp_path):
    """tools/plan_path.py end to end on a crafted grid file: the stats, a path, the plan file and the picture"""
    import json
    import os
    import subprocess
    import sys
    from semantic_suma_amd import mapio
    from test_gpu_cpp import ROOT
    c, gp, pp, goals = pc.soft_corridor(2)
    grid, plan, png = str(tmp_path / "c.grid.npz"), str(tmp_path / "c.plan.npz"), str(tmp_path / "c.plan.png")
    mapio.write_grid(grid, c, gp)
    line = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "plan_path.py"), grid, "--goal", "9.6", "1.1",
                                    "--start", "0.3", "0.6", "--start", "-5", "0", "--robot-radius", "0", "--max-clear-cells", "8",
                                    "--soft-cells", "4", "--out", plan, "--png", png], timeout=120).decode().strip().splitlines()[-1]
    res = json.loads(line)
    field, gp2, pp2 = mapio.read_plan(plan)
    want, _ = core.grid_plan(core.Context(params_with_size(900, 64)), c, gp, goals, pp)
    assert field.tobytes() == want.tobytes() and bytes(gp2) == bytes(gp) and bytes(pp2) == bytes(pp)
    assert res["stats"]["n_reached"] == 7 * 40 and res["goal_cells"] == goals
    assert [p["status"] for p in res["paths"]] == ["OK", "START_OUTSIDE"] and res["paths"][0]["cost"] == int(want[2, 1]["cost"])
    # north (10 * (5 + 3)), north-east onto the centre line (14 * (3 + 1)), 36 cells east at 20: cheaper than two diagonals
    assert res["paths"][0]["cost"] == 80 + 56 + 36 * 20
    assert res["paths"][0]["length"] == 39 and {"plan_classify", "plan_clearance", "plan_relax", "plan_next", "plan_walk"} <= set(res["kernels_us"])
    assert open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
