#!/usr/bin/env python3
"""Plan on a traversability grid file: the clearance and cost-to-go field towards a goal, and the paths from one or more
starts (core.GridPlanner on one MI355X; csrc/k_plan.hip states the rules).

    python tools/plan_path.py map.grid.npz --goal X Y --start X Y [--start X Y ...] [--robot-radius 0.4] [--max-step 0.15]
                              [--max-rough R] [--unknown-free] [--max-clear-cells 16] [--soft-cells 3] [--soft-weight 2]
                              [--out map.plan.npz] [--png map.plan.png] [--repeat 3] [--compare-host]

map.grid.npz is what tools/export_map.py --grid writes (mapio.write_grid); goal and starts are world coordinates.  Prints
one JSON line: the stats, each path's status, length and cost, the wall time of core.grid_plan on cells already on the
device (first and later calls) and the device-event time of every stage.  --out writes the field with both parameter
structs (mapio.write_plan); --png a picture of the cell states, shaded by clearance, with the paths in blue, the goal in
black; --compare-host also times the host restatement tests/plan_shim.c on the same grid and compares the bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from semantic_suma_amd import core, mapio  # noqa: E402
from semantic_suma_amd.types import PATH_STATUS_NAMES, PLAN_CELL_DTYPE, PlanParams, params_with_size  # noqa: E402

STATE_RGB = np.array([[255, 255, 255], [60, 170, 80], [200, 40, 40], [128, 128, 128]], np.float32)


def picture(cells, field, pp, paths, goal_cells):
    """RGBA [height, width]: the cell states; a traversable cell is shaded by its clearance (dark near what it must not
    touch), a free cell the robot does not fit on is pale; paths blue, goals black.  Row 0 is the greatest y."""
    rgb = STATE_RGB[np.minimum(cells["state"], 3)]
    cap = float((pp.max_clear_cells + 1) ** 2)
    shade = 0.55 + 0.45 * np.sqrt(field["clear2"] / cap)
    trav = (field["flags"] & 2) != 0
    rgb = np.where(trav[..., None], rgb * shade[..., None], rgb)
    pale = (cells["state"] == 1) & ~trav
    rgb = np.where(pale[..., None], 0.5 * rgb + 127.0, rgb)
    flat = rgb.reshape(-1, 3)
    for p in paths:
        flat[p] = (30, 60, 220)
    flat[goal_cells] = (0, 0, 0)
    out = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255.0, np.float32)], -1).astype(np.uint8)
    return out[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("grid", help="a grid file of tools/export_map.py --grid")
    ap.add_argument("--goal", nargs=2, type=float, action="append", required=True, metavar=("X", "Y"))
    ap.add_argument("--start", nargs=2, type=float, action="append", required=True, metavar=("X", "Y"))
    ap.add_argument("--robot-radius", type=float, default=0.4)
    ap.add_argument("--max-step", type=float, default=0.15)
    ap.add_argument("--max-rough", type=float, default=float("nan"))
    ap.add_argument("--unknown-free", action="store_true", help="UNKNOWN cells are not blocked")
    ap.add_argument("--max-clear-cells", type=int, default=16)
    ap.add_argument("--soft-cells", type=int, default=3)
    ap.add_argument("--soft-weight", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=None, help="cells of room per path (default width + height)")
    ap.add_argument("--out", default=None, help="write the field (.npz, mapio.write_plan)")
    ap.add_argument("--png", default=None, help="a picture of states, clearance and paths")
    ap.add_argument("--repeat", type=int, default=3, help="timed calls (the first one allocates the scratch)")
    ap.add_argument("--compare-host", action="store_true", help="also run and time tests/plan_shim.c on the host")
    args = ap.parse_args()

    cells, gp = mapio.read_grid(args.grid)
    pp = PlanParams.defaults(robot_radius=args.robot_radius, max_step=args.max_step, max_rough=args.max_rough,
                             unknown_blocked=not args.unknown_free, max_clear_cells=args.max_clear_cells,
                             soft_cells=args.soft_cells, soft_weight=args.soft_weight)
    ctx = core.Context(params_with_size(900, 64))
    planner = core.GridPlanner(ctx, cells, gp, pp)
    goal_cells = [planner.cell(g) for g in args.goal]
    res = dict(grid=args.grid, grid_size=[gp.width, gp.height], cell_size=gp.cell_size, goal_cells=goal_cells,
               plan_params={k: (None if isinstance(v, float) and v != v else v) for k, v in pp.as_dict().items()})
    wall = []
    for rep in range(max(1, args.repeat)):  # the last run with the ctx's kernel timers on
        last = rep == max(1, args.repeat) - 1
        ctx.profile(last)
        ctx.profile_reset()
        t = time.perf_counter()
        stats = planner.set_goals(args.goal)
        wall.append(round(1e3 * (time.perf_counter() - t), 3))
        if last:
            t = time.perf_counter()
            results, rows = core.grid_paths(ctx, planner._field, gp, [planner.cell(s) for s in args.start], args.capacity)
            res["paths_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
            res["kernels_us"] = {k["name"]: round(1e3 * k["total_ms"], 1) for k in ctx.profile_get() if k["name"].startswith("plan_")}
    ctx.profile(0)
    res.update(stats=stats, plan_wall_ms=wall)
    paths = []
    res["paths"] = []
    for s, r, row in zip(args.start, results, rows):
        n = min(int(r["length"]), row.shape[0])
        paths.append(row[:n])
        res["paths"].append(dict(start=s, status=PATH_STATUS_NAMES[int(r["status"])], length=int(r["length"]), cost=int(r["cost"]),
                                 metres=round(float(np.linalg.norm(np.diff(planner.centre(row[:n]), axis=0), axis=1).sum()), 2)))
    field = planner.field()
    if args.out:
        mapio.write_plan(args.out, field, gp, pp)
    if args.png:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from draw_map import write_png
        write_png(args.png, picture(cells, field, pp, paths, goal_cells))
    if args.compare_host:
        import tempfile
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import plan_common as pc
        with tempfile.TemporaryDirectory() as tmp:
            shim = pc.build_shim(tmp)
            t = time.perf_counter()
            want, wst = pc.shim_field(shim, cells, gp, pp, goal_cells)
            res["host_shim_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
        res["equals_host_shim"] = bool(want.tobytes() == field.tobytes() and dict(stats, n_rounds=0) == wst)
    assert field.dtype == PLAN_CELL_DTYPE
    print(json.dumps(res))


if __name__ == "__main__":
    main()
