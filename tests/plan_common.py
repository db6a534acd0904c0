"""Shared by the planner's tests (test_abi_plan.py, test_plan_host.py, test_gpu_plan.py, test_gpu_plan_cpp.py): the host
restatement tests/plan_shim.c, grids crafted directly as GRID_CELL_DTYPE arrays, and the entry's parameter checks."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd.types import (GRID_CELL_DTYPE, GRID_FREE, GRID_OBSTACLE, GRID_UNKNOWN, PLAN_CELL_DTYPE, PLAN_PATH_DTYPE,
                                     GridParams, PlanParams, PlanStats)

HERE = os.path.dirname(os.path.abspath(__file__))
INF = 0xffffffff
TILE = 32  # PLAN_TILE of semantic_suma_amd/csrc/suma_internal.h: the relaxation's tile (test_abi_plan.py compares them)
SHIM_FLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off"]


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "plan_shim.so")
    subprocess.check_call(["gcc"] + SHIM_FLAGS + ["-fPIC", "-shared", os.path.join(HERE, "plan_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.plan_shim_field.argtypes = [C.POINTER(GridParams), C.POINTER(PlanParams), vp, vp, u32, vp, C.POINTER(PlanStats)]
    L.plan_shim_paths.argtypes = [C.POINTER(GridParams), vp, vp, u32, u32, vp, vp]
    L.plan_shim_paths.restype = None
    L.plan_shim_sizeof.argtypes = [C.c_int]
    L.plan_shim_sizeof.restype = u32
    return L


def shim_field(shim, cells, gp, pp, goals):
    """-> (PLAN_CELL_DTYPE field [height, width], stats dict; n_rounds is 0) of the shim"""
    c = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(-1)
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.int64).reshape(-1))
    assert c.shape[0] == gp.width * gp.height and g.size and g.min() >= 0 and g.max() < c.shape[0]
    field = np.zeros((gp.height, gp.width), dtype=PLAN_CELL_DTYPE)
    st = PlanStats()
    rc = shim.plan_shim_field(C.byref(gp), C.byref(pp), c.ctypes.data, g.ctypes.data, g.shape[0], field.ctypes.data, C.byref(st))
    assert rc == 0, rc
    return field, st.as_dict()


def shim_paths(shim, field, gp, starts, capacity):
    f = np.ascontiguousarray(field, dtype=PLAN_CELL_DTYPE).reshape(-1)
    s = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
    res = np.zeros(s.shape[0], dtype=PLAN_PATH_DTYPE)
    rows = np.zeros((s.shape[0], capacity), dtype=np.uint32)
    shim.plan_shim_paths(C.byref(gp), f.ctypes.data, s.ctypes.data, s.shape[0], capacity, rows.ctypes.data, res.ctypes.data)
    return res, rows


def raster(width, height, cell_size=0.25, origin=(0.0, 0.0)):
    return GridParams.defaults(cell_size=cell_size, origin=origin, width=width, height=height)


def free_grid(width, height, ground_z=0.0, label=40):
    """[height, width] cells, all FREE on flat ground, as suma_world_grid writes a cell with one ground member"""
    c = np.zeros((height, width), dtype=GRID_CELL_DTYPE)
    for f in ("z_min", "z_max", "ground_z"):
        c[f] = ground_z
    c["ground_rough"], c["obstacle_z"], c["prob"] = 0.0, np.nan, 1.0
    c["label"], c["support"], c["n_ground"], c["state"], c["ground_source"] = label, 1, 1, GRID_FREE, 1
    return c


def block(c, where, state=GRID_OBSTACLE):
    """cells of ``c`` (an index expression) become ``state`` cells the way the grid writes them"""
    c["state"][where] = state
    if state == GRID_UNKNOWN:
        c["support"][where], c["n_ground"][where], c["ground_source"][where] = 0, 0, 0
        for f in ("ground_z", "ground_rough", "z_min", "z_max"):
            c[f][where] = np.nan
    return c


def random_grid(width, height, density, seed=3, bumpy=True):
    """a FREE grid with a share ``density`` of OBSTACLE / NO_GROUND / UNKNOWN cells; ground heights on a dyadic lattice of
    1/16 m around a default max_step, a few NaN, a few filled UNKNOWN cells, labels with a spread of costs"""
    rng = np.random.default_rng(seed + 1000 * width + height)
    c = free_grid(width, height)
    if bumpy:
        c["ground_z"] = rng.integers(0, 3, (height, width)) / 16.0
        c["ground_z"][rng.random((height, width)) < 0.01] = np.nan
    c["ground_rough"] = rng.integers(0, 5, (height, width)) / 32.0
    c["ground_rough"][rng.random((height, width)) < 0.05] = np.nan
    c["label"] = rng.choice([40, 48, 72, 300], (height, width))
    kind = rng.choice([GRID_OBSTACLE, 3, GRID_UNKNOWN], (height, width))
    hit = rng.random((height, width)) < density
    c["state"] = np.where(hit, kind, GRID_FREE)
    filled = (c["state"] == GRID_UNKNOWN) & (rng.random((height, width)) < 0.5)
    c["ground_source"][filled] = 2
    return c


def plain(**kw):
    """parameters under which every cell that is not blocked is traversable and costs 1: one-cell clearance window, a
    point robot, no soft cost"""
    d = dict(robot_radius=0.0, max_clear_cells=1, soft_cells=0, soft_weight=0)
    d.update(kw)
    return PlanParams.defaults(**d)


def numpy_clear2(blocked, R):
    """clear2 by brute force over ALL blocked cells (no window): [height, width] int64"""
    H, W = blocked.shape
    by, bx = np.nonzero(blocked)
    out = np.full((H, W), (R + 1) ** 2, dtype=np.int64)
    if len(bx):
        iy, ix = np.mgrid[0:H, 0:W]
        for lo in range(0, len(bx), 256):   # in slabs: the matrix is cells x blocked cells
            d2 = (ix[..., None] - bx[lo:lo + 256]) ** 2 + (iy[..., None] - by[lo:lo + 256]) ** 2
            out = np.minimum(out, d2.min(-1))
    return out


def probe_scene(R, corner):
    """one blocked cell in an otherwise free raster (cells, gp, pp, goals, the blocked cell): in a raster corner, or at
    (63, 15), the last column and row of the clearance kernels' 64-column and 16-row blocks and one short of the relaxation
    tile's second edge (k_plan.hip: PLAN_ROW_W, PLAN_COL_H, PLAN_TILE), so that the probes towards +x and +y lie across
    those edges"""
    if corner:
        W, H, at = R + 4, R + 3, (0, 0)
    else:
        W, H, at = 64 + R + 4, 16 + R + 3, (63, 15)
    c = free_grid(W, H)
    block(c, (at[1], at[0]))
    pp = PlanParams.defaults(max_clear_cells=R, robot_radius=0.0, soft_cells=min(3, R + 1))
    return c, raster(W, H), pp, [W * H - 1], at


def serpentine(width=65, height=33):
    """walls on every second row with one gap at alternating ends: the only way from the last row to the goal in the
    corner (0, 0) runs through every corridor"""
    c = free_grid(width, height)
    for y in range(1, height, 2):
        block(c, (y, slice(None)))
        c["state"][y, width - 1 if (y // 2) % 2 == 0 else 0] = GRID_FREE
    return c, raster(width, height), plain(), [0]


def edge_cases():
    """(name, cells, gp, pp, goals, {(x, y): (cost, next, flags)}) -- the rules of the edges, each on a raster of a few cells"""
    out = []
    ms = np.float32(0.15)
    up = np.nextafter(ms, np.float32(np.inf))
    c = free_grid(3, 1)
    c["ground_z"][0] = [ms, 0.0, -up]           # |dz| exactly max_step on the left, one ulp above it on the right
    out.append(("step", c, raster(3, 1), plain(), [1], {(0, 0): (20, 0, 6), (1, 0): (0, 8, 6), (2, 0): (INF, 255, 2)}))
    c = free_grid(3, 1)
    c["ground_z"][0, 2] = np.nan                # a NaN on one side forbids the move; the cell is still traversable
    out.append(("nan ground", c, raster(3, 1), plain(), [1], {(0, 0): (20, 0, 6), (2, 0): (INF, 255, 2)}))
    out.append(("nan ground at a goal", c, raster(3, 1), plain(), [2], {(0, 0): (INF, 255, 2), (1, 0): (INF, 255, 2), (2, 0): (0, 8, 6)}))
    for n_blocked, want in ((0, (28, 5, 6)), (1, (40, 6, 6)), (2, (INF, 255, 2))):
        c = free_grid(2, 2)                     # goal (0, 0), probe (1, 1): the diagonal passes between (1, 0) and (0, 1)
        if n_blocked >= 1:
            block(c, (1, 0))                    # cell (0, 1)
        if n_blocked == 2:
            block(c, (0, 1))                    # cell (1, 0)
        out.append((f"diagonal between {n_blocked} blocked", c, raster(2, 2), plain(), [0], {(1, 1): want, (0, 0): (0, 8, 6)}))
    c = free_grid(3, 1, label=48)
    c["label"][0, 2] = 72                       # FREE, but its label is forbidden
    c["label"][0, 0] = 300                      # reads as label 0
    pp = plain(label_cost={48: 3, 72: 0, 0: 5})
    out.append(("label cost", c, raster(3, 1), pp, [1], {(0, 0): (80, 0, 6), (1, 0): (0, 8, 6), (2, 0): (INF, 255, 1)}))
    c = free_grid(4, 1)
    c["ground_rough"][0] = [0.25, 0.0, np.nextafter(np.float32(0.25), np.float32(1.0)), np.nan]
    out.append(("max_rough", c, raster(4, 1), plain(max_rough=0.25), [1],
                {(0, 0): (20, 0, 6), (2, 0): (INF, 255, 1), (3, 0): (INF, 255, 2)}))
    out.append(("max_rough off", c, raster(4, 1), plain(), [1], {(2, 0): (20, 4, 6), (3, 0): (40, 4, 6)}))
    for ub in (0, 1):
        c = free_grid(4, 1)
        block(c, (0, 2), GRID_UNKNOWN)          # UNKNOWN with ground filled from a neighbour
        c["ground_z"][0, 2], c["ground_source"][0, 2] = 0.0, 2
        block(c, (0, 3), GRID_UNKNOWN)          # UNKNOWN without ground
        out.append((f"unknown_blocked {ub}", c, raster(4, 1), plain(unknown_blocked=bool(ub)), [1],
                    {(2, 0): (INF, 255, 1) if ub else (20, 4, 6), (3, 0): (INF, 255, 1) if ub else (INF, 255, 2)}))
    return out


def soft_corridor(soft_weight):
    """a corridor seven cells wide between two walls: with the soft cost its centre line (row 4) is the cheapest"""
    c = free_grid(40, 9)
    block(c, (0, slice(None)))
    block(c, (8, slice(None)))
    pp = PlanParams.defaults(robot_radius=0.0, max_clear_cells=8, soft_cells=4, soft_weight=soft_weight)
    return c, raster(40, 9), pp, [4 * 40 + 38]


def python_walk(field, start, capacity):
    """the walk of the specification in plain python: (length, status, cost, the recorded cells)"""
    H, W = field.shape
    f = field.reshape(-1)
    if not 0 <= start < W * H:
        return 0, 2, INF, []
    cost = int(f[start]["cost"])
    if f[start]["next"] == 255:
        return 0, 1, cost, []
    from semantic_suma_amd.types import PLAN_DIRECTIONS
    c, cells, status = int(start), [int(start)], 4
    for _ in range(W * H):
        k = int(f[c]["next"])
        if k == 8:
            status = 0
            break
        if k > 7:
            break
        x, y = c % W + PLAN_DIRECTIONS[k][0], c // W + PLAN_DIRECTIONS[k][1]
        if not (0 <= x < W and 0 <= y < H) or not f[y * W + x]["cost"] < f[c]["cost"]:
            break
        c = y * W + x
        cells.append(c)
    if status == 0 and len(cells) > capacity:
        status = 3
    return len(cells), status, cost, cells[:capacity]


def check_params(gp, pp):
    """the entry's verdict on (gp, pp) as the header states it: 0, -1 (invalid) or -3 (capacity)"""
    R = pp.max_clear_cells
    if not (1 <= R <= 64 and pp.soft_cells <= R + 1 and pp.soft_weight <= 255 and pp.unknown_blocked <= 1):
        return -1
    if np.isnan(pp.max_step) or not (np.isfinite(pp.robot_radius) and 0 <= pp.robot_radius <= np.float32(R) * np.float32(gp.cell_size)):
        return -1
    if gp.width * gp.height * 28 * (255 + pp.soft_weight * pp.soft_cells) >= 1 << 32:
        return -3
    return 0


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h
