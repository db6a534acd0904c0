"""C-ABI checks of the planner that need no GPU: the header's new symbols are exported, the ctypes mirrors and the numpy
cells have the C layouts (the shim's too), the defaults are as the header states, suma_grid_cell_index is the grid's own
cell expression."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_common as gc
import plan_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_plan_params_default", "suma_grid_cell_index", "suma_grid_plan_field", "suma_grid_plan_paths"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from semantic_suma_amd import core
    return core


def test_new_symbols_are_declared_and_exported(built):
    L = C.CDLL(built.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "suma_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(L, name), name
        assert hasattr(built.lib(), name) and getattr(built.lib(), name).argtypes is not None, name
    assert "0 E (1, 0), 1 NE (1, 1), 2 N (0, 1), 3 NW (-1, 1), 4 W (-1, 0), 5 SW (-1, -1), 6 S (0, -1), 7 SE (1, -1)" in header
    for f in ("k_plan.hip", "suma_plan.hip"):
        assert f in open(os.path.join(ROOT, "semantic_suma_amd", "csrc", "Makefile")).read()


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd import types
    from semantic_suma_amd.types import PLAN_CELL_DTYPE, PLAN_PATH_DTYPE, PlanParams, PlanStats
    structs = {"suma_plan_params": PlanParams, "suma_plan_stats": PlanStats}
    dtypes = {"suma_plan_cell": PLAN_CELL_DTYPE, "suma_plan_path": PLAN_PATH_DTYPE}
    body = []
    for cname, T in dtypes.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f in T.names]
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    consts = ["SUMA_PLAN_E", "SUMA_PLAN_NE", "SUMA_PLAN_N", "SUMA_PLAN_NW", "SUMA_PLAN_W", "SUMA_PLAN_SW", "SUMA_PLAN_S",
              "SUMA_PLAN_SE", "SUMA_PLAN_AT_GOAL", "SUMA_PLAN_NO_DIRECTION", "SUMA_PLAN_BLOCKED", "SUMA_PLAN_TRAVERSABLE",
              "SUMA_PLAN_REACHED", "SUMA_PATH_OK", "SUMA_PATH_UNREACHED", "SUMA_PATH_START_OUTSIDE", "SUMA_PATH_TRUNCATED",
              "SUMA_PATH_BAD_FIELD", "SUMA_PLAN_MAX_CLEAR_CELLS", "SUMA_PLAN_MAX_GOALS", "SUMA_PLAN_MAX_STARTS"]
    body += [f'printf("%u\\n", (unsigned){k});' for k in consts]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for T in dtypes.values():
        want += [T.itemsize] + [T.fields[f][1] for f in T.names]
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    want += list(range(8)) + [types.PLAN_AT_GOAL, types.PLAN_NO_DIRECTION, types.PLAN_BLOCKED, types.PLAN_TRAVERSABLE,
                              types.PLAN_REACHED, types.PATH_OK, types.PATH_UNREACHED, types.PATH_START_OUTSIDE,
                              types.PATH_TRUNCATED, types.PATH_BAD_FIELD, types.PLAN_MAX_CLEAR_CELLS, types.PLAN_MAX_GOALS,
                              types.PLAN_MAX_STARTS]
    assert v == want
    assert PLAN_CELL_DTYPE.itemsize == 8 and PLAN_PATH_DTYPE.itemsize == 16 and C.sizeof(PlanStats) == 28
    assert C.sizeof(PlanParams) == 28 + 260
    assert len(types.PATH_STATUS_NAMES) == 5 and len(types.PLAN_DIRECTIONS) == 8
    # the shim declares the structures again: the same sizes
    shim = pc.build_shim(tmp_path)
    assert [shim.plan_shim_sizeof(k) for k in range(4)] == [C.sizeof(PlanParams), 8, C.sizeof(PlanStats), 16]
    # the tile the tests place their edges at is the kernels'
    internal = open(os.path.join(ROOT, "semantic_suma_amd", "csrc", "suma_internal.h")).read()
    assert int(re.search(r"#define PLAN_TILE (\d+)u", internal).group(1)) == pc.TILE


def test_defaults(built):
    from semantic_suma_amd.types import PlanParams
    p = PlanParams(robot_radius=3.0, max_step=1.0, max_rough=2.0, unknown_blocked=0, max_clear_cells=5, soft_cells=1, soft_weight=9)
    p.label_cost[10] = 7
    built.lib().suma_plan_params_default(C.byref(p))
    f32 = lambda v: C.c_float(v).value  # noqa: E731
    assert (p.robot_radius, p.max_step) == (f32(0.4), f32(0.15)) and np.isnan(p.max_rough)
    assert (p.unknown_blocked, p.max_clear_cells, p.soft_cells, p.soft_weight) == (1, 16, 3, 2)
    assert list(p.label_cost) == [1] * 260
    assert bytes(p) == bytes(PlanParams.defaults())
    q = PlanParams.defaults(robot_radius=0.5, max_rough=0.25, unknown_blocked=False, max_clear_cells=4, soft_cells=0, soft_weight=0,
                            label_cost={48: 3, 72: 0})
    assert (q.robot_radius, q.max_rough, q.unknown_blocked, q.max_clear_cells, q.soft_cells, q.soft_weight) == (0.5, 0.25, 0, 4, 0, 0)
    assert q.as_dict()["label_cost"] == {48: 3, 72: 0}
    with pytest.raises(ValueError):
        PlanParams.defaults(label_cost=[1] * 259)


@pytest.mark.parametrize("gp", [gc.params(6, 4, 0.25, origin=(-1.0, -0.5)), gc.params(257, 129, 0.0703125, origin=(-1.03, -1.01)),
                                gc.params(1, 1, 32.0, origin=(-8.0, -16.0)), gc.params(2335, 255, 0.2, origin=(-30.2, -25.4))])
def test_cell_index_is_the_grids_own(built, gp):
    from semantic_suma_amd.types import WORLD_SURFEL_DTYPE
    k = np.arange(-2, max(gp.width, gp.height) + 3)
    xs = np.concatenate([np.float32(gp.origin_x) + k.astype(np.float32) * np.float32(gp.cell_size)] * 3)
    xs[len(k):2 * len(k)] = np.nextafter(xs[:len(k)], np.float32(-np.inf))     # an ulp below and above every edge
    xs[2 * len(k):] = np.nextafter(xs[:len(k)], np.float32(np.inf))
    ys = (xs - np.float32(gp.origin_x) + np.float32(gp.origin_y)).astype(np.float32)
    rng = np.random.default_rng(1)
    x = np.concatenate([xs, rng.permutation(xs), [np.nan, np.inf, -np.inf, 0.0, 0.0]]).astype(np.float32)
    y = np.concatenate([ys, ys, [0.0, 0.0, 0.0, np.nan, np.inf]]).astype(np.float32)
    rec = np.zeros(len(x), dtype=WORLD_SURFEL_DTYPE)
    rec["x"], rec["y"] = x, y
    want = gc.cell_of(rec, gp)                                               # -2 dropped, -1 outside
    got = np.array([built.grid_cell_index(gp, a, b) for a, b in zip(x, y)])
    assert np.array_equal(got, np.maximum(want, -1))
    assert (got >= 0).sum() > 0 and (got == -1).sum() > 5
    assert built.lib().suma_grid_cell_index(None, 0.0, 0.0) == -1
