"""suma_hip::planField / planPaths (include/suma_adapter.hpp) in a C++ host on the MI355X: tests/cpp/plan_driver.cpp plans
on a crafted grid and must print the stats and the digests of the field and the paths that core.grid_plan and
core.grid_paths give in Python -- which in turn equal the host restatement (tests/plan_shim.c)."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import plan_common as pc
from semantic_suma_amd import core
from semantic_suma_amd.types import PlanParams, params_with_size
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def test_cpp_adapter_plan(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "plan_driver.cpp"), "c++")
    shim = pc.build_shim(tmp_path)
    ctx = core.Context(params_with_size(900))
    for (W, H), density, radius, cap in (((70, 45), 0.05, 0.25, 30), ((33, 64), 0.2, 0.0, 100)):
        cells, gp = pc.random_grid(W, H, density), pc.raster(W, H)
        cells.tofile(str(tmp_path / "cells.bin"))
        free = np.flatnonzero(cells.reshape(-1)["state"] == 1)
        goal, starts = int(free[len(free) // 2]), [-1, W * H] + [int(s) for s in free[::97]]
        line = subprocess.check_output([exe, str(tmp_path / "cells.bin"), str(W), str(H), "0.25", str(radius), str(cap), str(goal)] +
                                       [str(s) for s in starts], timeout=120).decode().split()
        pp = PlanParams.defaults(robot_radius=radius)
        field, st = core.grid_plan(ctx, cells, gp, [goal], pp)
        res, rows = core.grid_paths(ctx, field, gp, starts, cap)
        want, wst = pc.shim_field(shim, cells, gp, pp, [goal])
        wres, wrows = pc.shim_paths(shim, want, gp, starts, cap)
        assert field.tobytes() == want.tobytes() and dict(st, n_rounds=0) == wst and st["n_reached"] > 100
        assert res.tobytes() == wres.tobytes() and rows.tobytes() == wrows.tobytes() and 0 in res["status"]
        assert line == [str(v) for k, v in st.items() if k != "n_rounds"] + \
            [f"{pc.fnv(a.tobytes()):016x}" for a in (field, res, rows)], line
