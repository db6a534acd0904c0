"""The live obstacle layer of suma_hip::Localizer (include/suma_adapter.hpp) in a C++ host on the MI355X:
tests/cpp/live_driver.cpp updates a layer over crafted cells with a crafted frame twice, composes, and must print the
counts, the stats and the digests of the composed cells and of the mask that the host restatement (tests/live_shim.c) and
core.Localizer give."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import live_common as lv
from semantic_suma_amd import core
from semantic_suma_amd.types import GRID_CELL_DTYPE, LIVE_COUNTS, LIVE_STATS, NovelParams, params_with_size
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_adapter_live_grid(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "live_driver.cpp"), "c++")
    shim = lv.build_shim(tmp_path)
    W, H = 130, 4
    gp, cells, lp, steps = lv.random_sequence(W, H, 65, 33, seed=8)
    V, fl, T, _ = steps[0]
    np.concatenate([np.ascontiguousarray(a, dtype="<f4").reshape(-1) for a in (V, np.zeros_like(V), np.zeros_like(V))]).tofile(
        str(tmp_path / "frame.bin"))
    fl.tofile(str(tmp_path / "flags.bin"))
    np.ascontiguousarray(np.asarray(T, dtype="<f8").T).tofile(str(tmp_path / "pose.bin"))
    np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).tofile(str(tmp_path / "cells.bin"))
    args = [W, H, gp.width, gp.height, repr(gp.cell_size), repr(gp.origin_x), repr(gp.origin_y), repr(gp.step_height),
            repr(gp.clearance), lp.hold_scans, lp.min_hits, repr(lp.carve_range), repr(lp.carve_margin)]
    out = subprocess.check_output([exe] + [str(tmp_path / n) for n in ("frame.bin", "flags.bin", "pose.bin", "cells.bin")] +
                                  [str(a) for a in args], timeout=120).decode().strip().splitlines()
    want = lv.ShimLayer(shim, cells, gp, lp)
    want.update(V, fl, T, 0)
    counts = want.update(V, fl, T, 1)
    comp, mask, st = want.compose()
    assert st["n_live"] > 5 and counts["n_hit_cells"] > 5, (st, counts)
    assert [int(x) for x in out[0].split()] == [counts[k] for k in LIVE_COUNTS], (out[0], counts)
    assert [int(x) for x in out[1].split()] == [st[k] for k in LIVE_STATS], (out[1], st)
    assert out[2].split() == [f"{fnv(comp.tobytes()):016x}", f"{fnv(mask.tobytes()):016x}"], out[2]
    loc = core.Localizer(params_with_size(W, H))
    loc.enableNovelty(NovelParams.defaults(max_candidates=1024))
    loc.enableLiveGrid(cells, gp, lp)
    frame = core.Frame(loc.ctx, W, H)
    frame.set(V, np.zeros_like(V), np.zeros_like(V))
    loc.liveUpdateFlags(frame, T, fl, 0)
    assert loc.liveUpdateFlags(frame, T, fl, 1) == counts
    got = loc.liveCells()
    assert got[0].tobytes() == comp.tobytes() and got[1].tobytes() == mask.tobytes() and got[2] == st
    loc.close()
