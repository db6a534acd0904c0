"""suma_hip::SurfelMap::exportGrid (include/suma_adapter.hpp) in a C++ host on the MI355X: tests/cpp/grid_driver.cpp grids
a crafted map and must print the raster, the stats and the digest of the cells that SurfelMap.export_grid gives in Python
-- which in turn equal the host restatement (tests/grid_shim.c) on the world export's records."""
import os
import subprocess

import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import draw_common as dc
import grid_common as gc
from semantic_suma_amd import core
from semantic_suma_amd.types import params_with_size
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_adapter_export_grid(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "grid_driver.cpp"), "c++")
    shim = gc.build_shim(tmp_path)
    s, poses = dc.planar_map(5000)
    s.tofile(str(tmp_path / "surfels.bin"))
    dc.cm_poses(poses).tofile(str(tmp_path / "poses.bin"))
    smap = core.SurfelMap(core.Context(params_with_size(900)))
    smap.upload(s, int(len(poses)))
    smap.updatePoses(poses)
    for cell_size, margin in ((0.5, 1), (0.2, 0)):
        line = subprocess.check_output([exe, str(tmp_path / "surfels.bin"), str(tmp_path / "poses.bin"), str(cell_size),
                                        str(margin)], timeout=120).decode().split()
        cells, gp, st = smap.export_grid(cell_size=cell_size, fit_margin=margin)
        want, wst = gc.shim_grid(shim, smap.export_world(), gp)
        assert st == wst and cells.tobytes() == want.tobytes() and st["n_occupied"] > 1000
        assert line == [str(gp.width), str(gp.height)] + [str(v) for v in st.values()] + [f"{fnv(cells.tobytes()):016x}"], line
