"""suma_hip::Localizer (include/suma_adapter.hpp) in a C++ host on the MI355X: tests/cpp/localize_driver.cpp localises
scans read from files in a map read from a file and must print the pose bits, gates and window of core.Localizer."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import localize_common as lc
from semantic_suma_amd import core
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu
N = 14  # crosses the first tile edge (x > 11 m)


def test_cpp_adapter_localizer(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "localize_driver.cpp"), "c++")
    p = lc.loc_params()
    scans = lc.loc_scans(N)
    pipe = core.SurfelMapping(p)
    for s in scans:
        pipe.processScan(*s)
    records = np.concatenate([pipe.map.export_world(), lc.edge_records(p.submap_extent)[-12:]])
    pipe.close()
    start = lc.perturbed(np.eye(4), 0.1, -0.05, 1.0)
    d = tmp_path / "scans"
    d.mkdir()
    for k, (pts, lab, prob) in enumerate(scans):
        for a, ext in ((pts, "bin"), (lab, "label"), (prob, "prob")):
            np.ascontiguousarray(a, dtype="<f4").tofile(str(d / f"{k:06d}.{ext}"))
    records.tofile(str(tmp_path / "map.bin"))
    np.ascontiguousarray(start.T, dtype="<f8").tofile(str(tmp_path / "start.bin"))
    out = subprocess.check_output([exe, str(tmp_path / "map.bin"), str(tmp_path / "start.bin"), str(d), str(N),
                                   str(lc.LOC_W), str(lc.LOC_H), str(p.submap_extent), str(p.submap_dimension)],
                                  timeout=120).decode().strip().splitlines()
    assert len(out) == N + 1
    loc = core.Localizer(p)
    dropped = loc.setMap(records)
    loc.setPose(start)
    moved = 0
    for k, s in enumerate(scans):
        r = loc.processScan(*s)
        f = out[k].split()
        bits = np.array([int(x, 16) for x in f[:16]], dtype=np.uint64).view(np.float64).reshape(4, 4).T
        assert bits.tobytes() == r["pose"].tobytes(), k
        assert [int(x) for x in f[16:]] == [int(r["tracked"]), int(r["window_rebuilt"]), r["n_window"], *r["origin"]], k
        moved += r["window_rebuilt"]
    h = 1469598103934665603
    for b in loc.downloadWindow().tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert out[N].split() == [str(dropped), str(loc.window()[2]), f"{h:016x}"], out[N]
    assert dropped == 8 and moved >= 1
    loc.close()
