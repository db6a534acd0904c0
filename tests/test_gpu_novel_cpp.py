"""The collection of newly seen surfaces of suma_hip::Localizer (include/suma_adapter.hpp) in a C++ host on the MI355X:
tests/cpp/novel_driver.cpp collects the crafted frame over the crafted map and must print the counts, the sizes and the
digest of updatedMap that core.Localizer gives, with evidence on and off."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import change_common as cc
import localize_common as lc
import novel_common as nc
from semantic_suma_amd import core
from semantic_suma_amd.types import NOVEL_COUNTS
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_adapter_updated_map(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "novel_driver.cpp"), "c++")
    lshim, cshim, nshim = lc.build_shim(tmp_path), cc.build_shim(tmp_path), nc.build_shim(tmp_path)
    case = nc.crafted_case(lshim, cshim, nshim, 257)
    rec, p, npar = case["records"], case["params"], case["np"]
    T = cc.crafted_pose(turned=True)
    rec.tofile(str(tmp_path / "map.bin"))
    np.ascontiguousarray(T.T, dtype="<f8").tofile(str(tmp_path / "pose.bin"))
    np.concatenate([np.ascontiguousarray(a, dtype="<f4").reshape(-1) for a in case["maps"]]).tofile(str(tmp_path / "frame.bin"))
    for evidence in (0, 1):
        out = subprocess.check_output([exe, str(tmp_path / "map.bin"), str(tmp_path / "pose.bin"), str(tmp_path / "frame.bin"),
                                       str(cc.CW), str(cc.CH), str(p.submap_extent), str(p.submap_dimension),
                                       str(npar.max_range), str(p.max_angle), str(evidence)],
                                      timeout=120).decode().strip().splitlines()
        q = nc.crafted_params()
        from semantic_suma_amd.types import default_params
        q.map_max_distance = default_params().map_max_distance   # the driver starts from suma_params_default
        loc = core.Localizer(q)
        loc.enableNovelty(npar)
        if evidence:
            loc.enableEvidence()
        loc.setMap(rec)
        loc.setPose(T)
        frame = core.Frame(loc.ctx, cc.CW, cc.CH)
        frame.set(*case["maps"])
        for _ in range(3 * evidence):                                 # the default rule removes nothing below three misses
            loc.observeFrame(frame, T)
        loc.collectFrame(frame, T, 0)
        cnt = loc.collectFrame(frame, T, 1)
        cand, fused, upd = loc.novelCandidates(), loc.novel()[0], loc.updatedMap(rec)
        assert [int(x) for x in out[0].split()] == [cnt[k] for k in NOVEL_COUNTS], (evidence, out[0], cnt)
        assert out[1].split() == [str(len(cand)), str(len(fused)), str(len(upd)), f"{fnv(upd.tobytes()):016x}"], (evidence, out[1])
        assert len(fused) > 50 and len(cand) == 2 * cnt["novel"]      # two collections of one frame: every voxel has two views
        assert (len(upd) < len(rec) + len(fused)) == bool(evidence)   # the rule prunes only with evidence
        loc.close()
