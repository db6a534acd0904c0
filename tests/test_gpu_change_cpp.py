"""The change evidence of suma_hip::Localizer (include/suma_adapter.hpp) in a C++ host on the MI355X:
tests/cpp/change_driver.cpp localises the edited run's scans read from files with evidence on and must print the totals
of every scan and the evidence digest of core.Localizer."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import change_common as cc
import localize_common as lc
from semantic_suma_amd import core
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def test_cpp_adapter_change_evidence(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "change_driver.cpp"), "c++")
    p = lc.loc_params()
    pipe = core.SurfelMapping(p)
    poses = []
    for s in lc.loc_scans():
        pipe.processScan(*s)
        poses.append(pipe.getCurrentPose())
    records = pipe.map.export_world()
    pipe.close()
    scans, start = cc.edited_scans(), poses[cc.FIRST]
    d = tmp_path / "scans"
    d.mkdir()
    for k, (pts, lab, prob) in enumerate(scans):
        for a, ext in ((pts, "bin"), (lab, "label"), (prob, "prob")):
            np.ascontiguousarray(a, dtype="<f4").tofile(str(d / f"{k:06d}.{ext}"))
    records.tofile(str(tmp_path / "map.bin"))
    np.ascontiguousarray(start.T, dtype="<f8").tofile(str(tmp_path / "start.bin"))
    out = subprocess.check_output([exe, str(tmp_path / "map.bin"), str(tmp_path / "start.bin"), str(d), str(len(scans)),
                                   str(lc.LOC_W), str(lc.LOC_H), str(p.submap_extent), str(p.submap_dimension)],
                                  timeout=120).decode().strip().splitlines()
    assert len(out) == len(scans) + 1
    loc = core.Localizer(p)
    loc.enableEvidence()
    loc.setMap(records)
    loc.setPose(start)
    order = cc.CATEGORIES + ("label_changes",)
    for k, s in enumerate(scans):
        loc.processScan(*s)
        cnt, observed = loc.lastObservation()
        assert [int(x) for x in out[k].split()] == [int(observed)] + [cnt[f] for f in order], k
        assert observed and cnt["hits"] > 1000
    ev = loc.evidence()
    h = 1469598103934665603
    for b in ev.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    kept, keep = loc.prunedMap(records)
    assert out[-1].split() == [str(len(records)), f"{h:016x}", str(int((~keep).sum())), str(len(kept))], out[-1]
    assert 0 < int((~keep).sum()) < len(records) // 10
    loc.close()
