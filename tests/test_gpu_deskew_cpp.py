"""suma_hip::SurfelMapping::enableDeskew (include/suma_adapter.hpp) in a C++ host on the MI355X: tests/cpp/deskew_driver.cpp
runs ten raw sweeps read from files with the correction on and one override, and must print the pose bits and the motion
sources of core.SurfelMapping."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import deskew_common as dc
from semantic_suma_amd import core
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu
N, K_OVERRIDE = 10, 5


def test_cpp_adapter_deskew(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "deskew_driver.cpp"), "c++")
    d = tmp_path / "scans"
    d.mkdir()
    for k in range(N):
        for a, ext in zip(dc.raw_scan(k), ("bin", "label", "prob")):
            np.ascontiguousarray(a, dtype="<f4").tofile(str(d / f"{k:06d}.{ext}"))
    motion = dc.true_motion(K_OVERRIDE)
    np.ascontiguousarray(motion.T, dtype="<f8").tofile(str(tmp_path / "motion.bin"))
    out = subprocess.check_output([exe, str(d), str(N), str(dc.W), str(dc.H), str(K_OVERRIDE), str(tmp_path / "motion.bin")],
                                  timeout=120).decode().strip().splitlines()
    assert len(out) == N
    pipe = core.SurfelMapping(dc.params())
    pipe.enableDeskew()
    sources = []
    for k in range(N):
        if k == K_OVERRIDE:
            pipe.setDeskewMotion(motion)
        pipe.processScan(*dc.raw_scan(k))
        f = out[k].split()
        bits = np.array([int(x, 16) for x in f[:16]], dtype=np.uint64).view(np.float64).reshape(4, 4).T
        assert bits.tobytes() == pipe.getCurrentPose().tobytes(), k
        m, source = pipe.deskewMotion()
        assert int(f[16]) == source and int(f[17], 16) == int(np.float64(m[0, 3]).view(np.uint64)), k
        sources.append(source)
    assert sources[K_OVERRIDE] == 2 and sources.count(1) == N - 1
    pipe.close()
