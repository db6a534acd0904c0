"""The per-scan objects of suma_hip::Localizer (include/suma_adapter.hpp) in a C++ host on the MI355X:
tests/cpp/objects_driver.cpp segments a crafted frame and must print the counts, the number of records and the digests of
the records and of the id image that the host restatement (tests/object_shim.c) and core.Localizer give."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import object_common as oc
from semantic_suma_amd import core
from semantic_suma_amd.types import NovelParams, OBJECT_COUNTS, ObjectParams, params_with_size
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_adapter_objects(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "objects_driver.cpp"), "c++")
    shim = oc.build_shim(tmp_path)
    W, H = 130, 4
    V, S = oc.loop_frame(W, H)
    rng = np.random.RandomState(4)
    fl = (rng.rand(H, W) < 0.45).astype(np.uint8)
    op = ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=2, max_objects=4096)
    np.concatenate([np.ascontiguousarray(a, dtype="<f4").reshape(-1) for a in (V, np.zeros_like(V), S)]).tofile(
        str(tmp_path / "frame.bin"))
    fl.tofile(str(tmp_path / "flags.bin"))
    np.ascontiguousarray(oc.POSE.T, dtype="<f8").tofile(str(tmp_path / "pose.bin"))
    out = subprocess.check_output([exe, str(tmp_path / "frame.bin"), str(tmp_path / "flags.bin"), str(tmp_path / "pose.bin"),
                                   str(W), str(H), str(op.link_base), str(op.link_slope), str(op.min_texels),
                                   str(op.max_objects)], timeout=120).decode().strip().splitlines()
    want = oc.shim_segment(shim, V, S, fl, oc.POSE, op, 7)
    assert want[2]["n_objects"] > 5 and want[2]["n_small"] > 0
    assert [int(x) for x in out[0].split()] == [want[2][k] for k in OBJECT_COUNTS], (out[0], want[2])
    assert out[1].split() == [str(len(want[0])), f"{fnv(want[0].tobytes()):016x}", f"{fnv(want[1].tobytes()):016x}"], out[1]
    loc = core.Localizer(params_with_size(W, H))
    loc.enableNovelty(NovelParams.defaults(max_candidates=1024))
    loc.enableObjects(op)
    frame = core.Frame(loc.ctx, W, H)
    frame.set(V, np.zeros_like(V), S)
    assert loc.segmentFlags(frame, oc.POSE, fl, 7) == want[2]
    assert loc.objects()[0].tobytes() == want[0].tobytes() and loc.objectIds().tobytes() == want[1].tobytes()
    loc.close()
