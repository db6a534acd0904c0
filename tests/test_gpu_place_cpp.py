"""suma_hip::PlaceIndex and suma_hip::Localizer::relocalize (include/suma_adapter.hpp) in a C++ host on the MI355X:
tests/cpp/place_driver.cpp queries an index read from files and relocalises a scan in a map read from a file, and must
print the matches and the pose bits that core.PlaceIndex and core.Localizer.relocalize return."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import localize_common as lc
import place_common as pc
from semantic_suma_amd import core
from semantic_suma_amd.types import PlaceParams
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu
N, QUERY, K = 14, 7, 3


def hexpose(fields):
    return np.array([int(x, 16) for x in fields], dtype=np.uint64).view(np.float64).reshape(4, 4).T


def test_cpp_adapter_place_index_and_relocalize(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "place_driver.cpp"), "c++")
    p = lc.loc_params()
    pp = PlaceParams.defaults(max_range=50.0)
    scans = lc.loc_scans(N)
    pipe = core.SurfelMapping(p)
    index = core.PlaceIndex(pp)
    poses, all_poses = [], []
    for k, s in enumerate(scans):
        pipe.processScan(*s)
        all_poses.append(pipe.getCurrentPose())
        if k % 2 == 0:
            index.addFrame(pipe.ctx, pipe.frame(0), k)
            poses.append(all_poses[-1])
    records = pipe.map.export_world()
    pipe.close()
    cells, _, ids = index.download()
    poses = np.stack(poses)
    query = pc.turned_scan(scans[QUERY], pc.turn_angle(7, pp.sectors))
    records.tofile(str(tmp_path / "map.bin"))
    cells.astype("<f4").tofile(str(tmp_path / "cells.bin"))
    ids.astype("<u4").tofile(str(tmp_path / "ids.bin"))
    np.ascontiguousarray(poses.transpose(0, 2, 1), dtype="<f8").tofile(str(tmp_path / "poses.bin"))
    for a, ext in zip(query, ("bin", "label", "prob")):
        np.ascontiguousarray(a, dtype="<f4").tofile(str(tmp_path / f"query.{ext}"))
    out = subprocess.check_output([exe] + [str(tmp_path / f) for f in ("map.bin", "cells.bin", "ids.bin", "poses.bin", "query")] +
                                  [str(lc.LOC_W), str(lc.LOC_H), str(p.submap_extent), str(p.submap_dimension), "50.0", str(K)],
                                  timeout=120).decode().strip().splitlines()
    # the Python path on the same inputs
    loc = core.Localizer(p)
    loc.setMap(records)
    frame = core.Frame(loc.ctx, p.data_width, p.data_height)
    core.Preprocessing(loc.ctx).process(query[0], frame, query[1], query[2], p.active_timestamps + 10)
    want = index.queryFrame(loc.ctx, frame, K)
    assert int(out[0]) == len(want) == K
    got = [dict(index=int(f[0]), id=int(f[1]), distance=np.array(int(f[2], 16), dtype=np.uint32).view(np.float32),
                shift=int(f[3]), yaw=np.array(int(f[4], 16), dtype=np.uint32).view(np.float32))
           for f in (line.split() for line in out[1:1 + K])]
    pc.matches_equal(got, want)
    assert want[0]["id"] in (QUERY - 1, QUERY + 1) and want[0]["shift"] == pp.sectors - 7
    own = out[1 + K].split()
    assert (int(own[0]), int(own[1]), int(own[3])) == (len(ids), 4242, 0) and int(own[5]) == len(ids) + 1
    assert np.array(int(own[2], 16), dtype=np.uint32).view(np.float32) < 1e-6
    assert int(own[4]) == want[0]["index"]
    rel = loc.relocalize(index, poses, *query, max_candidates=K)
    assert out[2 + K].split() == [str(int(rel["found"])), str(rel["n_tried"]), str(rel["winner"])] and rel["found"]
    for c, line in zip(rel["candidates"], out[3 + K:3 + K + rel["n_tried"]]):
        f = line.split()
        assert (int(f[0]), int(f[1])) == (c["match"]["index"], int(c["result"]["tracked"]))
        assert hexpose(f[2:]).tobytes() == c["result"]["pose"].tobytes()
    assert hexpose(out[3 + K + rel["n_tried"]].split()).tobytes() == rel["result"]["pose"].tobytes()
    assert not lc.tracking_failures([rel["result"]["pose"]] * (QUERY + 1), all_poses, first=QUERY)[0]
    loc.close()
    index.close()

