"""suma_map_export_world on the MI355X (csrc/k_world.hip, core.SurfelMap.export_world): records and stats byte for byte
against the host restatement (tests/world_shim.c) -- sizes around every boundary, run extremes, ties, edge inputs, parked
tiles before and after a pose update, no side effects on a pipeline, capacity, validation, determinism."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import draw_common as dc
import loop_scenario as ls
import world_common as wc
from semantic_suma_amd import core
from semantic_suma_amd.types import WORLD_SURFEL_DTYPE, WorldParams, WorldStats, params_with_size

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return wc.build_shim(tmp_path_factory.mktemp("world_gpu"))


@pytest.fixture(scope="module")
def smap():
    return core.SurfelMap(core.Context(params_with_size(900, 64)))


def load(smap, s, poses):
    smap.upload(s, int(len(poses)))
    smap.updatePoses(poses)


def check(shim, smap, src, poses, where="", n_active=None, n_tiles=0, **kw):
    """the export equals the shim's on (src, poses): records and every stat; returns (records, stats)"""
    got, st = smap.export_world(stats=True, **kw)
    want, wst, _ = wc.shim_export(shim, src, poses, smap.ctx.params.max_poses, **kw)
    n_active = len(src) if n_active is None else n_active
    assert st == dict(n_active=n_active, n_tiles=n_tiles, n_parked=len(src) - n_active, **wst), (where, kw, st, wst)
    assert got.dtype == WORLD_SURFEL_DTYPE and got.tobytes() == want.tobytes(), (where, kw)
    return got, st


@pytest.mark.parametrize("voxel", [0.0, 0.25, 1.0, 8.0])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_sizes_around_every_boundary(shim, smap, n, voxel):
    s, poses = dc.planar_map(n)
    load(smap, s, poses)
    got, st = check(shim, smap, s, poses, voxel_size=voxel, min_confidence=0.0)
    assert st["n_passed"] == int((s["confidence"] > 0).sum()) and (n < 63 or 0 < st["n_out"] <= st["n_passed"])
    if voxel > 0 and n:
        assert int(got["support"].sum()) == st["n_passed"] - st["n_dropped"]


def test_run_extremes(shim, smap):
    s, poses = dc.planar_map(3000)
    load(smap, s, poses)
    got, st = check(shim, smap, s, poses, voxel_size=1000.0)  # one voxel per sign octant at most; all in a few runs
    assert st["n_out"] <= 8 and int(got["support"].sum()) == 3000 and got["support"].max() > 256
    s["x"], s["y"], s["z"] = 1000.0 + 0.01 * np.arange(3000), 2.0, 3.0  # every point in one voxel: a run of 3000
    s["count"] = 0.0  # pose 0 of planar_map is the identity
    load(smap, s, poses)
    got, st = check(shim, smap, s, poses, voxel_size=1000.0)
    assert st["n_out"] == 1 and got["support"][0] == 3000
    s["x"] = 0.01 * np.arange(3000) - 15.0  # 10 voxels apart: every run has length 1
    load(smap, s, poses)
    got, st = check(shim, smap, s, poses, voxel_size=1e-3)
    assert st["n_out"] == 3000 and np.all(got["support"] == 1)


def test_ties(shim, smap):
    s, poses = dc.planar_map(400)
    twin = s.copy()
    twin["radius"] = 9.0  # the same place and confidence, later in the source sequence: never the representative
    both = np.concatenate([s, twin])
    load(smap, both, poses)
    got, _ = check(shim, smap, both, poses, voxel_size=1.0)
    assert np.all(got["radius"] < 1.0) and np.all(got["support"] % 2 == 0)
    # two labels with equal vote sums: the smaller id; all weights 0: the representative's label, prob 0
    t = s[:4].copy()
    t["x"], t["y"], t["z"], t["count"] = [0.1, 0.2, 50.1, 50.2], 0.1, 0.1, 0.0
    t["r"] = t["g"] = t["b"] = (np.array([40, 10, 40, 10]) / 255.0).astype(np.float32)
    t["w"] = [0.5, 0.5, 0.0, 0.0]
    t["confidence"] = [1.0, 2.0, 1.0, 2.0]
    load(smap, t, poses)
    got, st = check(shim, smap, t, poses, voxel_size=1.0)
    assert st["n_out"] == 2
    assert (got["label"][0], got["prob"][0], got["support"][0]) == (10, 0.5, 2)
    assert (got["label"][1], got["prob"][1], got["confidence"][1]) == (10, 0.0, 2.0)
    t["confidence"] = [1.0, 2.0, 3.0, 2.0]
    load(smap, t, poses)
    got, _ = check(shim, smap, t, poses, voxel_size=1.0)
    assert (got["label"][1], got["prob"][1]) == (40, 0.0)


def edge_map():
    s, poses = dc.planar_map(1000)
    poses = np.concatenate([poses, poses[:2]])
    poses[4, 0, 3] = np.inf   # a pose with an infinite entry
    poses[5, 1, 1] = np.nan   # and one with a NaN
    e = s[:16].copy()
    e["count"][0:2] = [4.0, 5.0]
    e["x"][2], e["y"][3], e["z"][4] = np.nan, np.inf, -np.inf
    e["count"][5:9] = [-3.0, 1e9, np.nan, 10000.0]          # clamped as draw does: 0, max_poses - 1, 0, max_poses - 1
    e["x"][9], e["y"][9], e["z"][9] = -0.5, -7.25, -0.001    # negative coordinates: floorf, not truncation
    e["count"][9] = 0.0
    e["x"][10], e["count"][10] = 3.0e5, 0.0                  # |i| >= 2^20 at voxel 0.25
    e["x"][11], e["count"][11] = -262144.0, 0.0              # i = -2^20 exactly at voxel 0.25: dropped; -2^20 + 1 stays
    e["x"][12], e["count"][12] = -262143.75, 0.0                # i = -2^20 + 1
    e["confidence"][13] = np.nan
    e["r"][14], e["r"][15] = 2.0, np.nan
    e["w"][15] = np.nan
    return np.concatenate([s[:500], e, s[500:]]), poses


@pytest.mark.parametrize("voxel", [0.0, 0.25, 8.0])
def test_edge_inputs(shim, smap, voxel):
    s, poses = edge_map()
    load(smap, s, poses)
    got, st = check(shim, smap, s, poses, voxel_size=voxel)
    assert st["n_passed"] == len(s) - 1                    # the NaN confidence never passes
    assert st["n_dropped"] == (7 if voxel == 0.25 else 5)  # 2 poses + 3 positions; + the two beyond the grid
    # dropping the majority label of the voxels changes their vote, not the other members
    labels = wc.labels_of(s)
    major = int(np.bincount(labels).argmax())
    got2, st2 = check(shim, smap, s, poses, voxel_size=voxel, keep_labels=[l for l in range(260) if l != major])
    assert st2["n_passed"] == st["n_passed"] - int((labels[np.isfinite(s["confidence"])] == major).sum())
    assert not np.any(got2["label"] == major)
    check(shim, smap, s, poses, voxel_size=voxel, min_confidence=float("inf"))


@pytest.fixture(scope="module")
def circle():
    """the closed circle of loop_scenario at 360 x 32 with small submap tiles: most of the map is parked"""
    W, H = 360, 32
    p = params_with_size(W, H, submap_extent=4.0, submap_dimension=2)
    pipe = core.SurfelMapping(p)
    for k in range(ls.lap_scans() + 40):
        pipe.processScan(*ls.scan(k, W, H), fixed_iterations=6)
    return pipe


def test_parked_tiles(shim, circle):
    m = circle.map
    tiles = m.cached_tiles()
    assert tiles == sorted(tiles) and len(set(tiles)) == len(tiles)
    src, tiles2, parked = wc.source_sequence(m)
    active = m.size()
    assert tiles2 == tiles and len(tiles) >= 3 and parked >= 0.2 * len(src), (len(tiles), parked, len(src))
    assert m.counts()[2] == parked
    poses = m.poses()
    for voxel in (0.0, 0.5):
        got, st = check(shim, m, src, poses, "circle", n_active=active, n_tiles=len(tiles), voxel_size=voxel)
        assert st["n_out"] > 1000
    # a window of tiles around the origin that were never parked, or are empty, are not listed
    assert all(m.cached_tile(i, j).shape[0] > 0 for i, j in tiles)
    before = m.export_world(voxel_size=0.5)
    m.updatePoses(np.array([ls.small_motion(k) @ poses[k] for k in range(len(poses))]))
    poses2 = m.poses()
    assert not np.array_equal(poses2, poses)
    for voxel in (0.0, 0.5):
        got, _ = check(shim, m, src, poses2, "nudged", n_active=active, n_tiles=len(tiles), voxel_size=voxel)
    assert got.tobytes() != before.tobytes()
    m.updatePoses(poses)
    assert m.export_world(voxel_size=0.5).tobytes() == before.tobytes()


def test_no_side_effects_on_a_pipeline():
    W, H = 360, 32
    p = params_with_size(W, H, submap_extent=4.0, submap_dimension=2)
    a, b = core.SurfelMapping(p), core.SurfelMapping(p)
    exported = 0
    for k in range(30):
        sc = ls.scan(k, W, H)
        a.processScan(*sc, fixed_iterations=6)
        b.processScan(*sc, fixed_iterations=6)
        if k % 5 == 4:
            exported += len(b.map.export_world()) + len(b.map.export_world(voxel_size=0.5, min_confidence=0.0))
        assert np.array_equal(a.getCurrentPose(), b.getCurrentPose()), k
    assert exported > 10000
    assert a.map.getAllSurfels().tobytes() == b.map.getAllSurfels().tobytes()
    assert a.map.poses().tobytes() == b.map.poses().tobytes()
    assert a.map.counts() == b.map.counts() and a.map.cache_stats() == b.map.cache_stats()
    assert a.map.cached_tiles() == b.map.cached_tiles()
    for ij in a.map.cached_tiles():
        assert a.map.cached_tile(*ij).tobytes() == b.map.cached_tile(*ij).tobytes()


@pytest.mark.parametrize("voxel", [0.0, 1.0])
def test_capacity_and_determinism(shim, smap, voxel):
    s, poses = dc.planar_map(5000)
    load(smap, s, poses)
    wp = WorldParams.defaults(voxel, 0.0)
    full, st = smap.export_world(voxel_size=voxel, min_confidence=0.0, stats=True)
    again = smap.export_world(voxel_size=voxel, min_confidence=0.0)
    assert full.tobytes() == again.tobytes() and st["n_out"] == len(full) > 100
    size = smap.export_world_device(wp, None, 0)  # d_out = NULL, capacity = 0: the size
    assert size.as_dict() == st
    half = st["n_out"] // 2
    buf = torch.full((st["n_out"] * 12,), 0x7fc00001, dtype=torch.int32, device="cuda")
    st2 = smap.export_world_device(wp, buf, half)
    assert st2.as_dict() == st
    host = buf.cpu().numpy().view(WORLD_SURFEL_DTYPE)
    assert host[:half].tobytes() == full[:half].tobytes()
    assert np.all(buf.cpu().numpy()[half * 12:] == 0x7fc00001)  # nothing behind the capacity is written


BAD = [("voxel_size", -1.0, "voxel_size"), ("voxel_size", float("nan"), "voxel_size"),
       ("voxel_size", float("inf"), "voxel_size"), ("min_confidence", float("nan"), "min_confidence")]


@pytest.mark.parametrize("field,value,needle", BAD + [("wp", None, "parameters"), ("stats", None, "stats")])
def test_invalid_parameters_are_rejected(shim, smap, field, value, needle):
    s, poses = dc.planar_map(1000)
    load(smap, s, poses)
    ctx = smap.ctx
    wp, st = WorldParams.defaults(), WorldStats()
    a_wp, a_st = C.byref(wp), C.byref(st)
    if field == "wp":
        a_wp = None
    elif field == "stats":
        a_st = None
    else:
        setattr(wp, field, value)
    rc = ctx.L.suma_map_export_world(ctx.h, a_wp, None, 0, a_st)
    msg = ctx.L.suma_last_error(ctx.h).decode()
    assert rc == -1 and msg and needle in msg, (rc, msg)
    if field not in ("wp", "stats"):
        with pytest.raises(core.SumaError, match=needle):
            smap.export_world_device(wp, None, 0)
    check(shim, smap, s, poses, voxel_size=1.0)  # a valid call still works


def test_a_null_buffer_with_a_capacity_is_rejected(smap):
    ctx = smap.ctx
    wp, st = WorldParams.defaults(), WorldStats()
    rc = ctx.L.suma_map_export_world(ctx.h, C.byref(wp), None, 16, C.byref(st))
    assert rc == -1 and "output buffer" in ctx.L.suma_last_error(ctx.h).decode()


def test_export_repeats_once_when_the_guess_is_too_small(shim):
    """core.export_world starts from 65536 records: a larger map makes it run a second time, a smaller one does not"""
    m = core.SurfelMap(core.Context(params_with_size(900, 64)))
    s, poses = dc.planar_map(70000)
    load(m, s, poses)
    got, st = check(shim, m, s, poses)
    assert st["n_out"] == 70000 and m._world_capacity == 87500
    check(shim, m, s, poses, voxel_size=1.0)


def test_export_map_tool(tmp_path):
    """tools/export_map.py end to end on three small scans: the PLY it writes holds the records its stats count"""
    import json
    import os
    import subprocess
    import sys
    from semantic_suma_amd import mapio
    from test_gpu_cpp import ROOT
    out = str(tmp_path / "map.ply")
    line = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "export_map.py"), "--out", out, "--scans", "3",
                                    "--width", "360", "--voxel", "0.2", "--repeat", "1", "--compare"],
                                   timeout=120).decode().strip().splitlines()[-1]
    res = json.loads(line)
    ws, rgb = mapio.read_ply(out)
    st = res["stats"]
    assert len(ws) == st["n_out"] > 100 and int(ws["support"].sum()) == st["n_passed"] - st["n_dropped"]
    assert res["host_route_points"] == st["n_active"] + st["n_parked"]


def test_cpp_adapter_export_world(shim, tmp_path):
    """suma_hip::SurfelMap::exportWorld in a C++ host: the checksum of its records is the shim's"""
    import os
    import subprocess
    from test_gpu_cpp import ROOT, build
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "world_driver.cpp"), "c++")
    s, poses = dc.planar_map(5000)
    s.tofile(str(tmp_path / "surfels.bin"))
    dc.cm_poses(poses).tofile(str(tmp_path / "poses.bin"))
    for voxel in (0.0, 0.5):
        line = subprocess.check_output([exe, str(tmp_path / "surfels.bin"), str(tmp_path / "poses.bin"), str(voxel)],
                                       timeout=120).decode().split()
        want, st, _ = wc.shim_export(shim, s, poses, params_with_size(900).max_poses, voxel_size=voxel)
        h = 1469598103934665603
        for b in want.tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        assert line == [str(st["n_out"]), str(st["n_passed"]), str(st["n_dropped"]), "0", f"{h:016x}"], (voxel, line)
