"""Pipeline checkpoint on the MI355X (suma_pipeline_checkpoint_save / _load, csrc/k_checkpoint.hip, suma_checkpoint.hip):
a resumed run is the uninterrupted run to the bit -- with parked tiles coming back into the map, with loop closing at
four kinds of save point --, the image is canonical, crafted images exercise the kernels at their boundaries, refused
loads leave the pipeline untouched, a pipeline that saves computes what one that never does computes, and the C example
and the C++ adapter stop and resume a run over scan files."""
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

from conftest import get_scan
import loop_closing_host as lh
import loop_scenario as ls
from semantic_suma_amd import checkpoint as ck
from semantic_suma_amd import core
from semantic_suma_amd.types import SURFEL_DTYPE, LoopParams, params_with_size

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, ITER = 360, 32, 6


def circle_params(**over):
    return params_with_size(W, H, submap_extent=4.0, submap_dimension=2, **over)


def state(p):
    m = p.map
    tiles = m.cached_tiles()
    return dict(surfels=m.getAllSurfels().tobytes(), poses=m.poses().tobytes(), counts=m.counts(), tiles=tiles,
                tile_data=[m.cached_tile(i, j).tobytes() for i, j in tiles],
                frame=[p.frame(0).download(w).tobytes() for w in range(3)],
                pose0=p.getPose(0).tobytes(), pose1=p.getPose(1).tobytes(), track_loss=p.trackLoss(),
                timestamp=p.timestamp())


def assert_same_state(a, b, where):
    for k in a:
        assert a[k] == b[k], (where, k)


def step(p, k):
    p.processScan(*ls.scan(k, W, H), fixed_iterations=ITER)
    return p.getCurrentPose().tobytes(), bytes(p.lastStats())


@pytest.fixture(scope="module")
def circle():
    """run A, uninterrupted, with its images after scan M (twice); run B to K, its image and state; C = B resumed and
    run to the end, with its state right after the load, its trace, its image after scan M and the pipeline itself.
    Everything is computed here, once; the tests only read."""
    N = ls.lap_scans() + 40
    a = core.SurfelMapping(circle_params())
    trace, K, M, img_m = [], None, None, None
    for k in range(N):
        trace.append(step(a, k))
        if K is None and k >= 40 and len(a.map.cached_tiles()) >= 3:
            K, M = k, k + 20
        if k == M:
            img_m = (a.save(), a.save())
    assert K is not None and K <= N - 30, K
    b = core.SurfelMapping(circle_params())
    for k in range(K + 1):
        assert step(b, k) == trace[k], k
    img_k = b.save()
    saved = state(b)
    parked = b.map.counts()[2]
    b.close()
    c = core.SurfelMapping(circle_params())
    c.load(img_k)
    loaded = state(c)  # before any scan
    c_trace, c_img_m = {}, None
    for k in range(K + 1, N):
        c_trace[k] = step(c, k)
        if k == M:
            c_img_m = c.save()
    return dict(N=N, K=K, M=M, trace=trace, img_k=img_k, img_m=img_m, saved=saved, parked=parked, loaded=loaded,
                c_trace=c_trace, c_img_m=c_img_m, a_final=state(a), c_final=state(c))


def test_resume_with_parked_tiles(circle):
    K, N = circle["K"], circle["N"]
    info = core.checkpoint_info(circle["img_k"])
    assert info["n_parked"] == circle["parked"] > 0 and info["n_tiles"] >= 3 and info["timestamp"] == K + 1
    assert not info["has_loop"] and not info["has_opt"]
    assert_same_state(circle["saved"], circle["loaded"], "right after the load")
    for k in range(K + 1, N):
        assert circle["c_trace"][k] == circle["trace"][k], k
    assert_same_state(circle["a_final"], circle["c_final"], "at the end")
    # the lap closed after the save point: a tile that was parked at K has come back into the map since -- it is no
    # longer parked, or it has been parked again with other records
    at_k = dict(zip(circle["saved"]["tiles"], circle["saved"]["tile_data"]))
    at_end = dict(zip(circle["c_final"]["tiles"], circle["c_final"]["tile_data"]))
    assert len(at_k) >= 3 and any(at_end.get(ij) != data for ij, data in at_k.items())


def test_canonical_bytes(circle):
    first, second = circle["img_m"]
    assert first == second and len(first) % 64 == 0
    assert circle["c_img_m"] == first  # the resumed pipeline after scan M: the same bytes as the uninterrupted one's
    assert ck.verify(first) == []


# ---- loop closing ----
LW, LH = 900, 64


def loop_params(**over):
    return LoopParams.defaults(**dict(lh.SCENARIO, min_valid_ratio=ls.MIN_VALID_RATIO, optimize_wait=1, **over))


def loop_step(sm, k):
    sm.processScan(*lh.scenario_scan(k, LW, LH), fixed_iterations=8)
    return sm.loopStatus().as_dict()


def loop_final(sm):
    g = sm.posegraph
    return dict(pose=sm.getCurrentPose().tobytes(), pose_old=sm.getPose(1).tobytes(), table=sm.map.poses().tobytes(),
                surfels=sm.map.getAllSurfels().tobytes(), traj=sm.trajectoryDistances().tobytes(),
                graph=g.poses().tobytes(), edges=[(a, b, Z.tobytes(), I.tobytes()) for a, b, Z, I in g.edges()])


@pytest.fixture(scope="module")
def loop_run():
    """the uninterrupted run with its images at the four save points, chosen from its own status log as it goes"""
    n = lh.scenario_length()
    sm = core.SurfelMapping(params_with_size(LW, LH), loop_params=loop_params())
    log, points = [], {}
    for k in range(n):
        log.append(loop_step(sm, k))
        first_found = next((j for j, s in enumerate(log) if s["found_candidate"]), None)
        if k == 50:
            points["quiet"] = k
        if first_found is not None and k == first_found + 3:
            points["queued"] = k
        if log[k]["started_optimization"] and "started" not in points:
            points["started"] = k
        if log[k]["integrated"] and "integrated" not in points:
            points["integrated"] = k
        for name, at in points.items():
            if at == k and not isinstance(at, tuple):
                points[name] = (k, sm.save())
    return dict(sm=sm, log=log, points=points, n=n, final=loop_final(sm))


@pytest.mark.parametrize("point", ["quiet", "queued", "started", "integrated"])
def test_resume_with_loop_closing(loop_run, point):
    assert set(loop_run["points"]) == {"quiet", "queued", "started", "integrated"}, list(loop_run["points"])
    k0, img = loop_run["points"][point]
    info = core.checkpoint_info(img)
    assert info["has_loop"] and info["n_nodes"] == k0 + 1 and info["n_edges"] >= k0
    assert bool(info["has_opt"]) == (point == "started"), (point, info["has_opt"])
    print(point, k0, {k: loop_run["log"][k0][k] for k in ("n_unverified", "already_verified", "loop_count",
                                                             "currently_optimizing")}, len(img))
    sm = core.SurfelMapping.restore(img)
    assert sm.posegraph is not None and sm.timestamp() == k0 + 1
    bad = lh.status_equal(sm.loopStatus().as_dict(), loop_run["log"][k0])
    assert not bad, ("after the load", bad)
    for k in range(k0 + 1, loop_run["n"]):
        got = loop_step(sm, k)
        bad = lh.status_equal(got, loop_run["log"][k])
        assert not bad, (point, k, bad, got, loop_run["log"][k])
    got, want = loop_final(sm), loop_run["final"]
    for key in want:
        assert got[key] == want[key], (point, key)
    sm.close()


# ---- crafted images at the kernels' boundaries ----
TILE_COUNTS = [1, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]


def records(rng, n):
    r = rng.integers(0, 1 << 32, (n, 16), dtype=np.uint32)
    r[:, 15] = np.arange(n, dtype=np.uint32) + 0x10000  # distinct
    if n > 2:
        r[0, 0], r[1, 1], r[2, 2] = 0x7fc00001, 0x80000000, 0xff800000  # a NaN, -0, -inf
    return r.view(SURFEL_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def small():
    p = core.SurfelMapping(params_with_size(64, 16))
    for k in range(3):
        p.processScan(*ls.scan(k, 64, 16), fixed_iterations=ITER)
    return p, ck.read(p.save())


@pytest.mark.parametrize("n_active", [0, 1, 4097])
def test_crafted_images(small, n_active):
    p, secs = small
    rng = np.random.default_rng(n_active)
    tiles = {(k - 5, (3 * k) % 7 - 3): records(rng, n) for k, n in enumerate(TILE_COUNTS)}
    active = records(rng, n_active)
    if n_active:  # one active record and one tile record that differ in a single bit, exchanged
        key = sorted(tiles)[4]
        x, y = n_active // 2, len(tiles[key]) // 2
        twin = active[x:x + 1].copy().view(np.uint32).reshape(1, 16)
        twin[0, 7] ^= 1 << 13
        tiles[key][y], active[x] = active[x].copy(), twin.view(SURFEL_DTYPE).reshape(-1)[0]
    img = ck.write(ck.with_map(secs, active, tiles))
    assert ck.verify(img) == []
    p.load(img)
    assert p.map.cached_tiles() == sorted(tiles)
    for ij in tiles:
        assert p.map.cached_tile(*ij).tobytes() == tiles[ij].tobytes(), ij
    assert p.map.getAllSurfels().tobytes() == active.tobytes() and p.map.size() == n_active
    assert p.map.counts()[2] == sum(TILE_COUNTS) and p.map.cache_stats()[0] == sum(TILE_COUNTS)
    out = p.save()
    assert out == img
    back = ck.read(out)
    for name, v in back.items():  # every directory digest (the device's, for the surfel sections) equals numpy's
        assert v["digest"] == ck.digest(v["data"]), name
    info = core.checkpoint_info(out)
    assert (info["n_active"], info["n_tiles"], info["n_parked"]) == (n_active, len(TILE_COUNTS), sum(TILE_COUNTS))


# ---- refusals ----
def load_rc(p, img):
    rc = p.L.suma_pipeline_checkpoint_load(p.h, img, len(img))
    return rc, p.L.suma_last_error(p.ctx.h).decode()


def test_refusals_leave_the_pipeline_untouched():
    cap = 60000
    a, b = core.SurfelMapping(circle_params(max_surfels=cap)), core.SurfelMapping(circle_params(max_surfels=cap))
    for k in range(20):
        assert step(a, k) == step(b, k)
    twin = b.save()
    img = a.save()
    assert img == twin
    secs = ck.read(img)
    assert secs["TILES"]["count"] > 0 and 0 < secs["ACTIVE"]["count"] < cap
    dirs = {name: v for name, v in secs.items()}
    n = len(secs)
    d = np.frombuffer(img, dtype=np.uint8)[24:24 + 40 * n].view(ck.DIR_DTYPE)
    offsets = {ck.SECTION_NAMES[int(e["id"])]: (int(e["offset"]), int(e["bytes"])) for e in d}
    bad = []
    for name, (off, size) in offsets.items():  # truncated at every section boundary, and at that boundary +- 1
        for cut in (off - 1, off, off + 1, off + size - 1, off + size, off + size + 1):
            if 0 <= cut < len(img):
                bad.append((f"cut {name} {cut}", img[:cut], -1, ""))
    for name in ("ACTIVE", "TILES", "POSES"):  # one flipped payload byte: the message names the section
        off, size = offsets[name]
        m = bytearray(img)
        m[off + size // 2] ^= 0x10
        bad.append((f"flip {name}", bytes(m), -1, f"section {name}"))
    m = bytearray(img)
    m[13] ^= 0x01
    bad.append(("flip header", bytes(m), -1, ""))
    other = dict(dirs)
    pw = secs["PARAMS"]["data"].copy().view("<u4")
    pw[0] += 4
    other["PARAMS"] = dict(data=pw.view(np.uint8), count=1)
    bad.append(("data_width", ck.write(other), -1, "data_width"))
    big = ck.write(ck.with_map(secs, np.zeros(cap + 1, dtype=SURFEL_DTYPE), {}))
    bad.append(("n_active", big, -3, "max_surfels"))
    for what, image, code, needle in bad:
        rc, msg = load_rc(a, image)
        assert rc == code and msg and needle in msg, (what, rc, msg)
        assert a.save() == twin, what
    # save between beginScan and updateMap; a size query
    a.beginScan(*ls.scan(20, W, H))
    n = core.C.c_uint64()
    assert a.L.suma_pipeline_checkpoint_save(a.h, None, 0, core.C.byref(n)) == -1
    assert a.L.suma_pipeline_checkpoint_size(a.h, core.C.byref(n)) == -1
    with pytest.raises(core.SumaError):
        a.load(img)
    a.updatePose(ITER)
    a.updateMap()
    b.processScan(*ls.scan(20, W, H), fixed_iterations=ITER)
    assert a.L.suma_pipeline_checkpoint_save(a.h, None, 0, core.C.byref(n)) == -3 and n.value == len(b.save())
    for k in range(21, 30):
        assert step(a, k) == step(b, k), k
    assert a.save() == b.save()


def test_off_is_off():
    a, b = core.SurfelMapping(circle_params()), core.SurfelMapping(circle_params())
    saved = 0
    for k in range(30):
        assert step(a, k) == step(b, k), k
        if k % 5 == 4:
            saved += len(b.save())
    assert saved > 100000
    assert a.map.getAllSurfels().tobytes() == b.map.getAllSurfels().tobytes()
    assert a.map.poses().tobytes() == b.map.poses().tobytes()
    assert a.map.counts() == b.map.counts() and a.map.cache_stats() == b.map.cache_stats()
    assert a.map.cached_tiles() == b.map.cached_tiles()
    for ij in a.map.cached_tiles():
        assert a.map.cached_tile(*ij).tobytes() == b.map.cached_tile(*ij).tobytes()
    assert [a.frame(0).download(w).tobytes() for w in range(3)] == [b.frame(0).download(w).tobytes() for w in range(3)]


# ---- the compiled hosts: examples/odometry.c and include/suma_adapter.hpp ----
C_SCANS, C_SAVE_AT, C_WIDTH = 20, 10, 900


@pytest.fixture(scope="module")
def scan_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("velodyne")
    for k in range(C_SCANS):
        pts = get_scan(k, C_WIDTH, False)[0].copy()
        pts[:, 3] = 1.0
        pts.astype("<f4").tofile(str(d / f"{k:06d}.bin"))
    return str(d)


def build_host(tmp, src, lang):
    exe = os.path.join(tmp, os.path.basename(src).split(".")[0])
    libdir = os.path.dirname(core.LIB_PATH)
    cc = ["g++", "-std=c++11", "-O1"] if lang == "c++" else ["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O1"]
    subprocess.check_call(cc + ["-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lsuma_hip",
                                "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_c_example_checkpoint_and_resume(scan_dir, tmp_path):
    """examples/odometry.c: 20 scans in one run; 10 scans with --checkpoint, then --resume to 20.  The two pose files one
    after the other are the single run's file, character for character."""
    exe = build_host(str(tmp_path), os.path.join(ROOT, "examples", "odometry.c"), "c")
    image = str(tmp_path / "session.ckpt")

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)

    whole = run(scan_dir, C_SCANS)
    assert whole.returncode == 0 and len(whole.stdout.splitlines()) == C_SCANS, whole.stderr
    head = run("--checkpoint", image, "--checkpoint-every", C_SAVE_AT, scan_dir, C_SAVE_AT)
    assert head.returncode == 0 and len(head.stdout.splitlines()) == C_SAVE_AT, head.stderr
    assert os.path.exists(image) and not os.path.exists(image + ".tmp")
    with open(image, "rb") as f:
        info = core.checkpoint_info(f.read())
    assert info["timestamp"] == C_SAVE_AT and info["n_active"] > 10000 and not info["has_loop"]
    tail = run("--resume", image, scan_dir, C_SCANS)
    assert tail.returncode == 0 and len(tail.stdout.splitlines()) == C_SCANS - C_SAVE_AT, tail.stderr
    assert head.stdout + tail.stdout == whole.stdout
    # a file that is no image is refused before a scan is read; --checkpoint without --checkpoint-every is the usage
    junk = tmp_path / "junk.ckpt"
    junk.write_bytes(b"\0" * 4096)
    bad = run("--resume", junk, scan_dir, C_SCANS)
    assert bad.returncode == 1 and bad.stdout == "" and "junk.ckpt" in bad.stderr
    assert run("--checkpoint", image, scan_dir, C_SCANS).returncode == 2


def test_cpp_adapter_checkpoint_and_resume(scan_dir, tmp_path):
    """suma_hip::SurfelMapping::saveCheckpoint / loadCheckpoint (tests/cpp/checkpoint_driver.cpp): a second object that
    loads the file written after scan 10 continues with the pose bits of the first"""
    exe = build_host(str(tmp_path), os.path.join(ROOT, "tests", "cpp", "checkpoint_driver.cpp"), "c++")
    image = str(tmp_path / "adapter.ckpt")
    out = subprocess.run([exe, scan_dir, str(C_SCANS), str(C_SAVE_AT), str(C_WIDTH), image], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 2 * C_SCANS - C_SAVE_AT and not os.path.exists(image + ".tmp")
    assert lines[C_SCANS:] == lines[C_SAVE_AT:C_SCANS]
    assert [int(l.split()[0]) for l in lines[C_SCANS:]] == list(range(C_SAVE_AT, C_SCANS))
    assert len(set(lines[:C_SCANS])) == C_SCANS  # it moved
