"""The host restatement of the localiser's specification (tests/localize_shim.c, csrc/k_localize.hip) against a numpy
restatement -- lexsort by (i, j, source index) -- on crafted maps around every boundary, the re-centring hysteresis, and
the tracking condition on the whole localiser over the CPU oracle (tests/localize_host.py).  No GPU."""
import numpy as np
import pytest

import localize_common as lc
import world_common as wc
from semantic_suma_amd.types import SURFEL_DTYPE, WORLD_SURFEL_DTYPE

E = 10.0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return lc.build_shim(tmp_path_factory.mktemp("localize_host"))


def windows_equal(shim, records, extent, origins, dims=(0, 1, 2)):
    m = lc.ShimMap(shim, records, extent)
    for oi, oj in origins:
        for dim in dims:
            want, dropped = lc.numpy_window(records, extent, oi, oj, dim)
            got = m.window(oi, oj, dim)
            assert m.n_dropped == dropped and m.n_kept == len(records) - dropped
            assert got.dtype == SURFEL_DTYPE and got.tobytes() == want.tobytes(), (oi, oj, dim, len(got), len(want))
    return m


def test_cells_on_the_tile_edges(shim):
    e = np.float32(E)
    assert lc.shim_cell(shim, E, 0.0, 0.0) == (0, 0) and lc.shim_cell(shim, E, -0.0, -0.0) == (0, 0)
    assert lc.shim_cell(shim, E, e, -e) == (1, 0)            # x = e opens tile 1, y = -e opens tile 0
    # the sum x + e is rounded as written: the float just below e still gives 2e and falls into tile 1
    assert lc.shim_cell(shim, E, np.nextafter(e, np.float32(0)), np.nextafter(-e, np.float32(-100))) == (1, -1)
    assert lc.shim_cell(shim, E, 9.99999, -10.00001) == (0, -1)
    assert lc.shim_cell(shim, E, 3 * e, -3 * e) == (2, -1) and lc.shim_cell(shim, E, 5 * e, 7 * e) == (3, 4)
    assert lc.shim_cell(shim, E, -0.5, -72.5) == (0, -4)     # floorf, not truncation
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 0, np.nan), (3e38, 0, 0), (0, -3e38, 0)):
        assert lc.shim_cell(shim, E, *bad) is None, bad
    g = float(lc.GRID)
    assert lc.shim_cell(shim, E, 2 * g * E, 0.0) is None and lc.shim_cell(shim, E, -2 * g * E, 0.0) is None
    assert lc.shim_cell(shim, E, -(2 * g - 2) * E, (2 * g - 2) * E) == (-lc.GRID + 1, lc.GRID - 1)
    assert shim.loc_shim_key(-lc.GRID + 1, lc.GRID - 1) == (1 << 21) | (2 * lc.GRID - 1)
    assert shim.loc_shim_key(0, 0) == (lc.GRID << 21) | lc.GRID


def test_edge_records(shim):
    r = lc.edge_records(E)
    origins = [(0, 0), (1, 0), (-1, -1), (2, 1), (-4, 0), (-lc.GRID + 1, 0), (0, lc.GRID - 1), (lc.GRID - 1, lc.GRID - 1)]
    m = windows_equal(shim, r, E, origins)
    assert m.n_dropped == 8
    keys = m.dir["key"]
    assert np.all(keys[1:] > keys[:-1]) and int(m.dir["count"].sum()) == m.n_kept
    assert np.array_equal(m.dir["start"], np.concatenate([[0], np.cumsum(m.dir["count"])[:-1]]))
    # a window at the grid's edge holds the one record there, and its tiles beyond the grid are skipped
    assert len(m.window(-lc.GRID + 1, 0, 2)) == 1 and len(m.window(0, lc.GRID - 1, 2)) == 1


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 5000])
def test_crafted_maps(shim, n):
    r = lc.crafted_records(n, E)
    m = windows_equal(shim, r, E, [(0, 0), (1, -2), (-3, 3), (9, 9)], dims=(0, 2))
    assert m.n_dropped == 0 and (n == 0 or m.n_tiles > 1 or n == 1)
    if n >= 255:
        assert 0 < len(m.window(0, 0, 2)) < n
    both = np.concatenate([r, lc.edge_records(E)])
    windows_equal(shim, both, E, [(0, 0), (-1, 1)], dims=(2,))


def test_all_records_in_one_tile(shim):
    r = lc.crafted_records(777, E)
    r["x"] = np.linspace(-9.99, 9.99, 777).astype(np.float32) + np.float32(40.0)
    r["y"] = np.float32(-20.0) + np.linspace(-9.5, 9.5, 777).astype(np.float32)[::-1]
    m = windows_equal(shim, r, E, [(2, -1), (0, 0), (4, -3), (5, -1)], dims=(0, 2))
    assert m.n_tiles == 1 and int(m.dir["count"][0]) == 777
    w = m.window(2, -1, 0)
    assert np.array_equal(w["x"], r["x"]) and np.all(w["timestamp"] == 0) and np.all(w["count"] == 0)  # source order
    assert len(m.window(5, -1, 2)) == 0 and len(m.window(4, -3, 2)) == 777


def test_conversion(shim):
    r = lc.crafted_records(300, E)
    r["label"][:260] = np.arange(260)
    m = lc.ShimMap(shim, r, E)
    w = m.window(0, 0, 8)
    assert len(w) == 300
    src = r[np.lexsort((np.arange(300), np.floor((r["y"] + np.float32(E)) / np.float32(2 * E)),
                        np.floor((r["x"] + np.float32(E)) / np.float32(2 * E))))]
    for f in ("x", "y", "z", "radius", "nx", "ny", "nz", "confidence"):
        assert w[f].tobytes() == src[f].tobytes(), f
    assert w["w"].tobytes() == src["prob"].tobytes()
    for f in ("timestamp", "color", "weight", "count"):
        assert not w[f].view(np.uint32).any(), f
    # the label comes back through the export's own rule (k_world.hip step 1)
    assert np.array_equal(wc.labels_of(w), src["label"]) and np.array_equal(w["r"], w["g"]) and np.array_equal(w["g"], w["b"])


def test_hysteresis(shim):
    e = E
    assert lc.shim_recentre(shim, e, 1.09 * e, 0.0, 0, 0) == (False, 0, 0)
    assert lc.shim_recentre(shim, e, 1.11 * e, 0.0, 0, 0) == (True, 1, 0)
    assert lc.shim_recentre(shim, e, -1.11 * e, 0.0, 0, 0) == (True, -1, 0)
    assert lc.shim_recentre(shim, e, 0.0, 1.09 * e, 0, 0) == (False, 0, 0)
    assert lc.shim_recentre(shim, e, 0.0, -1.11 * e, 0, 0) == (True, 0, -1)
    # both axes in one scan, one step each however far the pose lies
    assert lc.shim_recentre(shim, e, 1.2 * e, -1.2 * e, 0, 0) == (True, 1, -1)
    assert lc.shim_recentre(shim, e, 9.0 * e, 9.0 * e, 0, 0) == (True, 1, 1)
    # around another origin: the centre is (2 oi e, 2 oj e)
    assert lc.shim_recentre(shim, e, (6 + 1.09) * e, (-4 - 1.09) * e, 3, -2) == (False, 3, -2)
    assert lc.shim_recentre(shim, e, (6 + 1.11) * e, (-4 - 1.11) * e, 3, -2) == (True, 4, -3)
    # the threshold itself is fp32 1.1f * e: exactly on it does not move
    thr = float(np.float32(1.1) * np.float32(e))
    assert lc.shim_recentre(shim, e, thr, 0.0, 0, 0) == (False, 0, 0)
    assert lc.shim_recentre(shim, e, float(np.nextafter(np.float32(thr), np.float32(100))), 0.0, 0, 0) == (True, 1, 0)
    # a pose that has just re-centred sits inside the new window's band: no step back
    assert lc.shim_recentre(shim, e, 1.11 * e, 0.0, 1, 0) == (False, 1, 0)


# ---- the whole localiser over the CPU oracle

@pytest.fixture(scope="module")
def mapped(shim, tmp_path_factory):
    """45 scans mapped by the oracle pipeline, and the world map the export's host restatement gives (flat and 0.1 m)"""
    from oracle import pyoracle
    pyoracle.build()
    p = lc.loc_params()
    scans = lc.loc_scans()
    op = pyoracle.OraclePipeline(p, threads=8)
    poses = []
    for s in scans:
        op.process_scan(*s, fixed_iterations=0)
        poses.append(op.pose().copy())
    parts = [op.ctx.map_surfels()]
    for i in range(-8, 9):
        for j in range(-8, 9):
            t = op.ctx.map_cache_tile(i, j)
            if len(t):
                parts.append(np.ascontiguousarray(t).view(SURFEL_DTYPE).reshape(-1))
    src = np.concatenate(parts)
    n = len(scans)
    table = op.ctx.map_poses(n).reshape(n, 4, 4).transpose(0, 2, 1)
    wshim = wc.build_shim(tmp_path_factory.mktemp("localize_world"))
    maps = {v: wc.shim_export(wshim, src, table, p.max_poses, voxel_size=v)[0] for v in (0.0, 0.1)}
    assert len(maps[0.0]) == len(src) > 10000 and 1000 < len(maps[0.1]) < len(src)
    return p, scans, poses, maps


def run_host(shim, p, scans, records, start, constant_velocity):
    import localize_host as lh
    from semantic_suma_amd.types import LocalizerParams
    loc = lh.HostLocalizer(p, shim, LocalizerParams.defaults(p, constant_velocity=constant_velocity))
    assert loc.set_map(records) == 0
    loc.set_pose(start)
    return loc, [loc.process_scan(*s) for s in scans]


def tracking(shim, mapped, setting, constant_velocity):
    p, scans, poses, maps = mapped
    records = maps[0.1 if setting == "voxel" else 0.0]
    start = lc.perturbed(poses[0]) if setting == "perturbed" else poses[0]
    loc, res = run_host(shim, p, scans, records, start, constant_velocity)
    bad, worst = lc.tracking_failures([r["pose"] for r in res], poses, first=2 if setting == "perturbed" else 1)
    print(setting, "scans that fail", bad, "worst error %.4f m" % worst, "rebuilds", loc.rebuilds, "window",
          min(r["n_window"] for r in res), max(r["n_window"] for r in res))
    return loc, res, bad, worst


@pytest.mark.parametrize("setting", ["flat", "voxel", "perturbed"])
def test_it_localises_on_the_oracle(shim, mapped, setting):
    """the tracking condition with the default parameters (constant-velocity guess), on a map the oracle pipeline made:
    worst errors 0.086 m (flat), 0.103 m (0.1 m voxels), 0.085 m (perturbed start) of 0.55 m of room; two re-centres"""
    loc, res, bad, worst = tracking(shim, mapped, setting, 1)
    assert not bad, (bad, worst)
    assert loc.rebuilds == 1 + 2 and sum(r["window_rebuilt"] for r in res) == 2
    for r in res:  # the poses stay rigid
        R = r["pose"][:3, :3]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14
    if setting != "perturbed":
        assert all(r["tracked"] for r in res)
    assert np.array_equal(res[0]["increment"], np.eye(4)) and not np.array_equal(res[1]["increment"], np.eye(4))


@pytest.mark.parametrize("setting", ["flat", "voxel", "perturbed"])
def test_it_localises_on_the_oracle_without_the_motion_model(shim, mapped, setting):
    """the same condition with constant_velocity = 0: worst errors 0.065 m (flat), 0.057 m (0.1 m voxels), 0.066 m
    (perturbed start) of 0.55 m of room; two re-centres; every scan passes both gates"""
    loc, res, bad, worst = tracking(shim, mapped, setting, 0)
    assert not bad, (bad, worst)
    assert worst < 0.55 / 2
    assert loc.rebuilds == 1 + 2 and sum(r["window_rebuilt"] for r in res) == 2
    assert all(r["tracked"] for r in res)
    assert np.array_equal(res[0]["increment"], np.eye(4)) and not np.array_equal(res[1]["increment"], np.eye(4))
