"""The traversability grid's specification on the host (tests/grid_shim.c, the yardstick of test_gpu_grid.py): every rule
of the shim against an independent numpy fp32 statement on crafted records, the .npz round trip of semantic_suma_amd.mapio,
and one semantic check end to end without a GPU -- a short synthetic sequence through the CPU oracle pipeline, the world
shim and the grid shim, against the scene's known geometry."""
import math

import numpy as np
import pytest

import grid_common as gc
import world_common as wc
from semantic_suma_amd import mapio, synth
from semantic_suma_amd.types import (GRID_CELL_DTYPE, GRID_FREE, GRID_NO_GROUND, GRID_OBSTACLE, GRID_UNKNOWN,
                                     WORLD_SURFEL_DTYPE, params_with_size)

NAN = np.array([gc.NAN_BITS], dtype=np.uint32).view(np.float32)[0]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return gc.build_shim(tmp_path_factory.mktemp("grid_host"))


def most_confident(conf, s):
    """of the members with confidences conf and source indices s: a number beats a NaN, then the greatest, then the
    smallest s"""
    ok = ~np.isnan(conf)
    if ok.any():
        pick = ok & (conf == conf[ok].max())
        return s[pick].min()
    return s.min()


def lowest(z):
    return z[np.lexsort((~np.signbit(z), z))[0]]   # -0 below +0


def highest(z):
    return z[np.lexsort((~np.signbit(z), z))[-1]]


def numpy_grid(rec, gp):
    """the specification stated with numpy, cell by cell (slow: for small rasters)"""
    W, H = gp.width, gp.height
    cell = gc.cell_of(rec, gp)
    L = np.where(rec["label"] < 260, rec["label"], 0)
    w = rec["prob"].astype(np.float32)
    q = np.rint(np.where(w > 0, np.minimum(w, np.float32(1.0)), np.float32(0.0)).astype(np.float32) * np.float32(65535.0)).astype(np.int64)
    is_ground = np.array([gp.ground_label[int(l)] != 0 for l in L], dtype=bool)
    with np.errstate(invalid="ignore"):
        is_ground &= np.abs(rec["nz"]) >= np.float32(gp.min_normal_z)
    out = np.zeros((H, W), dtype=GRID_CELL_DTYPE)
    for f in ("ground_z", "ground_rough", "z_min", "z_max", "obstacle_z"):
        out[f] = NAN
    flat = out.reshape(-1)
    members = {}
    for c in np.unique(cell[cell >= 0]):
        s = np.flatnonzero(cell == c)
        members[int(c)] = s
        o = flat[c]
        z = rec["z"][s]
        o["support"], o["z_min"], o["z_max"] = len(s), lowest(z), highest(z)
        sums = np.bincount(L[s], weights=q[s].astype(np.float64), minlength=260)  # exact: < 2^53
        if sums.sum() > 0:
            o["label"] = sums.argmax()
            o["prob"] = np.float32(sums.max()) / np.float32(sums.sum())
        else:
            o["label"] = L[most_confident(rec["confidence"][s], s)]
        g = s[is_ground[s]]
        o["n_ground"] = len(g)
        if len(g):
            o["ground_z"] = rec["z"][most_confident(rec["confidence"][g], g)]
            o["ground_rough"] = highest(rec["z"][g]) - lowest(rec["z"][g])
    own = flat["ground_z"].copy()
    R = gp.fill_radius
    for c in range(W * H):
        o = flat[c]
        ix, iy = c % W, c // W
        g = None
        if o["n_ground"]:
            g, o["ground_source"] = own[c], 1
        else:
            cand = [(dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)
                    if 0 <= ix + dx < W and 0 <= iy + dy < H and flat["n_ground"][(iy + dy) * W + ix + dx] > 0]
            if cand:
                _, dy, dx = min(cand)
                g = own[(iy + dy) * W + ix + dx]
                o["ground_z"], o["ground_rough"], o["ground_source"] = g, NAN, 2
        if g is not None and o["support"]:
            z = rec["z"][members[c]]
            h = (z - np.float32(g)).astype(np.float32)
            over = h > np.float32(gp.clearance)
            obst = ~over & (h > np.float32(gp.step_height))
            o["n_overhang"], o["n_obstacle"] = over.sum(), obst.sum()
            if obst.any():
                o["obstacle_z"] = highest(z[obst])
        o["state"] = GRID_UNKNOWN if not o["support"] else GRID_NO_GROUND if g is None else \
            GRID_OBSTACLE if o["n_obstacle"] else GRID_FREE
    st = dict(n_records=len(rec), n_dropped=int((cell == -2).sum()), n_outside=int((cell == -1).sum()),
              n_binned=int((cell >= 0).sum()), n_occupied=int((flat["support"] > 0).sum()),
              n_free=int((flat["state"] == GRID_FREE).sum()), n_obstacle=int((flat["state"] == GRID_OBSTACLE).sum()),
              n_no_ground=int((flat["state"] == GRID_NO_GROUND).sum()), n_filled=int((flat["ground_source"] == 2).sum()))
    return out, st


def same(shim, rec, gp):
    """the shim equals the numpy statement on (rec, gp), byte for byte; -> the cells and the stats"""
    got, st = gc.shim_grid(shim, rec, gp)
    want, wst = numpy_grid(rec, gp)
    assert st == wst
    for f in GRID_CELL_DTYPE.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    return got, st


def test_cell_index(shim):
    rng = np.random.default_rng(1)
    for gp in (gc.params(7, 5, 0.25), gc.params(7, 5, 0.2, origin=(-0.7, -0.3)), gc.params(1, 1, 3.0, origin=(-1.5, -1.5))):
        v = np.concatenate([rng.uniform(-2.0, 3.0, 400), np.arange(-8, 12) * gp.cell_size + gp.origin_x,
                            [np.nan, np.inf, -np.inf, -0.0, 1e30, -1e30]]).astype(np.float32)
        r = np.zeros(len(v), dtype=WORLD_SURFEL_DTYPE)
        r["x"], r["y"] = v, rng.permutation(v)
        r["z"][::17] = np.nan
        want = gc.cell_of(r, gp)
        got = [shim.grid_shim_cell(gp, float(a), float(b), float(c)) for a, b, c in zip(r["x"], r["y"], r["z"])]
        assert got == want.tolist() and {-2, -1} <= set(got) and max(got) >= 0
    gp = gc.params(4, 3, 0.25)  # edges: the lower edge belongs to the cell, the window's far edge is outside
    assert shim.grid_shim_cell(gp, 0.25, 0.5, 0.0) == 2 * 4 + 1 and shim.grid_shim_cell(gp, 0.0, 0.0, 0.0) == 0
    assert shim.grid_shim_cell(gp, 1.0, 0.0, 0.0) == -1 and shim.grid_shim_cell(gp, 0.0, 0.75, 0.0) == -1
    assert shim.grid_shim_cell(gp, -0.0, 0.0, 0.0) == 0 and shim.grid_shim_cell(gp, -1e-9, 0.0, 0.0) == -1


@pytest.mark.parametrize("fill", [0, 1, 3, 8])
def test_a_scene_against_numpy(shim, fill):
    rec = gc.scene(1500)
    rec["confidence"][::41] = np.nan
    rec["prob"][::29] = 0.0
    rec["label"][::53] = 300
    got, st = same(shim, rec, gc.params(40, 22, 0.5, origin=(-2.0, -1.5), fill_radius=fill))
    assert st["n_outside"] == 0 and st["n_occupied"] > 500 and len(set(got["state"].reshape(-1).tolist())) >= 3
    got, st = same(shim, rec, gc.params(23, 9, 0.25, origin=(3.0, 2.0), fill_radius=fill))  # most records outside
    assert st["n_outside"] > 1000 and (fill == 0) == (st["n_filled"] == 0)


one = gc.one


def test_ground_membership_and_representative(shim):
    gp = gc.params(1, 1, 1.0)
    rec = np.concatenate([
        one(0.5, 0.5, 1.0, conf=np.nan),            # a NaN confidence never wins over a number
        one(0.5, 0.5, 2.0, conf=3.0),
        one(0.5, 0.5, 3.0, conf=3.0),               # a tie: the smaller source index stays
        one(0.5, 0.5, 4.0, conf=9.0, label=10),     # not a ground label
        one(0.5, 0.5, 5.0, conf=9.0, nz=0.69),      # too steep
        one(0.5, 0.5, 6.0, conf=9.0, nz=np.nan),    # NaN fails
        one(0.5, 0.5, 0.5, conf=-np.inf, nz=-0.7),  # |nz| at the threshold counts; -inf is a number
    ])
    got, _ = same(shim, rec, gp)
    c = got[0, 0]
    assert (c["n_ground"], c["ground_z"], c["ground_rough"], c["support"]) == (4, 2.0, 2.5, 7)
    assert (c["z_min"], c["z_max"]) == (0.5, 6.0)
    got, _ = same(shim, rec[[0, 3]], gp)            # alone, the NaN member is the representative
    assert got[0, 0]["ground_z"] == 1.0 and got[0, 0]["ground_rough"] == 0.0
    # the vote: equal sums -> the smaller id; all weights 0 -> the most confident member's label, prob 0
    v = np.concatenate([one(0.5, 0.5, 0.0, label=48, prob=0.5), one(0.5, 0.5, 0.0, label=40, prob=0.5)])
    got, _ = same(shim, v, gp)
    assert (got[0, 0]["label"], got[0, 0]["prob"]) == (40, 0.5)
    v["prob"], v["confidence"] = 0.0, [5.0, 1.0]
    got, _ = same(shim, v, gp)
    assert (got[0, 0]["label"], got[0, 0]["prob"]) == (48, 0.0)
    z = np.concatenate([one(0.5, 0.5, 0.0), one(0.5, 0.5, -0.0), one(0.5, 0.5, 0.0)])   # -0 is below +0, in any order
    got, _ = same(shim, z, gp)
    assert np.signbit(got[0, 0]["z_min"]) and not np.signbit(got[0, 0]["z_max"])


def test_thresholds_are_strict(shim):
    gp = gc.params(1, 1, 1.0, step_height=0.25, clearance=2.0)
    rec = np.concatenate([one(0.5, 0.5, -1.75), one(0.5, 0.5, -1.5, label=10), one(0.5, 0.5, 0.25, label=10),
                          one(0.5, 0.5, 0.5, label=10)])
    got, _ = same(shim, rec, gp)   # h = 0.25: surface; h = 2.0: obstacle; h = 2.25: overhang
    c = got[0, 0]
    assert (c["n_obstacle"], c["n_overhang"], c["obstacle_z"], c["state"]) == (1, 1, 0.25, GRID_OBSTACLE)
    got, _ = same(shim, rec[[0, 1, 3]], gp)
    assert (got[0, 0]["n_obstacle"], got[0, 0]["n_overhang"], got[0, 0]["state"]) == (0, 1, GRID_FREE)
    assert np.isnan(got[0, 0]["obstacle_z"])
    got, _ = same(shim, rec[1:], gp)
    assert got[0, 0]["state"] == GRID_NO_GROUND and got[0, 0]["n_obstacle"] == 0 and np.isnan(got[0, 0]["ground_z"])


def test_fill_choice(shim):
    # ground at the four neighbours of the centre of a 5 x 5 raster, a car in the centre: the smallest dy wins
    heights = {(2, 1): 1.0, (1, 2): 2.0, (3, 2): 3.0, (2, 3): 4.0}
    rec = np.concatenate([one(ix + 0.5, iy + 0.5, z) for (ix, iy), z in heights.items()] + [one(2.5, 2.5, 2.5, label=10)])
    got, st = same(shim, rec, gc.params(5, 5, 1.0, fill_radius=1))
    assert (got[2, 2]["ground_z"], got[2, 2]["ground_source"], got[2, 2]["state"]) == (1.0, 2, GRID_OBSTACLE)
    assert np.isnan(got[2, 2]["ground_rough"])
    assert got[1, 1]["ground_z"] == 1.0 and got[1, 1]["state"] == GRID_UNKNOWN   # dy = 0, dx = 1 and dy = 1, dx = 0: dy first
    assert got[3, 3]["ground_z"] == 3.0                                          # dy = -1, dx = 0 before dy = 0, dx = -1
    assert got[0, 0]["ground_source"] == 0 and st["n_filled"] == 17
    got, _ = same(shim, rec[1:], gc.params(5, 5, 1.0, fill_radius=1))            # without the south one: smallest dx
    assert got[2, 2]["ground_z"] == 2.0
    got, st = same(shim, rec, gc.params(5, 5, 1.0, fill_radius=8))               # the window is clipped at the borders
    assert st["n_filled"] == 21 and got[0, 0]["ground_z"] == 1.0 and got[4, 4]["ground_z"] == 3.0
    got, st = same(shim, rec, gc.params(5, 5, 1.0, fill_radius=0))
    assert st["n_filled"] == 0 and got[2, 2]["state"] == GRID_NO_GROUND
    # a nearer cell wins over a smaller dy; a filled cell never feeds another
    rec = np.concatenate([one(0.5, 0.5, 1.0), one(3.5, 2.5, 2.0)])
    got, _ = same(shim, rec, gc.params(5, 5, 1.0, fill_radius=2))
    assert got[2, 2]["ground_z"] == 2.0 and got[2, 1]["ground_z"] == 2.0 and got[1, 1]["ground_z"] == 1.0
    assert got[4, 0]["ground_source"] == 0


def test_grid_file_round_trip(tmp_path, shim):
    gp = gc.params(23, 9, 0.25, origin=(3.0, 2.0), ground_labels=[40, 72], fill_radius=3)
    cells, _ = gc.shim_grid(shim, gc.scene(800), gp)
    path = str(tmp_path / "map.grid.npz")
    mapio.write_grid(path, cells, gp)
    back, gp2 = mapio.read_grid(path)
    assert back.dtype == GRID_CELL_DTYPE and back.shape == (9, 23) and back.tobytes() == cells.tobytes()
    assert bytes(gp2) == bytes(gp)
    with pytest.raises(ValueError):
        mapio.write_grid(path, cells[:, :5], gp)


# ---- end to end on the CPU: synth -> oracle pipeline -> world shim -> grid shim, against the scene
K0, SCANS, CELL = 148, 3, 0.2
# Road cells away from every footprint that are not FREE, as a share of such cells.  Observed with the shim on this scene
# (3 scans from scan 148, 900 x 64, 0.2 m cells): 20 of 12469 = 0.16 % -- 19 NO_GROUND (sparse far cells whose few surfels
# have normals below min_normal_z and no ground cell within the fill radius) and 1 OBSTACLE.  The cap leaves room for a
# different libm or compiler on the oracle's side, not for a wrong rule: one mislabelled threshold moves whole classes
# of cells, tens of per cent.
ROAD_NOT_FREE_CAP = 0.01


@pytest.fixture(scope="module")
def synth_grid(shim, tmp_path_factory):
    """the grid of the map after SCANS scans that start beside a low static cube (cube 8 of synth.py: 1.5 m wide, its top
    at 1.4 m, 2 m beside the track and below the sensor, so its top is seen), and the map frame's pose in the scene.  The
    cubes are cars (label 10), whose points preprocessing drops during the first ten scans: they are relabelled
    other-object (99) here, so that three scans map them; the geometry is untouched."""
    from oracle import pyoracle
    p = params_with_size(900, 64)
    op = pyoracle.OraclePipeline(p)
    for k in range(K0, K0 + SCANS):
        pts, lab, prob, _ = synth.generate_scan(k, n_azimuth=900)
        lab = np.where(lab == synth.LABEL_CAR, np.float32(99.0), lab)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    src = op.ctx.map_surfels()
    poses = op.ctx.map_poses().reshape(-1, 4, 4).transpose(0, 2, 1)
    world, wst, _ = wc.shim_export(wc.build_shim(tmp_path_factory.mktemp("grid_world")), src, poses, p.max_poses)
    assert wst["n_out"] == len(src) > 20000
    fit = gc.fit_of(world, CELL, 1)
    gp = gc.params(fit[2], fit[3], CELL, origin=fit[:2])
    cells, st = gc.shim_grid(shim, world, gp)
    assert st["n_outside"] == 0 and st["n_dropped"] == 0
    return cells, gp, synth.trajectory_pose(K0)


def footprint_distance(xy, k_range, moving=True):
    """how far inside (negative) or outside (positive) the nearest footprint every scene point [n, 2] lies: the boxes
    of every scan in k_range as rotated rectangles (the odd cubes move and sweep theirs; moving=False leaves them out),
    the two walls as lines"""
    d = np.minimum(np.abs(xy[:, 1] - synth.WALL_Y), np.abs(xy[:, 1] + synth.WALL_Y))
    for k in k_range:
        c, half, yaw, _ = synth._boxes(k)
        for b in range(len(c)):
            if not moving and b < len(synth._CUBES) and b % 2 == 1:
                continue
            cs, sn = math.cos(yaw[b]), math.sin(yaw[b])
            rel = xy - c[b, :2]
            q = np.abs(np.stack([cs * rel[:, 0] + sn * rel[:, 1], -sn * rel[:, 0] + cs * rel[:, 1]], 1)) - half[b, :2]
            outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
            d = np.minimum(d, np.where(outside > 0, outside, q.max(1)))
    return d


def test_the_grid_of_a_synthetic_street_matches_the_scene(synth_grid):
    cells, gp, T0 = synth_grid
    iy, ix = np.mgrid[0:gp.height, 0:gp.width]
    centre = np.stack([gp.origin_x + (ix + 0.5) * gp.cell_size, gp.origin_y + (iy + 0.5) * gp.cell_size], -1).reshape(-1, 2)
    scene_xy = centre @ T0[:2, :2].T + T0[:2, 3]          # the map frame is the first scan's sensor frame: yaw and shift
    d = footprint_distance(scene_xy, range(K0, K0 + SCANS)).reshape(gp.height, gp.width)
    d_static = footprint_distance(scene_xy, [K0], moving=False).reshape(gp.height, gp.width)
    supported = cells["support"] > 0
    # 1. inside a footprint shrunk by one cell nothing is FREE (a moving cube uncovers the ground behind it: static ones)
    inside = supported & (d_static < -gp.cell_size)
    assert inside.sum() >= 10, inside.sum()
    assert not np.any(cells["state"][inside] == GRID_FREE)
    assert np.any(cells["state"][inside] == GRID_OBSTACLE)  # the cube's top over ground filled from beside it
    # 2. road cells more than one cell away from every footprint are FREE, except a share
    road = supported & (cells["label"] == 40) & (d > gp.cell_size)
    not_free = road & (cells["state"] != GRID_FREE)
    share = not_free.sum() / road.sum()
    print(f"road cells {road.sum()}, not FREE {not_free.sum()} (by state {np.bincount(cells['state'][not_free], minlength=4)}), "
          f"share {share:.5f}")
    assert road.sum() > 5000
    assert share <= ROAD_NOT_FREE_CAP
