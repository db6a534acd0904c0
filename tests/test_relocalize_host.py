"""Relocalisation over the CPU oracle (tests/relocalize_host.py): the steps of suma_localizer_relocalize with the place
shim and HostLocalizer, on a map the oracle pipeline made -- the numbers test_gpu_place.py's docstring quotes come from
here, and the restoring of a localiser that finds nothing is checked without a GPU."""
import numpy as np
import pytest

import localize_common as lc
import localize_host as lh
import place_common as pc
import relocalize_host as rh
import world_common as wc
from semantic_suma_amd.types import SURFEL_DTYPE, PlaceParams


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    """45 scans mapped by the oracle pipeline, the flat world map of the export's host restatement, and the places of the
    even scans (each scan's own data frame, max_range = 50) with the mapping poses"""
    from oracle import pyoracle
    pyoracle.build()
    tmp = tmp_path_factory.mktemp("relocalize_host")
    shim, pshim, wshim = lc.build_shim(tmp), pc.build_shim(tmp), wc.build_shim(tmp)
    p = lc.loc_params()
    scans = lc.loc_scans()
    pp = PlaceParams.defaults(max_range=50.0)
    op = pyoracle.OraclePipeline(p, threads=8)
    poses, cells = [], []
    for k, s in enumerate(scans):
        op.process_scan(*s, fixed_iterations=0)
        poses.append(op.pose().copy())
        if k % 2 == 0:
            f = op.frame(0)
            cells.append(pc.shim_describe(pshim, f.vertex, f.semantic, pp))
    parts = [op.ctx.map_surfels()]
    for i in range(-8, 9):
        for j in range(-8, 9):
            t = op.ctx.map_cache_tile(i, j)
            if len(t):
                parts.append(np.ascontiguousarray(t).view(SURFEL_DTYPE).reshape(-1))
    n = len(scans)
    table = op.ctx.map_poses(n).reshape(n, 4, 4).transpose(0, 2, 1)
    records = wc.shim_export(wshim, np.concatenate(parts), table, p.max_poses, voxel_size=0.0)[0]
    ids = np.arange(0, n, 2)
    places = rh.HostPlaces(pshim, pp, np.stack(cells), ids, [poses[k] for k in ids])
    return p, shim, scans, poses, records, places


@pytest.mark.parametrize("k,turn", [(5, (0, 0.0)), (15, (7, 0.0)), (35, (31, 2.0))])
def test_it_relocalises_on_the_oracle(mapped, k, turn):
    """a fresh localiser with no pose, 4 candidates: found, within half a step of the scan's own mapping pose (0.020 m,
    0.048 m, 0.024 m), the yaw within 0.001 rad; the localiser goes on from there"""
    p, shim, scans, poses, records, places = mapped
    h = lh.HostLocalizer(p, shim)
    h.set_map(records)
    theta = pc.turn_angle(turn[0], places.pp.sectors, turn[1])
    r = rh.relocalize(h, places, *pc.turned_scan(scans[k], theta), 4)
    assert r["found"] and r["n_tried"] == 4
    bad, err = lc.tracking_failures([r["result"]["pose"]] * (k + 1), poses, first=k)
    yaw_err = pc.yaw_difference(pc.turned_pose(poses[k], theta), r["result"]["pose"])
    print("scan %d turn %s: winner %d, error %.4f m, yaw error %.5f rad" % (k, turn, r["winner"], err, yaw_err))
    assert not bad and err < 0.1 and abs(yaw_err) < 1e-3
    assert abs(r["match"]["id"] - k) == 1
    tracked = [c for c in r["candidates"] if c["result"]["tracked"]]
    score = lambda c: c["result"]["stats"]["error"] / c["result"]["stats"]["valid"]  # noqa: E731
    assert score(r["candidates"][r["winner"]]) == min(score(c) for c in tracked)
    nxt = h.process_scan(*pc.turned_scan(scans[k + 1], theta))
    assert nxt["tracked"] and not lc.tracking_failures([nxt["pose"]] * (k + 2), poses, first=k + 1)[0]


@pytest.mark.parametrize("with_pose", [False, True])
def test_a_relocalisation_that_finds_nothing_restores_the_localiser(mapped, with_pose):
    p, shim, scans, poses, records, places = mapped
    h, twin = lh.HostLocalizer(p, shim), lh.HostLocalizer(p, shim)
    for x in (h, twin):
        x.set_map(records)
        if with_pose:
            x.set_pose(poses[0])
            x.process_scan(*scans[0])
            x.process_scan(*scans[1])
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    r = rh.relocalize(h, places, *empty, 3)
    assert not r["found"] and r["n_tried"] == 3 and r["winner"] == -1
    assert [(c["match"]["index"], c["match"]["distance"], c["match"]["shift"]) for c in r["candidates"]] == \
        [(i, 1.0, 0) for i in range(3)]
    assert (h.have_pose, h.origin, h.n_window, h.rebuilds) == (twin.have_pose, twin.origin, twin.n_window, twin.rebuilds)
    if with_pose:
        assert h.window.tobytes() == twin.window.tobytes()
        lh.results_equal(h.process_scan(*scans[2]), twin.process_scan(*scans[2]))
