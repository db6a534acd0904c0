"""The place-recognition specification (csrc/k_place.hip) on the CPU: tests/place_shim.c against an independent NumPy
restatement on vertex maps the CPU oracle makes from the synthetic scans, and what the descriptor is for -- the best
entry is a neighbouring scan and the shift is the turn."""
import numpy as np
import pytest

import localize_common as lc
import place_common as pc
from oracle import pyoracle
from semantic_suma_amd.types import PlaceParams

PP = dict(rings=20, sectors=60, max_range=50.0, height_offset=2.0)
TURNS = (0, 7, 31)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return pc.build_shim(tmp_path_factory.mktemp("place_shim"))


@pytest.fixture(scope="module")
def maps():
    """vertex / semantic maps of the 45 scans (K1-K3 at the scan's own timestamp, as the mapping pipeline makes them) and
    of the odd scans turned by 0, 7 and 31 sectors (at T_loc, as a localiser makes them)"""
    pyoracle.build()
    p = lc.loc_params()
    ora = pyoracle.Oracle(p, threads=8)
    frame = ora.frame()
    scans = lc.loc_scans()
    t_loc = p.active_timestamps + 10

    def pre(scan, stamp):
        ora.preprocess(*scan, stamp, frame)
        return frame.vertex.copy(), frame.semantic.copy()
    base = [pre(s, k) for k, s in enumerate(scans)]
    S = PP["sectors"]
    turned = {(k, t): pre(pc.turned_scan(scans[k], pc.turn_angle(t, S)), t_loc) for k in range(1, 45, 2) for t in TURNS}
    return base, turned


@pytest.mark.parametrize("kw", [PP, dict(rings=1, sectors=1), dict(rings=64, sectors=64), dict(rings=7, sectors=13),
                                dict(PP, height_offset=0.5)], ids=lambda k: "%dx%d" % (k["rings"], k["sectors"]))
def test_shim_equals_numpy_on_cells(shim, maps, kw):
    pp = PlaceParams.defaults(**kw)
    filled = 0
    for v, s in maps[0][::4] + [maps[1][(5, 7)], maps[1][(21, 31)]]:
        a, b = pc.shim_describe(shim, v, s, pp), pc.numpy_describe(v, s, pp)
        assert a.tobytes() == b.tobytes()
        filled += int((a > 0).sum())
    assert filled > 0


def test_label_mask(shim, maps):
    v, s = maps[0][20]
    labels = set(np.unique((s[..., 0] * np.float32(255.0) + np.float32(0.5)).astype(np.int64)[v[..., 3] > 0]))
    assert len(labels) >= 2, labels
    whole = pc.shim_describe(shim, v, s, PlaceParams.defaults(**PP))
    parts = []
    for l in labels:
        pp = PlaceParams.defaults(keep_labels=[l], **PP)
        a = pc.shim_describe(shim, v, s, pp)
        assert a.tobytes() == pc.numpy_describe(v, s, pp).tobytes()
        parts.append(a)
    assert np.array_equal(np.maximum.reduce(parts), whole)
    none = pc.shim_describe(shim, v, s, PlaceParams.defaults(keep_labels=[], **PP))
    assert not none.any()


def test_best_entry_is_a_neighbour_and_the_shift_is_the_turn(shim, maps):
    """database: the even scans 0 .. 44; queries: the odd scans turned by 0, 7 and 31 sectors -- 66 cases"""
    pp = PlaceParams.defaults(**PP)
    S = pp.sectors
    base, turned = maps
    ids = np.arange(0, 45, 2)
    db = np.stack([pc.shim_describe(shim, *base[k], pp) for k in ids])
    worst = 0.0
    for (k, t), (v, s) in sorted(turned.items()):
        dist, shift = pc.shim_search(shim, db, pc.shim_describe(shim, v, s, pp))
        best = pc.shim_topk(shim, dist, shift, ids, 1, S)[0]
        print("scan %2d turn %2d: best id %2d distance %.4f shift %2d" % (k, t, best["id"], best["distance"], best["shift"]))
        assert abs(best["id"] - k) == 1, (k, t, best)
        assert best["shift"] == (S - t) % S, (k, t, best)
        worst = max(worst, best["distance"])
    assert worst < 0.5, worst


def test_distance_properties(shim):
    S, R = 13, 7
    db = pc.crafted_database(40, S, R)
    norms = pc.shim_norms(shim, db)
    assert np.array_equal(norms[6], np.zeros(S, dtype=np.float32))
    for e in (0, 1, 3):
        # an entry against itself: the least shift that reproduces it is 0, the distance is 0 up to rounding
        dist, shift = pc.shim_search(shim, db[e:e + 1], db[e])
        assert shift[0] == 0 and abs(float(dist[0])) < 1e-6, (e, dist, shift)
        # rolled by t sectors (query column j + t holds entry column j): shift t
        for t in (1, 5, S - 1):
            dist, shift = pc.shim_search(shim, db[e:e + 1], np.roll(db[e], t, axis=0))
            assert shift[0] == t and abs(float(dist[0])) < 1e-6, (e, t, dist, shift)
    # nothing to compare: distance 1, shift 0
    dist, shift = pc.shim_search(shim, db, np.zeros((S, R), dtype=np.float32))
    assert np.array_equal(dist, np.ones(40, dtype=np.float32)) and not shift.any()
    dist, shift = pc.shim_search(shim, db[6:7], db[0])
    assert dist[0] == 1.0 and shift[0] == 0


def test_topk_order_ties_and_exclusion(shim):
    dist = np.array([0.5, 0.25, 0.5, 0.125, 0.25, 1.0, 0.125], dtype=np.float32)
    shift = np.arange(7, dtype=np.int32)
    ids = np.array([10, 11, 12, 13, 14, 15, 16], dtype=np.uint32)
    order = [m["index"] for m in pc.shim_topk(shim, dist, shift, ids, 32, 12)]
    assert order == [3, 6, 1, 4, 0, 2, 5]
    assert [m["index"] for m in pc.shim_topk(shim, dist, shift, ids, 3, 12)] == [3, 6, 1]
    assert [m["index"] for m in pc.shim_topk(shim, dist, shift, ids, 4, 12, exclude=(13, 14))] == [6, 1, 0, 2]
    assert pc.shim_topk(shim, dist, shift, ids, 4, 12, exclude=(0, 100)) == []
    m = pc.shim_topk(shim, dist, shift, ids, 7, 12)
    D = np.float32(2.0) * pc.PI_F / np.float32(12)
    for x in m:
        s = x["shift"]
        want = -np.float32(s) * D if s <= 6 else np.float32(12 - s) * D
        assert np.float32(x["yaw"]).tobytes() == np.float32(want).tobytes()


def test_hypothesis_is_a_turn_about_z(shim):
    T = pc.turned_pose(np.eye(4), 0.3)
    T[:3, 3] = 4.0, -2.0, 0.5
    H = pc.shim_hypothesis(shim, T, 0.7330383)
    assert np.allclose(H, pc.turned_pose(T, 0.7330383), atol=1e-7)
    assert np.array_equal(pc.shim_hypothesis(shim, T, 0.0), T)


def test_hand_made_vertex_maps(shim):
    """every boundary of the descriptor on a hand-made map: the shim, the NumPy restatement and the reading by hand"""
    pp, v, s, _ = pc.hand_made_maps(180, 16)
    cells = pc.shim_describe(shim, v, s, pp)
    assert cells.tobytes() == pc.numpy_describe(v, s, pp).tobytes()
    pc.check_hand_made_cells(cells)
