"""suma_place_* and suma_localizer_relocalize on the MI355X (csrc/k_place.hip, csrc/suma_place.hip, core.PlaceIndex,
core.Localizer.relocalize): descriptors, per-entry distances, shifts and matches to the bit against the host restatement
(tests/place_shim.c), storage, the yaw convention, and the relocalisation to the bit against the same steps over the
CPU oracle (tests/relocalize_host.py) and against setPose + processScan on a twin."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import localize_common as lc
import localize_host as lh
import place_common as pc
import relocalize_host as rh
from semantic_suma_amd import core, places, synth
from semantic_suma_amd.types import PlaceParams, WORLD_SURFEL_DTYPE, params_with_size

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 180, 16


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return pc.build_shim(tmp_path_factory.mktemp("place_gpu"))


@pytest.fixture(scope="module")
def lshim(tmp_path_factory):
    return lc.build_shim(tmp_path_factory.mktemp("place_gpu_loc"))


class Small:
    """one 180 x 16 ctx with a frame, six synthetic scans and their vertex / semantic maps (K1-K3 at timestamp 20)"""

    def __init__(self):
        self.p = params_with_size(W, H)
        self.ctx = core.Context(self.p)
        self.pre = core.Preprocessing(self.ctx)
        self.frame = core.Frame(self.ctx, W, H)
        self.scans = [synth.generate_scan(k, W, H)[:3] for k in range(6)]
        self.maps = []
        for s in self.scans:
            self.pre.process(s[0], self.frame, s[1], s[2], 20)
            self.maps.append((self.frame.vertex, self.frame.semantic))

    def load(self, vertex, semantic):
        self.frame.upload(0, vertex)
        self.frame.upload(2, semantic)
        return self.frame

    def describe(self, pp, vertex, semantic):
        """the library's cells and norms of a hand-made frame"""
        idx = core.PlaceIndex(pp)
        idx.addFrame(self.ctx, self.load(vertex, semantic), 7)
        cells, norms, ids = idx.download()
        assert ids.tolist() == [7] and idx.size() == 1
        idx.close()
        return cells[0], norms[0]


@pytest.fixture(scope="module")
def small():
    return Small()


def check_descriptor(shim, small, pp, vertex, semantic, where=""):
    cells, norms = small.describe(pp, vertex, semantic)
    want = pc.shim_describe(shim, vertex, semantic, pp)
    assert cells.tobytes() == want.tobytes(), (where, np.argwhere(cells != want)[:5])
    assert norms.tobytes() == pc.shim_norms(shim, want).tobytes(), where
    return cells


# ---- 1. descriptors equal the shim to the bit

@pytest.mark.parametrize("RS", [(20, 60), (1, 1), (64, 64), (7, 13)], ids=lambda x: "%dx%d" % x)
def test_descriptors_equal_the_shim(shim, small, RS):
    pp = PlaceParams.defaults(rings=RS[0], sectors=RS[1], max_range=50.0)
    filled = 0
    for k, (v, s) in enumerate(small.maps):
        filled += int((check_descriptor(shim, small, pp, v, s, (RS, k)) > 0).sum())
    assert filled >= 6


def test_descriptor_through_add_frame_after_preprocess(shim, small):
    """the frame straight from K1-K3 (side stream, not downloaded in between), six scans into one index"""
    pp = PlaceParams.defaults(max_range=50.0)
    idx = core.PlaceIndex(pp, capacity=8)
    for k, s in enumerate(small.scans):
        small.pre.process(s[0], small.frame, s[1], s[2], 20)
        idx.addFrame(small.ctx, small.frame, 100 + k)
    cells, norms, ids = idx.download()
    assert ids.tolist() == [100 + k for k in range(6)]
    for k, (v, s) in enumerate(small.maps):
        want = pc.shim_describe(shim, v, s, pp)
        assert cells[k].tobytes() == want.tobytes() and norms[k].tobytes() == pc.shim_norms(shim, want).tobytes(), k
    idx.close()


def test_label_mask(shim, small):
    v, s = small.maps[3]
    labels = np.unique((s[..., 0] * f32(255.0) + f32(0.5)).astype(np.int64)[v[..., 3] > 0])
    assert len(labels) >= 2, labels
    whole = check_descriptor(shim, small, PlaceParams.defaults(max_range=50.0), v, s)
    for keep in ([int(labels[0])], [int(l) for l in labels[1:]], []):
        part = check_descriptor(shim, small, PlaceParams.defaults(keep_labels=keep, max_range=50.0), v, s, keep)
        assert np.all(part <= whole) and (len(keep) == 0) == (not part.any())
    check_descriptor(shim, small, PlaceParams.static_only(max_range=50.0), v, s)


def test_empty_and_broken_scans(shim, small):
    pp = PlaceParams.defaults(max_range=50.0)
    small.pre.process(np.zeros((0, 4), f32), small.frame, None, None, 20)
    idx = core.PlaceIndex(pp)
    idx.addFrame(small.ctx, small.frame, 1)
    cells, norms, _ = idx.download()
    assert not cells.any() and not norms.any()
    pts, lab, prob = (np.array(a, copy=True) for a in small.scans[2])
    bad = np.arange(0, len(pts), 7)
    pts[bad[0::3], 0] = np.nan
    pts[bad[1::3], 1] = np.inf
    pts[bad[2::3], 2] = 1e30
    small.pre.process(pts, small.frame, lab, prob, 20)
    idx.addFrame(small.ctx, small.frame, 2)
    v, s = small.frame.vertex, small.frame.semantic
    cells, norms, _ = idx.download(1, 1)
    want = pc.shim_describe(shim, v, s, pp)
    assert cells[0].tobytes() == want.tobytes() and want.any() and np.isfinite(norms).all()
    idx.close()


# ---- 2. hand-made vertex maps

def test_hand_made_vertex_maps(shim, small):
    """R = 4, S = 8, max_range = 8, height_offset = 2: ring edges at d = 2, 4, 6 (the scale is exactly 0.5), sector edges
    at multiples of pi / 4"""
    pp, v, s, at = pc.hand_made_maps(W, H)
    cells = check_descriptor(shim, small, pp, v, s)
    pc.check_hand_made_cells(cells)  # what the specification says about them, by hand
    # an image of nothing but w = 0
    v0 = v.copy()
    v0[..., 3] = 0.0
    assert not check_descriptor(shim, small, pp, v0, s).any()
    # the label mask on a hand-made frame: labels 40 and 10, out-of-range and NaN labels count as 0
    s2 = s.copy().reshape(-1, 4)
    s2[at[::2], 0] = f32(10.0) / f32(255.0)
    s2[at[3], 0], s2[at[9], 0], s2[at[10], 0] = np.nan, f32(2.0), f32(-1.0)
    for keep in ([40], [10], [0], [0, 10, 40]):
        check_descriptor(shim, small, PlaceParams.defaults(keep_labels=keep, rings=4, sectors=8, max_range=8.0), v,
                         s2.reshape(H, W, 4), keep)


# ---- 3. search equals the shim

def frame_from_cells(cells, pp):
    """a vertex map with one texel in the middle of every non-empty cell; -> (vertex, semantic)"""
    S, R = cells.shape
    v = np.zeros((H, W, 4), f32)
    flat = v.reshape(-1, 4)
    assert S * R <= W * H
    for j in range(S):
        for r in range(R):
            if cells[j, r] > 0:
                d, a = (r + 0.5) * pp.max_range / R, (j + 0.5) * 2.0 * np.pi / S
                flat[j * R + r] = d * np.cos(a), d * np.sin(a), cells[j, r] - pp.height_offset, 1.0
    s = np.zeros((H, W, 4), f32)
    return v, s


@pytest.mark.parametrize("RS", [(20, 60), (7, 13)], ids=lambda x: "%dx%d" % x)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 45, 257])
def test_search_equals_the_shim(shim, small, n, RS):
    R, S = RS
    pp = PlaceParams.defaults(rings=R, sectors=S, max_range=50.0)
    db = pc.crafted_database(n, S, R)
    ids = (np.arange(n, dtype=np.uint32) * 3 + 5)
    idx = core.PlaceIndex(pp, capacity=4)
    idx.upload(db[:n // 2], ids[:n // 2])
    idx.upload(db[n // 2:], ids[n // 2:])
    assert idx.size() == n
    cells, norms, got_ids = idx.download()
    assert cells.tobytes() == db.tobytes() and got_ids.tolist() == ids.tolist()
    assert norms.tobytes() == pc.shim_norms(shim, db).tobytes()
    zero = (np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32))
    for name, (v, s) in (("rolled", frame_from_cells(pc.crafted_query(db, S, R), pp)), ("zero", zero),
                         ("copy", frame_from_cells(db[min(3, n - 1)], pp))):
        frame = small.load(v, s)
        q = pc.shim_describe(shim, v, s, pp)
        want_d, want_s = pc.shim_search(shim, db, q)
        dist, shift = idx.queryAll(small.ctx, frame)
        assert dist.tobytes() == want_d.tobytes(), (name, np.argwhere(dist != want_d)[:5])
        assert shift.tolist() == want_s.tolist(), name
        if name == "zero":
            assert np.array_equal(dist, np.ones(n, f32)) and not shift.any()
        for k in (1, 4, 32):
            want = pc.shim_topk(shim, want_d, want_s, ids, k, S)
            assert len(want) == min(k, n)
            got = idx.queryFrame(small.ctx, frame, k)
            pc.matches_equal(got, want, (name, k))
            pc.matches_equal(idx.query(q, k), want, (name, k, "host descriptor"))
            if name == "zero":
                assert [m["index"] for m in got] == list(range(min(k, n)))
        # the exclusion window, in ids: around the best match, everything, nothing (lo > hi)
        best = int(pc.shim_topk(shim, want_d, want_s, ids, 1, S)[0]["id"])
        for window in ((best, best), (best - 3, best + 3), (0, 2 ** 32 - 1), (9, 8), (int(ids[-1]), 2 ** 32 - 1)):
            want = pc.shim_topk(shim, want_d, want_s, ids, 4, S, window)
            pc.matches_equal(idx.queryFrame(small.ctx, frame, 4, exclude=window), want, (name, window))
            assert all(not (window[0] <= m["id"] <= window[1]) for m in want)
    if n >= 45:  # the crafted ties are there: two entries with one distance, kept in index order
        d, _ = pc.shim_search(shim, db, pc.shim_describe(shim, *frame_from_cells(pc.crafted_query(db, S, R), pp), pp))
        assert len(np.unique(d)) < n - n // 7
    idx.close()


def test_query_refusals(small):
    idx = core.PlaceIndex(PlaceParams.defaults(rings=7, sectors=13))
    assert idx.queryFrame(small.ctx, small.frame, 4) == [] and idx.query(np.zeros((13, 7), f32), 4) == []
    for k in (0, 33):
        with pytest.raises(core.SumaError, match="k must be"):
            idx.queryFrame(small.ctx, small.frame, k)
    bad = np.zeros((1, 13, 7), f32)
    for value in (np.nan, -1.0, 1001.0, np.inf):
        bad[0, 3, 2] = value
        with pytest.raises(core.SumaError, match="neither 0 nor"):
            idx.upload(bad, [1])
    assert idx.size() == 0
    with pytest.raises(core.SumaError, match="beyond"):
        idx.download(0, 1)
    idx.close()


# ---- 4. storage

def test_storage_grows_clears_and_round_trips(shim, small, tmp_path):
    pp = PlaceParams.defaults(max_range=50.0)
    S, R = pp.sectors, pp.rings
    idx = core.PlaceIndex(pp, capacity=2)
    db = pc.crafted_database(45, S, R)
    want = []
    for k in range(45):  # frames and host entries in turn; the block grows several times on the way
        if k % 2 == 0:
            v, s = small.maps[k % 6]
            idx.addFrame(small.ctx, small.load(v, s), 1000 + k)
            want.append(pc.shim_describe(shim, v, s, pp))
        else:
            idx.upload(db[k:k + 1], [1000 + k])
            want.append(db[k])
        assert idx.size() == k + 1
    want = np.stack(want)
    cells, norms, ids = idx.download()
    assert cells.tobytes() == want.tobytes() and ids.tolist() == list(range(1000, 1045))
    assert norms.tobytes() == pc.shim_norms(shim, want).tobytes()
    part = idx.download(7, 5)
    assert part[0].tobytes() == want[7:12].tobytes() and part[2].tolist() == list(range(1007, 1012))
    # download -> upload into a fresh index: the same answers
    frame = small.load(*small.maps[1])
    fresh = core.PlaceIndex(pp)
    fresh.upload(cells, ids)
    a, b = idx.queryAll(small.ctx, frame), fresh.queryAll(small.ctx, frame)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist()
    pc.matches_equal(idx.queryFrame(small.ctx, frame, 32), fresh.queryFrame(small.ctx, frame, 32))
    # places.py: one file with params, cells, ids and poses
    poses = np.stack([pc.turned_pose(np.eye(4), 0.01 * k) for k in range(45)])
    path = str(tmp_path / "session.places.npz")
    places.save(path, idx, poses)
    loaded, got_poses = places.load(path)
    assert bytes(loaded.params) == bytes(pp) and got_poses.tobytes() == poses.tobytes() and loaded.size() == 45
    pc.matches_equal(loaded.queryFrame(small.ctx, frame, 32), idx.queryFrame(small.ctx, frame, 32))
    with pytest.raises(ValueError):
        places.save(path, idx, poses[:3])
    # clear: empty, and usable again from entry 0
    idx.clear()
    assert idx.size() == 0 and idx.queryFrame(small.ctx, frame, 4) == []
    idx.upload(db[3:5], [8, 9])
    cells, _, ids = idx.download()
    assert cells.tobytes() == db[3:5].tobytes() and ids.tolist() == [8, 9]
    for x in (idx, fresh, loaded):
        x.close()


# ---- 5, 6, 7: the mapping run

K_CAND = 4
TURNS = ((0, 0.0), (7, 0.0), (31, 2.0))


class Mapped:
    """45 scans mapped by the GPU pipeline once (test_gpu_localize.py's set-up, from localize_common): the trajectory,
    the flat export, and a place index of the even scans -- each scan's frame added right behind the scan -- with the
    mapping poses; max_range = 50"""

    def __init__(self, shim, lshim):
        self.shim, self.lshim = shim, lshim
        self.p = lc.loc_params()
        self.scans = lc.loc_scans()
        self.pp = PlaceParams.defaults(max_range=50.0)
        self.index = core.PlaceIndex(self.pp, capacity=2)
        pipe = core.SurfelMapping(self.p)
        self.poses = []
        for k, s in enumerate(self.scans):
            pipe.processScan(*s)
            self.poses.append(pipe.getCurrentPose())
            if k % 2 == 0:
                self.index.addFrame(pipe.ctx, pipe.frame(0), k)
        self.records = pipe.map.export_world()
        pipe.close()
        self.ids = list(range(0, lc.LOC_SCANS, 2))
        self.entry_poses = np.stack([self.poses[k] for k in self.ids])
        cells, _, ids = self.index.download()
        assert ids.tolist() == self.ids
        self.places = rh.HostPlaces(shim, self.pp, cells, ids, self.entry_poses)
        self.loc = core.Localizer(self.p)    # relocalised; a new setMap forgets its pose
        self.twin = core.Localizer(self.p)   # never relocalises
        self.twin.setMap(self.records)
        self.host = lh.HostLocalizer(self.p, lshim)

    def query(self, k, turn, extra):
        theta = pc.turn_angle(turn, self.pp.sectors, extra)
        return theta, pc.turned_scan(self.scans[k], theta)


@pytest.fixture(scope="module")
def mapped(shim, lshim):
    return Mapped(shim, lshim)


def test_yaw_convention(mapped):
    """scan 10 is entry 5; turned by 7 sectors and matched against the index it finds itself at shift S - 7"""
    S = mapped.pp.sectors
    D = f32(2.0) * pc.PI_F / f32(S)
    loc = mapped.loc
    for turn, want_shift in ((7, S - 7), (0, 0), (31, S - 31)):
        theta, scan = mapped.query(10, turn, 0.0)
        core.Preprocessing(loc.ctx).process(scan[0], loc_frame(loc), scan[1], scan[2], mapped.p.active_timestamps + 10)
        m = mapped.index.queryFrame(loc.ctx, loc_frame(loc), 8)
        assert m[0]["id"] == 10 and m[0]["index"] == 5 and m[0]["shift"] == want_shift, (turn, m[0])
        assert all(m[0]["distance"] <= x["distance"] for x in m) and m[0]["distance"] < 0.05
        want_yaw = -f32(want_shift) * D if want_shift <= S // 2 else f32(S - want_shift) * D
        assert f32(m[0]["yaw"]).tobytes() == f32(want_yaw).tobytes()
        if turn == 7:
            assert f32(m[0]["yaw"]).tobytes() == (f32(7) * D).tobytes()
        hyp = pc.shim_hypothesis(mapped.shim, mapped.entry_poses[m[0]["index"]], m[0]["yaw"])
        assert abs(pc.yaw_difference(pc.turned_pose(mapped.poses[10], theta), hyp)) <= float(D) / 2
        # the exclusion window takes the scan itself out: a neighbour is next
        m2 = mapped.index.queryFrame(loc.ctx, loc_frame(loc), 8, exclude=(10, 10))
        assert m2[0]["id"] in (8, 12) and m2[0]["shift"] == want_shift


_FRAMES = {}


def loc_frame(loc):
    """a data frame on the localiser's ctx (made once)"""
    if id(loc) not in _FRAMES:
        _FRAMES[id(loc)] = core.Frame(loc.ctx, loc.params.data_width, loc.params.data_height)
    return _FRAMES[id(loc)]


@pytest.mark.parametrize("turn", TURNS, ids=lambda t: "turn%d+%g" % t)
@pytest.mark.parametrize("k", [5, 15, 25, 35])
def test_relocalisation(mapped, k, turn):
    """A fresh localiser, no setPose: the odd scans 5, 15, 25, 35 -- none is in the index -- each as it is, turned by 7
    sectors, and turned by 31 sectors plus 2 degrees; max_candidates = 4.  Over the CPU oracle (relocalize_host.py on a
    map the oracle pipeline made) all twelve are found, with these errors against the scan's own mapping pose, in metres:
        scan  5: 0.0204 (turn 0), 0.0205 (7), 0.0204 (31 + 2 deg)      scan 15: 0.0480, 0.0483, 0.0478
        scan 25: 0.0233, 0.0234, 0.0219                                 scan 35: 0.0232, 0.0243, 0.0239
    of 0.55 m of room, and yaw errors below 0.0006 rad.  No query scan had to be replaced.  Wrong places pass both gates
    too (entry 2 for scan 35: error / valid 0.40 against 0.05): the winner is chosen by the objective."""
    theta, scan = mapped.query(k, *turn)
    loc, host, twin = mapped.loc, mapped.host, mapped.twin
    loc.setMap(mapped.records)
    host.set_map(mapped.records)
    got = loc.relocalize(mapped.index, mapped.entry_poses, *scan, max_candidates=K_CAND)
    assert got["found"] and got["n_tried"] == K_CAND
    # the tracking condition: the nearest mapping pose is the query's own
    bad, err = lc.tracking_failures([got["result"]["pose"]] * (k + 1), mapped.poses, first=k)
    yaw_err = pc.yaw_difference(pc.turned_pose(mapped.poses[k], theta), got["result"]["pose"])
    print("scan %d turn %d + %g deg: winner %d (id %d), error %.4f m, yaw error %.5f rad" % (
        k, turn[0], turn[1], got["winner"], got["match"]["id"], err, yaw_err))
    assert not bad, (bad, err)
    assert abs(yaw_err) < 0.02
    # to the bit what the same steps give over the CPU oracle
    want = rh.relocalize(host, mapped.places, *scan, K_CAND)
    rh.relocalized_equal(got, want, (k, turn))
    # every candidate is setPose + processScan
    for c in got["candidates"]:
        twin.setPose(pc.shim_hypothesis(mapped.shim, mapped.entry_poses[c["match"]["index"]], c["match"]["yaw"]))
        lh.results_equal(c["result"], twin.processScan(*scan), (k, turn, c["match"]))
    # the localiser is left in the winner's state: window, and the next scan
    origin, n_window, _ = loc.window()
    assert (origin, n_window) == (host.origin, host.n_window) == (got["result"]["origin"], got["result"]["n_window"])
    assert loc.downloadWindow().tobytes() == host.window.tobytes()
    nxt = pc.turned_scan(mapped.scans[k + 1], theta)
    a, b = loc.processScan(*nxt), host.process_scan(*nxt)
    lh.results_equal(a, b, (k, turn, "next scan"))
    assert a["tracked"] and not lc.tracking_failures([a["pose"]] * (k + 2), mapped.poses, first=k + 1)[0]


def moved(records, dx):
    r = records.copy()
    r["x"] += f32(dx)
    return r


@pytest.mark.parametrize("case", ["empty-scan", "map-1km-away"])
@pytest.mark.parametrize("with_pose", [False, True], ids=["no-pose", "with-pose"])
def test_a_relocalisation_that_finds_nothing(mapped, case, with_pose):
    far = case == "map-1km-away"
    records = moved(mapped.records, 1000.0) if far else mapped.records
    shift = np.eye(4)
    shift[0, 3] = 1000.0 if far else 0.0
    start = shift @ mapped.poses[0]
    loc, twin = core.Localizer(mapped.p), core.Localizer(mapped.p)
    for x in (loc, twin):
        x.setMap(records)
        if with_pose:
            x.setPose(start)
            for s in mapped.scans[:2]:
                r = x.processScan(*s)
            assert r["tracked"]
    before = (loc.window(), loc.downloadWindow().tobytes())
    empty = (np.zeros((0, 4), f32), np.zeros(0, f32), np.zeros(0, f32))
    got = loc.relocalize(mapped.index, mapped.entry_poses, *(mapped.scans[7] if far else empty), max_candidates=K_CAND)
    assert not got["found"] and got["winner"] == -1 and got["match"] is None and got["result"] is None
    assert got["n_tried"] == K_CAND and not any(c["result"]["tracked"] for c in got["candidates"])
    if far:
        assert all(c["result"]["n_window"] == 0 for c in got["candidates"])
    else:  # nothing to compare: distance 1, shift 0, index order
        assert [(c["match"]["index"], c["match"]["distance"], c["match"]["shift"]) for c in got["candidates"]] == \
            [(i, 1.0, 0) for i in range(K_CAND)]
    assert (loc.window(), loc.downloadWindow().tobytes()) == before
    assert loc.window() == twin.window() and loc.downloadWindow().tobytes() == twin.downloadWindow().tobytes()
    if not with_pose:  # it still has no pose
        with pytest.raises(core.SumaError, match="no start pose"):
            loc.processScan(*mapped.scans[2])
        loc.setPose(start)
        twin.setPose(start)
    for s in mapped.scans[2:4]:  # pose, increment and window are as before: the next scans equal the twin's
        lh.results_equal(loc.processScan(*s), twin.processScan(*s), (case, with_pose))
    loc.close()
    twin.close()


def test_relocalize_refusals(mapped):
    loc = core.Localizer(mapped.p)
    scan = mapped.scans[3]
    with pytest.raises(core.SumaError, match="no map"):
        loc.relocalize(mapped.index, mapped.entry_poses, *scan)
    loc.setMap(np.zeros(0, dtype=WORLD_SURFEL_DTYPE))
    with pytest.raises(core.SumaError, match="one pose per entry"):
        loc.relocalize(mapped.index, mapped.entry_poses[:5], *scan)
    for k in (0, 33):
        with pytest.raises(core.SumaError, match="max_candidates"):
            loc.relocalize(mapped.index, mapped.entry_poses, *scan, max_candidates=k)
    empty = core.PlaceIndex(mapped.pp)
    got = loc.relocalize(empty, np.zeros((0, 4, 4)), *scan)
    assert not got["found"] and got["n_tried"] == 0
    empty.close()
    loc.close()
