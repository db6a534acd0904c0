"""suma_localizer_* on the MI355X (csrc/k_localize.hip, csrc/suma_localize.hip, core.Localizer): the window byte for byte
against the host restatement (tests/localize_shim.c), every scan's result to the bit against the whole localiser over the
CPU oracle (tests/localize_host.py) and against the same sequence made by hand from the class-by-class entries, the
tracking condition against the mapping pipeline's trajectory, no side effects, no length limit, refusals."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import localize_common as lc
import localize_host as lh
from loop_closing_host import mul4, rigid_inv
from semantic_suma_amd import core
from semantic_suma_amd.types import LocalizerParams, LocalizerResult, SURFEL_DTYPE, WORLD_SURFEL_DTYPE

pytestmark = pytest.mark.gpu

E, DIM = 10.0, 2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return lc.build_shim(tmp_path_factory.mktemp("localize_gpu"))


@pytest.fixture(scope="module")
def loc():
    return core.Localizer(lc.loc_params())


def pose_at(x, y, z=0.0, yaw=0.3):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = x, y, z
    return T


def check_window(loc, m, where=""):
    """the localiser's window equals the shim's around the same origin; returns (origin, n_window, rebuilds)"""
    origin, n, rebuilds = loc.window()
    want = m.window(origin[0], origin[1], DIM)
    got = loc.downloadWindow()
    assert n == len(want), (where, origin, n, len(want))
    assert got.dtype == SURFEL_DTYPE and got.tobytes() == want.tobytes(), (where, origin, n)
    return origin, n, rebuilds


# poses on, beside and across the tile edges in x, in y and diagonally; the cell each lies in comes from the shim
WALK = [(0.0, 0.0), (9.99999, 0.0), (10.0, 0.0), (10.00001, 0.0), (30.0, 0.25), (-10.0, 0.0), (-10.00001, 0.0),
        (0.0, 9.99999), (0.0, 10.0), (0.25, -10.0), (0.0, -30.0), (10.0, 10.0), (-10.00001, 29.9999), (25.0, -25.0),
        (-50.0, 50.0), (70.0, 70.0), (1.0e6, -1.0e6), (0.0, 0.0)]


@pytest.mark.parametrize("spread", [3.6, 1.2])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025])
def test_window_equals_shim(shim, loc, n, spread):
    plain = lc.crafted_records(n, E, spread=spread)
    for records in (plain, np.concatenate([lc.edge_records(E)[::2], plain, lc.edge_records(E)[1::2]])):
        m = lc.ShimMap(shim, records, E)
        assert loc.setMap(records) == m.n_dropped
        assert loc.window() == ((0, 0), 0, 0) or loc.window()[1:] == (0, 0)
        cells = set()
        for k, (x, y) in enumerate(WALK):
            loc.setPose(pose_at(x, y))
            origin, nw, rebuilds = check_window(loc, m, (n, spread, x, y))
            assert origin == lc.shim_cell(shim, E, x, y) and rebuilds == k + 1
            cells.add(origin)
        assert len(cells) >= 12
        if spread == 1.2 and len(records) == n:  # the whole map lies inside the window around the origin
            assert nw == n


def test_a_device_map_is_binned_like_a_host_map(shim, loc):
    records = np.concatenate([lc.crafted_records(5000, E), lc.edge_records(E)])
    m = lc.ShimMap(shim, records, E)
    t = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    assert loc.setMapDevice(t, len(records)) == m.n_dropped == 8
    for x, y in ((0.0, 0.0), (-35.0, 41.0)):
        loc.setPose(pose_at(x, y))
        check_window(loc, m)
    assert t.cpu().numpy().tobytes() == records.tobytes()


# ---- localisation in the map of a mapping run

class Mapped:
    """45 scans mapped by the GPU pipeline once, its trajectory and exported maps; the localisation runs on the GPU and
    over the CPU oracle, each made once and shared by the tests"""

    def __init__(self, shim):
        self.shim = shim
        self.p = lc.loc_params()
        self.scans = lc.loc_scans()
        pipe = core.SurfelMapping(self.p)
        self.poses = []
        for s in self.scans:
            pipe.processScan(*s)
            self.poses.append(pipe.getCurrentPose())
        self.maps = {0.0: pipe.map.export_world(), 0.1: pipe.map.export_world(voxel_size=0.1)}
        pipe.close()
        self.gpu, self.host, self.kept = {}, {}, {}

    def setting(self, key):
        """-> (records, start pose, scans, fixed_iterations, params); a name that ends in "-still" runs without the motion
        model (constant_velocity = 0)"""
        name, n, fi = key
        name = name.replace("-still", "")
        records, start = self.maps[0.1 if name == "voxel" else 0.0], self.poses[0]
        if name == "perturbed":
            start = lc.perturbed(start)
        if name.startswith("yaw"):  # the same world turned about z: the walk crosses tile edges in y / diagonally
            a = np.deg2rad(float(name[3:]))
            R = np.eye(4)
            R[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            Rf = R[:3, :3].astype(np.float32)
            records = records.copy()
            xyz = np.stack([records["x"], records["y"], records["z"]], 1) @ Rf.T
            nrm = np.stack([records["nx"], records["ny"], records["nz"]], 1) @ Rf.T
            records["x"], records["y"], records["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            records["nx"], records["ny"], records["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
            start = R @ start
        return records, start, self.scans[:n], fi, self.p

    def loc_params(self, key):
        return LocalizerParams.defaults(self.p, constant_velocity=0 if key[0].endswith("-still") else 1)

    def gpu_run(self, key, params=None):
        if key not in self.gpu or params is not None:
            records, start, scans, fi, p = self.setting(key)
            loc = core.Localizer(p if params is None else params, self.loc_params(key))
            t = torch.from_numpy(records.view(np.uint8).copy()).cuda()  # the caller's device buffer: only read
            loc.setMapDevice(t, len(records))
            loc.setPose(start)
            res = [loc.processScan(*s, fixed_iterations=fi) for s in scans]
            out = (res, loc.window(), loc.downloadWindow())
            if params is not None:
                return out
            self.gpu[key] = out
            self.kept[key] = (t, records)
            loc.close()
        return self.gpu[key]

    def host_run(self, key):
        if key not in self.host:
            records, start, scans, fi, p = self.setting(key)
            h = lh.HostLocalizer(p, self.shim, self.loc_params(key))
            h.set_map(records)
            h.set_pose(start)
            self.host[key] = ([h.process_scan(*s, fixed_iterations=fi) for s in scans], h)
        return self.host[key]


@pytest.fixture(scope="module")
def mapped(shim):
    return Mapped(shim)


FLAT, VOXEL, PERTURBED = ("flat", 45, 0), ("voxel", 45, 0), ("perturbed", 45, 0)


@pytest.mark.parametrize("key", [FLAT, VOXEL, ("flat", 10, 10), ("yaw90", 14, 0), ("yaw45", 18, 0), ("flat-still", 45, 0)],
                         ids=lambda k: "%s-%d-%d" % k)
def test_equals_the_host_restatement(mapped, key):
    """pose, increment, statistics, ratios, gates, origin, rebuilds and window size of every scan, to the bit"""
    got, (origin, n_window, rebuilds), window = mapped.gpu_run(key)
    want, h = mapped.host_run(key)
    for k, (a, b) in enumerate(zip(got, want)):
        lh.results_equal(a, b, (key, k))
    assert (origin, n_window, rebuilds) == (h.origin, h.n_window, h.rebuilds)
    assert window.tobytes() == h.window.tobytes()
    moved = sum(r["window_rebuilt"] for r in got)
    assert moved == rebuilds - 1
    if key[1] == 45:
        assert moved >= 2, moved
    if key[0] == "yaw90":
        assert moved >= 1 and origin[1] != got[0]["origin"][1], (origin, got[0]["origin"])
    if key[0] == "yaw45":
        assert origin[0] != got[0]["origin"][0] and origin[1] != got[0]["origin"][1], (origin, got[0]["origin"])


def test_nothing_but_plumbing(mapped):
    """5 scans made by hand on a second ctx from the class-by-class entries give the same bits"""
    p = mapped.p
    records, start, scans, _, _ = mapped.setting(("flat", 5, 0))
    loc = core.Localizer(p)
    loc.setMap(records)
    loc.setPose(start)
    t_loc = p.active_timestamps + 10
    ctx = core.Context(p)
    smap, pre, frame = core.SurfelMap(ctx), core.Preprocessing(ctx), core.Frame(ctx, p.data_width, p.data_height)
    objective, gn = core.Frame2Model(ctx), core.LieGaussNewton(ctx)
    smap.upload(loc.downloadWindow(), t_loc)
    pose, inc = np.asarray(start, dtype=np.float64), np.eye(4)
    for k, s in enumerate(scans):
        r = loc.processScan(*s)
        if r["window_rebuilt"]:
            smap.upload(loc.downloadWindow(), t_loc)
        guess = mul4(pose, inc)
        pre.process(s[0], frame, s[1], s[2], t_loc)
        smap.render_inactive(guess.astype(np.float32), p.confidence_threshold)
        objective.setData(frame, smap.oldMapFrame())
        gn.minimize(objective, np.eye(4))
        new = lh.orthonormalize(mul4(guess, gn.pose()))
        inc = np.eye(4) if k == 0 else mul4(rigid_inv(pose), new)
        pose = new
        assert r["guess"].tobytes() == guess.tobytes() and r["pose"].tobytes() == pose.tobytes(), k
        assert r["increment"].tobytes() == inc.tobytes(), k
        assert r["stats"] == gn.stats.as_dict() and r["stats"]["valid"] > 1000, (k, r["stats"])
    loc.close()


def tracking(mapped, key):
    res = mapped.gpu_run(key)[0]
    first = 2 if key[0].startswith("perturbed") else 1
    bad, worst = lc.tracking_failures([r["pose"] for r in res], mapped.poses, first=first)
    print(key[0], "scans that fail", bad, "worst error %.4f m" % worst, "untracked", [k for k, r in enumerate(res) if not r["tracked"]])
    return res, bad, worst


@pytest.mark.parametrize("key", [FLAT, VOXEL, PERTURBED], ids=lambda k: k[0])
def test_it_localises(mapped, key):
    """The tracking condition against the mapping pipeline's trajectory, with the default parameters (constant-velocity
    guess): for every scan k >= 1 (perturbed start: k >= 2) the mapping pose nearest to the localised pose is scan k's,
    i.e. the error is below half the 1.1 m between neighbouring scans.  On the CPU oracle the worst errors are 0.086 m
    (flat), 0.103 m (0.1 m voxels) and 0.085 m (start moved by 0.3 m / -0.15 m / 2 degrees).  It holds because the pose is
    kept orthonormal (mat4_orthonormalize): without that the transposes of step 7 feed the rotation's defect back 2.4-fold
    per scan and every such run is lost between scan 36 and 41."""
    res, bad, worst = tracking(mapped, key)
    assert not bad, (bad, worst)
    if key != PERTURBED:
        assert all(r["tracked"] for r in res)


@pytest.mark.parametrize("key", [("flat-still", 45, 0), ("voxel-still", 45, 0), ("perturbed-still", 45, 0)], ids=lambda k: k[0])
def test_it_localises_without_the_motion_model(mapped, key):
    """the same condition with constant_velocity = 0 (guess = the last pose, one 1.1 m step behind): on the CPU oracle the
    worst errors are 0.065 m (flat), 0.057 m (0.1 m voxels) and 0.066 m (perturbed start), and every scan passes both
    gates"""
    res, bad, worst = tracking(mapped, key)
    assert not bad, (bad, worst)
    assert all(r["tracked"] for r in res[2:])
    assert sum(r["window_rebuilt"] for r in res) >= 2


def test_the_callers_records_are_only_read(mapped):
    mapped.gpu_run(FLAT)
    t, records = mapped.kept[FLAT]
    assert t.cpu().numpy().tobytes() == records.tobytes()


def test_no_length_limit(mapped):
    """max_poses = 8 and 20 scans: nothing consumes the pose table, and the poses are those of the default run"""
    res = mapped.gpu_run(("flat", 20, 0), params=lc.loc_params(max_poses=8))[0]
    ref = mapped.gpu_run(FLAT)[0]
    assert len(res) == 20
    for k in range(20):
        assert res[k]["pose"].tobytes() == ref[k]["pose"].tobytes() and res[k]["tracked"], k


def test_capacity_is_refused_and_changes_nothing(mapped):
    records, start, _, _, _ = mapped.setting(FLAT)
    full = mapped.gpu_run(FLAT)[0][0]["n_window"]
    loc = core.Localizer(lc.loc_params(max_surfels=full - 1))
    loc.setMap(records)
    loc.setPose(pose_at(900.0, -900.0))  # an empty window far away is legal
    before = loc.window()
    assert before[1:] == (0, 1)
    with pytest.raises(core.SumaError, match=r"\(-3\).*max_surfels"):
        loc.setPose(start)
    assert loc.window() == before and len(loc.downloadWindow()) == 0
    r = loc.processScan(*mapped.scans[0])  # and it still answers, from where it was
    assert r["n_window"] == 0 and r["origin"] == before[0]
    loc.close()
    ok = core.Localizer(lc.loc_params(max_surfels=full))
    ok.setMap(records)
    ok.setPose(start)
    assert ok.window()[1] == full
    ok.close()


def test_a_pipeline_beside_a_localiser_is_not_disturbed(mapped):
    records, start, scans, _, p = mapped.setting(("flat", 12, 0))
    pipe, loc = core.SurfelMapping(p), core.Localizer(p)
    loc.setMap(records)
    loc.setPose(start)
    ref = mapped.gpu_run(FLAT)[0]
    for k, s in enumerate(scans):
        pipe.processScan(*s)
        r = loc.processScan(*s)
        assert np.array_equal(pipe.getCurrentPose(), mapped.poses[k]), k
        assert r["pose"].tobytes() == ref[k]["pose"].tobytes(), k
    pipe.close()
    loc.close()


def test_refusals(mapped):
    p = mapped.p
    records, start, scans, _, _ = mapped.setting(("flat", 1, 0))
    loc = core.Localizer(p)
    pts, lab, prob = (np.ascontiguousarray(a, dtype=np.float32) for a in scans[0])
    with pytest.raises(core.SumaError, match="no map"):
        loc.processScan(pts, lab, prob)
    with pytest.raises(core.SumaError, match="no map"):
        loc.setPose(start)
    loc.setMap(records)
    with pytest.raises(core.SumaError, match="no start pose"):
        loc.processScan(pts, lab, prob)
    bad = np.array(start)
    bad[1, 3] = np.nan
    with pytest.raises(core.SumaError, match="non-finite"):
        loc.setPose(bad)
    with pytest.raises(core.SumaError, match="outside the tile grid"):
        loc.setPose(pose_at(2.0 * lc.GRID * E, 0.0))
    assert loc.window() == ((0, 0), 0, 0)  # nothing was gathered by the refused calls
    loc.setPose(start)
    L = loc.L
    args = (core._ptr(pts), core._ptr(lab), core._ptr(prob), pts.shape[0], 0)
    assert L.suma_localizer_process_scan(loc.h, *args, None) == -1
    assert "NULL result" in L.suma_last_error(loc.ctx.h).decode()
    res = LocalizerResult()
    assert L.suma_localizer_process_scan(None, *args, C.byref(res)) == -1
    assert L.suma_localizer_set_map(loc.h, None, 5, None) == -1
    r = loc.processScan(pts, lab, prob)  # the refused calls left it usable
    assert r["tracked"] and r["stats"]["valid"] > 1000
    loc.close()


def test_an_empty_map_is_legal(mapped):
    loc = core.Localizer(mapped.p)
    assert loc.setMap(np.zeros(0, dtype=WORLD_SURFEL_DTYPE)) == 0
    start = mapped.poses[3]
    loc.setPose(start)
    assert loc.window() == (loc.window()[0], 0, 1) and len(loc.downloadWindow()) == 0
    for s in mapped.scans[:2]:
        r = loc.processScan(*s)
        assert r["stats"]["valid"] == 0 and not r["tracked"] and r["n_window"] == 0
        assert r["pose"].tobytes() == r["guess"].tobytes() == np.asarray(start, dtype=np.float64).tobytes()
        assert np.isnan(r["valid_ratio"]) and np.isnan(r["outlier_ratio"])
    loc.close()
