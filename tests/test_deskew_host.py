"""Motion compensation of raw sweeps on the host (no GPU): the restatement tests/deskew_shim.c of csrc/k_deskew.hip
against fp64 on crafted points, its geometry on a raw sweep of the circle, the odometry of the oracle pipeline on
instantaneous, raw and corrected scans, and the localiser over the CPU oracle on raw scans with the correction off and on
(tests/deskew_host.py).  Every figure is printed before it is asserted; deskew_common.MEASURED holds what was measured."""
import numpy as np
import pytest

import deskew_common as dc
import deskew_host as dh
from loop_scenario import circle_pose
from semantic_suma_amd import synth
from semantic_suma_amd.types import DESKEW_MOTION_INCREMENT, DESKEW_MOTION_NONE, DESKEW_MOTION_OVERRIDE, SURFEL_DTYPE

M = dc.MEASURED


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return dc.build_shim(tmp_path_factory.mktemp("deskew_host"))


# ---- 1. the shim against fp64

def test_shim_equals_fp64_on_crafted_points(shim):
    """worst deviation over the crafted set: 1.1e-5 m (fp32 at 120 m has a spacing of 7.6e-6 m).  Asserted: at most four
    times the measured figure, and -- a condition, not a measurement -- at most 1e-3 m, a twentieth of the generator's
    0.02 m range noise."""
    pts = dc.crafted_points()
    radii = np.linalg.norm(pts[np.isfinite(pts[:, :3]).all(1), :3].astype(np.float64), axis=1)
    assert np.sum(np.abs(radii - 0.5) < 1e-3) > 100 and np.sum(np.abs(radii - 120.0) < 1e-3) > 100
    worst, n_cases = 0.0, 0
    for mname, motion in dc.MOTIONS.items():
        for cname, dp, use_times in dc.cases():
            times = dc.crafted_times(len(pts)) if use_times else None
            out = dc.shim_points(shim, pts, motion, dp, times)
            ref, moved = dc.numpy_deskew(pts, motion, dp, times)
            assert moved.sum() > 600 and (~moved).sum() == 7 + (2 if use_times else 0)
            dev = float(np.abs(out[moved, :3].astype(np.float64) - ref[moved]).max())
            worst, n_cases = max(worst, dev), n_cases + 1
            assert dev <= 1e-3, (mname, cname, dev)
            # exactness: non-finite points keep their bits, the remission always does, the identity changes nothing
            assert out[~moved].tobytes() == pts[~moved].tobytes(), (mname, cname)
            assert out[:, 3].tobytes() == pts[:, 3].tobytes(), (mname, cname)
            if mname == "identity":
                assert out.tobytes() == pts.tobytes(), cname
            elif mname != "rotation_tilted":
                assert not np.array_equal(out[moved, :3], pts[moved, :3])
    print("worst |shim - fp64| over %d cases: %.3e m (MEASURED %.3e)" % (n_cases, worst, M["shim_vs_fp64"]))
    assert n_cases == len(dc.MOTIONS) * 12
    assert worst <= 4.0 * M["shim_vs_fp64"], worst


def test_both_sides_of_the_small_angle_threshold(shim):
    """below it the kernel gets theta = 0 (pure translation), above it the rotation; the two results differ by no more
    than the rotation dropped: 1e-6 rad over 120 m"""
    tw = {}
    for name in ("below_small_angle", "above_small_angle"):
        t = dc.Twist()
        shim.deskew_shim_twist(dc._cm(dc.MOTIONS[name]).ctypes.data, 1.0, t)
        tw[name] = t
    assert tw["below_small_angle"].theta == 0.0 and tw["below_small_angle"].inv_theta == 0.0
    assert tw["above_small_angle"].theta == np.float32(2e-6) and tw["above_small_angle"].inv_theta > 4e5
    assert list(tw["below_small_angle"].v) == [np.float32(1.1), np.float32(0.1), 0.0]
    pts = dc.crafted_points()
    a = dc.shim_points(shim, pts, dc.MOTIONS["below_small_angle"])
    b = dc.shim_points(shim, pts, dc.MOTIONS["above_small_angle"])
    ok = np.isfinite(pts[:, :3]).all(1)
    assert np.abs(a[ok, :3] - b[ok, :3]).max() < 120.0 * 2e-6 + 1e-5


def test_what_u_equal_zero_gives(shim):
    """a point on the start azimuth is the START of a counter-clockwise sweep and the END of a clockwise one"""
    motion = dc.MOTIONS["translation"]
    p = np.array([[5.0, 0.0, 0.0, 1.0]], dtype=np.float32)
    for cw, s in ((0, 0.0), (1, 1.0)):
        for t_ref in (0.0, 0.5, 1.0):
            out = dc.shim_points(shim, p, motion, dc.DeskewParams.defaults(clockwise=cw, t_ref=t_ref))
            want = p[0, :3].astype(np.float64) + (s - t_ref) * motion[:3, 3]
            assert np.abs(out[0, :3] - want).max() < 1e-6, (cw, t_ref, out, want)


# ---- 2. geometry

def _unit(p):
    return p[:, :3] / np.linalg.norm(p[:, :3], axis=1, keepdims=True)


def test_a_corrected_sweep_lies_on_the_instantaneous_scan(shim):
    """sweep 10 of the circle, corrected with the true motion, against the world seen from the mid-sweep pose.  The match
    is per point by nearest direction (azimuth and elevation); so that the generator's own angular sampling (1 degree a
    column: 0.17 m sideways at 10 m) does not swamp the figure, the instantaneous scan is cast eight times as densely and
    without range noise.  Static surfaces: walls and buildings -- the ground plane is the same from every pose of a
    planar motion and says nothing.  Measured: median 0.354 m before, 0.027 m after (the range noise is 0.02 m)."""
    from scipy.spatial import cKDTree
    k = 10
    raw, lab, _ = dc.raw_scan(k)
    ref, lab_ref, _, _ = synth.generate_scan(k, n_azimuth=8 * dc.W, height=8 * dc.H, noise=0.0, pose=circle_pose(k))
    ref = ref[lab_ref == synth.LABEL_BUILDING]
    tree = cKDTree(_unit(ref))
    m = lab == synth.LABEL_BUILDING
    assert m.sum() > 2000
    cor = dc.shim_points(shim, raw, dc.true_motion(k))
    med = []
    for pts in (raw[m], cor[m]):
        _, j = tree.query(_unit(pts))
        med.append(float(np.median(np.linalg.norm(pts[:, :3] - ref[j, :3], axis=1))))
    before, after = med
    print("median distance to the instantaneous scan: %.4f m before, %.4f m after (MEASURED %.4f / %.4f)"
          % (before, after, M["geometry_before"], M["geometry_after"]))
    assert after <= 0.25 * before, (before, after)
    assert after <= 2.0 * M["geometry_after"], after


# ---- 3. the pipeline on the CPU oracle

@pytest.fixture(scope="module")
def runs(shim):
    """the 60-scan circle through the oracle pipeline: instantaneous scans, raw sweeps, raw sweeps with the correction"""
    out = {}
    for name in ("control", "uncorrected", "corrected"):
        hp = dh.HostPipeline(dc.params(), shim)
        if name == "corrected":
            hp.enable_deskew()
        poses, motions = [], []
        for k in range(dc.N_SCANS):
            inc = hp.last_increment()
            hp.process_scan(*(dc.control_scan(k) if name == "control" else dc.raw_scan(k)), fixed_iterations=0)
            poses.append(hp.pose())
            motions.append((inc, hp.deskew_motion()))
        out[name] = (poses, motions)
    return out


def test_correction_restores_the_odometry(runs):
    """mean relative translation error per scan over scans 3 .. 59: 0.0188 m on instantaneous scans, 0.0575 m on raw
    sweeps, 0.0151 m on corrected ones (worst drift from scan 3: 0.23 m, 0.96 m, 0.21 m)"""
    err = {k: dc.odometry_error(v[0]) for k, v in runs.items()}
    print({k: (round(e, 4), round(d, 3)) for k, (e, d) in err.items()})
    dc.assert_odometry(err["control"][0], err["uncorrected"][0], err["corrected"][0])


def test_the_motion_is_the_last_increment(runs):
    poses, motions = runs["corrected"]
    for k, (inc, (motion, source)) in enumerate(motions):
        assert source == DESKEW_MOTION_INCREMENT and np.array_equal(motion, inc), k
    assert np.array_equal(motions[0][1][0], np.eye(4)) and np.array_equal(motions[1][1][0], np.eye(4))
    assert not np.array_equal(motions[2][1][0], np.eye(4))
    # scans 0 and 1 are not corrected (no increment yet), so they equal the uncorrected run's
    for k in (0, 1):
        assert np.array_equal(poses[k], runs["uncorrected"][0][k])
    assert not np.array_equal(poses[2], runs["uncorrected"][0][2])
    assert runs["uncorrected"][1][5][1][1] == DESKEW_MOTION_NONE


def test_the_override_is_used_once(shim):
    hp = dh.HostPipeline(dc.params(), shim)
    hp.enable_deskew()
    hp.process_scan(*dc.raw_scan(0))
    hp.set_deskew_motion(dc.true_motion(1))
    hp.process_scan(*dc.raw_scan(1))
    assert hp.deskew_motion()[1] == DESKEW_MOTION_OVERRIDE and np.array_equal(hp.deskew_motion()[0], dc.true_motion(1))
    inc = hp.last_increment()
    hp.process_scan(*dc.raw_scan(2))
    assert hp.deskew_motion()[1] == DESKEW_MOTION_INCREMENT and np.array_equal(hp.deskew_motion()[0], inc)


# ---- 4. the localiser on the CPU restatement

@pytest.fixture(scope="module")
def localised(shim, tmp_path_factory):
    """the circle mapped from instantaneous scans by the oracle pipeline, exported flat by the export's restatement;
    raw sweeps 20 .. 59 localised in it with the correction off and on.  The localiser has no increment for its first two
    scans (identity after set_pose, identity after the first scan), so the run with the correction gives those two the
    motion of the mapping run through the one-shot override -- what a host with odometry does"""
    import localize_common as lc
    import world_common as wc
    from oracle import pyoracle
    pyoracle.build()
    p = dc.params(submap_extent=10.0, submap_dimension=2)
    op = pyoracle.OraclePipeline(p, threads=8)
    poses = []
    for k in range(dc.N_SCANS):
        op.process_scan(*dc.control_scan(k), fixed_iterations=0)
        poses.append(op.pose().copy())
    parts = [op.ctx.map_surfels()]
    for i in range(-8, 9):
        for j in range(-8, 9):
            t = op.ctx.map_cache_tile(i, j)
            if len(t):
                parts.append(np.ascontiguousarray(t).view(SURFEL_DTYPE).reshape(-1))
    src = np.concatenate(parts)
    table = op.ctx.map_poses(dc.N_SCANS).reshape(dc.N_SCANS, 4, 4).transpose(0, 2, 1)
    records = wc.shim_export(wc.build_shim(tmp_path_factory.mktemp("deskew_world")), src, table, p.max_poses)[0]
    lshim = lc.build_shim(tmp_path_factory.mktemp("deskew_localize"))
    out = {}
    for on in (False, True):
        loc = dh.HostLocalizer(p, lshim, shim)
        assert loc.set_map(records) == 0
        loc.set_pose(poses[20])
        if on:
            loc.enable_deskew()
        res = []
        for k in range(20, dc.N_SCANS):
            if on and k < 22:
                loc.set_deskew_motion(np.linalg.inv(poses[k - 1]) @ poses[k])
            res.append(loc.process_scan(*dc.raw_scan(k)))
        err = [float(np.linalg.norm(r["pose"][:3, 3] - poses[20 + i][:3, 3])) for i, r in enumerate(res)]
        print("correction", "on" if on else "off", np.round(err, 3))
        out[on] = (res, max(err), sum(r["tracked"] for r in res))
    return out


def test_the_localiser_tracks_raw_sweeps_with_the_correction(localised):
    """worst distance to the mapping run's pose of the same scan (scans 20 .. 59) and scans tracked of 40: see
    deskew_common.MEASURED and DESIGN.md 16.  Asserted: every scan tracked with the correction on, and its worst error
    at most 1.5 times the measured one."""
    (_, worst_off, tracked_off), (res_on, worst_on, tracked_on) = localised[False], localised[True]
    print("localiser on raw sweeps: worst error %.4f m off / %.4f m on, tracked %d / %d of %d"
          % (worst_off, worst_on, tracked_off, tracked_on, len(res_on)))
    assert tracked_on == len(res_on) == 40
    assert worst_on <= 1.5 * M["loc_worst_on"], worst_on
    if M["loc_worst_off"] >= 1.5 * M["loc_worst_on"]:  # the restatement showed the factor: then it is asserted
        assert worst_off >= 1.5 * worst_on, (worst_off, worst_on)
