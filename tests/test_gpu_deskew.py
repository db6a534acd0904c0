"""Motion compensation of raw sweeps on the MI355X (csrc/k_deskew.hip, csrc/suma_deskew.hip): kd_deskew byte for byte
against the host restatement (tests/deskew_shim.c) on crafted points and on every block edge, the pipeline and the
localiser with the correction on to the bit against the same sequence over the CPU oracle (tests/deskew_host.py), off is
off, the refusing entries, the odometry figures on the device's poses, and a checkpoint in the middle of a corrected run."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import deskew_common as dc
import deskew_host as dh
import localize_host as lh
from semantic_suma_amd import core
from semantic_suma_amd.types import (DESKEW_MOTION_INCREMENT, DESKEW_MOTION_NONE, DESKEW_MOTION_OVERRIDE, DESKEW_TIME_TIMES,
                                     DeskewParams)

pytestmark = pytest.mark.gpu

N_PIPE = 25      # scans of the pipeline comparison
K_OVERRIDE = 5   # the scan that gets a one-shot override in every corrected run


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return dc.build_shim(tmp_path_factory.mktemp("deskew_gpu"))


@pytest.fixture(scope="module")
def ctx():
    return core.Context(dc.params())


# ---- 1. the kernel against the shim

def dev_deskew(ctx, pts, motion, dp, times, in_place):
    """through suma_deskew_points_device on torch tensors -> (output, the input buffer afterwards)"""
    n = len(pts)
    d_in = torch.from_numpy(pts.copy()).cuda()
    d_t = None if times is None else torch.from_numpy(times.copy()).cuda()
    d_out = d_in if in_place else torch.full((max(n, 1), 4), 7.0, dtype=torch.float32).cuda()
    torch.cuda.synchronize()
    core.deskew_points_device(ctx, d_in if n else None, motion, n, d_out if n else None, dp, d_t if n else None)
    ctx.synchronize()
    return d_out.cpu().numpy()[:n], d_in.cpu().numpy()


def test_kernel_equals_shim_on_the_crafted_set(shim, ctx):
    """every motion x every case (t_ref, sense, start azimuth, scale, both time sources), host entry and device entry, in
    place and out of place"""
    pts = dc.crafted_points()
    for mname, motion in dc.MOTIONS.items():
        for cname, dp, use_times in dc.cases():
            times = dc.crafted_times(len(pts)) if use_times else None
            want = dc.shim_points(shim, pts, motion, dp, times)
            got = core.deskew_points(ctx, pts, motion, dp, times)
            assert got.tobytes() == want.tobytes(), ("host entry", mname, cname)
            for in_place in (False, True):
                got, src = dev_deskew(ctx, pts, motion, dp, times, in_place)
                assert got.tobytes() == want.tobytes(), ("device entry", mname, cname, in_place)
                if not in_place:
                    assert src.tobytes() == pts.tobytes(), ("the input was written", mname, cname)


@pytest.mark.parametrize("n", dc.BLOCK_EDGES)
def test_kernel_equals_shim_on_the_block_edges(shim, ctx, n):
    pts = dc.tiled(dc.crafted_points(), n) if n else np.zeros((0, 4), dtype=np.float32)
    for mname, motion in dc.MOTIONS.items():
        for use_times in (False, True):
            dp = DeskewParams.defaults(time_source=DESKEW_TIME_TIMES) if use_times else DeskewParams.defaults(start_azimuth=0.7)
            times = dc.crafted_times(max(n, 10))[:n] if use_times else None
            want = dc.shim_points(shim, pts, motion, dp, times) if n else pts
            assert core.deskew_points(ctx, pts, motion, dp, times).tobytes() == want.tobytes(), (mname, use_times)
            for in_place in (False, True):
                got, src = dev_deskew(ctx, pts, motion, dp, times, in_place)
                assert got.tobytes() == want.tobytes(), (mname, use_times, in_place)
                if not in_place:
                    assert src.tobytes() == pts.tobytes()


def test_refused_parameters_on_the_device(ctx):
    pts = dc.crafted_points()[:8]
    for dp, motion, times in ((DeskewParams.defaults(t_ref=1.5), np.eye(4), None),
                              (DeskewParams.defaults(scale=float("nan")), np.eye(4), None),
                              (DeskewParams.defaults(time_source=DESKEW_TIME_TIMES), np.eye(4), None),
                              (None, np.full((4, 4), np.nan), None)):
        with pytest.raises(core.SumaError, match=r"\(-1\)"):
            core.deskew_points(ctx, pts, motion, dp, times)
    assert len(core.deskew_points(ctx, np.zeros((0, 4), dtype=np.float32), dc.MOTIONS["general"])) == 0  # n = 0 is fine


# ---- 2 .. 5, 7: the pipeline

def drive(pipe, k, host=False):
    """scan k of a corrected run: the override on scan K_OVERRIDE, raw sweeps throughout"""
    if k == K_OVERRIDE:
        (pipe.set_deskew_motion if host else pipe.setDeskewMotion)(dc.true_motion(k))
    return dc.raw_scan(k)


def frame_bytes(pipe):
    f = pipe.frame(0)
    return [f.download(m).tobytes() for m in range(3)]


class Runs:
    """the corrected run over the CPU oracle and on the GPU (N_PIPE scans, alternating the device and the host entry),
    each made once and shared"""

    def __init__(self, shim):
        self.shim = shim
        h = dh.HostPipeline(dc.params(), shim)
        h.enable_deskew()
        self.host = []
        for k in range(N_PIPE):
            h.process_scan(*drive(h, k, host=True))
            self.host.append(dict(pose=h.pose(), inc=h.last_increment(), stats=h.stats(),
                                  frame=[a.tobytes() for a in h.frame_maps(0)], motion=h.deskew_motion()))
        pipe = core.SurfelMapping(dc.params())
        pipe.enableDeskew()
        self.gpu, self.untouched = [], True
        for k in range(N_PIPE):
            pts, lab, prob = drive(pipe, k)
            if k % 2 == 0:
                d = [pipe.ctx.device_array(a) for a in (pts, lab, prob)]
                pipe.processScanDevice(d[0], d[1], d[2], len(pts))
                pipe.ctx.synchronize()
                self.untouched &= pipe.ctx.device_download(d[0], pts.nbytes).tobytes() == pts.tobytes()
                for a in d:
                    pipe.ctx.device_free(a)
            else:
                pipe.processScan(pts, lab, prob)
            self.gpu.append(dict(pose=pipe.getCurrentPose(), inc=pipe.lastIncrement(), stats=pipe.lastStats().as_dict(),
                                 frame=frame_bytes(pipe), motion=pipe.deskewMotion()))
        pipe.close()


@pytest.fixture(scope="module")
def runs(shim):
    return Runs(shim)


def off_run(n, toggle):
    pipe = core.SurfelMapping(dc.params())
    if toggle:
        pipe.enableDeskew()
        pipe.disableDeskew()
    out = []
    for k in range(n):
        pipe.processScan(*dc.raw_scan(k))
        out.append((pipe.getCurrentPose().tobytes(), pipe.lastIncrement().tobytes(), frame_bytes(pipe)))
    surfels = pipe.map.getAllSurfels().tobytes()
    motion = pipe.deskewMotion()
    pipe.close()
    return out, surfels, motion


def test_pipeline_equals_the_restatement(runs):
    """every pose, increment, statistic and the three maps of the current frame, scan by scan, to the bit"""
    for k, (g, h) in enumerate(zip(runs.gpu, runs.host)):
        assert g["pose"].tobytes() == h["pose"].tobytes(), k
        assert g["inc"].tobytes() == h["inc"].tobytes(), k
        sg, sh = dict(g["stats"]), dict(h["stats"])
        for key in ("error", "inlier_residual"):
            assert np.float64(sg.pop(key)).tobytes() == np.float64(sh.pop(key)).tobytes(), (k, key)
        assert sg == sh, (k, sg, sh)
        assert g["frame"] == h["frame"], k
    assert runs.untouched, "the caller's device points were written"


def test_the_motion_reported(runs):
    """deskewMotion gives the increment before the scan, and the override once"""
    for k, (g, h) in enumerate(zip(runs.gpu, runs.host)):
        motion, source = g["motion"]
        assert motion.tobytes() == h["motion"][0].tobytes() and source == h["motion"][1], k
        if k == K_OVERRIDE:
            assert source == DESKEW_MOTION_OVERRIDE and np.array_equal(motion, dc.true_motion(k))
        else:
            assert source == DESKEW_MOTION_INCREMENT
            assert np.array_equal(motion, runs.gpu[k - 1]["inc"] if k else np.eye(4)), k


def test_off_is_off_and_scan_0_is_untouched(runs):
    """never enabled == enabled and disabled before the first scan, to the bit; and with the correction on the first scan
    (identity motion, nothing launched) equals the uncorrected run's"""
    a, sa, ma = off_run(N_PIPE, False)
    b, sb, mb = off_run(N_PIPE, True)
    assert a == b and sa == sb
    assert ma[1] == DESKEW_MOTION_NONE and mb[1] == DESKEW_MOTION_NONE and np.array_equal(ma[0], np.eye(4))
    g = runs.gpu[0]
    assert (g["pose"].tobytes(), g["inc"].tobytes(), g["frame"]) == a[0]
    assert runs.gpu[3]["frame"] != a[3][2]  # and later scans are corrected


def test_refusals_while_enabled(runs):
    """each entry that hands a scan over before the previous pose exists returns SUMA_ERR_INVALID and changes nothing: the
    next blocking scan still gives the restatement's bits"""
    from semantic_suma_amd import segmentation
    pipe = core.SurfelMapping(dc.params())
    pipe.enableDeskew()
    for k in range(3):
        pipe.processScan(*dc.raw_scan(k))
    pts, lab, prob = dc.raw_scan(3)
    L, h = pipe.L, pipe.h
    sp = segmentation.semantic_params(64, 16, 3.0, -25.0, [0.0] * 5, [1.0] * 5)
    knn = segmentation.semantic_knn()
    d = torch.zeros(64 * 16 * 20, dtype=torch.float32).cuda()
    di = torch.zeros(1024, dtype=torch.int32).cuda()
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    job = pipe.prepareScans([(pts, lab, prob)], False)
    calls = {
        "prefetch_scan": lambda: L.suma_pipeline_prefetch_scan(h, core._ptr(pts), core._ptr(lab), core._ptr(prob), len(pts)),
        "process_prefetched": lambda: L.suma_pipeline_process_prefetched(h, 0),
        "begin_prefetched": lambda: L.suma_pipeline_begin_prefetched(h),
        "process_scan_async": lambda: L.suma_pipeline_process_scan_async(h, core._ptr(pts), core._ptr(lab), core._ptr(prob),
                                                                         len(pts), 0),
        "begin_scan_scores": lambda: L.suma_pipeline_begin_scan_scores(h, C.byref(sp), vp(d), vp(d), 0, vp(di), 16, None),
        "process_scan_scores": lambda: L.suma_pipeline_process_scan_scores(h, C.byref(sp), vp(d), vp(d), 0, vp(di), 16, None, 0),
        "begin_scan_scores_knn": lambda: L.suma_pipeline_begin_scan_scores_knn(h, C.byref(sp), C.byref(knn), vp(d), vp(d), 0,
                                                                               vp(di), vp(di), 16, None),
        "process_scan_scores_knn": lambda: L.suma_pipeline_process_scan_scores_knn(h, C.byref(sp), C.byref(knn), vp(d), vp(d),
                                                                                   0, vp(di), vp(di), 16, None, 0),
        "run_scans": lambda: L.suma_pipeline_run_scans(h, C.byref(job[0]), 0, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert "motion compensation" in L.suma_last_error(pipe.ctx.h).decode(), (name, L.suma_last_error(pipe.ctx.h))
        assert pipe.timestamp() == 3, name
    pipe.processScan(pts, lab, prob)
    assert pipe.getCurrentPose().tobytes() == runs.host[3]["pose"].tobytes()
    assert frame_bytes(pipe) == runs.host[3]["frame"]
    # a bad switch changes nothing either; the scan entries carry no times
    with pytest.raises(core.SumaError, match=r"\(-1\)"):
        pipe.enableDeskew(DeskewParams.defaults(time_source=DESKEW_TIME_TIMES))
    with pytest.raises(core.SumaError, match=r"\(-1\)"):
        pipe.setDeskewMotion(np.full((4, 4), np.inf))
    pipe.processScan(*dc.raw_scan(4))
    assert pipe.getCurrentPose().tobytes() == runs.host[4]["pose"].tobytes()
    # disabled: the entries work again
    pipe.disableDeskew()
    with pytest.raises(core.SumaError, match=r"\(-1\)"):
        pipe.setDeskewMotion(np.eye(4))
    pipe.prefetchScan(*dc.raw_scan(5))
    pipe.processPrefetched()
    assert pipe.timestamp() == 6
    pipe.close()


def test_accuracy_on_the_device():
    """the 60-scan assertions of the CPU oracle's runs (test_deskew_host.py), on the library's poses"""
    err = {}
    for name in ("control", "uncorrected", "corrected"):
        pipe = core.SurfelMapping(dc.params())
        if name == "corrected":
            pipe.enableDeskew()
        poses = []
        for k in range(dc.N_SCANS):
            pipe.processScan(*(dc.control_scan(k) if name == "control" else dc.raw_scan(k)))
            poses.append(pipe.getCurrentPose())
        pipe.close()
        err[name] = dc.odometry_error(poses)[0]
    dc.assert_odometry(err["control"], err["uncorrected"], err["corrected"])


def test_checkpoint_in_a_corrected_run(runs):
    """saved after scan 10 with the correction on, loaded into a fresh pipeline, enabled again: five more scans give the
    uninterrupted run's poses -- the increment is in the image, the switch is not"""
    pipe = core.SurfelMapping(dc.params())
    pipe.enableDeskew()
    for k in range(11):
        pipe.processScan(*drive(pipe, k))
    image = pipe.save()
    pipe.close()
    fresh = core.SurfelMapping(dc.params())
    fresh.load(image)
    assert fresh.deskewMotion()[1] == DESKEW_MOTION_NONE  # no deskew state in the image
    fresh.enableDeskew()
    for k in range(11, 16):
        fresh.processScan(*drive(fresh, k))
        assert fresh.getCurrentPose().tobytes() == runs.gpu[k]["pose"].tobytes(), k
        assert fresh.deskewMotion()[0].tobytes() == runs.gpu[k - 1]["inc"].tobytes(), k
    fresh.close()


# ---- 6. the localiser

def test_localiser_equals_the_restatement(shim, tmp_path_factory):
    """20 raw sweeps localised in the map of the instantaneous scans, correction, evidence and novelty on: every result
    to the bit, and every observation and collection -- they read the corrected frame"""
    import change_common as cc
    import localize_common as lc
    import novel_common as nc
    p = dc.params(submap_extent=10.0, submap_dimension=2)
    pipe = core.SurfelMapping(p)
    poses = []
    for k in range(45):
        pipe.processScan(*dc.control_scan(k))
        poses.append(pipe.getCurrentPose())
    records = pipe.map.export_world()
    pipe.close()
    tmp = tmp_path_factory.mktemp("deskew_loc")
    host = dh.HostMaintLocalizer(p, lc.build_shim(tmp), cc.build_shim(tmp), nc.build_shim(tmp), shim)
    loc = core.Localizer(p)
    loc.enableEvidence()
    loc.enableNovelty()
    assert loc.setMap(records) == host.set_map(records) == 0
    loc.setPose(poses[20])
    host.set_pose(poses[20])
    loc.enableDeskew()
    host.enable_deskew()
    assert loc.deskewMotion()[1] == DESKEW_MOTION_NONE
    for k in range(20, 40):
        if k < 22:  # no increment yet: the motion of the mapping run, as a host with odometry gives it
            m = np.linalg.inv(poses[k - 1]) @ poses[k]
            loc.setDeskewMotion(m)
            host.set_deskew_motion(m)
        want = host.process_scan(*dc.raw_scan(k))
        got = loc.processScan(*dc.raw_scan(k))
        lh.results_equal(got, want, k)
        assert got["tracked"], k
        assert loc.lastObservation() == (want["observation"], want["observed"]), k
        assert loc.lastCollection() == (want["collection"], want["collected"]), k
        motion, source = loc.deskewMotion()
        assert source == host.deskew_motion()[1] == (DESKEW_MOTION_OVERRIDE if k < 22 else DESKEW_MOTION_INCREMENT)
        assert motion.tobytes() == host.deskew_motion()[0].tobytes(), k
    assert loc.evidence().tobytes() == host.evidence.tobytes()
    assert loc.novelCandidates().tobytes() == host.candidates().tobytes()
    # relocalize does not correct; disabling drops a pending override
    loc.setDeskewMotion(np.eye(4))
    loc.disableDeskew()
    with pytest.raises(core.SumaError, match=r"\(-1\)"):
        loc.setDeskewMotion(np.eye(4))
    loc.close()
