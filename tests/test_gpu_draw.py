"""SurfelMap::draw on the MI355X (csrc/k_draw.hip, suma_map_draw, core.SurfelMap.draw): RGBA8 and ids bit for bit against
the host restatement (tests/draw_shim.c) in every colour mode, on a map a synthetic run built and on the same map after a
pose-graph update; the GL fixture of the reference's own shaders; the empty map; no side effects on a pipeline; a map of
more than 9 M surfels; parameter validation."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import draw_common as dc
import gl_draw_ref
from conftest import get_scan
from semantic_suma_amd import core, kitti
from semantic_suma_amd.types import SURFEL_DTYPE, params_with_size
from test_draw_host import WHITE, load_gl_fixture

pytestmark = pytest.mark.gpu

SIZES = [(1280, 720), (333, 197)]
CAMERAS = ["chase", "birdseye", "inside"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return dc.build_shim(tmp_path_factory.mktemp("draw_gpu"))


@pytest.fixture(scope="module")
def run30():
    """a 30-scan synthetic 64 x 2048 run: the pipeline, its trajectory"""
    p = params_with_size(2048, 64)
    pipe = core.SurfelMapping(p)
    traj = []
    for k in range(30):
        pts, lab, prob, _ = get_scan(k, 2048, True, 64)
        pipe.processScan(pts, lab, prob, fixed_iterations=10)
        traj.append(pipe.getCurrentPose().copy())
    return pipe, p, np.array(traj)


def cameras(traj, W, H):
    centre = traj[:, :3, 3].mean(0)
    return {"chase": dc.chase_camera(traj[-1], W, H),
            "birdseye": dc.birdseye_camera(centre, W, H, half=45.0),
            # standing 0.2 m above the sensor height at scan 15, looking along the trajectory: walls and ground
            # straddle the near plane
            "inside": dc.inside_camera(traj[15][:3, 3] + [0.0, 0.0, 0.2], np.arctan2(traj[15][1, 0], traj[15][0, 0]),
                                       W, H)}


def compare_all(shim, smap, p, label):
    surf, poses = smap.getAllSurfels(), smap.poses()
    assert surf.shape[0] > 10000
    for W, H in SIZES:
        cams = cameras(label["traj"], W, H)
        for cam in CAMERAS:
            mvp, eye = cams[cam]
            for mode in range(6):
                img, ids = smap.draw(mvp, W, H, eye, color_mode=mode, color_map=kitti.semantic_color_map(), ids=True)
                want, want_ids = dc.shim_draw(shim, surf, poses, dc.params(mvp, eye, W, H, mode), n_poses=p.max_poses)
                where = f"{label['name']} {cam} {W}x{H} mode {mode}"
                np.testing.assert_array_equal(ids, want_ids[::-1], err_msg=where + ": ids")
                assert img.tobytes() == want[::-1].tobytes(), where + ": rgba"
                if mode == 2:
                    assert (ids >= 0).mean() > 0.05, where
                    assert ids.max() < surf.shape[0]


def test_bit_exact_against_the_shim_every_mode(shim, run30):
    pipe, p, traj = run30
    compare_all(shim, pipe.map, p, dict(name="30 scans", traj=traj))


def test_bit_exact_after_update_poses(shim, run30):
    """loop-closure deformation: the picture follows the pose table"""
    pipe, p, traj = run30
    smap = pipe.map
    W, H = 333, 197
    mvp, eye = cameras(traj, W, H)["birdseye"]
    before = smap.draw(mvp, W, H, eye, color_mode=2)
    poses = smap.poses()
    bent = poses.copy()
    for k in range(bent.shape[0]):
        a = 0.004 * k
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float32)
        bent[k, :3, :3] = R @ poses[k, :3, :3]
        bent[k, :3, 3] = R @ poses[k, :3, 3] + np.float32(0.02 * k)
    smap.updatePoses(bent)
    after = smap.draw(mvp, W, H, eye, color_mode=2)
    assert np.count_nonzero(np.any(after != before, -1)) > 1000
    compare_all(shim, smap, p, dict(name="after updatePoses", traj=traj))


def test_gl_fixture_of_the_reference_shaders(shim):
    z, s, poses, W, H = load_gl_fixture()
    p = params_with_size(900, 64)
    ctx = core.Context(p)
    smap = core.SurfelMap(ctx)
    smap.upload(s, int(poses.shape[0]))
    smap.updatePoses(poses)
    for mode in (int(m) for m in z["modes"]):
        dp = core.draw_params(z["mvp"], W, H, z["view_pos"], color_mode=mode, color_map=z["color_map"])
        img, ids = smap.draw(z["mvp"], W, H, z["view_pos"], color_mode=mode, color_map=z["color_map"], ids=True)
        want, want_ids = dc.shim_draw(shim, s, poses, dp, n_poses=p.max_poses)
        assert img.tobytes() == want[::-1].tobytes(), f"mode {mode}"
        np.testing.assert_array_equal(ids, want_ids[::-1])
        frac, n = gl_draw_ref.agreement(img[::-1], z[f"gl_mode{mode}"], WHITE)
        assert n > 0.3 * W * H and frac >= 0.97, (mode, frac, n)


def test_empty_map_gives_the_clear_colour_and_repeats_bit_for_bit():
    ctx = core.Context(params_with_size(900, 64))
    smap = core.SurfelMap(ctx)
    mvp, eye = dc.chase_camera(np.eye(4), 333, 197)
    img, ids = smap.draw(mvp, 333, 197, eye, ids=True, clear_color=(0.0, 0.5, 1.0, 1.0))
    assert np.all(ids == -1) and np.all(img == np.array([0, 128, 255, 255], dtype=np.uint8))
    s, poses = dc.planar_map(5000)
    smap.upload(s, 4)
    smap.updatePoses(poses)
    a = smap.draw(mvp, 333, 197, eye, ids=True)
    b = smap.draw(mvp, 333, 197, eye, ids=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (a[1] >= 0).sum() > 1000


def test_draw_after_the_z_buffer_grows(shim):
    """a fresh context draws the smaller image first: the larger one needs a new z-buffer on a used context"""
    p = params_with_size(900, 64)
    smap = core.SurfelMap(core.Context(p))
    s, poses = dc.planar_map(5000)
    smap.upload(s, 4)
    smap.updatePoses(poses)
    surf, table = smap.getAllSurfels(), smap.poses()
    for W, H in reversed(SIZES):
        mvp, eye = dc.chase_camera(np.eye(4), W, H)
        img, ids = smap.draw(mvp, W, H, eye, color_mode=2, ids=True)
        want, want_ids = dc.shim_draw(shim, surf, table, dc.params(mvp, eye, W, H, 2), n_poses=p.max_poses)
        np.testing.assert_array_equal(ids, want_ids[::-1], err_msg=f"{W}x{H}: ids")
        assert img.tobytes() == want[::-1].tobytes(), f"{W}x{H}: rgba"
        assert (ids >= 0).sum() > 1000


def test_draw_device_into_torch_buffers():
    ctx = core.Context(params_with_size(900, 64))
    smap = core.SurfelMap(ctx)
    s, poses = dc.planar_map(5000)
    smap.upload(s, 4)
    smap.updatePoses(poses)
    W, H = 320, 200
    mvp, eye = dc.chase_camera(poses[2], W, H)
    rgba = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    ids = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    smap.draw_device(rgba, ids, mvp, W, H, eye)
    ctx.synchronize()
    img, want_ids = smap.draw(mvp, W, H, eye, ids=True)
    assert rgba.cpu().numpy()[::-1].tobytes() == img.tobytes()
    assert np.array_equal(ids.cpu().numpy()[::-1], want_ids)


def test_no_side_effects_on_a_pipeline():
    p = params_with_size(900, 64)
    W, H = 333, 197

    def run(with_draws):
        pipe = core.SurfelMapping(p)
        poses = []
        for k in range(10):
            pts, lab, prob, _ = get_scan(k, 900, True, 64)
            pipe.processScan(pts, lab, prob, fixed_iterations=10)
            poses.append(pipe.getCurrentPose().copy())
            if with_draws:
                mvp, eye = dc.chase_camera(poses[-1], W, H)
                for mode in (0, 5):
                    img = pipe.map.draw(mvp, W, H, eye, color_mode=mode)
                    assert (img != 255).any()
        return (np.array(poses).tobytes(), pipe.map.getAllSurfels().tobytes(), pipe.map.poses().tobytes(),
                pipe.map.counts(), pipe.lastStats().as_dict(), pipe.map.size())

    a, b = run(False), run(True)
    for k, name in enumerate(("poses", "surfels", "pose table", "counts", "stats", "size")):
        assert a[k] == b[k], name


def big_map(S, seed=7):
    """planar patches within +-88 m (tests/test_gpu_long.py::synthetic_map, after tools/stress_map.py), with labels"""
    rng = np.random.default_rng(seed)
    surf = np.zeros(S, dtype=SURFEL_DTYPE)
    xy = rng.uniform(-88, 88, (S, 2)).astype(np.float32)
    ground = rng.random(S) < 0.7
    surf["x"], surf["y"] = xy[:, 0], xy[:, 1]
    surf["z"] = np.where(ground, -1.73, rng.uniform(-1.7, 4.0, S)).astype(np.float32)
    ang = np.arctan2(-xy[:, 1], -xy[:, 0])
    surf["nx"] = np.where(ground, 0.0, np.cos(ang)).astype(np.float32)
    surf["ny"] = np.where(ground, 0.0, np.sin(ang)).astype(np.float32)
    surf["nz"] = np.where(ground, 1.0, 0.0).astype(np.float32)
    d = np.maximum(np.hypot(xy[:, 0], xy[:, 1]), 2.0)
    surf["radius"] = np.clip(1.41 * d * 0.0019, 0.03, 1.0).astype(np.float32)
    surf["confidence"] = rng.uniform(-1.0, 5.0, S).astype(np.float32)
    surf["weight"] = 1.0
    lab = np.asarray(dc.LABELS, dtype=np.float32)[rng.integers(0, len(dc.LABELS), S)]
    surf["r"] = surf["g"] = surf["b"] = lab / np.float32(255.0)
    surf["w"] = 0.9
    return surf


def test_scale_9m_surfels_from_inside_the_map(shim):
    S = 9_200_000
    p = params_with_size(900, 64, max_surfels=S + 1024, cache_surfels=1 << 20)
    ctx = core.Context(p)
    smap = core.SurfelMap(ctx)
    surf = big_map(S)
    smap.upload(surf, 1)
    W, H = 1920, 1080
    mvp, eye = dc.inside_camera([3.0, 1.0, 0.0], 0.4, W, H)
    img, ids = smap.draw(mvp, W, H, eye, color_mode=5, ids=True)
    assert (ids >= 0).mean() > 0.5 and ids.max() < S
    want, want_ids = dc.shim_draw(shim, surf, np.eye(4, dtype=np.float32)[None],
                                  dc.params(mvp, eye, W, H, 5), n_poses=p.max_poses)
    rng = np.random.default_rng(1)
    sel = rng.integers(0, W * H, 200_000)
    np.testing.assert_array_equal(ids.reshape(-1)[sel], want_ids[::-1].reshape(-1)[sel])
    assert np.array_equal(img.reshape(-1, 4)[sel], want[::-1].reshape(-1, 4)[sel])


@pytest.mark.parametrize("field,value,needle", [("width", 0, "width"), ("width", 8193, "width"),
                                                ("color_mode", 6, "color_mode"), ("num_lights", 11, "num_lights")])
def test_invalid_parameters_are_rejected(field, value, needle):
    ctx = core.Context(params_with_size(900, 64))
    smap = core.SurfelMap(ctx)
    dp = core.draw_params(np.eye(4), 64, 32, (0.0, 0.0, 0.0))
    setattr(dp, field, value)
    buf = torch.zeros(8193 * 32 * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(core.SumaError, match=needle):
        smap.draw_device(buf, None, params=dp)
    rc = ctx.L.suma_map_draw(ctx.h, C.byref(dp), C.c_void_p(buf.data_ptr()), None)
    assert rc == -1 and needle in ctx.L.suma_last_error(ctx.h).decode()
