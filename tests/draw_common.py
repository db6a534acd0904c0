"""Shared by the SurfelMap::draw tests (test_draw_host.py, test_gpu_draw.py) and tests/golden/make_gl_draw_golden.py:
the host restatement tests/draw_shim.c, a synthetic surfel map and the cameras the tests look through."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd import core, kitti
from semantic_suma_amd.types import SURFEL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "draw_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "draw_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.draw_shim.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.draw_shim_raster.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp]
    return L


def cm_poses(poses):
    """[n, 4, 4] row-major -> the column-major table the ctx keeps"""
    return np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))


def shim_draw(shim, surfels, poses, dp, n_poses=None):
    """-> (uint8 [H, W, 4], int32 [H, W]) in glReadPixels order (row 0 = bottom); n_poses: the size of the pose table
    the ctx keeps (max_poses) -- int(count) is clamped to it -- default len(poses)"""
    surfels = np.ascontiguousarray(surfels, dtype=SURFEL_DTYPE)
    table = cm_poses(poses)
    n_poses = table.shape[0] if n_poses is None else n_poses
    if table.shape[0] < n_poses:
        pad = np.tile(np.eye(4, dtype=np.float32), (n_poses - table.shape[0], 1, 1))
        table = np.ascontiguousarray(np.concatenate([table, pad]))
    W, H = int(dp.width), int(dp.height)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    ids = np.zeros((H, W), dtype=np.int32)
    rc = shim.draw_shim(C.byref(dp), surfels.ctypes.data if surfels.size else None, surfels.shape[0],
                        table.ctypes.data, n_poses, rgba.ctypes.data, ids.ctypes.data)
    assert rc == 0, rc
    return rgba, ids


LABELS = [10, 40, 44, 48, 50, 51, 70, 71, 72, 80, 81, 30]


def planar_map(n, seed=3, extent=30.0, n_poses=4):
    """n surfels on planar patches (ground z = -1.73 and vertical walls) within +-extent m around the origin, in the
    sensor frames of n_poses poses (returned row-major), with SemanticKITTI labels, packed colours and confidences"""
    rng = np.random.default_rng(seed)
    poses = np.tile(np.eye(4), (n_poses, 1, 1))
    for k in range(n_poses):
        a = 0.05 * k
        poses[k, :3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        poses[k, :3, 3] = [1.5 * k, 0.3 * k, 0.0]
    s = np.zeros(n, dtype=SURFEL_DTYPE)
    world = rng.uniform(-extent, extent, (n, 2))
    ground = rng.random(n) < 0.6
    z = np.where(ground, -1.73 + rng.normal(0.0, 0.03, n), rng.uniform(-1.7, 4.0, n))
    ang = np.arctan2(-world[:, 1], -world[:, 0])
    nrm = np.stack([np.where(ground, 0.0, np.cos(ang)), np.where(ground, 0.0, np.sin(ang)), np.where(ground, 1.0, 0.0)], 1)
    count = rng.integers(0, n_poses, n)
    pw = np.concatenate([world, z[:, None], np.ones((n, 1))], 1)
    inv = np.linalg.inv(poses)
    pl = np.einsum("nij,nj->ni", inv[count], pw)
    nl = np.einsum("nij,nj->ni", inv[count, :3, :3], nrm)
    s["x"], s["y"], s["z"] = pl[:, 0], pl[:, 1], pl[:, 2]
    s["nx"], s["ny"], s["nz"] = nl[:, 0], nl[:, 1], nl[:, 2]
    s["radius"] = rng.uniform(0.1, 0.6, n)
    s["confidence"] = rng.uniform(-2.0, 12.0, n)
    s["timestamp"] = count
    s["count"] = count.astype(np.float32)
    s["weight"] = 1.0
    rgb = rng.integers(0, 256, (n, 3))
    s["color"] = (rgb[:, 0] * 65536 + rgb[:, 1] * 256 + rgb[:, 2]).astype(np.float32)
    lab = np.asarray(LABELS)[rng.integers(0, len(LABELS), n)]
    lab[rng.random(n) < 0.05] = 0
    s["r"] = s["g"] = s["b"] = (lab / 255.0).astype(np.float32)
    s["w"] = rng.uniform(0.5, 1.0, n)
    return s, poses.astype(np.float32)


def chase_camera(pose, W, H, back=12.0, up=6.0):
    """the viewer behind and above the sensor at `pose` (row-major), looking at a point ahead of it: (mvp, view_pos)"""
    pose = np.asarray(pose, dtype=np.float64)
    eye = (pose @ np.array([-back, 0.0, up, 1.0]))[:3]
    target = (pose @ np.array([8.0, 0.0, 0.0, 1.0]))[:3]
    V = core.look_at(core.ROSE2GL[:3, :3] @ eye, core.ROSE2GL[:3, :3] @ target, [0.0, 1.0, 0.0])
    return core.perspective(45.0, W / H, 0.1, 10000.0) @ V @ core.ROSE2GL, eye


def birdseye_camera(center, W, H, half=40.0, height=100.0):
    """orthographic, looking straight down on `center` (map frame), map x up the image"""
    c = np.asarray(center, dtype=np.float64)
    eye = c + np.array([0.0, 0.0, height])
    V = core.look_at(core.ROSE2GL[:3, :3] @ eye, core.ROSE2GL[:3, :3] @ c, core.ROSE2GL[:3, :3] @ np.array([1.0, 0.0, 0.0]))
    a = W / H
    return core.orthographic(-half * a, half * a, -half, half, 0.1, 1000.0) @ V @ core.ROSE2GL, eye


def inside_camera(pos, yaw, W, H, pitch=-0.15):
    """perspective camera at `pos` (map frame) inside the map, looking along `yaw`: surfels straddle its near plane"""
    eye = np.asarray(pos, dtype=np.float64).reshape(3)
    d = np.array([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)])
    V = core.look_at(core.ROSE2GL[:3, :3] @ eye, core.ROSE2GL[:3, :3] @ (eye + d), [0.0, 1.0, 0.0])
    return core.perspective(45.0, W / H, 0.1, 10000.0) @ V @ core.ROSE2GL, eye


def params(mvp, eye, W, H, mode, **kw):
    return core.draw_params(mvp, W, H, eye, color_mode=mode, color_map=kitti.semantic_color_map(), **kw)
