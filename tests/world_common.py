"""Shared by the world-export tests (test_world_host.py, test_gpu_world.py): the host restatement tests/world_shim.c,
the source sequence of a map and the pose table as the ctx keeps it."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd.types import SURFEL_DTYPE, WORLD_SURFEL_DTYPE, WorldParams, WorldStats

HERE = os.path.dirname(os.path.abspath(__file__))


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "world_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "world_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.world_shim.argtypes = [vp, u32, vp, u32, C.POINTER(WorldParams), vp, u32, C.POINTER(WorldStats), vp]
    L.world_shim_transform.argtypes = [vp, u32, vp, u32, vp, vp]
    L.world_shim_transform.restype = None
    L.world_shim_label.argtypes = [C.c_float]
    L.world_shim_label.restype = u32
    L.world_shim_weight.argtypes = [C.c_float]
    L.world_shim_weight.restype = u32
    return L


def pose_table(poses, n_poses):
    """[n, 4, 4] row-major -> the column-major table of n_poses entries the ctx keeps (identity behind the given ones)"""
    table = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    if table.shape[0] < n_poses:
        pad = np.tile(np.eye(4, dtype=np.float32), (n_poses - table.shape[0], 1, 1))
        table = np.ascontiguousarray(np.concatenate([table, pad]))
    return table[:n_poses]


def shim_export(shim, sources, poses, n_poses, wp=None, capacity=None, **kw):
    """-> (WORLD_SURFEL_DTYPE records, dict(n_passed, n_dropped, n_out), uint64 keys); wp: a WorldParams, or the keywords
    of WorldParams.defaults; capacity: None = everything"""
    wp = WorldParams.defaults(**kw) if wp is None else wp
    src = np.ascontiguousarray(sources, dtype=SURFEL_DTYPE)
    table = pose_table(poses, n_poses)
    cap = src.shape[0] if capacity is None else capacity
    out = np.zeros(cap, dtype=WORLD_SURFEL_DTYPE)
    keys = np.zeros(cap, dtype=np.uint64)
    st = WorldStats()
    rc = shim.world_shim(src.ctypes.data, src.shape[0], table.ctypes.data, n_poses, C.byref(wp), out.ctypes.data, cap,
                         C.byref(st), keys.ctypes.data)
    assert rc == 0, rc
    m = min(cap, st.n_out)
    return out[:m], dict(n_passed=st.n_passed, n_dropped=st.n_dropped, n_out=st.n_out), keys[:m]


def shim_transform(shim, sources, poses, n_poses):
    src = np.ascontiguousarray(sources, dtype=SURFEL_DTYPE)
    table = pose_table(poses, n_poses)
    p, n = np.zeros((src.shape[0], 4), np.float32), np.zeros((src.shape[0], 4), np.float32)
    shim.world_shim_transform(src.ctypes.data, src.shape[0], table.ctypes.data, n_poses, p.ctypes.data, n.ctypes.data)
    return p, n


def source_sequence(smap):
    """getAllSurfels() ++ cached_tile(i, j) over cached_tiles(): (records, tiles, parked count)"""
    parts = [smap.getAllSurfels()]
    tiles = smap.cached_tiles()
    for i, j in tiles:
        t = np.ascontiguousarray(smap.cached_tile(i, j)).view(SURFEL_DTYPE).reshape(-1)
        assert t.shape[0] > 0, (i, j)
        parts.append(t)
    src = np.concatenate(parts)
    return src, tiles, src.shape[0] - parts[0].shape[0]


def labels_of(sources):
    """the label rule in numpy fp32"""
    t = sources["r"].astype(np.float32) * np.float32(255.0) + np.float32(0.5)
    ok = np.isfinite(t) & (t >= 0) & (t < 260)
    return np.where(ok, np.where(ok, t, 0).astype(np.uint32), 0).astype(np.uint32)


def weights_of(sources):
    w = sources["w"].astype(np.float32)
    c = np.where(w > 0, np.minimum(w, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return np.rint(c * np.float32(65535.0)).astype(np.uint64)


def voxel_index(xyz, voxel_size):
    """floorf(p / voxel_size) per axis in fp32, as int64"""
    return np.floor(xyz.astype(np.float32) / np.float32(voxel_size)).astype(np.int64)


def key_of(ijk):
    return ((ijk[:, 0] + (1 << 20)).astype(np.uint64) << np.uint64(42)) | \
           ((ijk[:, 1] + (1 << 20)).astype(np.uint64) << np.uint64(21)) | (ijk[:, 2] + (1 << 20)).astype(np.uint64)
