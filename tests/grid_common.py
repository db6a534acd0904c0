"""Shared by the traversability-grid tests (test_grid_host.py, test_gpu_grid.py, test_gpu_grid_cpp.py): the host
restatement tests/grid_shim.c, crafted world-frame records, and the numpy fp32 statement of the cell index."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd.types import GRID_CELL_DTYPE, WORLD_SURFEL_DTYPE, GridParams, GridStats

HERE = os.path.dirname(os.path.abspath(__file__))
NAN_BITS = 0x7fc00000  # the NaN the grid writes


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "grid_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "grid_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.grid_shim.argtypes = [C.POINTER(GridParams), vp, u32, vp, C.POINTER(GridStats)]
    L.grid_shim_cell.argtypes = [C.POINTER(GridParams), C.c_float, C.c_float, C.c_float]
    L.grid_shim_cell.restype = C.c_int64
    L.grid_shim_weight.argtypes = [C.c_float]
    L.grid_shim_weight.restype = u32
    return L


def shim_grid(shim, records, gp):
    """-> (GRID_CELL_DTYPE cells [height, width], stats dict) of the shim on WORLD_SURFEL_DTYPE records"""
    rec = np.ascontiguousarray(records, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
    cells = np.zeros((gp.height, gp.width), dtype=GRID_CELL_DTYPE)
    st = GridStats()
    rc = shim.grid_shim(C.byref(gp), rec.ctypes.data, rec.shape[0], cells.ctypes.data, C.byref(st))
    assert rc == 0, rc
    return cells, st.as_dict()


def params(width, height, cell_size=0.25, origin=(0.0, 0.0), **kw):
    return GridParams.defaults(cell_size=cell_size, origin=origin, width=width, height=height, **kw)


def scene(n, seed=7, lo=(-1.0, -1.0), hi=(17.0, 9.0)):
    """n records of a street-like scene inside [lo, hi): 60 % ground (labels 40 / 48 / 72, normals near +z, z near
    -1.75 on a dyadic lattice so that thresholds are met exactly now and then), the rest things on it (cars, buildings,
    vegetation up to 4 m, sideways normals).  Confidences are small integers (ties are common), and so are a tenth of the
    probabilities (equal vote sums)."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=WORLD_SURFEL_DTYPE)
    r["x"] = rng.uniform(lo[0], hi[0], n)
    r["y"] = rng.uniform(lo[1], hi[1], n)
    ground = rng.random(n) < 0.6
    r["z"] = np.where(ground, -1.75 + rng.integers(-2, 3, n) / 64.0, -1.75 + rng.integers(0, 257, n) / 64.0)
    r["nz"] = np.where(ground, rng.uniform(0.6, 1.0, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-0.3, 0.3, n))
    r["nx"] = np.sqrt(np.maximum(0.0, 1.0 - r["nz"].astype(np.float64) ** 2))
    r["radius"] = rng.uniform(0.05, 0.5, n)
    r["confidence"] = rng.integers(-2, 6, n)
    r["label"] = np.where(ground, rng.choice([40, 48, 72], n), rng.choice([10, 50, 70, 0], n))
    r["prob"] = np.where(rng.random(n) < 0.1, 0.5, rng.uniform(0.3, 1.0, n))
    r["timestamp"] = rng.integers(0, 50, n)
    r["support"] = 1
    return r


def one(x, y, z, label=40, nz=1.0, conf=1.0, prob=1.0):
    """one record"""
    r = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
    r["x"], r["y"], r["z"], r["label"], r["nz"], r["confidence"], r["prob"], r["support"] = x, y, z, label, nz, conf, prob, 1
    return r


def cell_of(records, gp):
    """the cell of every record in numpy fp32: -2 dropped, -1 outside, else iy * width + ix"""
    x, y, z = (records[k].astype(np.float32) for k in "xyz")
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((x - np.float32(gp.origin_x)) / np.float32(gp.cell_size))
        fy = np.floor((y - np.float32(gp.origin_y)) / np.float32(gp.cell_size))
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    inside = finite & (fx >= 0) & (fx < np.float32(gp.width)) & (fy >= 0) & (fy < np.float32(gp.height))
    c = np.where(inside, np.where(inside, fy, 0).astype(np.int64) * gp.width + np.where(inside, fx, 0).astype(np.int64), -1)
    return np.where(finite, c, -2)


def fit_of(records, cell_size, margin):
    """suma_world_grid_fit in numpy fp32: (origin_x, origin_y, width, height), or None without a finite record"""
    ok = np.isfinite(records["x"]) & np.isfinite(records["y"]) & np.isfinite(records["z"])
    if not ok.any():
        return None
    cs, m = np.float32(cell_size), np.float32(margin)
    out = []
    for a in "xy":
        v = records[a][ok].astype(np.float32)
        lo, hi = np.floor(v.min() / cs), np.floor(v.max() / cs)
        out.append((np.float32((lo - m) * cs), int(np.float32(hi - lo)) + 1 + 2 * margin))
    return float(out[0][0]), float(out[1][0]), out[0][1], out[1][1]
