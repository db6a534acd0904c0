"""Shared by the localiser tests (test_localize_host.py, test_gpu_localize.py): the host restatement
tests/localize_shim.c, crafted world maps around every boundary of the specification (csrc/k_localize.hip), the
synthetic mapping run whose exported map is localised in, and the tracking condition."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd.types import SURFEL_DTYPE, WORLD_SURFEL_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))

TILE_DTYPE = np.dtype([("key", "<u8"), ("start", "<u4"), ("count", "<u4")])
GRID = 1 << 20


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "localize_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "localize_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int32, C.c_float
    L.loc_shim_cell.argtypes = [f32, f32, f32, f32, C.POINTER(i32), C.POINTER(i32)]
    L.loc_shim_key.argtypes = [i32, i32]
    L.loc_shim_key.restype = C.c_uint64
    L.loc_shim_bin.argtypes = [vp, u32, f32, vp, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.loc_shim_window.argtypes = [vp, vp, vp, u32, i32, i32, i32, vp, u32]
    L.loc_shim_window.restype = C.c_uint64
    L.loc_shim_recentre.argtypes = [f32, f32, f32, C.POINTER(i32), C.POINTER(i32)]
    return L


def shim_cell(shim, extent, x, y, z=0.0):
    """(i, j) or None for a dropped position"""
    i, j = C.c_int32(0), C.c_int32(0)
    return (i.value, j.value) if shim.loc_shim_cell(extent, x, y, z, C.byref(i), C.byref(j)) else None


def shim_recentre(shim, extent, x, y, oi, oj):
    """-> (moved, oi, oj)"""
    i, j = C.c_int32(oi), C.c_int32(oj)
    moved = shim.loc_shim_recentre(extent, x, y, C.byref(i), C.byref(j))
    return bool(moved), i.value, j.value


class ShimMap:
    """a world map binned by the shim: order, directory, n_dropped; window(oi, oj, dim) -> SURFEL_DTYPE records"""

    def __init__(self, shim, records, extent):
        self.shim, self.extent = shim, float(extent)
        self.records = np.ascontiguousarray(records, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
        n = self.records.shape[0]
        self.order = np.zeros(max(n, 1), dtype=np.uint32)
        self.dir = np.zeros(max(n, 1), dtype=TILE_DTYPE)
        kept, dropped, tiles = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        rc = shim.loc_shim_bin(self.records.ctypes.data, n, self.extent, self.order.ctypes.data, self.dir.ctypes.data,
                               C.byref(kept), C.byref(dropped), C.byref(tiles))
        assert rc == 0, rc
        self.n_kept, self.n_dropped, self.n_tiles = kept.value, dropped.value, tiles.value
        self.order, self.dir = self.order[:self.n_kept], self.dir[:self.n_tiles]

    def window_size(self, oi, oj, dim):
        return int(self.shim.loc_shim_window(self.records.ctypes.data, self.order.ctypes.data, self.dir.ctypes.data,
                                             self.n_tiles, oi, oj, dim, None, 0))

    def window(self, oi, oj, dim):
        n = self.window_size(oi, oj, dim)
        out = np.zeros(n, dtype=SURFEL_DTYPE)
        if n:
            got = self.shim.loc_shim_window(self.records.ctypes.data, self.order.ctypes.data, self.dir.ctypes.data,
                                            self.n_tiles, oi, oj, dim, out.ctypes.data, n)
            assert got == n
        return out


# ---- crafted maps

def edge_records(extent):
    """records exactly on the tile edges x = +-e and (2i + 1) e, negative coordinates, NaN / inf, |i| >= 2^20"""
    e = np.float32(extent)
    xs = [e, -e, np.float32(3) * e, -np.float32(3) * e, np.float32(5) * e, np.nextafter(e, np.float32(0)),
          np.nextafter(-e, np.float32(0)), np.nextafter(-e, np.float32(-1e9)), np.float32(-0.5), np.float32(-7.25) * e,
          np.float32(0.0), np.float32(-0.0)]
    rows = [(x, y) for x in xs for y in (np.float32(0.25), -e, e)]
    r = np.zeros(len(rows) + 12, dtype=WORLD_SURFEL_DTYPE)
    k = len(rows)
    r["x"][:k], r["y"][:k] = [a for a, _ in rows], [b for _, b in rows]
    r["z"][:k] = 1.0
    # dropped: a non-finite coordinate each, and cells at / beyond the grid's edge; kept: the last cell inside
    r["x"][k + 0], r["y"][k + 1], r["z"][k + 2] = np.nan, np.inf, -np.inf
    r["x"][k + 3] = np.float32(2 * GRID) * e                 # i = 2^20 (+ 1/2 rounds into it): dropped
    r["x"][k + 4] = -np.float32(2 * GRID) * e                # i = -2^20: dropped
    r["x"][k + 5] = -np.float32(2 * GRID - 2) * e            # i = -2^20 + 1: the last cell inside
    r["y"][k + 6] = np.float32(2 * GRID - 2) * e             # j = 2^20 - 1: the last cell inside
    r["y"][k + 7] = np.float32(3.0e38)                       # the sum overflows or the quotient is huge: dropped
    r["x"][k + 8] = np.float32(-3.0e38)
    r["z"][k + 9] = np.nan
    r["x"][k + 10], r["y"][k + 10] = np.float32(1e-30), np.float32(-1e-30)
    r["x"][k + 11], r["y"][k + 11] = np.float32(2.5) * e, np.float32(-2.5) * e
    fill_payload(r, 7)
    return r


def fill_payload(r, seed):
    """everything but the position: distinct values in every field the conversion copies or reads"""
    rng = np.random.RandomState(seed)
    n = r.shape[0]
    r["radius"] = rng.uniform(0.03, 1.0, n)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    r["nx"], r["ny"], r["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    r["confidence"] = rng.uniform(-2.0, 20.0, n)
    r["label"] = rng.randint(0, 260, n)
    r["prob"] = rng.uniform(0.0, 1.0, n)
    r["timestamp"] = rng.randint(0, 5000, n)
    r["support"] = rng.randint(1, 9, n)
    return r


def crafted_records(n, extent, seed=1, spread=3.6):
    """n records scattered over (2 spread + 1)^2 tiles around the origin, shuffled, so that every tile's run interleaves
    with the others' in the source order; n = 0 gives an empty map"""
    rng = np.random.RandomState(seed + n)
    r = np.zeros(n, dtype=WORLD_SURFEL_DTYPE)
    lim = np.float32(2.0 * spread * extent)
    r["x"] = rng.uniform(-lim, lim, n)
    r["y"] = rng.uniform(-lim, lim, n)
    r["z"] = rng.uniform(-2.0, 2.0, n)
    return fill_payload(r, seed + 1000 + n)


def numpy_window(records, extent, oi, oj, dim):
    """the specification in numpy: kept records of the window's tiles by lexsort (i, j, source index), converted;
    -> (SURFEL_DTYPE window, n_dropped)"""
    r = np.ascontiguousarray(records, dtype=WORLD_SURFEL_DTYPE).reshape(-1)
    e = np.float32(extent)
    w = np.float32(2.0) * e
    with np.errstate(all="ignore"):
        fi = np.floor((r["x"] + e) / w)
        fj = np.floor((r["y"] + e) / w)
        kept = np.isfinite(r["x"]) & np.isfinite(r["y"]) & np.isfinite(r["z"]) & (np.abs(fi) < GRID) & (np.abs(fj) < GRID)
    n_dropped = int((~kept).sum())
    src = np.nonzero(kept)[0]
    i, j = fi[src].astype(np.int64), fj[src].astype(np.int64)
    inside = (np.abs(i - oi) <= dim) & (np.abs(j - oj) <= dim)
    src, i, j = src[inside], i[inside], j[inside]
    order = np.lexsort((src, j, i))
    s = r[src[order]]
    out = np.zeros(s.shape[0], dtype=SURFEL_DTYPE)
    for f in ("x", "y", "z", "radius", "nx", "ny", "nz", "confidence"):
        out[f] = s[f]
    lab = s["label"].astype(np.float32) / np.float32(255.0)
    out["r"] = out["g"] = out["b"] = lab
    out["w"] = s["prob"]
    return out, n_dropped


# ---- the mapping run that is localised in

LOC_W, LOC_H, LOC_SCANS = 360, 32, 45


def loc_params(**kw):
    from semantic_suma_amd.types import params_with_size
    return params_with_size(LOC_W, LOC_H, **dict(dict(submap_extent=10.0, submap_dimension=2), **kw))


def loc_scans(n=LOC_SCANS):
    from semantic_suma_amd import synth
    return [synth.generate_scan(k, LOC_W, LOC_H)[:3] for k in range(n)]


def perturbed(T, dx=0.3, dy=-0.15, yaw_deg=2.0):
    """T moved by (dx, dy) and turned by yaw in its own frame"""
    a = np.deg2rad(yaw_deg)
    P = np.eye(4)
    P[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    P[0, 3], P[1, 3] = dx, dy
    return np.asarray(T, dtype=np.float64) @ P


def tracking_failures(loc_poses, map_poses, first=1):
    """the tracking condition: for every scan k >= first the mapping pose nearest in translation to the localised pose is
    the mapping pose of scan k itself.  -> (the scans that fail it, the worst error from `first` on, in metres)"""
    mp = np.asarray(map_poses)[:, :3, 3]
    bad, worst = [], 0.0
    for k, T in enumerate(loc_poses):
        if k < first:
            continue
        d = np.linalg.norm(mp - np.asarray(T)[:3, 3], axis=1)
        worst = max(worst, float(d[k]))
        if int(np.argmin(d)) != k or not np.isfinite(d[k]):
            bad.append(k)
    return bad, worst
