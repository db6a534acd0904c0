"""Shared by the tests of the live obstacle layer (test_abi_live.py, test_live_host.py, test_gpu_live.py): the host
restatement tests/live_shim.c of csrc/k_live.hip, a plain Python restatement of it (a dict per cell, Python integers, the
hits of a scan gathered per cell before the rule is applied once), crafted static cells, and crafted sequences of frames on
every boundary of the specification, each with what the specification says must come out."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd.types import (GRID_CELL_DTYPE, GridParams, LIVE_CELL_DTYPE, LIVE_COUNTS, LiveCounts, LiveParams,
                                     LiveStats)

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_FLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off"]
NONE = 0xffffffff
f32 = np.float32
NAN = f32(np.nan)
ZERO = dict.fromkeys(LIVE_COUNTS, 0)


class ShimGrid(C.Structure):
    """lgrid_t of live_shim.c: the fields of suma_grid_params the layer reads"""
    _fields_ = [("cell_size", C.c_float), ("origin_x", C.c_float), ("origin_y", C.c_float), ("width", C.c_uint32),
                ("height", C.c_uint32), ("step_height", C.c_float), ("clearance", C.c_float)]

    @classmethod
    def of(cls, gp: GridParams):
        return cls(gp.cell_size, gp.origin_x, gp.origin_y, gp.width, gp.height, gp.step_height, gp.clearance)


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "live_shim.so")
    subprocess.check_call(["gcc"] + SHIM_FLAGS + ["-fPIC", "-shared", os.path.join(HERE, "live_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.live_shim_update.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, vp, C.POINTER(ShimGrid), vp, C.POINTER(LiveParams),
                                   C.c_uint32, vp, C.POINTER(LiveCounts)]
    L.live_shim_update.restype = None
    L.live_shim_compose.argtypes = [C.POINTER(ShimGrid), vp, C.POINTER(LiveParams), vp, C.c_uint32, vp, vp,
                                    C.POINTER(LiveStats)]
    L.live_shim_compose.restype = None
    return L


class ShimLayer:
    """the layer kept by live_shim.c: the interface of the Python restatement and of the GPU rig"""

    def __init__(self, shim, cells, gp: GridParams, lp: LiveParams = None):
        self.shim, self.gp = shim, gp
        self.lp = LiveParams.defaults() if lp is None else lp
        self.g = ShimGrid.of(gp)
        self.cells = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(-1).copy()
        assert self.cells.shape[0] == gp.width * gp.height
        self.clear()

    def clear(self):
        self.state_ = np.zeros(self.cells.shape[0], dtype=LIVE_CELL_DTYPE)
        self.now = 0

    def update(self, V, flags, T, scan_id, ids=None):
        """V: H x W x 4; flags: H x W; T: row-major 4x4; ids: H x W uint32 or None -> the counts dict"""
        V = np.ascontiguousarray(V, dtype=np.float32)
        H, W = V.shape[:2]
        fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(H, W)
        idp = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32).reshape(H, W)
        Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4).T)
        assert scan_id + 1 > self.now
        cnt = LiveCounts()
        self.shim.live_shim_update(V.ctypes.data, fl.ctypes.data, None if idp is None else idp.ctypes.data, W, H,
                                   Tc.ctypes.data, C.byref(self.g), self.cells.ctypes.data, C.byref(self.lp), scan_id + 1,
                                   self.state_.ctypes.data, C.byref(cnt))
        self.now = scan_id + 1
        return cnt.as_dict()

    def state(self):
        return self.state_.reshape(self.gp.height, self.gp.width).copy()

    def set_state(self, state, last_stamp):
        self.state_ = np.ascontiguousarray(state, dtype=LIVE_CELL_DTYPE).reshape(-1).copy()
        self.now = last_stamp

    def compose(self):
        """-> (cells[height, width], mask[height, width], the stats dict)"""
        out = np.zeros_like(self.cells)
        mask = np.zeros(self.cells.shape[0], dtype=np.uint8)
        st = LiveStats()
        self.shim.live_shim_compose(C.byref(self.g), self.cells.ctypes.data, C.byref(self.lp), self.state_.ctypes.data, self.now,
                                    out.ctypes.data, mask.ctypes.data, C.byref(st))
        shape = (self.gp.height, self.gp.width)
        return out.reshape(shape), mask.reshape(shape), st.as_dict()


# ---- the specification once more in plain Python.  fp32 by numpy scalars; a fused multiply-add is the fp64 product (exact)
# plus the addend rounded once to fp32 -- exact whenever the fp64 sum is, which holds for the inputs of these tests: all
# coordinates and pose entries are multiples of 2^-6 below 2^10, or the pose is a pure translation
def _fma(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def _dot(a, b):
    return _fma(a[2], b[2], _fma(a[1], b[1], f32(a[0] * b[0])))


def _point(P, m):
    return [f32(_fma(P[r, 2], m[2], _fma(P[r, 1], m[1], f32(P[r, 0] * m[0]))) + P[r, 3]) for r in range(3)]


def _ordered(z):
    b = int(np.array(z, dtype=np.float32).view(np.uint32))
    return (~b & 0xffffffff) if b & 0x80000000 else (b | 0x80000000)


def _unordered(o):
    b = (o & 0x7fffffff) if o & 0x80000000 else (~o & 0xffffffff)
    return np.array(b, dtype=np.uint32).view(np.float32)[()]


class PyLayer:
    """a dict per cell that has ever been hit: {stamp, top (an ordered integer), clear, hits}"""

    def __init__(self, cells, gp: GridParams, lp: LiveParams = None):
        self.gp = gp
        self.lp = LiveParams.defaults() if lp is None else lp
        self.cells = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(-1).copy()
        self.clear()

    def clear(self):
        self.cell, self.now = {}, 0

    def _cell_of(self, x, y):
        gp = self.gp
        with np.errstate(all="ignore"):
            fx = np.floor(f32(f32(x - f32(gp.origin_x)) / f32(gp.cell_size)))
            fy = np.floor(f32(f32(y - f32(gp.origin_y)) / f32(gp.cell_size)))
        if not (fx >= 0 and fx < gp.width and fy >= 0 and fy < gp.height):
            return None
        return int(fy) * gp.width + int(fx)

    def update(self, V, flags, T, scan_id, ids=None):
        gp, lp = self.gp, self.lp
        V = np.ascontiguousarray(V, dtype=np.float32)
        H, W = V.shape[:2]
        Vf, fl = V.reshape(-1, 4), np.asarray(flags).reshape(-1)
        idf = None if ids is None else np.asarray(ids).reshape(-1)
        s = scan_id + 1
        assert s > self.now
        cnt = dict(ZERO, n_texels=W * H)
        step_h, clearance = f32(gp.step_height), f32(gp.clearance)
        with np.errstate(all="ignore"):
            P = np.asarray(T, dtype=np.float64).reshape(4, 4).astype(np.float32)
            world = [_point(P, Vf[t, :3]) for t in range(W * H)]
            ret = [bool(Vf[t, 3] > f32(0.5) and np.all(np.isfinite(Vf[t, :3])) and np.all(np.isfinite(world[t])))
                   for t in range(W * H)]
            per_cell = {}
            for t in range(W * H):
                if not (ret[t] and fl[t] != 0) or (idf is not None and idf[t] == NONE):
                    continue
                cnt["n_members"] += 1
                w = world[t]
                c = self._cell_of(w[0], w[1])
                if c is None:
                    cnt["n_outside"] += 1
                    continue
                g = self.cells["ground_z"][c]
                if np.isnan(g):
                    cnt["n_no_ground"] += 1
                    continue
                h = f32(w[2] - g)
                if h <= step_h:
                    cnt["n_low"] += 1
                elif h > clearance:
                    cnt["n_high"] += 1
                else:
                    cnt["n_hit_texels"] += 1
                    per_cell.setdefault(c, []).append(_ordered(w[2]))
            for c, tops in per_cell.items():
                st = self.cell.setdefault(c, dict(stamp=0, top=0, clear=0, hits=0))
                old = st["stamp"]
                run = old != 0 and old > st["clear"] and s - old <= lp.hold_scans
                st["hits"] = min(st["hits"] + 1, 65535) if run else 1
                st["stamp"], st["top"] = s, max(tops)
                cnt["n_hit_cells"] += 1
            self.now = s
            if lp.carve_range == 0:
                return cnt
            o = [P[0, 3], P[1, 3], P[2, 3]]
            step = f32(f32(0.5) * f32(gp.cell_size))
            margin, rng = f32(lp.carve_margin), f32(lp.carve_range)
            cleared = set()
            for t in range(W * H):
                if not ret[t]:
                    continue
                cnt["n_rays"] += 1
                u = [f32(world[t][k] - o[k]) for k in range(3)]
                r = np.sqrt(_dot(u, u))
                lim = f32(r - margin)
                prev = -1
                for k in range(1, 4097):
                    tk = f32(f32(k) * step)
                    if not (tk < lim and tk <= rng):
                        break
                    q = f32(tk / r)
                    p = [f32(o[a] + f32(u[a] * q)) for a in range(3)]
                    c = self._cell_of(p[0], p[1])
                    if c == prev:
                        continue
                    prev = c
                    st = None if c is None else self.cell.get(c)
                    if st is None or not (0 < st["stamp"] < s):
                        continue
                    if p[2] <= _unordered(st["top"]) and f32(p[2] - self.cells["ground_z"][c]) > step_h:
                        cleared.add(c)
            for c in cleared:
                if self.cell[c]["clear"] < s:
                    self.cell[c]["clear"] = s
                    cnt["n_cleared"] += 1
        return cnt

    def state(self):
        out = np.zeros(self.cells.shape[0], dtype=LIVE_CELL_DTYPE)
        for c, st in self.cell.items():
            out[c] = ((st["stamp"] << 32) | st["top"], st["clear"], st["hits"])
        return out.reshape(self.gp.height, self.gp.width)

    def set_state(self, state, last_stamp):
        self.clear()
        for c, st in enumerate(np.asarray(state).reshape(-1)):
            if int(st["hit"]) or int(st["clear"]) or int(st["hits"]):
                self.cell[c] = dict(stamp=int(st["hit"]) >> 32, top=int(st["hit"]) & 0xffffffff, clear=int(st["clear"]),
                                    hits=int(st["hits"]))
        self.now = last_stamp

    def classify(self, c):
        """'live', 'pending', 'expired', 'carved' or None"""
        st = self.cell.get(c)
        if st is None or st["stamp"] == 0:
            return None
        if not st["stamp"] > st["clear"]:
            return "carved"
        if not self.now - st["stamp"] < self.lp.hold_scans:
            return "expired"
        return "live" if st["hits"] >= self.lp.min_hits else "pending"

    def compose(self):
        out = self.cells.copy()
        mask = np.zeros(out.shape[0], dtype=np.uint8)
        stats = dict(n_live=0, n_pending=0, n_expired=0, n_carved=0)
        for c in self.cell:
            k = self.classify(c)
            if k is None:
                continue
            stats["n_" + k] += 1
            if k == "pending":
                mask[c] = 2
            if k == "live":
                mask[c] = 1
                out["state"][c] = 2
                top, oz = _unordered(self.cell[c]["top"]), out["obstacle_z"][c]
                if np.isnan(oz) or _ordered(oz) < self.cell[c]["top"]:
                    out["obstacle_z"][c] = top
        shape = (self.gp.height, self.gp.width)
        return out.reshape(shape), mask.reshape(shape), stats


def same_layer(got, want, what):
    """two layers' state and composition, byte for byte"""
    gs, ws = got.state(), want.state()
    assert gs.dtype == LIVE_CELL_DTYPE and gs.tobytes() == ws.tobytes(), (what, "state", np.argwhere(gs != ws)[:8])
    (gc, gm, gst), (wc, wm, wst) = got.compose(), want.compose()
    assert gst == wst, (what, gst, wst)
    assert gm.tobytes() == wm.tobytes(), (what, "mask")
    assert gc.dtype == GRID_CELL_DTYPE and gc.tobytes() == wc.tobytes(), (what, "cells")
    return wc, wm, wst


# ---- crafted static cells and frames
def grid_params(width, height, cell_size=1.0, origin=(0.0, 0.0), step_height=0.25, clearance=2.0):
    return GridParams.defaults(cell_size=cell_size, origin=origin, width=width, height=height, step_height=step_height,
                               clearance=clearance)


def flat_cells(gp: GridParams, ground=0.0):
    """every cell FREE with its own ground at ``ground``, no obstacle"""
    cells = np.zeros(gp.width * gp.height, dtype=GRID_CELL_DTYPE)
    for k in ("ground_rough", "z_min", "z_max", "obstacle_z"):
        cells[k] = NAN
    cells["ground_z"], cells["z_min"], cells["z_max"] = ground, ground, ground
    cells["ground_rough"], cells["prob"], cells["label"], cells["support"], cells["n_ground"] = 0.0, 1.0, 40, 3, 3
    cells["state"], cells["ground_source"] = 1, 1
    return cells


def varied_cells(gp: GridParams, seed):
    """flat cells with, scattered: no ground (NaN, NO_GROUND and UNKNOWN), a filled ground, a deep ground (hits become
    overhangs), static obstacles with an obstacle_z below and above what the frames hit, and -0 for a ground"""
    rng = np.random.RandomState(seed)
    cells = flat_cells(gp, -1.25)
    n = cells.shape[0]
    k = rng.randint(0, 12, n)
    cells["ground_z"][k == 0] = NAN
    cells["state"][k == 0], cells["ground_source"][k == 0] = 3, 0
    cells["ground_source"][k == 1], cells["support"][k == 1], cells["state"][k == 1] = 2, 0, 0
    cells["ground_z"][k == 2] = -4.0
    cells["state"][k == 3], cells["obstacle_z"][k == 3], cells["n_obstacle"][k == 3] = 2, -0.875, 1
    cells["state"][k == 4], cells["obstacle_z"][k == 4], cells["n_obstacle"][k == 4] = 2, 3.0, 2
    cells["ground_z"][k == 5] = -0.0
    return cells


def frame_of(W, H, points):
    """-> V (H x W x 4): no return anywhere but at the texels of ``points`` = {(tx, ty): (x, y, z)}"""
    V = np.zeros((H, W, 4), dtype=np.float32)
    for (tx, ty), p in points.items():
        V[ty, tx] = (p[0], p[1], p[2], 1.0)
    return V


def flags_of(W, H, texels):
    fl = np.zeros((H, W), dtype=np.uint8)
    for tx, ty in texels:
        fl[ty, tx] = 1
    return fl


def translation(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def random_frame(W, H, seed, radius, z_lo=-1.25, z_hi=1.0, squash=1.0):
    """dyadic points (multiples of 2^-6) at about ``radius`` around the origin (y times ``squash``), with texels without
    a return, NaN and infinite components among them -> (V, flags)"""
    rng = np.random.RandomState(seed)
    V = np.zeros((H, W, 4), dtype=np.float32)
    ang = rng.rand(H, W) * 2 * np.pi
    rad = radius * (0.5 + 0.5 * rng.rand(H, W))
    V[..., 0] = np.round(rad * np.cos(ang) * 64) / 64
    V[..., 1] = np.round(rad * np.sin(ang) * squash * 64) / 64
    V[..., 2] = rng.randint(int(z_lo * 64), int(z_hi * 64) + 1, (H, W)) / 64.0
    V[..., 3] = rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 1.0, 1.0], dtype=np.float32), (H, W))
    bad = rng.rand(H, W) < 0.04
    comp = rng.randint(0, 3, (H, W))
    val = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), (H, W))
    for k in range(3):
        V[..., k] = np.where(bad & (comp == k), val, V[..., k])
    flags = (rng.rand(H, W) < 0.6).astype(np.uint8) * rng.randint(1, 255, (H, W)).astype(np.uint8)
    return V, flags


ROT = np.array([[0.0, -1.0, 0.0, 0.25], [1.0, 0.0, 0.0, -0.5], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def random_sequence(W, H, gw, gh, seed=0):
    """-> (gp, cells, lp, steps): six updates of random frames whose ranges shrink and grow, so that later rays cross
    cells hit before; the raster covers the middle of the points, the rest lie outside; for a strip of a raster the points
    are squashed into a strip and the sensor does not turn.  steps = [(V, flags, T, scan_id)]"""
    extent = 8.0
    cell = max(extent / max(gw, gh), 1.0 / 64)
    cell = 2.0 ** np.ceil(np.log2(cell))
    if gw * gh == 1:
        cell = 16.0
    gp = grid_params(gw, gh, cell_size=cell, origin=(-cell * gw / 2, -cell * gh / 2))
    cells = varied_cells(gp, seed + 11)
    lp = LiveParams.defaults(hold_scans=3, min_hits=2, carve_range=6.0, carve_margin=0.25)
    steps = []
    for k, (radius, sid) in enumerate([(3.0, 0), (3.0, 1), (6.0, 2), (2.0, 4), (6.0, 5), (6.0, 9)]):
        strip = gw > 4 * gh
        V, fl = random_frame(W, H, seed * 100 + k, radius, squash=2.0 * gh / gw if strip else 1.0)
        T = ROT if k % 2 and not strip else translation(0.5 if k % 2 else -0.25, 0.0 if strip else -0.25, -0.5)
        steps.append((V, fl, T, sid))
    return gp, cells, lp, steps


# ---- the named cases: each a sequence on one layer, and what the specification says about its end.  All on a 70 x 3
# frame and a 7 x 5 raster of 1 m cells at the origin with the ground at 0 unless they say otherwise.
W0, H0 = 70, 3


class Case:
    def __init__(self, name, steps, expect, gp=None, cells=None, lp=None, preset=None):
        self.name, self.steps, self.expect = name, steps, expect
        self.gp = grid_params(7, 5) if gp is None else gp
        self.cells = flat_cells(self.gp) if cells is None else cells
        self.lp = LiveParams.defaults() if lp is None else lp
        self.preset = preset                      # (state, last_stamp) put in front of the first step

    def run(self, layer):
        """applies the steps to a freshly made or cleared layer -> the list of counts"""
        if self.preset is not None:
            layer.set_state(*self.preset)
        return [layer.update(V, fl, T, sid) for V, fl, T, sid in self.steps]


def _all(points):
    return flags_of(W0, H0, points.keys())


def cell_index(gp, ix, iy):
    return iy * gp.width + ix


def named_cases():
    out = []
    I = np.eye(4)
    up, dn = (lambda v: np.nextafter(f32(v), f32(np.inf))), (lambda v: np.nextafter(f32(v), f32(-np.inf)))

    # h at step_height and clearance and the next fp32 either side (the ground is 0 and the pose the identity: h = z)
    pts = {(k, 0): (k + 0.5, 0.5, z) for k, z in enumerate([dn(0.25), 0.25, up(0.25), dn(2.0), 2.0, up(2.0)])}

    def e_thresholds(counts, layer):
        assert counts[0] == dict(ZERO, n_texels=210, n_members=6, n_low=2, n_high=1, n_hit_texels=3, n_hit_cells=3, n_rays=6)
        st = layer.state().reshape(-1)
        assert [int(h) >> 32 for h in st["hit"][:7]] == [0, 0, 1, 1, 1, 0, 0] and list(st["hits"][:7]) == [0, 0, 1, 1, 1, 0, 0]
    out.append(Case("hit_thresholds", [(frame_of(W0, H0, pts), _all(pts), I, 0)], e_thresholds))

    # a point an ulp either side of a cell edge and of the raster's border
    pts = {(0, 0): (dn(3.0), 0.5, 1.0), (1, 0): (3.0, 1.5, 1.0), (2, 0): (dn(0.0), 2.5, 1.0), (3, 0): (0.0, 2.5, 1.0),
           (4, 0): (dn(7.0), 3.5, 1.0), (5, 0): (7.0, 3.5, 1.0), (6, 0): (0.5, dn(5.0), 1.0), (7, 0): (0.5, 5.0, 1.0),
           (8, 0): (-0.0, -0.0, 1.0)}

    def e_edges(counts, layer):
        assert counts[0]["n_outside"] == 3 and counts[0]["n_hit_cells"] == 6, counts
        gp = layer.gp
        hit = np.nonzero(layer.state().reshape(-1)["hit"])[0]
        assert list(hit) == sorted(cell_index(gp, *c) for c in [(2, 0), (3, 1), (0, 2), (6, 3), (0, 4), (0, 0)])
    out.append(Case("cell_edges", [(frame_of(W0, H0, pts), _all(pts), I, 0)], e_edges))

    # a cell without ground, and a filled one
    gp = grid_params(7, 5)
    cells = flat_cells(gp)
    cells["ground_z"][cell_index(gp, 1, 1)], cells["ground_source"][cell_index(gp, 1, 1)] = NAN, 0
    cells["ground_z"][cell_index(gp, 2, 1)], cells["ground_source"][cell_index(gp, 2, 1)] = 0.5, 2
    cells["support"][cell_index(gp, 2, 1)], cells["state"][cell_index(gp, 2, 1)] = 0, 0
    pts = {(0, 1): (1.5, 1.5, 1.0), (1, 1): (2.5, 1.5, 1.0), (2, 1): (2.25, 1.25, 0.75)}

    def e_ground(counts, layer):
        assert counts[0]["n_no_ground"] == 1 and counts[0]["n_hit_texels"] == 1 and counts[0]["n_low"] == 1, counts
    out.append(Case("no_ground_and_filled", [(frame_of(W0, H0, pts), _all(pts), I, 0)], e_ground, gp=gp, cells=cells))

    # all members in one cell with equal z, and with +-0 (the ground at -1: h = 1)
    for name, zs, top in (("one_cell_equal_z", [0.5] * 40, 0.5), ("one_cell_signed_zero", [-0.0, 0.0] * 20, 0.0)):
        pts = {(k, 1): (3.0 + k / 64.0, 2.0 + k / 64.0, z) for k, z in enumerate(zs)}

        def e_one(counts, layer, top=top):
            assert counts[0]["n_hit_texels"] == 40 and counts[0]["n_hit_cells"] == 1, counts
            st = layer.state().reshape(-1)[cell_index(layer.gp, 3, 2)]
            assert int(st["hit"]) == (1 << 32) | _ordered(f32(top)) and st["hits"] == 1
            assert not np.signbit(_unordered(int(st["hit"]) & 0xffffffff))
        g1 = grid_params(7, 5)
        out.append(Case(name, [(frame_of(W0, H0, pts), _all(pts), I, 0)], e_one, gp=g1, cells=flat_cells(g1, -1.0),
                        lp=LiveParams.defaults(min_hits=1)))

    # no flag set; every flag set
    V, _ = random_frame(W0, H0, 5, 3.0, z_lo=0.5, z_hi=1.5)
    T = translation(3.5, 2.5, 0.0)

    def e_none(counts, layer):
        assert counts[0] == dict(ZERO, n_texels=210, n_rays=counts[0]["n_rays"]) and counts[0]["n_rays"] > 100
        assert not layer.state().view(np.uint8).any()

    def e_every(counts, layer):
        assert counts[0]["n_members"] == counts[0]["n_rays"] > 100 and counts[0]["n_hit_cells"] > 10, counts
    out.append(Case("no_flag", [(V, np.zeros((H0, W0), dtype=np.uint8), T, 0)], e_none))
    out.append(Case("every_flag", [(V, np.ones((H0, W0), dtype=np.uint8), T, 0)], e_every))

    # ---- sequences.  One obstacle texel in cell (3, 2), seen from (0.5, 2.5, 1); an empty scan has no flag
    hit = {(0, 0): (3.5, 2.5, 1.0)}
    Vh, Fh, F0 = frame_of(W0, H0, hit), _all(hit), np.zeros((H0, W0), dtype=np.uint8)
    S = translation(0.5, 2.5, 1.0)
    Vh = Vh.copy()
    Vh[0, 0, :3] = (3.0, 0.0, 0.0)                 # sensor frame: world = point + (0.5, 2.5, 1)
    off = LiveParams.defaults                      # carving off below unless a case is about it
    c32 = cell_index(grid_params(7, 5), 3, 2)

    def kind(layer):
        m = layer.compose()[1].reshape(-1)[c32]
        return {0: None, 1: "live", 2: "pending"}[int(m)]

    # expiry exactly at hold_scans: a hit at stamp 1, hold 3: live up to now = 3, expired at now = 4
    def e_expiry(counts, layer):
        assert layer.now == 4 and kind(layer) is None and layer.compose()[2] == dict(n_live=0, n_pending=0, n_expired=1, n_carved=0)
    out.append(Case("expiry_at_hold", [(Vh, Fh, S, 0), (Vh, F0, S, 1), (Vh, F0, S, 2), (Vh, F0, S, 3)], e_expiry,
                    lp=off(hold_scans=3, min_hits=1, carve_range=0.0)))

    def e_before_expiry(counts, layer):
        assert layer.now == 3 and kind(layer) == "live"
    out.append(Case("live_until_hold", [(Vh, Fh, S, 0), (Vh, F0, S, 1), (Vh, F0, S, 2)], e_before_expiry,
                    lp=off(hold_scans=3, min_hits=1, carve_range=0.0)))

    # min_hits 1, 2, 3 after two hits in a row
    for mh, want in ((1, "live"), (2, "live"), (3, "pending")):
        def e_min(counts, layer, want=want):
            assert layer.state().reshape(-1)[c32]["hits"] == 2 and kind(layer) == want
        out.append(Case("min_hits_%d" % mh, [(Vh, Fh, S, 0), (Vh, Fh, S, 1)], e_min, lp=off(min_hits=mh, carve_range=0.0)))

    # a re-hit after expiry restarts hits: hold 2, hits at stamps 1, 2, 3 (hits = 3), then at 6 (6 - 3 > 2)
    def e_rehit(counts, layer):
        st = layer.state().reshape(-1)[c32]
        assert int(st["hit"]) >> 32 == 6 and st["hits"] == 1 and kind(layer) == "pending"
    out.append(Case("rehit_after_expiry", [(Vh, Fh, S, 0), (Vh, Fh, S, 1), (Vh, Fh, S, 2), (Vh, Fh, S, 5)], e_rehit,
                    lp=off(hold_scans=2, carve_range=0.0)))

    # ... and at the edge: 5 - 3 <= 2 goes on counting
    def e_rehit_edge(counts, layer):
        assert layer.state().reshape(-1)[c32]["hits"] == 4
    out.append(Case("rehit_at_hold", [(Vh, Fh, S, 0), (Vh, Fh, S, 1), (Vh, Fh, S, 2), (Vh, Fh, S, 4)], e_rehit_edge,
                    lp=off(hold_scans=2, carve_range=0.0)))

    # a re-hit after a carve restarts hits: hits at 1, 2; at 3 a ray to (6.5, 2.5, 1) passes through at the top; at 4 a hit
    far = frame_of(W0, H0, {(0, 0): (6.0, 0.0, 0.0)})

    def e_carved(counts, layer):
        assert counts[2]["n_cleared"] == 1 and counts[2]["n_rays"] == 1, counts
        st = layer.state().reshape(-1)[c32]
        assert st["clear"] == 3 and int(st["hit"]) >> 32 == 2 and st["hits"] == 2 and kind(layer) is None
        assert layer.compose()[2]["n_carved"] == 1
    out.append(Case("carved", [(Vh, Fh, S, 0), (Vh, Fh, S, 1), (far, F0, S, 2)], e_carved))

    def e_rehit_carve(counts, layer):
        st = layer.state().reshape(-1)[c32]
        assert st["clear"] == 3 and int(st["hit"]) >> 32 == 4 and st["hits"] == 1 and kind(layer) == "pending"
    out.append(Case("rehit_after_carve", [(Vh, Fh, S, 0), (Vh, Fh, S, 1), (far, F0, S, 2), (Vh, Fh, S, 3)], e_rehit_carve))

    # hits saturate at 65 535
    pre = np.zeros(35, dtype=LIVE_CELL_DTYPE)
    pre[c32] = ((7 << 32) | _ordered(f32(1.0)), 0, 65534)

    def e_saturate(counts, layer):
        assert layer.state().reshape(-1)[c32]["hits"] == 65535 and kind(layer) == "live"
    out.append(Case("hits_saturate", [(Vh, Fh, S, 7), (Vh, Fh, S, 8)], e_saturate, lp=off(carve_range=0.0), preset=(pre, 7)))

    # ---- the carve rule.  Cells (5, 2), (1, 2) and (3, 4) were hit at stamp 1 with tops just above 1, 1 and just below 1;
    # at stamp 2 three horizontal rays at z = 1 leave (3.5, 2.5) along +x, -x and +y and pass through them: below the top,
    # at it, above it
    tops = {(0, 0): (5.5, 2.5, up(1.0)), (1, 0): (1.5, 2.5, 1.0), (2, 0): (3.5, 4.5, dn(1.0))}
    rays = frame_of(W0, H0, {(0, 0): (3.0, 0.0, 0.0), (1, 0): (-3.0, 0.0, 0.0), (2, 0): (0.0, 2.25, 0.0)})

    def e_tops(counts, layer):
        assert counts[1]["n_cleared"] == 2 and counts[1]["n_rays"] == 3, counts
        st = layer.state().reshape(-1)
        assert [int(st["clear"][cell_index(layer.gp, *c)]) for c in ((5, 2), (1, 2), (3, 4))] == [2, 2, 0]
    # the tops are placed in the world frame by the identity so that up(1) and dn(1) arrive exactly
    out.append(Case("ray_below_at_above_top", [(frame_of(W0, H0, tops), _all(tops), I, 0),
                                               (rays, F0, translation(3.5, 2.5, 1.0), 1)], e_tops))

    # a horizontal ray at step_height over the ground clears nothing, one at the next fp32 above does
    def e_low(counts, layer):
        assert [c["n_cleared"] for c in counts] == [0, 0, 1], counts
    out.append(Case("ray_at_step_height", [(Vh, Fh, S, 0), (far, F0, translation(0.5, 2.5, 0.25), 1),
                                           (far, F0, translation(0.5, 2.5, float(up(0.25))), 2)], e_low))

    # The sensor at x = 0.25 from here on: the samples lie at x = 0.75, 1.25, ... and the first one in cell (3, 2) is
    # t = 3.0 at x = 3.25, well inside it.  A ray that ends in the cell: the return at x = 3.75, margin 0.25, so t = 3.0 <
    # 3.25 is taken.  Unflagged it clears the cell; flagged it hits it, H = s, and nothing is cleared
    S2 = translation(0.25, 2.5, 1.0)
    ends = frame_of(W0, H0, {(0, 0): (3.5, 0.0, 0.0)})

    def e_ends(counts, layer):
        assert counts[1]["n_cleared"] == 1 and layer.state().reshape(-1)[c32]["clear"] == 2, counts

    def e_ends_hit(counts, layer):
        st = layer.state().reshape(-1)[c32]
        assert counts[1]["n_cleared"] == 0 and st["clear"] == 0 and st["hits"] == 2 and int(st["hit"]) >> 32 == 2
    out.append(Case("ray_ends_in_cell", [(Vh, Fh, S2, 0), (ends, F0, S2, 1)], e_ends, lp=off(carve_margin=0.25)))
    out.append(Case("hit_and_crossed_in_one_scan", [(Vh, Fh, S2, 0), (ends, Fh, S2, 1)], e_ends_hit, lp=off(carve_margin=0.25)))

    # a cell hit by one texel and crossed by another ray of the same scan is not cleared either
    both = frame_of(W0, H0, {(0, 0): (3.0, 0.0, 0.0), (1, 0): (6.0, 0.0, 0.0)})

    def e_both(counts, layer):
        assert counts[1]["n_cleared"] == 0 and counts[1]["n_rays"] == 2 and layer.state().reshape(-1)[c32]["clear"] == 0
    out.append(Case("hit_by_one_crossed_by_another", [(Vh, Fh, S, 0), (both, flags_of(W0, H0, [(0, 0)]), S, 1)], e_both))

    # carve_margin at its edge (0.5): r = 3.75 leaves t = 3.0 < 3.25 in; r = 3.5 gives 3.0 < 3.0, and the cell stays
    def e_in(counts, layer):
        assert counts[1]["n_cleared"] == 1, counts

    def e_out(counts, layer):
        assert counts[1]["n_cleared"] == 0, counts
    out.append(Case("carve_margin_inside", [(Vh, Fh, S2, 0), (frame_of(W0, H0, {(0, 0): (3.75, 0.0, 0.0)}), F0, S2, 1)], e_in))
    out.append(Case("carve_margin_edge", [(Vh, Fh, S2, 0), (frame_of(W0, H0, {(0, 0): (3.5, 0.0, 0.0)}), F0, S2, 1)], e_out))
    # carve_range at its edge: t = 3.0 <= 3.0 is taken, with the fp32 below 3.0 the ray ends in front of the cell
    out.append(Case("carve_range_edge_in", [(Vh, Fh, S2, 0), (far, F0, S2, 1)], e_in, lp=off(carve_range=3.0)))
    out.append(Case("carve_range_edge_out", [(Vh, Fh, S2, 0), (far, F0, S2, 1)], e_out, lp=off(carve_range=float(dn(3.0)))))

    def e_range0(counts, layer):
        assert counts[1]["n_cleared"] == 0 and counts[1]["n_rays"] == 0 and kind(layer) == "pending"
    out.append(Case("carve_range_zero", [(Vh, Fh, S, 0), (far, F0, S, 1)], e_range0, lp=off(carve_range=0.0)))

    # a ray from outside the raster through it and out again (a straight ray cannot enter a raster twice; what a ray does
    # between two visits of "outside" is this): the sensor at x = -2.5, the return at x = 9.5
    through = frame_of(W0, H0, {(0, 0): (12.0, 0.0, 0.0)})

    def e_through(counts, layer):
        assert counts[1]["n_cleared"] == 1 and counts[1]["n_outside"] == 0
    out.append(Case("ray_through_the_raster", [(Vh, Fh, S, 0), (through, F0, translation(-2.5, 2.5, 1.0), 1)], e_through))

    # cell_size larger than the whole scene: one cell of 64 m; half a cell is further than any return, no sample is taken
    g64 = grid_params(1, 1, cell_size=64.0, origin=(-32.0, -32.0))

    def e_big(counts, layer):
        assert [c["n_cleared"] for c in counts] == [0, 0] and counts[1]["n_rays"] == 1 and counts[0]["n_hit_cells"] == 1
        assert layer.compose()[1][0, 0] == 2
    out.append(Case("cell_larger_than_scene", [(Vh, Fh, S, 0), (far, F0, S, 1)], e_big, gp=g64, cells=flat_cells(g64)))
    return out


# ---- the scenario of DESIGN.md 19 (novel_common has the runs): 360 x 32, mapped without cube 2 and building 41, scans
# 20-44 of the full world localised on the CPU restatement of the localiser, the grid of the map as mapped at 0.2 m
SCENARIO_CELL, KEEP = 0.2, (4, 24)


def scenario_shims(tmp):
    import change_common as cc
    import grid_common as gc
    import localize_common as lc
    import novel_common as nc
    import object_common as oc
    import plan_common as pc
    return dict(l=lc.build_shim(tmp), c=cc.build_shim(tmp), n=nc.build_shim(tmp), o=oc.build_shim(tmp), v=build_shim(tmp),
                g=gc.build_shim(tmp), p=pc.build_shim(tmp))


def scenario_grid(shims, records):
    """the static grid of the mapped records -> (gp, cells[height, width])"""
    import grid_common as gc
    ox, oy, w, h = gc.fit_of(records, SCENARIO_CELL, 1)
    gp = GridParams.defaults(cell_size=SCENARIO_CELL, origin=(ox, oy), width=w, height=h)
    return gp, gc.shim_grid(shims["g"], records, gp)[0]


def scenario_run(shims, tmp, without, lp=None, gone_from=None, gone_without=(), mapped=None):
    """the host localiser over the 25 scans with novelty and objects on and the shim's layer updated behind every scan
    -> dict(gp, cells, mapped poses and records, per scan: counts, masks, stats, poses; composed: {index: cells} for KEEP).
    From scan index ``gone_from`` on the scans are those of the world without ``gone_without``.  ``mapped``: (params,
    poses, records) of a map made elsewhere in place of the oracle's"""
    import change_common as cc
    import novel_common as nc
    import novel_host as nh
    import object_common as oc
    p, poses, records = nc.map_on_oracle(tmp, without) if mapped is None else mapped
    gp, cells = scenario_grid(shims, records)
    layer = ShimLayer(shims["v"], cells, gp, lp)
    scans = nc.localise_scans()
    if gone_from is not None:
        scans = scans[:gone_from] + cc.edited_scans(without=gone_without)[gone_from:]
    h = nh.HostNovelLocalizer(p, shims["l"], shims["c"], shims["n"])
    h.set_map(records)
    h.set_pose(poses[nc.FIRST])
    out = dict(gp=gp, cells=cells, params=p, start=poses[nc.FIRST], records=records, counts=[], masks=[], stats=[], poses=[],
               composed={})
    for k, s in enumerate(scans):
        r = h.process_scan(*s)
        assert r["collected"] and r["tracked"], k
        V, S = np.array(h.frame.vertex, dtype=np.float32), np.array(h.frame.semantic, dtype=np.float32)
        flags = (h.col.category == 5).astype(np.uint8)                     # novel: what kn_collect flags
        ids = oc.shim_segment(shims["o"], V, S, flags, r["pose"], None, k)[1]
        out["counts"].append(layer.update(V, flags, r["pose"], k, ids))
        comp, mask, st = layer.compose()
        out["masks"].append(mask)
        out["stats"].append(st)
        out["poses"].append(np.array(r["pose"]))
        if k in KEEP:
            out["composed"][k] = comp
    return out


def footprint(gp, box, grow):
    """bool [height, width]: the cells whose centre lies inside the box's x / y extent grown by ``grow`` metres (the
    boxes live in the generator's world, the grid in the frame of scan 0)"""
    from semantic_suma_amd import synth
    T0 = synth.trajectory_pose(0)
    ix, iy = np.meshgrid(np.arange(gp.width), np.arange(gp.height))
    xyz = np.stack([gp.origin_x + (ix + 0.5) * gp.cell_size, gp.origin_y + (iy + 0.5) * gp.cell_size,
                    np.zeros(ix.shape)], -1).reshape(-1, 3)
    c, h, yaw = box
    cs, sn = np.cos(yaw), np.sin(yaw)
    Rb = np.array([[cs, sn, 0], [-sn, cs, 0], [0, 0, 1]])
    q = (xyz @ T0[:3, :3].T + T0[:3, 3] - c) @ Rb.T
    return np.all(np.abs(q[:, :2]) <= h[:2] + grow, axis=1).reshape(gp.height, gp.width)


def scenario_measure(run):
    """-> (scans after which a live cell lies in building 41's footprint, the smallest share over the scans with live cells
    of those inside the footprint grown by one cell, the greatest number of live cells after a scan)"""
    import object_common as oc
    gp = run["gp"]
    fin, fgrow = footprint(gp, oc.building_box(), 0.0), footprint(gp, oc.building_box(), gp.cell_size)
    live = [m == 1 for m in run["masks"]]
    shares = [float((m & fgrow).sum()) / float(m.sum()) for m in live if m.any()]
    return sum(1 for m in live if (m & fin).any()), (min(shares) if shares else 0.0), max(int(m.sum()) for m in live)


def scenario_path(shims, gp, cells, start, goal):
    """the plan shim's path between two cells (ix, iy) with unknown cells traversable -> (the suma_plan_path record, the
    path's cell indices)"""
    import plan_common as pc
    from semantic_suma_amd.types import PlanParams
    pp = PlanParams.defaults(unknown_blocked=False)
    field, _ = pc.shim_field(shims["p"], cells, gp, pp, [goal[1] * gp.width + goal[0]])
    res, rows = pc.shim_paths(shims["p"], field, gp, [start[1] * gp.width + start[0]], gp.width + gp.height)
    return res[0], rows[0, :min(int(res["length"][0]), rows.shape[1])]


# What the semantic check of test_live_host.py measured on the restatement with the default parameters:
# of the 25 scans, those after which a live cell lies inside building 41's footprint; the smallest share of the live cells
# inside the footprint grown by one cell; the live cells of the control run (the same world mapped and localised); the
# first scan index from which the path between PATH_START and PATH_GOAL, cells on either side of the building, avoids
# the footprint (on the static grid it crosses it) and the path costs; and, with the building taken out of the world
# from scan index TRAIL_GONE on, the scans until no cell of the grown footprint is live, with carving on and off
MEASURED = dict(scans_with_building=24, min_share=0.878788, control_live=0, path_from=4, static_cost=920, live_cost=1136,
                trail_carve_on=1, trail_carve_off=9)
PATH_START, PATH_GOAL, TRAIL_GONE = (396, 25), (442, 25), 10
# the same goal for a robot that starts where the run does: tools/localize.py --goal
ROBOT_GOAL = (440, 20)


def check_measured(scans_with_building, min_share, control_live):
    """the issue's conditions"""
    assert scans_with_building > 0 and scans_with_building >= 0.5 * MEASURED["scans_with_building"], (scans_with_building, MEASURED)
    assert min_share >= 0.5 * MEASURED["min_share"], (min_share, MEASURED)
    assert control_live <= max(2 * MEASURED["control_live"], 5), (control_live, MEASURED)
