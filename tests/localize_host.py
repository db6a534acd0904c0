"""The whole localiser (csrc/suma_localize.hip) over the CPU oracle: the shim's window (tests/localize_shim.c), then
Oracle.map_upload(window, T_loc), preprocess, map_render_inactive, minimize -- the same step order and the same matrix
product order as the library, so that suma_localizer_process_scan must equal it to the bit.  Precedents:
loop_closing_host.py, posegraph_host.py."""
import copy
import math

import numpy as np

import localize_common as lc
from loop_closing_host import mul4, rigid_inv
from oracle import pyoracle
from semantic_suma_amd.types import LocalizerParams


def f32(x):
    return np.float32(x)


def orthonormalize(T):
    """mat4_orthonormalize (csrc/suma_internal.h) in the same operation order: the rotation's columns by Gram-Schmidt --
    c0 normalised, c1 made orthogonal to c0 and normalised, c2 = c0 x c1 -- the translation kept, the last row 0 0 0 1"""
    T = np.asarray(T, dtype=np.float64)
    a = [float(T[r, 0]) for r in range(3)]
    b = [float(T[r, 1]) for r in range(3)]
    dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]  # noqa: E731
    n = math.sqrt(dot(a, a))
    a = [x / n for x in a]
    d = dot(a, b)
    b = [b[r] - d * a[r] for r in range(3)]
    n = math.sqrt(dot(b, b))
    b = [x / n for x in b]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    out = np.eye(4)
    for r in range(3):
        out[r, 0], out[r, 1], out[r, 2], out[r, 3] = a[r], b[r], c[r], T[r, 3]
    return out


class HostLocalizer:
    def __init__(self, params, shim, loc_params: LocalizerParams = None, threads: int = 8):
        self.p, self.shim = params, shim
        self.lp = LocalizerParams.defaults(params) if loc_params is None else loc_params
        self.ora = pyoracle.Oracle(params, threads=threads)
        self.frame = self.ora.frame()
        self.t_loc = int(params.active_timestamps) + 10
        self.map = None
        self.have_pose = False
        self.rebuilds = 0
        self.n_window = 0
        self.origin = (0, 0)

    def set_map(self, records):
        self.map = lc.ShimMap(self.shim, records, self.p.submap_extent)
        self.have_pose = False
        self.rebuilds, self.n_window = 0, 0
        return self.map.n_dropped

    def _gather(self, oi, oj):
        w = self.map.window(oi, oj, self.p.submap_dimension)
        if len(w) > self.p.max_surfels:
            raise OverflowError("window beyond max_surfels")
        self.ora.map_upload(w, self.t_loc)
        self.window = w
        self.origin, self.n_window = (oi, oj), len(w)
        self.rebuilds += 1

    def set_pose(self, T):
        T = np.asarray(T, dtype=np.float64)
        assert self.map is not None and np.all(np.isfinite(T))
        cell = lc.shim_cell(self.shim, self.p.submap_extent, f32(T[0, 3]), f32(T[1, 3]), f32(T[2, 3]))
        assert cell is not None
        self._gather(*cell)
        self.pose, self.increment = T.copy(), np.eye(4)
        self.have_pose, self.first = True, True

    def process_scan(self, points, labels, probs, fixed_iterations=0):
        assert self.map is not None and self.have_pose
        guess = mul4(self.pose, self.increment) if self.lp.constant_velocity else self.pose.copy()
        gf = guess.astype(np.float32)
        moved, oi, oj = lc.shim_recentre(self.shim, self.p.submap_extent, gf[0, 3], gf[1, 3], *self.origin)
        if moved:
            self._gather(oi, oj)
        T_gn, minimised = np.eye(4), False
        st = dict(error=0.0, inlier_residual=0.0, valid=0, outlier=0, inlier=0, invalid=0, iterations=0, converged=0)
        if self.n_window:
            self.ora.preprocess(points, labels, probs, self.t_loc, self.frame)
            self.ora.map_render_inactive(gf, float(self.lp.conf_threshold))
            model = self.ora.map_frame(0)
            if fixed_iterations > 0:  # processScan's override (o_pipeline.c, o_minimize_cfg)
                q = copy.copy(self.p)
                q.max_iterations, q.stopping_threshold, q.delta = fixed_iterations, 0.0, 0.0
                self.ora.set_params(q)
            T_gn, _, s = self.ora.minimize(self.frame, model, np.eye(4))
            if fixed_iterations > 0:
                self.ora.set_params(self.p)
            st = s.as_dict()
            minimised = bool(np.all(np.isfinite(T_gn)))
        if minimised:
            pose = orthonormalize(mul4(guess, T_gn))
            self.increment = np.eye(4) if self.first else mul4(rigid_inv(self.pose), pose)
        else:  # nothing was minimised: pose = guess, the increment stays
            pose = guess.copy()
        self.pose, self.first = pose, False
        with np.errstate(all="ignore"):
            valid_ratio = f32(st["valid"]) / f32(f32(st["valid"]) + f32(st["invalid"]))
            outlier_ratio = f32(st["outlier"]) / f32(f32(st["outlier"]) + f32(st["inlier"]))
        tracked = bool(float(valid_ratio) > float(f32(self.lp.min_valid_ratio)) and
                       float(outlier_ratio) < float(f32(self.lp.max_outlier_ratio)))
        return dict(guess=guess, pose=pose.copy(), increment=self.increment.copy(), stats=st,
                    valid_ratio=float(valid_ratio), outlier_ratio=float(outlier_ratio), tracked=tracked,
                    window_rebuilt=bool(moved), origin=self.origin, n_window=self.n_window)


def results_equal(a, b, where=""):
    """two result dicts (core.Localizer.processScan / HostLocalizer.process_scan) equal to the bit"""
    for k in ("guess", "pose", "increment"):
        assert np.asarray(a[k], dtype=np.float64).tobytes() == np.asarray(b[k], dtype=np.float64).tobytes(), (where, k, a[k], b[k])
    sa, sb = dict(a["stats"]), dict(b["stats"])
    for k in ("error", "inlier_residual"):
        assert np.float64(sa.pop(k)).tobytes() == np.float64(sb.pop(k)).tobytes(), (where, k)
    assert sa == sb, (where, sa, sb)
    for k in ("valid_ratio", "outlier_ratio"):
        assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (where, k, a[k], b[k])
    for k in ("tracked", "window_rebuilt", "origin", "n_window"):
        assert a[k] == b[k], (where, k, a[k], b[k])
