"""SurfelMapping::checkLoopClosure and the pose-graph bookkeeping around it, restated in plain Python from the reference
(SurfelMapping.cpp:42-60, :212-253, :461-471, :478-518, :527-795, :819-826) -- not from the library's C code.

It drives a `Pipe` of tests/loop_scenario.py (`HipPipe` on the GPU, `OraclePipe` on the CPU) through the phase calls and
keeps its pose graph behind a small protocol (setInitial, addEdge, pose, poses, size, error, clone, optimize):
`core.Posegraph` on the GPU, `HostGraph` below (tests/posegraph_host.py) on the CPU.

Arithmetic: np.float32 where the reference has `float`, Python floats (fp64) where it has `double`; 0 / 0 gives NaN and
comparisons with it are false.  The reference leaves the operation order of its 4x4 products and inverses to Eigen; the
project fixes one order for every host-side product, ((a0 b0 + a1 b1) + a2 b2) + a3 b3, and inverts rigidly -- `mul4`
and `rigid_inv` below state it.  Left out, as in the library: loopClosurePoses_ and genResidualPlot.

The asynchronous optimisation runs in its deterministic form only: a clone started in scan k is integrated at the start
of scan k + 1 + integrate_lag.
"""
import math

import numpy as np

import posegraph_host as ph

F32 = np.float32


def mul4(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    return ((A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]) + A[:, 3:4] * B[3:4, :]


def rigid_inv(T):
    T = np.asarray(T, dtype=np.float64)
    out = np.zeros((4, 4))
    out[:3, :3] = T[:3, :3].T
    for r in range(3):
        out[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    out[3, 3] = 1.0
    return out


def translation_distance(A, B):
    """pose_distance (:499-501): |a.col(3) - b.col(3)|, the fourth components both 1"""
    dx, dy, dz = float(A[0, 3]) - float(B[0, 3]), float(A[1, 3]) - float(B[1, 3]), float(A[2, 3]) - float(B[2, 3])
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def fdiv(a, b):
    """float / float with IEEE semantics"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(a) / F32(b)


def ddiv(a, b):
    """double / double with IEEE semantics"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def find_candidate(poses, trajectory_distances, timestamp, current_pose, radius, min_trajectory_distance,
                   delta_timestamp):
    """getCandidateIndexes / getClosestIndex (:478-518)"""
    closest_idx = -1
    min_distance = F32(radius)
    for j in range(int(timestamp) - int(delta_timestamp), -1, -1):
        distance = F32(translation_distance(current_pose, poses[j]))
        tdistance = F32(trajectory_distances[timestamp]) - F32(trajectory_distances[j])
        if distance < min_distance and tdistance > F32(min_trajectory_distance):
            closest_idx = j
            min_distance = distance
    return closest_idx


class HostGraph:
    """the graph protocol on tests/posegraph_host.py (fp64 numpy, gtsam's Levenberg-Marquardt restated there)"""

    def __init__(self, nodes=(), edges=()):
        self.g = ph.HostGraph(nodes, edges)

    def setInitial(self, i, T):
        T = ph._rigid(T)
        if i == len(self.g.nodes):
            self.g.nodes.append(T)
        else:
            self.g.nodes[i] = T

    def addEdge(self, a, b, Z, info):
        info = np.asarray(info, dtype=np.float64)
        self.g.edges.append((int(a), int(b), ph._rigid(Z), 0.5 * (info + info.T)))

    def pose(self, i):
        return self.g.nodes[i].copy()

    def poses(self):
        return np.array(self.g.nodes).reshape(-1, 4, 4)

    def size(self):
        return len(self.g.nodes)

    def edges(self):
        return [(a, b, Z.copy(), O.copy()) for a, b, Z, O in self.g.edges]

    def error(self):
        return ph.error(self.g, np.array(self.g.nodes))

    def clone(self):
        return HostGraph(self.g.nodes, self.g.edges)

    def optimize(self, iterations):
        X, _ = ph.levenberg_marquardt(self.g, max_iterations=iterations)
        self.g.nodes = [ph._rigid(T) for T in X]
        return True


DEFAULTS = dict(residual_threshold=1.05, outlier_threshold=1.1, valid_threshold=0.9, search_distance=20.0,
                min_trajectory_distance=200.0, min_verifications=3, delta_timestamp=100, optimize_iterations=100,
                integrate_lag=0)


def _last_increment(pipe):
    s = pipe.s
    return s.lastIncrement() if hasattr(s, "lastIncrement") else s.last_increment()


class OptResult:  # SurfelMapping.h:112-122
    def __init__(self):
        self.error = self.residual = self.inlier_residual = 10000.0
        self.inlier = self.outlier = self.valid = self.invalid = 0
        self.outlier_ratio = F32(1.0)


class LoopClosing:
    """one SurfelMapping with close-loops = true; `scan()` is processScan (:175-210)"""

    def __init__(self, pipe, graph, iterations=8, **params):
        unknown = set(params) - set(DEFAULTS)
        assert not unknown, unknown
        self.p = dict(DEFAULTS, **params)
        self.pipe, self.graph, self.iterations = pipe, graph, iterations
        self.information = np.eye(6)  # :49-59
        self.timestamp = 0
        graph.setInitial(0, np.eye(4))  # :43
        self.trajectory_distances = [F32(0)]
        self.unverified, self.verified = [], []
        self.already_verified = False
        self.loop_count = 0
        self.time_without = 0
        self.optimizing = False
        self.opt_graph = None
        self.edges = []  # every addEdge, in order: (from, to, Z)
        self.table_at_integration = []  # (scan, the float32 pose table handed to the map)
        self._open_status()

    def _open_status(self):
        self.found = self.use = self.started = self.integrated = False
        self.candidate_to = -1
        self.edges_added = 0
        self.result_old = OptResult()
        self.loop_valid_ratio = self.loop_outlier_ratio = self.loop_relative_error_all = F32(0)
        self.posegraph_error = 0.0

    def status(self):
        ro = self.result_old
        return dict(found_candidate=int(self.found), use_candidate=int(self.use), candidate_to=int(self.candidate_to),
                    n_unverified=len(self.unverified), already_verified=int(self.already_verified),
                    loop_count=int(self.loop_count), time_without_loop_closure=int(self.time_without),
                    currently_optimizing=int(self.optimizing), started_optimization=int(self.started),
                    integrated=int(self.integrated), edges_added=int(self.edges_added),
                    result_old_outlier_ratio=F32(ro.outlier_ratio),
                    result_old=dict(error=float(ro.error), inlier_residual=float(ro.inlier_residual), valid=int(ro.valid),
                                    outlier=int(ro.outlier), inlier=int(ro.inlier), invalid=int(ro.invalid),
                                    iterations=0, converged=0),
                    result_old_residual=float(ro.residual), loop_valid_ratio=F32(self.loop_valid_ratio),
                    loop_outlier_ratio=F32(self.loop_outlier_ratio),
                    loop_relative_error_all=F32(self.loop_relative_error_all),
                    posegraph_error=float(self.posegraph_error))

    def _add_edge(self, a, b, Z):
        self.graph.addEdge(a, b, Z, self.information)
        self.edges.append((a, b, np.array(Z, dtype=np.float64)))

    # ---- integrateLoopClosures (:212-253)
    def integrate(self):
        self._open_status()
        if not self.optimizing or self.timestamp < self.started_at + 1 + self.p["integrate_lag"]:
            return
        poses_opt = self.opt_graph.poses()
        poses_before = self.graph.poses()
        casted = []
        for i in range(len(poses_opt)):
            casted.append(poses_opt[i].astype(F32))
            self.graph.setInitial(i, poses_opt[i])
        self.loop_count -= self.before_loop_count
        difference = mul4(poses_opt[self.before_id], rigid_inv(self.before_pose))
        for i in range(len(poses_opt), len(poses_before)):
            moved = mul4(difference, poses_before[i])
            casted.append(moved.astype(F32))
            self.graph.setInitial(i, moved)
        casted = np.array(casted)
        self.table_at_integration.append((self.timestamp, casted))
        self.pipe.integrate(casted, difference)  # map_->updatePoses, currentPose_ = difference * currentPose_ ...
        self.optimizing = False
        self.opt_graph = None
        n = self.graph.size()
        last = self.graph.pose(0)
        distance = F32(0)
        self.trajectory_distances = [F32(0)] * n
        for t in range(n):
            P = self.graph.pose(t)
            distance = F32(float(distance) + translation_distance(last, P))
            self.trajectory_distances[t] = distance
            last = P
        self.integrated = True

    # ---- the tail of updatePose (:461-471)
    def odometry_edge(self):
        t = self.timestamp
        increment = _last_increment(self.pipe)
        prev = self.graph.pose(t - 1)
        self.graph.setInitial(t, mul4(prev, increment))
        self._add_edge(t - 1, t, increment)
        distance = F32(translation_distance(prev, self.pipe.pose(0)))
        distance = distance + self.trajectory_distances[t - 1]
        self.trajectory_distances.append(F32(distance))

    def closest_index(self):
        return find_candidate(self.graph.poses(), self.trajectory_distances, self.timestamp, self.pipe.pose(0),
                              self.p["search_distance"], self.p["min_trajectory_distance"], self.p["delta_timestamp"])

    # ---- checkLoopClosure (:527-795)
    def check(self):
        p, pipe = self.p, self.pipe
        rn = pipe.stats()  # result_new_
        result_new_residual = ddiv(rn["error"], float(rn["inlier"] + rn["outlier"]))
        self.found = False
        ro = self.result_old = OptResult()
        self.use = False
        candidate_added = False
        have_min_candidate = False
        outlier_ratio_new = fdiv(rn["outlier"], rn["outlier"] + rn["inlier"])
        valid_ratio_new = fdiv(rn["valid"], rn["invalid"] + rn["valid"])
        self.time_without += 1

        if len(self.unverified) > 0 or self.already_verified:  # :551
            tr = pipe.track()  # render_inactive(lastPose_old_), minimize(lastIncrement_), the gates of :567, :570-576
            if tr["passed"]:
                cs = tr["composed"]
                error = F32(cs["error"])
                residual = fdiv(error, cs["inlier"] + cs["outlier"])
                ro.error = float(error)
                ro.inlier, ro.outlier = cs["inlier"], cs["outlier"]
                ro.residual = ddiv(ro.error, float(F32(ro.inlier + ro.outlier)))  # :582
                ro.inlier_residual = float(fdiv(F32(cs["inlier_residual"]), ro.inlier))
                ro.valid, ro.invalid = cs["valid"], cs["invalid"]
                rel_error_all = F32(ddiv(float(residual), result_new_residual))
                self.found = True
                pose_old = tr["pose_old"]  # lastPose_old_ * increment_old
                pipe.set_pose_old(pose_old)  # :590
                loop_closure = bool(rel_error_all < F32(p["residual_threshold"])) or \
                    (float(residual) - result_new_residual) < 0.1
                if loop_closure:
                    self.time_without = 0
                    index = self.closest_index()  # getClosestIndex ignores its argument (:508)
                    if index > -1:
                        cand = (self.timestamp, index, mul4(rigid_inv(pose_old), self.graph.pose(index)))
                        self.candidate_to = index
                        (self.verified if self.already_verified else self.unverified).append(cand)
                    self.use = True

        if not self.already_verified and len(self.unverified) >= p["min_verifications"] + 1:  # :628-633
            self.verified += self.unverified
            self.unverified = []
            self.already_verified = True

        last_from = -1  # :635-653
        for frm, to, diff in self.verified:
            if last_from != frm:
                last_from = frm
                self.loop_count += 1
            self._add_edge(frm, to, diff)
            self.edges_added += 1
        self.verified = []

        if (self.loop_count > 6 and not self.optimizing) or \
                (self.loop_count > 0 and not self.optimizing and self.time_without > 3):  # :655-660
            self.opt_graph = self.graph.clone()
            self.optimizing = True  # optimizeAsync (:819-826), with the values at the start
            self.before_id = self.timestamp
            self.before_loop_count = self.loop_count
            self.before_pose = self.opt_graph.pose(self.timestamp)
            self.started_at = self.timestamp
            self.opt_graph.optimize(p["optimize_iterations"])
            self.started = True

        if self.time_without > 3:  # :662-779
            self.unverified = []
            self.use = False
            self.already_verified = False
            to = self.closest_index()
            loop_closure_timestamp = -1
            pose_old = None
            if to > -1:
                pose_prior = self.graph.pose(to)
                O = mul4(rigid_inv(pose_prior), pipe.pose(0))
                O[2, 3] = 0.0
                Rz = O.copy()
                Rz[:3, 3] = 0.0
                half = O.copy()
                half[0, 3] = 0.5 * O[0, 3]
                half[1, 3] = 0.5 * O[1, 3]
                for g in pipe.verify(pose_prior, [O, Rz, half]):
                    self.found = True
                    if not g["passed"]:
                        continue
                    cs = g["composed"]
                    error = F32(cs["error"])
                    residual = fdiv(error, cs["inlier"] + cs["outlier"])
                    outlier_ratio_old = fdiv(cs["outlier"], cs["outlier"] + cs["inlier"])
                    valid_ratio_old = fdiv(cs["valid"], cs["valid"] + cs["invalid"])
                    rel_error_all = F32(ddiv(float(residual), result_new_residual))
                    rel_valid_ratio = fdiv(valid_ratio_old, valid_ratio_new)
                    rel_outlier_ratio = fdiv(outlier_ratio_old, outlier_ratio_new)
                    if not candidate_added or (float(residual) < ro.residual and outlier_ratio_old < ro.outlier_ratio):
                        if rel_valid_ratio >= F32(p["valid_threshold"]) and rel_outlier_ratio < F32(p["outlier_threshold"]):
                            candidate_added = True
                            loop_closure_timestamp = to
                            have_min_candidate = True
                            ro.error = float(error)
                            ro.inlier, ro.outlier = cs["inlier"], cs["outlier"]
                            ro.outlier_ratio = outlier_ratio_old
                            ro.valid = cs["valid"]
                            ro.residual = ddiv(ro.error, float(ro.valid))  # :746
                            ro.inlier_residual = float(fdiv(F32(cs["inlier_residual"]), ro.inlier))
                            ro.invalid = cs["invalid"]
                            loop_closure = bool(rel_error_all < F32(p["residual_threshold"])) or \
                                (float(residual) - result_new_residual) < 0.1
                            if loop_closure:
                                pose_old = mul4(pose_prior, g["gn_pose"])  # :752
                                pipe.set_pose_old(pose_old)
            if have_min_candidate:  # :762-774
                current_pose_old = pipe.pose(1)
                cand = (self.timestamp, loop_closure_timestamp,
                        mul4(rigid_inv(current_pose_old), self.graph.pose(loop_closure_timestamp)))
                self.candidate_to = loop_closure_timestamp
                self.unverified.append(cand)

        valid_ratio_old = fdiv(ro.valid, ro.valid + ro.invalid)  # :781-786
        outlier_ratio_old = fdiv(ro.outlier, ro.outlier + ro.inlier)
        self.loop_valid_ratio = fdiv(valid_ratio_old, valid_ratio_new)
        self.loop_outlier_ratio = fdiv(outlier_ratio_old, outlier_ratio_new)
        self.loop_relative_error_all = F32(ddiv(ro.residual, result_new_residual))
        self.posegraph_error = self.graph.error()

    def scan(self, pts, lab, prob):
        self.integrate()  # :179
        self.pipe.begin(pts, lab, prob)
        self.pipe.update_pose(self.iterations)
        if self.timestamp > 0:
            self.odometry_edge()
            self.check()  # :196
        self.pipe.update_map()
        self.timestamp += 1
        return self.status()


def status_equal(a, b, skip=()):
    """two status dicts (LoopStatus.as_dict() or LoopClosing.status()): every field, floats by their bits (one NaN
    equals another); returns the names that differ"""
    bad = []
    for k, va in a.items():
        if k in skip:
            continue
        vb = b[k]
        if isinstance(va, dict):
            bad += [f"{k}.{x}" for x in status_equal(va, vb)]
        elif k in ("result_old_outlier_ratio", "loop_valid_ratio", "loop_outlier_ratio", "loop_relative_error_all"):
            fa, fb = F32(va), F32(vb)
            if not ((np.isnan(fa) and np.isnan(fb)) or fa.tobytes() == fb.tobytes()):
                bad.append(k)
        elif isinstance(va, float) or isinstance(vb, float):
            da, db = np.float64(va), np.float64(vb)
            if not ((np.isnan(da) and np.isnan(db)) or da.tobytes() == db.tobytes()):
                bad.append(k)
        elif int(va) != int(vb):
            bad.append(k)
    return bad


# ---- the scenario of the loop-closing tests: tests/loop_scenario.py's circle at 0.7 m per scan (a lap of 153 scans, longer
# than the 100 scans after which surfels turn inactive), 900 x 64, 8 fixed iterations.  With the search distance of 20 m the
# reference's rules queue their first candidate at scan 123 and it passes every gate -- no candidate ever fails.  At 30 m
# the search reaches back as soon as delta_timestamp allows (scan 101, 30 m across the circle from scan 0), where the
# inactive map is still a poor match: candidates are found and dropped for ten scans before one holds.  Everything the
# tests need has happened by scan 140, so the run ends there instead of at lap + 30.
STEP = 0.7
N_SCANS = 140
SCENARIO = dict(min_trajectory_distance=60.0, search_distance=30.0, delta_timestamp=100)
_SCANS = {}


def scenario_scan(k, W, H):
    import loop_scenario as ls
    from semantic_suma_amd import synth
    if (k, W, H) not in _SCANS:
        _SCANS[(k, W, H)] = synth.generate_scan(k, n_azimuth=W, height=H, pose=ls.circle_pose(k, step=STEP))[:3]
    return _SCANS[(k, W, H)]


def scenario_length():
    return N_SCANS


def run_scenario(lc, W, H, n_scans, on_scan=None):
    """drives a LoopClosing through the scenario; returns the per-scan status log"""
    log = []
    for k in range(n_scans):
        log.append(lc.scan(*scenario_scan(k, W, H)))
        if on_scan is not None:
            on_scan(k, lc)
    return log
