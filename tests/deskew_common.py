"""Shared by the tests of the motion compensation of raw sweeps (test_deskew_host.py, test_abi_deskew.py,
test_gpu_deskew.py): the host restatement tests/deskew_shim.c of csrc/k_deskew.hip, an fp64 numpy restatement that
shares nothing with it (logarithm by a linear solve, exponential by the matrix series / closed form), crafted points
and motions on every boundary of the specification, and the scenario -- loop_scenario's circle (17 m radius, 1.1 m a
scan) at 360 x 32, once as instantaneous scans and once as RAW sweeps: every azimuth column cast from the pose of its own
instant (synth.generate_scan(column_poses=...)), the scan's pose being the one at mid-sweep."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from loop_scenario import circle_pose
from semantic_suma_amd import synth
from semantic_suma_amd.types import DESKEW_TIME_AZIMUTH, DESKEW_TIME_TIMES, DeskewParams, params_with_size

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_THETA = 1e-6  # SUMA_DESKEW_SMALL_THETA

# Figures measured on the host restatement (test_deskew_host.py prints them again on every run); the asserts that use
# them are stated in the tests.
MEASURED = dict(
    # worst |shim - fp64| over the crafted set, metres (test 1): asserted <= 4 x this and <= 1e-3
    shim_vs_fp64=1.1e-5,
    # median distance to the instantaneous scan from the t_ref pose, static surfaces, metres (test 2)
    geometry_before=0.354, geometry_after=0.0269,
    # mean relative translation error per scan, scans 3 .. 59, metres (test 3): control, raw, corrected
    odo_control=0.0188, odo_uncorrected=0.0575, odo_corrected=0.0151,
    # the localiser on raw scans 20 .. 59 in the map of the instantaneous ones (test 4): worst error, scans tracked
    loc_worst_off=0.4835, loc_worst_on=0.0464, loc_tracked_off=40, loc_tracked_on=40,
)


class Twist(C.Structure):
    _fields_ = [("v", C.c_float * 3), ("a", C.c_float * 3), ("b", C.c_float * 3), ("c", C.c_float * 3),
                ("theta", C.c_float), ("inv_theta", C.c_float)]


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "deskew_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "deskew_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.deskew_shim_twist.argtypes = [vp, C.c_float, C.POINTER(Twist)]
    L.deskew_shim_twist.restype = None
    L.deskew_shim_points.argtypes = [C.POINTER(DeskewParams), vp, vp, C.c_uint32, vp, vp]
    L.deskew_shim_points.restype = None
    return L


def _cm(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4).T)


def shim_points(shim, points, motion, dp: DeskewParams = None, times=None):
    """the specification on N x 4 points; motion row-major 4x4"""
    dp = DeskewParams.defaults() if dp is None else dp
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
    tm = None if times is None else np.ascontiguousarray(times, dtype=np.float32)
    out = np.empty_like(pts)
    M = _cm(motion)
    shim.deskew_shim_points(C.byref(dp), pts.ctypes.data, None if tm is None else tm.ctypes.data, pts.shape[0],
                            M.ctypes.data, out.ctypes.data)
    return out


# ---- fp64, written from the operation  p' = Exp((s - t_ref) * scale * Log(motion)) * p  alone

def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _coeffs(phi):
    """sin(phi)/phi, (1 - cos phi)/phi^2, (phi - sin phi)/phi^3, by their series below 1e-2"""
    phi = np.asarray(phi, dtype=np.float64)
    small = np.abs(phi) < 1e-2
    p = np.where(small, 1.0, phi)
    A = np.where(small, 1 - phi ** 2 / 6 + phi ** 4 / 120, np.sin(p) / p)
    B = np.where(small, 0.5 - phi ** 2 / 24 + phi ** 4 / 720, (1 - np.cos(p)) / p ** 2)
    Cc = np.where(small, 1 / 6 - phi ** 2 / 120 + phi ** 4 / 5040, (p - np.sin(p)) / p ** 3)
    return A, B, Cc


def se3_log64(T):
    """(v, w) of a rigid motion: w from the rotation's skew part, v by solving V(w) v = t"""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    q = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = np.linalg.norm(q), 0.5 * (np.trace(R) - 1.0)
    theta = math.atan2(sn, cs)
    w = q * (theta / sn) if sn > 0 else np.zeros(3)
    if theta < SMALL_THETA:  # the specification's pure translation
        return t.copy(), np.zeros(3)
    _, B, Cc = _coeffs(theta)
    W = _hat(w)
    V = np.eye(3) + B * W + Cc * (W @ W)
    return np.linalg.solve(V, t), w


def sweep_fraction64(points, dp: DeskewParams):
    p = np.asarray(points, dtype=np.float64)
    az = np.arctan2(p[:, 1], p[:, 0])
    az = np.where((p[:, 0] == 0) & (p[:, 1] == 0), 0.0, az)
    u = (az - float(dp.start_azimuth)) / (2 * math.pi)
    u = u - np.floor(u)
    return 1.0 - u if dp.clockwise else u


def numpy_deskew(points, motion, dp: DeskewParams = None, times=None, s=None):
    """fp64 result (N x 3) and the mask of the points the operation moves (finite coordinates and time).  ``s``: sweep
    fractions to use instead of the time source's (the azimuth wrap is a discontinuity: a point within rounding of it is
    compared at the fraction the fp32 specification gave it)"""
    dp = DeskewParams.defaults() if dp is None else dp
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 4)
    p = pts[:, :3].astype(np.float64)
    if s is None:
        s = np.asarray(times, dtype=np.float64) if dp.time_source == DESKEW_TIME_TIMES else sweep_fraction64(np.nan_to_num(p), dp)
    moved = np.all(np.isfinite(p), axis=1) & np.isfinite(s)
    v, w = se3_log64(motion)
    v, w = float(dp.scale) * v, float(dp.scale) * w
    d = np.where(moved, s - float(dp.t_ref), 0.0)
    W, W2 = _hat(w), _hat(w) @ _hat(w)
    A, B, Cc = _coeffs(d * np.linalg.norm(w))
    pm = np.nan_to_num(p)
    out = pm + (A * d)[:, None] * (pm @ W.T) + (B * d * d)[:, None] * (pm @ W2.T)
    dv = d[:, None] * v[None, :]
    out += dv + (B * d)[:, None] * (dv @ W.T) + (Cc * d * d)[:, None] * (dv @ W2.T)
    return out, moved


# ---- crafted input

def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = _hat(a)
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _rigid(axis, angle, t):
    T = np.eye(4)
    T[:3, :3] = _rot(axis, angle)
    T[:3, 3] = t
    return T


MOTIONS = {
    "identity": np.eye(4),
    "translation": _rigid((0, 0, 1), 0.0, (1.1, -0.2, 0.05)),
    "rotation_tilted": _rigid((0.3, -0.2, 0.9), 0.07, (0.0, 0.0, 0.0)),
    "general": _rigid((0.05, 0.1, 1.0), 0.07, (1.1, 0.04, -0.01)),           # about (1.1 m, 0.07 rad)
    "below_small_angle": _rigid((0.1, 0.2, 1.0), 0.5 * SMALL_THETA, (1.1, 0.1, 0.0)),
    "above_small_angle": _rigid((0.1, 0.2, 1.0), 2.0 * SMALL_THETA, (1.1, 0.1, 0.0)),
}
TIMES = np.array([0.0, 1.0, -0.25, 1.5, np.nan], dtype=np.float32)
BLOCK_EDGES = (0, 1, 255, 256, 257, 1023, 1025, 5000)


def crafted_points():
    """radii 0.5 .. 120 m all round at several heights; the azimuth wrap (y = +0 / -0, x < 0) and the start azimuths of
    the cases; x = y = 0; NaN and inf coordinates; remissions with arbitrary bits (a NaN payload among them)"""
    rng = np.random.default_rng(7)
    rows = []
    for r in (0.5, 2.0, 9.7, 31.0, 75.0, 120.0):
        for az in np.linspace(-math.pi, math.pi, 37):
            for el in (-0.4, -0.05, 0.03):
                rows.append((r * math.cos(az) * math.cos(el), r * math.sin(az) * math.cos(el), r * math.sin(el)))
    P = np.array(rows, dtype=np.float32)
    special = np.array([(-5.0, 0.0, 1.0), (-5.0, -0.0, 1.0), (-120.0, 0.0, -2.0), (-0.5, -0.0, 0.0), (5.0, 0.0, 0.0),
                        (5.0, -0.0, 0.0), (0.0, 0.0, 3.0), (0.0, -0.0, -1.5), (-0.0, 0.0, 0.0), (0.0, 7.0, 0.0), (0.0, -7.0, 0.0),
                        (3.0 * math.cos(0.7), 3.0 * math.sin(0.7), 0.1),  # on the non-zero start azimuth of the cases
                        (np.nan, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, np.nan), (np.inf, 1.0, 1.0), (1.0, -np.inf, 1.0),
                        (1.0, 1.0, np.inf), (np.nan, np.nan, np.nan)], dtype=np.float32)
    xyz = np.concatenate([P, special])
    pts = np.empty((len(xyz), 4), dtype=np.float32)
    pts[:, :3] = xyz
    w = rng.integers(0, 2 ** 32, len(xyz), dtype=np.uint64).astype(np.uint32)
    w[:4] = (0x7fc00001, 0xff800000, 0x80000000, 0x00000001)
    pts[:, 3] = w.view(np.float32)
    return pts


def crafted_times(n):
    """the five stated fractions, then fractions all over [0, 1]"""
    t = np.random.default_rng(11).uniform(0.0, 1.0, n).astype(np.float32)
    t[:len(TIMES)] = TIMES
    t[len(TIMES):2 * len(TIMES)] = TIMES[::-1]
    return t


def cases():
    """(name, DeskewParams, uses times) over t_ref, the sense of rotation, the start azimuth, the scale and both sources"""
    out = []
    for t_ref in (0.0, 0.5, 1.0):
        for cw in (0, 1):
            out.append((f"az-tref{t_ref}-cw{cw}", DeskewParams.defaults(t_ref=t_ref, clockwise=cw), False))
    out.append(("az-start0.7", DeskewParams.defaults(start_azimuth=0.7), False))
    out.append(("az-start-2.5-cw", DeskewParams.defaults(start_azimuth=-2.5, clockwise=1, t_ref=1.0), False))
    out.append(("az-scale0.5", DeskewParams.defaults(scale=0.5), False))
    for t_ref in (0.0, 0.5, 1.0):
        out.append((f"times-tref{t_ref}", DeskewParams.defaults(time_source=DESKEW_TIME_TIMES, t_ref=t_ref), True))
    return out


def tiled(points, n):
    """n points: the crafted set repeated / cut"""
    reps = -(-max(n, 1) // len(points))
    return np.ascontiguousarray(np.tile(points, (reps, 1))[:n])


# ---- the scenario

W, H, N_SCANS = 360, 32, 60
_CACHE = {}


def params(**kw):
    return params_with_size(W, H, **kw)


def sweep_pose(k, s):
    """the sensor's pose at fraction s of sweep k: the scan's pose circle_pose(k) is the one at mid-sweep"""
    return circle_pose(k - 0.5 + s)


def true_motion(k):
    """the sensor's motion over sweep k"""
    return np.linalg.inv(sweep_pose(k, 0.0)) @ sweep_pose(k, 1.0)


def control_scan(k):
    key = ("control", k)
    if key not in _CACHE:
        _CACHE[key] = synth.generate_scan(k, n_azimuth=W, height=H, pose=circle_pose(k))[:3]
    return _CACHE[key]


def raw_scan(k):
    """sweep k as a counter-clockwise sensor that starts at azimuth 0 delivers it"""
    key = ("raw", k)
    if key not in _CACHE:
        _CACHE[key] = synth.generate_scan(k, n_azimuth=W, height=H, pose=circle_pose(k),
                                          column_poses=lambda s: np.stack([sweep_pose(k, float(x)) for x in s]))[:3]
    return _CACHE[key]


def odometry_error(poses, first=3):
    """mean over scans first .. end of |translation of inc_true^-1 inc_est|, the increments between consecutive scans;
    and the worst drift relative to scan `first`"""
    errs = []
    for k in range(first, len(poses)):
        est = np.linalg.inv(poses[k - 1]) @ poses[k]
        tru = np.linalg.inv(circle_pose(k - 1)) @ circle_pose(k)
        errs.append(float(np.linalg.norm((np.linalg.inv(tru) @ est)[:3, 3])))
    drift = 0.0
    for k in range(first, len(poses)):
        est = np.linalg.inv(poses[first]) @ poses[k]
        tru = np.linalg.inv(circle_pose(first)) @ circle_pose(k)
        drift = max(drift, float(np.linalg.norm(est[:3, 3] - tru[:3, 3])))
    return float(np.mean(errs)), drift


def assert_odometry(control, uncorrected, corrected):
    """the assertions of the 60-scan run, shared by the CPU oracle and the device"""
    print("mean relative translation error, scans 3 ..: control %.4f m, raw %.4f m, corrected %.4f m"
          % (control, uncorrected, corrected))
    assert corrected <= 2.0 * control, (corrected, control)
    assert uncorrected >= 2.0 * corrected, (uncorrected, corrected)
    assert corrected <= 1.5 * MEASURED["odo_corrected"], (corrected, MEASURED["odo_corrected"])
