"""TEST INFRASTRUCTURE: a plain fp64 / exact-rational reference of the Gauss-Newton step that consumes K6's sums
(LieGaussNewton::step: solve, exp, the three stopping rules), and crafted 6 x 6 systems for it.

Nothing here shares code, operation order or number format with oracle/o_icp.c or csrc/k_icp.hip.  The solve is exact
(fractions.Fraction Gaussian elimination on the 2^-28 fixed-point words, which ARE exact rationals), the exponential is
k6_ref.se3_exp, the rules are written down from LieGaussNewton.cpp:64-66.  numpy + fractions only; this is a helper
module, not a conftest.

    system_frames(rows, W, H, params, T0)   frames (nearest sampling) whose pairs are the listed rows J = [n, v_d x n]
    rows_for_step(J_rows, dx_target)        residuals r = -J dx_target
    exact_step(acc_words)                   (dx rounded to fp64, kappa_2(JtJ)) of the 27 fixed-point words
    step_pose(dx, T0)                       se3_exp(dx) @ T0
    stopping(...)                           which of the rules :64 / :65 / :66 fire
    ldlt_pivots_fp64(JtJ)                   the six pivots of the unpivoted LDL^T, in the stated operation order
    contained_step(JtJ, Jtr)                the containment rule: zero twist on a pivot that is not > 0
    chain_quantities(...)                   per-iteration |dx|inf, Jtr, F of the fp64 chain
    expected_chain(...)                     history / final pose / converged / iterations of a chain under the rules
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import k6_ref as K

ACC_ONE = 1 << 28


def tri(i, j):
    """word of JtJ entry (i, j), i <= j: row-major upper triangle"""
    return i * 6 - i * (i - 1) // 2 + (j - i)


# ---------------------------------------------------------------------------------------------------------------------
# crafted systems
# ---------------------------------------------------------------------------------------------------------------------
def project(v, W, H, params):
    """continuous texel coordinates of a point (the stage's projection, fp64)"""
    fov_up, fov_down = abs(float(params.data_fov_up)), abs(float(params.data_fov_down))
    v = np.asarray(v, dtype=np.float64)
    yaw = np.arctan2(v[1], v[0])
    pitch = -np.arcsin(v[2] / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    return 0.5 * (1.0 - yaw / np.pi) * W, (1.0 - (np.rad2deg(pitch) + fov_up) / (fov_up + fov_down)) * H


def system_frames(rows, W, H, params, T0):
    """rows: dict(at=(x, y), n=(3), r=float, and range=float | v=(3)).  The data vertex (given in the frame the stage
    works in, i.e. AFTER T0) lies on the ray of texel `at` at `range`, or is the stated point `v` (which must project
    into `at`); the model texel at `at` holds v_m = v_d - r n and the normal n.  Each row is one inlier pair with
    J = [n, v_d x n] and residual r.  Returns ((Vd, Nd, Sd), (Vm, Nm, Sm)), float32."""
    T0 = np.asarray(T0, dtype=np.float64)
    R0, t0 = T0[:3, :3], T0[:3, 3]
    rays = K.texel_rays(W, H, params)
    pixels, patch, seen = [], [], set()
    for row in rows:
        x, y = row["at"]
        assert (x, y) not in seen, "one row per texel"
        seen.add((x, y))
        n = np.asarray(row["n"], dtype=np.float64)
        v_d = np.asarray(row["v"], dtype=np.float64) if "v" in row else float(row["range"]) * rays[y, x]
        ix, iy = project(v_d, W, H, params)
        assert (int(np.floor(ix)), int(np.floor(iy))) == (x, y), f"{v_d} projects to ({ix}, {iy}), not into {(x, y)}"
        v_m = v_d - float(row["r"]) * n
        p_s, n_s = R0.T @ (v_d - t0), R0.T @ n  # what T0 carries onto v_d / n
        pixels.append(dict(at=(x, y), v=tuple(float(np.float32(c)) for c in p_s), n=tuple(float(np.float32(c)) for c in n_s)))
        patch.append((x, y, (*v_m, 1.0), (*n, 1.0), None))
    return K.single_pixel_frames(W, H, pixels, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), model_patch=patch)


def row_jacobian(row, W, H, params):
    """J = [n, v_d x n] of a row, fp64"""
    n = np.asarray(row["n"], dtype=np.float64)
    x, y = row["at"]
    v = np.asarray(row["v"], dtype=np.float64) if "v" in row else float(row["range"]) * K.texel_rays(W, H, params)[y, x]
    return np.concatenate([n, np.cross(v, n)])


def rows_for_step(J_rows, dx_target):
    """residuals r = -J dx_target: six independent rows then give the step dx_target (up to fp32 storage)"""
    return [-float(np.dot(np.asarray(J, dtype=np.float64), np.asarray(dx_target, dtype=np.float64))) for J in J_rows]


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------
def words_system(acc_words):
    """(JtJ 6 x 6, Jtr 6) of the fixed-point words, as exact rationals"""
    A = [[Fraction(int(acc_words[tri(min(i, j), max(i, j))]), ACC_ONE) for j in range(6)] for i in range(6)]
    b = [Fraction(int(acc_words[21 + i]), ACC_ONE) for i in range(6)]
    return A, b


def exact_step(acc_words):
    """dx = -JtJ^-1 Jtr of the 27 fixed-point words, solved in exact rational arithmetic and rounded once to fp64;
    and kappa_2(JtJ) (numpy).  Raises ZeroDivisionError on a singular system."""
    A, b = words_system(acc_words)
    M = [A[i] + [-b[i]] for i in range(6)]
    for c in range(6):
        piv = next((r for r in range(c, 6) if M[r][c] != 0), None)
        if piv is None:
            raise ZeroDivisionError("singular system")
        M[c], M[piv] = M[piv], M[c]
        for r in range(6):
            if r != c and M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [a - f * p for a, p in zip(M[r], M[c])]
    dx = np.array([float(M[i][6] / M[i][i]) for i in range(6)])
    return dx, float(np.linalg.cond(np.array([[float(a) for a in row] for row in A])))


def step_pose(dx, T0):
    return K.se3_exp(dx) @ np.asarray(T0, dtype=np.float64)


def stopping(dx_inf, Jtr, F, last_F, epsilon, delta):
    """(rule :64, rule :65, rule :66) of LieGaussNewton.cpp: the step is small; the SIGNED maximum of Jtr (not the
    largest magnitude) is small in magnitude; the error fell, by little"""
    return (bool(dx_inf < delta), bool(abs(max(float(x) for x in Jtr)) < epsilon),
            bool(F < last_F and abs(F - last_F) < epsilon))


def ldlt_pivots_fp64(JtJ):
    """d_j = A_jj - sum_k<j (L_jk L_jk) D_k, L_ij = (A_ij - sum_k<j (L_ik L_jk) D_k) / d_j: no pivoting, plain floats"""
    A = [[float(JtJ[i][j]) for j in range(6)] for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    with np.errstate(all="ignore"):
        for j in range(6):
            d = np.float64(A[j][j])
            for k in range(j):
                d = d - (L[j][k] * L[j][k]) * D[k]
            D[j] = d
            for i in range(j + 1, 6):
                s = np.float64(A[i][j])
                for k in range(j):
                    s = s - (L[i][k] * L[j][k]) * D[k]
                L[i][j] = s / d
    return [float(d) for d in D]


def contained_step(JtJ, Jtr):
    """the containment rule: any pivot not > 0 (zero, negative, NaN) or any non-finite component -> the zero twist"""
    if not all(d > 0.0 for d in ldlt_pivots_fp64(JtJ)):
        return np.zeros(6)
    dx = np.linalg.solve(np.asarray(JtJ, dtype=np.float64), -np.asarray(Jtr, dtype=np.float64))
    return dx if np.all(np.isfinite(dx)) else np.zeros(6)


FLOAT_MAX = float(np.finfo(np.float32).max)  # last_error at the start, LieGaussNewton.cpp:48


def chain_quantities(params, data, model, T0, n):
    """n fp64 Gauss-Newton steps from T0: (poses [T0 .. Tn], per-iteration dict(dx_inf, Jtr, max_jtr, F, dF, counts))"""
    T = np.asarray(T0, dtype=np.float64).copy()
    poses, q, last = [T.copy()], [], FLOAT_MAX
    for k in range(n):
        s = K.k6_fp64(params, data, model, T, k)
        dx = contained_step(s["JtJ"], s["Jtr"])
        q.append(dict(dx_inf=float(np.max(np.abs(dx))), Jtr=s["Jtr"], max_jtr=float(np.max(s["Jtr"])), F=s["F"],
                      dF=abs(s["F"] - last), counts=s["counts"], margin=s["margin"]))
        last = s["F"]
        T = K.se3_exp(dx) @ T
        poses.append(T.copy())
    return poses, q


def expected_chain(params, data, model, T0, max_iterations, epsilon, delta):
    """LieGaussNewton::minimize in plain fp64 under the three rules and the containment rule:
    dict(history, final, converged, iterations, counts).  A converged step is applied and not pushed."""
    assert max_iterations >= 1
    T = np.asarray(T0, dtype=np.float64).copy()
    history, last, k, counts = [], FLOAT_MAX, 0, None
    while True:
        history.append(T.copy())
        if k >= max_iterations:
            return dict(history=history, final=T, converged=0, iterations=k, counts=counts)
        s = K.k6_fp64(params, data, model, T, k)
        counts = s["counts"]
        dx = contained_step(s["JtJ"], s["Jtr"])
        fired = stopping(float(np.max(np.abs(dx))), s["Jtr"], s["F"], last, epsilon, delta)
        last = s["F"]
        T = K.se3_exp(dx) @ T
        if any(fired):
            return dict(history=history, final=T, converged=1, iterations=k, counts=counts, fired=fired)
        k += 1
