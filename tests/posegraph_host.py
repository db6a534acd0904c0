"""fp64 host restatement of the pose-graph optimiser (numpy + scipy.sparse): the yardstick of the HIP back end.

It states the mathematics of DESIGN.md "Pose graph" once more, independently of the kernels in
semantic_suma_amd/csrc/k_posegraph.hip:

* factor 0 is the prior on node 0 (P = identity, information 1e6 I), factors 1.. are the edges in insertion order;
* between factor e = Log(Z^-1 Xi^-1 Xj), prior e = Log(X0); tangent order [omega, v]; retraction X <- X Exp(delta);
* Jacobians de/dxj = Jr^-1(e), de/dxi = -Jr^-1(e) Ad((Xi^-1 Xj)^-1);
* total error 0.5 sum e^T Omega e;
* Levenberg-Marquardt with the rules of ``levenberg_marquardt`` below, the damped system solved directly
  (scipy.sparse.linalg.spsolve) where the device runs preconditioned CG.

Poses are row-major 4x4 numpy matrices.  Everything is vectorised over the factors.
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

SERIES_THETA = 0.5  # below this angle every coefficient is its Taylor series (no cancellation)

# Taylor coefficients in theta^2 (Horner order: constant first)
_A = [1.0, -1 / 6, 1 / 120, -1 / 5040, 1 / 362880, -1 / 39916800, 1 / 6227020800]          # sin(t)/t
_B = [1 / 2, -1 / 24, 1 / 720, -1 / 40320, 1 / 3628800, -1 / 479001600, 1 / 87178291200]   # (1-cos t)/t^2
_C = [1 / 6, -1 / 120, 1 / 5040, -1 / 362880, 1 / 39916800, -1 / 6227020800, 1 / 1307674368000]  # (t-sin t)/t^3
_D = [1 / 12, 1 / 720, 1 / 30240, 1 / 1209600, 1 / 47900160, 691 / 1307674368000, 7 / 523069747200]  # 1/t^2-cot(t/2)/(2t)
_QB = [1 / 24, -1 / 720, 1 / 40320, -1 / 3628800, 1 / 479001600, -1 / 87178291200, 1 / 20922789888000]
_QC = [1 / 120, -1 / 2520, 1 / 120960, -1 / 9979200, 1 / 1245404160, -1 / 217945728000, 1 / 50812489728000]


def _series(c, t2):
    r = np.full_like(t2, c[-1])
    for k in c[-2::-1]:
        r = r * t2 + k
    return r


def coefficients(theta):
    """A, B, C, D, b, c of DESIGN.md as arrays over theta (series below SERIES_THETA, closed forms above)"""
    th = np.asarray(theta, dtype=np.float64)
    t2 = th * th
    small = th < SERIES_THETA
    ts = np.where(small, 1.0, th)  # keeps the closed forms finite where the series is taken
    s, c = np.sin(ts), np.cos(ts)
    A = np.where(small, _series(_A, t2), s / ts)
    B = np.where(small, _series(_B, t2), (1 - c) / (ts * ts))
    C = np.where(small, _series(_C, t2), (ts - s) / (ts * ts * ts))
    D = np.where(small, _series(_D, t2), 1 / (ts * ts) - np.cos(ts / 2) / np.sin(ts / 2) / (2 * ts))
    qb = np.where(small, _series(_QB, t2), (ts * ts + 2 * c - 2) / (2 * ts ** 4))
    qc = np.where(small, _series(_QC, t2), (2 * ts - 3 * s + ts * c) / (2 * ts ** 5))
    return A, B, C, D, qb, qc


def hat(w):
    w = np.asarray(w, dtype=np.float64)
    H = np.zeros(w.shape[:-1] + (3, 3))
    H[..., 0, 1], H[..., 0, 2] = -w[..., 2], w[..., 1]
    H[..., 1, 0], H[..., 1, 2] = w[..., 2], -w[..., 0]
    H[..., 2, 0], H[..., 2, 1] = -w[..., 1], w[..., 0]
    return H


def _mm(*Ms):
    r = Ms[0]
    for M in Ms[1:]:
        r = np.matmul(r, M)
    return r


def so3_log(R):
    R = np.asarray(R, dtype=np.float64)
    w = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = np.linalg.norm(w, axis=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    th = np.arctan2(s, c)
    f = np.where(s > 0, th / np.where(s > 0, s, 1.0), 1.0)
    om = f[..., None] * w
    far = c < -0.5  # near pi the skew part loses the axis: take it from the symmetric part
    if np.any(far):
        Rf, cf, wf, thf = R[far], c[far], w[far], th[far]
        Bm = 0.5 * (Rf + np.swapaxes(Rf, -1, -2)) - cf[:, None, None] * np.eye(3)
        d = np.stack([Bm[:, 0, 0], Bm[:, 1, 1], Bm[:, 2, 2]], -1)
        k = np.argmax(d, axis=-1)
        a = Bm[np.arange(len(k)), :, k]
        a = a / np.linalg.norm(a, axis=-1)[:, None]
        sgn = np.where(np.sum(a * wf, -1) < 0, -1.0, 1.0)
        om[far] = (sgn * thf)[:, None] * a
    return om


def se3_exp(xi):
    xi = np.asarray(xi, dtype=np.float64)
    om, v = xi[..., :3], xi[..., 3:]
    th = np.linalg.norm(om, axis=-1)
    A, B, C, _, _, _ = coefficients(th)
    W = hat(om)
    W2 = W @ W
    I = np.eye(3)
    T = np.zeros(xi.shape[:-1] + (4, 4))
    T[..., :3, :3] = I + A[..., None, None] * W + B[..., None, None] * W2
    V = I + B[..., None, None] * W + C[..., None, None] * W2
    T[..., :3, 3] = np.einsum("...ij,...j->...i", V, v)
    T[..., 3, 3] = 1.0
    return T


def se3_log(T):
    T = np.asarray(T, dtype=np.float64)
    om = so3_log(T[..., :3, :3])
    t = T[..., :3, 3]
    th = np.linalg.norm(om, axis=-1)
    D = coefficients(th)[3]
    wt = np.cross(om, t)
    v = t - 0.5 * wt + D[..., None] * np.cross(om, wt)
    return np.concatenate([om, v], -1)


def jr_inv(xi):
    """right Jacobian inverse of SE(3) at xi, [omega, v] order"""
    xi = np.asarray(xi, dtype=np.float64)
    om, v = xi[..., :3], xi[..., 3:]
    th = np.linalg.norm(om, axis=-1)
    _, _, C, D, qb, qc = coefficients(th)
    W, V = hat(om), hat(v)
    I = np.eye(3)
    Ji = I + 0.5 * W + D[..., None, None] * (W @ W)
    WV, VW, WVW = W @ V, V @ W, _mm(W, V, W)
    WWV, VWW = W @ WV, VW @ W
    Q = (-0.5 * V + C[..., None, None] * (WV + VW - WVW) - qb[..., None, None] * (WWV + VWW - 3 * WVW)
         + qc[..., None, None] * (WVW @ W + W @ WVW))
    J = np.zeros(xi.shape[:-1] + (6, 6))
    J[..., :3, :3] = Ji
    J[..., 3:, 3:] = Ji
    J[..., 3:, :3] = -_mm(Ji, Q, Ji)
    return J


def adjoint(T):
    T = np.asarray(T, dtype=np.float64)
    R, t = T[..., :3, :3], T[..., :3, 3]
    Ad = np.zeros(T.shape[:-2] + (6, 6))
    Ad[..., :3, :3] = R
    Ad[..., 3:, 3:] = R
    Ad[..., 3:, :3] = hat(t) @ R
    return Ad


def inv(T):
    T = np.asarray(T, dtype=np.float64)
    R, t = T[..., :3, :3], T[..., :3, 3]
    out = np.zeros_like(T)
    Rt = np.swapaxes(R, -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ij,...j->...i", Rt, t)
    out[..., 3, 3] = 1.0
    return out


def _rigid(T):
    """a 4x4 with the bottom row forced to [0 0 0 1] (only the top 3 x 4 of a pose is read, as on the device)"""
    out = np.array(T, dtype=np.float64)
    out[..., 3, :] = [0.0, 0.0, 0.0, 1.0]
    return out


def compose(A, B):
    A, B = np.asarray(A), np.asarray(B)
    out = np.zeros(np.broadcast_shapes(A.shape, B.shape))
    out[..., :3, :3] = A[..., :3, :3] @ B[..., :3, :3]
    out[..., :3, 3] = np.einsum("...ij,...j->...i", A[..., :3, :3], B[..., :3, 3]) + A[..., :3, 3]
    out[..., 3, 3] = 1.0
    return out


PRIOR_INFORMATION = 1e6  # Posegraph.cpp:41-44: variances 1e-6 -> information 1e6 I

DEFAULTS = dict(lambda_initial=1e-5, lambda_factor=10.0, lambda_upper_bound=1e5, lambda_lower_bound=0.0,
                min_model_fidelity=1e-3, relative_error_tol=1e-5, absolute_error_tol=1e-5, error_tol=0.0)

MAX_ITERATIONS, CONVERGED, LAMBDA_BOUND, ERROR_TOL = 0, 1, 2, 3


class HostGraph:
    """nodes: list of 4x4; edges: (from, to, Z 4x4, information 6x6 in [omega, v] order)"""

    def __init__(self, nodes=(), edges=()):
        self.nodes = [_rigid(T) for T in nodes]
        self.edges = [(int(a), int(b), _rigid(Z), 0.5 * (np.asarray(O, float) + np.asarray(O, float).T))
                      for a, b, Z, O in edges]

    def factors(self):
        """(from, to, Z, Omega) arrays with the prior as factor 0 (from = -1)"""
        m = len(self.edges) + 1
        fr = np.array([-1] + [e[0] for e in self.edges], dtype=np.int64)
        to = np.array([0] + [e[1] for e in self.edges], dtype=np.int64)
        Z = np.stack([np.eye(4)] + [e[2] for e in self.edges]) if m > 1 else np.eye(4)[None]
        O = np.stack([PRIOR_INFORMATION * np.eye(6)] + [e[3] for e in self.edges]) if m > 1 \
            else (PRIOR_INFORMATION * np.eye(6))[None]
        return fr, to, Z, O


def factor_terms(graph, X):
    """per factor: e (m x 6), Ji, Jj (m x 6 x 6; Ji = 0 for the prior), energy 0.5 e^T Omega e (m)"""
    fr, to, Z, O = graph.factors()
    X = np.asarray(X, dtype=np.float64)
    Xi = np.where((fr >= 0)[:, None, None], X[np.maximum(fr, 0)], np.eye(4))
    Xj = X[to]
    Tij = compose(inv(Xi), Xj)
    E = compose(inv(Z), Tij)
    e = se3_log(E)
    Jj = jr_inv(e)
    Ji = -Jj @ adjoint(inv(Tij))
    Ji[fr < 0] = 0.0
    energy = 0.5 * np.einsum("fi,fij,fj->f", e, O, e)
    return e, Ji, Jj, energy


def error(graph, X):
    return float(np.sum(factor_terms(graph, X)[3]))


def linearize(graph, X):
    """gradient g (6n), Hessian H (scipy csr, 6n x 6n), per-factor e and energy"""
    n = len(X)
    fr, to, Z, O = graph.factors()
    e, Ji, Jj, energy = factor_terms(graph, X)
    Oe = np.einsum("fij,fj->fi", O, e)
    g = np.zeros((n, 6))
    np.add.at(g, to, np.einsum("fji,fj->fi", Jj, Oe))
    has = fr >= 0
    np.add.at(g, fr[has], np.einsum("fji,fj->fi", Ji[has], Oe[has]))
    OJi, OJj = O @ Ji, O @ Jj
    JiT, JjT = np.swapaxes(Ji, -1, -2), np.swapaxes(Jj, -1, -2)
    blocks = [(to, to, JjT @ OJj)]
    blocks += [(fr[has], fr[has], (JiT @ OJi)[has]), (fr[has], to[has], (JiT @ OJj)[has]),
               (to[has], fr[has], (JjT @ OJi)[has])]
    rows, cols, vals = [], [], []
    ii, jj = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    for a, b, Bk in blocks:
        rows.append((6 * a[:, None, None] + ii).ravel())
        cols.append((6 * b[:, None, None] + jj).ravel())
        vals.append(Bk.ravel())
    H = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))
    return g.ravel(), H, e, energy


def retract(X, delta):
    return compose(X, se3_exp(np.asarray(delta).reshape(-1, 6)))


def levenberg_marquardt(graph, X0=None, max_iterations=100, **params):
    """the LM rules of DESIGN.md (gtsam's LevenbergMarquardtOptimizer with its default parameters); returns
    (poses n x 4 x 4, stats dict)"""
    p = dict(DEFAULTS, **params)
    X = np.array(graph.nodes if X0 is None else X0, dtype=np.float64)
    n = len(X)
    err = error(graph, X)
    lam = p["lambda_initial"]
    st = dict(iterations=0, initial_error=err, final_error=err, lambda_=lam, termination=MAX_ITERATIONS, tries=0)
    if max_iterations == 0:
        return X, st
    if err <= p["error_tol"]:
        st["termination"] = ERROR_TOL
        return X, st
    it = 0
    while True:
        g, H, _, _ = linearize(graph, X)
        it += 1
        accepted = bound = False
        prev = err
        while True:
            st["tries"] += 1
            accepted = stop = False
            delta = spla.spsolve((H + lam * sp.identity(6 * n, format="csr")).tocsc(), -g)
            lin = -(g @ delta + 0.5 * delta @ (H @ delta))
            if lin >= 0:
                Xn = retract(X, delta)
                en = error(graph, Xn)
                change = err - en
                accepted = (bool(change / lin > p["min_model_fidelity"]) if lin > 1e-20 else True) and bool(np.isfinite(en))
                stop = accepted or abs(change) < p["relative_error_tol"] * err
            if accepted:
                X, err = Xn, en
                lam = max(p["lambda_lower_bound"], lam / p["lambda_factor"])
                break
            if stop:
                break
            lam *= p["lambda_factor"]
            if lam >= p["lambda_upper_bound"]:
                bound = True
                break
        st.update(iterations=it, final_error=err, lambda_=lam)
        if bound:
            st["termination"] = LAMBDA_BOUND
            break
        if it >= max_iterations:
            st["termination"] = MAX_ITERATIONS
            break
        if err <= p["error_tol"]:
            st["termination"] = ERROR_TOL
            break
        dec = prev - err
        if dec <= p["absolute_error_tol"] or dec / prev <= p["relative_error_tol"]:
            st["termination"] = CONVERGED
            break
    return X, st


# ---- graphs shared by the CPU and the GPU tests -------------------------------------------------------------------


def random_pose(rng, angle=None, scale=1.0):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0, math.pi) if angle is None else angle
    return se3_exp(np.concatenate([th * ax, scale * rng.normal(size=3)]))


def perturb(rng, T, rot, trans):
    return compose(T, se3_exp(np.concatenate([rot * rng.normal(size=3), trans * rng.normal(size=3)])))


def info_matrix(rng, scale=1.0):
    """a random symmetric positive-definite information matrix"""
    M = rng.normal(size=(6, 6))
    return scale * (M @ M.T / 6 + np.eye(6))


def chain_graph(n, n_loops, rng, noise=(0.01, 0.05), trajectory=None, loop_min_gap=10):
    """ground truth (n x 4 x 4), and a graph with noisy odometry edges i -> i+1, n_loops noisy loop edges from a newer
    node to an older one (as SurfelMapping.cpp:629-649 adds them), and the odometry-integrated initial estimate"""
    if trajectory is None:
        gt = [np.eye(4)]
        for k in range(1, n):
            gt.append(compose(gt[-1], se3_exp([0.0, 0.0, 0.05 * math.sin(0.01 * k), 1.0, 0.0, 0.0])))
        gt = np.array(gt)
    else:
        gt = np.asarray(trajectory, dtype=np.float64)
        gt = compose(inv(gt[0])[None], gt)  # starts at identity, like the prior
    edges = []
    Om = np.diag([1e3, 1e3, 1e3, 1e2, 1e2, 1e2])
    for i in range(n - 1):
        Z = perturb(rng, compose(inv(gt[i]), gt[i + 1]), *noise)
        edges.append((i, i + 1, Z, Om))
    for _ in range(n_loops):
        j = int(rng.integers(loop_min_gap, n))
        i = int(rng.integers(0, j - loop_min_gap + 1))
        Z = perturb(rng, compose(inv(gt[j]), gt[i]), *noise)
        edges.append((j, i, Z, Om))
    init = [np.eye(4)]
    for i in range(n - 1):
        init.append(compose(init[-1], edges[i][2]))
    return np.array(gt), HostGraph(init, edges)


# ---- one damped solve: the yardstick of k_pg_solve ----------------------------------------------------------------
#
# optimize(1) with lambda_initial = lam and both error tolerances 0 runs the first damped solve at exactly lam; when the
# step is accepted (linear_solves == 1) the poses are X0 Exp(delta), so delta = Log(X0^-1 X1) per node is the solver's
# output.  lam = SOLVE_LAMBDA = 1 throughout: at gtsam's 1e-5 two orderings of the direct solve differ by up to 2e-10
# relative on these graphs, at 1 by 1e-13 or less.

SOLVE_LAMBDA = 1.0

# every n in 1..9, then 2^k - 1, 2^k, 2^k + 1 for k = 4..10 (the edges of the cyclic reduction's level count and of its
# `e >= s`, `k + s < n`, `k + 2s < n` branches), then 1537: three trips of the stride loop at s = 1 and two at s = 2
SOLVE_CHAIN_SIZES = tuple(range(1, 10)) + tuple(2 ** k + d for k in range(4, 11) for d in (-1, 0, 1)) + (1537,)
SOLVE_LOOP_CASES = ((64, 2), (257, 3), (513, 5), (1025, 20))  # (n, distinct off-band pairs)
SOLVE_ANISOTROPIC_SIZES = (33, 513)
# Seeds of the builders below as the tests use them.  They were picked so that, on the host alone, pcg_band meets
# the iteration caps of the GPU tests and Levenberg-Marquardt accepts the step (tests/test_posegraph_host.py).
SOLVE_SEED = 7


def _perturbed(rng, hg):
    """the odometry-integrated start satisfies every chain edge: perturb every node but the first, so that a chain has
    work to do.  A single node is perturbed itself (the prior then pulls it back)"""
    if len(hg.nodes) == 1:
        hg.nodes = [perturb(rng, hg.nodes[0], 0.01, 0.1)]
    else:
        hg.nodes = [hg.nodes[0]] + [perturb(rng, T, 0.01, 0.1) for T in hg.nodes[1:]]
    return hg


def solve_chain(n, seed=SOLVE_SEED):
    rng = np.random.default_rng([seed, n])
    return _perturbed(rng, chain_graph(n, 0, rng)[1])


def solve_loop_pairs(n, L, rng):
    """L distinct off-band pairs (a, b) with a < b - 1: (0, n-1) first, then up to two more at node n-1, which so takes
    part in three of them when L >= 3 (two distinct pairs cannot give a node three), then random ones"""
    pairs = [(0, n - 1)]
    while len(pairs) < min(L, 3):
        a = int(rng.integers(1, n - 2))
        if (a, n - 1) not in pairs:
            pairs.append((a, n - 1))
    while len(pairs) < L:
        a, b = sorted(int(v) for v in rng.integers(0, n, size=2))
        if b - a >= 2 and (a, b) not in pairs:
            pairs.append((a, b))
    return pairs


def solve_loops(n, L, seed=SOLVE_SEED):
    """a perturbed chain plus loop edges on L distinct off-band pairs; returns (graph, pairs).  Pair (0, n-1) is
    there, node n-1 is in min(L, 3) pairs, the edges alternate between newer -> older and older -> newer, and the
    second pair is entered twice, once in each direction (L + 1 loop edges)"""
    rng = np.random.default_rng([seed, n, L])
    gt, hg = chain_graph(n, 0, rng)
    pairs = solve_loop_pairs(n, L, rng)
    Om = np.diag([1e3, 1e3, 1e3, 1e2, 1e2, 1e2])
    directed = [(b, a) if k % 2 == 0 else (a, b) for k, (a, b) in enumerate(pairs)]
    directed.insert(2, directed[1][::-1])
    for a, b in directed:
        hg.edges.append((a, b, perturb(rng, compose(inv(gt[a]), gt[b]), 0.01, 0.05), Om))
    return _perturbed(rng, hg), pairs


def solve_anisotropic(n, seed=SOLVE_SEED):
    """a perturbed chain whose edge information is Q diag(1e6, 1e6, 1e-3, 1e3, 1e-3, 1e3) Q^T with a random orthogonal
    Q per edge: every block has condition number 1e9 and none is diagonal"""
    rng = np.random.default_rng([seed, n, 9])
    hg = chain_graph(n, 0, rng)[1]
    d = np.array([1e6, 1e6, 1e-3, 1e3, 1e-3, 1e3])
    edges = []
    for a, b, Z, _ in hg.edges:
        Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
        edges.append((a, b, Z, (Q * d) @ Q.T))
    return _perturbed(rng, HostGraph(hg.nodes, edges))


def damped_system(graph, X, lam):
    """(A, g) of the damped normal equations A delta = -g, A = H + lam I (csr)"""
    g, H, _, _ = linearize(graph, X)
    return (H + lam * sp.identity(H.shape[0], format="csr")).tocsr(), g


def single_solve(graph, X, lam, permc_spec=None):
    """delta of (H + lam I) delta = -g by a sparse direct solve (permc_spec: SuperLU's column ordering)"""
    A, g = damped_system(graph, X, lam)
    return spla.spsolve(A.tocsc(), -g, permc_spec=permc_spec)


def band_part(A, drop_band=None):
    """the block-tridiagonal part of A (6x6 blocks); drop_band = i also leaves out the band block (i, i+1) and its
    transpose, which keeps the matrix positive-definite (two principal sub-matrices of A's band part remain)"""
    C = A.tocoo()
    bi, bj = C.row // 6, C.col // 6
    keep = np.abs(bi - bj) <= 1
    if drop_band is not None:
        keep &= ~((np.minimum(bi, bj) == drop_band) & (bi != bj))
    return sp.csc_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=A.shape)


def pcg_band(graph, X, lam, tol, max_it, drop_band=None):
    """the preconditioned CG of DESIGN.md "Pose graph" in fp64 with k_pg_solve's order of operations and its stopping
    rule !(rzn > tol^2 rz0); the preconditioner is an exact sparse factorisation of the block-tridiagonal part.
    Returns (delta, iterations).  drop_band: see band_part (a deliberately inexact preconditioner)"""
    A, g = damped_system(graph, X, lam)
    M = spla.splu(band_part(A, drop_band))
    x = np.zeros_like(g)
    r = -g
    z = M.solve(r)
    p = z.copy()
    rz = rz0 = float(r @ z)
    it = 0
    if rz0 > 0:
        while it < max_it:
            q = A @ p
            pq = float(p @ q)
            if not pq > 0:
                break
            alpha = rz / pq
            x += alpha * p
            r -= alpha * q
            it += 1
            z = M.solve(r)
            rzn = float(r @ z)
            if not rzn > tol * tol * rz0:
                break
            p = z + (rzn / rz) * p
            rz = rzn
    return x, it


def step_of(X0, X1):
    """delta with X1 = X0 Exp(delta), per node (n x 6)"""
    return se3_log(compose(inv(np.asarray(X0)), np.asarray(X1)))


def model_fidelity(graph, X, delta):
    """(error(X) - error(X Exp(delta))) / linearised decrease: Levenberg-Marquardt accepts above min_model_fidelity"""
    g, H, _, _ = linearize(graph, X)
    lin = -(g @ delta + 0.5 * delta @ (H @ delta))
    return (error(graph, X) - error(graph, retract(X, delta))) / lin


_SOLVE_CASES = {}


def solve_case(kind, n, L=0):
    """one case of the single-solve tests, computed once and shared (read only): the graph, its start X, the direct
    solve's delta (n x 6), and pcg_band's iteration count at the tolerance the GPU test of that kind runs with"""
    key = (kind, n, L)
    if key not in _SOLVE_CASES:
        hg = {"chain": lambda: solve_chain(n), "loops": lambda: solve_loops(n, L)[0],
              "anisotropic": lambda: solve_anisotropic(n)}[kind]()
        X = np.array(hg.nodes)
        tol = 1e-13 if kind == "loops" else 1e-6
        _SOLVE_CASES[key] = dict(graph=hg, X=X, delta=single_solve(hg, X, SOLVE_LAMBDA).reshape(-1, 6), cg_tolerance=tol,
                                 pcg_iterations=pcg_band(hg, X, SOLVE_LAMBDA, tol, 1000)[1])
    return _SOLVE_CASES[key]


def step_errors(delta, reference):
    """(relative 2-norm over all entries, largest per-node error norm / largest per-node reference norm)"""
    d, r = np.asarray(delta).reshape(-1, 6), np.asarray(reference).reshape(-1, 6)
    return (np.linalg.norm(d - r) / np.linalg.norm(r),
            np.linalg.norm(d - r, axis=1).max() / np.linalg.norm(r, axis=1).max())


def reference_uncertainty(graph, X, lam):
    """how well the host knows delta: the larger of the relative difference between two column orderings of the direct
    solve and the relative error of the round trip Log(X^-1 (X Exp(delta)))"""
    d = single_solve(graph, X, lam)
    dn = single_solve(graph, X, lam, permc_spec="NATURAL")
    nd = np.linalg.norm(d)
    ordering = np.linalg.norm(d - dn) / nd
    trip = np.linalg.norm(step_of(X, retract(X, d)).ravel() - d) / nd
    return max(ordering, trip), ordering, trip


# The largest reference_uncertainty over every case of the single-solve tests, rounded up to one digit.  The GPU tests
# allow the device 1e3 times this (cyclic reduction is not backward stable the way sparse LU is).  Measured at
# SOLVE_LAMBDA with SOLVE_SEED (tests/test_posegraph_host.py asserts that no case exceeds the constant):
#
#   case                 ordering   round trip         case                 ordering   round trip
#   chain 1              0          3.7e-17            chain 63             5.2e-15    3.2e-14
#   chain 2              0          9.3e-16            chain 64             4.8e-15    3.2e-14
#   chain 3              0          3.0e-16            chain 65             2.1e-15    3.0e-14
#   chain 4              7.9e-16    3.3e-15            chain 127            2.9e-15    7.0e-14
#   chain 5              1.3e-15    2.2e-15            chain 128            1.4e-15    6.4e-14
#   chain 6              2.0e-15    6.1e-15            chain 129            4.3e-15    6.2e-14
#   chain 7              5.8e-16    4.3e-15            chain 255            1.2e-15    1.2e-13
#   chain 8              4.0e-15    3.5e-15            chain 256            1.9e-15    1.0e-13
#   chain 9              1.9e-15    5.2e-15            chain 257            1.3e-15    1.1e-13
#   chain 15             1.3e-14    7.1e-15            chain 511            1.1e-15    2.7e-13
#   chain 16             3.2e-15    7.3e-15            chain 512            1.7e-15    3.0e-13
#   chain 17             6.7e-15    7.2e-15            chain 513            9.3e-16    3.1e-13
#   chain 31             5.9e-15    1.1e-14            chain 1023           9.8e-16    7.6e-13
#   chain 32             6.7e-15    1.2e-14            chain 1024           1.2e-15    7.6e-13
#   chain 33             2.4e-15    1.6e-14            chain 1025           1.4e-15    7.7e-13
#   loops (64, 2)        3.7e-13    4.7e-14            chain 1537           5.7e-16    2.0e-12
#   loops (257, 3)       3.7e-14    1.0e-13            anisotropic 33       7.5e-11    1.7e-14
#   loops (513, 5)       1.1e-13    6.4e-13            anisotropic 513      9.1e-11    2.9e-13
#   loops (1025, 20)     4.9e-13    1.3e-12
#
# The round trip grows with n because X^-1 (X Exp(delta)) subtracts translations of the order of n metres.  The
# anisotropic chains set the constant: their damped system has condition number 5e6, and two orderings of the same
# LU differ by about that times the rounding unit.
SOLVE_REFERENCE_UNCERTAINTY = 1e-10
