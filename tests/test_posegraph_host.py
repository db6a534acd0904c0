"""CPU checks of the pose-graph host restatement (tests/posegraph_host.py), the yardstick of the HIP optimiser:
its Jacobians against central differences, and two known answers."""
import math

import numpy as np
import pytest

import posegraph_host as ph


def _fd_jacobians(graph, X, f, h=1e-6):
    """central differences of factor f's error in the retraction's tangent at both of its nodes"""
    fr, to, _, _ = graph.factors()
    out = []
    for node in (fr[f], to[f]):
        if node < 0:
            out.append(np.zeros((6, 6)))
            continue
        J = np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Xp, Xm = X.copy(), X.copy()
            Xp[node] = ph.compose(X[node], ph.se3_exp(d))
            Xm[node] = ph.compose(X[node], ph.se3_exp(-d))
            J[:, k] = (ph.factor_terms(graph, Xp)[0][f] - ph.factor_terms(graph, Xm)[0][f]) / (2 * h)
        out.append(J)
    return out


@pytest.mark.parametrize("angle", [None, 1e-7, 1e-3, 0.3, 0.49, 0.51, 2.0, math.pi - 1e-3, math.pi - 0.3])
def test_jacobians_match_central_differences(angle):
    rng = np.random.default_rng(17 if angle is None else int(1e3 * angle) + 3)
    X = np.array([ph.random_pose(rng, scale=2.0) for _ in range(3)])
    edges = []
    for a, b in [(0, 1), (2, 1), (1, 2)]:
        E = ph.random_pose(rng, angle=angle, scale=0.7)  # the error rotation of the factor has this angle
        Z = ph.compose(ph.inv(E), ph.compose(ph.inv(X[a]), X[b]))
        edges.append((a, b, Z, ph.info_matrix(rng)))
    g = ph.HostGraph(X, edges)
    e, Ji, Jj, _ = ph.factor_terms(g, X)
    for f in range(1, 4):
        if angle is not None:
            assert abs(np.linalg.norm(e[f, :3]) - angle) < 1e-9
        Fi, Fj = _fd_jacobians(g, X, f)
        for J, F in ((Ji[f], Fi), (Jj[f], Fj)):
            assert np.linalg.norm(J - F) <= 1e-7 * np.linalg.norm(F), (f, np.abs(J - F).max())


def test_exp_log_round_trip_and_series_seam():
    rng = np.random.default_rng(5)
    for th in [0.0, 1e-9, 1e-4, 0.4999999, 0.5, 0.5000001, 1.5, 3.0, math.pi - 1e-6]:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        xi = np.concatenate([th * ax, rng.normal(size=3)])
        T = ph.se3_exp(xi)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)
        assert np.allclose(ph.se3_log(T), xi, rtol=0, atol=1e-12 if th < 3 else 1e-9)
    # the coefficients are continuous across the series / closed-form seam
    lo, hi = ph.coefficients(np.array([np.nextafter(0.5, 0.0)])), ph.coefficients(np.array([0.5]))
    for a, b in zip(lo, hi):
        assert abs(a[0] - b[0]) <= 1e-13 * abs(b[0])


def test_exact_measurements_give_zero_error_and_ground_truth():
    rng = np.random.default_rng(11)
    gt, g0 = ph.chain_graph(60, 8, rng, noise=(0.0, 0.0))
    g = ph.HostGraph(gt, g0.edges)
    assert ph.error(g, gt) < 1e-20
    X, st = ph.levenberg_marquardt(g, max_iterations=20)
    assert st["final_error"] < 1e-20
    assert np.abs(X - gt).max() < 1e-12


def _gauss_newton_dense(graph, X, iters=30):
    for _ in range(iters):
        g, H, _, _ = ph.linearize(graph, X)
        d = np.linalg.solve(H.toarray(), -g)
        X = ph.retract(X, d)
        if np.abs(d).max() < 1e-15:
            break
    return X


def test_lm_reaches_the_dense_gauss_newton_optimum():
    rng = np.random.default_rng(3)
    gt, g = ph.chain_graph(50, 10, rng, loop_min_gap=5)
    X0 = np.array(g.nodes)
    e0 = ph.error(g, X0)
    X, st = ph.levenberg_marquardt(g, max_iterations=100, relative_error_tol=0.0, absolute_error_tol=0.0)
    assert st["final_error"] < e0
    Xgn = _gauss_newton_dense(g, X0)
    assert np.abs(X[:, :3, :] - Xgn[:, :3, :]).max() < 1e-10
    assert abs(st["final_error"] - ph.error(g, Xgn)) <= 1e-10 * ph.error(g, Xgn)
    # at the optimum the gradient vanishes
    grad = ph.linearize(g, X)[0]
    assert np.abs(grad).max() < 1e-6


def test_default_parameters_stop_on_the_relative_decrease():
    rng = np.random.default_rng(8)
    _, g = ph.chain_graph(40, 6, rng)
    X, st = ph.levenberg_marquardt(g, max_iterations=100)
    assert st["termination"] == ph.CONVERGED
    assert 1 <= st["iterations"] < 100
    assert st["final_error"] < st["initial_error"]
