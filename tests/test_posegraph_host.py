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


# ---- the single damped solve: the reference stays inside every cap that tests/test_gpu_posegraph_solve.py sets ---------
#
# The graphs come from ph.SOLVE_SEED.  The seed was picked so that the host alone meets the caps below: a GPU failure
# of the same assertions is then the device's doing.

SOLVE_CASES = ([("chain", n, 0) for n in ph.SOLVE_CHAIN_SIZES] + [("loops", n, L) for n, L in ph.SOLVE_LOOP_CASES]
               + [("anisotropic", n, 0) for n in ph.SOLVE_ANISOTROPIC_SIZES])


@pytest.mark.parametrize("kind,n,L", SOLVE_CASES)
def test_single_solve_reference_is_known_to_the_recorded_uncertainty(kind, n, L):
    c = ph.solve_case(kind, n, L)
    hg, X = c["graph"], c["X"]
    assert len(X) == n and np.abs(c["delta"]).max() > 0
    s, ordering, trip = ph.reference_uncertainty(hg, X, ph.SOLVE_LAMBDA)
    print(f"{kind} {n} {L}: ordering {ordering:.1e} round trip {trip:.1e}")
    assert s <= ph.SOLVE_REFERENCE_UNCERTAINTY
    # Levenberg-Marquardt accepts this step, so optimize(1) is one damped solve at SOLVE_LAMBDA and its poses are
    # X Exp(delta)
    assert ph.model_fidelity(hg, X, c["delta"].ravel()) > 0.9
    # the PCG's answer is the direct solve's
    d, it = ph.pcg_band(hg, X, ph.SOLVE_LAMBDA, c["cg_tolerance"], 1000)
    assert it == c["pcg_iterations"]
    assert max(ph.step_errors(d, c["delta"])) <= 1e3 * ph.SOLVE_REFERENCE_UNCERTAINTY


@pytest.mark.parametrize("kind,n", [("chain", n) for n in ph.SOLVE_CHAIN_SIZES]
                         + [("anisotropic", n) for n in ph.SOLVE_ANISOTROPIC_SIZES])
def test_band_preconditioner_solves_a_chain_in_one_iteration(kind, n):
    """on a chain the block-tridiagonal part is the whole system, ill-conditioned blocks or not"""
    assert ph.solve_case(kind, n)["pcg_iterations"] == 1


@pytest.mark.parametrize("n,L", ph.SOLVE_LOOP_CASES)
def test_loop_graphs_have_the_asked_structure_and_end_within_rank_plus_one(n, L):
    hg, pairs = ph.solve_loops(n, L)
    assert len(set(pairs)) == L and all(0 <= a < b - 1 < n - 1 for a, b in pairs)
    assert (0, n - 1) in pairs
    loop_edges = [(a, b) for a, b, _, _ in hg.edges if abs(a - b) > 1]
    assert {(min(a, b), max(a, b)) for a, b in loop_edges} == set(pairs)
    # one pair is entered twice, in opposite directions
    assert len(loop_edges) == L + 1
    assert sum((b, a) in loop_edges for a, b in loop_edges) == 2
    # one node takes part in three off-band pairs; two distinct pairs can give a node only two
    count = np.bincount(np.array(pairs).ravel(), minlength=n)
    assert count.max() >= min(L, 3)
    # M^-1 A = I + M^-1 E with E of rank <= 12 per off-band pair: exact CG ends within rank + 1 steps
    it = ph.solve_case("loops", n, L)["pcg_iterations"]
    print(f"loops ({n}, {L}): {it} iterations, cap {12 * L + 1}")
    assert 1 < it <= 12 * L + 1


def test_anisotropic_blocks_are_ill_conditioned_and_full():
    for n in ph.SOLVE_ANISOTROPIC_SIZES:
        hg = ph.solve_case("anisotropic", n)["graph"]
        assert len(hg.edges) == n - 1
        for _, _, _, O in hg.edges:
            w = np.linalg.eigvalsh(O)
            assert abs(w[-1] / w[0] - 1e9) < 1e9 * 1e-6
            assert np.abs(O - np.diag(np.diag(O))).max() > 1e3


@pytest.mark.parametrize("n,node", [(16, 7), (257, 0), (1025, 511)])
def test_iteration_count_tells_an_inexact_preconditioner(n, node):
    """without the band block (node, node + 1) the preconditioner is still positive-definite and CG still reaches the
    same delta, but not in one iteration: the count discriminates"""
    c = ph.solve_case("chain", n)
    d, it = ph.pcg_band(c["graph"], c["X"], ph.SOLVE_LAMBDA, 1e-6, 1000, drop_band=node)
    assert it > 1
    assert ph.step_errors(d, c["delta"])[0] < 1e-3  # it converges (the rule stops at 1e-6 in the M^-1 norm)


def test_default_parameters_stop_on_the_relative_decrease():
    rng = np.random.default_rng(8)
    _, g = ph.chain_graph(40, 6, rng)
    X, st = ph.levenberg_marquardt(g, max_iterations=100)
    assert st["termination"] == ph.CONVERGED
    assert 1 <= st["iterations"] < 100
    assert st["final_error"] < st["initial_error"]
