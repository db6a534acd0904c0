"""GPU checks of the pose graph's linear solver (k_pg_solve in k_posegraph.hip: preconditioned CG in one workgroup, the
preconditioner a block cyclic reduction of the block-tridiagonal part) observed directly, one damped solve at a time.

optimize(1) with lambda_initial = ph.SOLVE_LAMBDA and both error tolerances 0 runs its first damped solve at exactly
that lambda; linear_solves == 1 says the step was accepted, so poses() = X0 Exp(delta), delta = Log(X0^-1 X1) per node
is the solver's output and last_stats.cg_iterations is that one solve's count.  The yardstick is the sparse direct
solve of tests/posegraph_host.py.  tests/test_posegraph_host.py shows on the CPU that the host's own PCG meets every
iteration cap below and that the direct solve is known to ph.SOLVE_REFERENCE_UNCERTAINTY; the device gets 1e3 times
that, because cyclic reduction is not backward stable the way sparse LU is.  The figures measured on MI355X are in
each test's docstring; every test prints its own."""
import numpy as np
import pytest

import posegraph_host as ph

pytestmark = pytest.mark.gpu

T = 1e3 * ph.SOLVE_REFERENCE_UNCERTAINTY


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()
    return core


def _device_step(core, case, cg_max_iterations=1000):
    """(delta n x 6, stats) of one damped solve of the case on the device"""
    hg = case["graph"]
    g = core.Posegraph(0, node_capacity=len(hg.nodes), edge_capacity=max(len(hg.edges), 1))
    for i, X in enumerate(hg.nodes):
        g.setInitial(i, X)
    for a, b, Z, O in hg.edges:
        g.addEdge(a, b, Z, O)
    g.optimize(1, core.PosegraphParams.defaults(lambda_initial=ph.SOLVE_LAMBDA, relative_error_tol=0.0,
                                                absolute_error_tol=0.0, cg_tolerance=case["cg_tolerance"],
                                                cg_max_iterations=cg_max_iterations))
    st = g.last_stats
    assert st.linear_solves == 1 and st.iterations == 1, st.as_dict()
    assert st.final_error < st.initial_error, st.as_dict()  # accepted: the poses are X0 Exp(delta)
    X1 = g.poses()
    g.close()
    assert np.isfinite(X1).all()
    return ph.step_of(case["X"], X1), st


def _check_step(name, delta, st, case, cap):
    rel, node = ph.step_errors(delta, case["delta"])
    print(f"{name}: delta error {rel:.2e} (worst node {node:.2e}) against T = {T:.1e}; cg_iterations "
          f"{st.cg_iterations} against {cap} (host {case['pcg_iterations']})")
    assert st.cg_iterations <= cap, (st.as_dict(), cap)
    assert rel <= T, (rel, T)
    assert node <= T, (node, T)  # one wrong node cannot hide in a long vector


@pytest.mark.parametrize("n", ph.SOLVE_CHAIN_SIZES)
def test_chain_solve_is_exact_at_every_size(hip, n):
    """On a chain the cyclic reduction is the whole solve: at most one CG iteration, and delta equals the direct solve.
    The sizes sit on the edges of the reduction's level count and of its neighbour tests (2^k - 1, 2^k, 2^k + 1) and
    past the second and third trip of its stride loops (n > 512 at stride 1, n > 1024 at stride 2; 1537).

    Measured on MI355X: one iteration at every size; the error of delta grows with n from 3e-16 (n = 1) over 1.4e-13
    (255) and 7.7e-13 (1025) to its largest, 2.05e-12 over all entries and 5.08e-12 at the worst node, at n = 1537.  At
    every size that is the error of the round trip Log(X0^-1 X1) itself (ph.SOLVE_REFERENCE_UNCERTAINTY's table)."""
    case = ph.solve_case("chain", n)
    delta, st = _device_step(hip, case)
    _check_step(f"chain {n}", delta, st, case, 1)


@pytest.mark.parametrize("n,L", ph.SOLVE_LOOP_CASES)
def test_off_band_pairs_end_within_rank_plus_one(hip, n, L):
    """L distinct off-band pairs through pg_spmv: pair (0, n-1), a pair entered twice in opposite directions, node
    n-1 in min(L, 3) pairs.  The preconditioned matrix is I + (rank <= 12 L), so CG ends within 12 L + 1 iterations,
    and within 2 of what the host's PCG with an exact band factorisation takes.

    Measured on MI355X, (n, L): iterations (the host's; 12 L + 1), error of delta:  (64, 2): 13 (13; 25), 7.0e-14;
    (257, 3): 13 (13; 37), 1.1e-13;  (513, 5): 37 (37; 61), 6.5e-13;  (1025, 20): 146 (146; 241), 2.8e-12."""
    case = ph.solve_case("loops", n, L)
    delta, st = _device_step(hip, case)
    _check_step(f"loops ({n}, {L})", delta, st, case, min(12 * L + 1, case["pcg_iterations"] + 2))


@pytest.mark.parametrize("n", ph.SOLVE_ANISOTROPIC_SIZES)
def test_ill_conditioned_blocks(hip, n):
    """edge information of condition number 1e9, not diagonal: the reduced blocks of the cyclic reduction are then far
    from the benign diag(1e3, 1e3, 1e3, 1e2, 1e2, 1e2) of every other test.

    Measured on MI355X: one iteration; error of delta 2.0e-10 at n = 33 and 2.9e-10 at n = 513 (worst node 6.5e-10),
    the level of the system's conditioning (5e6 times the rounding unit).  With explicit inverses of the reduced blocks
    in place of their Cholesky factors, as the cyclic reduction first had them, this test measured 3.3e-7 and 5.0e-7
    (worst node 2.2e-6) and failed."""
    case = ph.solve_case("anisotropic", n)
    delta, st = _device_step(hip, case)
    _check_step(f"anisotropic {n}", delta, st, case, case["pcg_iterations"] + 2)
