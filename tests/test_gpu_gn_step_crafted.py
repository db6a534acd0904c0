"""The Gauss-Newton step of k_icp_step / k_icp_finish (solve6_wave, se3_exp, the stopping rules, the done / pending
carry-over, the history, batched hypotheses) on the crafted systems of tests/test_gn_step_crafted_host.py: words,
history, final pose, converged, iteration count and statistics bit for bit against the oracle, AND the kernel's own
step against the exact reference of tests/gn_step_ref.py within the same bound the host file proves for the oracle.
Singular systems give the zero twist (documented deviations): alone, inside a batch next to healthy
hypotheses, between healthy chains on one context, and in the scan pipeline across an empty scan."""
import numpy as np
import pytest

import test_gn_step_crafted_host as S
import test_k6_crafted_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


def hip_objective(hip, p, data, model):
    ctx = hip.Context(p)
    hd = hip.Frame(ctx, p.data_width, p.data_height)
    hm = hip.Frame(ctx, p.model_width, p.model_height)
    hd.set(*data)
    hm.set(*model)
    obj = hip.Frame2Model(ctx)
    obj.setData(hd, hm)
    return ctx, (hd, hm), obj


def stats_tuple(st):
    return (st.error, st.inlier_residual, st.valid, st.outlier, st.inlier, st.invalid, st.iterations, st.converged)


def hip_chain(hip, p, data, model, T0, iteration0=0):
    """(final pose, history, stats, information) of one minimisation on a fresh context"""
    ctx, frames, obj = hip_objective(hip, p, data, model)
    obj._iteration = iteration0
    gn = hip.LieGaussNewton(ctx)
    gn.minimize(obj, T0)
    return gn.pose(), gn.history(), gn.stats, gn.information()


def assert_chain_equals_oracle(got, want, what):
    (T, hist, st, _), (To, hist_o, sto) = got, want
    assert hist.shape == hist_o.shape and hist.tobytes() == hist_o.tobytes(), f"{what}: history differs from the oracle in bits"
    assert T.tobytes() == To.tobytes(), f"{what}: final pose differs from the oracle in bits"
    assert stats_tuple(st) == stats_tuple(sto), f"{what}: {stats_tuple(st)} != {stats_tuple(sto)}"


@pytest.mark.parametrize("sid", S.A_IDS + S.B_IDS)
def test_one_step(hip, oracle_lib, sid):
    p, data, model, T0, ref = S.system(sid)
    (Fo, acco, JtJo, Jtro, sto), want = S.oracle_step(oracle_lib, sid)
    ctx, frames, obj = hip_objective(hip, p, data, model)
    obj.initialize(T0)
    F, JtJ, Jtr = obj.jacobianProducts()
    np.testing.assert_array_equal(obj.acc, acco, err_msg=f"{sid}: fixed-point words")
    assert F == Fo and np.array_equal(JtJ, JtJo) and np.array_equal(Jtr, Jtro)
    gn = hip.LieGaussNewton(ctx)
    gn.minimize(obj, T0)
    got = (gn.pose(), gn.history(), gn.stats, gn.information())
    assert_chain_equals_oracle(got, want, sid)
    assert got[1].shape[0] == 2 and got[2].iterations == 1 and got[2].converged == 0
    assert np.array_equal(got[3], JtJo), "information() is the JtJ of the step"
    S.assert_step(sid, obj.acc, got[0], "kernel")


@pytest.mark.parametrize("cid", S.RULE_IDS)
def test_stopping_rule(hip, oracle_lib, cid):
    c = S.rule_cases()[cid]
    ora = oracle_lib.Oracle(c["p"])
    fd, fm = H.oracle_frames(ora, c["data"], c["model"])
    got = hip_chain(hip, c["p"], c["data"], c["model"], c["T0"])
    assert_chain_equals_oracle(got, ora.minimize(fd, fm, c["T0"]), cid)
    S.assert_rule_case(cid, got[0], got[1], got[2].converged, got[2].iterations, "kernel")


@pytest.mark.parametrize("mode", list(S.MODES))
@pytest.mark.parametrize("cid", S.SINGULAR_IDS)
def test_singular(hip, oracle_lib, cid, mode):
    p, data, model, T0, it0 = S.singular_case(cid, mode)
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    got = hip_chain(hip, p, data, model, T0, it0)
    assert_chain_equals_oracle(got, ora.minimize(fd, fm, T0, iteration0=it0), f"{cid}-{mode}")
    _, _, JtJo, Jtro, _ = ora.jacobian_products(fd, fm, T0, it0 + got[2].iterations - (0 if got[2].converged else 1))
    assert np.array_equal(got[3], JtJo), "information() of the last step"
    S.assert_singular(cid, mode, got[0], got[1], got[2], (got[3],), "kernel")


@pytest.mark.parametrize("cid", S.NOISE_IDS)
def test_noise_level_systems(hip, oracle_lib, cid):
    data, model = S.noise_cases()[cid]
    p = S.room_params(S.HUBER, max_iterations=3)
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    got = hip_chain(hip, p, data, model, np.eye(4))
    assert_chain_equals_oracle(got, ora.minimize(fd, fm, np.eye(4)), cid)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))


@pytest.mark.parametrize("cid", S.ROUNDING_PIVOT_IDS)
def test_rounding_level_pivot(hip, oracle_lib, cid):
    """a pivot of -1e-7 / +1e-7 beside pivots of 1 .. 100, finite solution either way: the kernel's own pivot test"""
    p, data, model = S.rounding_pivot_cases()[cid]
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    ctx, frames, obj = hip_objective(hip, p, data, model)
    obj.initialize(np.eye(4))
    _, JtJ, Jtr = obj.jacobianProducts()
    gn = hip.LieGaussNewton(ctx)
    gn.minimize(obj, np.eye(4))
    got = (gn.pose(), gn.history(), gn.stats, None)
    assert_chain_equals_oracle(got, ora.minimize(fd, fm, np.eye(4)), cid)
    S.assert_rounding_pivot(cid, JtJ, Jtr, got[0], got[1], got[2], "kernel")


@pytest.mark.parametrize("position", (0, 1, 2))
def test_batch_isolation(hip, oracle_lib, position):
    """a far (singular) hypothesis in a batch next to two healthy ones: it converges at its first step through :64 and
    is only carried from then on, while the others keep iterating; nobody sees anybody else"""
    p = H.chain_params(1, H.HUBER, 10)
    data, model = S.room_frames()
    starts = [T.copy() for T in H.batch_starts()[:2]]
    starts.insert(position, S.FAR_START.copy())
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    ctx, _, obj = hip_objective(hip, p, data, model)
    gn = hip.LieGaussNewton(ctx)
    Ts, stats = gn.minimize_batch(starts, obj)
    for k, T0 in enumerate(starts):
        To, _, sto = ora.minimize(fd, fm, T0)
        single = hip_chain(hip, p, data, model, T0)
        assert Ts[k].tobytes() == single[0].tobytes() == To.tobytes(), f"hypothesis {k} (far one at {position})"
        for key, a, b in (("iterations", single[2].iterations, sto.iterations), ("converged", single[2].converged, sto.converged),
                          ("valid", single[2].valid, sto.valid), ("outlier", single[2].outlier, sto.outlier),
                          ("error", single[2].error, sto.error)):
            assert stats[k][key] == a == b, f"hypothesis {k}: {key}"
        if k == position:  # (its texels still project into the model image: valid pairs, every one an outlier)
            assert Ts[k].tobytes() == S.FAR_START.tobytes() and stats[k]["valid"] == stats[k]["outlier"]
            assert stats[k]["converged"] == 1 and stats[k]["iterations"] == 0
        else:
            assert stats[k]["iterations"] >= 1 and stats[k]["valid"] - stats[k]["outlier"] >= 6


def test_repeat_singular_healthy_singular(hip, oracle_lib):
    """one context: a singular chain, a healthy chain, a singular chain, a healthy chain -- each equals the oracle and
    its own first run in bits (the accumulator rotation and the partial-sum records start clean)"""
    p = S.room_params(S.HUBER, max_iterations=4)
    data, model = S.room_frames()
    empty = tuple(np.zeros_like(m) for m in data)
    ora = oracle_lib.Oracle(p)
    ctx, (hd, hm), obj = hip_objective(hip, p, data, model)
    gn = hip.LieGaussNewton(ctx)
    first = {}
    for name, d in (("singular", empty), ("healthy", data), ("singular", empty), ("healthy", data)):
        hd.set(*d)
        obj.setData(hd, hm)
        gn.minimize(obj, np.eye(4))
        got = (gn.pose().copy(), gn.history().copy(), gn.stats, None)
        fd, fm = H.oracle_frames(ora, d, model)
        assert_chain_equals_oracle(got, ora.minimize(fd, fm, np.eye(4)), name)
        if name in first:
            assert got[0].tobytes() == first[name][0].tobytes() and got[1].tobytes() == first[name][1].tobytes()
            assert stats_tuple(got[2]) == first[name][2]
        else:
            first[name] = (got[0], got[1], stats_tuple(got[2]))
    assert np.array_equal(first["singular"][0], np.eye(4)) and first["healthy"][2][6] == 4


@pytest.mark.parametrize("mode", list(S.PIPELINE_MODES))
def test_pipeline_across_an_empty_scan(hip, oracle_lib, mode):
    from semantic_suma_amd.types import params_with_size
    p = params_with_size(*S.PIPELINE_SIZE)
    fi = S.PIPELINE_MODES[mode]
    hp, op = hip.SurfelMapping(p), oracle_lib.OraclePipeline(p)
    poses, incs = [], []
    for k, (pts, lab, prob) in enumerate(S.pipeline_scans(True)):
        hp.processScan(pts, lab, prob, fixed_iterations=fi)
        op.process_scan(pts, lab, prob, fixed_iterations=fi)
        assert hp.getCurrentPose().tobytes() == op.pose().tobytes(), f"scan {k}: pose bits"
        assert hp.lastStats().as_dict() == op.last_stats().as_dict(), f"scan {k}: statistics"
        assert hp.map.getAllSurfels().tobytes() == op.ctx.map_surfels().tobytes(), f"scan {k}: surfel bytes"
        poses.append(hp.getCurrentPose().copy())
        incs.append(hp.lastIncrement().copy())
    ref = hip.SurfelMapping(p)
    for pts, lab, prob in S.pipeline_scans(False):
        ref.processScan(pts, lab, prob, fixed_iterations=fi)
    S.assert_pipeline_across_empty_scan(poses, incs, ref.getCurrentPose(), f"kernel pipeline {mode}")
