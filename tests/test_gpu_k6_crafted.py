"""K6 (k_icp.hip) on the crafted frames of tests/test_k6_crafted_host.py: every room scene and every single-pixel row
bit for bit against the oracle AND, for the room scenes, directly against the fp64 evaluation of tests/k6_ref.py; the
Gauss-Newton chain and the batched chains on the 48 x 12 room against the oracle (bits) and against fp64 (the project's
bar of 1e-4 m / 1e-5 rad per iteration, and the known true pose).  The host file proves on the CPU that the oracle meets
the same bounds and that every row's words are the hand-computed ones."""
import numpy as np
import pytest

import k6_ref as K
import test_k6_crafted_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


def hip_objective(hip, p, data, model):
    """(context, frames, Frame2Model) with the frame pair uploaded"""
    ctx = hip.Context(p)
    hd = hip.Frame(ctx, p.data_width, p.data_height)
    hm = hip.Frame(ctx, p.model_width, p.model_height)
    hd.set(*data)
    hm.set(*model)
    obj = hip.Frame2Model(ctx)
    obj.setData(hd, hm)
    return ctx, (hd, hm), obj


def evaluate(obj, T, iteration):
    obj.initialize(T)
    obj._iteration = iteration
    F, JtJ, Jtr = obj.jacobianProducts()
    return F, JtJ, Jtr, obj.acc.copy(), (obj.valid(), obj.outlier(), obj.inlier(), obj.invalid())


def assert_equals_oracle(got, want, P, what, words=range(32)):
    """got: evaluate(); want: Oracle.jacobian_products().  The int64 words, F / JtJ / Jtr and the four counters."""
    F, JtJ, Jtr, acc, counts = got
    Fo, acco, JtJo, Jtro, st = want
    words = list(words)
    np.testing.assert_array_equal(acc[words], acco[words], err_msg=f"{what}: fixed-point words {words}")
    assert counts == (st.valid, st.outlier, st.inlier, st.invalid), what
    assert counts[0] + counts[3] == P, what
    if len(words) == 32:
        assert F == Fo and np.array_equal(JtJ, JtJo) and np.array_equal(Jtr, Jtro), what
    else:  # a row with an unspecified word: JtJ and Jtr do not depend on it, F does
        assert np.array_equal(JtJ, JtJo) and np.array_equal(Jtr, Jtro), what


@pytest.mark.parametrize("scene_id", H.SCENE_IDS)
def test_room_scene(hip, oracle_lib, scene_id):
    scene = H.SCENES[H.SCENE_IDS.index(scene_id)]
    p, data, model = H.room_scene(scene_id)
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    _, _, obj = hip_objective(hip, p, data, model)
    P = scene["size"][0] * scene["size"][1]
    for it in scene["its"]:
        got = evaluate(obj, np.eye(4), it)
        H.assert_within_fp64(H.room_reference(scene_id, it), got[0], got[1], got[2], (got[4][0], got[4][1], got[4][3]),
                             f"kernel {scene_id} iteration {it}")
        assert_equals_oracle(got, ora.jacobian_products(fd, fm, np.eye(4), it), P, f"{scene_id} iteration {it}")
    # away from the identity as well (the true pose: other texels, other gates), against the oracle
    got = evaluate(obj, H.TRUE_POSE, scene["its"][-1])
    assert_equals_oracle(got, ora.jacobian_products(fd, fm, H.TRUE_POSE, scene["its"][-1]), P, f"{scene_id} at the true pose")


@pytest.mark.parametrize("row_id", H.ROW_IDS)
def test_single_pixel_row(hip, oracle_lib, row_id):
    row = H.row_by_id(row_id)
    p = H.row_params(row)
    data, model = H.row_frames(row)
    _, _, obj = hip_objective(hip, p, data, model)
    got = evaluate(obj, row["pose"], row["iteration"])
    words = [k for k in range(32) if k not in row.get("unspecified", ())]
    assert_equals_oracle(got, H.oracle_row(oracle_lib, row), H.W13 * H.H5, row_id, words)
    assert (got[4][0], got[4][1], got[4][3]) == H.row_counts(row)
    if row["pairs"] is not None:  # the hand-computed words themselves, so that a failure names them
        want = H.expected_acc(row)
        assert [int(got[3][k]) for k in words] == [want[k] for k in words], row_id
    if "same_as" in row:
        other = H.row_by_id(row["same_as"])
        _, _, obj2 = hip_objective(hip, H.row_params(other), *H.row_frames(other))
        acc2 = evaluate(obj2, other["pose"], other["iteration"])[3]
        same = list(row["same_words"])
        np.testing.assert_array_equal(got[3][same], acc2[same], err_msg=f"{row_id} against {row['same_as']}")


def test_repeat_calls_carry_nothing_over(hip, oracle_lib):
    """twice on one context, then another scene on another context, then the first again; and a model of another size
    in one context: the rotating accumulator sets and the bias removal (one magic number per lane-trip: 128 for 65
    pixels, 576 for 576) must start clean every time"""
    small_id, big_id = "room13x5-bil-tukey", "room48x12-bil-huber"
    runs = {}
    for sid in (small_id, big_id):
        p, data, model = H.room_scene(sid)
        ora = oracle_lib.Oracle(p)
        fd, fm = H.oracle_frames(ora, data, model)
        ctx, frames, obj = hip_objective(hip, p, data, model)
        runs[sid] = (obj, ora.jacobian_products(fd, fm, np.eye(4), 1), p.data_width * p.data_height, ctx, frames, ora, fd)
    for sid in (small_id, small_id, big_id, small_id, big_id, big_id, small_id):
        obj, want, P = runs[sid][:3]
        assert_equals_oracle(evaluate(obj, np.eye(4), 1), want, P, f"{sid} in the sequence")
    # setData with a model of another size in the 48 x 12 context: 31 x 9, then back
    obj, _, P, ctx, (hd, hm), ora, fd = runs[big_id]
    p = H.room_scene(big_id)[0]
    Vm, Nm = K.room_frames(31, 9, p, np.eye(4))
    other = hip.Frame(ctx, 31, 9)
    other.set(Vm, Nm, np.zeros_like(Vm))
    fo = oracle_lib.OracleFrame(ora.L, 31, 9)
    fo.set(Vm, Nm, np.zeros_like(Vm))
    obj.setData(hd, other)
    assert_equals_oracle(evaluate(obj, np.eye(4), 0), ora.jacobian_products(fd, fo, np.eye(4), 0), P, "31 x 9 model")
    obj.setData(hd, hm)
    assert_equals_oracle(evaluate(obj, np.eye(4), 1), runs[big_id][1], P, "48 x 12 model again")


@pytest.mark.parametrize("max_iterations", H.CHAIN_ITERATIONS)
@pytest.mark.parametrize("bilinear,weight", H.CHAINS)
def test_chain_on_the_room(hip, oracle_lib, bilinear, weight, max_iterations):
    p = H.chain_params(bilinear, weight, max_iterations)
    _, data, model = H.room_scene("room48x12-bil-huber")
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    ctx, _, obj = hip_objective(hip, p, data, model)
    gn = hip.LieGaussNewton(ctx)
    gn.minimize(obj, np.eye(4))
    To, hist_o, st = ora.minimize(fd, fm, np.eye(4))
    hist = gn.history()
    assert hist.shape == hist_o.shape and np.array_equal(hist, hist_o), "history differs from the oracle in bits"
    assert np.array_equal(gn.pose(), To), "final pose differs from the oracle in bits"
    assert gn.iterationCount() == st.iterations and gn.stats.converged == st.converged
    H.assert_chain_against_fp64(hist, gn.pose(), gn.stats.converged, bilinear, weight,
                                f"kernel chain {bilinear}/{weight}/{max_iterations}")


def test_batched_chains_on_the_room(hip, oracle_lib):
    p = H.chain_params(1, H.HUBER, 10)
    _, data, model = H.room_scene("room48x12-bil-huber")
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    ctx, _, obj = hip_objective(hip, p, data, model)
    gn = hip.LieGaussNewton(ctx)
    starts = H.batch_starts()
    Ts, stats = gn.minimize_batch(starts, obj)
    for k, T0 in enumerate(starts):
        To, _, st = ora.minimize(fd, fm, T0)
        assert np.all(np.isfinite(To)) and st.valid - st.outlier >= 6, f"test setup: start {k}"
        assert np.array_equal(Ts[k], To), f"start {k}"
        assert stats[k]["iterations"] == st.iterations and stats[k]["converged"] == st.converged
        assert stats[k]["valid"] == st.valid and stats[k]["outlier"] == st.outlier and stats[k]["error"] == st.error
