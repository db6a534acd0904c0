"""GPU checks of loop closing inside the scan pipeline (suma_pipeline_enable_loop_closing, suma_loop.hip, k_loop.hip)
against the plain-Python restatement tests/loop_closing_host.py.

Scenario (loop_closing_host.SCENARIO): tests/loop_scenario.py's circle at 0.7 m per scan (a lap of 153 scans), 140 scans,
900 x 64, 8 fixed iterations, min_trajectory_distance 60, search_distance 30, delta_timestamp 100,
min_valid_ratio = loop_scenario.MIN_VALID_RATIO, everything else default.  Why 30 m and 140 scans, and what the CPU run
of the restatement gives on it, is written down in tests/test_loop_closing_host.py.

The native run and the restatement call the same library and the same deterministic optimiser
(test_gpu_posegraph.test_clones_optimise_to_identical_bits), so every comparison between them is exact."""
import numpy as np
import pytest

import loop_closing_host as lh
import loop_scenario as ls

pytestmark = pytest.mark.gpu

W, H = 900, 64


@pytest.fixture(scope="module")
def core():
    from semantic_suma_amd import core
    core.lib()
    return core


def loop_params(**over):
    from semantic_suma_amd.types import LoopParams
    return LoopParams.defaults(**dict(lh.SCENARIO, min_valid_ratio=ls.MIN_VALID_RATIO, **over))


def native_run(core, n, W=W, H=H, phases=False, on_scan=None, params=None, **over):
    from semantic_suma_amd.types import params_with_size
    sm = core.SurfelMapping(params_with_size(W, H) if params is None else params, loop_params=loop_params(**over))
    log = []
    for k in range(n):
        pts, lab, prob = lh.scenario_scan(k, W, H)
        if phases:
            sm.beginScan(pts, lab, prob)
            sm.updatePose(8)
            sm.checkLoopClosure()
            sm.updateMap()
        else:
            sm.processScan(pts, lab, prob, fixed_iterations=8)
        log.append(sm.loopStatus().as_dict())
        if on_scan is not None:
            on_scan(k, sm)
    return sm, log


def scripted_run(core, n, on_scan=None, **over):
    from semantic_suma_amd.types import params_with_size
    sm = core.SurfelMapping(params_with_size(W, H))
    lc = lh.LoopClosing(ls.HipPipe(sm), core.Posegraph(0, node_capacity=1024, edge_capacity=2048), **dict(lh.SCENARIO, **over))
    log = lh.run_scenario(lc, W, H, n, on_scan)
    return sm, lc, log


def final_state(sm):
    return dict(pose=sm.getCurrentPose().tobytes(), pose_old=sm.getPose(1).tobytes(), table=sm.map.poses().tobytes(),
                surfels=sm.map.getAllSurfels().tobytes())


def assert_logs_equal(a, b, upto=None, skip=()):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        if upto is not None and k > upto:
            break
        bad = lh.status_equal(x, y, skip)
        assert not bad, (k, bad, x, y)


def edge_list(graph):
    """(from, to, the bits of the measurement's top 3 x 4: what a pose graph keeps of it)"""
    return [(a, b, Z[:3].tobytes()) for a, b, Z, _ in graph.edges()]


def script_edges(lc):
    return [(a, b, Z[:3].tobytes()) for a, b, Z in lc.edges]


_RUNS = {}


def shared(core, name):
    """the two full runs, made once"""
    if name not in _RUNS:
        n = lh.scenario_length()
        if name == "native":
            at_first = {}

            def snap(k, sm):  # the graph as it stands after the scan that starts the first optimisation
                if not at_first and sm.loopStatus().started_optimization:
                    at_first.update(scan=k, poses=sm.posegraph.poses(), edges=edge_list(sm.posegraph),
                                    trajectory_distances=sm.trajectoryDistances().copy(), pose=sm.getCurrentPose(),
                                    pose_old=sm.getPose(1))

            sm, log = native_run(core, n, on_scan=snap)
            _RUNS[name] = dict(sm=sm, log=log, at_first=at_first)
        else:
            sm, lc, log = scripted_run(core, n)
            _RUNS[name] = dict(sm=sm, lc=lc, log=log)
    return _RUNS[name]


def test_native_equals_the_scripted_restatement(core):
    nat, scr = shared(core, "native"), shared(core, "scripted")
    log = nat["log"]
    summary = dict(failed=sum(1 for s in log if s["found_candidate"] and s["candidate_to"] < 0),
                   candidates=sum(1 for s in log if s["candidate_to"] >= 0), edges=sum(s["edges_added"] for s in log),
                   started=[k for k, s in enumerate(log) if s["started_optimization"]],
                   integrated=[k for k, s in enumerate(log) if s["integrated"]])
    print(summary)
    # the scenario does what it is there for, on the device too
    assert summary["failed"] >= 1 and summary["edges"] >= 4 and summary["started"] and summary["integrated"]
    assert summary["integrated"][0] < len(log) - 1
    assert_logs_equal(log, scr["log"])
    g = nat["sm"].posegraph
    assert edge_list(g) == script_edges(scr["lc"])
    assert g.poses().tobytes() == scr["lc"].graph.poses().tobytes()
    assert nat["sm"].trajectoryDistances().tobytes() == np.array(scr["lc"].trajectory_distances, np.float32).tobytes()
    assert final_state(nat["sm"]) == final_state(scr["sm"])
    assert nat["sm"].getOptimizedPoses().shape == (len(log), 4, 4)


def test_native_equals_the_oracle_until_the_first_optimisation(core):
    """The restatement over the CPU oracle and the fp64 host graph against the native run, up to and including the scan
    that starts the first optimisation: the status log, the edge list (measurements by their bits), the graph's poses,
    the trajectory distances and the pipeline's poses, bit for bit.  After that scan the two optimisers differ in the
    last bits, so nothing is asserted.

    One field is not compared by its bits: posegraph_error.  It is a sum of per-factor energies that the host graph
    (numpy) and the device (k_pg_factor, k_pg_energy) evaluate with different operation orders, so it is held to the
    bound tests/test_gpu_posegraph.py sets for that pair, 1e-12 relative, plus a floor for graphs whose error is
    rounding noise itself.  Until the first loop edge the graph is the odometry chain with pose(t) = pose(t-1) *
    increment, whose exact error is 0; what either side computes there is the rounding of a residual, at most
    d = 16 eps |t|max per component (a few dozen fp64 operations on translations up to |t|max = 35 m, the circle's
    diameter), so each of the m factors holds at most 3 d^2 of energy (identity information, six components, the
    half)."""
    from oracle import pyoracle
    from semantic_suma_amd.types import params_with_size
    nat = shared(core, "native")
    at = nat["at_first"]
    first = at["scan"]
    assert first == next(k for k, s in enumerate(nat["log"]) if s["started_optimization"])
    op = pyoracle.OraclePipeline(params_with_size(W, H), threads=16)
    lc = lh.LoopClosing(ls.OraclePipe(op), lh.HostGraph(), **lh.SCENARIO)
    log = lh.run_scenario(lc, W, H, first + 1)
    d = 16 * np.finfo(np.float64).eps * 35.0
    worst = 0.0
    for k in range(first + 1):
        a, b = nat["log"][k]["posegraph_error"], log[k]["posegraph_error"]
        floor = 3 * d * d * (k + 1 + sum(s["edges_added"] for s in log[:k + 1]))
        worst = max(worst, abs(a - b) / max(abs(b), 1e-300) if abs(a - b) > floor else 0.0)
        print(f"scan {k}: posegraph_error native {a!r} oracle {b!r} floor {floor:.3e}")
        assert abs(a - b) <= 1e-12 * abs(b) + floor, (k, a, b)
    print("worst relative difference above the floor", worst)
    assert_logs_equal(nat["log"][:first + 1], log, skip=("posegraph_error",))
    assert at["edges"] == script_edges(lc)
    assert at["poses"].shape == (first + 1, 4, 4)
    assert at["poses"].tobytes() == lc.graph.poses().tobytes()
    assert at["trajectory_distances"].tobytes() == np.array(lc.trajectory_distances, np.float32).tobytes()
    assert at["pose"].tobytes() == lc.pipe.pose(0).tobytes()
    assert at["pose_old"].tobytes() == lc.pipe.pose(1).tobytes()


@pytest.mark.parametrize("lag", [1, 5])
def test_tail_rows_of_a_late_integration(core, lag):
    """integrate_lag > 0: the graph has gained nodes while the optimiser ran.  The map's pose table after the integrating
    scan's start is float32 of the restatement's table (optimised rows, then difference * before rows), byte for byte;
    the trajectory distances and loopCount_ agree from there on."""
    first = next(k for k, s in enumerate(shared(core, "native")["log"]) if s["started_optimization"])
    n = min(first + lag + 6, lh.scenario_length())
    tables = {}

    def grab(k, sm):
        if sm.loopStatus().integrated:
            tables[k] = (sm.map.poses(), sm.trajectoryDistances().copy(), sm.loopStatus().loop_count)

    nat_sm, nat_log = native_run(core, n, on_scan=grab, integrate_lag=lag)
    _, lc, log = scripted_run(core, n, integrate_lag=lag)
    k_int = first + 1 + lag
    assert [k for k, s in enumerate(nat_log) if s["integrated"]][0] == k_int
    assert lc.table_at_integration[0][0] == k_int
    want = lc.table_at_integration[0][1]
    assert want.shape[0] == k_int and want.dtype == np.float32
    # rows of the table that scan k_int's own update has not touched: all k_int of them (it appends row k_int)
    got = tables[k_int][0]
    assert got.shape[0] == k_int + 1
    assert got[:k_int].tobytes() == want.tobytes()
    assert_logs_equal(nat_log, log)
    assert nat_sm.trajectoryDistances().tobytes() == np.array(lc.trajectory_distances, np.float32).tobytes()
    assert nat_log[k_int]["loop_count"] == log[k_int]["loop_count"] >= 0
    assert final_state(nat_sm)["table"] == nat_sm.map.poses().tobytes()


def test_phase_calls_equal_the_whole_scan_entry(core):
    a, log_a = native_run(core, 140, phases=True)
    b, log_b = native_run(core, 140)
    assert any(s["found_candidate"] for s in log_a)
    assert_logs_equal(log_a, log_b)
    assert final_state(a) == final_state(b)
    assert a.posegraph.poses().tobytes() == b.posegraph.poses().tobytes()
    assert edge_list(a.posegraph) == edge_list(b.posegraph)


def test_polling_mode_runs_to_the_end(core):
    """optimize_wait = 0.  When a result is integrated depends on timing; that the run starts an optimisation does not
    (the state machine up to that scan does not depend on the mode), and whatever was integrated left the map's pose
    table equal to float32 of the graph's poses."""
    seen = []

    def look(k, sm):
        st = sm.loopStatus()
        assert st.loop_count >= 0
        if st.integrated:
            # scan k has appended its own row behind the k integrated ones
            seen.append(sm.map.poses()[:k].tobytes() == sm.posegraph.poses()[:k].astype(np.float32).tobytes())

    sm, log = native_run(core, lh.scenario_length(), on_scan=look, optimize_wait=0)
    assert len(log) == lh.scenario_length() and sm.timestamp() == len(log)
    started = [k for k, s in enumerate(log) if s["started_optimization"]]
    assert started and started[0] == shared(core, "native")["at_first"]["scan"]
    assert all(seen), seen
    assert len(seen) == sum(s["integrated"] for s in log) <= len(started)
    # every scan but the last can leave a result to a later one; the last started optimisation may still be in flight
    assert len(seen) >= len(started) - 1
    # destroying a pipeline while an optimisation is in flight returns: stop right behind the scan that starts one
    sm2, log2 = native_run(core, started[0] + 1, optimize_wait=0)
    assert log2[-1]["started_optimization"] and log2[-1]["currently_optimizing"]
    sm2.close()
    sm.close()


def test_off_is_off(core):
    from semantic_suma_amd.types import params_with_size
    n, w, h = 60, 360, 32
    a = core.SurfelMapping(params_with_size(w, h))
    b = core.SurfelMapping(params_with_size(w, h), loop_params=loop_params())
    handed_out = b.posegraph
    assert handed_out.size() == 1
    b.enableLoopClosing(None)
    assert b.posegraph is None
    assert handed_out.h is None and handed_out.size() == 0  # the wrapper of the destroyed graph is dead, not dangling
    for k in range(n):
        sc = lh.scenario_scan(k, w, h)
        a.processScan(*sc, fixed_iterations=8)
        b.processScan(*sc, fixed_iterations=8)
    assert final_state(a) == final_state(b)
    with pytest.raises(core.SumaError, match="not enabled"):
        b.loopStatus()


def test_error_paths_and_graph_growth(core):
    from semantic_suma_amd.types import params_with_size
    w, h = 180, 16
    sm = core.SurfelMapping(params_with_size(w, h), loop_params=loop_params(node_capacity=8))
    sc = lh.scenario_scan(0, w, h)
    sm.beginScan(*sc)
    with pytest.raises(core.SumaError, match=r"\(-1\).*only between scans"):
        sm.enableLoopClosing(loop_params())
    with pytest.raises(core.SumaError, match=r"\(-1\).*between suma_pipeline_update_pose and suma_pipeline_update_map"):
        sm.checkLoopClosure()
    sm.updatePose(8)
    sm.checkLoopClosure()  # timestamp 0: nothing to do
    with pytest.raises(core.SumaError, match=r"\(-1\).*already run"):
        sm.checkLoopClosure()
    sm.updateMap()
    off = core.SurfelMapping(params_with_size(w, h))
    off.beginScan(*sc)
    off.updatePose(8)
    with pytest.raises(core.SumaError, match=r"\(-1\).*not enabled"):
        off.checkLoopClosure()
    off.updateMap()
    for k in range(1, 300):
        sm.processScan(*lh.scenario_scan(k, w, h), fixed_iterations=8)
    assert sm.posegraph.size() == 300 and sm.posegraph.edgeCount() >= 299
    assert sm.trajectoryDistances().shape == (300,)
    sm.reset()
    assert sm.posegraph.size() == 1 and sm.posegraph.edgeCount() == 0 and sm.timestamp() == 0
    assert np.array_equal(sm.posegraph.pose(0), np.eye(4))
