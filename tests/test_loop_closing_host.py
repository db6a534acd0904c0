"""CPU checks of loop closing: the scenario the GPU tests run (tests/loop_closing_host.py) does what it is there for
under the reference's own rules, and suma_loop_find_candidate (a pure host function of the library) equals the
restatement's search on crafted trajectories.

The scenario, restated over the CPU oracle and the fp64 host graph (circle at 0.7 m per scan, 900 x 64, 140 scans, 8 fixed
iterations, min_trajectory_distance 60, search_distance 30, delta_timestamp 100, min_valid_ratio =
loop_scenario.MIN_VALID_RATIO, everything else default) gave:
  scan 101      first candidate (to = 0), queued; its re-verification on scan 102 fails the gates and it is dropped
  scan 102      a candidate is found and fails the gates of :734 (found_candidate = 1, nothing queued)
  scans 103-111 candidates queued and dropped again by the next scan's re-verification
  scans 111-114 four verifications in a row (min_verifications + 1): promoted on scan 114, 4 loop edges, loopCount_ = 4
  scan 117      loopCount_ = 7 > 6: first optimisation starts; integrated at the start of scan 118 (loopCount_ 7 -> 1 after
                the scan's own edge), and again 124/125, 131/132, 138/139
With search_distance 20 (the issue's first choice) the first candidate appears on scan 123 and passes everything: no
candidate fails, so the distance was raised as the issue allows."""
import ctypes as C

import numpy as np
import pytest

import loop_closing_host as lh
import loop_scenario as ls


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from semantic_suma_amd import core
    return core


@pytest.fixture(scope="module")
def cpu_log(built):
    from oracle import pyoracle
    from semantic_suma_amd.types import params_with_size
    op = pyoracle.OraclePipeline(params_with_size(900, 64), threads=16)
    lc = lh.LoopClosing(ls.OraclePipe(op), lh.HostGraph(), **lh.SCENARIO)
    return lc, lh.run_scenario(lc, 900, 64, lh.scenario_length())


def test_the_scenario_exercises_the_state_machine(cpu_log):
    lc, log = cpu_log
    failed = [k for k, s in enumerate(log) if s["found_candidate"] and s["candidate_to"] < 0]
    promoted = [k for k, s in enumerate(log) if s["edges_added"] >= lh.DEFAULTS["min_verifications"] + 1]
    started = [k for k, s in enumerate(log) if s["started_optimization"]]
    integrated = [k for k, s in enumerate(log) if s["integrated"]]
    print(dict(failed=failed, promoted=promoted, started=started, integrated=integrated))
    assert failed, "no candidate failed the gates"
    assert promoted, "never min_verifications + 1 verified candidates"
    assert started and integrated and integrated[0] == started[0] + 1 and integrated[0] < len(log) - 1
    assert all(s["loop_count"] >= 0 for s in log)
    assert lc.graph.size() == len(log) and len(lc.edges) == len(log) - 1 + sum(s["edges_added"] for s in log)


def _poses(xyz):
    P = np.tile(np.eye(4), (len(xyz), 1, 1))
    P[:, :3, 3] = xyz
    return P


def _both(core, P, d, t, cur, radius, min_traj, delta):
    a = core.loop_find_candidate(P, d, t, cur, radius, min_traj, delta)
    b = lh.find_candidate(P, np.asarray(d, np.float32), t, cur, radius, min_traj, delta)
    assert a == b, (a, b)
    return a


def test_find_candidate_on_crafted_trajectories(built):
    core = built
    cur = np.eye(4)
    # an empty range: timestamp < delta_timestamp
    P = _poses(np.zeros((6, 3)))
    d = np.arange(6, dtype=np.float32) * 100
    assert _both(core, P, d, 5, cur, 20.0, 1.0, 100) == -1
    assert _both(core, P, d, 5, cur, 20.0, 1.0, 5) == 0
    # two poses at exactly equal distance: j runs downwards and the comparison is strict, so the higher index wins
    P = _poses([[3, 0, 0], [0, 3, 0], [9, 9, 9], [9, 9, 9]])
    d = np.array([0, 10, 20, 500], np.float32)
    assert _both(core, P, d, 3, cur, 20.0, 1.0, 2) == 1
    # nearer in double, equal after the cast to float: still the higher index
    P = _poses([[3.0 - 1e-12, 0, 0], [0, 3, 0], [9, 9, 9], [9, 9, 9]])
    assert np.float32(3.0 - 1e-12) == np.float32(3.0)
    assert _both(core, P, d, 3, cur, 20.0, 1.0, 2) == 1
    # ... and one that is nearer in float as well does win
    P = _poses([[3.0 - 1e-6, 0, 0], [0, 3, 0], [9, 9, 9], [9, 9, 9]])
    assert _both(core, P, d, 3, cur, 20.0, 1.0, 2) == 0
    # the trajectory-distance gate exactly at the threshold: strict >
    P = _poses([[1, 0, 0], [2, 0, 0], [9, 9, 9]])
    d = np.array([0, 50, 250], np.float32)
    assert _both(core, P, d, 2, cur, 20.0, 200.0, 1) == 0  # 250 - 50 = 200 is not > 200; 250 - 0 is
    assert _both(core, P, d, 2, cur, 20.0, 250.0, 1) == -1
    # the radius is strict as well
    assert _both(core, _poses([[20, 0, 0], [9, 9, 9]]), np.array([0, 500], np.float32), 1, cur, 20.0, 1.0, 1) == -1


def test_find_candidate_on_a_random_walk(built):
    core = built
    rng = np.random.default_rng(5)
    n = 5000
    steps = rng.normal(0, 0.6, (n, 3)) * [1, 1, 0.02]
    xyz = np.cumsum(steps, axis=0)
    P = _poses(xyz)
    d = np.zeros(n, np.float32)
    acc = np.float32(0)
    for t in range(1, n):
        acc = np.float32(float(acc) + float(np.linalg.norm(xyz[t] - xyz[t - 1])))
        d[t] = acc
    hits = 0
    for t in list(range(100, n, 97)) + [n - 1]:
        hits += _both(core, P, d, t, P[t], 20.0, 200.0, 100) >= 0
    assert hits > 5
