"""Wall time of Posegraph.optimize(100) on the 4541-node, 300-loop graph of tests/test_gpu_posegraph.py,
with LM iterations and CG iterations per damped solve; --host times the fp64 host restatement (tests/posegraph_host.py)
on the same graph instead.  Run under `rocprofv3 --kernel-trace --stats -- python tools/posegraph_timing.py` for the
per-kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import posegraph_host as ph  # noqa: E402
from semantic_suma_amd import synth  # noqa: E402


def make_graph():
    rng = np.random.default_rng(7)
    traj = [synth.trajectory_pose(k) for k in range(4541)]
    return ph.chain_graph(4541, 300, rng, trajectory=traj, loop_min_gap=50)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    hg = make_graph()
    if a.host:
        t0 = time.perf_counter()
        _, st = ph.levenberg_marquardt(hg, max_iterations=100)
        print(json.dumps(dict(host_seconds=time.perf_counter() - t0, **st)))
        return
    from semantic_suma_amd import core
    g = core.Posegraph(0, node_capacity=len(hg.nodes), edge_capacity=len(hg.edges))
    for i, T in enumerate(hg.nodes):
        g.setInitial(i, T)
    for f, t, Z, O in hg.edges:
        g.addEdge(f, t, Z, O)
    g.optimize(100)  # warm-up: code objects, allocations, structure upload
    times = []
    for _ in range(a.repeats):
        g.reinitialize()
        t0 = time.perf_counter()
        g.optimize(100)
        times.append(time.perf_counter() - t0)
    st = g.last_stats.as_dict()
    print(json.dumps(dict(wall_seconds=sorted(times)[len(times) // 2], all_seconds=times,
                          cg_per_solve=st["cg_iterations"] / max(st["linear_solves"], 1), **st)))


if __name__ == "__main__":
    main()
