#!/usr/bin/env python
"""Cost of loop closing inside the scan pipeline (suma_pipeline_enable_loop_closing): the scenario of
tests/loop_closing_host.py (circle at 0.7 m per scan, 900 x 64, 140 scans, 8 fixed iterations), same commit, same scans:

  off       processScan, loop closing not enabled
  on        processScan, loop closing enabled (the state machine in the library)
  scripted  the same decisions taken by the caller, as tests/test_gpu_posegraph.py::drifting_lap scripts them: the phase
            calls, verifyLoopClosure / trackLoopClosure and a core.Posegraph driven from Python
            (tests/loop_closing_host.LoopClosing); its states equal `on`'s scan for scan
  drifting_lap  tests/test_gpu_posegraph.py::drifting_lap itself (its own 167 scans, a closure test on every scan past
            the lap, one optimisation at the end), whole run only

Reported: scans/s over the whole run, and the host time of the scans that were quiet, searched only, verified
(candidate scan or re-verification), started an optimisation, or integrated one.  Nothing is gated.

  python tools/loop_closing_timing.py [--out profiles/loop_closing_timing.json] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(core, scans, loop_params):
    from semantic_suma_amd.types import params_with_size
    sm = core.SurfelMapping(params_with_size(900, 64), loop_params=loop_params)
    per_scan, status = [], []
    for sc in scans:
        t0 = time.perf_counter()
        sm.processScan(*sc, fixed_iterations=8)
        sm.ctx.synchronize()
        per_scan.append(time.perf_counter() - t0)
        status.append(sm.loopStatus().as_dict() if loop_params is not None else None)
    sm.close()
    return per_scan, status


def run_scripted(core, scans, scenario):
    import loop_closing_host as lh
    import loop_scenario as ls
    from semantic_suma_amd.types import params_with_size
    sm = core.SurfelMapping(params_with_size(900, 64))
    lc = lh.LoopClosing(ls.HipPipe(sm), core.Posegraph(0, node_capacity=1024, edge_capacity=2048), **scenario)
    per_scan, status = [], []
    for sc in scans:
        t0 = time.perf_counter()
        st = lc.scan(*sc)
        sm.ctx.synchronize()
        per_scan.append(time.perf_counter() - t0)
        status.append(st)
    sm.close()
    return per_scan, status


def by_kind(per_scan, status, delta_timestamp):
    kinds = dict(quiet=[], searched_only=[], verified=[], started_optimisation=[], integrated=[])
    for k in range(1, len(per_scan)):
        s = status[k]
        if s["integrated"]:
            kinds["integrated"].append(per_scan[k])
        elif s["started_optimization"]:
            kinds["started_optimisation"].append(per_scan[k])
        elif s["found_candidate"]:
            kinds["verified"].append(per_scan[k])
        elif s["time_without_loop_closure"] > 3 and k >= delta_timestamp:
            kinds["searched_only"].append(per_scan[k])
        else:
            kinds["quiet"].append(per_scan[k])
    return {k: dict(scans=len(v), mean_ms=mean_ms(v)) for k, v in kinds.items()}


def mean_ms(ts):
    return None if not ts else round(1e3 * sum(ts) / len(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_closing_timing.json"))
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import loop_closing_host as lh
    import loop_scenario as ls
    from semantic_suma_amd import core
    from semantic_suma_amd.buildinfo import kernel_source_sha
    from semantic_suma_amd.types import LoopParams
    n = lh.scenario_length()
    scans = [lh.scenario_scan(k, 900, 64) for k in range(n)]
    lp = LoopParams.defaults(**dict(lh.SCENARIO, min_valid_ratio=ls.MIN_VALID_RATIO))
    best = None
    for _ in range(args.repeat):
        off, _ = run(core, scans, None)
        on, st = run(core, scans, lp)
        scr, st_scr = run_scripted(core, scans, lh.SCENARIO)
        if best is None or sum(on) < sum(best[1]):
            best = (off, on, st, scr, st_scr)
    off, on, st, scr, st_scr = best
    import test_gpu_posegraph as tp
    lap = None
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        r = tp.drifting_lap(core, 0.004)
        dt = time.perf_counter() - t0
        if lap is None or dt < lap[0]:
            lap = (dt, r["n"], r["closures"])
    out = dict(kernel_source_sha=kernel_source_sha(), scans=n, width=900, height=64,
               scans_per_s_off=round(n / sum(off), 1), scans_per_s_on=round(n / sum(on), 1),
               scans_per_s_scripted=round(n / sum(scr), 1),
               ms_per_scan_off=mean_ms(off[1:]),
               ms_per_scan_on=by_kind(on, st, lp.delta_timestamp),
               ms_per_scan_scripted=by_kind(scr, st_scr, lp.delta_timestamp),
               loop_edges=sum(s["edges_added"] for s in st[1:]),
               optimisations=sum(s["started_optimization"] for s in st[1:]),
               drifting_lap=dict(scans=lap[1], closures=lap[2], scans_per_s=round(lap[1] / lap[0], 1)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
