"""Newly seen surfaces on the CPU: the localiser over the oracle with the collection and the fusion of
tests/novel_shim.c (tests/novel_host.py) on the scenario -- DESIGN.md 12's run mapped without one static cube and one
building, then scans 20-44 of the full world localised in it -- and a control mapped and localised in the same full
world.  The fused records must lie where the world grew and nowhere else.  No GPU."""
import numpy as np
import pytest

import change_common as cc
import localize_common as lc
import novel_common as nc
from semantic_suma_amd.types import NOVEL_COUNTS


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("novel_host")
    lshim, cshim, nshim = lc.build_shim(tmp), cc.build_shim(tmp), nc.build_shim(tmp)
    scans = nc.localise_scans()
    out = {}
    for name, without in (("added", nc.ADDED), ("control", ())):
        p, poses, records = nc.map_on_oracle(tmp, without)
        h, res = nc.host_run(lshim, cshim, nshim, p, records, poses[nc.FIRST], scans)
        out[name] = (h, res, poses, records)
    return (lshim, cshim, nshim), scans, out


def test_both_runs_stay_tracked_and_the_counts_partition(runs):
    _, scans, out = runs
    for name, (h, res, poses, records) in out.items():
        bad, worst = lc.tracking_failures([None] * nc.FIRST + [r["pose"] for r in res], poses, first=nc.FIRST + 1)
        print(name, "scans that fail", bad, "worst error %.4f m" % worst)
        assert not bad, (name, bad, worst)
        assert all(r["tracked"] and r["collected"] for r in res), name
        stored = 0
        for k, r in enumerate(res):
            c = r["collection"]
            print(name, "scan", nc.FIRST + k, c)
            assert c["n_texels"] == lc.LOC_W * lc.LOC_H == sum(c[f] for f in NOVEL_COUNTS[1:6]), (name, k, c)
            assert c["stored"] == c["novel"]
            stored += c["stored"]
        cand = h.candidates()
        assert len(cand) == stored and h.col.n_overflow.value == 0
        assert np.all(np.diff(cand["timestamp"].astype(np.int64)) >= 0) and cand["timestamp"].max() == len(res) - 1
        assert np.all(cand["support"] == 1)


def test_the_fused_records_lie_where_the_world_grew(runs):
    """Measured on this restatement with the default parameters (nc.MEASURED)."""
    _, scans, out = runs
    h, res, poses, records = out["added"]
    fused, views, st = h.novel()
    n_in, n_out = nc.box_counts(fused)
    hc = out["control"][0]
    n_control = hc.novel()[2]["n_out"]
    share = max(r["collection"]["novel"] / max(1, r["collection"]["novel"] + r["collection"]["explained"])
                for r in out["control"][1])
    first_in = nc.box_counts(h.candidates())[0]
    print("candidates %d (%d inside) fused %s n_in %d n_out %d | control candidates %d n_control %d share %.6f" %
          (len(h.candidates()), first_in, st, n_in, n_out, len(hc.candidates()), n_control, share))
    for name, box in zip(("cube", "building"), cc.removed_boxes()):
        print(name, int(cc.inside_boxes(fused, [box], 0.3).sum()), "fused records")
    assert np.all(views >= 2) and st["n_dropped"] == 0
    nc.check_counts(n_in, n_out, n_control)
    assert share <= max(2 * nc.MEASURED["control_share"], 0.001)


def test_round_trip_through_the_updated_map(runs):
    """the updated map explains what the first pass found new: localising the same scans in it again leaves few
    candidates inside the boxes"""
    (lshim, cshim, nshim), scans, out = runs
    h, res, poses, records = out["added"]
    upd = h.updated_map(records)
    fused = h.novel()[0]
    assert len(upd) == int(cc.shim_prune(cshim, h.evidence).sum()) + len(fused) and upd[-len(fused):].tobytes() == fused.tobytes()
    h2, res2 = nc.host_run(lshim, cshim, nshim, h.p, upd, poses[nc.FIRST], scans)
    bad, worst = lc.tracking_failures([None] * nc.FIRST + [r["pose"] for r in res2], poses, first=nc.FIRST + 1)
    assert not bad and all(r["tracked"] for r in res2), (bad, worst)
    first_in, second_in = nc.box_counts(h.candidates())[0], nc.box_counts(h2.candidates())[0]
    print("candidates inside the boxes: first pass %d, second pass %d" % (first_in, second_in))
    nc.check_round_trip(first_in, second_in)
