"""Change evidence on the CPU: the localiser over the oracle with the observation of tests/change_shim.c
(tests/change_host.py) on the edited scenario -- DESIGN.md 12's run, localised in again after one static cube and one
building have been taken out of the world -- and a control with nothing removed.  The default rule must prune what was
removed and leave the rest.  No GPU."""
import numpy as np
import pytest

import change_common as cc
import localize_common as lc
from semantic_suma_amd import synth


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("change_host")
    lshim, cshim = lc.build_shim(tmp), cc.build_shim(tmp)
    p, poses, records = cc.map_on_oracle(tmp)
    out = {}
    for name, without in (("edited", cc.REMOVED), ("control", ())):
        h, res = cc.host_run(lshim, cshim, p, records, poses[cc.FIRST], cc.edited_scans(without))
        out[name] = (h, res)
    return p, poses, records, cshim, out


def test_without_leaves_the_default_scans_alone():
    """the boxes draw no random numbers: the default is byte-identical, and a scan without a box differs"""
    for k in (0, 21, 33):
        a, b = synth.generate_scan(k, lc.LOC_W, lc.LOC_H), synth.generate_scan(k, lc.LOC_W, lc.LOC_H, without=())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = synth.generate_scan(30, lc.LOC_W, lc.LOC_H), synth.generate_scan(30, lc.LOC_W, lc.LOC_H, without=cc.REMOVED)
    assert a[0].tobytes() != b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    front = synth._BUILDINGS[cc.REMOVED[1] - len(synth._CUBES)]
    assert abs(abs(front[1]) - 0.5 * front[5] - 12.0) < 25.0  # its front face against the trajectory at y = -12


def test_both_runs_stay_tracked(runs):
    p, poses, records, cshim, out = runs
    for name, (h, res) in out.items():
        bad, worst = lc.tracking_failures([None] * cc.FIRST + [r["pose"] for r in res], poses, first=cc.FIRST + 1)
        print(name, "scans that fail", bad, "worst error %.4f m" % worst)
        assert not bad, (name, bad, worst)
        assert all(r["tracked"] and r["observed"] for r in res), name
        for r in res:
            o = r["observation"]
            assert o["n_window"] == r["n_window"] == sum(o[k] for k in cc.CATEGORIES[1:])


def test_the_control_confirms_the_map(runs):
    p, poses, records, cshim, out = runs
    for k, r in enumerate(out["control"][1]):
        o = r["observation"]
        print("control scan", cc.FIRST + k, o)
        assert o["misses"] <= o["hits"], (k, o)


def test_the_default_rule_prunes_what_was_removed(runs):
    """Measured on this restatement with the default parameters and rule (cc.MEASURED)."""
    p, poses, records, cshim, out = runs
    h, res = out["edited"]
    keep = cc.shim_prune(cshim, h.evidence)
    assert np.array_equal(keep, cc.numpy_prune(h.evidence))
    s_in, s_out, n_in = cc.shares(records, keep)
    f_control = float((~cc.shim_prune(cshim, out["control"][0].evidence)).mean())
    print("s_in %.6f (%d records inside) s_out %.6f f_control %.6f removed %d of %d" %
          (s_in, n_in, s_out, f_control, int((~keep).sum()), len(keep)))
    for name, box in zip(("cube", "building"), cc.removed_boxes()):
        si, _, ni = cc.shares(records, keep, [box])
        print(name, "s_in %.6f of %d records" % (si, ni))
    ev = h.evidence
    print("evidence sums", {f: int(ev[f].sum()) for f in ev.dtype.names})
    assert n_in > 100
    cc.check_shares(s_in, s_out, f_control)
    assert cc.MEASURED["s_in"] >= 10.0 * cc.MEASURED["s_out"]
