"""The live obstacle layer in the scan path on the MI355X: DESIGN.md 19's scenario at 360 x 32 (mapped without cube 2 and
building 41, scans 20-44 of the full world) through processScan with novelty, objects and the layer on.  Every scan's
counts and mask and the composed cells after the scans live_common.MEASURED names equal the host run (the CPU restatement
of the localiser with tests/live_shim.c behind every scan) byte for byte; every other output of the localiser is
bit-identical to a run with the layer off; and a grid_plan on the device-resident composed cells equals the plan shim."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import live_common as lv
import localize_common as lc
import novel_common as nc
import object_common as oc
import plan_common as pc
from semantic_suma_amd import core
from semantic_suma_amd.types import GRID_CELL_DTYPE, LocalizerResult, PlanParams

pytestmark = pytest.mark.gpu


def raw_scan(loc, scan):
    pts, lab, prob = (np.ascontiguousarray(a, dtype=np.float32) for a in scan)
    res = LocalizerResult()
    loc.ctx.check(loc.L.suma_localizer_process_scan(loc.h, core._ptr(pts), core._ptr(lab), core._ptr(prob), pts.shape[0], 0,
                                                    C.byref(res)), "suma_localizer_process_scan")
    return bytes(res), core.Localizer._result(res)


class Scenario:
    def __init__(self, tmp):
        from semantic_suma_amd import synth
        self.shims = lv.scenario_shims(tmp)
        self.p = lc.loc_params()
        self.scans = nc.localise_scans()
        pipe = core.SurfelMapping(self.p)
        self.poses = []
        for k in range(lc.LOC_SCANS):
            pipe.processScan(*synth.generate_scan(k, lc.LOC_W, lc.LOC_H, without=nc.ADDED)[:3])
            self.poses.append(pipe.getCurrentPose())
        self.records = pipe.map.export_world()
        pipe.close()
        self.host = lv.scenario_run(self.shims, tmp, nc.ADDED, mapped=(self.p, self.poses, self.records))
        self.gp = self.host["gp"]
        self.cache = {}

    def run(self, live):
        if live in self.cache:
            return self.cache[live]
        loc = core.Localizer(self.p)
        loc.enableNovelty()
        loc.enableObjects()
        out = dict(raw=[], res=[], col=[], model=[], window=[], obj=[], counts=[], masks=[], composed={}, plans={})
        if live:
            # the static grid on the localiser's own ctx equals the shim's; the layer takes its cells
            cells, gp, _ = core.world_grid(loc.ctx, self.records, params=self.gp)
            assert cells.tobytes() == self.host["cells"].tobytes()
            loc.enableLiveGrid(cells, self.gp)
        loc.setMap(self.records)
        loc.setPose(self.poses[nc.FIRST])
        for k, s in enumerate(self.scans):
            raw, res = raw_scan(loc, s)
            out["raw"].append(raw)
            out["res"].append(res)
            f = loc.modelFrame()
            out["model"].append(hashlib.sha1(b"".join(f.download(i).tobytes() for i in range(3))).hexdigest())
            out["window"].append(hashlib.sha1(loc.downloadWindow().tobytes()).hexdigest() if res["window_rebuilt"] else None)
            out["col"].append(loc.lastCollection())
            rec, cnt = loc.objects()
            out["obj"].append((rec.tobytes(), cnt, loc.objectIds().tobytes(), loc.novelFlags().tobytes()))
            if live:
                out["counts"].append(loc.liveCounts())
                if k in lv.KEEP:
                    comp, mask, st = loc.liveCells()
                    out["composed"][k] = (comp, st)
                    d = torch.zeros(self.gp.width * self.gp.height * 12, dtype=torch.int32, device="cuda")
                    _, mask_d, _ = loc.liveCells(out=d)
                    assert mask_d.tobytes() == mask.tobytes()
                    goal = lv.PATH_GOAL[1] * self.gp.width + lv.PATH_GOAL[0]
                    out["plans"][k] = core.grid_plan(loc.ctx, d, self.gp, [goal], PlanParams.defaults(unknown_blocked=False))
                else:
                    mask = loc.liveCells()[1]
                out["masks"].append(mask)
        out["final_window"] = loc.downloadWindow().tobytes()
        out["candidates"] = loc.novelCandidates().tobytes()
        loc.close()
        self.cache[live] = out
        return out


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    return Scenario(tmp_path_factory.mktemp("live_run"))


def test_in_loop_layer_equals_the_host_run(scenario):
    got, host = scenario.run(True), scenario.host
    for k in range(len(scenario.scans)):
        assert got["res"][k]["tracked"] and got["col"][k][1], k
        assert got["counts"][k] == host["counts"][k], (k, got["counts"][k], host["counts"][k])
        assert got["masks"][k].tobytes() == host["masks"][k].tobytes(), k
    for k in lv.KEEP:
        comp, st = got["composed"][k]
        assert comp.dtype == GRID_CELL_DTYPE and comp.tobytes() == host["composed"][k].tobytes(), k
        assert st == host["stats"][k], (k, st, host["stats"][k])
    hits, share, _ = lv.scenario_measure(dict(gp=scenario.gp, masks=got["masks"]))
    print("scans with a live cell in the building %d, smallest share %.6f" % (hits, share), [c["n_cleared"] for c in got["counts"]])
    lv.check_measured(hits, share, 0)


def test_the_layer_does_not_move_the_localiser(scenario):
    """every byte of every suma_localizer_result, every gathered window, every model frame, the counts of every
    collection, the objects, the id and flag images and the candidates"""
    on, off = scenario.run(True), scenario.run(False)
    for k in range(len(on["raw"])):
        assert on["raw"][k] == off["raw"][k], k
        assert on["model"][k] == off["model"][k] and on["window"][k] == off["window"][k], k
        assert on["col"][k] == off["col"][k] and on["obj"][k] == off["obj"][k], k
    assert on["final_window"] == off["final_window"] and on["candidates"] == off["candidates"]


def test_plan_on_the_device_resident_cells_equals_the_shim(scenario):
    got, host = scenario.run(True), scenario.host
    gp = scenario.gp
    fin = lv.footprint(gp, oc.building_box(), 0.0).reshape(-1)
    goal = lv.PATH_GOAL[1] * gp.width + lv.PATH_GOAL[0]
    pp = PlanParams.defaults(unknown_blocked=False)
    for k in lv.KEEP:
        field, st = got["plans"][k]
        want, wst = pc.shim_field(scenario.shims["p"], host["composed"][k], gp, pp, [goal])
        assert field.tobytes() == want.tobytes(), k
        assert {a: b for a, b in st.items() if a != "n_rounds"} == {a: b for a, b in wst.items() if a != "n_rounds"}
        res, rows = pc.shim_paths(scenario.shims["p"], field, gp, [lv.PATH_START[1] * gp.width + lv.PATH_START[0]],
                                  gp.width + gp.height)
        path = rows[0, :int(res["length"][0])]
        assert res["status"][0] == 0 and not fin[path].any() and res["cost"][0] > lv.MEASURED["static_cost"], (k, res)
