"""The tracks in the scan path on the MI355X: DESIGN.md 19's scenario at 360 x 32 (mapped without cube 2 and building 41,
scans 20-44 of the full world) through processScan with novelty, evidence, objects, the live layer and the tracks on.
Every scan's tracks(), objectTracks() and raw table equal tests/track_shim.c applied to the library's own objects() byte
for byte; the semantic conditions of DESIGN.md 21 hold; and every other output of the localiser -- results, windows,
model frames, collections, objects, ids, flags, candidates, evidence, live counts and composed cells -- is bit-identical
to a run with the tracks off."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import grid_common as gc
import localize_common as lc
import novel_common as nc
import track_common as tc
from semantic_suma_amd import core
from semantic_suma_amd.types import GridParams, LocalizerResult

pytestmark = pytest.mark.gpu


def raw_scan(loc, scan):
    pts, lab, prob = (np.ascontiguousarray(a, dtype=np.float32) for a in scan)
    res = LocalizerResult()
    loc.ctx.check(loc.L.suma_localizer_process_scan(loc.h, core._ptr(pts), core._ptr(lab), core._ptr(prob), pts.shape[0], 0,
                                                    C.byref(res)), "suma_localizer_process_scan")
    return bytes(res), core.Localizer._result(res)


class Scenario:
    def __init__(self, tmp):
        self.shim = tc.build_shim(tmp)
        self.p = lc.loc_params()
        self.scans = nc.localise_scans()
        self.maps, self.cache = {}, {}

    def mapped(self, without):
        from semantic_suma_amd import synth
        if without not in self.maps:
            pipe = core.SurfelMapping(self.p)
            poses = []
            for k in range(lc.LOC_SCANS):
                pipe.processScan(*synth.generate_scan(k, lc.LOC_W, lc.LOC_H, without=without)[:3])
                poses.append(pipe.getCurrentPose())
            self.maps[without] = (poses, pipe.map.export_world())
            pipe.close()
        return self.maps[without]

    def run(self, tracks, without=nc.ADDED, everything=True):
        key = (tracks, without, everything)
        if key in self.cache:
            return self.cache[key]
        poses, records = self.mapped(without)
        loc = core.Localizer(self.p)
        loc.enableNovelty()
        loc.enableObjects()
        out = dict(raw=[], model=[], window=[], col=[], obj=[], live=[], tracks=[], state=[])
        if everything:
            loc.enableEvidence()
            ox, oy, w, h = gc.fit_of(records, 0.2, 1)
            gp = GridParams.defaults(cell_size=0.2, origin=(ox, oy), width=w, height=h)
            cells, gp, _ = core.world_grid(loc.ctx, records, params=gp)
            loc.enableLiveGrid(cells, gp)
        if tracks:
            loc.enableTracks()
        loc.setMap(records)
        loc.setPose(poses[nc.FIRST])
        for k, s in enumerate(self.scans):
            raw, res = raw_scan(loc, s)
            assert res["tracked"]
            out["raw"].append(raw)
            f = loc.modelFrame()
            out["model"].append(hashlib.sha1(b"".join(f.download(i).tobytes() for i in range(3))).hexdigest())
            out["window"].append(hashlib.sha1(loc.downloadWindow().tobytes()).hexdigest() if res["window_rebuilt"] else None)
            out["col"].append(loc.lastCollection())
            rec, cnt = loc.objects()
            out["obj"].append((rec, cnt, loc.objectIds().tobytes(), loc.novelFlags().tobytes()))
            if everything:
                comp, mask, st = loc.liveCells()
                out["live"].append((loc.liveCounts(), hashlib.sha1(comp.tobytes() + mask.tobytes()).hexdigest(), st))
            if tracks:
                out["tracks"].append(loc.tracks() + (loc.objectTracks(),))
                out["state"].append(loc.trackState())
        out["final_window"] = loc.downloadWindow().tobytes()
        out["candidates"] = loc.novelCandidates().tobytes()
        out["evidence"] = loc.evidence().tobytes() if everything else b""
        loc.close()
        self.cache[key] = out
        return out


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    return Scenario(tmp_path_factory.mktemp("track_run"))


def test_in_loop_tracks_equal_the_shim_on_the_librarys_objects(scenario):
    got = scenario.run(True)
    want = tc.ShimTracker(scenario.shim)
    for k in range(len(scenario.scans)):
        rec = got["obj"][k][0]
        tracks, cnt, ot = got["tracks"][k]
        w = want.update(rec, k)                                 # processScan counts its scans from setMap
        tc.same((tracks, ot, cnt), w, k)
        slots, last, nxt = got["state"][k]
        assert slots.tobytes() == want.slots.tobytes() and (last, nxt) == (want.last_stamp, want.next_id), k
        tc.check_counts(cnt, want.tp, len(tracks))
        assert cnt["n_objects"] == len(rec) == len(ot)


def test_the_moving_car_keeps_its_track(scenario):
    """the semantic conditions on the device's own tracks: the quantities of track_common.MEASURED within its margins"""
    played = iter(scenario.run(True)["tracks"])
    m = tc.scenario_measure([o[0] for o in scenario.run(True)["obj"]], nc.FIRST, lambda rec, k: (lambda t: (t[0], t[2]))(next(played)))
    control = scenario.run(True, without=(), everything=False)
    played = iter(control["tracks"])
    c = tc.scenario_measure([o[0] for o in control["obj"]], nc.FIRST, lambda rec, k: (lambda t: (t[0], t[2]))(next(played)))
    print("added:", m)
    print("control:", c)
    tc.check_measured(m["cube_track_scans"], m["cube_ids"], m["net_error"], m["velocity_error"], m["still_speed"],
                      c["max_confirmed"], m["net_velocity"])
    # one id from the confirmation on, across the scans without the car
    assert m["cube_id_scans"][-1] >= 38 and len(m["cube_id_scans"]) >= 12, m


def test_the_tracks_do_not_move_the_localiser(scenario):
    """every byte of every suma_localizer_result, every gathered window, every model frame, the counts of every
    collection, the objects, the id and flag images, the candidates, the evidence, the live counts and composed cells"""
    on, off = scenario.run(True), scenario.run(False)
    for k in range(len(on["raw"])):
        assert on["raw"][k] == off["raw"][k], k
        assert on["model"][k] == off["model"][k] and on["window"][k] == off["window"][k], k
        assert on["col"][k] == off["col"][k] and on["live"][k] == off["live"][k], k
        a, b = on["obj"][k], off["obj"][k]
        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:], k
    assert on["final_window"] == off["final_window"] and on["candidates"] == off["candidates"]
    assert on["evidence"] == off["evidence"] and len(on["evidence"]) > 0
