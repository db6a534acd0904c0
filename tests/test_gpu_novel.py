"""Newly seen surfaces on the MI355X (csrc/k_novel.hip, suma_localizer_*novel*, core.Localizer): kn_mark, kn_collect and
kn_emit byte for byte against the host restatement (tests/novel_shim.c) on a crafted frame around every boundary of the
specification; the fusion against the shim; the 25-scan scenario against the whole localiser over the CPU oracle
(tests/novel_host.py) with the conditions of DESIGN.md 15; novelty on or off does not move the localiser; bookkeeping;
the round trip through the updated map."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import change_common as cc
import localize_common as lc
import novel_common as nc
from semantic_suma_amd import core
from semantic_suma_amd.types import (LocalizerParams, LocalizerResult, NOVEL_COUNTS, NovelFuseParams, NovelParams,
                                     WORLD_SURFEL_DTYPE)

pytestmark = pytest.mark.gpu

ZERO = dict.fromkeys(NOVEL_COUNTS, 0)


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("novel_gpu")
    return lc.build_shim(tmp), cc.build_shim(tmp), nc.build_shim(tmp)


@pytest.fixture(scope="module")
def crafted_loc():
    loc = core.Localizer(nc.crafted_params())
    loc.enableNovelty(nc.crafted_novel_params())
    yield loc
    loc.close()


def upload(loc, maps):
    p = loc.params
    f = core.Frame(loc.ctx, p.data_width, p.data_height)
    f.set(*maps)
    return f


# ---- 1. mark and candidates against the shim
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1025])
def test_collection_equals_shim(shims, crafted_loc, n):
    lshim, cshim, nshim = shims
    loc = crafted_loc
    case = nc.crafted_case(lshim, cshim, nshim, n)
    rec, p = case["records"], case["params"]
    m = lc.ShimMap(lshim, rec, p.submap_extent)
    assert loc.setMap(rec) == m.n_dropped == 8
    frame = upload(loc, case["maps"])
    assert loc.collectFrame(frame, cc.crafted_pose(), 3) == ZERO      # no window yet: nothing is collected
    assert len(loc.novelCandidates()) == 0 and loc.lastCollection() == (ZERO, False)
    loc.setPose(cc.crafted_pose())
    origin, n_window, _ = loc.window()
    win = cc.window_sources(m, origin[0], origin[1], p.submap_dimension)
    assert origin == (0, 0) and n_window == len(win) > 900
    col = nc.ShimCollector(nshim, p, case["np"])
    # the plain pose: every boundary to the bit
    want = col.collect(rec, win, case["maps"], cc.crafted_pose(), 7)
    nc.crafted_expectations(case, col.category, col.mark, col.candidates())
    got = loc.collectFrame(frame, cc.crafted_pose(), 7)
    assert got == want and sum(got[k] for k in NOVEL_COUNTS[1:6]) == got["n_texels"] == cc.CW * cc.CH, (got, want)
    assert all(got[k] > 0 for k in NOVEL_COUNTS), got
    assert loc.novelMarks().tobytes() == col.mark.tobytes()
    assert loc.lastCollection() == (want, True)
    cand = loc.novelCandidates()
    assert cand.dtype == WORLD_SURFEL_DTYPE and cand.tobytes() == col.candidates().tobytes()
    # a turned pose appends behind it: the general path
    T = cc.crafted_pose(turned=True)
    want2 = col.collect(rec, win, case["maps"], T, 8)
    assert loc.collectFrame(frame, T, 8) == want2 and want2["novel"] > 0
    assert loc.novelMarks().tobytes() == col.mark.tobytes()
    both = loc.novelCandidates()
    assert len(both) == want["stored"] + want2["stored"] and both.tobytes() == col.candidates().tobytes()
    assert both[:len(cand)].tobytes() == cand.tobytes() and set(both["timestamp"][len(cand):]) == {8}
    # a pose whose fp32 translation is infinite: no world position is finite, nothing is collected
    far = cc.crafted_pose()
    far[0, 3] = 1e39
    want3 = col.collect(rec, win, case["maps"], far, 9)
    assert loc.collectFrame(frame, far, 9) == want3 and want3["novel"] == 0 and want3["out_of_range"] > 200
    assert loc.novelCandidates().tobytes() == both.tobytes()
    # the device download equals the host one
    d = torch.zeros(len(both) * 12 + 8, dtype=torch.int32, device="cuda")
    n_dev = C.c_uint32(0)
    loc.ctx.check(loc.L.suma_localizer_novel_candidates_device(loc.h, core._dev(d), len(both), C.byref(n_dev)), "device")
    back = d.cpu().numpy().view(np.uint32)
    assert n_dev.value == len(both) and back[:len(both) * 12].tobytes() == both.tobytes() and not back[len(both) * 12:].any()
    fused, views = loc.novel(NovelFuseParams(0.2, 2, 1.0))
    sf = col.fuse(NovelFuseParams(0.2, 2, 1.0))
    assert fused.tobytes() == sf[0].tobytes() and views.tobytes() == sf[1].tobytes()
    loc.clearNovelty()
    assert len(loc.novelCandidates()) == 0 and loc.lastCollection() == (ZERO, False)


def test_capacity(shims):
    """max_candidates below the crafted count: the first records are kept in order, n_overflow is exact and the
    downloads return SUMA_ERR_CAPACITY after filling their outputs"""
    lshim, cshim, nshim = shims
    case = nc.crafted_case(lshim, cshim, nshim, 257)
    rec, p = case["records"], case["params"]
    m = lc.ShimMap(lshim, rec, p.submap_extent)
    full = nc.ShimCollector(nshim, p, case["np"])
    win = cc.window_sources(m, 0, 0, p.submap_dimension)
    first = full.collect(rec, win, case["maps"], cc.crafted_pose(), 0)
    second = full.collect(rec, win, case["maps"], cc.crafted_pose(turned=True), 1)
    cap = first["novel"] + 40
    assert second["novel"] > 40
    small = nc.crafted_novel_params(max_candidates=cap)
    col = nc.ShimCollector(nshim, p, small)
    loc = core.Localizer(p)
    loc.enableNovelty(small)
    loc.setMap(rec)
    loc.setPose(cc.crafted_pose())
    frame = upload(loc, case["maps"])
    for k, T in enumerate((cc.crafted_pose(), cc.crafted_pose(turned=True), cc.crafted_pose())):
        want = col.collect(rec, win, case["maps"], T, k)
        assert loc.collectFrame(frame, T, k) == want, k
    assert want["stored"] == 0 and want["novel"] == first["novel"]
    with pytest.raises(core.SumaError, match="did not fit"):
        loc.novelCandidates()
    with pytest.raises(core.SumaError, match="did not fit"):
        loc.lastCollection()
    with pytest.raises(core.SumaError, match="did not fit"):
        loc.novel()
    n = C.c_uint32(0)
    buf = np.zeros(cap + 4, dtype=WORLD_SURFEL_DTYPE)
    assert loc.L.suma_localizer_novel_candidates(loc.h, core._ptr(buf), len(buf), C.byref(n)) == -3   # SUMA_ERR_CAPACITY
    assert n.value == cap and buf[:cap].tobytes() == full.candidates()[:cap].tobytes() and not buf[cap:].view(np.uint32).any()
    assert loc.novelCandidates(allow_overflow=True).tobytes() == col.candidates().tobytes()
    _, _, st = loc.novel(allow_overflow=True, stats=True)
    assert st["n_candidates"] == cap and st["n_overflow"] == col.n_overflow.value == second["novel"] - 40 + first["novel"]
    assert loc.lastCollection(allow_overflow=True) == (want, True)
    loc.clearNovelty()
    assert len(loc.novelCandidates()) == 0                       # and the overflow is forgotten
    loc.close()


# ---- 2. fusion against the shim
def test_fusion_equals_shim(shims, crafted_loc):
    nshim = shims[2]
    loc = crafted_loc
    crafted, _ = nc.crafted_candidates()
    sets = [crafted, crafted[:0], crafted[:1], crafted[:2], np.concatenate([crafted, nc.random_candidates()])]
    for cand in sets:
        if len(cand) > 4096:
            loc.enableNovelty(nc.crafted_novel_params(max_candidates=8192))
        loc.setNovelCandidates(cand)
        assert loc.novelCandidates().tobytes() == cand.tobytes()
        for fp in (NovelFuseParams(0.2, 2, 1.0), NovelFuseParams(0.2, 1, -2.0), NovelFuseParams(0.2, 3, 1.0),
                   NovelFuseParams(0.5, 2, 4.0)):
            want = nc.shim_fuse(nshim, cand, fp)
            rec, views, st = loc.novel(fp, stats=True)
            assert {k: st[k] for k in want[2]} == want[2] and st["n_candidates"] == len(cand), (len(cand), st, want[2])
            assert rec.tobytes() == want[0].tobytes() and views.tobytes() == want[1].tobytes(), (len(cand), fp.min_views)
            again = loc.novel(fp)
            assert again[0].tobytes() == rec.tobytes() and again[1].tobytes() == views.tobytes()
    # the device variant, and a capacity below n_out: the first records
    fp = NovelFuseParams(0.2, 2, 1.0)
    want = nc.shim_fuse(nshim, sets[-1], fp)
    k = want[2]["n_out"]
    assert k > 100
    d = torch.zeros(k * 12, dtype=torch.int32, device="cuda")
    dv = torch.zeros(k, dtype=torch.int32, device="cuda")
    st = core.NovelStats()
    loc.ctx.check(loc.L.suma_localizer_novel_device(loc.h, C.byref(fp), core._dev(d), core._dev(dv), k - 50, C.byref(st)), "dev")
    got = d.cpu().numpy().view(np.uint32)
    assert st.n_out == k and got[:(k - 50) * 12].tobytes() == want[0][:k - 50].tobytes() and not got[(k - 50) * 12:].any()
    assert dv.cpu().numpy().view(np.uint32)[:k - 50].tobytes() == want[1][:k - 50].tobytes()
    with pytest.raises(core.SumaError, match="max_candidates"):
        loc.setNovelCandidates(np.zeros(8193, dtype=WORLD_SURFEL_DTYPE))
    loc.enableNovelty(nc.crafted_novel_params())


# ---- 3-6. the scenario
def raw_scan(loc, scan):
    pts, lab, prob = (np.ascontiguousarray(a, dtype=np.float32) for a in scan)
    res = LocalizerResult()
    loc.ctx.check(loc.L.suma_localizer_process_scan(loc.h, core._ptr(pts), core._ptr(lab), core._ptr(prob), pts.shape[0], 0,
                                                    C.byref(res)), "suma_localizer_process_scan")
    return bytes(res), core.Localizer._result(res)


def model_digest(loc):
    f = loc.modelFrame()
    return hashlib.sha1(b"".join(f.download(k).tobytes() for k in range(3))).hexdigest()


class Scenario:
    """scans 0-44 of the world without the two boxes mapped on the GPU once; scans 20-44 of the full world localised with
    novelty / evidence on and off, and over the CPU oracle; each made once and shared"""

    def __init__(self, shims):
        self.lshim, self.cshim, self.nshim = shims
        self.p = lc.loc_params()
        self.scans = nc.localise_scans()
        self.cache = {}
        self.index = None
        self.poses, self.records = self.mapped(nc.ADDED, index=True)
        self.start = self.poses[nc.FIRST]

    def mapped(self, without, index=False):
        """-> (poses, records); with ``index`` a place index of the even scans is kept too"""
        from semantic_suma_amd import synth
        from semantic_suma_amd.types import PlaceParams
        pipe = core.SurfelMapping(self.p)
        if index:
            self.index = core.PlaceIndex(PlaceParams.defaults(max_range=50.0), capacity=2)
        poses = []
        for k in range(lc.LOC_SCANS):
            pipe.processScan(*synth.generate_scan(k, lc.LOC_W, lc.LOC_H, without=without)[:3])
            poses.append(pipe.getCurrentPose())
            if index and k % 2 == 0:
                self.index.addFrame(pipe.ctx, pipe.frame(0), k)
        records = pipe.map.export_world()
        pipe.close()
        return poses, records

    def gpu(self, novelty, evidence, records=None, start=None):
        key = (novelty, evidence, records is None)
        if key in self.cache:
            return self.cache[key]
        loc = core.Localizer(self.p)
        if evidence:
            loc.enableEvidence()
        if novelty:
            loc.enableNovelty()
        recs = self.records if records is None else records
        loc.setMap(recs)
        loc.setPose(self.start if start is None else start)
        out = dict(raw=[], res=[], col=[], model=[], window=[])
        for s in self.scans:
            raw, res = raw_scan(loc, s)
            out["raw"].append(raw)
            out["res"].append(res)
            out["model"].append(model_digest(loc))
            out["window"].append(hashlib.sha1(loc.downloadWindow().tobytes()).hexdigest() if res["window_rebuilt"] else None)
            if novelty:
                out["col"].append(loc.lastCollection())
        out["final_window"] = loc.downloadWindow().tobytes()
        if evidence:
            out["evidence"] = loc.evidence()
        if novelty:
            out["candidates"] = loc.novelCandidates()
            out["fused"] = loc.novel(stats=True)
            out["updated"] = loc.updatedMap(recs)
        loc.close()
        self.cache[key] = out
        return out

    def host(self):
        if "host" not in self.cache:
            self.cache["host"] = nc.host_run(self.lshim, self.cshim, self.nshim, self.p, self.records, self.start, self.scans)
        return self.cache["host"]


@pytest.fixture(scope="module")
def scenario(shims):
    return Scenario(shims)


def test_scenario_equals_the_host_restatement(scenario):
    """candidates, every scan's counts and the fused records against tests/novel_host.py over the CPU oracle, and the
    conditions of DESIGN.md 15"""
    import localize_host as lh
    got = scenario.gpu(True, True)
    h, want = scenario.host()
    assert len(got["res"]) == len(want) == nc.LAST - nc.FIRST + 1
    for k, (a, b) in enumerate(zip(got["res"], want)):
        lh.results_equal(a, b, k)
        assert got["col"][k] == (b["collection"], b["collected"]), (k, got["col"][k], b["collection"])
        assert got["col"][k][1] and a["tracked"]
    assert sum(r["window_rebuilt"] for r in got["res"]) >= 1
    cand = got["candidates"]
    assert cand.tobytes() == h.candidates().tobytes()
    fused, views, st = got["fused"]
    hf = h.novel()
    assert fused.tobytes() == hf[0].tobytes() and views.tobytes() == hf[1].tobytes()
    assert {k: st[k] for k in hf[2]} == hf[2] and st["n_candidates"] == len(cand) and st["n_overflow"] == 0
    assert got["evidence"].tobytes() == h.evidence.tobytes()
    assert got["updated"].tobytes() == h.updated_map(scenario.records).tobytes()
    bad, worst = lc.tracking_failures([None] * nc.FIRST + [r["pose"] for r in got["res"]], scenario.poses, first=nc.FIRST + 1)
    assert not bad, (bad, worst)
    n_in, n_out = nc.box_counts(fused)
    print("candidates %d fused %d n_in %d n_out %d" % (len(cand), len(fused), n_in, n_out))
    nc.check_counts(n_in, n_out)


def test_the_control_collects_little(scenario):
    """mapped and localised in the same full world, against the host restatement run on the same map"""
    poses, records = scenario.mapped(())
    loc = core.Localizer(scenario.p)
    loc.enableNovelty()
    loc.setMap(records)
    loc.setPose(poses[nc.FIRST])
    h, _ = nc.host_run(scenario.lshim, scenario.cshim, scenario.nshim, scenario.p, records, poses[nc.FIRST], scenario.scans)
    shares = []
    for s in scenario.scans:
        assert loc.processScan(*s)["tracked"]
        c = loc.lastCollection()[0]
        shares.append(c["novel"] / max(1, c["novel"] + c["explained"]))
    fused, views, st = loc.novel(stats=True)
    assert loc.novelCandidates().tobytes() == h.candidates().tobytes() and fused.tobytes() == h.novel()[0].tobytes()
    print("control candidates %d fused %d share %.6f" % (st["n_candidates"], st["n_out"], max(shares)))
    assert st["n_out"] <= max(2 * nc.MEASURED["n_control"], 5)
    assert max(shares) <= max(2 * nc.MEASURED["control_share"], 0.001)
    loc.close()


def test_novelty_does_not_move_the_localiser(scenario):
    """all bytes of every suma_localizer_result, every gathered window and every model frame; and the evidence"""
    on, off = scenario.gpu(True, False), scenario.gpu(False, False)
    for k in range(len(on["raw"])):
        assert on["raw"][k] == off["raw"][k], k
        assert on["model"][k] == off["model"][k] and on["window"][k] == off["window"][k], k
    assert on["final_window"] == off["final_window"]
    both, ev = scenario.gpu(True, True), scenario.gpu(False, True)
    assert both["raw"] == ev["raw"] == off["raw"] and both["model"] == off["model"]
    assert both["evidence"].tobytes() == ev["evidence"].tobytes()
    assert both["candidates"].tobytes() == on["candidates"].tobytes()
    # nothing is pruned while evidence is off: the records, then the fused ones
    fused = on["fused"][0]
    assert on["updated"].tobytes() == np.concatenate([scenario.records, fused]).tobytes()


def test_round_trip_through_the_updated_map(scenario):
    first = scenario.gpu(True, True)
    second = scenario.gpu(True, True, records=first["updated"])
    assert all(r["tracked"] for r in second["res"])
    bad, worst = lc.tracking_failures([None] * nc.FIRST + [r["pose"] for r in second["res"]], scenario.poses, first=nc.FIRST + 1)
    assert not bad, (bad, worst)
    first_in, second_in = nc.box_counts(first["candidates"])[0], nc.box_counts(second["candidates"])[0]
    print("candidates inside the boxes: first pass %d, second pass %d" % (first_in, second_in))
    nc.check_round_trip(first_in, second_in)


# ---- 5. behaviour at the edges
def test_tracked_only(scenario):
    lp = LocalizerParams.defaults(scenario.p, min_valid_ratio=1.1)   # passes no scan
    loc = core.Localizer(scenario.p, lp)
    loc.enableNovelty()
    loc.setMap(scenario.records)
    loc.setPose(scenario.start)
    for s in scenario.scans[:2]:
        r = loc.processScan(*s)
        assert not r["tracked"] and r["n_window"] > 0 and loc.lastCollection() == (ZERO, False)
    assert len(loc.novelCandidates()) == 0
    loc.enableNovelty(NovelParams.defaults(tracked_only=0))         # the parameters change at once, the candidates stay
    r = loc.processScan(*scenario.scans[2])
    cnt, collected = loc.lastCollection()
    cand = loc.novelCandidates()
    assert not r["tracked"] and collected and cnt["stored"] == cnt["novel"] == len(cand) > 0
    assert set(cand["timestamp"]) == {2}                            # the scans that did not collect have counted
    loc.close()


def test_empty_window_relocalize_set_map_and_refusals(scenario):
    p = scenario.p
    loc = core.Localizer(p)
    frame = core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H)
    for call in (loc.lastCollection, loc.novelCandidates, loc.novel, loc.clearNovelty, loc.novelMarks,
                 lambda: loc.collectFrame(frame, scenario.start, 0), lambda: loc.setNovelCandidates(scenario.records[:2])):
        with pytest.raises(core.SumaError, match="novelty is off"):
            call()
    for bad, what in ((dict(agree_margin=0.0), "agree_margin"), (dict(agree_margin=float("nan")), "agree_margin"),
                      (dict(max_range=float("inf")), "max_range"), (dict(max_range=-1.0), "max_range"),
                      (dict(max_candidates=0), "max_candidates"), (dict(max_candidates=(1 << 30) + 1), "max_candidates")):
        with pytest.raises(core.SumaError, match=what):
            loc.enableNovelty(NovelParams.defaults(**bad))
    with pytest.raises(core.SumaError, match="novelty is off"):   # a refused enable switches nothing on
        loc.novelCandidates()
    loc.enableNovelty(NovelParams.defaults(max_candidates=1 << 16))
    assert loc.collectFrame(frame, scenario.start, 0) == ZERO       # no map yet
    loc.setMap(scenario.records)
    # an empty window collects nothing
    far = np.array(scenario.start)
    far[0, 3], far[1, 3] = 900.0, -900.0
    loc.setPose(far)
    assert loc.window()[1] == 0
    r = loc.processScan(*scenario.scans[0])
    assert r["n_window"] == 0 and loc.lastCollection() == (ZERO, False) and len(loc.novelCandidates()) == 0
    full = core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H)
    full.set(*[np.ones((lc.LOC_H, lc.LOC_W, 4), dtype=np.float32)] * 3)
    assert loc.collectFrame(full, far, 0) == ZERO
    # refusals of the primitive
    loc.setPose(scenario.start)
    with pytest.raises(core.SumaError, match="non-finite"):
        loc.collectFrame(full, np.full((4, 4), np.nan), 0)
    with pytest.raises(core.SumaError, match="data image"):
        loc.collectFrame(core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H + 1), scenario.start, 0)
    other = core.Localizer(p)
    with pytest.raises(core.SumaError, match="another ctx"):
        loc.collectFrame(core.Frame(other.ctx, lc.LOC_W, lc.LOC_H), scenario.start, 0)
    other.close()
    for fp, what in ((NovelFuseParams(0.0, 2, 1.0), "voxel_size"), (NovelFuseParams(float("inf"), 2, 1.0), "voxel_size"),
                     (NovelFuseParams(0.2, 0, 1.0), "min_views"), (NovelFuseParams(0.2, 2, float("nan")), "confidence")):
        with pytest.raises(core.SumaError, match=what):
            loc.novel(fp)
    # the scan after the empty one is scan 1; relocalize collects nothing and does not count
    loc.processScan(*scenario.scans[0])
    cand = loc.novelCandidates()
    assert len(cand) > 0 and set(cand["timestamp"]) == {1}
    entry_poses = np.stack(scenario.poses[0:lc.LOC_SCANS:2])
    got = loc.relocalize(scenario.index, entry_poses, *scenario.scans[10], max_candidates=4)
    assert got["found"] and got["n_tried"] >= 1
    assert loc.novelCandidates().tobytes() == cand.tobytes()
    loc.processScan(*scenario.scans[11])
    assert set(loc.novelCandidates()["timestamp"]) == {1, 2}        # the relocalisation was no scan
    loc.setMap(scenario.records)                                    # a new map clears and restarts the count
    assert len(loc.novelCandidates()) == 0 and loc.lastCollection() == (ZERO, False)
    loc.setPose(scenario.start)
    loc.processScan(*scenario.scans[0])
    assert set(loc.novelCandidates()["timestamp"]) == {0}
    loc.disableNovelty()
    with pytest.raises(core.SumaError, match="novelty is off"):
        loc.novelCandidates()
    assert loc.processScan(*scenario.scans[1])["tracked"]           # and the scan path goes on without it
    loc.close()
