"""Change evidence on the MI355X (csrc/k_change.hip, suma_localizer_*evidence*, core.Localizer): kc_observe and
kc_scatter byte for byte against the host restatement (tests/change_shim.c) on crafted input around every boundary of
the specification; the edited 25-scan run against the whole localiser over the CPU oracle (tests/change_host.py) with
the pruning conditions of DESIGN.md 14; evidence on or off does not move the localiser; bookkeeping."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import change_common as cc
import localize_common as lc
from semantic_suma_amd import core
from semantic_suma_amd.types import ChangeParams, EVIDENCE_DTYPE, LocalizerParams, LocalizerResult, WORLD_SURFEL_DTYPE

pytestmark = pytest.mark.gpu

TOTALS = cc.CATEGORIES + ("label_changes",)


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("change_gpu")
    return lc.build_shim(tmp), cc.build_shim(tmp)


@pytest.fixture(scope="module")
def crafted_loc():
    loc = core.Localizer(cc.crafted_params())
    loc.enableEvidence(cc.crafted_change_params())
    yield loc
    loc.close()


def upload(loc, maps):
    p = loc.params
    f = core.Frame(loc.ctx, p.data_width, p.data_height)
    f.set(*maps)
    return f


# ---- 1. the kernels against the shim
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025])
def test_observation_equals_shim(shims, crafted_loc, n):
    lshim, cshim = shims
    loc = crafted_loc
    case = cc.crafted_case(lshim, cshim, n)
    rec, p, cp = case["records"], case["params"], case["cp"]
    m = lc.ShimMap(lshim, rec, p.submap_extent)
    assert loc.setMap(rec) == m.n_dropped == 8
    frame = upload(loc, case["maps"])
    want = np.zeros(len(rec), dtype=EVIDENCE_DTYPE)
    assert loc.evidence().tobytes() == want.tobytes()
    before = loc.observeFrame(frame, cc.crafted_pose())          # no window yet: nothing is observed
    assert before == dict.fromkeys(TOTALS, 0)
    loc.setPose(cc.crafted_pose())
    origin, n_window, _ = loc.window()
    win = cc.window_sources(m, origin[0], origin[1], p.submap_dimension)
    assert origin == (0, 0) and n_window == len(win) > 900
    # the plain pose: every boundary to the bit
    cnt, pb = cc.shim_observe(cshim, rec, win, case["maps"], p, cc.crafted_pose(), cp, want, probes=True)
    full = np.zeros(len(rec), dtype=cc.PROBE_DTYPE)
    full[win] = pb
    cc.crafted_expectations(case, full)
    assert all(cnt[k] > 0 for k in TOTALS), cnt
    got = loc.observeFrame(frame, cc.crafted_pose())
    assert got == cnt, (got, cnt)
    ev = loc.evidence()
    assert ev.dtype == EVIDENCE_DTYPE and ev.tobytes() == want.tobytes()
    assert not ev[-8:].view(np.uint32).any()                     # the dropped records stay zero
    # the same observation again: the evidence doubles
    assert loc.observeFrame(frame, cc.crafted_pose()) == cnt
    doubled = loc.evidence()
    for f in EVIDENCE_DTYPE.names:
        assert np.array_equal(doubled[f], 2 * want[f]), f
    cc.shim_observe(cshim, rec, win, case["maps"], p, cc.crafted_pose(), cp, want)
    # a turned pose: the general path on top of it
    T = cc.crafted_pose(turned=True)
    cnt2 = cc.shim_observe(cshim, rec, win, case["maps"], p, T, cp, want)
    assert loc.observeFrame(frame, T) == cnt2 and cnt2["hits"] > 0 and cnt2["unseen"] > cnt["unseen"]
    assert loc.evidence().tobytes() == want.tobytes()
    # the device download equals the host one
    d = torch.zeros(len(rec) * 4 + 8, dtype=torch.int32, device="cuda")
    assert loc.evidenceDevice(d, len(rec)) == len(rec)
    back = d.cpu().numpy().view(np.uint32)
    assert back[:len(rec) * 4].tobytes() == want.tobytes() and not back[len(rec) * 4:].any()
    loc.clearEvidence()
    assert not loc.evidence().view(np.uint32).any()


@pytest.mark.parametrize("n", [0, 1])
def test_tiny_maps(shims, crafted_loc, n):
    """an empty map and a single record: nothing to observe, or one lane"""
    lshim, cshim = shims
    loc, p, cp = crafted_loc, cc.crafted_params(), cc.crafted_change_params()
    rec = np.zeros(n, dtype=WORLD_SURFEL_DTYPE)
    maps = [np.zeros((cc.CH, cc.CW, 4), dtype=np.float32) for _ in range(3)]
    if n:
        rec["x"], rec["y"], rec["z"] = np.float32(8) + np.float32(cc.CRAFT_T[0]), cc.CRAFT_T[1], cc.CRAFT_T[2]
        rec["nx"], rec["label"] = -1.0, 50
        maps[0][:, :], maps[1][:, :] = (12.0, 0.0, 0.0, 1.0), (-1.0, 0.0, 0.0, 1.0)
    assert loc.setMap(rec) == 0
    loc.setPose(cc.crafted_pose())
    got = loc.observeFrame(upload(loc, maps), cc.crafted_pose())
    want = np.zeros(n, dtype=EVIDENCE_DTYPE)
    m = lc.ShimMap(lshim, rec, p.submap_extent)
    cnt = cc.shim_observe(cshim, rec, cc.window_sources(m, 0, 0, p.submap_dimension), maps, p, cc.crafted_pose(), cp, want)
    assert got == cnt and got["n_window"] == n and got["misses"] == n
    ev = loc.evidence()
    assert ev.shape == (n,) and ev.tobytes() == want.tobytes()


# ---- 2, 3. the edited run
def raw_scan(loc, scan):
    """one scan through the C entry: (the result's bytes, the result as a dict)"""
    pts, lab, prob = (np.ascontiguousarray(a, dtype=np.float32) for a in scan)
    res = LocalizerResult()
    loc.ctx.check(loc.L.suma_localizer_process_scan(loc.h, core._ptr(pts), core._ptr(lab), core._ptr(prob), pts.shape[0], 0,
                                                    C.byref(res)), "suma_localizer_process_scan")
    return bytes(res), core.Localizer._result(res)


def model_digest(loc):
    f = loc.modelFrame()
    return hashlib.sha1(b"".join(f.download(k).tobytes() for k in range(3))).hexdigest()


class Edited:
    """scans 0-44 mapped on the GPU once; scans 20-44 of the edited world localised with evidence on and off, and over
    the CPU oracle; each made once and shared"""

    def __init__(self, shims):
        self.lshim, self.cshim = shims
        self.p = lc.loc_params()
        pipe = core.SurfelMapping(self.p)
        self.poses = []
        for s in lc.loc_scans():
            pipe.processScan(*s)
            self.poses.append(pipe.getCurrentPose())
        self.records = pipe.map.export_world()
        pipe.close()
        self.scans = cc.edited_scans()
        self.start = self.poses[cc.FIRST]
        self.cache = {}

    def gpu(self, evidence, loc_params=None, keep=False):
        key = (evidence, loc_params is None)
        if key in self.cache and not keep:
            return self.cache[key]
        loc = core.Localizer(self.p, loc_params)
        if evidence:
            loc.enableEvidence()
        loc.setMap(self.records)
        loc.setPose(self.start)
        out = dict(raw=[], res=[], obs=[], model=[], window=[])
        for s in self.scans:
            raw, res = raw_scan(loc, s)
            out["raw"].append(raw)
            out["res"].append(res)
            out["model"].append(model_digest(loc))
            out["window"].append(hashlib.sha1(loc.downloadWindow().tobytes()).hexdigest() if res["window_rebuilt"] else None)
            if evidence:
                out["obs"].append(loc.lastObservation())
        out["final_window"] = loc.downloadWindow().tobytes()
        if evidence:
            out["evidence"] = loc.evidence()
        if keep:
            return out, loc
        loc.close()
        self.cache[key] = out
        return out

    def host(self):
        if "host" not in self.cache:
            self.cache["host"] = cc.host_run(self.lshim, self.cshim, self.p, self.records, self.start, self.scans)
        return self.cache["host"]


@pytest.fixture(scope="module")
def edited(shims):
    return Edited(shims)


def test_edited_run_equals_the_host_restatement(edited):
    """evidence bytes and every scan's totals against tests/change_host.py over the CPU oracle, and the conditions of
    DESIGN.md 14 on what the default rule prunes"""
    import localize_host as lh
    got = edited.gpu(True)
    h, want = edited.host()
    assert len(got["res"]) == len(want) == cc.LAST - cc.FIRST + 1
    for k, (a, b) in enumerate(zip(got["res"], want)):
        lh.results_equal(a, b, k)
        assert got["obs"][k] == (b["observation"], b["observed"]), (k, got["obs"][k], b["observation"])
        assert got["obs"][k][1] and a["tracked"]
    assert sum(r["window_rebuilt"] for r in got["res"]) >= 1
    ev = got["evidence"]
    assert ev.shape == h.evidence.shape and ev.tobytes() == h.evidence.tobytes()
    bad, worst = lc.tracking_failures([None] * cc.FIRST + [r["pose"] for r in got["res"]], edited.poses, first=cc.FIRST + 1)
    assert not bad, (bad, worst)
    kept, keep = core.pruned_map(edited.records, ev)
    assert np.array_equal(keep, cc.numpy_prune(ev)) and kept.tobytes() == edited.records[keep].tobytes()
    s_in, s_out, n_in = cc.shares(edited.records, keep)
    print("s_in %.6f (%d records inside) s_out %.6f" % (s_in, n_in, s_out))
    assert n_in > 100
    cc.check_shares(s_in, s_out)


def test_evidence_does_not_move_the_localiser(edited):
    """all bytes of every suma_localizer_result, every gathered window and every model frame"""
    on, off = edited.gpu(True), edited.gpu(False)
    for k in range(len(on["raw"])):
        assert on["raw"][k] == off["raw"][k], k
        assert on["model"][k] == off["model"][k] and on["window"][k] == off["window"][k], k
    assert on["final_window"] == off["final_window"]


# ---- 4. bookkeeping
def test_tracked_only(edited):
    """min_valid_ratio = 1.1 passes no scan: nothing is observed; tracked_only = 0 observes all the same"""
    lp = LocalizerParams.defaults(edited.p, min_valid_ratio=1.1)
    loc = core.Localizer(edited.p, lp)
    loc.enableEvidence()
    loc.setMap(edited.records)
    loc.setPose(edited.start)
    for s in edited.scans[:3]:
        r = loc.processScan(*s)
        assert not r["tracked"] and r["n_window"] > 0
        assert loc.lastObservation() == (dict.fromkeys(TOTALS, 0), False)
    assert not loc.evidence().view(np.uint32).any()
    loc.enableEvidence(ChangeParams.defaults(tracked_only=0))   # the parameters change at once, the evidence stays
    loc.setPose(edited.start)
    r = loc.processScan(*edited.scans[0])
    cnt, observed = loc.lastObservation()
    assert not r["tracked"] and observed and cnt["n_window"] == r["n_window"] and cnt["hits"] > 1000
    assert int(loc.evidence()["hits"].sum()) == cnt["hits"]
    loc.close()


def test_clear_set_map_and_refusals(edited):
    loc = core.Localizer(edited.p)
    loc.setMap(edited.records)
    loc.setPose(edited.start)
    for call in (loc.evidence, loc.lastObservation, loc.clearEvidence,
                 lambda: loc.observeFrame(core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H), edited.start)):
        with pytest.raises(core.SumaError, match="no evidence"):
            call()
    with pytest.raises(core.SumaError, match="free_margin"):
        loc.enableEvidence(ChangeParams.defaults(free_margin=0.0))
    with pytest.raises(core.SumaError, match="min_view_cos"):
        loc.enableEvidence(ChangeParams.defaults(min_view_cos=1.0))
    with pytest.raises(core.SumaError, match="max_range"):
        loc.enableEvidence(ChangeParams.defaults(max_range=float("inf")))
    loc.enableEvidence()
    with pytest.raises(core.SumaError, match="no evidence"):   # enabled, but no set_map has followed
        loc.evidence()
    r = loc.processScan(*edited.scans[0])                       # and the scan path does not observe yet
    assert r["tracked"]
    loc.setMap(edited.records)
    loc.setPose(edited.start)
    assert loc.lastObservation() == (dict.fromkeys(TOTALS, 0), False)
    loc.processScan(*edited.scans[0])
    cnt, observed = loc.lastObservation()
    ev = loc.evidence()
    assert observed and int(ev["hits"].sum()) == cnt["hits"] > 1000 and int(ev["misses"].sum()) == cnt["misses"]
    assert int(ev["occluded"].sum()) == cnt["occluded"] and int(ev["label_changes"].sum()) == cnt["label_changes"]
    frame = core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H, handle=None)
    with pytest.raises(core.SumaError, match="non-finite"):
        loc.observeFrame(frame, np.full((4, 4), np.nan))
    with pytest.raises(core.SumaError, match="data image"):
        loc.observeFrame(core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H + 1), edited.start)
    loc.clearEvidence()
    assert not loc.evidence().view(np.uint32).any() and loc.lastObservation()[1] is False
    loc.processScan(*edited.scans[1])
    assert loc.evidence().view(np.uint32).any()
    loc.setMap(edited.records)                                  # a new map clears
    assert not loc.evidence().view(np.uint32).any()
    loc.disableEvidence()
    with pytest.raises(core.SumaError, match="no evidence"):
        loc.evidence()
    loc.close()


def test_a_window_rebuild_keeps_the_evidence(edited):
    """records that leave the window keep what they have collected"""
    got = edited.gpu(True)
    k = next(i for i, r in enumerate(got["res"]) if r["window_rebuilt"])
    loc = core.Localizer(edited.p)
    loc.enableEvidence()
    loc.setMap(edited.records)
    loc.setPose(edited.start)
    for s in edited.scans[:k]:
        loc.processScan(*s)
    before = loc.evidence()
    r = loc.processScan(*edited.scans[k])
    assert r["window_rebuilt"]
    after = loc.evidence()
    for f in EVIDENCE_DTYPE.names:
        assert np.all(after[f] >= before[f]), f
    # the records of the tiles that left: in no span of the new window, and unchanged
    m = lc.ShimMap(edited.lshim, edited.records, edited.p.submap_extent)
    old = set(cc.window_sources(m, *got["res"][k - 1]["origin"], edited.p.submap_dimension).tolist())
    new = set(cc.window_sources(m, *r["origin"], edited.p.submap_dimension).tolist())
    left = np.array(sorted(old - new), dtype=np.int64)
    assert len(left) > 100 and before[left].view(np.uint32).any()
    assert after[left].tobytes() == before[left].tobytes()
    loc.close()


def test_an_empty_window_observes_nothing(edited):
    loc = core.Localizer(edited.p)
    loc.enableEvidence()
    loc.setMap(edited.records)
    far = np.array(edited.start)
    far[0, 3], far[1, 3] = 900.0, -900.0
    loc.setPose(far)
    assert loc.window()[1] == 0
    r = loc.processScan(*edited.scans[0])
    assert r["n_window"] == 0 and loc.lastObservation() == (dict.fromkeys(TOTALS, 0), False)
    f = core.Frame(loc.ctx, lc.LOC_W, lc.LOC_H)
    f.set(*[np.ones((lc.LOC_H, lc.LOC_W, 4), dtype=np.float32)] * 3)
    assert loc.observeFrame(f, far) == dict.fromkeys(TOTALS, 0)
    assert not loc.evidence().view(np.uint32).any() and len(loc.evidence()) == len(edited.records)
    loc.close()
