"""Per-scan objects on the MI355X (csrc/k_objects.hip, suma_localizer_*objects*, core.Localizer): the six kernels byte
for byte against the host restatement (tests/object_shim.c) -- records, id image, counts -- on crafted frames at the
smallest shapes where they can go wrong, through suma_localizer_segment_flags; DESIGN.md 15's added run with novelty and
objects on, per scan against the shim applied to the library's own flags, frame and pose; and objects on or off does not
move anything else the localiser gives."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import change_common as cc
import localize_common as lc
import novel_common as nc
import object_common as oc
from semantic_suma_amd import core
from semantic_suma_amd.types import (LocalizerResult, NovelParams, ObjectCounts, ObjectParams, SCAN_OBJECT_DTYPE,
                                     WORLD_SURFEL_DTYPE, params_with_size)

pytestmark = pytest.mark.gpu

# W x H: 210 texels (no multiple of the wave), 520 (three blocks of 256), 257 x 1 (H = 1, two blocks), W = 1, W = 2
SHAPES = [(70, 3), (130, 4), (257, 1), (1, 5), (2, 4)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return oc.build_shim(tmp_path_factory.mktemp("object_gpu"))


class Rig:
    """a localiser with a one-record map, novelty and objects on, and one data-sized frame"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.loc = core.Localizer(params_with_size(W, H, submap_extent=10.0, submap_dimension=2))
        rec = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
        rec["nz"], rec["radius"], rec["confidence"] = 1.0, 0.1, 5.0
        self.loc.setMap(rec)
        self.loc.enableNovelty(NovelParams.defaults(max_candidates=1024))
        self.loc.enableObjects()
        self.frame = core.Frame(self.loc.ctx, W, H)

    def segment(self, V, S, flags, pose, op, scan_id, allow_overflow=False):
        """-> (records, ids, counts) as object_common.shim_segment gives them"""
        self.loc.enableObjects(op)
        self.frame.set(V, np.zeros_like(V), S)
        counts = self.loc.segmentFlags(self.frame, pose, flags, scan_id)
        got = self.loc.objects(allow_overflow=allow_overflow)
        assert got is not None and got[1] == counts
        return got[0], self.loc.objectIds(), counts

    def close(self):
        self.loc.close()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = Rig(W, H)
        return made[(W, H)]

    yield get
    for r in made.values():
        r.close()


def same(got, want, what):
    assert got[2] == want[2], (what, got[2], want[2])
    assert got[0].dtype == SCAN_OBJECT_DTYPE and got[0].tobytes() == want[0].tobytes(), (what, got[0], want[0])
    assert got[1].tobytes() == want[1].tobytes(), what
    c = got[2]
    assert c["n_small"] + c["n_objects"] == c["n_components"] and c["stored"] == len(got[0]), (what, c)


# ---- 1. every crafted case at every shape
@pytest.mark.parametrize("W,H", SHAPES)
def test_crafted_frames_equal_shim(shim, rigs, W, H):
    rig = rigs(W, H)
    seen = {}
    for k, (name, V, S, fl, pose, op) in enumerate(oc.crafted_cases(W, H)):
        want = oc.shim_segment(shim, V, S, fl, pose, op, 100 + k)
        got = rig.segment(V, S, fl, pose, op, 100 + k, allow_overflow=True)
        print(W, H, name, want[2])
        same(got, want, (W, H, name))
        seen[name] = want
    P = W * H
    c = seen["all_flags_one_component"][2]
    assert c["n_members"] == P and c["n_components"] == 1 and c["n_objects"] == 1
    assert seen["all_flags_one_component"][0]["n_texels"][0] == P and not seen["all_flags_one_component"][1].any()
    assert seen["all_flags_zero"][2] == dict(oc.ZERO, n_texels=P)
    c = seen["all_flags_no_link"][2]
    assert c["n_components"] == c["n_objects"] == c["stored"] == P
    assert np.array_equal(seen["all_flags_no_link"][1].reshape(-1), np.arange(P))
    c = seen["min_texels_above_image"][2]
    assert c["n_small"] == c["n_components"] == 1 and c["n_objects"] == 0
    assert np.all(seen["min_texels_above_image"][1] == oc.NONE)
    assert seen["pose_overflow"][2] == dict(oc.ZERO, n_texels=P)
    assert seen["around_the_turn"][2]["n_components"] == 1 and seen["across_the_seam"][2]["n_components"] == 1
    box = seen["signed_zero_box"][0]
    if P > 1:        # both zeros are among the members: the box runs from -0 to +0
        assert np.signbit(box["min"][0, 0]) and not np.signbit(box["max"][0, 0]) and box["min"][0, 0] == box["max"][0, 0] == 0
    if H >= 3 and W >= 70:
        assert seen["serpentine"][2]["n_components"] == 1 and seen["spiral"][2]["n_components"] == 1
        assert seen["serpentine"][2]["n_members"] > W and seen["checkerboard"][2]["n_components"] == 1
        c = seen["random_sparse"][2]                       # more objects than max_objects = 3
        assert c["n_objects"] > c["stored"] == 3 and set(np.unique(seen["random_sparse"][1])) == {0, 1, 2, oc.NONE}
        c = seen["flagged_non_members"][2]
        assert c["n_members"] == P - 5 and c["n_components"] == 1


# ---- 2. the link threshold to the ulp, at small and at large range
@pytest.mark.parametrize("near", [True, False])
def test_link_threshold(shim, rigs, near):
    V, S, fl, pose, op = oc.threshold_case(70, 3, near)
    want = oc.shim_segment(shim, V, S, fl, pose, op, 1)
    same(rigs(70, 3).segment(V, S, fl, pose, op, 1), want, near)
    # A and B are one object (their distance is the threshold), C and D two (one ulp more)
    assert want[2]["n_components"] == 3 and list(want[0]["n_texels"]) == [6, 3, 3]


# ---- 3. min_texels - 1, min_texels, min_texels + 1
@pytest.mark.parametrize("min_texels", [1, 5, 9])
def test_min_texels(shim, rigs, min_texels):
    V, S, fl, pose, op = oc.sized_components(70, 3, min_texels)
    want = oc.shim_segment(shim, V, S, fl, pose, op, 2)
    same(rigs(70, 3).segment(V, S, fl, pose, op, 2), want, min_texels)
    assert list(want[0]["n_texels"]) == [min_texels, min_texels + 1]
    assert want[2]["n_small"] == (1 if min_texels > 1 else 0)


# ---- 4. more objects than max_objects
def test_capacity(shim, rigs):
    rig = rigs(130, 4)
    V, S = oc.loop_frame(130, 4)
    op = ObjectParams.defaults(link_base=0.0, link_slope=0.0, min_texels=1, max_objects=7)
    fl = np.ones((4, 130), dtype=np.uint8)
    want = oc.shim_segment(shim, V, S, fl, oc.POSE, op, 9)
    rig.loc.enableObjects(op)
    rig.frame.set(V, np.zeros_like(V), S)
    assert rig.loc.segmentFlags(rig.frame, oc.POSE, fl, 9) == want[2]
    with pytest.raises(core.SumaError, match="did not fit"):
        rig.loc.objects()
    buf = np.zeros(10, dtype=SCAN_OBJECT_DTYPE)
    n, cnt, seg = C.c_uint32(0), ObjectCounts(), C.c_int32(0)
    rc = rig.loc.L.suma_localizer_objects(rig.loc.h, core._ptr(buf), len(buf), C.byref(n), C.byref(cnt), C.byref(seg))
    assert rc == -3 and n.value == 7 and seg.value == 1 and cnt.as_dict() == want[2]           # SUMA_ERR_CAPACITY, filled
    assert buf[:7].tobytes() == want[0].tobytes() and not buf[7:].view(np.uint32).any()
    ids = rig.loc.objectIds()
    assert ids.tobytes() == want[1].tobytes()
    assert np.array_equal(ids.reshape(-1)[:7], np.arange(7)) and np.all(ids.reshape(-1)[7:] == oc.NONE)
    # a capacity below the stored count: the first records
    small = np.zeros(3, dtype=SCAN_OBJECT_DTYPE)
    rig.loc.enableObjects(ObjectParams.defaults(link_base=0.0, link_slope=0.0, min_texels=1))
    rig.loc.segmentFlags(rig.frame, oc.POSE, fl, 9)
    assert rig.loc.L.suma_localizer_objects(rig.loc.h, core._ptr(small), 3, C.byref(n), None, None) == 0
    assert n.value == 520 and small.tobytes() == want[0][:3].tobytes()
    # the device download equals the host one
    d = torch.zeros(520 * 16 + 8, dtype=torch.int32, device="cuda")
    assert rig.loc.L.suma_localizer_objects_device(rig.loc.h, core._dev(d), 520, C.byref(n), None, None) == 0
    back = d.cpu().numpy().view(np.uint32)
    assert back[:520 * 16].tobytes() == rig.loc.objects()[0].tobytes() and not back[520 * 16:].any()


# ---- 5. repeats and changing content on one context
def test_repeats_on_one_context(shim, rigs):
    rig = rigs(130, 4)
    cases = oc.crafted_cases(130, 4)
    first = {}
    for rnd in range(2):
        for k in (3, 0, 6, 1, 2, 5, 0):
            name, V, S, fl, pose, op = cases[k]
            got = rig.segment(V, S, fl, pose, op, k, allow_overflow=True)
            if k not in first:
                first[k] = got
                same(got, oc.shim_segment(shim, V, S, fl, pose, op, k), name)
            same(got, first[k], (rnd, name))
    # what does not segment leaves nothing behind: a new map, and clearNovelty
    rig.loc.clearNovelty()
    assert rig.loc.objects() is None and rig.loc.objectIds() is None
    name, V, S, fl, pose, op = cases[0]
    rig.segment(V, S, fl, pose, op, 0)
    rec = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
    rec["nz"], rec["radius"] = 1.0, 0.1
    rig.loc.setMap(rec)
    assert rig.loc.objects() is None


# ---- 6. the geometry the localiser runs: 2048 x 64, one component
def test_full_size_single_component(shim):
    W, H = 2048, 64
    rig = Rig(W, H)
    V, S = oc.loop_frame(W, H)
    fl = np.ones((H, W), dtype=np.uint8)
    want = oc.shim_segment(shim, V, S, fl, oc.POSE, oc.LINK, 5)
    same(rig.segment(V, S, fl, oc.POSE, oc.LINK, 5), want, "full size")
    assert want[2]["n_components"] == 1 and want[0]["n_texels"][0] == W * H
    fl = oc.serpentine(W, H)
    want = oc.shim_segment(shim, V, S, fl, oc.POSE, oc.LINK, 6)
    same(rig.segment(V, S, fl, oc.POSE, oc.LINK, 6), want, "full size serpentine")
    assert want[2]["n_components"] == 1
    rig.close()


def test_refusals(rigs):
    rig = rigs(70, 3)
    loc = rig.loc
    for bad, what in ((dict(link_base=-0.1), "link_base"), (dict(link_base=float("nan")), "link_base"),
                      (dict(link_slope=float("inf")), "link_slope"), (dict(min_texels=0), "min_texels"),
                      (dict(max_objects=0), "max_objects"), (dict(max_objects=65537), "max_objects")):
        with pytest.raises(core.SumaError, match=what):
            loc.enableObjects(ObjectParams.defaults(**bad))
    fl = np.ones((3, 70), dtype=np.uint8)
    with pytest.raises(core.SumaError, match="non-finite"):
        loc.segmentFlags(rig.frame, np.full((4, 4), np.nan), fl, 0)
    with pytest.raises(core.SumaError, match="data image"):
        loc.segmentFlags(core.Frame(loc.ctx, 70, 4), np.eye(4), fl, 0)
    other = core.Localizer(params_with_size(70, 3, submap_extent=10.0, submap_dimension=2))
    with pytest.raises(core.SumaError, match="novelty is off"):
        other.enableObjects()
    other.enableNovelty(NovelParams.defaults(max_candidates=64))
    with pytest.raises(core.SumaError, match="objects are off"):
        other.objects()
    other.enableObjects()
    assert other.objects() is None
    other.disableNovelty()                                   # takes the objects with it
    with pytest.raises(core.SumaError, match="objects are off"):
        other.objects()
    other.close()


# ---- 7, 8. the scenario: DESIGN.md 15's added run at 360 x 32 over 25 scans
def raw_scan(loc, scan):
    pts, lab, prob = (np.ascontiguousarray(a, dtype=np.float32) for a in scan)
    res = LocalizerResult()
    loc.ctx.check(loc.L.suma_localizer_process_scan(loc.h, core._ptr(pts), core._ptr(lab), core._ptr(prob), pts.shape[0], 0,
                                                    C.byref(res)), "suma_localizer_process_scan")
    return bytes(res), core.Localizer._result(res)


class Scenario:
    """scans 0-44 of the world without the two boxes (and of the full world, the control) mapped on the GPU once; scans
    20-44 of the full world localised with objects on and off"""

    def __init__(self):
        self.p = lc.loc_params()
        self.scans = nc.localise_scans()
        self.cache = {}

    def mapped(self, without):
        from semantic_suma_amd import synth
        key = ("map", tuple(without))
        if key not in self.cache:
            pipe = core.SurfelMapping(self.p)
            poses = []
            for k in range(lc.LOC_SCANS):
                pipe.processScan(*synth.generate_scan(k, lc.LOC_W, lc.LOC_H, without=without)[:3])
                poses.append(pipe.getCurrentPose())
            self.cache[key] = (poses, pipe.map.export_world())
            pipe.close()
        return self.cache[key]

    def run(self, objects, evidence, without=nc.ADDED):
        key = (objects, evidence, tuple(without))
        if key in self.cache:
            return self.cache[key]
        poses, records = self.mapped(without)
        loc = core.Localizer(self.p)
        if evidence:
            loc.enableEvidence()
        loc.enableNovelty()
        if objects:
            loc.enableObjects()
        loc.setMap(records)
        loc.setPose(poses[nc.FIRST])
        out = dict(raw=[], res=[], col=[], model=[], window=[], obj=[])
        for s in self.scans:
            raw, res = raw_scan(loc, s)
            out["raw"].append(raw)
            out["res"].append(res)
            f = loc.modelFrame()
            out["model"].append(hashlib.sha1(b"".join(f.download(k).tobytes() for k in range(3))).hexdigest())
            out["window"].append(hashlib.sha1(loc.downloadWindow().tobytes()).hexdigest() if res["window_rebuilt"] else None)
            out["col"].append(loc.lastCollection())
            if objects:
                sf = loc.scanFrame()
                out["obj"].append((loc.objects(), loc.objectIds(), loc.novelFlags(), sf.download(0), sf.download(2)))
        out["final_window"] = loc.downloadWindow().tobytes()
        out["candidates"] = loc.novelCandidates().tobytes()
        if evidence:
            out["evidence"] = loc.evidence().tobytes()
        loc.close()
        self.cache[key] = out
        return out


@pytest.fixture(scope="module")
def scenario():
    return Scenario()


def test_in_loop_objects_equal_shim(shim, scenario):
    """per scan objects() and objectIds() against the shim applied to the library's own flags, frame and pose; the
    conditions of DESIGN.md 19 on the added run and on the control"""
    got = scenario.run(True, False)
    hits, shares = 0, []
    for k, (res, (obj, ids, flags, V, S)) in enumerate(zip(got["res"], got["obj"])):
        assert res["tracked"] and got["col"][k][1] and obj is not None, k
        assert int(flags.sum()) == got["col"][k][0]["novel"], k
        want = oc.shim_segment(shim, V, S, flags, res["pose"], None, k)
        same((obj[0], ids, obj[1]), want, k)
        assert np.all(obj[0]["scan_id"] == k) and obj[1]["n_members"] == got["col"][k][0]["novel"]
        hit, share = oc.scan_measure(obj[0], ids, V, flags, res["pose"])
        hits += bool(hit)
        if hit:
            shares.append(share)
    control = scenario.run(True, False, without=())
    per_scan = [o[0][1]["n_objects"] for o in control["obj"]]
    print("scans with the building %d, smallest share %.6f, control objects per scan %s" %
          (hits, min(shares) if shares else -1.0, per_scan))
    oc.check_measured(hits, min(shares) if shares else 0.0, max(per_scan))


def test_objects_do_not_move_the_localiser(scenario):
    """every byte of every suma_localizer_result, every gathered window, every model frame, the counts of every
    collection, the candidates and -- with evidence on -- every evidence word"""
    for evidence in (False, True):
        on, off = scenario.run(True, evidence), scenario.run(False, evidence)
        for k in range(len(on["raw"])):
            assert on["raw"][k] == off["raw"][k], (evidence, k)
            assert on["model"][k] == off["model"][k] and on["window"][k] == off["window"][k], (evidence, k)
            assert on["col"][k] == off["col"][k], (evidence, k)
        assert on["final_window"] == off["final_window"] and on["candidates"] == off["candidates"]
        if evidence:
            assert on["evidence"] == off["evidence"]
    assert sum(r["window_rebuilt"] for r in scenario.run(True, False)["res"]) >= 1
