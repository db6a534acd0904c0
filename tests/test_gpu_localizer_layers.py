"""The chain behind a flag image on the MI355X (csrc/suma_localize.hip: segmentation, tracker update, live update) as its
three entries run it -- collectFrame behind its own collection, liveUpdateFlags and segmentFlags on a caller's flags --, on
a localiser with a one-record map: a stamp that one layer refuses leaves every layer as it was, the three entries leave the
same bytes in every layer they share, and a download reports its total and writes min(total, capacity) records."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import live_common as lv
import object_common as oc
import track_common as tc
from semantic_suma_amd import core
from semantic_suma_amd.types import (NovelParams, OBJECT_TRACK_DTYPE, ObjectCounts, ObjectParams, SCAN_OBJECT_DTYPE,
                                     TrackCounts, TrackParams, WORLD_SURFEL_DTYPE, params_with_size)

pytestmark = pytest.mark.gpu

W, H = 70, 3
GP = lv.grid_params(24, 24, cell_size=0.5, origin=(-4.0, -4.0))
OP = ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=2, max_objects=4096)
TP = TrackParams.defaults(max_tracks=64, join_dist=0.125)


def make_localizer():
    """novelty, objects, tracks and the live layer on, a window of the one record around oc.POSE, and the frame"""
    loc = core.Localizer(params_with_size(W, H, submap_extent=10.0, submap_dimension=2))
    rec = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
    rec["nz"], rec["radius"], rec["confidence"] = 1.0, 0.1, 5.0
    loc.setMap(rec)
    loc.enableNovelty(NovelParams.defaults(max_candidates=1024))
    loc.enableObjects(OP)
    loc.enableTracks(TP)
    loc.enableLiveGrid(lv.flat_cells(GP), GP)
    loc.setPose(oc.POSE)
    V, S = oc.loop_frame(W, H)
    N = np.ones_like(V)                                # normals towards the sensor: a collection takes every texel as novel
    N[..., :3] = -V[..., :3] / np.linalg.norm(V[..., :3], axis=-1, keepdims=True)
    frame = core.Frame(loc.ctx, W, H)
    frame.set(V, N, S)
    return loc, frame


def flag_image():
    return (np.random.RandomState(9).rand(H, W) < 0.5).astype(np.uint8)


def layers(loc):
    """the bytes of everything a refused call must leave alone"""
    obj = loc.objects()
    return dict(live=loc.liveState().tobytes(), live_counts=loc.liveCounts(),
                objects=None if obj is None else (obj[0].tobytes(), obj[1]),
                candidates=loc.novelCandidates().tobytes(), tracks=(loc.trackState()[0].tobytes(),) + loc.trackState()[1:])


# ---- 1. mixed stamps: one layer's refusal is the whole call's
def test_a_stamp_the_tracker_refuses_leaves_every_layer_alone():
    loc, frame = make_localizer()
    try:
        assert loc.trackObjects(tc.grid_points(2), 7)["n_born"] == 2           # the tracker's stamp alone: 8
        before = layers(loc)
        assert before["live_counts"] is None and before["objects"] is None and before["tracks"][1] == 8
        with pytest.raises(core.SumaError, match="stamp"):
            loc.liveUpdateFlags(frame, oc.POSE, flag_image(), 5)
        with pytest.raises(core.SumaError, match="stamp"):
            loc.collectFrame(frame, oc.POSE, 5)
        assert layers(loc) == before
    finally:
        loc.close()


def test_a_stamp_the_live_layer_refuses_does_not_concern_segment_flags():
    loc, frame = make_localizer()
    try:
        loc.setLiveState(loc.liveState(), last_stamp=8)                        # the live layer's stamp alone
        before = layers(loc)
        with pytest.raises(core.SumaError, match="stamp"):
            loc.liveUpdateFlags(frame, oc.POSE, flag_image(), 5)
        assert layers(loc) == before
        cnt = loc.segmentFlags(frame, oc.POSE, flag_image(), 5)
        assert cnt["n_objects"] > 3 and loc.trackState()[1] == 6
        after = layers(loc)
        assert after["live"] == before["live"] and after["live_counts"] is None
    finally:
        loc.close()


# ---- 2. the three entries run one chain
def shared(loc):
    rec, cnt = loc.objects()
    tracks, tcnt = loc.tracks()
    return dict(objects=rec.tobytes(), counts=cnt, ids=loc.objectIds().tobytes(), tracks=tracks.tobytes(), track_counts=tcnt,
                object_tracks=loc.objectTracks().tobytes(), table=loc.trackState()[0].tobytes(), stamps=loc.trackState()[1:])


def test_the_three_entries_leave_the_same_bytes():
    s = 4
    a, frame_a = make_localizer()
    b, frame_b = make_localizer()
    c, frame_c = make_localizer()
    try:
        untouched = c.liveState().tobytes()
        a.collectFrame(frame_a, oc.POSE, s)
        flags = a.novelFlags()
        want = shared(a)
        assert flags.any() and want["counts"]["n_objects"] > 0 and len(want["tracks"]) > 0   # the chain had work to do
        b.liveUpdateFlags(frame_b, oc.POSE, flags, s)
        assert shared(b) == want
        assert b.liveState().tobytes() == a.liveState().tobytes()
        assert b.liveCounts() == a.liveCounts() and a.liveCounts() is not None
        c.segmentFlags(frame_c, oc.POSE, flags, s)
        assert shared(c) == want
        assert c.liveState().tobytes() == untouched and c.liveCounts() is None
    finally:
        for l in (a, b, c):
            l.close()


# ---- 3. a download: *n is the total, min(n, capacity) records are written
def test_downloads_below_at_and_above_n():
    loc, frame = make_localizer()
    try:
        loc.segmentFlags(frame, oc.POSE, flag_image(), 0)
        rec, tracks = loc.objects()[0], loc.tracks()[0]
        assert len(rec) > 3 and len(tracks) > 3
        for total, dtype in ((len(rec), SCAN_OBJECT_DTYPE), (len(tracks), OBJECT_TRACK_DTYPE)):
            for capacity in (0, 1, total - 1, total, total + 2):
                n = C.c_uint32(0xdead)
                if dtype is SCAN_OBJECT_DTYPE:                                 # a host entry
                    out = np.full((total + 3) * dtype.itemsize, 0xa5, dtype=np.uint8)
                    cnt, flag = ObjectCounts(), C.c_int32(0)
                    rc = loc.L.suma_localizer_objects(loc.h, core._ptr(out), capacity, C.byref(n), C.byref(cnt), C.byref(flag))
                    got, want = out.tobytes(), rec.tobytes()
                    assert cnt.as_dict() == loc.objects()[1]
                else:                                                          # a _device entry
                    d = torch.full(((total + 3) * dtype.itemsize,), 0xa5, dtype=torch.uint8, device="cuda")
                    cnt, flag = TrackCounts(), C.c_int32(0)
                    rc = loc.L.suma_localizer_tracks_device(loc.h, core._dev(d), capacity, C.byref(n), C.byref(cnt),
                                                            C.byref(flag))
                    torch.cuda.synchronize()
                    got, want = d.cpu().numpy().tobytes(), tracks.tobytes()
                    assert cnt.as_dict() == loc.tracks()[1]
                m = min(total, capacity) * dtype.itemsize
                assert rc == 0 and n.value == total and flag.value == 1, (dtype, capacity)
                assert got[:m] == want[:m] and got[m:] == b"\xa5" * (len(got) - m), (dtype, capacity)
    finally:
        loc.close()
