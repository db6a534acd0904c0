"""The tracks on the MI355X (csrc/k_tracks.hip, suma_localizer_*track*, core.Localizer): live tracks, raw table, per-object
track ids and counts byte for byte against the host restatement (tests/track_shim.c) through trackObjects, on a localiser
with a one-record map: every named case of track_common, random sequences compared after every update, what clears the
tracks, two runs giving the same bytes, the device download, the refusals, and the updates behind segmentFlags and
liveUpdateFlags."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import track_common as tc
from semantic_suma_amd import core
from semantic_suma_amd.types import (NovelParams, OBJECT_TRACK_DTYPE, ObjectParams, TrackCounts, TrackParams,
                                     WORLD_SURFEL_DTYPE, params_with_size)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return tc.build_shim(tmp_path_factory.mktemp("track_gpu"))


def one_record():
    rec = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
    rec["nz"], rec["radius"], rec["confidence"] = 1.0, 0.1, 5.0
    return rec


class GpuTracker:
    """the library's tracker with the interface of track_common.ShimTracker"""

    def __init__(self, loc, tp):
        self.loc, self.tp = loc, tp
        loc.enableTracks(tp)                     # enabling again forgets the tracks

    def clear(self):
        self.loc.clearTracks()

    def set_state(self, slots, last_stamp, next_id):
        self.loc.setTrackState(slots, last_stamp, next_id)
        assert self.loc.tracks() is None

    def update(self, rec, scan_id):
        try:
            cnt = self.loc.trackObjects(rec, scan_id)
        except core.SumaError as e:
            assert "stamp" in str(e), e
            return None
        tracks, again = self.loc.tracks(allow_overflow=True)
        assert again == cnt
        return tracks, self.loc.objectTracks(), cnt

    @property
    def state(self):
        return self.loc.trackState()


@pytest.fixture(scope="module")
def loc():
    l = core.Localizer(params_with_size(70, 3, submap_extent=10.0, submap_dimension=2))
    l.setMap(one_record())
    l.enableNovelty(NovelParams.defaults(max_candidates=1024))
    l.enableObjects(ObjectParams.defaults(max_objects=4096))
    yield l
    l.close()


def same_state(got: GpuTracker, want: tc.ShimTracker, what):
    slots, last, nxt = got.state
    assert slots.tobytes() == want.slots.tobytes(), what
    assert (last, nxt) == (want.last_stamp, want.next_id), what


def play(got, want, steps, what):
    out = []
    for u, st in enumerate(steps):
        a, b = tc.run(got, [st]), tc.run(want, [st])
        if st[0] == "update":
            tc.same(a[0], b[0], (what, u))
            out.append(a[0])
        same_state(got, want, (what, u))
    return out


# ---- 1. every named case, compared after every step
CASES = tc.named_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_named_cases_equal_shim(shim, loc, case):
    name, tp, steps = case
    got = play(GpuTracker(loc, tp), tc.ShimTracker(shim, tp), steps, name)
    for g in got:
        if g is not None:
            tc.check_counts(g[2], tp, len(g[0]))
    if name == "births_exceed_free_slots":
        # the downloads' convention: the outputs are filled, then SUMA_ERR_CAPACITY
        n, cnt, upd = C.c_uint32(0), TrackCounts(), C.c_int32(0)
        out = np.zeros(3, dtype=OBJECT_TRACK_DTYPE)
        rc = loc.L.suma_localizer_tracks(loc.h, core._ptr(out), 3, C.byref(n), C.byref(cnt), C.byref(upd))
        assert rc == -3 and n.value == 3 and cnt.n_dropped == 4 and upd.value == 1 and out.tobytes() == got[-1][0].tobytes()
        with pytest.raises(core.SumaError, match="free slot"):
            loc.tracks()


# ---- 2. random sequences of eight updates
@pytest.mark.parametrize("n_objects", [0, 1, 5, 70, 300])
def test_random_sequences_equal_shim(shim, loc, n_objects):
    for seed in range(3):
        tp, steps = tc.random_sequence(seed + 10 * n_objects, n_objects)
        got = play(GpuTracker(loc, tp), tc.ShimTracker(shim, tp), steps, (n_objects, seed))
        print(n_objects, seed, [g[2] for g in got][-1])


# ---- 3. what forgets the tracks
def test_clear_set_map_and_reenabling_forget_the_tracks(shim, loc):
    tp = TrackParams.defaults(max_tracks=64)
    rec = tc.grid_points(5)
    empty = np.zeros(64, dtype=OBJECT_TRACK_DTYPE).tobytes()

    def fresh(t):
        slots, last, nxt = t.state
        return slots.tobytes() == empty and (last, nxt) == (0, 1) and loc.tracks() is None and len(loc.objectTracks()) == 0

    t = GpuTracker(loc, tp)
    assert fresh(t)
    for forget in (loc.clearTracks, lambda: loc.setMap(one_record()), loc.clearNovelty, lambda: loc.enableTracks(tp)):
        t.update(rec, 7)
        assert not fresh(t) and list(loc.tracks()[0]["id"]) == [1, 2, 3, 4, 5]
        forget()
        assert fresh(t)
        assert t.update(rec, 0)[2]["n_born"] == 5                 # the stamps start again, and the ids
    loc.disableObjects()
    with pytest.raises(core.SumaError, match="tracks are off"):
        loc.tracks()
    loc.enableObjects(ObjectParams.defaults(max_objects=4096))
    with pytest.raises(core.SumaError, match="tracks are off"):
        loc.clearTracks()
    assert fresh(GpuTracker(loc, tp))
    # another max_objects: the tracker's blocks are made again, the tracks forgotten, the parameters kept
    t.update(rec, 0)
    loc.enableObjects(ObjectParams.defaults(max_objects=512))
    assert fresh(t)
    with pytest.raises(core.SumaError, match="max_objects"):
        loc.trackObjects(tc.grid_points(513), 0)
    want = tc.ShimTracker(shim, tp)
    tc.same(t.update(tc.grid_points(512), 0), want.update(tc.grid_points(512), 0), "512")
    loc.enableObjects(ObjectParams.defaults(max_objects=4096))


# ---- 4. two runs, the same bytes
def test_two_runs_give_the_same_bytes(loc):
    tp, steps = tc.random_sequence(3, 300)
    runs = []
    for _ in range(2):
        t = GpuTracker(loc, tp)
        res = tc.run(t, steps)
        runs.append(b"".join(r[0].tobytes() + r[1].tobytes() for r in res if r is not None) + t.state[0].tobytes())
    assert runs[0] == runs[1]


# ---- 5. the device download
def test_device_download(shim, loc):
    tp = TrackParams.defaults(max_tracks=65)
    t, want = GpuTracker(loc, tp), tc.ShimTracker(shim, tp)
    rec = tc.grid_points(40)
    t.update(rec, 0), want.update(rec, 0)
    a, b = t.update(rec[5:], 1), want.update(rec[5:], 1)
    d = torch.zeros(65 * 112 // 4, dtype=torch.int32, device="cuda")
    n, cnt = loc.tracks(out=d)
    torch.cuda.synchronize()
    assert n == 40 and cnt == b[2]
    assert d.cpu().numpy().tobytes()[:40 * 112] == b[0].tobytes() == a[0].tobytes()


# ---- 6. the refusals
def test_refusals(loc):
    tp = TrackParams.defaults(max_tracks=8)
    loc.disableTracks()
    for call in (lambda: loc.trackObjects(tc.grid_points(1), 0), loc.tracks, loc.objectTracks, loc.trackState, loc.clearTracks,
                 lambda: loc.setTrackState(np.zeros(8, dtype=OBJECT_TRACK_DTYPE), 0, 1)):
        with pytest.raises(core.SumaError, match="tracks are off"):
            call()
    loc.disableObjects()
    with pytest.raises(core.SumaError, match="objects are off"):
        loc.enableTracks(tp)
    loc.enableObjects(ObjectParams.defaults(max_objects=4096))
    for bad, what in ((dict(max_tracks=0), "max_tracks"), (dict(max_tracks=4097), "max_tracks"), (dict(max_rounds=65), "max_rounds"),
                      (dict(alpha=1.5), "alpha"), (dict(join_dist=float("nan")), "join_dist"), (dict(confirm_hits=0), "confirm_hits")):
        with pytest.raises(core.SumaError, match=what):
            loc.enableTracks(TrackParams.defaults(**bad))
    with pytest.raises(core.SumaError, match="tracks are off"):
        loc.tracks()
    loc.enableTracks(tp)
    with pytest.raises(core.SumaError, match="max_objects"):
        loc.trackObjects(tc.grid_points(4097), 0)
    with pytest.raises(core.SumaError, match="slots"):
        loc.setTrackState(np.zeros(7, dtype=OBJECT_TRACK_DTYPE), 0, 1)
    bad = tc.table(8, [tc.track_slot(0, 1, (0, 0, 0))])
    for change, stamp, nxt, what in ((dict(state=3), 1, 2, "state"), (dict(id=0), 1, 2, "id"), (dict(id=2), 1, 2, "id"),
                                     (dict(last_matched=2), 1, 2, "stamp"), (dict(first_stamp=2, last_matched=1), 3, 2, "stamp")):
        sl = bad.copy()
        for k, v in change.items():
            sl[k][0] = v
        with pytest.raises(core.SumaError, match=what):
            loc.setTrackState(sl, stamp, nxt)
    with pytest.raises(core.SumaError, match="next_id"):
        loc.setTrackState(np.zeros(8, dtype=OBJECT_TRACK_DTYPE), 0, 0)
    assert loc.trackState()[1:] == (0, 1) and loc.tracks() is None      # nothing was launched or changed
    assert loc.trackObjects(tc.grid_points(2), 4)["n_born"] == 2
    with pytest.raises(core.SumaError, match="stamp"):
        loc.trackObjects(tc.grid_points(2), 4)
    assert loc.tracks()[1]["n_born"] == 2 and loc.trackState()[1:] == (5, 3)


# ---- 7. every segmentation is followed by an update: the primitives on a caller's flag image too
def test_segment_flags_and_live_update_flags_feed_the_tracks(shim, loc):
    import live_common as lv
    import object_common as oc
    W, H = 70, 3
    V, S = oc.loop_frame(W, H)
    frame = core.Frame(loc.ctx, W, H)
    frame.set(V, np.zeros_like(V), S)
    rng = np.random.RandomState(9)
    op = ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=2, max_objects=4096)
    loc.enableObjects(op)
    tp = TrackParams.defaults(max_tracks=64, join_dist=0.125)
    got, want = GpuTracker(loc, tp), tc.ShimTracker(shim, tp)
    gp = lv.grid_params(24, 24, cell_size=0.5, origin=(-4.0, -4.0))
    for k, scan_id in enumerate((3, 4, 9)):
        fl = (rng.rand(H, W) < 0.5).astype(np.uint8)
        if k == 2:
            loc.enableLiveGrid(lv.flat_cells(gp), gp)
            loc.liveUpdateFlags(frame, oc.POSE, fl, scan_id)
        else:
            loc.segmentFlags(frame, oc.POSE, fl, scan_id)
        rec, cnt = loc.objects()
        assert cnt["n_objects"] > 3
        tracks, tcnt = loc.tracks()
        w = want.update(rec, scan_id)
        tc.same((tracks, loc.objectTracks(), tcnt), w, scan_id)
        same_state(got, want, scan_id)
    # a stamp that is not above the last one refuses the whole call: the segmentation stays as it was
    before = loc.objects()[0].tobytes()
    with pytest.raises(core.SumaError, match="stamp"):
        loc.segmentFlags(frame, oc.POSE, np.ones((H, W), dtype=np.uint8), 9)
    assert loc.objects()[0].tobytes() == before and loc.trackState()[1] == 10
    loc.disableLiveGrid()
    loc.enableObjects(ObjectParams.defaults(max_objects=4096))
