"""The tracks of suma_hip::Localizer (include/suma_adapter.hpp) in a C++ host on the MI355X: tests/cpp/tracks_driver.cpp
plays a random sequence through trackObjects and must print, per update, the counts, the number of live tracks and the
digests of the tracks and of the per-object track ids that the host restatement (tests/track_shim.c) and core.Localizer
give."""
import os
import struct
import subprocess

import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import track_common as tc
from semantic_suma_amd import core
from semantic_suma_amd.types import NovelParams, TRACK_COUNTS, TrackParams, params_with_size
from test_gpu_cpp import ROOT, build

pytestmark = pytest.mark.gpu


def fnv(data: bytes) -> int:
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def lines(res):
    tracks, ot, cnt = res[:3]
    return [" ".join(str(cnt[k]) for k in TRACK_COUNTS), "%d %016x %016x" % (len(tracks), fnv(tracks.tobytes()), fnv(ot.tobytes()))]


def test_cpp_adapter_tracks(tmp_path):
    exe = build(core, str(tmp_path), os.path.join(ROOT, "tests", "cpp", "tracks_driver.cpp"), "c++")
    shim = tc.build_shim(tmp_path)
    _, steps = tc.random_sequence(2, 70)
    updates = [s for s in steps if s[0] == "update"]
    tp = TrackParams.defaults(max_tracks=256, join_dist=0.25, max_missed=2)
    with open(str(tmp_path / "updates.bin"), "wb") as f:
        for _, rec, scan_id in updates:
            f.write(struct.pack("<II", scan_id, len(rec)) + rec.tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "updates.bin"), "256", "0.25", "2"], timeout=120).decode().strip().splitlines()
    want = tc.ShimTracker(shim, tp)
    expect = []
    for _, rec, scan_id in updates:
        expect += lines(want.update(rec, scan_id))
    want.clear()
    expect += lines(want.update(updates[0][1], updates[0][2]))
    assert want.slots["state"].any() and len(expect) == 18
    assert out == expect, (out, expect)
    # and Python gives the same
    loc = core.Localizer(params_with_size(70, 3))
    loc.enableNovelty(NovelParams.defaults(max_candidates=1024))
    loc.enableObjects()
    loc.enableTracks(tp)
    got = []
    for _, rec, scan_id in updates:
        cnt = loc.trackObjects(rec, scan_id)
        got += lines((loc.tracks(allow_overflow=True)[0], loc.objectTracks(), cnt))
    assert got == expect[:16]
    assert [t.id for t in loc.trackList(confirmed_only=False)] == [int(i) for i in loc.tracks(allow_overflow=True)[0]["id"]]
    loc.close()
