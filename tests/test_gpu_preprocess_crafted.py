"""K1 .. K3 (k_preprocess.hip) and the vertex-map filters (k_filters.hip) on the crafted scans of
tests/test_preprocess_crafted_host.py: every room scene, every small size and every row through Preprocessing.process and
through the device-resident entry (suma_preprocess_device), the three frame maps compared bit for bit with the oracle AND
-- whatever fp64 decides -- directly with the fp64 statement of tests/preprocess_ref.py under the host file's
assertions.  The host file proves on the CPU that the oracle meets the same bounds and that every row's property holds.
Repeats on one context give the same bits: a second call on the same frame, and a filter set switched on and off between."""
import numpy as np
import pytest

import test_preprocess_crafted_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


def maps(frame):
    return tuple(frame.download(m) for m in range(3))


def process(hip, ctx, sc, frame=None):
    p = sc["params"]
    frame = frame or hip.Frame(ctx, p.data_width, p.data_height)
    hip.Preprocessing(ctx).process(sc["pts"], frame, sc["labels"], sc["probs"], sc["timestamp"])
    return frame


def process_device(hip, ctx, sc):
    """the same scan from device-resident arrays"""
    p = sc["params"]
    frame = hip.Frame(ctx, p.data_width, p.data_height)
    n = sc["pts"].shape[0]
    held = [ctx.device_array(a) if a is not None and a.size else None for a in (sc["pts"], sc["labels"], sc["probs"])]
    try:
        ctx.check(ctx.L.suma_preprocess_device(ctx.h, held[0], held[1], held[2], n, sc["timestamp"], frame.h),
                  "suma_preprocess_device")
        return maps(frame)
    finally:
        for d in held:
            if d is not None:
                ctx.device_free(d)


_RESULTS = {}


def hip_results(hip, sid):
    """the kernel's maps of a scene, computed once and shared; the second call on the same frame and the
    device-resident entry must give the same bits"""
    if sid not in _RESULTS:
        sc = H.get_scene(sid)
        ctx = hip.Context(sc["params"])
        frame = process(hip, ctx, sc)
        got = maps(frame)
        H.assert_frames_equal(maps(process(hip, ctx, sc, frame)), got, f"{sid}: second call on the same frame")
        H.assert_frames_equal(process_device(hip, ctx, sc), got, f"{sid}: device-resident entry")
        _RESULTS[sid] = got
    return _RESULTS[sid]


@pytest.mark.parametrize("sid", H.ROOM_IDS)
def test_room_scene(hip, oracle_lib, sid):
    got = hip_results(hip, sid)
    fig = H.check_frame(sid, got, f"kernel {sid}")
    print(H._fmt(sid, fig))
    H.assert_frames_equal(got, H.oracle_results(sid), sid)


@pytest.mark.parametrize("sid", H.SMALL_IDS)
def test_small_sizes(hip, oracle_lib, sid):
    """widths 3 .. 23: below tile + halo of K2 + K3, the staging loop wraps a column many times; below 13 columns K1c's
    window revisits columns, as the shader's does"""
    got = hip_results(hip, sid)
    H.check_frame(sid, got, f"kernel {sid}", caps=False)
    H.assert_frames_equal(got, H.oracle_results(sid), sid)


@pytest.mark.parametrize("sid", H.ROW_IDS)
def test_row(hip, oracle_lib, sid):
    got = hip_results(hip, sid)
    H.assert_frames_equal(got, H.oracle_results(sid), sid)
    H.run_rows_property(sid, got)
    H.check_frame(sid, got, f"kernel {sid}", caps=False)


@pytest.mark.parametrize("size", H.ROOM_SIZES + H.SMALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filters_switched_on_one_context(hip, oracle_lib, size):
    """one context, the parameter sets in turn with the plain set between: each result equals the fresh context's (which
    equals the oracle's); the filters' scratch buffers and the z-buffer carry nothing over"""
    W, Hh = size
    ctx = hip.Context(H.params(W, Hh))
    order = ["quirk", "filter4", "quirk", "filter1", "filter2", "quirk", "filter0", "filter3", "offset0", "filter5", "quirk"]
    for v in order:
        sid = H.scene_id(W, Hh, v, 12)
        sc = H.get_scene(sid)
        ctx.set_params(sc["params"])
        H.assert_frames_equal(maps(process(hip, ctx, sc)), H.oracle_results(sid), f"{sid} on a live context")
