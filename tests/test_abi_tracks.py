"""C-ABI checks of the tracks that need no GPU: the header's new symbols are exported and bound, the ctypes mirrors, the
numpy record and the shim's own structures have the C layouts (the track record: a multiple of 16 bytes, at most 128),
every earlier structure keeps its size, the defaults are as the header states, each parameter just outside its range is
refused with a message by the rule suma_localizer_enable_tracks applies, and NULL handles are refused before any device
exists.  (That enabling refuses a localiser whose objects are off needs a localiser, hence a device:
test_gpu_tracks.py::test_refusals.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_track_params_default", "suma_track_params_check", "suma_localizer_enable_tracks", "suma_localizer_disable_tracks",
       "suma_localizer_clear_tracks", "suma_localizer_tracks", "suma_localizer_tracks_device", "suma_localizer_object_tracks",
       "suma_localizer_track_objects", "suma_localizer_track_state", "suma_localizer_set_track_state"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from semantic_suma_amd import core
    return core


def test_new_symbols_are_declared_and_exported(built):
    L = C.CDLL(built.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "suma_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(L, name), name
        assert hasattr(built.lib(), name) and getattr(built.lib(), name).argtypes is not None, name
    for m in ("enableTracks", "disableTracks", "clearTracks", "tracks", "objectTracks", "trackObjects", "trackState", "setTrackState"):
        assert hasattr(built.Localizer, m), m
    from semantic_suma_amd import types as T
    for t in ("TrackParams", "ObjectTrack", "TrackCounts"):
        assert hasattr(T, t), t
    adapter = open(os.path.join(ROOT, "include", "suma_adapter.hpp")).read()
    for m in ("enableTracks(", "tracks(", "objectTracks("):
        assert m in adapter, m


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd import types as T
    structs = {"suma_track_params": T.TrackParams, "suma_track_counts": T.TrackCounts}
    body = []
    for cname, S in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in S._fields_]
    body.append('printf("%zu\\n", sizeof(suma_object_track));')
    body += [f'printf("%zu\\n", offsetof(suma_object_track, {f}));' for f in T.OBJECT_TRACK_DTYPE.names]
    # the structures every earlier entry uses keep their sizes
    earlier = {"suma_params": T.SumaParams, "suma_localizer_params": T.LocalizerParams, "suma_localizer_result": T.LocalizerResult,
               "suma_world_surfel": T.WORLD_SURFEL_DTYPE, "suma_novel_params": T.NovelParams, "suma_novel_counts": T.NovelCounts,
               "suma_novel_fuse_params": T.NovelFuseParams, "suma_novel_stats": T.NovelStats,
               "suma_object_params": T.ObjectParams, "suma_object_counts": T.ObjectCounts, "suma_scan_object": T.SCAN_OBJECT_DTYPE,
               "suma_live_params": T.LiveParams, "suma_live_counts": T.LiveCounts, "suma_live_stats": T.LiveStats,
               "suma_live_cell": T.LIVE_CELL_DTYPE,
               "suma_grid_params": T.GridParams, "suma_grid_cell": T.GRID_CELL_DTYPE, "suma_grid_stats": T.GridStats,
               "suma_plan_params": T.PlanParams, "suma_plan_cell": T.PLAN_CELL_DTYPE, "suma_plan_stats": T.PlanStats,
               "suma_change_params": T.ChangeParams, "suma_change_counts": T.ChangeCounts, "suma_change_evidence": T.EVIDENCE_DTYPE,
               "suma_place_params": T.PlaceParams, "suma_deskew_params": T.DeskewParams, "suma_world_params": T.WorldParams}
    body += [f'printf("%zu\\n", sizeof({c}));' for c in earlier]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for S in structs.values():
        want += [C.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_]
    D = T.OBJECT_TRACK_DTYPE
    want += [D.itemsize] + [D.fields[f][1] for f in D.names]
    want += [S.itemsize if hasattr(S, "itemsize") else C.sizeof(S) for S in earlier.values()]
    assert v == want
    assert C.sizeof(T.TrackParams) == 36 and C.sizeof(T.TrackCounts) == 48
    assert D.itemsize == 112 and D.itemsize % 16 == 0 and D.itemsize <= 128
    assert D.names == ("id", "slot", "state", "label", "n_texels", "n_dynamic", "n_objects", "hits", "missed", "first_stamp",
                       "last_matched", "position", "velocity", "origin", "min", "max", "r_min", "detection")
    assert T.TRACK_COUNTS == ("n_objects", "n_detections", "n_joined", "n_tracks_before", "n_matched", "n_missed", "n_expired",
                              "n_born", "n_dropped", "n_confirmed", "n_unresolved", "rounds")
    # what the earlier sizes were before the tracks existed
    assert (T.GRID_CELL_DTYPE.itemsize, T.SCAN_OBJECT_DTYPE.itemsize, C.sizeof(T.ObjectParams), C.sizeof(T.ObjectCounts),
            T.PLAN_CELL_DTYPE.itemsize, T.WORLD_SURFEL_DTYPE.itemsize, C.sizeof(T.NovelParams), C.sizeof(T.LiveParams),
            C.sizeof(T.LiveCounts), T.LIVE_CELL_DTYPE.itemsize) == (48, 64, 16, 24, 8, 48, 16, 16, 40, 16)


def test_shim_structures_match_c(built, tmp_path):
    """tests/track_shim.c declares the structures again: its copies have the header's layouts, and the shim as compiled
    for the tests reports the same sizes"""
    from semantic_suma_amd.types import OBJECT_TRACK_DTYPE, SCAN_OBJECT_DTYPE, TRACK_COUNTS, TrackParams
    import track_common as tc
    shim = open(os.path.join(ROOT, "tests", "track_shim.c")).read()
    decls = shim[shim.index("typedef struct"):shim.index("} tcounts_t;") + len("} tcounts_t;")]
    pairs = [("tobject_t", "suma_scan_object", list(SCAN_OBJECT_DTYPE.names)),
             ("tparams_t", "suma_track_params", [f for f, _ in TrackParams._fields_]),
             ("ttrack_t", "suma_object_track", list(OBJECT_TRACK_DTYPE.names)),
             ("tcounts_t", "suma_track_counts", list(TRACK_COUNTS))]
    checks = []
    for a, b, fields in pairs:
        checks.append(f"ok &= sizeof({a}) == sizeof({b});")
        checks += [f"ok &= offsetof({a}, {f}) == offsetof({b}, {f});" for f in fields]
    src = tmp_path / "shim_sz.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "suma_hip.h"\n' + decls +
                   "\nint main(){int ok = 1;" + "".join(checks) + "return ok ? 0 : 1;}\n")
    exe = tmp_path / "shim_sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
    L = tc.build_shim(tmp_path)
    assert (L.track_shim_sizeof_object(), L.track_shim_sizeof_params(), L.track_shim_sizeof_track(),
            L.track_shim_sizeof_counts()) == (64, 36, 112, 48)


def test_defaults(built):
    from semantic_suma_amd.types import TrackParams
    L = built.lib()
    q = TrackParams(9.0, 9.0, 9.0, 9.0, 9.0, 7, 7, 7, 7)
    L.suma_track_params_default(C.byref(q))
    got = (q.join_dist, q.gate_base, q.gate_speed, q.alpha, q.beta, q.confirm_hits, q.max_missed, q.max_tracks, q.max_rounds)
    assert got == (2.0, 1.5, 0.5, 0.5, float(np.float32(0.2)), 3, 3, 1024, 16)
    assert bytes(q) == bytes(TrackParams.defaults())
    L.suma_track_params_default(None)
    assert TrackParams.defaults(max_tracks=9).max_tracks == 9
    with pytest.raises(KeyError):
        TrackParams.defaults(no_such_field=1)


def test_refusals_without_a_device(built):
    """nothing here reaches a device: a NULL localiser"""
    L = built.lib()
    n = C.c_uint32(7)
    assert L.suma_localizer_enable_tracks(None, None) == -1 and L.suma_localizer_disable_tracks(None) == -1
    assert L.suma_localizer_clear_tracks(None) == -1
    assert L.suma_localizer_tracks(None, None, 0, C.byref(n), None, None) == -1 and n.value == 7
    assert L.suma_localizer_tracks_device(None, None, 0, C.byref(n), None, None) == -1
    assert L.suma_localizer_object_tracks(None, None, 0, C.byref(n)) == -1
    assert L.suma_localizer_track_objects(None, None, 0, 0, None) == -1
    assert L.suma_localizer_track_state(None, None, 0, C.byref(n), None, None) == -1 and n.value == 7
    assert L.suma_localizer_set_track_state(None, None, 0, 0, 1) == -1


def test_out_of_range_parameters_are_refused_with_a_message(built):
    from semantic_suma_amd.types import TrackParams
    L = built.lib()
    L.suma_last_error.restype = C.c_char_p
    up = float(np.nextafter(np.float32(1e6), np.float32(np.inf)))
    assert L.suma_track_params_check(C.byref(TrackParams.defaults())) == 0
    for ok in (dict(join_dist=-1.0), dict(join_dist=0.0), dict(join_dist=1e6), dict(join_dist=float("-inf")), dict(gate_base=0.0),
               dict(gate_base=1e6), dict(gate_speed=0.0), dict(gate_speed=1e6), dict(alpha=0.0), dict(alpha=1.0), dict(beta=0.0),
               dict(beta=2.0), dict(confirm_hits=1), dict(confirm_hits=65535), dict(max_missed=0), dict(max_missed=65535),
               dict(max_tracks=1), dict(max_tracks=4096), dict(max_rounds=1), dict(max_rounds=64)):
        assert L.suma_track_params_check(C.byref(TrackParams.defaults(**ok))) == 0, ok
    below0 = float(np.nextafter(np.float32(0.0), np.float32(-1.0)))
    for bad, what in ((dict(join_dist=float("nan")), "join_dist"), (dict(join_dist=up), "join_dist"),
                      (dict(gate_base=below0), "gate_base"), (dict(gate_base=up), "gate_base"), (dict(gate_base=float("nan")), "gate_base"),
                      (dict(gate_speed=below0), "gate_speed"), (dict(gate_speed=up), "gate_speed"), (dict(gate_speed=float("inf")), "gate_speed"),
                      (dict(alpha=below0), "alpha"), (dict(alpha=float(np.nextafter(np.float32(1.0), np.float32(2.0)))), "alpha"),
                      (dict(alpha=float("nan")), "alpha"),
                      (dict(beta=below0), "beta"), (dict(beta=float(np.nextafter(np.float32(2.0), np.float32(3.0)))), "beta"),
                      (dict(beta=float("nan")), "beta"),
                      (dict(confirm_hits=0), "confirm_hits"), (dict(confirm_hits=65536), "confirm_hits"),
                      (dict(max_missed=65536), "max_missed"), (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=4097), "max_tracks"),
                      (dict(max_rounds=0), "max_rounds"), (dict(max_rounds=65), "max_rounds")):
        assert L.suma_track_params_check(C.byref(TrackParams.defaults(**bad))) == -1, bad
        assert what in L.suma_last_error(None).decode(), (bad, L.suma_last_error(None))
    assert L.suma_track_params_check(None) == -1
