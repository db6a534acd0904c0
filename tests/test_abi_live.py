"""C-ABI checks of the live obstacle layer that need no GPU: the header's new symbols are exported and bound, the ctypes
mirrors, the numpy record and the shim's own structures have the C layouts, every earlier structure keeps its size, the
defaults are as the header states, out-of-range parameters are refused with a message by the rule
suma_localizer_enable_live_grid applies, and NULL handles are refused before any device exists.  (That enabling refuses a
localiser whose novelty is off needs a localiser, hence a device: test_gpu_live.py::test_refusals.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_live_params_default", "suma_live_params_check", "suma_localizer_enable_live_grid", "suma_localizer_disable_live_grid",
       "suma_localizer_clear_live_grid", "suma_localizer_live_update_flags", "suma_localizer_live_counts",
       "suma_localizer_live_cells_device", "suma_localizer_live_state", "suma_localizer_set_live_state"]


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
    for m in ("enableLiveGrid", "disableLiveGrid", "clearLiveGrid", "liveUpdateFlags", "liveCounts", "liveCells", "liveState",
              "setLiveState"):
        assert hasattr(built.Localizer, m), m
    assert hasattr(built, "LiveParams")
    adapter = open(os.path.join(ROOT, "include", "suma_adapter.hpp")).read()
    for m in ("enableLiveGrid", "liveCells("):
        assert m in adapter, m


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd import types as T
    structs = {"suma_live_params": T.LiveParams, "suma_live_counts": T.LiveCounts, "suma_live_stats": T.LiveStats}
    body = []
    for cname, S in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in S._fields_]
    body.append('printf("%zu\\n", sizeof(suma_live_cell));')
    body += [f'printf("%zu\\n", offsetof(suma_live_cell, {f}));' for f in T.LIVE_CELL_DTYPE.names]
    # the structures every earlier entry uses keep their sizes
    earlier = {"suma_params": T.SumaParams, "suma_localizer_params": T.LocalizerParams, "suma_localizer_result": T.LocalizerResult,
               "suma_world_surfel": T.WORLD_SURFEL_DTYPE, "suma_novel_params": T.NovelParams, "suma_novel_counts": T.NovelCounts,
               "suma_novel_fuse_params": T.NovelFuseParams, "suma_novel_stats": T.NovelStats,
               "suma_object_params": T.ObjectParams, "suma_object_counts": T.ObjectCounts, "suma_scan_object": T.SCAN_OBJECT_DTYPE,
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
    want += [T.LIVE_CELL_DTYPE.itemsize] + [T.LIVE_CELL_DTYPE.fields[f][1] for f in T.LIVE_CELL_DTYPE.names]
    want += [S.itemsize if hasattr(S, "itemsize") else C.sizeof(S) for S in earlier.values()]
    assert v == want
    assert C.sizeof(T.LiveParams) == 16 and C.sizeof(T.LiveCounts) == 40 and C.sizeof(T.LiveStats) == 16
    assert T.LIVE_CELL_DTYPE.itemsize == 16
    assert T.LIVE_COUNTS == ("n_texels", "n_members", "n_outside", "n_no_ground", "n_low", "n_high", "n_hit_texels",
                             "n_hit_cells", "n_rays", "n_cleared")
    assert T.LIVE_STATS == ("n_live", "n_pending", "n_expired", "n_carved")
    # what the earlier sizes were before this layer existed
    assert (T.GRID_CELL_DTYPE.itemsize, T.SCAN_OBJECT_DTYPE.itemsize, C.sizeof(T.ObjectParams), C.sizeof(T.ObjectCounts),
            T.PLAN_CELL_DTYPE.itemsize, T.WORLD_SURFEL_DTYPE.itemsize, C.sizeof(T.NovelParams)) == (48, 64, 16, 24, 8, 48, 16)


def test_shim_structures_match_c(built, tmp_path):
    """tests/live_shim.c declares the structures again: its copies have the header's layouts"""
    from semantic_suma_amd.types import GRID_CELL_DTYPE, LIVE_CELL_DTYPE, LIVE_COUNTS, LIVE_STATS
    shim = open(os.path.join(ROOT, "tests", "live_shim.c")).read()
    decls = shim[shim.index("typedef struct"):shim.index("} gcell_t;") + len("} gcell_t;")]
    pairs = [("lparams_t", "suma_live_params", ["hold_scans", "min_hits", "carve_range", "carve_margin"]),
             ("lcell_t", "suma_live_cell", list(LIVE_CELL_DTYPE.names)),
             ("lcounts_t", "suma_live_counts", list(LIVE_COUNTS)),
             ("lstats_t", "suma_live_stats", list(LIVE_STATS)),
             ("gcell_t", "suma_grid_cell", list(GRID_CELL_DTYPE.names))]
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
    assert len(re.findall(r"typedef struct", decls)) == 6          # the five above and lgrid_t, the shim's own
    import live_common as lv
    from semantic_suma_amd.types import GridParams
    g = lv.ShimGrid.of(GridParams.defaults(cell_size=0.5, origin=(1.0, 2.0), width=3, height=4, step_height=0.125, clearance=3.0))
    assert (g.cell_size, g.origin_x, g.origin_y, g.width, g.height, g.step_height, g.clearance) == (0.5, 1.0, 2.0, 3, 4, 0.125, 3.0)
    assert C.sizeof(lv.ShimGrid) == 28


def test_defaults(built):
    from semantic_suma_amd.types import LiveParams
    L = built.lib()
    q = LiveParams(7, 7, 9.0, 9.0)
    L.suma_live_params_default(C.byref(q))
    assert (q.hold_scans, q.min_hits, q.carve_range, q.carve_margin) == (10, 2, 20.0, 0.5)
    assert bytes(q) == bytes(LiveParams.defaults())
    L.suma_live_params_default(None)
    assert LiveParams.defaults(min_hits=9).min_hits == 9
    with pytest.raises(KeyError):
        LiveParams.defaults(no_such_field=1)


def test_refusals_without_a_device(built):
    """nothing here reaches a device: a NULL localiser"""
    L = built.lib()
    n = C.c_uint32(7)
    assert L.suma_localizer_enable_live_grid(None, None, None, None) == -1 and L.suma_localizer_disable_live_grid(None) == -1
    assert L.suma_localizer_clear_live_grid(None) == -1
    assert L.suma_localizer_live_update_flags(None, None, None, None, 0, None) == -1
    assert L.suma_localizer_live_counts(None, None, None) == -1
    assert L.suma_localizer_live_cells_device(None, None, None, None) == -1
    assert L.suma_localizer_live_state(None, None, 0, C.byref(n)) == -1 and n.value == 7
    assert L.suma_localizer_set_live_state(None, None, 0, 0) == -1


def test_out_of_range_parameters_are_refused_with_a_message(built):
    from semantic_suma_amd.types import LiveParams
    L = built.lib()
    L.suma_last_error.restype = C.c_char_p
    assert L.suma_live_params_check(C.byref(LiveParams.defaults())) == 0
    for ok in (dict(hold_scans=1), dict(hold_scans=65535), dict(min_hits=1), dict(min_hits=65535), dict(carve_range=0.0),
               dict(carve_margin=0.0), dict(carve_range=1e30)):
        assert L.suma_live_params_check(C.byref(LiveParams.defaults(**ok))) == 0, ok
    for bad, what in ((dict(hold_scans=0), "hold_scans"), (dict(hold_scans=65536), "hold_scans"), (dict(min_hits=0), "min_hits"),
                      (dict(min_hits=65536), "min_hits"), (dict(carve_range=-1.0), "carve_range"),
                      (dict(carve_range=float("nan")), "carve_range"), (dict(carve_range=float("inf")), "carve_range"),
                      (dict(carve_margin=-0.5), "carve_margin"), (dict(carve_margin=float("nan")), "carve_margin"),
                      (dict(carve_margin=float("inf")), "carve_margin")):
        assert L.suma_live_params_check(C.byref(LiveParams.defaults(**bad))) == -1, bad
        assert what in L.suma_last_error(None).decode(), (bad, L.suma_last_error(None))
    assert L.suma_live_params_check(None) == -1
