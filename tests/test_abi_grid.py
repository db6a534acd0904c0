"""C-ABI checks of the traversability grid that need no GPU: the header's new symbols are exported, the ctypes mirrors and
the numpy cell have the C layouts, the defaults are as the header states."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_grid_params_default", "suma_world_grid_fit", "suma_world_grid"]


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
    assert "z UP" in header  # the header says which way the world frame's z points


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import GRID_CELL_DTYPE, GridParams, GridStats
    structs = {"suma_grid_params": GridParams, "suma_grid_stats": GridStats}
    body = ['printf("%zu\\n", sizeof(suma_grid_cell));']
    body += [f'printf("%zu\\n", offsetof(suma_grid_cell, {f}));' for f in GRID_CELL_DTYPE.names]
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    body.append('printf("%d %d %d %d\\n", SUMA_GRID_UNKNOWN, SUMA_GRID_FREE, SUMA_GRID_OBSTACLE, SUMA_GRID_NO_GROUND);')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [GRID_CELL_DTYPE.itemsize] + [GRID_CELL_DTYPE.fields[f][1] for f in GRID_CELL_DTYPE.names]
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    from semantic_suma_amd import types
    want += [types.GRID_UNKNOWN, types.GRID_FREE, types.GRID_OBSTACLE, types.GRID_NO_GROUND]
    assert v == want
    assert v[0] == 48 and C.sizeof(GridStats) == 36 and C.sizeof(GridParams) == 20 + 260 + 16


def test_defaults(built):
    from semantic_suma_amd.types import GridParams
    p = GridParams(cell_size=3.0, origin_x=1.0, width=7, fill_radius=5)
    p.ground_label[10] = 1
    built.lib().suma_grid_params_default(C.byref(p))
    assert (p.origin_x, p.origin_y, p.width, p.height, p.fill_radius) == (0.0, 0.0, 0, 0, 2)
    f32 = lambda v: C.c_float(v).value  # noqa: E731
    assert (p.cell_size, p.min_normal_z, p.step_height, p.clearance) == (f32(0.2), f32(0.7), f32(0.2), 2.0)
    assert [l for l in range(260) if p.ground_label[l]] == [40, 44, 48, 49, 60, 72]
    assert bytes(p) == bytes(GridParams.defaults())
    q = GridParams.defaults(0.5, origin=(-3.0, 4.0), width=9, height=2, ground_labels=[40], fill_radius=0)
    assert (q.cell_size, q.origin_x, q.origin_y, q.width, q.height, q.fill_radius) == (0.5, -3.0, 4.0, 9, 2, 0)
    assert q.as_dict()["ground_labels"] == [40]
