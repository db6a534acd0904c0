"""C-ABI checks of the world export that need no GPU: the header's new symbols are exported, the ctypes mirrors and the
numpy record have the C layouts, the defaults are as the header states."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_world_params_default", "suma_map_cached_tiles", "suma_map_export_world"]


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


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import WORLD_SURFEL_DTYPE, WorldParams, WorldStats
    structs = {"suma_world_params": WorldParams, "suma_world_stats": WorldStats}
    body = ['printf("%zu\\n", sizeof(suma_world_surfel));']
    body += [f'printf("%zu\\n", offsetof(suma_world_surfel, {f}));' for f in WORLD_SURFEL_DTYPE.names]
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [WORLD_SURFEL_DTYPE.itemsize] + [WORLD_SURFEL_DTYPE.fields[f][1] for f in WORLD_SURFEL_DTYPE.names]
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    assert v == want
    assert v[0] == 48 and C.sizeof(WorldStats) == 24 and C.sizeof(WorldParams) == 8 + 260


def test_defaults(built):
    from semantic_suma_amd.types import WorldParams
    p = WorldParams(voxel_size=3.0, min_confidence=1.0)
    built.lib().suma_world_params_default(C.byref(p))
    assert p.voxel_size == 0.0 and p.min_confidence == -math.inf
    assert list(p.keep_label) == [1] * 260
    assert bytes(p) == bytes(WorldParams.defaults())
    q = WorldParams.defaults(0.5, 2.0, keep_labels=[10, 40])
    assert (q.voxel_size, q.min_confidence) == (0.5, 2.0)
    assert [l for l in range(260) if q.keep_label[l]] == [10, 40]
