"""C-ABI checks of the place index and the relocalisation that need no GPU: the header's new symbols are exported and
bound, the ctypes mirrors have the C layouts, the defaults are as the header states, create refuses bad parameters
before it touches a device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_place_params_default", "suma_place_index_create", "suma_place_index_destroy", "suma_place_index_clear",
       "suma_place_index_size", "suma_place_index_last_error", "suma_place_index_add_frame", "suma_place_index_download",
       "suma_place_index_upload", "suma_place_index_query_frame", "suma_place_index_query", "suma_place_index_query_all",
       "suma_localizer_relocalize", "suma_localizer_relocalize_device"]


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
    assert hasattr(built, "PlaceIndex") and hasattr(built.Localizer, "relocalize")
    from semantic_suma_amd import places
    assert callable(places.save) and callable(places.load)
    assert "there is no global relocalisation" not in header


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import (DRAW_COLORS, LocalizerResult, PLACE_MAX_DIM, PLACE_MAX_MATCHES, PlaceMatch,
                                         PlaceParams, RelocalizeCandidate, RelocalizeResult)
    structs = {"suma_place_params": PlaceParams, "suma_place_match": PlaceMatch,
               "suma_relocalize_candidate": RelocalizeCandidate, "suma_relocalize_result": RelocalizeResult}
    body = ['printf("%d\\n%d\\n", SUMA_PLACE_MAX_DIM, SUMA_PLACE_MAX_MATCHES);']
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [PLACE_MAX_DIM, PLACE_MAX_MATCHES]
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    assert v == want
    assert C.sizeof(PlaceMatch) == 20 and C.sizeof(PlaceParams) == 16 + DRAW_COLORS
    assert C.sizeof(RelocalizeCandidate) == 24 + C.sizeof(LocalizerResult)
    assert C.sizeof(RelocalizeResult) == 40 + C.sizeof(LocalizerResult) + 32 * C.sizeof(RelocalizeCandidate)


def test_defaults(built):
    from semantic_suma_amd.types import DRAW_COLORS, DYNAMIC_LABELS, PlaceParams
    pp = PlaceParams(1, 1, 1.0, 1.0)
    built.lib().suma_place_params_default(C.byref(pp))
    assert (pp.rings, pp.sectors, pp.max_range, pp.height_offset) == (20, 60, 80.0, 2.0)
    assert list(pp.keep_label) == [1] * DRAW_COLORS
    assert bytes(pp) == bytes(PlaceParams.defaults())
    q = PlaceParams.defaults(rings=7, max_range=50.0)
    assert (q.rings, q.sectors, q.max_range) == (7, 60, 50.0)
    s = PlaceParams.static_only()
    assert [l for l in range(DRAW_COLORS) if not s.keep_label[l]] == sorted(DYNAMIC_LABELS)
    # is_dynamic_label (csrc/dev_math.h) names exactly these
    text = open(os.path.join(ROOT, "semantic_suma_amd", "csrc", "dev_math.h")).read()
    body = text[text.index("bool is_dynamic_label"):]
    body = body[:body.index("}")]
    import re
    assert sorted(int(float(x)) for x in re.findall(r"l == ([0-9.]+)f", body)) == sorted(DYNAMIC_LABELS)
    with pytest.raises(KeyError):
        PlaceParams.defaults(ringz=3)


def test_create_refuses_bad_parameters_without_a_device(built):
    """checked before a device is touched, so no GPU is needed: the message is suma_last_error(NULL)"""
    from semantic_suma_amd.types import PlaceParams
    L = built.lib()
    cases = ((dict(rings=0), "rings"), (dict(rings=65), "rings"), (dict(sectors=0), "sectors"), (dict(sectors=65), "sectors"),
             (dict(max_range=0.0), "max_range"), (dict(max_range=-1.0), "max_range"),
             (dict(max_range=float("inf")), "max_range"), (dict(max_range=float("nan")), "max_range"),
             (dict(height_offset=float("nan")), "height_offset"), (dict(height_offset=float("inf")), "height_offset"))
    for kw, needle in cases:
        h = C.c_void_p()
        pp = PlaceParams.defaults(**kw)
        assert L.suma_place_index_create(C.byref(pp), 0, 4, C.byref(h)) == -1 and not h.value, kw
        assert needle in L.suma_last_error(None).decode(), kw
        assert needle in L.suma_place_index_last_error(None).decode(), kw
    with pytest.raises(built.SumaError, match="sectors"):
        built.PlaceIndex(PlaceParams.defaults(sectors=100))
    assert L.suma_place_index_size(None) == 0
