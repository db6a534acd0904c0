"""C-ABI checks of the per-scan objects that need no GPU: the header's new symbols are exported and bound, the ctypes
mirrors, the numpy record and the shim's own structures have the C layouts, the defaults are as the header states,
out-of-range parameters are refused with a message by the rule suma_localizer_enable_objects applies, and NULL handles are
refused before any device exists.  (That enabling refuses a localiser whose novelty is off needs a localiser, hence a
device: test_gpu_objects.py::test_refusals.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_object_params_default", "suma_object_params_check", "suma_localizer_enable_objects", "suma_localizer_disable_objects",
       "suma_localizer_objects", "suma_localizer_objects_device", "suma_localizer_object_ids",
       "suma_localizer_segment_flags", "suma_localizer_novel_flags", "suma_localizer_frame"]


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
    for m in ("enableObjects", "disableObjects", "objects", "objectIds", "segmentFlags", "novelFlags", "scanFrame"):
        assert hasattr(built.Localizer, m), m
    adapter = open(os.path.join(ROOT, "include", "suma_adapter.hpp")).read()
    for m in ("enableObjects", "objects("):
        assert m in adapter, m


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import (LocalizerParams, LocalizerResult, OBJECT_COUNTS, ObjectCounts, ObjectParams,
                                         SCAN_OBJECT_DTYPE, WORLD_SURFEL_DTYPE)
    structs = {"suma_object_params": ObjectParams, "suma_object_counts": ObjectCounts}
    body = []
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    body.append('printf("%zu\\n", sizeof(suma_scan_object));')
    body += [f'printf("%zu\\n", offsetof(suma_scan_object, {f}));' for f in SCAN_OBJECT_DTYPE.names]
    # the structures every earlier entry uses keep their sizes
    body += ['printf("%zu\\n", sizeof(suma_localizer_params));', 'printf("%zu\\n", sizeof(suma_localizer_result));',
             'printf("%zu\\n", sizeof(suma_world_surfel));', 'printf("%zu\\n", sizeof(suma_novel_params));',
             'printf("%zu\\n", sizeof(suma_novel_counts));']
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    want += [SCAN_OBJECT_DTYPE.itemsize] + [SCAN_OBJECT_DTYPE.fields[f][1] for f in SCAN_OBJECT_DTYPE.names]
    from semantic_suma_amd.types import NovelCounts, NovelParams
    want += [C.sizeof(LocalizerParams), C.sizeof(LocalizerResult), WORLD_SURFEL_DTYPE.itemsize, C.sizeof(NovelParams),
             C.sizeof(NovelCounts)]
    assert v == want
    assert C.sizeof(ObjectParams) == 16 and C.sizeof(ObjectCounts) == 24 and SCAN_OBJECT_DTYPE.itemsize == 64
    assert OBJECT_COUNTS == ("n_texels", "n_members", "n_components", "n_small", "n_objects", "stored")


def test_shim_structures_match_c(built, tmp_path):
    """tests/object_shim.c declares the structures again: its copies have the header's layouts"""
    from semantic_suma_amd.types import SCAN_OBJECT_DTYPE
    shim = open(os.path.join(ROOT, "tests", "object_shim.c")).read()
    decls = shim[shim.index("typedef struct"):shim.index("} ocounts_t;") + len("} ocounts_t;")]
    pairs = [("oparams_t", "suma_object_params", ["link_base", "link_slope", "min_texels", "max_objects"]),
             ("object_t", "suma_scan_object", list(SCAN_OBJECT_DTYPE.names)),
             ("ocounts_t", "suma_object_counts", ["n_texels", "n_members", "n_components", "n_small", "n_objects", "stored"])]
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
    assert len(re.findall(r"typedef struct", decls)) == 3


def test_defaults(built):
    from semantic_suma_amd.types import ObjectParams
    L = built.lib()
    q = ObjectParams(9.0, 9.0, 7, 7)
    L.suma_object_params_default(C.byref(q))
    assert (q.link_base, q.link_slope, q.min_texels, q.max_objects) == (C.c_float(0.3).value, C.c_float(0.03).value, 5, 4096)
    assert bytes(q) == bytes(ObjectParams.defaults())
    L.suma_object_params_default(None)
    assert ObjectParams.defaults(min_texels=9).min_texels == 9
    with pytest.raises(KeyError):
        ObjectParams.defaults(no_such_field=1)


def test_refusals_without_a_device(built):
    """nothing here reaches a device: a NULL localiser"""
    L = built.lib()
    n = C.c_uint32(7)
    assert L.suma_localizer_enable_objects(None, None) == -1 and L.suma_localizer_disable_objects(None) == -1
    assert L.suma_localizer_objects(None, None, 0, C.byref(n), None, None) == -1 and n.value == 7
    assert L.suma_localizer_objects_device(None, None, 0, C.byref(n), None, None) == -1
    assert L.suma_localizer_object_ids(None, None, 0, C.byref(n)) == -1
    assert L.suma_localizer_segment_flags(None, None, None, None, 0, None) == -1
    assert L.suma_localizer_novel_flags(None, None, 0, C.byref(n)) == -1
    assert L.suma_localizer_frame(None) is None


def test_out_of_range_parameters_are_refused_with_a_message(built):
    from semantic_suma_amd.types import ObjectParams
    L = built.lib()
    L.suma_last_error.restype = C.c_char_p
    assert L.suma_object_params_check(C.byref(ObjectParams.defaults())) == 0
    for ok in (dict(link_base=0.0), dict(link_slope=0.0), dict(min_texels=1), dict(max_objects=1), dict(max_objects=65536),
               dict(min_texels=0xffffffff)):
        assert L.suma_object_params_check(C.byref(ObjectParams.defaults(**ok))) == 0, ok
    for bad, what in ((dict(link_base=-0.1), "link_base"), (dict(link_base=float("nan")), "link_base"),
                      (dict(link_base=float("inf")), "link_base"), (dict(link_slope=-1.0), "link_slope"),
                      (dict(link_slope=float("nan")), "link_slope"), (dict(min_texels=0), "min_texels"),
                      (dict(max_objects=0), "max_objects"), (dict(max_objects=65537), "max_objects")):
        assert L.suma_object_params_check(C.byref(ObjectParams.defaults(**bad))) == -1, bad
        assert what in L.suma_last_error(None).decode(), (bad, L.suma_last_error(None))
    assert L.suma_object_params_check(None) == -1
