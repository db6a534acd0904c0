"""C-ABI checks of the localiser that need no GPU: the header's new symbols are exported and bound, the ctypes mirrors
have the C layouts, the defaults are as the header states."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_localizer_params_default", "suma_localizer_create", "suma_localizer_destroy", "suma_localizer_ctx",
       "suma_localizer_set_map", "suma_localizer_set_map_device", "suma_localizer_set_pose",
       "suma_localizer_process_scan", "suma_localizer_process_scan_device", "suma_localizer_window",
       "suma_localizer_download_window"]


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
    assert hasattr(built, "Localizer") and hasattr(built.Localizer, "from_ply")


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import IcpStats, LocalizerParams, LocalizerResult
    structs = {"suma_localizer_params": LocalizerParams, "suma_localizer_result": LocalizerResult}
    body = []
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    assert v == want
    assert C.sizeof(LocalizerParams) == 16 and C.sizeof(LocalizerResult) == 3 * 128 + C.sizeof(IcpStats) + 32


def test_defaults(built):
    from semantic_suma_amd.types import LocalizerParams, default_params
    p = default_params(confidence_threshold=0.75)
    lp = LocalizerParams(1.0, 1.0, 1.0, 7)
    built.lib().suma_localizer_params_default(C.byref(p), C.byref(lp))
    assert lp.conf_threshold == 0.75 and lp.constant_velocity == 1
    assert lp.min_valid_ratio == C.c_float(0.2).value and lp.max_outlier_ratio == C.c_float(0.85).value
    assert bytes(lp) == bytes(LocalizerParams.defaults(p))
    built.lib().suma_localizer_params_default(None, C.byref(lp))
    assert lp.conf_threshold == 0.0 and bytes(lp) == bytes(LocalizerParams.defaults())
    q = LocalizerParams.defaults(p, constant_velocity=0, min_valid_ratio=0.5)
    assert (q.constant_velocity, q.min_valid_ratio, q.conf_threshold) == (0, 0.5, 0.75)


def test_create_refuses_bad_parameters_without_a_device(built):
    """checked before a ctx is made, so no GPU is needed: the message is suma_last_error(NULL)"""
    from semantic_suma_amd.types import LocalizerParams, default_params
    L = built.lib()
    for kw, needle in ((dict(active_timestamps=50), "active_timestamps"), (dict(submap_extent=0.0), "submap_extent"),
                       (dict(submap_extent=float("nan")), "submap_extent"), (dict(submap_dimension=-1), "submap_dimension")):
        h = C.c_void_p()
        p = default_params(**kw)
        assert L.suma_localizer_create(C.byref(p), None, 0, C.byref(h)) == -1 and not h.value
        assert needle in L.suma_last_error(None).decode(), kw
    p, h = default_params(), C.c_void_p()
    lp = LocalizerParams.defaults(p, min_valid_ratio=float("nan"))
    assert L.suma_localizer_create(C.byref(p), C.byref(lp), 0, C.byref(h)) == -1 and "NaN" in L.suma_last_error(None).decode()
