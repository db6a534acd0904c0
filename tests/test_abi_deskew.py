"""C-ABI checks of the motion compensation of raw sweeps that need no GPU: the header's new symbols are exported and
bound, suma_deskew_params has the stated size and offsets, the defaults are as the header states, and every
SUMA_ERR_INVALID case of the parameters is returned before any device exists (suma_deskew_check; NULL handles)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_deskew_params_default", "suma_deskew_check", "suma_deskew_points", "suma_deskew_points_device",
       "suma_pipeline_enable_deskew", "suma_pipeline_disable_deskew", "suma_pipeline_set_deskew_motion",
       "suma_pipeline_deskew_motion", "suma_localizer_enable_deskew", "suma_localizer_disable_deskew",
       "suma_localizer_set_deskew_motion", "suma_localizer_deskew_motion"]


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
    assert hasattr(built, "deskew_points") and hasattr(built, "deskew_points_device")
    adapter = open(os.path.join(ROOT, "include", "suma_adapter.hpp")).read()
    for m in ("enableDeskew", "disableDeskew", "setDeskewMotion", "deskewMotion"):
        assert hasattr(built.SurfelMapping, m) and hasattr(built.Localizer, m), m
        assert adapter.count(m + "(") == 2, m  # SurfelMapping and Localizer
    flat = " ".join(header.replace("*", " ").split())
    assert "pending one-shot override is NOT saved" in flat  # what the header says about checkpoints


def test_layout_matches_c(built, tmp_path):
    from semantic_suma_amd.types import DeskewParams
    body = ['printf("%zu\\n", sizeof(suma_deskew_params));']
    body += [f'printf("%zu\\n", offsetof(suma_deskew_params, {f}));' for f, _ in DeskewParams._fields_]
    body += ['printf("%d %d %d %d %d\\n", SUMA_DESKEW_TIME_AZIMUTH, SUMA_DESKEW_TIME_TIMES, SUMA_DESKEW_MOTION_NONE, '
             'SUMA_DESKEW_MOTION_INCREMENT, SUMA_DESKEW_MOTION_OVERRIDE);']
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert v[:6] == [20, 0, 4, 8, 12, 16]  # the stated layout
    assert v[:6] == [C.sizeof(DeskewParams)] + [getattr(DeskewParams, f).offset for f, _ in DeskewParams._fields_]
    from semantic_suma_amd import types as t
    assert v[6:] == [t.DESKEW_TIME_AZIMUTH, t.DESKEW_TIME_TIMES, t.DESKEW_MOTION_NONE, t.DESKEW_MOTION_INCREMENT,
                     t.DESKEW_MOTION_OVERRIDE]


def test_defaults(built):
    from semantic_suma_amd.types import DESKEW_TIME_AZIMUTH, DeskewParams
    dp = DeskewParams(time_source=7, clockwise=7, start_azimuth=7.0, t_ref=7.0, scale=7.0)
    built.lib().suma_deskew_params_default(C.byref(dp))
    want = DeskewParams.defaults()
    assert bytes(dp) == bytes(want)
    assert (dp.time_source, dp.clockwise, dp.start_azimuth, dp.t_ref, dp.scale) == (DESKEW_TIME_AZIMUTH, 0, 0.0, 0.5, 1.0)
    built.lib().suma_deskew_params_default(None)  # tolerated


def test_every_invalid_case_without_a_device(built):
    from semantic_suma_amd.types import DESKEW_TIME_TIMES, DeskewParams
    L = built.lib()
    eye = np.ascontiguousarray(np.eye(4))
    check = lambda dp, have_times=0, motion=eye: L.suma_deskew_check(  # noqa: E731
        None if dp is None else C.byref(dp), have_times, None if motion is None else motion.ctypes.data)
    assert check(None) == 0 and check(DeskewParams.defaults()) == 0
    for t_ref in (0.0, 1.0):
        assert check(DeskewParams.defaults(t_ref=t_ref)) == 0
    bad = [DeskewParams.defaults(t_ref=-1e-6), DeskewParams.defaults(t_ref=float(np.nextafter(np.float32(1), np.float32(2)))),
           DeskewParams.defaults(t_ref=float("nan")), DeskewParams.defaults(t_ref=float("inf")),
           DeskewParams.defaults(scale=float("nan")), DeskewParams.defaults(scale=float("-inf")),
           DeskewParams.defaults(start_azimuth=float("nan")), DeskewParams.defaults(start_azimuth=float("inf")),
           DeskewParams.defaults(start_azimuth=7.0), DeskewParams.defaults(time_source=2), DeskewParams.defaults(time_source=-1),
           DeskewParams.defaults(clockwise=2)]
    for dp in bad:
        assert check(dp) == -1, (dp.time_source, dp.clockwise, dp.start_azimuth, dp.t_ref, dp.scale)
        assert L.suma_last_error(None).decode().startswith("suma_deskew_points: ")
    # the times source needs times
    times = DeskewParams.defaults(time_source=DESKEW_TIME_TIMES)
    assert check(times, 1) == 0 and check(times, 0) == -1 and b"times" in L.suma_last_error(None)
    # the motion: NULL, NaN, inf -- anywhere in the 16
    assert check(None, 0, None) == -1
    for k in range(16):
        for v in (np.nan, np.inf):
            m = eye.copy()
            m.reshape(-1)[k] = v
            assert check(None, 0, m) == -1 and b"non-finite motion" in L.suma_last_error(None)
    # NULL handles are refused before any device exists
    dp = DeskewParams.defaults()
    pts = np.zeros((4, 4), dtype=np.float32)
    assert L.suma_deskew_points(None, C.byref(dp), pts.ctypes.data, None, 4, eye.ctypes.data, pts.ctypes.data) == -1
    assert L.suma_deskew_points_device(None, C.byref(dp), None, None, 0, eye.ctypes.data, None) == -1
    src = C.c_int32(5)
    for who in ("pipeline", "localizer"):
        assert getattr(L, f"suma_{who}_enable_deskew")(None, C.byref(dp)) == -1
        assert getattr(L, f"suma_{who}_disable_deskew")(None) == -1
        assert getattr(L, f"suma_{who}_set_deskew_motion")(None, eye.ctypes.data) == -1
        assert getattr(L, f"suma_{who}_deskew_motion")(None, eye.ctypes.data, C.byref(src)) == -1 and src.value == 5
