"""C-ABI checks of the loop-closing entry points that need no GPU: the header's new symbols are exported, the ctypes
mirrors of suma_loop_params / suma_loop_status have the C layouts, the defaults are the reference's, and
examples/odometry.c (now with --close-loops) still compiles and links."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_loop_params_default", "suma_pipeline_enable_loop_closing", "suma_pipeline_check_loop_closure",
       "suma_pipeline_loop_status", "suma_pipeline_posegraph", "suma_pipeline_trajectory_distances",
       "suma_loop_find_candidate", "suma_posegraph_reserve", "suma_posegraph_edge"]


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


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import LoopParams, LoopStatus
    fields_p = [n for n, _ in LoopParams._fields_]
    fields_s = [n for n, _ in LoopStatus._fields_]
    src = tmp_path / "sz.c"
    body = ['printf("%zu %zu\\n", sizeof(suma_loop_params), sizeof(suma_loop_status));']
    body += [f'printf("%zu\\n", offsetof(suma_loop_params, {f}));' for f in fields_p]
    body += [f'printf("%zu\\n", offsetof(suma_loop_status, {f}));' for f in fields_s]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert v[0] == C.sizeof(LoopParams) and v[1] == C.sizeof(LoopStatus)
    off = v[2:]
    assert off[:len(fields_p)] == [getattr(LoopParams, f).offset for f in fields_p]
    assert off[len(fields_p):] == [getattr(LoopStatus, f).offset for f in fields_s]


def test_defaults_are_the_reference_values(built):
    from semantic_suma_amd.types import LoopParams
    p = LoopParams()
    built.lib().suma_loop_params_default(C.byref(p))
    f32 = lambda x: C.c_float(x).value
    assert (p.residual_threshold, p.outlier_threshold, p.valid_threshold) == (f32(1.05), f32(1.1), f32(0.9))
    assert (p.search_distance, p.min_trajectory_distance) == (20.0, 200.0)
    assert (p.min_verifications, p.delta_timestamp) == (3, 100)
    assert (p.min_valid_ratio, p.max_outlier_ratio, p.max_increment_difference) == (0.2, 0.85, 0.1)
    assert [p.information[i] for i in range(36)] == [1.0 if i % 7 == 0 else 0.0 for i in range(36)]
    assert (p.optimize_iterations, p.optimize_wait, p.integrate_lag) == (100, 1, 0)
    assert bytes(p) == bytes(LoopParams.defaults())


def test_c_example_with_close_loops_compiles_and_links(built, tmp_path):
    exe = tmp_path / "odometry"
    libdir = os.path.dirname(built.LIB_PATH)
    path = os.path.join(ROOT, "examples", "odometry.c")
    assert "--close-loops" in open(path).read()
    subprocess.check_call(["gcc", "-std=c99", "-D_POSIX_C_SOURCE=200809L", "-O1", "-Wall", "-Wextra", "-Werror", "-I",
                           os.path.join(ROOT, "include"), path, "-o", str(exe), "-L", libdir, "-lsuma_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 2 and "--close-loops" in out.stderr
