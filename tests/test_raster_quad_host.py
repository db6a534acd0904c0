"""The per-quad set-up of k_render's rasteriser (semantic_suma_amd/csrc/raster_quad.h) against its specification, on the
CPU: tests/cpp/raster_quad_driver.cpp -- a stand-alone program, its own main, only raster_quad.h -- holds
quad_test(quad_setup(q), ...) == min(raster_key(T1), raster_key(T2)) as 64-bit keys over 10^7 random quads (integer
vertices below 2^21 in 1/256 px, depths in [-0.1, 1.1], pixels in and just around the box, the three tie modes) and over
crafted quads: both orientations of each strip triangle independently, zero-area triangles, pixel centres exactly on the
shared diagonal, on every outline edge and on a corner, horizontal and vertical edges, tu^2 + tv^2 == 1 exactly.  The
driver asserts itself that each of these classes occurred.  Built as the kernels are, with -ffp-contract=off."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "raster_quad_driver.cpp")
INC = os.path.join(ROOT, "semantic_suma_amd", "csrc")


def build_and_run(tmp_path, flags, n):
    exe = tmp_path / "raster_quad_driver"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-I", INC, SRC,
                           "-o", str(exe)])
    out = subprocess.run([str(exe), str(n)], capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = {l.split(":")[0]: l for l in out.stdout.splitlines()}
    for part in ("random", "crafted"):
        assert re.search(r"\b0 mismatches", lines[part]), lines[part]
    return lines


def test_quad_test_equals_raster_key(tmp_path):
    lines = build_and_run(tmp_path, ["-O2"], 10_000_000)
    m = re.match(r"random: (\d+) quads, (\d+) tests, (\d+) drawn, (\d+) by both triangles, (\d+) on an edge \((\d+) drawn\), "
                 r"orientations \+\+ (\d+) \+- (\d+) -\+ (\d+) -- (\d+), (\d+) with a zero-area triangle", lines["random"])
    quads, tests, drawn, both, on_edge, on_edge_drawn, pp, pn, np_, nn, degenerate = map(int, m.groups())
    assert quads >= 10_000_000 and tests == 9 * quads
    # the random part must itself reach every class: fragments, overlapping triangles, each orientation pair, exact edges
    assert drawn > quads // 100 and both > 0 and min(pp, pn, np_, nn) > quads // 100 and degenerate > 0 and on_edge_drawn > 0
    assert "0 failed expectations" in lines["crafted"]


def test_quad_test_equals_raster_key_plain_division(tmp_path):
    """the -DSUMA_BARY_PLAIN_DIV form of both sides (IEEE `/` instead of exact_div.h)"""
    build_and_run(tmp_path, ["-O2", "-DSUMA_BARY_PLAIN_DIV"], 1_000_000)


def test_driver_under_sanitizers(tmp_path):
    """the same program under the address and undefined-behaviour sanitizers (a plain host program: nothing preloaded);
    a tenth of the random quads and every crafted one -- what the sanitizers look for does not depend on the count"""
    build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], 1_000_000)
