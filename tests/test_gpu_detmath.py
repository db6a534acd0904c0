"""Device against host, bit for bit, for the arithmetic every parity test relies on (run with -m gpu on an MI355X).

All GPU parity tests compare a gfx950 kernel with a gcc-built host restatement, which holds only if the elementary
functions of include/suma_detmath.h, the IEEE primitives they are made of and the fp32 helpers of csrc/dev_math.h give
the same bits on both sides.  tests/detmath_device.hip evaluates them on the device, compiled with the CXXFLAGS of
semantic_suma_amd/csrc/Makefile (a flag edit in the library's build reaches this test), and compares every output with
tests/detmath_shim.c compiled by gcc with the CFLAGS of oracle/Makefile (the oracle's compiler and flags).  Inputs
(tests/detmath_inputs.h) are made from an index on both sides:

* unary fp32: 2^30 bit patterns at the odd stride 0x9E3779B1 (every 4th pattern on average; all 2^32 would take
  ~4x the host time), the edge set (+-0, +-min / max subnormal, +-FLT_MIN, +-FLT_MAX, +-inf, quiet and signalling
  NaNs with payloads), +-4096-ulp windows around every branch threshold of the header and, for sin / cos, around
  k*pi/4 for all k <= 8192 * 4/pi;
* atan2 on a 2^13 x 2^13 grid of strided patterns, `/` on 2^24 random pairs, fma on 2^24 random triples, each plus the
  edge set's Cartesian product; float <-> int32 conversions inside the header's guards;
* sdm_sin_d / sdm_cos_d on strided doubles over |x| <= 2^30, windows around k*pi/4, tiny arguments, the 2^30 cut-off;
* dev_math.h against oracle/o_math.h on 2^24 vectors whose components are normal, subnormal, huge (the products
  overflow), +0 or -0; depth24 on every pattern of [0, 1].

The assertion is bit equality, NaN payloads included (assert_bit_equal of the parity tests compares NaN bits too).
"""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
LOG2N = 30  # strided fp32 patterns per unary function (all 2^32: ~4x the host time, over a minute more)

UNARY = ["atan", "asin", "acos", "sin", "cos", "exp", "log", "floor", "round", "sqrt"]
PRIMITIVES = ["rint", "f2i", "i2f", "div", "fma"]
VECTOR = ["dot3", "len3", "normalize3", "cross3", "divs3", "m4_point", "m4_dir", "m4_mul", "pack_rgb", "depth24"]
ALL = UNARY + ["atan2"] + PRIMITIVES + ["sin_d", "cos_d"] + VECTOR
MIN_INPUTS = {**{f: 1 << 30 for f in UNARY + ["rint", "f2i", "i2f"]}, "atan2": 1 << 26, "div": 1 << 24, "fma": 1 << 24,
              "sin_d": 1 << 24, "cos_d": 1 << 24, "depth24": 0x3f800001,
              **{f: 1 << 24 for f in VECTOR if f != "depth24"}}


def make_var(path, name):
    """the value of `name = ...` in a Makefile, with $(ARCH) / $(FMA) expanded as make would here"""
    text = open(path).read()
    m = re.search(rf"^{name}\s*=\s*(.*)$", text, re.M)
    assert m, f"{name} not found in {path}"
    val = m.group(1)
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M)
    if arch:
        val = val.replace("$(ARCH)", arch.group(1))
    with open("/proc/cpuinfo") as f:
        fma = "-mfma" if re.search(r"\bfma\b", f.read()) else ""
    val = val.replace("$(FMA)", fma)
    assert "$(" not in val, val
    return val.split()


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("detmath_device")
    so = str(d / "libdetmath_shim.so")
    subprocess.check_call(["gcc"] + make_var(os.path.join(ROOT, "oracle", "Makefile"), "CFLAGS") +
                          ["-shared", os.path.join(HERE, "detmath_shim.c"), "-o", so, "-lm"])
    exe = str(d / "detmath_device")
    subprocess.check_call(["/opt/rocm/bin/hipcc"] +
                          make_var(os.path.join(ROOT, "semantic_suma_amd", "csrc", "Makefile"), "CXXFLAGS") +
                          [os.path.join(HERE, "detmath_device.hip"), "-o", exe, "-L", str(d), "-ldetmath_shim",
                           "-Wl,-rpath," + str(d)])
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
    out = subprocess.run([exe, str(LOG2N)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = {}
    for line in out.stdout.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            res[r["fn"]] = r
    return res


# Functions compared as NaN-class equal instead of bit equal (every non-NaN result still bit for bit):
# fma with two or three NaN operands of different bits returns a different one of them on the two sides.
# gfx950's v_fma_f32 picks by operand position (a's NaN, quieted, in every such case seen).  x86's vfmadd132ss /
# 213ss / 231ss return the first NaN in *encoding* order, and which form gcc picks (which operand lands in which
# register) is the register allocator's choice, so the host's pick is not even fixed across builds.
# No parity test can see it: the only NaNs their inputs carry are numpy's one quiet NaN (NaN points, NaN logits),
# so any NaNs meeting in one fma have the same bits, and NaN points are dropped by the range tests before any fma
# that could meet a second NaN.
NAN_CLASS_ONLY = {"fma"}


@pytest.mark.parametrize("fn", ALL)
def test_device_bits_equal_host(results, fn):
    r = results[fn]
    assert r["n"] >= MIN_INPUTS[fn], r
    bad = r["mismatch_not_nan"] if fn in NAN_CLASS_ONLY else r["mismatch"]
    assert bad == 0, f"{fn}: {r['mismatch']} of {r['n']} inputs differ ({r['mismatch_not_nan']} beyond NaN bits); " \
                     f"first (inputs, host, device): {r['first']}"
