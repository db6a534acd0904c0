"""The deterministic math specification (include/suma_detmath.h) against a high-precision reference: accuracy in ulp
over the whole domain each function serves (strided bit patterns, the edge set, windows around every branch threshold),
numpy float64 for the fp32 functions and np.longdouble for the fp64 sin / cos, and the exact results of the specials.

Measured worst cases (host, gcc): atan 2.72 ulp, asin 2.30, acos 1.23, exp 1.0 (subnormal results in subnormal ulps),
log 0.82, sin / cos 1.28 / 1.46 on |x| <= pi and 7.8e-8 absolute on |x| <= 8192, atan2 3.06 on a 2^12 x 2^12 grid of
bit patterns.  The bounds below are those rounded up a little.

Conventions of the specification that differ from C's (GLSL leaves them open; every kernel, the GLSL prelude of
oracle/glref.py and the recorded fixtures follow them, so they are kept and pinned here as deliberate):
atan2(-0, x < 0) = +pi (C: -pi), atan2(+-0, -0) = 0 (C: +-pi), atan2(+-inf, +-inf) = NaN (C: +-pi/4, +-3pi/4),
atan(-0) = +0 and so atan2(-0, x > 0) = +0 (C: -0), floor(-0) = +0 (C: -0).

That the gfx950 computes the same bits as this host build is checked by tests/test_gpu_detmath.py (-m gpu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("detmath") / "detmath_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "detmath_shim.c"), "-o", so, "-lm"])
    return C.CDLL(so)


def run1(shim, name, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    getattr(shim, name)(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size)
    return y


def ulp_err(y, ref):
    ref32 = ref.astype(np.float32)
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    return np.abs(y.astype(np.float64) - ref) / np.maximum(ulp, 1e-45)


@pytest.mark.parametrize("name,fn,lo,hi,tol", [
    ("t_atan", np.arctan, -100.0, 100.0, 2.5), ("t_asin", np.arcsin, -1.0, 1.0, 3.0),
    ("t_acos", np.arccos, -1.0, 1.0, 3.0), ("t_sin", np.sin, -3.2, 3.2, 2.5), ("t_cos", np.cos, -3.2, 3.2, 2.5),
    ("t_exp", np.exp, -20.0, 5.0, 2.5), ("t_log", np.log, 1e-6, 100.0, 2.5), ("t_sqrt", np.sqrt, 0.0, 1e4, 0.5001),
])
def test_accuracy_vs_libm(shim, name, fn, lo, hi, tol):
    rng = np.random.default_rng(0)
    x = rng.uniform(lo, hi, 200000).astype(np.float32)
    y = run1(shim, name, x)
    err = ulp_err(y, fn(x.astype(np.float64)))
    # near zeros of sin/cos the absolute error is what matters (argument reduction); exclude |ref| tiny
    mask = np.abs(fn(x.astype(np.float64))) > 1e-3
    assert err[mask].max() <= tol, f"{name}: {err[mask].max()} ulp"


def test_atan2_quadrants_and_floor_round(shim):
    rng = np.random.default_rng(1)
    y = rng.uniform(-50, 50, 100000).astype(np.float32)
    x = rng.uniform(-50, 50, 100000).astype(np.float32)
    r = np.empty_like(x)
    shim.t_atan2(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), x.size)
    assert ulp_err(r, np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() <= 4.0  # division + atan + quadrant add
    v = np.concatenate([rng.uniform(-3000, 3000, 100000), [0.0, -0.0, 0.5, -0.5, 2047.999, -1e-30, 1e9, -1e9]]).astype(np.float32)
    assert np.array_equal(run1(shim, "t_floor", v), np.floor(v))
    near = np.round(rng.uniform(0, 255, 1000)).astype(np.float32) + rng.uniform(-0.2, 0.2, 1000).astype(np.float32)
    assert np.array_equal(run1(shim, "t_round", near), np.round(near))
    # GLSL round() at .5: to even, as the GL implementations do (76.5 and 178.5 are pack()'s ties, color.glsl:34-36)
    ties = np.array([0.5, 1.5, 2.5, 76.5, 77.5, 178.5, 179.5, -0.5, -1.5, -2.5, 8388607.5, 0.49999997, 0.50000006], dtype=np.float32)
    assert np.array_equal(run1(shim, "t_round", ties), np.round(ties))
    assert run1(shim, "t_round", np.array([76.5, 178.5], np.float32)).tolist() == [76.0, 178.0]


def test_double_sincos(shim):
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-10, 10, 100000), rng.uniform(-1e-3, 1e-3, 10000), [0.0, 1e-300]])
    s, c = np.empty_like(x), np.empty_like(x)
    shim.t_sin_d(x.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), x.size)
    shim.t_cos_d(x.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), x.size)
    assert np.abs(s - np.sin(x)).max() < 3e-16 and np.abs(c - np.cos(x)).max() < 3e-16


# ---- the whole domain: strided bit patterns, the edge set and windows around the branch thresholds ----
# (the same sets as tests/detmath_inputs.h, smaller: this runs on the CPU)

STRIDE = 0x9E3779B1
EDGE = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
                 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc12345, 0xffd5aa55,
                 0x7f800001, 0xff812345, 0x7fbfffff, 0xffa00001], np.uint32).view(np.float32)
THRESHOLDS = np.array([1e-4, 0.5, 1.0, 0.4142135623730950, 2.414213562373095, 0.707106781186547524, 88.72283905206835,
                       87.33654475, 103.278929903431851, 8192.0, 8388608.0, 2147483648.0, 1.17549435e-38], np.float32)


def strided(n, stride=STRIDE):
    return ((np.arange(n, dtype=np.uint64) * stride) & 0xffffffff).astype(np.uint32).view(np.float32)


def windows(centres, w):
    """every pattern within +-w ulps of each centre, both signs"""
    b = np.asarray(centres, np.float32).view(np.uint32).astype(np.int64)[:, None] + np.arange(-w, w + 1)[None, :]
    b = np.unique(b[b >= 0]).astype(np.uint32)
    return np.concatenate([b, b | np.uint32(0x80000000)]).view(np.float32)


@pytest.fixture(scope="module")
def domain():
    x = np.concatenate([strided(1 << 23), EDGE, windows(THRESHOLDS, 4096)])
    return x[np.isfinite(x)]


@pytest.mark.parametrize("name,fn,serves,tol", [
    ("t_atan", np.arctan, lambda x: np.ones(x.shape, bool), 3.0),
    ("t_asin", np.arcsin, lambda x: np.abs(x) <= 1, 2.5),
    ("t_acos", np.arccos, lambda x: np.abs(x) <= 1, 1.5),
    ("t_exp", np.exp, lambda x: np.ones(x.shape, bool), 1.5),  # subnormal results measured in subnormal ulps
    ("t_log", np.log, lambda x: x > 0, 1.0),
])
def test_accuracy_full_domain(shim, domain, name, fn, serves, tol):
    x = domain[serves(domain)]
    y = run1(shim, name, x)
    with np.errstate(over="ignore"):
        ref = fn(x.astype(np.float64))
        ref32 = ref.astype(np.float32)
    inf = np.isinf(ref32)  # exp beyond FLT_MAX (+ half an ulp): +inf, exactly where the rounded reference overflows
    assert np.array_equal(np.isinf(y), inf), f"{name}: inf where the rounded reference is finite, or back, at " \
                                             f"{x[np.isinf(y) != inf][:4]}"
    err = ulp_err(y[~inf], ref[~inf])
    i = int(np.argmax(err))
    assert err[i] <= tol, f"{name}({x[~inf][i]!r}) = {y[~inf][i]!r}, reference {ref[~inf][i]!r}: {err[i]:.3f} ulp"


def test_sincos_accuracy_full_domain(shim, domain):
    kpi4 = (np.arange(0, 10431) * (np.pi / 4)).astype(np.float32)  # every k*pi/4 up to 8192
    x = np.concatenate([domain, windows(kpi4, 64)])
    x = x[np.abs(x) <= 8192]
    for name, fn in (("t_sin", np.sin), ("t_cos", np.cos)):
        y = run1(shim, name, x)
        ref = fn(x.astype(np.float64))
        small = np.abs(x) <= np.float32(np.pi)
        err = ulp_err(y[small], ref[small])
        assert err.max() <= 1.5, f"{name}({x[small][np.argmax(err)]!r}): {err.max():.3f} ulp"
        a = np.abs(y.astype(np.float64) - ref)
        assert a.max() <= 1e-7, f"{name}({x[np.argmax(a)]!r}): absolute error {a.max():.3g}"


def test_atan2_accuracy_grid(shim):
    g = 4096
    y = np.repeat(strided(g), g)
    x = np.tile(strided(g, 0x85EBCA77), g)
    ok = np.isfinite(x) & np.isfinite(y)
    y, x = np.ascontiguousarray(y[ok]), np.ascontiguousarray(x[ok])
    r = np.empty_like(x)
    shim.t_atan2(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), x.size)
    err = ulp_err(r, np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    i = int(np.argmax(err))
    assert err[i] <= 3.5, f"atan2({y[i]!r}, {x[i]!r}) = {r[i]!r}: {err[i]:.3f} ulp"


def run_d(shim, name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    getattr(shim, name)(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size)
    return y


def test_double_sincos_long_double(shim):
    n = 1 << 21
    i = np.arange(n, dtype=np.uint64)
    strided_d = ((i * np.uint64(0x9E3779B97F4A7C15)) % np.uint64(0x41D0000000000001)).view(np.float64)  # [0, 2^30]
    k = np.concatenate([np.arange(8192), np.arange(8192, 1367130551, 166880)])
    c = (k * (np.pi / 4)).view(np.uint64)[:, None] + np.arange(-16, 17, dtype=np.int64)[None, :].astype(np.uint64)
    kpi4 = c[c < np.uint64(0x41D0000000000001)].view(np.float64)  # k*pi/4 up to 2^30, +-16 ulps
    tiny = (np.arange(1 << 14, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) %
            np.uint64(0x3EB0000000000000)).view(np.float64)  # [0, 2^-20)
    x = np.concatenate([strided_d, kpi4, tiny])
    x = np.concatenate([x, -x])
    xl = x.astype(np.longdouble)
    for name, fn in (("t_sin_d", np.sin), ("t_cos_d", np.cos)):
        y = run_d(shim, name, x)
        ref = fn(xl)
        a = np.abs(y.astype(np.longdouble) - ref).astype(np.float64)
        assert a.max() <= 2.5e-16, f"{name}({x[np.argmax(a)]!r}): absolute error {a.max():.3g}"
        big = np.abs(ref) >= 2.0 ** -10  # away from the zeros the error is in ulps of the result
        u = a[big] / np.spacing(np.abs(ref[big].astype(np.float64)))
        assert u.max() <= 2.0, f"{name}({x[big][np.argmax(u)]!r}): {u.max():.3f} ulp"
    # tiny arguments: sin x = x, cos x = 1 exactly
    t = tiny[tiny < 2.0 ** -30]
    assert np.array_equal(run_d(shim, "t_sin_d", t), t) and np.all(run_d(shim, "t_cos_d", t) == 1.0)
    # the cut-off: 2^30 is served, above it both return 0 (x - x), inf and NaN give NaN
    two30 = 2.0 ** 30
    above = np.array([np.nextafter(two30, np.inf), 2.0 ** 31, 1e300, -np.nextafter(two30, np.inf)])
    for name, fn in (("t_sin_d", np.sin), ("t_cos_d", np.cos)):
        assert abs(run_d(shim, name, np.array([two30]))[0] - float(fn(np.longdouble(two30)))) <= 2.5e-16
        assert np.array_equal(run_d(shim, name, above), np.zeros(4))
        assert np.isnan(run_d(shim, name, np.array([np.inf, -np.inf, np.nan]))).all()


# ---- specials: exact expected results ----

def f32(*v):
    return np.array(v, np.float32)


def test_specials_exact(shim):
    nans = EDGE[np.isnan(EDGE)]
    for name in ("t_atan", "t_asin", "t_acos", "t_sin", "t_cos", "t_exp", "t_log", "t_floor", "t_round", "t_sqrt"):
        assert np.isnan(run1(shim, name, nans)).all(), f"{name}: NaN in must give NaN out"
    assert run1(shim, "t_exp", f32(-np.inf, np.inf)).tolist() == [0.0, np.inf]
    assert run1(shim, "t_log", f32(0.0, -0.0, np.inf)).tolist() == [-np.inf, -np.inf, np.inf]
    assert np.isnan(run1(shim, "t_log", f32(-1e-45, -1.0, -np.inf))).all()
    outside = f32(np.nextafter(np.float32(1), np.float32(2)), -np.nextafter(np.float32(1), np.float32(2)), 2.0, -np.inf,
                  np.inf)
    assert np.isnan(run1(shim, "t_asin", outside)).all() and np.isnan(run1(shim, "t_acos", outside)).all()
    assert run1(shim, "t_asin", f32(1.0, -1.0)).tolist() == [np.float32(np.pi / 2), -np.float32(np.pi / 2)]
    assert run1(shim, "t_acos", f32(1.0, -1.0)).tolist() == [0.0, np.float32(np.pi)]
    assert np.isnan(run1(shim, "t_sin", f32(np.nextafter(np.float32(8192), np.float32(9e3)), np.inf, -np.inf))).all()


def atan2(shim, y, x):
    y, x = np.broadcast_arrays(np.asarray(y, np.float32), np.asarray(x, np.float32))
    y, x = np.ascontiguousarray(y), np.ascontiguousarray(x)
    r = np.empty_like(x)
    shim.t_atan2(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), x.size)
    return r


def test_deliberate_conventions(shim):
    """Where the specification departs from C on purpose (GLSL leaves these open; the kernels, the GLSL prelude of
    oracle/glref.py and the recorded fixtures all follow them): pinned as they are."""
    pi = np.float32(np.pi)
    # atan2(-0, x < 0) = +pi (C: -pi): a point with y = -0 behind the sensor lands in column 0, not W - 1
    assert atan2(shim, f32(-0.0, 0.0), f32(-1.0, -1.0)).tolist() == [pi, pi]
    # atan2(+-0, +-0) = +0 (C: +-0 or +-pi)
    r = atan2(shim, f32(0.0, -0.0, 0.0, -0.0), f32(0.0, 0.0, -0.0, -0.0))
    assert r.view(np.uint32).tolist() == [0, 0, 0, 0]
    # atan2(+-inf, +-inf) = NaN (C: +-pi/4, +-3pi/4)
    assert np.isnan(atan2(shim, f32(np.inf, np.inf, -np.inf, -np.inf), f32(np.inf, -np.inf, np.inf, -np.inf))).all()
    # atan(-0) = +0, hence atan2(-0, x > 0) = +0 (C: -0)
    assert run1(shim, "t_atan", f32(-0.0)).view(np.uint32).tolist() == [0]
    assert atan2(shim, f32(-0.0), f32(1.0)).view(np.uint32).tolist() == [0]
    # the C quadrants everywhere else
    assert atan2(shim, f32(1.0, -1.0, 1.0, -1.0, 0.0, -0.0), f32(0.0, 0.0, -0.0, -0.0, 1.0, 1.0)).tolist() == \
        [np.float32(np.pi / 2), -np.float32(np.pi / 2), np.float32(np.pi / 2), -np.float32(np.pi / 2), 0.0, 0.0]
    assert atan2(shim, f32(np.inf, 1.0, -1.0), f32(1.0, -np.inf, -np.inf)).tolist() == [np.float32(np.pi / 2), pi, -pi]
    # floor(-0) = +0 (C: -0); round(-0) = +0 as well, round(-0.25) = -0
    assert run1(shim, "t_floor", f32(-0.0)).view(np.uint32).tolist() == [0]
    assert run1(shim, "t_round", f32(-0.0, -0.25)).view(np.uint32).tolist() == [0, 0x80000000]
