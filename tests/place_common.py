"""Shared by the place-recognition tests (test_place_shim.py, test_gpu_place.py): the host restatement
tests/place_shim.c, an independent NumPy restatement of the descriptor, scans turned about z, crafted descriptor
databases around the ties and empty columns of the specification (csrc/k_place.hip)."""
import ctypes as C
import os
import subprocess

import numpy as np

from semantic_suma_amd.types import PlaceMatch, PlaceParams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

f32 = np.float32
PI_F = f32(3.14159265358979323846)
TWO_PI = f32(2.0) * PI_F


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "place_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "include"), os.path.join(HERE, "place_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, u32, i32, cf, ci = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_int
    L.place_shim_describe.argtypes = [vp, vp, u32, ci, ci, cf, cf, vp, vp]
    L.place_shim_describe.restype = None
    L.place_shim_norms.argtypes = [vp, ci, ci, vp]
    L.place_shim_norms.restype = None
    L.place_shim_distance.argtypes = [vp, vp, vp, vp, ci, ci, C.POINTER(i32)]
    L.place_shim_distance.restype = cf
    L.place_shim_search.argtypes = [vp, vp, u32, vp, vp, ci, ci, vp, vp]
    L.place_shim_search.restype = None
    L.place_shim_yaw.argtypes = [i32, ci]
    L.place_shim_yaw.restype = cf
    L.place_shim_topk.argtypes = [vp, vp, vp, u32, u32, u32, u32, ci, vp]
    L.place_shim_topk.restype = u32
    L.place_shim_hypothesis.argtypes = [vp, cf, vp]
    L.place_shim_hypothesis.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def shim_describe(shim, vertex, semantic, pp: PlaceParams):
    """-> cells (S, R) of a vertex / semantic map pair (any shape x 4)"""
    v = np.ascontiguousarray(vertex, dtype=np.float32).reshape(-1, 4)
    s = np.ascontiguousarray(semantic, dtype=np.float32).reshape(-1, 4)
    keep = np.frombuffer(bytes(pp.keep_label), dtype=np.uint8).copy()
    cells = np.full((pp.sectors, pp.rings), -1.0, dtype=np.float32)
    shim.place_shim_describe(_p(v), _p(s), v.shape[0], pp.rings, pp.sectors, pp.max_range, pp.height_offset, _p(keep),
                             _p(cells))
    return cells


def shim_norms(shim, cells):
    cells = np.ascontiguousarray(cells, dtype=np.float32)
    S, R = cells.shape[-2:]
    flat = cells.reshape(-1, S, R)
    out = np.zeros((flat.shape[0], S), dtype=np.float32)
    for e in range(flat.shape[0]):
        shim.place_shim_norms(_p(flat[e]), S, R, _p(out[e]))
    return out.reshape(cells.shape[:-1])


def shim_search(shim, db_cells, q_cells):
    """-> (dist (N,) fp32, shift (N,) int32); the norms are the shim's own"""
    db = np.ascontiguousarray(db_cells, dtype=np.float32)
    q = np.ascontiguousarray(q_cells, dtype=np.float32)
    N, S, R = db.shape
    dn, qn = shim_norms(shim, db), shim_norms(shim, q)
    dist, shift = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.int32)
    shim.place_shim_search(_p(db), _p(dn), N, _p(q), _p(qn), S, R, _p(dist), _p(shift))
    return dist, shift


def shim_topk(shim, dist, shift, ids, k, S, exclude=None):
    """-> list of dicts as core.PlaceIndex.queryFrame gives them"""
    lo, hi = (1, 0) if exclude is None else exclude
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    shift = np.ascontiguousarray(shift, dtype=np.int32)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    out = (PlaceMatch * max(k, 1))()
    n = shim.place_shim_topk(_p(dist), _p(shift), _p(ids), dist.shape[0], lo, hi, k, S, out)
    return [out[i].as_dict() for i in range(n)]


def shim_hypothesis(shim, T, yaw):
    """T . Rz(yaw) in the library's operation order; row-major in and out"""
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T)
    out = np.zeros((4, 4), dtype=np.float64)
    shim.place_shim_hypothesis(_p(Tc), float(yaw), _p(out))
    return out.T.copy()


def matches_equal(a, b, where=""):
    """two match lists equal to the bit"""
    assert len(a) == len(b), (where, len(a), len(b))
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x["index"], x["id"], x["shift"]) == (y["index"], y["id"], y["shift"]), (where, k, x, y)
        for f in ("distance", "yaw"):
            assert f32(x[f]).tobytes() == f32(y[f]).tobytes(), (where, k, f, x, y)


# ---- an independent restatement of the descriptor in NumPy (vectorised; fp32 throughout)

def _ma(a, b, c):
    """a * b + c with one rounding: the product of two floats is exact in a double"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def np_atan(xx):
    x = np.abs(xx)
    big, mid = x > f32(2.414213562373095), x > f32(0.4142135623730950)
    with np.errstate(all="ignore"):
        xr = np.where(big, -(f32(1.0) / x), np.where(mid, (x - f32(1.0)) / (x + f32(1.0)), x)).astype(np.float32)
    y = np.where(big, f32(1.57079632679489661923), np.where(mid, f32(0.78539816339744830962), f32(0.0))).astype(np.float32)
    z = xr * xr
    k = lambda v: np.full_like(z, f32(v))  # noqa: E731
    p = _ma(k(8.05374449538e-2), z, k(-1.38776856032e-1))
    p = _ma(p, z, k(1.99777106478e-1))
    p = _ma(p, z, k(-3.33329491539e-1))
    p = _ma(p * z, xr, xr)
    y = y + p
    return np.where(xx < 0, -y, y).astype(np.float32)


def np_atan2(y, x):
    with np.errstate(all="ignore"):
        z = np_atan(y / x)
    z = np.where(x < 0, np.where(y < 0, z - PI_F, z + PI_F), z).astype(np.float32)
    zero = np.where(y > 0, f32(1.57079632679489661923), np.where(y < 0, -f32(1.57079632679489661923), f32(0.0)))
    return np.where(x == 0, zero, z).astype(np.float32)


def numpy_describe(vertex, semantic, pp: PlaceParams):
    v = np.asarray(vertex, dtype=np.float32).reshape(-1, 4)
    s = np.asarray(semantic, dtype=np.float32).reshape(-1, 4)
    R, S = pp.rings, pp.sectors
    keep = np.frombuffer(bytes(pp.keep_label), dtype=np.uint8) != 0
    with np.errstate(all="ignore"):
        t = s[:, 0] * f32(255.0) + f32(0.5)
        label = np.where((t >= 0) & (t < 260), t, 0).astype(np.int64)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        d = np.sqrt(x * x + y * y)
        ok = (v[:, 3] > 0) & keep[label] & (d > 0) & (d < f32(pp.max_range))
        x, y, z, d = x[ok], y[ok], z[ok], d[ok]
        ring = np.minimum((d * (f32(R) / f32(pp.max_range))).astype(np.int64), R - 1)
        a = np_atan2(y, x)
        a = np.where(a < 0, a + TWO_PI, a).astype(np.float32)
        sector = np.minimum((a * (f32(S) / TWO_PI)).astype(np.int64), S - 1)
        h = z + f32(pp.height_offset)
    ok = (h > 0) & (h <= f32(1000.0))
    cells = np.zeros((S, R), dtype=np.float32)
    np.maximum.at(cells, (sector[ok], ring[ok]), h[ok])
    return cells


# ---- scans and poses turned about z

def turn_angle(turn, S, extra_deg=0.0):
    return turn * (2.0 * np.pi / S) + np.deg2rad(extra_deg)


def turned_scan(scan, theta):
    """the scan a sensor turned by +theta about its z axis sees: the points turned by -theta"""
    pts, lab, prob = scan
    c, s = np.cos(-theta), np.sin(-theta)
    out = np.array(pts, dtype=np.float32, copy=True)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    out[:, 0], out[:, 1] = c * x - s * y, s * x + c * y
    return out, lab, prob


def turned_pose(T, theta):
    Rz = np.eye(4)
    Rz[:2, :2] = [[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]]
    return np.asarray(T, dtype=np.float64) @ Rz


def yaw_difference(A, B):
    """the angle about z between two poses' headings, in (-pi, pi]"""
    R = np.asarray(A)[:3, :3].T @ np.asarray(B)[:3, :3]
    return float(np.arctan2(R[1, 0], R[0, 0]))


# ---- crafted descriptor databases

def crafted_database(n, S, R, seed=5):
    """n entries: random heights with empty cells and empty columns, every third entry a copy of an earlier one (ties
    in distance), every seventh all zero, every fifth a single column"""
    rng = np.random.RandomState(seed + 1000 * n + S + R)
    db = np.zeros((n, S, R), dtype=np.float32)
    for e in range(n):
        if e % 7 == 6:
            continue
        if e % 3 == 2 and e > 2:
            db[e] = db[rng.randint(0, e - 1)]
            continue
        c = rng.uniform(0.05, 30.0, (S, R)).astype(np.float32)
        c[rng.uniform(size=(S, R)) < 0.3] = 0.0
        c[rng.uniform(size=S) < 0.2] = 0.0
        if e % 5 == 4:
            keep = rng.randint(0, S)
            col = c[keep].copy()
            col[0] = max(col[0], f32(1.0))
            c[:] = 0.0
            c[keep] = col
        db[e] = c
    return db


def crafted_query(db, S, R, seed=11):
    """an entry of the database rolled by a few sectors with a little noise: near ties, exact ties on the copies"""
    rng = np.random.RandomState(seed + db.shape[0])
    q = np.roll(db[0], 3 % S, axis=0).copy()
    q[q > 0] += rng.uniform(0.0, 0.5, int((q > 0).sum())).astype(np.float32)
    return q.astype(np.float32)


# ---- hand-made vertex maps around every boundary of the descriptor

def hand_made_maps(W, H):
    """R = 4, S = 8, max_range = 8, height_offset = 2: ring edges at d = 2, 4, 6 (the scale is exactly 0.5), sector edges
    at multiples of pi / 4.  -> (params, vertex, semantic (label 40 everywhere), the texels' flat positions)"""
    pp = PlaceParams.defaults(rings=4, sectors=8, max_range=8.0, height_offset=2.0)
    up = lambda x: np.nextafter(f32(x), f32(np.inf))    # noqa: E731
    down = lambda x: np.nextafter(f32(x), f32(-np.inf))  # noqa: E731
    texels = [
        (2.0, 0.0, 1.0, 1.0),            # d on a ring edge: ring 1, sector 0, h = 3
        (down(2.0), 0.0, 7.0, 1.0),      # just inside ring 0
        (0.0, 4.0, 1.5, 1.0),            # d = 4: ring 2; x = 0: the angle is pi / 2
        (-6.0, 0.0, 0.5, 1.0),           # d = 6: ring 3; the angle pi on a sector edge
        (8.0, 0.0, 5.0, 1.0),            # d = max_range: left out
        (down(8.0), 0.0, 0.25, 1.0),     # the last d inside: ring 3
        (0.0, 0.0, 5.0, 1.0),            # d = 0: left out
        (1.0, 1.0, 1.0, 1.0), (-1.0, 1.0, 1.0, 1.0), (-1.0, -1.0, 1.0, 1.0), (1.0, -1.0, 1.0, 1.0),  # the diagonals
        (3.0, -1e-7, 2.0, 1.0),          # just below 2 pi: the sector index is clamped to S - 1
        (3.0, -1e-30, 2.5, 1.0),
        (5.0, 0.5, -2.0, 1.0),           # h = 0: left out
        (5.0, 0.5, down(-2.0), 1.0),     # h < 0
        (5.0, 0.6, up(-2.0), 1.0),       # the least h > 0 (same cell as the two above)
        (0.5, 5.0, 998.0, 1.0),          # h = 1000: kept
        (0.5, 5.1, up(1000.0) - f32(2.0), 1.0),  # the next float above 1000: left out (same cell)
        (-3.0, -2.0, 4.0, 1.0), (-3.1, -2.0, 9.0, 1.0), (-3.0, -2.1, 6.0, 1.0),  # one cell: the max wins
        (1.0, 2.5, 50.0, 0.0),           # w = 0: ignored
        (1.0, 2.5, 60.0, -1.0),
        (-0.0, 3.0, 1.0, 1.0), (1.0, -0.0, 1.25, 1.0), (-0.0, -0.0, 3.0, 1.0), (-5.0, -0.0, 1.0, 1.0),
        (np.nan, 1.0, 1.0, 1.0), (1.0, np.nan, 1.0, 1.0), (1.0, 1.5, np.nan, 1.0), (1.0, 1.0, 1.0, np.nan),
        (np.inf, 1.0, 1.0, 1.0), (1.0, -np.inf, 1.0, 1.0), (2.0, 2.5, np.inf, 1.0), (1e30, 1.0, 1.0, 1.0),
        (1.0, 1e30, 1.0, 1.0), (2.5, 2.0, 1e30, 1.0), (2.5, 2.0, -1e30, 1.0),
    ]
    v = np.zeros((H, W, 4), f32)
    flat = v.reshape(-1, 4)
    # scattered over the image, so that several blocks and both ends of the grid-stride loop hold some
    at = (np.arange(len(texels)) * 79 + 3) % (W * H)
    assert len(set(at.tolist())) == len(texels)
    with np.errstate(all="ignore"):
        flat[at] = np.array(texels, dtype=np.float64).astype(f32)
    s = np.zeros((H, W, 4), f32)
    s[..., 0] = f32(40.0) / f32(255.0)
    s[..., 3] = 1.0
    return pp, v, s, at


def check_hand_made_cells(cells):
    """what the specification says about hand_made_maps, by hand: cell[sector][ring]"""
    up = np.nextafter(f32(-2.0), f32(np.inf))
    assert cells[0, 1] == f32(3.0) and cells[0, 0] == f32(9.0)        # d = 2 is ring 1, the float below it ring 0
    assert cells[2, 2] == f32(3.5) and cells[2, 1] == f32(3.0)         # x = +-0, y > 0: pi / 2, the start of sector 2
    assert cells[4, 3] == f32(2.5) and cells[4, 2] == f32(3.0)         # y = +-0, x < 0: pi, the start of sector 4
    assert cells[0, 3] == f32(2.25)                                    # d just below max_range; d = max_range is not there
    assert cells[7, 1] == f32(4.5)                                     # both texels just below 2 pi
    assert cells[0, 2] == up + f32(2.0) and cells[0, 2] > 0            # only the least positive h of its cell
    assert cells[1, 2] == f32(1000.0)
    assert cells[4, 1] == f32(11.0)                                    # the max of three
    assert cells[1, 1] == 0                                            # w <= 0 texels are not there
    assert not np.isnan(cells).any() and cells.max() == f32(1000.0)
    assert int((cells > 0).sum()) == 15, np.argwhere(cells > 0)
