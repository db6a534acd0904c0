"""Shared by the tests of the per-scan objects (test_abi_objects.py, test_objects_host.py, test_gpu_objects.py): the host
restatement tests/object_shim.c of csrc/k_objects.hip, a plain Python restatement of it (breadth-first search over the
link graph, sums in Python integers), crafted frames on every boundary of the specification, and the measurements of
DESIGN.md 15's scenario -- mapped without cube 2 and building 41, scans 20-44 of the full world."""
import ctypes as C
import os
import subprocess
from collections import deque

import numpy as np

from semantic_suma_amd.types import OBJECT_COUNTS, ObjectCounts, ObjectParams, SCAN_OBJECT_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_FLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off"]
NONE = 0xffffffff
f32 = np.float32
ZERO = dict.fromkeys(OBJECT_COUNTS, 0)


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "object_shim.so")
    subprocess.check_call(["gcc"] + SHIM_FLAGS + ["-fPIC", "-shared", os.path.join(HERE, "object_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.object_shim_segment.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, vp, C.POINTER(ObjectParams), C.c_uint32, vp, vp,
                                      C.POINTER(ObjectCounts)]
    L.object_shim_segment.restype = None
    return L


def shim_segment(shim, V, S, flags, T, op: ObjectParams = None, scan_id=0):
    """V, S: H x W x 4; flags: H x W; T: row-major 4x4 -> (records, ids H x W, counts dict)"""
    op = ObjectParams.defaults() if op is None else op
    V, S = (np.ascontiguousarray(a, dtype=np.float32) for a in (V, S))
    H, W = V.shape[:2]
    fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(H, W)
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4).T)
    out = np.zeros(int(op.max_objects), dtype=SCAN_OBJECT_DTYPE)
    ids = np.zeros((H, W), dtype=np.uint32)
    cnt = ObjectCounts()
    shim.object_shim_segment(V.ctypes.data, S.ctypes.data, fl.ctypes.data, W, H, Tc.ctypes.data, C.byref(op), scan_id,
                             out.ctypes.data, ids.ctypes.data, C.byref(cnt))
    return out[:cnt.stored].copy(), ids, cnt.as_dict()


# ---- the specification once more in plain Python.  fp32 by numpy scalars; a fused multiply-add is the fp64 product (exact)
# plus the addend rounded once to fp32 -- exact whenever the fp64 sum is, which holds for the inputs of these tests: all
# coordinates and pose entries are multiples of 2^-6 below 2^10
def _fma(a, b, c):
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def _dot(a, b):
    return _fma(a[2], b[2], _fma(a[1], b[1], f32(a[0] * b[0])))


def _len(a):
    return np.sqrt(_dot(a, a))


def _point(P, m):
    """P: row-major 4x4 fp32"""
    return [f32(_fma(P[r, 2], m[2], _fma(P[r, 1], m[1], f32(P[r, 0] * m[0]))) + P[r, 3]) for r in range(3)]


def _below(a, b):
    return a < b or (a == b and np.signbit(a) and not np.signbit(b))


DYNAMIC = (10, 11, 13, 15, 18, 20, 30, 31, 32)


def _label(r):
    t = f32(f32(r * f32(255.0)) + f32(0.5))
    return int(t) if (t >= 0 and t < 260) else 0


def python_segment(V, S, flags, T, op: ObjectParams = None, scan_id=0):
    """-> (records, ids, counts) as shim_segment gives them"""
    op = ObjectParams.defaults() if op is None else op
    V, S = (np.ascontiguousarray(a, dtype=np.float32) for a in (V, S))
    H, W = V.shape[:2]
    fl = np.asarray(flags).reshape(-1)
    Vf, Sf = V.reshape(-1, 4), S.reshape(-1, 4)
    n_tex = W * H
    with np.errstate(all="ignore"):
        P = np.asarray(T, dtype=np.float64).reshape(4, 4).astype(np.float32)
        world = [_point(P, Vf[t, :3]) for t in range(n_tex)]
        rng = [_len(Vf[t, :3]) for t in range(n_tex)]
        member = [bool(fl[t] != 0 and Vf[t, 3] > f32(0.5) and np.all(np.isfinite(Vf[t, :3])) and np.all(np.isfinite(world[t])))
                  for t in range(n_tex)]
    base, slope = f32(op.link_base), f32(op.link_slope)

    def neighbours(t):
        tx, ty = t % W, t // W
        out = set()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y, x = ty + dy, (tx + dx) % W
                if 0 <= y < H and y * W + x != t:
                    out.add(y * W + x)
        return out

    def linked(a, b):
        a, b = min(a, b), max(a, b)
        with np.errstate(all="ignore"):
            d = _len([f32(Vf[a, k] - Vf[b, k]) for k in range(3)])
            return bool(d <= f32(base + f32(slope * min(rng[a], rng[b]))))

    seen, comps = set(), []
    for t in range(n_tex):
        if not member[t] or t in seen:
            continue
        seen.add(t)
        queue, comp = deque([t]), []
        while queue:
            a = queue.popleft()
            comp.append(a)
            for b in neighbours(a):
                if member[b] and b not in seen and linked(a, b):
                    seen.add(b)
                    queue.append(b)
        comps.append(sorted(comp))
    comps.sort(key=lambda c: c[0])
    counts = dict(n_texels=n_tex, n_members=sum(member), n_components=len(comps),
                  n_small=sum(len(c) < op.min_texels for c in comps))
    objs = [c for c in comps if len(c) >= op.min_texels]
    counts["n_objects"], counts["stored"] = len(objs), min(len(objs), int(op.max_objects))
    rec = np.zeros(counts["stored"], dtype=SCAN_OBJECT_DTYPE)
    ids = np.full(n_tex, NONE, dtype=np.uint32)
    lim = f32(2.0 ** 40)
    for k, comp in enumerate(objs[:counts["stored"]]):
        ids[comp] = k
        r = rec[k]
        r["root"], r["n_texels"], r["scan_id"] = comp[0], len(comp), scan_id
        sums, total, S3 = {}, 0, [0, 0, 0]
        for t in comp:
            L = _label(Sf[t, 0])
            pr = Sf[t, 3]
            c = f32(0.0) if not (pr > 0) else (f32(pr) if pr < 1 else f32(1.0))
            q = int(np.rint(f32(c * f32(65535.0))))
            sums[L] = sums.get(L, 0) + q
            total += q
            for a in range(3):
                S3[a] += int(np.rint(min(max(f32(world[t][a] * f32(1024.0)), -lim), lim)))
        if total:
            best = max(sums.values())
            r["label"] = min(L for L, s in sums.items() if s == best)
            r["prob"] = f32(best) / f32(total)
        else:
            r["label"], r["prob"] = _label(Sf[comp[0], 0]), 0.0
        r["n_dynamic"] = sum(1 for t in comp if float(f32(Sf[t, 0] * f32(255.0))) in DYNAMIC)
        for a in range(3):
            lo = hi = world[comp[0]][a]
            for t in comp[1:]:
                v = world[t][a]
                lo = v if _below(v, lo) else lo
                hi = v if _below(hi, v) else hi
            r["min"][a], r["max"][a] = lo, hi
            r["centroid"][a] = f32(float(S3[a]) / (float(len(comp)) * 1024.0))
        r["r_min"] = min(rng[t] for t in comp)
    return rec, ids.reshape(H, W), counts


# ---- crafted frames.  The specification does not look at the projection: a vertex image is any H x W x 4 array.  In
# loop_frame's the columns lie on a closed path, so that with LINK every image neighbour -- across the column seam too --
# links; which texels form components is then the flag image's 8-connectivity with wrapped columns
LINK = ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=1, max_objects=4096)
POSE = np.array([[0.0, -1.0, 0.0, 2.0], [1.0, 0.0, 0.0, -3.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])


def loop_frame(W, H, seed=1):
    """-> (V, S): neighbouring columns 1/8 m apart in x or y on a closed rectangle path, rows 1/8 m apart in z: every
    image neighbour is at most sqrt(3) / 8 < 0.25 m away, dyadic coordinates throughout"""
    V, S = np.zeros((H, W, 4), dtype=np.float32), np.zeros((H, W, 4), dtype=np.float32)
    half = (W + 1) // 2
    for tx in range(W):
        # out along x for the first half of the columns, back along the same line one step of y away
        x, y = (8.0 + tx / 8.0, 0.0) if tx < half else (8.0 + (W - 1 - tx) / 8.0, 0.125)
        for ty in range(H):
            V[ty, tx] = (x, y, ty / 8.0 - 1.0, 1.0)
    rng = np.random.RandomState(seed)
    S[..., 0] = (rng.choice([0, 10, 40, 50, 70, 259], (H, W)).astype(np.float32) / f32(255.0))
    S[..., 3] = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], dtype=np.float32), (H, W))
    return V, S


def serpentine(W, H):
    """one texel wide: full rows at even ty, joined at alternating ends through the odd rows; column W - 1 stays empty so
    that the rows do not close around the turn"""
    fl = np.zeros((H, W), dtype=np.uint8)
    fl[0::2, :W - 1] = 1
    for ty in range(1, H, 2):
        if ty + 1 < H:
            fl[ty, W - 2 if (ty // 2) % 2 == 0 else 0] = 1
    return fl


def spiral(W, H):
    """a rectangular spiral one texel wide with one empty texel between its turns"""
    fl = np.zeros((H, W), dtype=np.uint8)
    Wu = max(W - 1, 1)                        # column W - 1 stays empty: no link around the turn

    def free(x, y):
        return not (0 <= x < Wu and 0 <= y < H) or fl[y, x] == 0

    x, y, d, turns = 0, 0, 0, 0
    fl[0, 0] = 1
    while turns < 2:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d]
        nx, ny = x + dx, y + dy
        if 0 <= nx < Wu and 0 <= ny < H and fl[ny, nx] == 0 and free(nx + dx, ny + dy):
            x, y, turns = nx, ny, 0
            fl[y, x] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return fl


def checkerboard(W, H):
    ty, tx = np.mgrid[0:H, 0:W]
    return ((tx + ty) % 2 == 0).astype(np.uint8)


def crafted_cases(W, H):
    """-> list of (name, V, S, flags, pose, params) at one image size, each on a rule of the specification"""
    V, S = loop_frame(W, H)
    rng = np.random.RandomState(W * 131 + H)
    out = []

    def add(name, flags, v=None, s=None, pose=POSE, op=LINK):
        out.append((name, V if v is None else v, S if s is None else s, np.ascontiguousarray(flags, dtype=np.uint8), pose, op))

    ones = np.ones((H, W), dtype=np.uint8)
    add("all_flags_one_component", ones)
    add("all_flags_zero", np.zeros((H, W), dtype=np.uint8))
    add("serpentine", serpentine(W, H))
    add("spiral", spiral(W, H))
    add("checkerboard", checkerboard(W, H))
    add("random_half", rng.rand(H, W) < 0.5, op=ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=3))
    add("random_sparse", (rng.rand(H, W) < 0.3) * 7, op=ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=2,
                                                                              max_objects=3))
    # no link at all: every member is its own component
    add("all_flags_no_link", ones, op=ObjectParams.defaults(link_base=0.0, link_slope=0.0, min_texels=1, max_objects=65536))
    add("min_texels_above_image", ones, op=ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=W * H + 1))
    # the seam: a run that crosses it, and a full row that meets itself around the turn
    fl = np.zeros((H, W), dtype=np.uint8)
    fl[0, [0, W - 1]] = 1
    if W > 4:
        fl[0, [1, W - 2]] = 1
    add("across_the_seam", fl)
    fl = np.zeros((H, W), dtype=np.uint8)
    fl[H - 1, :] = 1
    add("around_the_turn", fl)
    # non-members among the flagged: dv.w = 0 and 0.5, NaN and infinite points, each cutting a row in two
    v = V.copy()
    cuts = [(0, 0.0, None), (1, 0.5, None), (2, 1.0, np.nan), (3, 1.0, np.inf), (4, 1.0, -np.inf)]
    for k, w, bad in cuts:
        tx, ty = (3 + 5 * k) % W, k % H
        v[ty, tx, 3] = w
        if bad is not None:
            v[ty, tx, k % 3] = bad
    add("flagged_non_members", ones, v=v)
    # a pose whose fp32 translation overflows: no world position is finite, nothing is a member
    far = POSE.copy()
    far[0, 3] = 1e39
    add("pose_overflow", ones, pose=far)
    # +-0 in the box: x alternates between +0 and -0, y and z are not negative, and the pose's first row is (1, -0, -0, -0),
    # so that world x = fma(-0, z, fma(-0, y, 1 * x)) + -0 keeps the sign of x
    v = V.copy()
    v[..., 0] = np.where((np.arange(W)[None, :] + np.arange(H)[:, None]) % 2 == 0, f32(0.0), f32(-0.0))
    v[..., 1] = (np.minimum(np.arange(W), W - 1 - np.arange(W)) / 8.0)[None, :]
    v[..., 2] = (np.arange(H) / 8.0)[:, None]
    zero = np.eye(4)
    zero[0, 1:] = -0.0
    add("signed_zero_box", ones, v=v, pose=zero)
    return out


def threshold_case(W, H, near):
    """two runs adjacent in the image whose distance is the fp32 on either side of the link threshold: at x = 4 (near) or
    x = 512 (far), with link_base 0.25 and link_slope 2^-5 the threshold is 0.375 / 16.25 exactly.  Columns 0 .. 2 hold
    run A, columns 3 .. 5 run B at the threshold (linked), columns 8 .. 10 run C, 11 .. 13 run D one ulp beyond it"""
    op = ObjectParams.defaults(link_base=0.25, link_slope=0.03125, min_texels=1)
    x = f32(4.0) if near else f32(512.0)
    thr = f32(0.25) + f32(0.03125) * x
    V, S = np.zeros((H, W, 4), dtype=np.float32), np.zeros((H, W, 4), dtype=np.float32)
    S[..., 0], S[..., 3] = f32(40) / f32(255), 0.5
    fl = np.zeros((H, W), dtype=np.uint8)
    at = f32(x + thr)
    beyond = np.nextafter(at, f32(np.inf))
    for c0, xs in ((0, (x, x, x, at, at, at)), (8, (x, x, x, beyond, beyond, beyond))):
        for k, xv in enumerate(xs):
            V[0, c0 + k] = (xv, 0.0, 0.0, 1.0)
            fl[0, c0 + k] = 1
    return V, S, fl, np.eye(4), op


def sized_components(W, H, min_texels):
    """runs of min_texels - 1, min_texels and min_texels + 1 texels in rows 0, 2 (and 0 again further right)"""
    V, S = loop_frame(W, H)
    fl = np.zeros((H, W), dtype=np.uint8)
    x = 1
    for n in (min_texels - 1, min_texels, min_texels + 1):
        fl[0, x:x + n] = 1
        x += n + 2
    assert x < W - 1
    return V, S, fl, POSE, ObjectParams.defaults(link_base=0.25, link_slope=0.0, min_texels=min_texels)


# ---- the scenario (novel_common has the runs): building 41 is the second of the added boxes
def building_box():
    import change_common as cc
    return cc.removed_boxes()[1]


def inside_box(xyz, box, inflate):
    """bool per world-map position: inside the box grown by ``inflate`` (change_common.inside_boxes for bare positions)"""
    from semantic_suma_amd import synth
    T0 = synth.trajectory_pose(0)
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3) @ T0[:3, :3].T + T0[:3, 3]
    c, h, yaw = box
    cs, sn = np.cos(yaw), np.sin(yaw)
    Rb = np.array([[cs, sn, 0], [-sn, cs, 0], [0, 0, 1]])
    return np.all(np.abs((p - c) @ Rb.T) <= h + inflate, axis=1)


def scan_measure(rec, ids, V, flags, T):
    """one scan's objects against building 41 -> (has an object whose centroid lies in the grown box, the share of the
    novel texels inside the grown box that belong to the largest such object -- None when the scan has no such texel)"""
    box = building_box()
    H, W = ids.shape
    Tm = np.asarray(T, dtype=np.float64).reshape(4, 4)
    world = V.reshape(-1, 4)[:, :3].astype(np.float64) @ Tm[:3, :3].T + Tm[:3, 3]
    with np.errstate(all="ignore"):
        novel_in = (np.asarray(flags).reshape(-1) != 0) & inside_box(np.nan_to_num(world), box, 0.3)
    hit = inside_box(rec["centroid"], box, 0.3) if len(rec) else np.zeros(0, dtype=bool)
    if not hit.any():
        return False, (0.0 if novel_in.any() else None)
    k = int(np.nonzero(hit)[0][np.argmax(rec["n_texels"][hit])])
    share = float(((ids.reshape(-1) == k) & novel_in).sum()) / max(1, int(novel_in.sum()))
    return True, share


# what tests/object_shim.c measured on the CPU restatement of the localiser (novel_common.host_run) with the default
# parameters: of the 25 scans, those with an object whose centroid lies inside building 41's box grown by
# 0.3 m; the smallest per-scan share of the novel texels inside that box that the largest such object holds, over those
# scans; the greatest number of objects a scan of the control run (same world mapped and localised) has
MEASURED = dict(scans_with_building=25, min_share=0.171946, control_objects=2)


def check_measured(scans_with_building, min_share, control_objects):
    """the issue's conditions"""
    assert scans_with_building > 0 and scans_with_building >= 0.5 * MEASURED["scans_with_building"], (scans_with_building, MEASURED)
    assert min_share >= 0.5 * MEASURED["min_share"], (min_share, MEASURED)
    assert control_objects <= max(2 * MEASURED["control_objects"], 5), (control_objects, MEASURED)
