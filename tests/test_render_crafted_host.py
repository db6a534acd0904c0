"""K4 + K5 (+ the K7 splat) on crafted surfel maps, CPU side: pins the oracle (oracle/o_map.c) against a plain fp64
statement of surfel rendering (tests/render_ref.py), proves each structural row's precondition, and fixes the inputs
that tests/test_gpu_render_crafted.py runs through k_render.hip.

A. Room scenes against fp64 (ROOM_IDS): one surfel per texel of k6_ref's analytic room, ranges spread by +-30 % and
   normals tilted by up to 12 degrees in fixed low-discrepancy patterns, creation stamps over four non-identity pose-table
   entries, timestamp 150 (thr = 50) with stamps on both sides; the left quarter of the columns is old only and a band in
   the middle is never drawn, so K5 takes each of its branches.  Each scene makes three calls: a merged render, an
   unmerged render (pose_new moved on) and render_composed.

   A pixel is DECIDED when its three margins (render_ref.raster_fp64) exceed bounds measured against the ORACLE, never the
   kernel: EPS_PX = 1/512 px (the snapping half step) + 2 max|oracle corner - fp64 corner| from ora_debug_render_quads;
   EPS_Z = 2^-23 + 2 max|corner depth difference| (and, per pixel, + EPS_PX * the two fragments' depth slopes: a corner
   that moves takes the interpolated depth with it); EPS_DISC = 6 EPS_PX / (the quad's narrowest extent in pixels).
   Conditions on a scene (a scene that misses one is changed, never the cap): at most 2 % of the pixels any quad box
   touches are undecided, in every rendering of every call; quads of 3 to 40 px; every named pixel decided.
   Checked on decided pixels: the winner ids equal fp64's; positions and normals are within 8 * 2^-24 * sum|terms|.

   measured with the CPU oracle (EPS_DISC: the scene's largest; decided: the scene's worst rendering; |x - fp64| / u: the
   worst position / normal component in units of 2^-24 sum|terms|, bound 8):

       scene                         EPS_PX [px]  EPS_DISC   EPS_Z      decided   |x-fp64|/u  K5 pixels new / old / neither
       room48x12-identity-compose1   0.001966     0.01529    1.948e-07  98.78 %   1.80        (43, 5) / (0, 6) / (26, 6)
       room48x12-identity-compose0   0.001966     0.01529    1.948e-07  99.12 %   1.80        -
       room48x12-moved-compose1      0.001965     0.01593    1.909e-07  98.94 %   1.51        (43, 5) / (6, 6) / (29, 6)
       room48x12-moved-compose0      0.001965     0.01593    1.909e-07  98.94 %   1.51        -
       room64x16-identity-compose1   0.001971     0.01059    1.849e-07  98.42 %   1.74        (59, 7) / (1, 8) / (32, 8)
       room64x16-identity-compose0   0.001971     0.01059    1.849e-07  98.42 %   1.74        -
       room64x16-moved-compose1      0.001970     0.00861    1.906e-07  98.06 %   1.67        (61, 7) / (9, 8) / (35, 8)
       room64x16-moved-compose0      0.001970     0.00861    1.906e-07  98.06 %   1.52        -
       room333x10-identity-compose1  0.002038     0.01821    1.884e-07  98.28 %   2.00        (330, 4) / (0, 5) / (149, 5)
       room333x10-identity-compose0  0.002038     0.01821    1.884e-07  98.68 %   2.00        -
       room333x10-moved-compose1     0.002037     0.01855    1.873e-07  98.53 %   2.19        (0, 5) / (34, 5) / (166, 5)
       room333x10-moved-compose0     0.002037     0.01855    1.873e-07  98.76 %   2.19        -

   Two refinements of "the smallest distance to any outline edge of any quad whose box touches the pixel" were needed for
   ANY one-surfel-per-texel scene to reach 98 % (576 quads of 12 px perimeter put 4.7 % of 576 pixels within 1/512 px of
   an outline): a quad counts at a pixel only while it CONTENDS there (not behind the winner by a safe margin), and its
   outline only where the disc test is not already failed by a safe margin.  Both are stated and argued in
   render_ref.raster_fp64; neither looks at the oracle or the kernel.

B. Structural rows (ROW_IDS, BIG_IDS): compared with the oracle in bits on the GPU; here each row's precondition is proved
   and the oracle is held to what the row states (and to fp64 on decided pixels, where the row is geometric).
     size-S                     S = 0, 1, 255, 256, 257, 513 records (the 256-record tile edge); S = 0 between two maps
     tiles-empty-between-full   tiles of 256: old / back-facing / new / mixed, merged and unmerged, and tiles 0, 2 swapped
     batch-edges-T              one tile whose boxes sum to exactly T = 511, 512, 513, 1025 pixel tests (512 per trip)
     tie                        twins in different tiles, identical to the bit but for a doubled normal: lowest id wins
                                render / render_active / render_inactive, highest id render_composed, new over old there
     diagonal-once-*            a pixel centre exactly on the strip's shared diagonal is covered (once).  Two sizes; a
                                mirrored arrangement does not exist: u = normalize(n.y - n.z, -n.x, n.x) is fixed by
                                n = -x, and n by facing the sensor on the axis
     rim-exact                  pixel centres exactly on the rim, tu^2 + tv^2 == 1: drawn where the outline owns them
     seam                       quads across yaw +-180 degrees are drawn on their centre's side only
     big-box-2047 / 2048x1024   one quad of about 10^6 pixel tests (> 2^19) among 300 ordinary ones: the reciprocal row /
                                column split at the largest index the geometry allows, and the dividing BIG instantiation
     gates-*                    confidence at / one ulp above the threshold, use_stability 0, creation and stamp at
                                thr - 1 and thr, thr = -1, 0, 1, the front-face product at 0.0098 and 0.0102
     bad-*                      NaN / inf / zero in position, normal, radius; the sensor origin: nothing drawn or changed
     carry-nothing-over         repeats on one context equal the first run: the resolve leaves both z-buffers clear
     index map                  K7 on two of the maps, one with a data image of another size
"""
from functools import lru_cache

import numpy as np
import pytest

import k6_ref as K
import render_ref as R
from semantic_suma_amd.types import SURFEL_DTYPE, default_params

F32 = np.float32
CREATION_STAMPS = (3, 40, 60, 120)  # non-identity pose-table entries; 3, 40 are "old" at timestamp 150, 60, 120 "new"
TIMESTAMP = 150                     # thr = timestamp - 100 = 50
N_POSES = 256


# ---------------------------------------------------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------------------------------------------------
def rot(roll=0.0, pitch=0.0, yaw=0.0, t=(0.0, 0.0, 0.0)):
    """4 x 4 pose, angles in degrees, R = Rz(yaw) Ry(pitch) Rx(roll), rounded to fp32 as the stage receives it"""
    a, b, c = np.deg2rad([roll, pitch, yaw])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(F32).astype(np.float64)


def pose_table():
    P = np.tile(np.eye(4), (N_POSES, 1, 1))
    P[3] = rot(1.0, -2.0, 5.0, (0.5, 0.2, 0.05))
    P[40] = rot(-1.5, 0.5, -12.0, (2.0, -1.0, 0.1))
    P[60] = rot(0.5, 1.0, 30.0, (3.5, 1.5, -0.1))
    P[120] = rot(2.0, -1.0, -45.0, (-1.0, 2.5, 0.2))
    return P.astype(F32)


VIEW_I = np.eye(4)
VIEW_B = rot(2.0, -1.5, 21.3, (0.41, -0.29, 0.1))


def nudged(view):
    """pose_new of an unmerged render: the view a little further on"""
    return (view @ rot(0.3, -0.2, 1.0, (0.3, -0.1, 0.02))).astype(F32).astype(np.float64)


def params(W, H, **ov):
    base = dict(data_width=W, data_height=H, model_width=W, model_height=H, max_surfels=4096, max_poses=N_POSES)
    base.update(ov)
    return default_params(**base)


def make_records(p_world, n_world, radius, creation, timestamp, confidence=1.0, poses=None):
    """64-byte records of surfels given in the WORLD frame: stored in the frame of their creation pose (fp64 inverse,
    then rounded to fp32), payload (r, g, b, w) = (own index, 0, 0, 1)"""
    poses = pose_table() if poses is None else poses
    p_world, n_world = np.atleast_2d(np.asarray(p_world, float)), np.atleast_2d(np.asarray(n_world, float))
    n = p_world.shape[0]
    creation = np.broadcast_to(np.asarray(creation), (n,)).astype(np.int64)
    rec = np.zeros(n, dtype=SURFEL_DTYPE)
    Pc = poses.astype(np.float64)[creation]
    Rc, tc = Pc[:, :3, :3], Pc[:, :3, 3]
    pl = np.einsum("nji,nj->ni", Rc, p_world - tc)
    nl = np.einsum("nji,nj->ni", Rc, n_world)
    rec["x"], rec["y"], rec["z"] = pl.T
    rec["nx"], rec["ny"], rec["nz"] = nl.T
    rec["radius"] = np.broadcast_to(radius, (n,))
    rec["confidence"] = np.broadcast_to(confidence, (n,))
    rec["timestamp"] = np.broadcast_to(np.asarray(timestamp), (n,)).astype(np.uint32)
    rec["weight"] = 1.0
    rec["count"] = creation
    return number(rec)


def world(rec, poses=None):
    """(positions, normals) of records in the world frame, fp64"""
    P = (pose_table() if poses is None else poses).astype(np.float64)[rec["count"].astype(int)]
    p = np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float64)
    n = np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float64)
    return np.einsum("nij,nj->ni", P[:, :3, :3], p) + P[:, :3, 3], np.einsum("nij,nj->ni", P[:, :3, :3], n)


def number(rec, first=0):
    rec["r"] = np.arange(first, first + len(rec), dtype=np.float32)
    rec["g"], rec["b"], rec["w"] = 0.0, 0.0, 1.0
    return rec


def pixel_angle(p):
    """radians per pixel, the larger of the two axes"""
    fov = np.deg2rad(abs(p.model_fov_up) + abs(p.model_fov_down))
    return max(2 * np.pi / p.model_width, fov / p.model_height)


def direction(p, x, y):
    """unit ray through window position (x, y) [pixels] of the model image"""
    fov_up, fov = abs(p.model_fov_up), abs(p.model_fov_up) + abs(p.model_fov_down)
    yaw = np.pi * (1.0 - 2.0 * np.asarray(x, float) / p.model_width)
    elev = np.deg2rad(fov_up - (1.0 - np.asarray(y, float) / p.model_height) * fov)
    return np.stack([np.cos(elev) * np.cos(yaw), np.cos(elev) * np.sin(yaw), np.sin(elev)], axis=-1)


def shell(p, n, seed, px=3.0, columns=(0.03, 0.97)):
    """n ordinary surfels around the origin: 4 .. 30 m away, facing the sensor within 40 degrees, quads about `px`
    pixels along the coarser image axis; creation stamps over all four pose-table entries, stamps on both sides of 50"""
    rng = np.random.default_rng(seed)
    W, H = p.model_width, p.model_height
    d = direction(p, rng.uniform(columns[0] * W, columns[1] * W, n), rng.uniform(0.08 * H, 0.92 * H, n))
    depth = rng.uniform(4.0, 30.0, n)
    tilt = rng.normal(size=(n, 3)) * 0.35
    nrm = -d + tilt - np.sum(tilt * d, axis=1, keepdims=True) * d
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    creation = np.asarray(CREATION_STAMPS)[rng.integers(0, 4, n)]
    ts = np.where(creation < 50, creation + np.where(rng.integers(0, 3, n) == 0, 70, 5), creation + 10)
    return make_records(depth[:, None] * d, nrm, 0.5 * px * depth * pixel_angle(p), creation, ts)


# ---------------------------------------------------------------------------------------------------------------------
# scenes: dict(id, params, poses, records, timestamp, calls); a call is (kind, pose_a, pose_b, conf_threshold)
# ---------------------------------------------------------------------------------------------------------------------
def scene(id, p, records, calls, timestamp=TIMESTAMP, poses=None, **more):
    records.setflags(write=False)
    return dict(id=id, params=p, poses=pose_table() if poses is None else poses, records=records, timestamp=timestamp,
                calls=calls, **more)


def usual_calls(view, ct=0.0):
    """merged render, unmerged render, then the three single-target calls"""
    return [("render", view, view, ct), ("render", view, nudged(view), ct), ("active", nudged(view), None, ct),
            ("inactive", view, None, ct), ("composed", view, nudged(view), ct)]


ROOM_SIZES = ((48, 12), (64, 16), (333, 10))
ROOM_IDS = [f"room{W}x{H}-{v}-compose{c}" for (W, H) in ROOM_SIZES for v in ("identity", "moved") for c in (1, 0)]


def room_records(p):
    """one surfel per texel of the analytic room (k6_ref.room_cast from the identity); ranges spread by +-30 % in a fixed
    low-discrepancy pattern so that neighbouring discs are not coplanar, normals tilted by up to 12 degrees; the left quarter of the columns is old only, a band in the middle
    is unstable (never drawn), the rest mixes the four creation stamps"""
    W, H = p.model_width, p.model_height
    pts, nrm, _ = K.room_cast(W, H, p, np.eye(4))
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    pts = pts * (0.7 + 0.6 * np.modf(0.7548776662 * ii + 0.5698402910 * jj)[0])[..., None]
    depth = np.linalg.norm(pts, axis=-1)
    # ... nor axis-parallel: a wall seen square on gives quads whose outlines run along whole pixel columns
    nrm = nrm + 0.25 * (np.stack([np.modf(0.8191725134 * ii + 0.6710436067 * jj)[0], np.modf(0.5497004779 * ii + 0.3819660113 * jj)[0],
                                  np.modf(0.4142135624 * ii + 0.7320508076 * jj)[0]], axis=-1) - 0.5)
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    f = ii / W
    creation = np.asarray(CREATION_STAMPS)[(ii + 2 * jj) % 4]
    creation = np.where(f < 0.25, np.where((ii + jj) % 2 == 0, 3, 40), creation)
    ts = np.where(creation < 50, creation + np.where((f >= 0.25) & ((ii * jj) % 3 == 0), 70, 5), creation + 10)
    conf = np.where((f > 0.42) & (f < 0.67), -1.0, 1.0)
    radius = 0.5 * 6.0 * depth * pixel_angle(p)
    return make_records(pts.reshape(-1, 3), nrm.reshape(-1, 3), radius.ravel(), creation.ravel(), ts.ravel(), conf.ravel())


@lru_cache(maxsize=None)
def get_scene(sid):
    return _SCENES[sid]()


def _room(W, H, view_name, compose):
    def build():
        p = params(W, H, compose_rendering=compose)
        view = VIEW_I if view_name == "identity" else VIEW_B
        calls = [("render", view, view, 0.0), ("render", view, nudged(view), 0.0), ("composed", view, nudged(view), 0.0)]
        return scene(f"room{W}x{H}-{view_name}-compose{compose}", p, room_records(p), calls)
    return build


_SCENES = {f"room{W}x{H}-{v}-compose{c}": _room(W, H, v, c) for (W, H) in ROOM_SIZES for v in ("identity", "moved")
           for c in (1, 0)}

# ---- structural rows -------------------------------------------------------------------------------------------------
SIZES = (0, 1, 255, 256, 257, 513)
for _S in SIZES:
    _SCENES[f"size-{_S}"] = (lambda S: lambda: scene(f"size-{S}", params(48, 12), shell(params(48, 12), 513, 11)[:S].copy(),
                                                    usual_calls(VIEW_B)))(_S)


def tiles_records(swapped):
    """four tiles of 256 records: old and visible / back-facing / new / mixed (swapped: new / back-facing / old / mixed)"""
    src = shell(params(48, 12), 1024, 23)
    t = np.arange(1024) // 256
    old_t, new_t = (2, 0) if swapped else (0, 2)
    creation = np.where(t == old_t, np.where(np.arange(1024) % 2 == 0, 3, 40), np.where(t == new_t, 60, src["count"].astype(int)))
    ts = np.where(t == old_t, creation + 5, np.where(t == new_t, 70, src["timestamp"].astype(int)))
    pw, nw = world(src)  # the surfels stay where they are in the world, whatever their stamps
    nw = np.where((t == 1)[:, None], -nw, nw)  # tile 1 looks away
    return make_records(pw, nw, src["radius"], creation, ts)


for _sw in (False, True):
    _SCENES["tiles-empty-between-full" + ("-swapped" if _sw else "")] = (lambda sw: lambda: scene(
        "tiles-empty-between-full" + ("-swapped" if sw else ""), params(48, 12), tiles_records(sw),
        [("render", VIEW_I, VIEW_I, 0.0), ("render", VIEW_I, nudged(VIEW_I), 0.0), ("composed", VIEW_I, nudged(VIEW_I), 0.0),
         ("render", VIEW_I, VIEW_I, 0.0)]))(_sw)


def snapped_boxes(p, corners01):
    """pixel tests per quad, from corners in [0,1]^3 (n x 4 x 3, float32): the 1/256-pixel snapping and the box of pixel
    centres as DESIGN.md "K4" states them -- floor(x * 256 + 0.5), centres at 256 i + 128, clipped to the image"""
    W, H = p.model_width, p.model_height
    c = np.asarray(corners01, dtype=F32)
    X = np.floor((c[..., 0] * F32(W)) * F32(256) + F32(0.5)).astype(np.int64)
    Y = np.floor((c[..., 1] * F32(H)) * F32(256) + F32(0.5)).astype(np.int64)
    i0, i1 = np.maximum((X.min(1) - 128 + 255) >> 8, 0), np.minimum((X.max(1) - 128) >> 8, W - 1)
    j0, j1 = np.maximum((Y.min(1) - 128 + 255) >> 8, 0), np.minimum((Y.max(1) - 128) >> 8, H - 1)
    return np.maximum(i1 - i0 + 1, 0) * np.maximum(j1 - j0 + 1, 0), X, Y


BATCH_TOTALS = (511, 512, 513, 1025)  # RENDER_BATCH * RENDER_THREADS = 512 tests per trip of phase 2


def batch_records(total):
    """a subset of one pool of new, visible surfels (at most one tile) whose boxes sum to exactly `total` tests: chosen
    from the fp64 corners, among quads none of whose corners lies within 0.02 px of a value that would change its box"""
    p = params(48, 12)
    src = shell(p, 400, 37)
    pool = make_records(*world(src), src["radius"], 60, 70)
    Q = R.quads_fp64(p, pose_table(), pool, VIEW_I)
    frac = np.abs((Q["xy"] - 0.5) - np.rint(Q["xy"] - 0.5))
    safe = Q["geometric"] & np.all(frac > 0.02, axis=(1, 2))
    xy = np.where(Q["geometric"][:, None, None], Q["xy"], 0.0)
    lo, hi = np.ceil(xy.min(1) - 0.5), np.floor(xy.max(1) - 0.5)
    w = np.clip(np.minimum(hi[:, 0], 47) - np.maximum(lo[:, 0], 0) + 1, 0, None)
    h = np.clip(np.minimum(hi[:, 1], 11) - np.maximum(lo[:, 1], 0) + 1, 0, None)
    tests = (w * h).astype(int)
    order = [i for i in np.argsort(-tests, kind="stable") if safe[i] and tests[i] > 0]
    # exact subset sum over at most 255 records, by dynamic programming on the totals
    reach = {0: []}
    for i in order:
        for s, chosen in list(reach.items()):
            s2 = s + int(tests[i])
            if s2 <= total and s2 not in reach and len(chosen) < 255:
                reach[s2] = chosen + [int(i)]
        if total in reach:
            break
    assert total in reach, f"no subset of the pool sums to {total}"
    return number(pool[sorted(reach[total])].copy())


for _T in BATCH_TOTALS:
    _SCENES[f"batch-edges-{_T}"] = (lambda T: lambda: scene(f"batch-edges-{T}", params(48, 12), batch_records(T),
                                                           [("render", VIEW_I, VIEW_I, 0.0), ("composed", VIEW_I, VIEW_I, 0.0)],
                                                           total=T))(_T)

# tie rows: (name, id of the first record, id of its twin, first is old?, twin is old?, window position).  A twin repeats
# its partner with the normal doubled: every product of the vertex stage and the tangent frame scale exactly by two, so
# the quads are identical to the bit (asserted) while the normal map says who won.
TIE_PAIRS = (("new-new", 5, 270, False, False, (6.5, 6.5)), ("old-old", 10, 600, True, True, (14.5, 5.5)),
             ("old-high-new-low", 20, 700, False, True, (22.5, 6.5)), ("old-low-new-high", 30, 650, True, False, (30.5, 5.5)))


def tie_records():
    """768 records: ordinary ones in the right-hand part of the image, four tied pairs alone on the left.  Creation
    stamps 3 (old) and 60 (new) are given ONE pose here, so that an old record and a new one can coincide to the bit."""
    p = params(48, 12)
    poses = pose_table()
    poses[60] = poses[3]
    src = shell(p, 768, 41, columns=(0.75, 0.97))
    c0 = src["count"].astype(int)
    rec = make_records(*world(src), src["radius"], np.where(c0 < 50, 40, 120), np.where(c0 < 50, 45, 130), poses=poses)
    for _, a, b, a_old, b_old, (x, y) in TIE_PAIRS:
        d = direction(p, x, y)
        one = make_records(8.0 * d, -d, 0.5 * 3.4 * 8.0 * pixel_angle(p), 3, 8, poses=poses)[0]
        for idx, old, scale in ((a, a_old, 1.0), (b, b_old, 2.0)):
            r = one.copy()
            r["count"], r["timestamp"] = (3.0, 8) if old else (60.0, 70)
            r["nx"], r["ny"], r["nz"] = F32(scale) * one["nx"], F32(scale) * one["ny"], F32(scale) * one["nz"]
            rec[idx] = r
    return number(rec), poses


def _tie():
    rec, poses = tie_records()
    calls = [("render", VIEW_I, VIEW_I, 0.0), ("active", VIEW_I, None, 0.0), ("inactive", VIEW_I, None, 0.0),
             ("composed", VIEW_I, VIEW_I, 0.0), ("render", VIEW_I, nudged(VIEW_I), 0.0)]
    return scene("tie", params(48, 12), rec, calls, poses=poses)


_SCENES["tie"] = _tie


def diagonal_params(W, H):
    return params(W, H, model_fov_up=10.0, model_fov_down=-10.0, data_fov_up=10.0, data_fov_down=-10.0)


DIAGONALS = {"diagonal-once-13x5": (13, 5, 6.0, 2.2), "diagonal-once-25x9": (25, 9, 9.0, 4.1)}  # W, H, range, radius
for _id in DIAGONALS:
    _SCENES[_id] = (lambda sid: lambda: scene(
        sid, diagonal_params(*DIAGONALS[sid][:2]),
        make_records([[DIAGONALS[sid][2], 0.0, 0.0]], [[-1.0, 0.0, 0.0]], DIAGONALS[sid][3], 0, 140,
                     poses=np.tile(np.eye(4, dtype=F32), (N_POSES, 1, 1))),
        [("render", VIEW_I, VIEW_I, 0.0), ("composed", VIEW_I, VIEW_I, 0.0)],
        poses=np.tile(np.eye(4, dtype=F32), (N_POSES, 1, 1))))(_id)


# rim-exact: the diamond of a surfel on the +x axis, sized so that the midpoints of its four outline edges -- where the disc
# touches the outline, tu^2 + tv^2 = 1 exactly (barycentric weights 1/2, 1/2, 0) -- are pixel centres: 65 columns, the
# corners 2 px left / right and 2 px above / below the centre pixel (32, 4).  render_surfels.frag discards on > 1 only.
RIM_W, RIM_H, RIM_RANGE = 65, 9, 6.0
RIM_ANGLE = 4.0 * np.pi / RIM_W                      # two columns
RIM_FOV = float(np.rad2deg(RIM_ANGLE * RIM_H / 4.0))  # fov_up = fov_down: two rows span RIM_ANGLE
RIM_MIDPOINTS = ((31, 5), (33, 5), (31, 3), (33, 3))


def rim_params():
    return params(RIM_W, RIM_H, model_fov_up=RIM_FOV, model_fov_down=-RIM_FOV, data_fov_up=RIM_FOV, data_fov_down=-RIM_FOV)


_SCENES["rim-exact"] = lambda: scene(
    "rim-exact", rim_params(),
    make_records([[RIM_RANGE, 0.0, 0.0]], [[-1.0, 0.0, 0.0]], RIM_RANGE * np.tan(RIM_ANGLE) / np.sqrt(2.0), 0, 140,
                 poses=np.tile(np.eye(4, dtype=F32), (N_POSES, 1, 1))),
    [("render", VIEW_I, VIEW_I, 0.0), ("composed", VIEW_I, VIEW_I, 0.0)], poses=np.tile(np.eye(4, dtype=F32), (N_POSES, 1, 1)))


def seam_records():
    """id 0 just on the +180 degree side (window x ~ 0.3), id 1 just on the -180 degree side (x ~ W - 0.3); 3 px quads"""
    p = params(48, 12)
    d = direction(p, np.array([0.3, 47.7]), np.array([6.5, 3.5]))
    return make_records(7.0 * d, -d, 0.5 * 3.2 * 7.0 * pixel_angle(p), [60, 3], [70, 8])


_SCENES["seam"] = lambda: scene("seam", params(48, 12), seam_records(), usual_calls(VIEW_I))

BIG_RADIUS = 30.0


def big_records(p):
    """300 ordinary surfels and, at id 150, one 2.05 m ahead on the x axis with a radius of 30 m: its quad spans 174
    degrees of yaw and every row"""
    rec = shell(p, 301, 53, px=9.0).copy()
    big = make_records([[2.05, 0.0, 0.0]], [[-1.0, 0.0, 0.0]], BIG_RADIUS, 60, 70)[0]
    rec[150] = big
    return number(rec)


for _W in (2047, 2048):
    _SCENES[f"big-box-{_W}x1024"] = (lambda W: lambda: scene(
        f"big-box-{W}x1024", params(W, 1024, data_width=48, data_height=12),
        big_records(params(W, 1024, data_width=48, data_height=12)), [("render", VIEW_I, VIEW_I, 0.0)]))(_W)

# gates: each probe surfel stands alone at its own column of a 48 x 12 image (row 6), 3 px wide
ULP_ABOVE_0_25 = float(np.nextafter(F32(0.25), F32(1)))
GATE_PROBES = (  # name, column, creation, timestamp, confidence, front-face dot (None: facing the sensor)
    ("conf-at-threshold", 3, 60, 70, 0.25, None), ("conf-one-ulp-above", 7, 60, 70, ULP_ABOVE_0_25, None),
    ("creation-thr-1", 11, 49, 49, 1.0, None), ("creation-thr", 15, 50, 50, 1.0, None),
    ("stamp-thr-1", 19, 10, 49, 1.0, None), ("stamp-thr", 23, 10, 50, 1.0, None),
    ("creation-0", 27, 0, 0, 1.0, None), ("creation-1", 31, 1, 1, 1.0, None),
    ("front-below", 35, 60, 70, 1.0, 0.0098), ("front-above", 39, 60, 70, 1.0, 0.0102),
    ("plain-new", 43, 120, 130, 1.0, None))
GATE_CONF = 0.25


def gate_records():
    p = params(48, 12)
    recs = []
    for _, col, creation, ts, conf, dot in GATE_PROBES:
        d = direction(p, col + 0.5, 6.5)
        n = -d
        if dot is not None:  # tilt the normal about the vertical until n . (-d) = dot
            side = np.cross(d, [0.0, 0.0, 1.0])
            side /= np.linalg.norm(side)
            n = dot * (-d) + np.sqrt(1.0 - dot * dot) * side
        recs.append(make_records(6.0 * d, n, 0.5 * 3.2 * 6.0 * pixel_angle(p), creation, ts, conf)[0])
    return number(np.array(recs, dtype=SURFEL_DTYPE))


def _gates(timestamp, use_stability):
    def build():
        return scene(f"gates-t{timestamp}-stability{use_stability}", params(48, 12, use_stability=use_stability),
                     gate_records(), usual_calls(VIEW_I, GATE_CONF), timestamp=timestamp)
    return build


GATE_SCENES = [(150, 1), (150, 0), (99, 1), (100, 1), (101, 1)]
for _t, _u in GATE_SCENES:
    _SCENES[f"gates-t{_t}-stability{_u}"] = _gates(_t, _u)

BAD_KINDS = ("nan-position", "inf-position", "nan-normal", "inf-normal", "nan-radius", "inf-radius", "zero-normal",
             "zero-radius", "at-origin")
BAD_AT = 100


def bad_records(kind):
    """300 good records (two tiles) with one bad record at id 100, placed where good ones are drawn; kind None: the same
    map WITHOUT that record (the payload keeps every other record's original index)"""
    p = params(48, 12)
    rec = shell(p, 300, 61).copy()
    if kind is None:
        return np.delete(rec, BAD_AT)
    b = rec[BAD_AT:BAD_AT + 1]
    b["count"], b["timestamp"] = 0.0, 140  # identity creation pose: the bad value reaches the stage as written
    d = direction(p, 24.5, 6.5)
    b["x"], b["y"], b["z"] = (6.0 * d).astype(F32)
    b["nx"], b["ny"], b["nz"] = (-d).astype(F32)
    b["radius"] = 0.5
    what, field = kind.split("-")
    val = dict(nan=np.nan, inf=np.inf, zero=0.0, at=0.0)[what]
    if field == "position":
        b["y"] = val
    elif field == "normal":
        b["nx"], b["ny"], b["nz"] = (val, val, val) if what == "zero" else (b["nx"][0], val, b["nz"][0])
    elif field == "radius":
        b["radius"] = val
    else:
        b["x"], b["y"], b["z"] = 0.0, 0.0, 0.0
    return rec


_SCENES["bad-none"] = lambda: scene("bad-none", params(48, 12), bad_records(None), usual_calls(VIEW_I))
for _k in BAD_KINDS:
    _SCENES[f"bad-{_k}"] = (lambda k: lambda: scene(f"bad-{k}", params(48, 12), bad_records(k), usual_calls(VIEW_I)))(_k)

BIG_IDS = ["big-box-2047x1024", "big-box-2048x1024"]  # 2 M pixels: run where they are used, never kept
ROW_IDS = [s for s in _SCENES if not s.startswith("room") and s not in BIG_IDS]
FP64_ROW_IDS = [s for s in ROW_IDS if not s.startswith("bad")]


# ---------------------------------------------------------------------------------------------------------------------
# running a scene on a backend (the oracle here, the kernel in the GPU file)
# ---------------------------------------------------------------------------------------------------------------------
class OracleSide:
    def __init__(self, lib, p):
        self.lib, self.o, self.p = lib, lib.Oracle(p), p

    def load(self, poses, records, timestamp):
        self.o.map_update_poses(poses)
        self.o.map_upload(records, timestamp)

    def call(self, c):
        kind, a, b, ct = c
        out = None
        if kind == "render":
            out = self.o.map_render(a, b, ct, self.o.frame(model=True))
        elif kind == "active":
            self.o.map_render_active(a, ct)
        elif kind == "inactive":
            self.o.map_render_inactive(a, ct)
        else:
            self.o.map_render_composed(a, b, ct)
        res = {nm: np.stack([self.o.map_frame(w).map(m).copy() for m in range(3)]) for w, nm in enumerate(FRAMES)}
        if out is not None:
            res["out"] = np.stack([out.map(m).copy() for m in range(3)])
        return res

    def index_map(self, pose):
        """one update of an all-invalid frame: K7 alone decides the index map"""
        self.o.map_update(pose, self.o.frame())
        return self.o.map_index_map()


FRAMES = ("old", "new", "composed")


def run_scene(side, sc):
    side.load(sc["poses"], sc["records"], sc["timestamp"])
    return [side.call(c) for c in sc["calls"]]


def assert_results_equal(got, want, what):
    """bit for bit, all three maps of old, new, composed and out, after every call"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.keys() == w.keys()
        for nm in g:
            ne = g[nm].view(np.uint32) != w[nm].view(np.uint32)
            assert not ne.any(), f"{what}: call {k} {nm}: {int(ne.sum())} words differ, first at (map, y, x, c) " \
                                 f"{np.argwhere(ne)[:4].tolist()}"


WRITES = {"render": (("old", 3), ("new", 3), ("out", 3)), "active": (("new", 2),), "inactive": (("old", 2),),
          "composed": (("composed", 2),)}


def written(results, calls):
    """only what each call itself writes (frame, leading maps): the other frames keep what earlier calls left there"""
    return [{nm: r[nm][:n] for nm, n in WRITES[c[0]]} for r, c in zip(results, calls)]


@lru_cache(maxsize=None)
def oracle_results(sid):
    """the oracle's frames of a scene, computed once and shared (read-only)"""
    from oracle import pyoracle
    pyoracle.build()
    sc = get_scene(sid)
    res = run_scene(OracleSide(pyoracle, sc["params"]), sc)
    for r in res:
        for a in r.values():
            a.setflags(write=False)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# fp64 expectation of a call, and the bounds measured against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def call_passes(sc, c):
    """{target frame: [(view pose, mode, thr), ..]} -- the passes a call draws into each of its depth buffers"""
    kind, a, b, ct = c
    thr = int(np.int32(np.uint32((sc["timestamp"] - 100) % 2 ** 32)))
    if kind == "render":
        if sc["params"].compose_rendering:
            return {"old": [(a, R.OLD, thr)], "new": [(b, R.NEW, thr)]}
        return {"out": [(a, R.NEW, 0)]}
    if kind == "active":
        return {"new": [(a, R.NEW, thr)]}
    if kind == "inactive":
        return {"old": [(a, R.OLD, thr)]}
    return {"composed": [(a, R.OLD, thr), (b, R.NEW, thr)]}


@lru_cache(maxsize=None)
def _quads(sid, view_key):
    sc = get_scene(sid)
    return R.quads_fp64(sc["params"], sc["poses"], sc["records"], np.frombuffer(view_key).reshape(4, 4))


def quads(sid, view):
    return _quads(sid, np.ascontiguousarray(view, dtype=np.float64).tobytes())


@lru_cache(maxsize=None)
def fp64_call(sid, k):
    """{target: dict(raster result, Q per pass)}; for a composing render also "out": (winner, source)"""
    sc = get_scene(sid)
    p, c = sc["params"], sc["calls"][k]
    res = {}
    for target, passes in call_passes(sc, c).items():
        qs = [quads(sid, view) for view, _, _ in passes]
        sel = [R.selected(p, sc["records"], mode, thr, c[3]) for _, mode, thr in passes]
        r = R.raster_fp64(p.model_width, p.model_height, list(zip(qs, sel)))
        r["Q"], r["sel"] = qs, sel
        res[target] = r
    if "old" in res and "new" in res:
        res["out"] = R.compose_fp64(res["old"], res["new"])
    return res


@lru_cache(maxsize=None)
def measured_eps(sid):
    """(EPS_PX, EPS_Z, largest corner difference [px], largest corner-depth difference) of a scene, from the ORACLE's
    corners (ora_debug_render_quads) against the fp64 corners, over every pass of every call; also asserts that the two
    emit the same surfels"""
    from oracle import pyoracle
    pyoracle.build()
    sc = get_scene(sid)
    p = sc["params"]
    o = pyoracle.Oracle(p)
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    dpx = dz = 0.0
    for c in sc["calls"]:
        for passes in call_passes(sc, c).values():
            for view, mode, thr in passes:
                emitted, corners, _ = o.debug_render_quads(view, c[3], mode, thr)
                Q = quads(sid, view)
                want = Q["geometric"] & R.selected(p, sc["records"], mode, thr, c[3])
                sure = ~(Q["finite"] & (Q["gate_margin"] < R.GATE_EPS))
                assert np.array_equal(emitted.astype(bool)[sure], want[sure]), f"{sid}: the oracle emits other surfels than fp64"
                e = emitted.astype(bool) & want
                if not e.any():
                    continue
                xw = (corners[e][..., 0] * F32(p.model_width)).astype(np.float64)
                yw = (corners[e][..., 1] * F32(p.model_height)).astype(np.float64)
                zw = (F32(0.5) * (F32(2.0) * corners[e][..., 2] - F32(1.0)) + F32(0.5)).astype(np.float64)
                dpx = max(dpx, float(np.max(np.abs(xw - Q["xy"][e][..., 0]))), float(np.max(np.abs(yw - Q["xy"][e][..., 1]))))
                dz = max(dz, float(np.max(np.abs(zw - Q["z"][e]))))
    return 1.0 / 512.0 + 2.0 * dpx, 2.0 ** -23 + 2.0 * dz, dpx, dz


def decided_mask(sid, r):
    eps_px, eps_z, _, _ = measured_eps(sid)
    return R.decided(r, eps_px, eps_z)


def semantic_ids(sem):
    """winner id per pixel from the payload (-1: no surfel); sem: H x W x 4"""
    return np.where(sem[..., 3] > 0.5, np.rint(sem[..., 0]).astype(np.int64), -1)


def check_against_fp64(sid, results, what):
    """winner ids (where the semantic map is written), positions and normals of every call against fp64, on decided
    pixels.  Returns the worst |x - fp64| / (2^-24 sum|terms|) seen."""
    sc = get_scene(sid)
    worst = 0.0
    for k, c in enumerate(sc["calls"]):
        ref = fp64_call(sid, k)
        targets = [t for t in ref if t != "out"]
        if c[0] == "render" and not sc["params"].compose_rendering:
            frames = {"out": ref["out"], "old": ref["out"], "new": ref["out"]}  # the single pass is copied to all three
        else:
            frames = {t: ref[t] for t in targets}
        for nm, r in frames.items():
            dec = decided_mask(sid, r)
            V, N, S = results[k][nm]
            win = r["winner"]
            has = dec & (win >= 0)
            none = dec & (win < 0)
            assert not V[none][:, 3].any() and not N[none][:, 3].any(), f"{what} call {k} {nm}: a surfel where fp64 has none"
            assert np.all(V[has][:, 3] == 1.0), f"{what} call {k} {nm}: no surfel where fp64 has one"
            if c[0] == "render":
                ids = semantic_ids(S)
                bad = dec & (ids != win)
                assert not bad.any(), f"{what} call {k} {nm}: winner ids differ from fp64 at (y, x) {np.argwhere(bad)[:5].tolist()}: " \
                                      f"{ids[bad][:5]} vs {win[bad][:5]}"
            # positions / normals of the winner, through the pose of the pass that drew it
            for pk, Q in enumerate(r["Q"]):
                m = has & (r["winner_pass"] == pk)
                w = win[m]
                for got, ref_v, terms in ((V, Q["pos"], Q["pos_terms"]), (N, Q["nrm"], Q["nrm_terms"])):
                    unit = 2.0 ** -24 * terms[w]
                    diff = np.abs(got[m][:, :3].astype(np.float64) - ref_v[w])
                    ratio = np.divide(diff, unit, out=np.where(diff > 0, np.inf, 0.0), where=unit > 0)
                    if ratio.size:
                        worst = max(worst, float(np.max(ratio)))
                    assert np.all(diff <= 8.0 * unit), f"{what} call {k} {nm}: |x - fp64| up to {np.max(ratio):.2f} x 2^-24 sum|terms|"
        if "out" in ref and sc["params"].compose_rendering and c[0] == "render":
            winner, source = ref["out"]
            dec = decided_mask(sid, ref["old"]) & decided_mask(sid, ref["new"])
            ids = semantic_ids(results[k]["out"][2])
            bad = dec & (ids != winner)
            assert not bad.any(), f"{what} call {k} composed output: ids differ from fp64 at {np.argwhere(bad)[:5].tolist()}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# A. room scenes against fp64
# ---------------------------------------------------------------------------------------------------------------------
# K5 branch pixels (x, y) of the merged render of every composing room scene: new rendering taken / old fills / neither
K5_PIXELS = {
    "room48x12-identity-compose1": {"new": (43, 5), "old": (0, 6), "neither": (26, 6)},
    "room48x12-moved-compose1": {"new": (43, 5), "old": (6, 6), "neither": (29, 6)},
    "room64x16-identity-compose1": {"new": (59, 7), "old": (1, 8), "neither": (32, 8)},
    "room64x16-moved-compose1": {"new": (61, 7), "old": (9, 8), "neither": (35, 8)},
    "room333x10-identity-compose1": {"new": (330, 4), "old": (0, 5), "neither": (149, 5)},
    "room333x10-moved-compose1": {"new": (0, 5), "old": (34, 5), "neither": (166, 5)},
}


def room_statistics(sid):
    """(undecided share among touched pixels, per call and target), quad extents"""
    sc = get_scene(sid)
    shares = []
    for k in range(len(sc["calls"])):
        for t, r in fp64_call(sid, k).items():
            if t == "out":
                continue
            dec = decided_mask(sid, r)
            n = int(np.count_nonzero(r["touched"]))
            shares.append(float(np.count_nonzero(r["touched"] & ~dec)) / max(n, 1))
    return shares


@pytest.mark.parametrize("sid", ROOM_IDS)
def test_room_scene_is_decided(oracle_lib, sid):
    """conditions on the scene itself: at most 2 % undecided among the touched pixels of every rendering, quads of 3 to
    40 px, stamps on both sides of the threshold over at least three non-identity poses, K5's three branches named"""
    sc = get_scene(sid)
    rec = sc["records"]
    used = np.unique(rec["count"].astype(int))
    assert len(used) >= 3 and not any(np.array_equal(sc["poses"][c], np.eye(4)) for c in used)
    assert (rec["count"] < 50).any() and (rec["count"] >= 50).any() and (rec["timestamp"] < 50).any() and (rec["timestamp"] >= 50).any()
    eps_px, eps_z, dpx, dz = measured_eps(sid)
    shares = room_statistics(sid)
    print(f"{sid}: EPS_PX {eps_px:.6f} (corner diff {dpx:.2e} px) EPS_Z {eps_z:.3e} (depth diff {dz:.2e}) "
          f"undecided share max {max(shares):.4f}")
    assert max(shares) <= 0.02, f"undecided shares {shares}"
    for view in {c[1].tobytes(): c[1] for c in sc["calls"]}.values():
        Q = quads(sid, view)
        e = Q["geometric"] & (rec["confidence"] > 0)
        ext = np.max(Q["xy"][e].max(1) - Q["xy"][e].min(1), axis=1)
        assert ext.min() >= 3.0 and ext.max() <= 40.0, f"quad extents {ext.min():.2f} .. {ext.max():.2f} px"
    if sc["params"].compose_rendering:
        ref = fp64_call(sid, 0)
        winner, source = ref["out"]
        dec = decided_mask(sid, ref["old"]) & decided_mask(sid, ref["new"])
        found = {}
        for s, nm in ((1, "new"), (0, "old"), (-1, "neither")):
            at = np.argwhere(dec & (source == s))
            found[nm] = tuple(int(v) for v in at[len(at) // 2][::-1]) if len(at) else None
        print(f"{sid}: K5 pixels {found}")
        for nm, s in (("new", 1), ("old", 0), ("neither", -1)):
            x, y = K5_PIXELS[sid][nm]
            assert dec[y, x] and source[y, x] == s, f"K5 pixel {nm} at ({x}, {y})"


@pytest.mark.parametrize("sid", ROOM_IDS)
def test_oracle_room_scene_against_fp64(oracle_lib, sid):
    worst = check_against_fp64(sid, oracle_results(sid), f"oracle {sid}")
    print(f"{sid}: worst |oracle - fp64| / (2^-24 sum|terms|) = {worst:.2f}")
    if get_scene(sid)["params"].compose_rendering:
        out = oracle_results(sid)[0]["out"]
        ids = semantic_ids(out[2])
        winner, source = fp64_call(sid, 0)["out"]
        for nm in ("new", "old", "neither"):
            x, y = K5_PIXELS[sid][nm]
            assert ids[y, x] == winner[y, x], f"K5 pixel {nm}"


# ---------------------------------------------------------------------------------------------------------------------
# B. structural rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", FP64_ROW_IDS)
def test_oracle_row_against_fp64(oracle_lib, sid):
    check_against_fp64(sid, oracle_results(sid), f"oracle {sid}")


def check_size_rows(results_of):
    """size-S: S = 0 renders all-zero frames; the other sizes draw something and repeat themselves"""
    for S in SIZES:
        res = results_of(f"size-{S}")
        drawn = sum(int(np.count_nonzero(r[nm][0][..., 3])) for r in res for nm in r)
        assert (drawn == 0) if S == 0 else (drawn > 0), f"size-{S}: {drawn} pixels drawn"
        if S == 0:
            assert all(not a.any() for r in res for a in r.values())


def test_size_rows(oracle_lib):
    check_size_rows(oracle_results)


def check_empty_map_between(side_factory):
    """S = 0 on a context that has rendered: all-zero frames, and the next render of another map is as if it were the first"""
    a = get_scene("size-257")
    first = written(run_scene(side_factory(a["params"]), a), a["calls"])
    side = side_factory(a["params"])
    assert_results_equal(written(run_scene(side, a), a["calls"]), first, "size-257")
    empty = get_scene("size-0")
    for r in written(run_scene(side, empty), empty["calls"]):
        assert all(not f.any() for f in r.values()), "S = 0 must render all-zero frames"
    assert_results_equal(written(run_scene(side, a), a["calls"]), first, "size-257 after S = 0")


def test_empty_map_between(oracle_lib):
    check_empty_map_between(lambda p: OracleSide(oracle_lib, p))


def check_tiles_rows(results_of):
    """tiles-empty-between-full: the merged render repeated after the unmerged calls equals the first; both the old and
    the new rendering draw something; swapping tiles 0 and 2 swaps what the two renderings see"""
    for sid in ("tiles-empty-between-full", "tiles-empty-between-full-swapped"):
        res = results_of(sid)
        assert_results_equal([res[3]], [{**res[0], "composed": res[3]["composed"]}], f"{sid}: merged render repeated")
        for k in (0, 1):
            assert res[k]["old"][0][..., 3].sum() > 20 and res[k]["new"][0][..., 3].sum() > 20
    a, b = get_scene("tiles-empty-between-full"), get_scene("tiles-empty-between-full-swapped")
    t = np.arange(1024) // 256
    for sc, old_t, new_t in ((a, 0, 2), (b, 2, 0)):
        rec = sc["records"]
        assert np.all(rec["count"][t == old_t] < 50) and np.all(rec["timestamp"][t == old_t] < 50)
        assert np.all(rec["count"][t == new_t] >= 50)
        Q = R.quads_fp64(sc["params"], sc["poses"], rec, VIEW_I)
        assert not Q["geometric"][t == 1].any() and Q["front"][t == 1].max() < -0.1, "tile 1 must be back-facing"
        assert Q["geometric"][t == old_t].sum() > 100 and Q["geometric"][t == new_t].sum() > 100
        assert 0 < (rec["count"][t == 3] < 50).sum() < 256


def test_tiles_rows(oracle_lib):
    check_tiles_rows(oracle_results)


@pytest.mark.parametrize("total", BATCH_TOTALS)
def test_batch_edges_precondition(oracle_lib, total):
    """the boxes of the tile, from the ORACLE's snapped corners, sum to exactly the stated number of pixel tests"""
    sc = get_scene(f"batch-edges-{total}")
    assert 0 < len(sc["records"]) <= 256
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    emitted, corners, _ = o.debug_render_quads(VIEW_I, 0.0, R.NEW, 50)
    assert emitted.all()
    tests, _, _ = snapped_boxes(sc["params"], corners)
    assert int(tests.sum()) == total


def tie_expectations():
    """[(call index, frame, (x, y), expected id, expected normal scale)] of the tie scene"""
    out = []
    for name, a, b, a_old, b_old, (x, y) in TIE_PAIRS:
        at = (int(x), int(y))
        olds = [i for i, o in ((a, a_old), (b, b_old)) if o]
        news = [i for i, o in ((a, a_old), (b, b_old)) if not o]
        scale = {a: 1.0, b: 2.0}
        if news:
            out += [(0, "new", at, min(news), scale[min(news)]), (1, "new", at, min(news), scale[min(news)])]
        if olds:
            out += [(0, "old", at, min(olds), scale[min(olds)]), (2, "old", at, min(olds), scale[min(olds)])]
        comp = max(news) if news else max(olds)  # GL_LEQUAL: the later primitive, and the new pass is the later pass
        out.append((3, "composed", at, comp, scale[comp]))
    return out


def check_tie_rows(results):
    sc = get_scene("tie")
    Q = R.quads_fp64(sc["params"], sc["poses"], sc["records"], VIEW_I)
    for k, frame, (x, y), want_id, want_scale in tie_expectations():
        V, N, S = results[k][frame]
        assert V[y, x, 3] == 1.0, f"tie: call {k} {frame} ({x}, {y}) is empty"
        if sc["calls"][k][0] == "render":
            assert int(round(float(S[y, x, 0]))) == want_id, f"tie: call {k} {frame} ({x}, {y}): id {S[y, x, 0]} != {want_id}"
        n = Q["nrm"][want_id]
        assert abs(np.linalg.norm(n) - want_scale) < 1e-3
        assert np.max(np.abs(N[y, x, :3] - n)) <= 8 * 2.0 ** -24 * np.max(Q["nrm_terms"][want_id]), \
            f"tie: call {k} {frame} ({x}, {y}): normal {N[y, x, :3]} is not record {want_id}'s ({n})"


def test_tie_rows(oracle_lib):
    """precondition: the twins' quads are the same to the bit, so they tie in the 24-bit depth at every pixel"""
    sc = get_scene("tie")
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    for name, a, b, a_old, b_old, _ in TIE_PAIRS:
        ca = o.debug_render_quads(VIEW_I, 0.0, R.OLD if a_old else R.NEW, 50)
        cb = o.debug_render_quads(VIEW_I, 0.0, R.OLD if b_old else R.NEW, 50)
        assert ca[0][a] and cb[0][b], name
        assert ca[1][a].tobytes() == cb[1][b].tobytes(), f"{name}: the quads differ"
        zw = lambda c: F32(0.5) * (F32(2.0) * c[:, 2] - F32(1.0)) + F32(0.5)
        assert np.array_equal(o.debug_depth24(zw(ca[1][a])), o.debug_depth24(zw(cb[1][b]))), name
        assert a // 256 != b // 256, "the twins must sit in different tiles"
    check_tie_rows(oracle_results("tie"))


def check_diagonal_rows(results_of):
    for sid, (W, H, _, _) in DIAGONALS.items():
        for k in (0, 1):
            r = results_of(sid)[k]
            V = r["new" if k == 0 else "composed"][0]
            assert V[H // 2, W // 2, 3] == 1.0, f"{sid}: the centre pixel on the shared diagonal is not covered (call {k})"
            assert V[..., 3].sum() >= 3


@pytest.mark.parametrize("sid", list(DIAGONALS))
def test_diagonal_rows(oracle_lib, sid):
    """precondition: the centre pixel lies exactly on the diagonal v1 - v2 of the snapped quad"""
    sc = get_scene(sid)
    W, H = DIAGONALS[sid][:2]
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    emitted, corners, _ = o.debug_render_quads(VIEW_I, 0.0, R.NEW, 50)
    assert emitted[0]
    _, X, Y = snapped_boxes(sc["params"], corners)
    px, py = 256 * (W // 2) + 128, 256 * (H // 2) + 128
    assert X[0, 1] + X[0, 2] == 2 * px and Y[0, 1] + Y[0, 2] == 2 * py, (X, Y)
    assert X[0, 1] != X[0, 2], "a diagonal with two ends"
    check_diagonal_rows(oracle_results)


def check_rim_row(results):
    """a pixel centre on the rim (tu^2 + tv^2 == 1) that the outline's ownership rule gives to the quad is drawn"""
    V = results[0]["new"][0]
    drawn = [(x, y) for x, y in RIM_MIDPOINTS if V[y, x, 3] == 1.0]
    assert len(drawn) >= 1, "none of the four rim pixels is drawn"
    assert V[4, 32, 3] == 1.0 and V[..., 3].sum() >= 5
    return drawn


def test_rim_exact_row(oracle_lib):
    """precondition: every outline edge of the snapped quad has its midpoint exactly on a pixel centre"""
    sc = get_scene("rim-exact")
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    emitted, corners, _ = o.debug_render_quads(VIEW_I, 0.0, R.NEW, 50)
    assert emitted[0]
    _, X, Y = snapped_boxes(sc["params"], corners)
    mids = {((X[0, a] + X[0, b]) // 2, (Y[0, a] + Y[0, b]) // 2) for a, b in ((0, 1), (1, 3), (3, 2), (2, 0))
            if (X[0, a] + X[0, b]) % 2 == 0 and (Y[0, a] + Y[0, b]) % 2 == 0}
    assert mids == {(256 * x + 128, 256 * y + 128) for x, y in RIM_MIDPOINTS}, (X, Y)
    print("rim pixels drawn by the oracle:", check_rim_row(oracle_results("rim-exact")))


def check_seam_rows(results):
    """each surfel is drawn on its centre's side only: id 0 in column 0, id 1 in column 47, nothing of either beyond"""
    for k, c in enumerate(get_scene("seam")["calls"]):
        if c[0] != "render" or k != 0:
            continue
        new_ids, old_ids = semantic_ids(results[k]["new"][2]), semantic_ids(results[k]["old"][2])
        assert new_ids[6, 0] == 0 and old_ids[3, 47] == 1
        assert not (new_ids[:, 24:] == 0).any() and not (old_ids[:, :24] == 1).any()
        assert (new_ids == 0).sum() >= 2 and (old_ids == 1).sum() >= 2


def test_seam_rows(oracle_lib):
    sc = get_scene("seam")
    Q = R.quads_fp64(sc["params"], sc["poses"], sc["records"], VIEW_I)
    assert Q["xy"][0, :, 0].min() < -0.5 and Q["xy"][1, :, 0].max() > 48.5, "the quads must cross the seam"
    check_seam_rows(oracle_results("seam"))


@pytest.mark.parametrize("W", (2047, 2048))
def test_big_box_precondition(oracle_lib, W):
    sc = get_scene(f"big-box-{W}x1024")
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    emitted, corners, _ = o.debug_render_quads(VIEW_I, 0.0, R.NEW, 50)
    tests, _, _ = snapped_boxes(sc["params"], corners)
    assert emitted[150] and 2 ** 19 < tests[150] < 2 ** 21, tests[150]
    assert (W * 1024 >= 2 ** 21) == (W == 2048)


def check_big_box(sid, results, what):
    check_against_fp64(sid, results, what)
    ids = semantic_ids(results[0]["new"][2])
    assert (ids == 150).sum() > 2 ** 17, "the big disc must own a large part of the image"
    assert ((ids >= 0) & (ids != 150)).sum() > 1000, "and the ordinary surfels in front of it theirs"


@pytest.mark.parametrize("W", (2047, 2048))
def test_oracle_big_box_against_fp64(oracle_lib, W):
    sid = f"big-box-{W}x1024"
    sc = get_scene(sid)
    check_big_box(sid, run_scene(OracleSide(oracle_lib, sc["params"]), sc), f"oracle {sid}")
    fp64_call.cache_clear()
    _quads.cache_clear()


def test_reciprocal_split_is_exact_for_these_images():
    """k_render splits a test index q into row and column as floor((q + 0.5) * rcp(w)) below 2^21 pixels and divides
    above.  With a reciprocal within one ulp and fp32 products the two agree at every row boundary of every box that fits
    an image of up to 1024 rows (a quad spans under half of the at most 5461 columns) -- so at the big-box sizes a kernel
    that never divides is not wrong, and no test there can tell (the mutation is recorded as equivalent)."""
    w = np.arange(1, 2732, dtype=np.int64)[:, None]
    k = np.arange(1, 1025, dtype=np.int64)[None, :]
    r0 = (F32(1) / w.astype(F32)).astype(F32)
    for r in (np.nextafter(r0, F32(0)), r0, np.nextafter(r0, F32(2))):
        for q, want in ((k * w - 1, k - 1), (k * w, k)):
            assert np.array_equal(np.floor((q.astype(F32) + F32(0.5)) * r).astype(np.int64), np.broadcast_to(want, q.shape))


def gate_expectations(timestamp, use_stability):
    """{probe: (in old rendering, in new rendering)} by the rules of render_surfels.geom, by hand"""
    thr = timestamp - 100
    exp = {}
    for name, col, creation, ts, conf, dot in GATE_PROBES:
        ok = (not use_stability or F32(conf) > F32(GATE_CONF)) and (dot is None or dot > 0.01)
        exp[name] = (ok and creation < thr, ok and (creation >= thr or ts >= thr))
    return exp


def check_gate_rows(results_of):
    for timestamp, use_stability in GATE_SCENES:
        res = results_of(f"gates-t{timestamp}-stability{use_stability}")[0]
        old_ids, new_ids = semantic_ids(res["old"][2]), semantic_ids(res["new"][2])
        for k, (name, col, *_) in enumerate(GATE_PROBES):
            want = gate_expectations(timestamp, use_stability)[name]
            got = (old_ids[6, col] == k, new_ids[6, col] == k)
            assert got == want, f"gates t = {timestamp}, stability {use_stability}: {name}: (old, new) {got}, expected {want}"


def test_gate_rows(oracle_lib):
    exp = gate_expectations(150, 1)
    assert exp["conf-at-threshold"] == (False, False) and exp["conf-one-ulp-above"] == (False, True)
    assert exp["creation-thr-1"] == (True, False) and exp["creation-thr"] == (False, True)
    assert exp["stamp-thr-1"] == (True, False) and exp["stamp-thr"] == (True, True)
    assert gate_expectations(99, 1)["creation-0"] == (False, True) and gate_expectations(101, 1)["creation-0"] == (True, False)
    Q = R.quads_fp64(params(48, 12), pose_table(), gate_records(), VIEW_I)
    for k, (name, *_rest, dot) in enumerate(GATE_PROBES):
        if dot is not None:
            assert abs(Q["front"][k] - dot) < 2e-5 and abs(Q["front"][k] - 0.01) > 10 * R.GATE_EPS, (name, Q["front"][k])
    check_gate_rows(oracle_results)


def check_bad_rows(results_of):
    """a bad record draws nothing and changes nothing: the frames equal those of the map without it, bit for bit"""
    clean = results_of("bad-none")
    for kind in BAD_KINDS:
        assert_results_equal(results_of(f"bad-{kind}"), clean, f"bad-{kind} against the map without the record")
    assert semantic_ids(clean[0]["new"][2]).max() > 256, "both tiles must be drawn"


def test_bad_rows(oracle_lib):
    good = bad_records(None)
    Q = R.quads_fp64(params(48, 12), pose_table(), good, VIEW_I)
    assert Q["geometric"][:255].sum() > 100, "the bad record must sit in a tile of drawn records"
    check_bad_rows(oracle_results)


CARRY = ("size-513", "tiles-empty-between-full", "size-513")


def check_carry_nothing_over(side_factory):
    """scene A, scene B, A again on ONE context, then A's single-target calls and its render once more: every repeat
    equals the first in bits -- the resolve leaves both z-buffers clear"""
    a, b = get_scene(CARRY[0]), get_scene(CARRY[1])
    side = side_factory(a["params"])
    calls = a["calls"]
    first = written(run_scene(side, a), calls)
    run_scene(side, b)
    assert_results_equal(written(run_scene(side, a), calls), first, "A after B")
    order = (2, 3, 4, 0)
    tail = written([side.call(calls[k]) for k in order], [calls[k] for k in order])
    assert_results_equal(tail, [first[k] for k in order], "A's single-target calls and its render once more")


def test_carry_nothing_over(oracle_lib):
    check_carry_nothing_over(lambda p: OracleSide(oracle_lib, p))


INDEX_MAP_SCENES = (("room48x12-moved-compose1", None), ("tiles-empty-between-full", (31, 9)))


def index_map_params(sid, data_size):
    sc = get_scene(sid)
    if data_size is None:
        return sc["params"]
    p = sc["params"]
    return params(p.model_width, p.model_height, data_width=data_size[0], data_height=data_size[1])


@lru_cache(maxsize=None)
def index_map_reference(sid, data_size):
    sc = get_scene(sid)
    return R.indexmap_fp64(index_map_params(sid, data_size), sc["poses"], sc["records"], VIEW_B)


def check_index_map(side_factory, sid, data_size, what):
    """K7: one update of an all-invalid frame; returns the index map after comparing it with fp64 on decided texels"""
    sc = get_scene(sid)
    side = side_factory(index_map_params(sid, data_size))
    side.load(sc["poses"], sc["records"], sc["timestamp"])
    got = side.index_map(VIEW_B).astype(np.int64)
    want, dec = index_map_reference(sid, data_size)
    assert dec.mean() > 0.8 and (dec & (want > 0)).sum() > 0.3 * want.size, "test setup"
    bad = dec & (got != want)
    assert not bad.any(), f"{what}: index map differs from fp64 at (y, x) {np.argwhere(bad)[:5].tolist()}"
    return got


@pytest.mark.parametrize("sid,data_size", INDEX_MAP_SCENES)
def test_oracle_index_map(oracle_lib, sid, data_size):
    check_index_map(lambda p: OracleSide(oracle_lib, p), sid, data_size, f"oracle {sid}")
