"""K8 .. K12 (the surfel update) on crafted maps, CPU side: pins the oracle (oracle/o_map.c) against a plain fp64 statement
of surfel fusion (tests/update_ref.py), proves each structural row's precondition, and fixes the inputs that
tests/test_gpu_update_crafted.py runs through k_update.hip.

A. Room scenes against fp64 (ROOM_IDS): one UPLOADED surfel per texel of k6_ref's analytic room at 48 x 12, 64 x 16 and
   333 x 10 (K10: a partial tile, exactly one tile, three tiles and a part with H not dividing 1024), creation stamps over
   four non-identity pose-table entries, ranges / normals / radii / confidences / stamps / labels in fixed patterns that
   put every decision of update_surfels.vert on both sides; the frame is the room from a moved pose with a band of
   invalid texels and a patch of a nearer wall.  Identity travels in the payload (g = id, b = -1; new surfels carry their
   pixel in the frame's semantic y, z).  Parameter sets: default, weighting_scheme 1, weighting 2 + averaging 1 +
   update_always, confidence_mode 0 / 1 / 2, use_stability 0.

   A surfel is DECIDED when every margin that applies to it (update_ref.MARGINS) exceeds its bound; the bounds are
   measured on the ORACLE (ora_debug_update_terms), never on the kernel: EPS = 2 max|oracle term - fp64 term| over the
   scene, the texel coordinates + one fp32 ulp of the coordinate.  Conditions asserted on every scene: at most 2 % of the
   surfels and 2 % of the pixels undecided; every outcome the parameter set allows, a deletion and a K11 drop at least 10
   times among the decided.  Checked on the decided: outcome, surviving ids in order, marked pixels, K10's pixels in
   x-major order behind the survivors, counts() and the map size; position, K8 radius, avg_prob and weight within
   8 * 2^-24 * sum|terms|; the slerped normal and the confidence within 2 x the oracle's worst deviation over all room
   scenes (NORMAL_BOUND, CONF_BOUND below).

   measured with the CPU oracle (EPS as above; undecided: surfels / mask and K10 pixels, in %; |x - fp64| / u: the worst of
   position, radius, avg_prob, weight in units of 2^-24 sum|terms|, bound 8; normal / conf: worst absolute deviation):

       scene                   EPS texel [px] front    imz      distance angle    radius   conf     undecided   |x-fp64|/u normal   conf     grey green magen. cyan delet. dropp.  new
       room48x12-default       1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  1.7e-06  1.22 / 1.04  1.89       1.0e-07  8.7e-07    36   125     20   78    190    120  342
       room48x12-weighting1    1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  1.7e-06  1.22 / 1.04  1.89       1.2e-07  8.7e-07    36   125     22   78    190    118  342
       room48x12-push          1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  1.7e-06  1.22 / 1.04  3.26       1.4e-07  8.7e-07    36     0    151   78    190    114  342
       room48x12-confmode0     1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  1.7e-06  1.22 / 1.04  1.89       1.2e-07  8.7e-07    36   143     23   78    163    126  316
       room48x12-confmode1     1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  1.7e-06  1.22 / 1.04  1.89       1.0e-07  8.7e-07    36   125     20   78    187    123  339
       room48x12-confmode2     1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  2.1e-06  1.22 / 1.04  1.89       1.2e-07  1.0e-06    36   138     22   78    171    124  324
       room48x12-nostability   1.36e-05       4.6e-07  3.3e-08  1.9e-06  1.7e-07  3.8e-07  n/a      1.22 / 1.04  1.89       1.2e-07  n/a        55   204     30  111      0    169  233
       room64x16-default       1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  2.2e-06  1.86 / 1.76  2.59       1.2e-07  1.1e-06    62   247     32  125    337    202  578
       room64x16-weighting1    1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  2.2e-06  1.86 / 1.76  2.59       1.4e-07  1.1e-06    62   247     33  125    337    201  578
       room64x16-push          1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  2.2e-06  1.86 / 1.76  4.20       1.5e-07  1.1e-06    62     0    293  125    337    188  578
       room64x16-confmode0     1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  1.7e-06  1.86 / 1.76  2.59       1.2e-07  8.7e-07    62   274     38  125    290    216  534
       room64x16-confmode1     1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  2.2e-06  1.86 / 1.76  2.59       1.2e-07  1.1e-06    62   247     32  125    331    208  573
       room64x16-confmode2     1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  1.8e-06  1.86 / 1.76  2.59       1.2e-07  9.1e-07    62   268     36  125    310    204  552
       room64x16-nostability   1.64e-05       4.4e-07  3.4e-08  1.8e-06  1.5e-07  2.6e-07  n/a      1.86 / 1.76  2.59       1.2e-07  n/a        90   382     57  186      0    290  371
       room333x10-default      9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  1.9e-06  1.26 / 1.29  2.71       1.4e-07  9.7e-07   216   765    119  423   1094    671 1959
       room333x10-weighting1   9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  1.9e-06  1.26 / 1.29  2.71       1.3e-07  9.7e-07   216   765    125  423   1094    665 1959
       room333x10-push         9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  1.9e-06  1.26 / 1.29  3.47       1.5e-07  9.7e-07   216     0    925  423   1094    630 1959
       room333x10-confmode0    9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  1.7e-06  1.26 / 1.29  2.71       1.4e-07  8.7e-07   216   847    137  423    947    718 1820
       room333x10-confmode1    9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  2.2e-06  1.26 / 1.29  2.71       1.4e-07  1.1e-06   216   770    120  423   1075    684 1941
       room333x10-confmode2    9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  2.1e-06  1.26 / 1.29  2.71       1.4e-07  1.1e-06   216   817    134  423   1011    687 1881
       room333x10-nostability  9.72e-05       4.4e-07  4.9e-08  2.9e-06  1.8e-07  2.0e-07  n/a      1.29 / 1.29  2.71       1.4e-07  n/a       336  1181    196  615      0    959 1342
       (undecided: surfels / mask and K10 pixels, in %; worst normal deviation 1.53e-07, worst confidence deviation 1.11e-06;
       the confidence EPS is measured on surviving records only; n/a: use_stability = 0 leaves the confidence alone)

B. Structural rows (bit for bit against the oracle on the GPU; here each row's own property is proved on the oracle).
   Keep / delete is set per record and needs no geometry: out of view, confidence 5, or -1 with age 10 >= unstable_age.
     size-S / group-S            S = 0, 1, 1023, 1024, 1025, 2049 (the 1024-record tile); 65535, 65536, 65537, 65536 + 1025 (the
                                 64-tile group): survivor ids in input order, counts, records unchanged but for the colour
     grid-S                      262144 + 1025 and 2 * 262144 + 7 records, the 333 x 10 room map tiled: more tiles than blocks;
                                 copies tie in K7's depth to the bit, the lowest id wins, later copies share one fate
     keep-*                      at 4 and at 130 tiles: all, none, alternating tiles, one empty group between full ones, the
                                 first / the last slot of every tile, only the last record of the map
     epochs, epochs-extract      maps of 130 -> 2 -> 130 tiles on ONE context: every step equals a fresh context; with a
                                 standalone K12 (three extractions) between the steps: equal to the oracle's one context
     area-edges                  |pos - c| equal to K11's extent and one ulp beyond, both axes, both signs; a stamp with
                                 the sign bit set
     extraction-*                submap_extent 4, dimension 2, a pose that moves a tile row out of the window: the fused,
                                 flags, standalone and all-at-once paths give the same tile and map; K9's records before
                                 K10's in the tile; records on the tile's edge and one ulp off; the tile equals fp64's
                                 predicate on the decided; it comes back (append) while another tile is flagged
     k10-WxH-all / none / masked 64 x 16 (the column-patch walk), 48 x 10 and 48 x 12 (the linear walk), 130 x 16 (two
                                 tiles and a part): every pixel generating in x-major order, none, the mask fully set
     capacity-*                  max_surfels = 1500 filled exactly by K9 (in the middle of its second tile) and passed in
                                 the middle of K10: the map is the first 1500 records in order; on the GPU the overflow is
                                 reported by size() and the truncated buffer, read with suma_map_download, is the oracle's
C. Branch rows: one or two surfels on the ray of one valid pixel.
     gate-*-below / above        the two fp32 inputs, one ulp of the knob apart, between which the ORACLE's outcome flips
                                 (found by bisection on the oracle): distance, angle, the front-face product at 0, imz at 1,
                                 z_ndc at -1 (imz at 0), the new confidence at log_unstable.  Precondition: the oracle's
                                 fp32 term is within 8 ulps of the gate (the distance within 8 position steps of 2^-20 m).
                                 z_ndc = +1 needs imz = 1, which `inside` (imz < 1) already excludes: no row.
                                 Quirk B-6 (inside = all(img < dim) && !all(img < 0)) has no row of its own: it is what
                                 gate-zclip-0-below shows -- imz < 0 with imx, imy >= 0 still counts as inside, the surfel
                                 is matched (and, z_ndc < -1, marks nothing).  Its other leg, imx < 0 or imy < 0, cannot be
                                 observed: the texel fetched there is the border, which is invalid
     branch-distance-exact       distance == map_max_distance to the bit: not compatible
     branch-*                    timestamp - creation = active_timestamps - 1 / + 0; age = unstable_age - 1 / + 0; confidence
                                 one ulp below the threshold / at it; new_radius one ulp below / equal / above old_radius;
                                 the cap at 20; max_weight; the penalty only when the MODEL label is dynamic; a stored label
                                 that does not round-trip through * 255; two surfels on one pixel, K7's winner cyan, the
                                 other grey, in both orders; slerp of identical normals (v0) and of normals 179 degrees
                                 apart; a surfel a hair either side of the yaw seam; the image's top and bottom rows
     bad-records, bad-texels     NaN, +-inf and 0 in position, normal, radius, confidence, weight, payload and in every
                                 channel of the three maps: nothing faults, the outcomes are the oracle's
   Every record's `count` is an integer in [0, max_poses): the domain stated at suma_map_upload (asserted for every scene).
"""
from functools import lru_cache

import numpy as np
import pytest

import k6_ref as K
import test_render_crafted_host as RH
import update_ref as UR
from semantic_suma_amd.types import SURFEL_DTYPE, default_params

F32 = np.float32
TIMESTAMP = 150
N_POSES = 256
POSE_B = K.pose_from(7.0, (0.4, -0.3, 0.0)).astype(F32).astype(np.float64)
TILE = 1024  # records per K9 tile; 64 tiles per look-back group

# 2 x the oracle's worst deviation from fp64 over all room scenes (the header table): no sum-of-products bound follows
# simply through acos / sin (the slerped normal) or exp / log (the confidence)
NORMAL_BOUND = 2 * 1.53e-07
CONF_BOUND = 2 * 1.11e-06


def params(W, H, **ov):
    base = dict(data_width=W, data_height=H, model_width=W, model_height=H, max_surfels=8192, max_poses=N_POSES)
    base.update(ov)
    return default_params(**base)


PARAM_SETS = {
    "default": {},
    "weighting1": dict(weighting_scheme=1),
    "push": dict(weighting_scheme=2, averaging_scheme=1, update_always=1),
    "confmode0": dict(confidence_mode=0),
    "confmode1": dict(confidence_mode=1),
    "confmode2": dict(confidence_mode=2),
    "nostability": dict(use_stability=0),
}
ROOM_SIZES = ((48, 12), (64, 16), (333, 10))
ROOM_IDS = [f"room{W}x{H}-{s}" for (W, H) in ROOM_SIZES for s in PARAM_SETS]
# K11's window in the room scenes: extent 2 * 1 * 1.68 + 1.68 = 5.04 m around the origin; the walls stand at 5 m and
# the surfels on them within +-3 % of that
ROOM_SUBMAP = dict(submap_extent=1.68, submap_dimension=1)


def _lds(a, b, ii, jj):
    """fixed low-discrepancy pattern in [0, 1)"""
    return np.modf(a * ii + b * jj)[0]


def with_ids(rec, first=0):
    rec["g"] = np.arange(first, first + len(rec), dtype=F32)
    rec["b"] = -1.0
    return rec


def room_map(p):
    """one surfel per texel of the room seen from the identity, every input of update_surfels.vert spread in a fixed
    pattern (see the header)"""
    W, H = p.data_width, p.data_height
    k = UR.consts(p)
    pts, nrm, _ = K.room_cast(W, H, p, np.eye(4))
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    # ranges: three quarters within +-3 % (distance lands on both sides of map_max_distance), one quarter within +-30 %
    u = _lds(0.7548776662, 0.5698402910, ii, jj)
    wide = (ii + 3 * jj) % 4 == 0
    pts = pts * (1.0 + np.where(wide, 0.6, 0.06) * (u - 0.5))[..., None]
    depth = np.linalg.norm(pts, axis=-1)
    # normals: tilted by 1 to 12 degrees (identical normals are a branch row of their own); every seventh by 38 .. 52 degrees (angle on both sides of sin 45)
    t = np.stack([_lds(0.8191725134, 0.6710436067, ii, jj), _lds(0.5497004779, 0.3819660113, ii, jj),
                  _lds(0.4142135624, 0.7320508076, ii, jj)], axis=-1) - 0.5
    t = t - np.sum(t * nrm, axis=-1, keepdims=True) * nrm
    t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    steep = (2 * ii + jj) % 7 == 0
    ang = np.deg2rad(np.where(steep, 38.0 + 14.0 * _lds(0.3247179572, 0.2207440846, ii, jj),
                              1.0 + 11.0 * _lds(0.3247179572, 0.2207440846, ii, jj)))
    nrm = np.cos(ang)[..., None] * nrm + np.sin(ang)[..., None] * t
    creation = np.asarray(RH.CREATION_STAMPS)[(ii + 2 * jj) % 4]
    # radii 0.7 .. 1.4 x what K8 gives a measurement at that range
    radius = 1.41 * depth * k["pixel_size"] * (0.7 + 0.7 * _lds(0.6180339887, 0.7548776662, jj, ii))
    conf = np.asarray([1.2, -0.3, 0.2, 2.5, 19.9, -0.42, 0.5, -1.0])[(3 * ii + 5 * jj) % 8]
    # stamps: ages 2 and 3 (unstable_age), 10, and the creation stamp itself
    ts = np.where((ii + jj) % 3 == 0, TIMESTAMP - 2, np.where((ii + jj) % 3 == 1, TIMESTAMP - 3, np.maximum(creation, TIMESTAMP - 10)))
    rec = RH.make_records(pts.reshape(-1, 3), nrm.reshape(-1, 3), radius.ravel(), creation.ravel(), ts.ravel(), conf.ravel())
    rec["r"] = (np.asarray([40.0, 10.0, 50.0, 18.0, 30.0, 40.0])[(ii + 4 * jj) % 6] / 255.0).astype(F32).ravel()
    rec["w"] = (0.3 + 0.6 * _lds(0.2891, 0.6173, ii, jj)).astype(F32).ravel()
    rec["weight"] = (1.0 + (ii * 7 + jj) % 5).astype(F32).ravel()
    return with_ids(rec)


def room_frame(p, pose):
    """the room from `pose`; a band of invalid texels, a patch of a wall 25 % nearer; semantic = (label / 255, x, y, prob)"""
    W, H = p.data_width, p.data_height
    V, N = K.room_frames(W, H, p, pose)
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    f = ii / W
    near = (f > 0.55) & (f < 0.70)
    V[..., :3] = np.where(near[..., None], V[..., :3] * F32(0.75), V[..., :3])
    band = (f > 0.30) & (f < 0.36)
    V[band] = 0.0
    N[band] = 0.0
    S = np.zeros((H, W, 4), dtype=F32)
    S[..., 0] = (np.asarray([40.0, 10.0, 50.0, 40.0, 30.0])[(ii + jj) % 5] / 255.0).astype(F32)
    S[..., 1], S[..., 2] = ii, jj
    S[..., 3] = (0.5 + 0.45 * _lds(0.7071, 0.3141, ii, jj)).astype(F32)
    return V, N, S


def scene(id, p, records, updates, timestamp=TIMESTAMP, poses=None, **more):
    """updates: list of (pose, frame) or (pose, frame, (poses, records, timestamp)) -- frame a (V, N, S) triple, the third
    entry a map to load before that update; more: env (environment variables the product reads during an update),
    threads (for the oracle), expect (what the row states)"""
    records.setflags(write=False)
    return dict(id=id, params=p, poses=RH.pose_table() if poses is None else poses, records=records, timestamp=timestamp,
                updates=updates, **more)


def _room(W, H, pset):
    def build():
        p = params(W, H, **ROOM_SUBMAP, **PARAM_SETS[pset])
        return scene(f"room{W}x{H}-{pset}", p, room_map(p), [(POSE_B, room_frame(p, POSE_B))])
    return build


_SCENES = {f"room{W}x{H}-{s}": _room(W, H, s) for (W, H) in ROOM_SIZES for s in PARAM_SETS}


@lru_cache(maxsize=None)
def get_scene(sid):
    return _SCENES[sid]()


# ---------------------------------------------------------------------------------------------------------------------
# running a scene on a backend (the oracle here, the kernel in the GPU file)
# ---------------------------------------------------------------------------------------------------------------------
class OracleSide:
    def __init__(self, lib, p, threads=1):
        self.lib, self.o, self.p = lib, lib.Oracle(p, threads=threads), p

    def load(self, poses, records, timestamp):
        self.o.map_update_poses(poses)
        self.o.map_upload(records, timestamp)

    def update(self, pose, frame, env=None):
        f = self.o.frame()
        f.set(*frame)
        self.o.map_update(pose, f)
        s, d = self.o.map_counts()
        oi, oj = self.o.map_submap_origin()
        tiles = {}
        for (i, j) in TILE_WINDOW:
            t = self.o.map_cache_tile(i, j)
            if len(t):
                tiles[(i, j)] = np.ascontiguousarray(t).view(np.uint32).reshape(len(t), 16).copy()
        assert sum(len(t) for t in tiles.values()) == self.o.map_cached_surfels(), "a parked tile outside TILE_WINDOW"
        return dict(surfels=self.o.map_surfels().copy(), radius_conf=self.o.map_radius_conf().copy(),
                    index=self.o.map_index_map().copy(), mask=self.o.map_integrated().copy(), counts=(s, d),
                    size=self.o.map_size(), origin=(int(oi), int(oj)), tiles=tiles)


TILE_WINDOW = [(i, j) for i in range(-8, 9) for j in range(-8, 9)]  # every submap tile a scene of this file parks


def run_scene(side, sc):
    side.load(sc["poses"], sc["records"], sc["timestamp"])
    res = []
    for u in sc["updates"]:
        if len(u) == 3:
            side.load(*u[2])
        res.append(side.update(u[0], u[1], sc.get("env")))
    return res


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize % 4 == 0 and a.dtype != np.uint8 else a


def assert_results_equal(got, want, what):
    """bit for bit: the surfel buffer, radius_conf, index map, integration mask, counts, cached tiles and origin"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["counts"] == w["counts"] and g["size"] == w["size"] and g["origin"] == w["origin"], \
            f"{what}: update {k}: counts / size / origin {g['counts'], g['size'], g['origin']} vs {w['counts'], w['size'], w['origin']}"
        assert g["surfels"].tobytes() == w["surfels"].tobytes(), f"{what}: update {k}: the surfel buffers differ, first at " \
            f"record {int(np.argmax(np.any(words(g['surfels']).reshape(-1, 16) != words(w['surfels']).reshape(-1, 16), axis=1)))}"
        for nm in ("radius_conf", "index", "mask"):
            ne = words(g[nm]) != words(w[nm])
            assert not ne.any(), f"{what}: update {k}: {nm}: {int(ne.sum())} words differ, first at {np.argwhere(ne)[:4].tolist()}"
        assert g["tiles"].keys() == w["tiles"].keys(), f"{what}: update {k}: cached tiles {sorted(g['tiles'])} vs {sorted(w['tiles'])}"
        for ij in g["tiles"]:
            assert np.array_equal(g["tiles"][ij], w["tiles"][ij]), f"{what}: update {k}: cached tile {ij} differs"


@lru_cache(maxsize=None)
def oracle_results(sid):
    from oracle import pyoracle
    pyoracle.build()
    sc = get_scene(sid)
    return run_scene(OracleSide(pyoracle, sc["params"], threads=sc.get("threads", 1)), sc)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 expectation of a room scene, and the bounds measured against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def fp64_scene(sid):
    """(update_ref result, EPS measured on the oracle, decided masks) of the scene's first update"""
    from oracle import pyoracle
    pyoracle.build()
    sc = get_scene(sid)
    pose, frame = sc["updates"][0][:2]
    r = UR.update_fp64(sc["params"], sc["poses"], sc["records"], sc["timestamp"], pose, frame)
    eps = UR.measure_eps(r, oracle_run(sc)[1])
    return r, eps, UR.decide(r, eps)


@pytest.mark.parametrize("sid", ROOM_IDS)
def test_debug_terms_belong_to_the_oracle(oracle_lib, sid):
    """oracle/debug/o_update_terms.c restates K9's front half beside the oracle: what it exports must be what o_k9_update
    itself acted on -- every surviving matched surfel has distance below the gate, none it left unmatched is compatible
    by the exported terms, and the pixels K9 marked are texels that the exported coordinates name"""
    sc = get_scene(sid)
    res, terms = oracle_run(sc)
    old = res["surfels"][res["surfels"]["b"] == F32(-1.0)]
    ids = old["g"].astype(np.int64)
    matched = ids[np.isin(colour_of(old), (UR.GREEN, UR.MAGENTA))]
    assert len(matched) > 50 and np.all(terms[matched, 4] < F32(sc["params"].map_max_distance)) and np.all(terms[matched, 3] > 0)
    unmatched = ids[np.isin(colour_of(old), (UR.GREY, UR.CYAN))]
    thr = np.sin(np.deg2rad(float(sc["params"].map_max_angle)))
    with np.errstate(invalid="ignore"):
        compatible = (terms[unmatched, 4] < F32(sc["params"].map_max_distance)) & (terms[unmatched, 5] < thr - 1e-6) & \
            (terms[unmatched, 3] > 0) & (terms[unmatched, 2] < 1)
    assert not compatible.any(), "a surfel the export calls compatible was not matched by K9"
    m = matched[(terms[matched, 2] >= 0) & (terms[matched, 2] <= 1)]
    mask = np.zeros_like(res["mask"])
    mask[np.floor(terms[m, 1]).astype(np.int64), np.floor(terms[m, 0]).astype(np.int64)] = 1
    # the map holds the survivors K11 kept; one it dropped has marked its pixel all the same.  So: what the map's matched
    # records name is marked, and everything marked is named by a surfel whose exported distance is below the gate
    assert not (mask & ~res["mask"]).any(), "a texel the exported coordinates name was not marked by K9"
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero((terms[:, 4] < F32(sc["params"].map_max_distance)) & (terms[:, 2] >= 0) & (terms[:, 2] <= 1))
    named = np.zeros_like(res["mask"])
    named[np.floor(terms[cand, 1]).astype(np.int64), np.floor(terms[cand, 0]).astype(np.int64)] = 1
    assert not (res["mask"] & ~named).any(), "K9 marked a pixel that no exported coordinate names"


def colour_of(rec):
    """outcome colour of records from the packed rgb K9 / K10 write: UR.GREY .. UR.CYAN, 5 = blue (new)"""
    c = rec["color"].astype(np.int64)
    r, g, b = c >> 16, (c >> 8) & 255, c & 255
    return np.where((r == g) & (g == b), UR.GREY, np.where((r == 0) & (b == 0), UR.GREEN, np.where((r == 255) & (g == 0), UR.MAGENTA,
                    np.where((r == 0) & (g == 255), UR.CYAN, 5))))


def check_against_fp64(sid, got, what):
    """the first update of a scene, as a backend computed it, against update_ref on the decided; returns the figures"""
    sc = get_scene(sid)
    r, eps, (dec, member, mask_dec, gen_dec, new_member) = fp64_scene(sid)
    g = got[0]
    out = g["surfels"]
    W, H, ts = r["W"], r["H"], sc["timestamp"]
    is_old = out["b"] == F32(-1.0)
    n_old = int(is_old.sum())
    assert is_old[:n_old].all(), f"{what}: K10's new surfels must stand behind K9's survivors"
    old, new = out[:n_old], out[n_old:]
    ids = old["g"].astype(np.int64)
    # survivors: ids in input order, and exactly fp64's among the decided
    assert np.all(np.diff(ids) > 0), f"{what}: survivors out of input order"
    want = np.flatnonzero(r["keep"] & r["in_area"])
    assert np.array_equal(ids[member[ids]], want[member[want]]), f"{what}: surviving ids differ from fp64's on the decided"
    # new surfels: pixels in x-major order, exactly fp64's among the decided
    px = new["g"].astype(np.int64) * H + new["b"].astype(np.int64)
    assert np.all(np.diff(px) > 0), f"{what}: new surfels out of x-major order"
    gen_x = r["gen"][r["pixels"][:, 1], r["pixels"][:, 0]] & r["new_in_area"]
    wantp = np.flatnonzero(gen_x)
    assert np.array_equal(px[new_member[px]], wantp[new_member[wantp]]), f"{what}: new surfels differ from fp64's on the decided"
    assert g["size"] == len(out)
    # counts() = (S', D) before K11: equal to fp64's when nothing undecided could change them, else within the undecided
    s_lo, s_hi = int((r["keep"] & dec).sum()), int((r["keep"] | ~dec).sum())
    assert s_lo <= g["counts"][0] <= s_hi, f"{what}: S' = {g['counts'][0]} outside fp64's [{s_lo}, {s_hi}]"
    d_lo, d_hi = int((r["gen"] & gen_dec).sum()), int((r["gen"] | ~gen_dec).sum())
    assert d_lo <= g["counts"][1] <= d_hi, f"{what}: D = {g['counts'][1]} outside fp64's [{d_lo}, {d_hi}]"
    # the integration mask and K8
    ne = (g["mask"].astype(bool) != r["mask"]) & mask_dec
    assert not ne.any(), f"{what}: integration mask differs from fp64's at decided pixels {np.argwhere(ne)[:4].tolist()}"
    k8_dec = r["k8_margin"] > UR.K10_EPS
    rc = g["radius_conf"].astype(np.float64)
    assert np.array_equal(rc[..., 3][k8_dec] > 0.5, r["k8_valid"][k8_dec]), f"{what}: K8 validity"
    assert not rc[..., 1].any() and not rc[..., 2].any()
    worst = float(np.max(np.abs(rc[..., 0] - r["radius_map"])[k8_dec] / (UR.U * np.maximum(r["radius_terms"], 1e-30))[k8_dec]))
    # outcome and values of decided survivors
    sel = dec[ids] & member[ids]
    i = ids[sel]
    o = old[sel]
    assert np.array_equal(colour_of(o), r["outcome"][i]), f"{what}: outcome colours differ from fp64's on the decided"
    assert np.array_equal(o["timestamp"].astype(np.int64), r["stamp"][i]) and np.array_equal(o["count"].astype(np.int64), r["creation"][i])
    assert np.array_equal(o["r"], sc["records"]["r"][i]), "the label channel is never written"

    def rel(a, b, terms):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.abs(a.astype(np.float64) - b) / (UR.U * terms)
        return float(np.nanmax(np.where(terms > 0, q, np.where(a.astype(np.float64) == b, 0.0, np.inf)), initial=0.0))

    av = r["averaged"][i]
    gp = np.stack([o["x"], o["y"], o["z"]], -1)
    worst = max(worst, rel(gp[av], r["pos"][i][av], r["pos_terms"][i][av]), rel(o["w"][av], r["prob"][i][av], r["prob_terms"][i][av]),
                rel(o["weight"][av], r["weight"][i][av], r["weight_terms"][i][av]))
    assert np.array_equal(gp[~av].astype(np.float64), r["pos"][i][~av]) and np.array_equal(o["w"][~av].astype(np.float64), r["prob"][i][~av])
    assert np.array_equal(o["weight"][~av].astype(np.float64), r["weight"][i][~av])
    rad_dev = rel(o["radius"], r["radius"][i], np.where(r["match"][i], r["radius_terms"][np.clip(r["ty"][i], 0, H - 1), np.clip(r["tx"][i], 0, W - 1)], 0.0))
    worst = max(worst, rad_dev)
    assert worst <= 8.0, f"{what}: position / radius / avg_prob / weight off by {worst:.2f} x 2^-24 sum|terms| (bound 8)"
    gn = np.stack([o["nx"], o["ny"], o["nz"]], -1).astype(np.float64)
    # the room scenes, whose worst deviation is the bound, turn normals by less than 90 degrees; towards 180 degrees
    # slerp's 1 / sin(omega) amplifies the rounding of acos without limit (branch-slerp-179 has a property of its own)
    acute = ~av | (r["margins"]["slerp"][i] <= np.pi / 2)
    ndev = float(np.max(np.abs(gn - r["nrm"][i])[acute], initial=0.0))
    with np.errstate(invalid="ignore"):
        cdev = float(np.nanmax(np.abs(o["confidence"].astype(np.float64) - r["confidence"][i]), initial=0.0))
    assert ndev <= NORMAL_BOUND, f"{what}: slerped normal off by {ndev:.3g} (bound {NORMAL_BOUND:.3g})"
    assert cdev <= CONF_BOUND, f"{what}: confidence off by {cdev:.3g} (bound {CONF_BOUND:.3g})"
    # new surfels: values straight from the frame
    V, N, S = sc["updates"][0][1]
    sel = new_member[px]
    x, y = new["g"].astype(np.int64)[sel], new["b"].astype(np.int64)[sel]
    nn = new[sel]
    assert np.array_equal(np.stack([nn["x"], nn["y"], nn["z"]], -1), V[y, x, :3]) and np.array_equal(nn["w"], S[y, x, 3])
    assert np.array_equal(nn["r"], S[y, x, 0]) and np.all(nn["weight"] == 1) and np.all(nn["timestamp"] == ts) and np.all(nn["count"] == ts)
    assert np.all(colour_of(nn) == 5)
    assert np.max(np.abs(np.stack([nn["nx"], nn["ny"], nn["nz"]], -1) - r["new_normal"][y, x]), initial=0.0) <= 8 * UR.U
    assert np.max(np.abs(nn["confidence"] - r["new_conf"][y, x]), initial=0.0) <= 8 * UR.U
    assert np.max(np.abs(nn["radius"].astype(np.float64) - r["radius_map"][y, x]) / (UR.U * r["radius_terms"][y, x]), initial=0.0) <= 8.0
    return dict(worst=worst, normal=ndev, conf=cdev)


def scene_figures(sid):
    r, eps, (dec, member, mask_dec, gen_dec, new_member) = fp64_scene(sid)
    ok = dec & member
    counts = {nm: int(((r["outcome"] == c) & ok & ((c == UR.DELETED) | r["in_area"])).sum()) for c, nm in enumerate(UR.OUTCOMES)}
    counts["dropped"] = int((r["keep"] & ~r["in_area"] & ok).sum())
    counts["new"] = int((r["gen"] & gen_dec).sum())
    return dict(eps=eps, undecided=(1 - ok.mean(), 1 - mask_dec.mean(), 1 - gen_dec.mean()), counts=counts)


def allowed_outcomes(pset):
    out = ["grey", "green", "magenta", "cyan", "deleted", "dropped"]
    if PARAM_SETS[pset].get("update_always"):
        out.remove("green")
    if PARAM_SETS[pset].get("use_stability", 1) == 0:
        out.remove("deleted")
    return out


@pytest.mark.parametrize("sid", ROOM_IDS)
def test_room_scene_is_decided(oracle_lib, sid):
    f = scene_figures(sid)
    print(f"{sid}: EPS {f['eps']}  undecided {f['undecided']}  counts {f['counts']}")
    assert f["undecided"][0] <= 0.02, f"{sid}: {100 * f['undecided'][0]:.2f} % of the surfels undecided"
    assert f["undecided"][1] <= 0.02 and f["undecided"][2] <= 0.02, f"{sid}: undecided pixels {f['undecided'][1:]}"
    for nm in allowed_outcomes(sid.split("-", 1)[1]):
        assert f["counts"][nm] >= 10, f"{sid}: only {f['counts'][nm]} decided surfels end {nm}"
    assert f["counts"]["new"] >= 10


@pytest.mark.parametrize("sid", ROOM_IDS)
def test_oracle_room_scene_against_fp64(oracle_lib, sid):
    fig = check_against_fp64(sid, oracle_results(sid), f"oracle {sid}")
    print(f"{sid}: worst |oracle - fp64| / (2^-24 sum|terms|) = {fig['worst']:.2f}, normal {fig['normal']:.3g}, conf {fig['conf']:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# B. structural rows
# ---------------------------------------------------------------------------------------------------------------------
def plain_records(keep):
    """records whose fate needs no geometry: straight above the sensor (out of view), identity creation pose; to keep:
    confidence 5; to delete: confidence -1 (below the threshold) with age 10 >= unstable_age"""
    keep = np.asarray(keep, dtype=bool)
    n = len(keep)
    rec = np.zeros(n, dtype=SURFEL_DTYPE)
    rec["x"] = 0.1 + 0.01 * (np.arange(n) % 7)
    rec["y"], rec["z"], rec["nz"], rec["radius"], rec["weight"], rec["w"] = 0.1, 8.0, -1.0, 0.1, 1.0, 0.5
    rec["confidence"] = np.where(keep, 5.0, -1.0)
    rec["timestamp"] = TIMESTAMP - 10
    rec["r"] = F32(40.0 / 255.0)
    return with_ids(rec)


def empty_frame(p):
    return tuple(np.zeros((p.data_height, p.data_width, 4), dtype=F32) for _ in range(3))


def keep_scene(sid, keep, **more):
    p = params(48, 12, max_surfels=len(keep) + 1024)
    return scene(sid, p, plain_records(keep), [(POSE_B, empty_frame(p))], expect=dict(keep=np.asarray(keep, bool)), **more)


SIZES = (0, 1, 1023, 1024, 1025, 2049)                     # the 1024-record tile
GROUP_SIZES = (65535, 65536, 65537, 65536 + 1025)         # the 64-tile group: the first tile that sums a complete group word
GRID_SIZES = (262144 + 1025, 2 * 262144 + 7)              # more tiles than blocks: second and third tickets
for _S in SIZES + GROUP_SIZES:
    _nm = ("size-" if _S in SIZES else "group-") + str(_S)
    _SCENES[_nm] = (lambda nm, S: lambda: keep_scene(nm, np.arange(S) % 3 != 1))(_nm, _S)


def _pattern(name, T):
    i = np.arange(T * TILE)
    t, slot = i // TILE, i % TILE
    return {"full": np.ones(T * TILE, bool), "empty": np.zeros(T * TILE, bool), "alternating": t % 2 == 0,
            "empty-group": (t < 64) | (t >= 128) if T > 64 else (t == 0) | (t == T - 1),
            "first-slot": slot == 0, "last-slot": slot == TILE - 1, "last-record": i == T * TILE - 1}[name]


KEEP_PATTERNS = ("full", "empty", "alternating", "empty-group", "first-slot", "last-slot", "last-record")
KEEP_IDS = [f"keep-{nm}-{T}" for T in (4, 130) for nm in KEEP_PATTERNS]
for _T in (4, 130):
    for _nm in KEEP_PATTERNS:
        _SCENES[f"keep-{_nm}-{_T}"] = (lambda nm, T: lambda: keep_scene(f"keep-{nm}-{T}", _pattern(nm, T)))(_nm, _T)
KEEP_ROW_IDS = [f"size-{S}" for S in SIZES] + [f"group-{S}" for S in GROUP_SIZES] + KEEP_IDS


def check_keep_row(sid, got):
    """survivor ids in input order, counts, and records unchanged but for the grey colour"""
    sc = get_scene(sid)
    keep = sc["expect"]["keep"]
    g = got[0]
    assert g["counts"] == (int(keep.sum()), 0) and g["size"] == int(keep.sum()), f"{sid}: counts {g['counts']}, size {g['size']}"
    out = g["surfels"]
    assert np.array_equal(out["g"].astype(np.int64), np.flatnonzero(keep)), f"{sid}: survivor ids"
    want = sc["records"][keep].copy()
    want["color"] = out["color"]
    assert out.tobytes() == want.tobytes() and np.all(colour_of(out) == UR.GREY), f"{sid}: survivors changed"
    assert not g["mask"].any() and not g["index"].any()


@pytest.mark.parametrize("sid", KEEP_ROW_IDS)
def test_keep_rows(oracle_lib, sid):
    check_keep_row(sid, oracle_results(sid))


# ---- grid rows: a room map tiled -------------------------------------------------------------------------------------
GRID_BASE = "room333x10-default"


def _grid(S):
    def build():
        base = get_scene(GRID_BASE)
        p = params(333, 10, max_surfels=S + 8192, **ROOM_SUBMAP)
        n0 = len(base["records"])
        rec = with_ids(np.tile(base["records"], S // n0 + 1)[:S].copy())
        return scene(f"grid-{S}", p, rec, base["updates"], threads=8)
    return build


GRID_IDS = [f"grid-{S}" for S in GRID_SIZES]
for _S in GRID_SIZES:
    _SCENES[f"grid-{_S}"] = _grid(_S)


def check_grid_row(sid, got, base_result):
    """copies of a surfel are identical to the bit, so K7 ties in depth and the lowest id -- a record of the first copy --
    owns every texel; every later copy shares one fate (none of them is K7's winner), the mask and D are the base map's"""
    sc = get_scene(sid)
    n0, S = len(get_scene(GRID_BASE)["records"]), len(sc["records"])
    g, b = got[0], base_result[0]
    assert g["index"].max() <= n0 and np.array_equal(g["index"], b["index"]), f"{sid}: K7 ties must go to the lowest id"
    assert np.array_equal(g["mask"], b["mask"]) and g["counts"][1] == b["counts"][1]
    out = g["surfels"]
    old = out[out["b"] == F32(-1.0)]
    ids = old["g"].astype(np.int64)
    assert np.all(np.diff(ids) > 0), f"{sid}: survivors out of input order"
    alive = np.zeros(S, bool)
    alive[ids] = True
    col = np.full(S, -1)
    col[ids] = colour_of(old)
    copies = (S - n0) // n0  # complete later copies
    a = alive[n0:n0 + copies * n0].reshape(copies, n0)
    c = col[n0:n0 + copies * n0].reshape(copies, n0)
    assert np.all(a == a[0]) and np.all(c == c[0]), f"{sid}: later copies of one surfel must share one fate"
    assert not np.any(c == UR.CYAN), f"{sid}: a later copy cannot be K7's winner"
    first_cyan = col[:n0] == UR.CYAN
    assert first_cyan.sum() >= 10 and np.all((c[0][first_cyan] == UR.GREY) | ~a[0][first_cyan])
    same = ~first_cyan & alive[:n0]
    assert np.array_equal(col[:n0][same], c[0][same])
    gone = ~alive[:n0]  # deleted or outside K11's area in the first copy: so are the later ones, unless it was the winner
    assert np.all(~a[0][gone] | (c[0][gone] == UR.GREY))
    new = out[out["b"] != F32(-1.0)]
    bn = b["surfels"][b["surfels"]["b"] != F32(-1.0)]
    assert new.tobytes() == bn.tobytes(), f"{sid}: the new surfels are the base map's"


@pytest.mark.parametrize("sid", GRID_IDS)
def test_grid_rows(oracle_lib, sid):
    check_grid_row(sid, oracle_results(sid), oracle_results(GRID_BASE))


# ---- epochs: maps of 130 -> 2 -> 130 tiles on one context ------------------------------------------------------------
def _epochs(extract):
    def build():
        ov = dict(submap_extent=4.0, submap_dimension=2) if extract else {}
        p = params(48, 12, max_surfels=131 * TILE, **ov)
        maps = [plain_records(_pattern("alternating", 130)), plain_records(np.arange(2 * TILE) % 5 != 0),
                plain_records(~_pattern("alternating", 130))]
        poses = RH.pose_table()
        if extract:  # a third of the records in each of the tiles (-2, 2), (-1, 2), (0, 2) that the three steps extract
            for m in maps:
                m["x"] += np.asarray([-16.0, -8.0, 0.0], dtype=F32)[np.arange(len(m)) % 3]
                m["y"] = 16.0
        shift = [K.pose_from(0.0, (4.5 + 8.5 * k if extract else 0.3 * k, 0.0, 0.0)).astype(F32).astype(np.float64) for k in range(3)]
        ups = [(shift[k], empty_frame(p), (poses, maps[k], TIMESTAMP + k)) for k in range(3)]
        return scene("epochs" + ("-extract" if extract else ""), p, maps[0], ups,
                     env={"SUMA_NO_EXTRACT_FLAGS": "1"} if extract else None)
    return build


_SCENES["epochs"] = _epochs(False)
_SCENES["epochs-extract"] = _epochs(True)
EPOCH_IDS = ["epochs", "epochs-extract"]


def check_epochs(make_side):
    """every step on the one context equals the same step on a fresh one (no extraction: nothing else carries over)"""
    sc = get_scene("epochs")
    got = run_scene(make_side(sc["params"]), sc)
    for k, u in enumerate(sc["updates"]):
        fresh = make_side(sc["params"])
        fresh.load(*u[2])
        assert_results_equal([got[k]], [fresh.update(u[0], u[1])], f"epochs step {k} against a fresh context")
        keep = u[2][1]["confidence"] > 0
        assert got[k]["counts"] == (int(keep.sum()), 0)
        assert np.array_equal(got[k]["surfels"]["g"].astype(np.int64), np.flatnonzero(keep))


def test_epochs(oracle_lib):
    check_epochs(lambda p: OracleSide(oracle_lib, p))
    got = oracle_results("epochs-extract")
    assert [g["origin"] for g in got] == [(1, 0), (2, 0), (3, 0)] and all(g["size"] > 0 for g in got)
    for k, ij in enumerate(((-2, 2), (-1, 2), (0, 2))):  # what the standalone K12 took out of each map
        assert len(got[k]["tiles"][ij]) > 100


# ---- K11 / K12 edges -------------------------------------------------------------------------------------------------
def _area_edges():
    p = params(48, 12)
    E = float(UR.area(p, (0, 0), False)[2])  # 2 * 4 * 10 + 10 = 90, exact
    up, rec = np.nextafter(F32(E), F32(np.inf)), plain_records(np.ones(10, bool))
    rec["x"][:8] = [E, up, -E, -up, 1.0, 1.0, 1.0, 1.0]
    rec["y"][:8] = [1.0, 1.0, 1.0, 1.0, E, up, -E, -up]
    rec["timestamp"][8] = np.uint32(0x80000000 + 5)  # a negative stamp as the shader reads it
    keep = np.array([1, 0, 1, 0, 1, 0, 1, 0, 0, 1], bool)
    return scene("area-edges", p, rec, [(POSE_B, empty_frame(p))], expect=dict(k11=keep))


_SCENES["area-edges"] = _area_edges


def check_area_edges(got):
    sc = get_scene("area-edges")
    g = got[0]
    assert sc["params"].submap_extent == 10.0 and sc["params"].submap_dimension == 4
    assert g["counts"] == (10, 0), "every record survives K9 (the one with the negative stamp too: its confidence is high)"
    assert np.array_equal(g["surfels"]["g"].astype(np.int64), np.flatnonzero(sc["expect"]["k11"]))


def test_area_edges(oracle_lib):
    check_area_edges(oracle_results("area-edges"))


# ---- extraction paths --------------------------------------------------------------------------------------------------
EXTRACT_SUBMAP = dict(submap_extent=4.0, submap_dimension=2)
EXTRACT_TILE = (-2, 2)  # the last tile of the row pushed when the sensor moves on in +x: what a partial extraction takes


def floor_frame(p, pose):
    """a floor at z = -1.7 and a ceiling at z = 3 seen from `pose` (a yaw and a translation): every texel valid"""
    W, H = p.data_width, p.data_height
    T = np.asarray(pose, dtype=np.float64)
    d = K.texel_rays(W, H, p)
    dw = d @ T[:3, :3].T
    up = dw[..., 2] > 0
    s = np.where(up, 3.0 - T[2, 3], -1.7 - T[2, 3]) / dw[..., 2]
    V = np.ones((H, W, 4), dtype=F32)
    N = np.ones((H, W, 4), dtype=F32)
    V[..., :3] = s[..., None] * d
    N[..., :3] = np.where(up[..., None], (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)) @ T[:3, :3]
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    S = np.zeros((H, W, 4), dtype=F32)
    S[..., 0] = F32(40.0 / 255.0)
    S[..., 1], S[..., 2], S[..., 3] = ii, jj, 0.7
    return V, N, S


# records beside the grid, all inside or on the edge of the extracted tile (-2, 2) = [-20, -12] x [12, 20], all leaning (so
# that no measurement moves or re-stamps them): (x, y, fate) -- "in": |pos - c| == extent, in the tile; "out": one ulp beyond
# the tile's edge; "deleted": K9 deletes it (confidence -1, age 10); "dropped": K9 keeps it, K11 drops it (negative stamp)
_dn, _up32 = (lambda v: float(np.nextafter(F32(v), F32(-np.inf)))), (lambda v: float(np.nextafter(F32(v), F32(np.inf))))
FLOOR_EXTRAS = ((-12.0, 15.0, "in"), (_up32(-12.0), 17.0, "out"), (-20.0, 15.0, "in"), (_dn(-20.0), 17.0, "out"),
                (-15.0, 12.0, "in"), (-17.0, _dn(12.0), "out"), (-15.0, 20.0, "in"), (-17.0, _up32(20.0), "out"),
                (-15.0, 15.0, "deleted"), (-17.0, 13.0, "deleted"), (-13.0, 19.0, "deleted"),
                (-15.0, 17.0, "dropped"), (-13.0, 13.0, "dropped"), (-19.0, 19.0, "dropped"))
FLOOR_GRID = 21 * 21


def floor_records():
    """a 2 m grid of stable floor surfels over [-20, 20]^2, identity creation pose, and FLOOR_EXTRAS behind it"""
    g = np.arange(-20.0, 20.5, 2.0)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    assert len(xy) == FLOOR_GRID
    xy = np.concatenate([xy, [e[:2] for e in FLOOR_EXTRAS]])
    fate = np.array(["grid"] * FLOOR_GRID + [e[2] for e in FLOOR_EXTRAS])
    rec = plain_records(fate != "deleted")
    rec["x"], rec["y"], rec["z"], rec["nz"], rec["radius"] = xy[:, 0], xy[:, 1], -1.7, 1.0, 0.3
    rec["timestamp"][fate == "dropped"] = np.uint32(0x80000000 + 5)
    # three of four lean 60 degrees off the floor's normal: incompatible with the measurement, so their pixels stay
    # unmarked and K10 adds new surfels beside them
    lean = (((xy[:, 0] + 2 * xy[:, 1]) / 2).astype(np.int64) % 4 != 0) | (fate != "grid")
    rec["nx"], rec["nz"] = np.where(lean, np.sin(np.pi / 3), 0.0), np.where(lean, np.cos(np.pi / 3), 1.0)
    return rec


def _extraction(variant):
    def build():
        ov = dict(EXTRACT_SUBMAP)
        if variant == "all-at-once":
            ov["partial_extraction"] = 0
        p = params(512, 16, max_surfels=16384, **ov)
        poses = [K.pose_from(7.0, (4.5, 0.2, 0.0)), K.pose_from(-3.0, (-0.5, 0.1, 0.0)), K.pose_from(-3.0, (-0.5, 0.1, 0.0))]
        poses = [T.astype(F32).astype(np.float64) for T in poses]
        env = {"flags": {"SUMA_NO_FUSED_EXTRACT": "1"}, "standalone": {"SUMA_NO_EXTRACT_FLAGS": "1"}}.get(variant)
        return scene(f"extraction-{variant}", p, floor_records(), [(T, floor_frame(p, T)) for T in poses], env=env)
    return build


EXTRACT_VARIANTS = ("fused", "flags", "standalone", "all-at-once")
EXTRACT_IDS = [f"extraction-{v}" for v in EXTRACT_VARIANTS]
for _v in EXTRACT_VARIANTS:
    _SCENES[f"extraction-{_v}"] = _extraction(_v)


def check_extraction(results_of):
    """the same cached tile and the same map on every path; K9's records before K10's in the tile; the tile's records are
    fp64's predicate on the decided; the tile comes back into the map on the second update while another is flagged"""
    ref = results_of("extraction-fused")
    for v in ("flags", "standalone"):
        assert_results_equal(results_of(f"extraction-{v}"), ref, f"extraction-{v} against the fused path")
    p = get_scene("extraction-fused")["params"]
    first = ref[0]
    assert first["origin"] == (1, 0) and list(first["tiles"]) == [EXTRACT_TILE]
    tile = first["tiles"][EXTRACT_TILE].view(SURFEL_DTYPE).ravel()
    whole = results_of("extraction-all-at-once")[0]
    assert sorted(whole["tiles"]) == [(-2, j) for j in range(-2, 3)] and np.array_equal(whole["tiles"][EXTRACT_TILE], first["tiles"][EXTRACT_TILE])
    assert whole["surfels"].tobytes() == first["surfels"].tobytes()
    is_old = tile["b"] == F32(-1.0)
    n_old = int(is_old.sum())
    assert 10 <= n_old < len(tile) and is_old[:n_old].all(), "K9's records stand before K10's in the tile, and both occur"
    # fp64's predicate on the map the update left (every record: identity or the update's own pose -> world frame)
    m = first["surfels"]
    poses = get_scene("extraction-fused")["poses"].astype(np.float64).copy()
    poses[TIMESTAMP] = get_scene("extraction-fused")["updates"][0][0]
    Pm = poses[m["count"].astype(np.int64)]
    loc = np.stack([m["x"], m["y"], m["z"]], -1).astype(np.float64)
    world = np.einsum("nij,nj->ni", Pm[:, :3, :3], loc) + Pm[:, :3, 3]
    terms = np.einsum("nij,nj->ni", np.abs(Pm[:, :3, :3]), np.abs(loc)) + np.abs(Pm[:, :3, 3])
    inside, margin, eps = UR.tile_fp64(world, terms, p, *EXTRACT_TILE)
    dec = margin > eps
    key = lambda r: np.stack([r["g"], r["b"]], -1).astype(np.int64)  # noqa: E731
    want, have = key(m[inside & dec]), key(tile)
    have_dec = np.array([any((h == k).all() for k in key(m[dec])) for h in have])
    assert np.array_equal(have[have_dec], want), "the tile's records differ from fp64's predicate on the decided"
    # the extras: on the edge in, one ulp beyond out, and what K9 deleted or K11 dropped is not extracted although it
    # lies in the tile (the fused path ranks a record for the tile only if it is also emitted into the map)
    tile_ids = set(tile["g"][is_old].astype(np.int64).tolist())
    map_ids = set(m["g"][m["b"] == F32(-1.0)].astype(np.int64).tolist())
    for k, (x, y, fate) in enumerate(FLOOR_EXTRAS):
        i = FLOOR_GRID + k
        assert (i in tile_ids) == (fate == "in"), f"extra record {i} at ({x!r}, {y!r}), {fate}: in the tile = {i in tile_ids}"
        assert (i in map_ids) == (fate in ("in", "out") and abs(y) <= 20.0 and abs(x) <= 20.0), f"extra record {i} ({fate}) in the map"
    assert first["counts"][0] == len(floor_records()) - 3, "K9 deletes the three records meant for it, and only those"
    # second update: the sensor turns back, the parked tile is appended behind the map while tile (3, 2) is extracted
    second = ref[1]
    assert second["origin"] == (0, 0) and sorted(second["tiles"]) == [EXTRACT_TILE, (3, 2)]
    tail = second["surfels"][-len(tile):]
    assert tail.tobytes() == tile.tobytes(), "the appended tile stands behind the updated map, unchanged"
    assert sorted(ref[2]["tiles"]) == [EXTRACT_TILE, (3, 1), (3, 2)]


def test_extraction_rows(oracle_lib):
    check_extraction(oracle_results)


# ---- K10 shapes ------------------------------------------------------------------------------------------------------
K10_SHAPES = ((64, 16), (48, 10), (48, 12), (130, 16))  # the column-patch walk; the linear walk (two heights); two tiles and a part


def full_room_frame(p, pose):
    V, N = K.room_frames(p.data_width, p.data_height, p, pose)
    ii, jj = np.meshgrid(np.arange(p.data_width), np.arange(p.data_height))
    S = np.zeros(V.shape, dtype=F32)
    S[..., 0] = F32(40.0 / 255.0)
    S[..., 1], S[..., 2], S[..., 3] = ii, jj, 0.7
    return V, N, S


def _k10(W, H, kind):
    def build():
        p = params(W, H)
        V, N, S = full_room_frame(p, POSE_B)
        rec = plain_records(np.zeros(0, bool))
        if kind == "none":
            V, N, S = empty_frame(p)
        elif kind == "masked":  # one surfel on every measurement, three times as large: all averaged, every pixel marked
            v = V[..., :3].reshape(-1, 3).astype(np.float64)
            pw = v @ POSE_B[:3, :3].T + POSE_B[:3, 3]
            nw = N[..., :3].reshape(-1, 3).astype(np.float64) @ POSE_B[:3, :3].T
            tilt = np.cross(nw, [0.3, 0.5, 0.8])
            nw = nw + 0.05 * tilt
            nw /= np.linalg.norm(nw, axis=1, keepdims=True)
            rec = with_ids(RH.make_records(pw, nw, 3.0 * np.linalg.norm(v, axis=1) * UR.consts(p)["pixel_size"] * 1.41, 60, 140, 1.2))
            rec["r"], rec["w"] = F32(40.0 / 255.0), 0.5
        return scene(f"k10-{W}x{H}-{kind}", p, rec, [(POSE_B, (V, N, S))], expect=dict(kind=kind))
    return build


K10_IDS = [f"k10-{W}x{H}-{k}" for (W, H) in K10_SHAPES for k in ("all", "none", "masked")]
for (_W, _H) in K10_SHAPES:
    for _k in ("all", "none", "masked"):
        _SCENES[f"k10-{_W}x{_H}-{_k}"] = _k10(_W, _H, _k)


def check_k10_row(sid, got):
    sc = get_scene(sid)
    W, H, kind = sc["params"].data_width, sc["params"].data_height, sc["expect"]["kind"]
    g = got[0]
    if kind == "all":
        assert g["counts"] == (0, W * H) and g["size"] == W * H and not g["mask"].any()
        px = g["surfels"]["g"].astype(np.int64) * H + g["surfels"]["b"].astype(np.int64)
        assert np.array_equal(px, np.arange(W * H)), f"{sid}: the new surfels must come in x-major order"
    elif kind == "none":
        assert g["counts"] == (0, 0) and g["size"] == 0 and not g["mask"].any()
    else:
        assert g["mask"].all(), f"{sid}: {int((g['mask'] == 0).sum())} pixels not marked"
        assert g["counts"] == (W * H, 0) and g["size"] == W * H and np.all(colour_of(g["surfels"]) == UR.MAGENTA)


@pytest.mark.parametrize("sid", K10_IDS)
def test_k10_rows(oracle_lib, sid):
    got = oracle_results(sid)
    check_k10_row(sid, got)
    check_against_fp64(sid, got, f"oracle {sid}")


# ---- capacity --------------------------------------------------------------------------------------------------------
def _capacity(kind):
    def build():
        S = 1500 if kind == "k9-fills" else 1000  # max_surfels 1500 lies in the middle of the second K9 tile
        p = params(64, 16, max_surfels=1500)
        return scene(f"capacity-{kind}", p, plain_records(np.ones(S, bool)), [(POSE_B, full_room_frame(p, POSE_B))])
    return build


CAPACITY_IDS = ["capacity-k9-fills", "capacity-mid-k10"]
for _k in ("k9-fills", "mid-k10"):
    _SCENES[f"capacity-{_k}"] = _capacity(_k)


def check_capacity_row(sid, got):
    """S survivors and 1024 new surfels against max_surfels = 1500: the map is the first 1500 of them, in order"""
    S = len(get_scene(sid)["records"])
    out = got[0]["surfels"]
    assert len(out) == 1500 and np.array_equal(out["g"][:S].astype(np.int64), np.arange(S)) and np.all(out["b"][:S] == -1)
    px = out["g"][S:].astype(np.int64) * 16 + out["b"][S:].astype(np.int64)
    assert np.array_equal(px, np.arange(1500 - S))


@pytest.mark.parametrize("sid", CAPACITY_IDS)
def test_capacity_rows(oracle_lib, sid):
    check_capacity_row(sid, oracle_results(sid))


# ---------------------------------------------------------------------------------------------------------------------
# C. branch rows: one or two surfels against a frame of one valid pixel
# ---------------------------------------------------------------------------------------------------------------------
BW, BH, BPIX, BRANGE = 48, 12, (20, 6), 8.0
S_DEFAULT = dict(off=0.05, tilt=5.0, rscale=1.3, radius=None, conf=1.2, ts=TIMESTAMP - 10, creation=60, label=40.0, weight=1.0,
                 prob=0.5, at=BPIX, rng=BRANGE, label_raw=None)
P_DEFAULT = dict(at=BPIX, rng=BRANGE, ntilt=0.0, label=40.0, prob=0.7)


def _tilted(d, deg):
    """the unit vector -d turned by `deg` degrees about an axis across the ray"""
    a = np.cross(d, (0.0, 0.0, 1.0))
    a /= np.linalg.norm(a)
    t = np.deg2rad(float(deg))
    return np.cos(t) * (-d) + np.sin(t) * np.cross(a, -d)


def branch_scene(sid, surfels, pixels=({},), expect=None, pose=POSE_B, **pov):
    """surfels: dicts over S_DEFAULT -- the surfel sits on the ray of pixel `at`, `off` metres behind the point at range
    `rng`, its normal `tilt` degrees off the ray, its radius rscale x what K8 gives that point; pixels: dicts over
    P_DEFAULT -- the only valid texels of the frame, each a point at range `rng` on its ray, normal `ntilt` degrees off"""
    p = params(BW, BH, **pov)
    rays = K.texel_rays(BW, BH, p)
    T = np.asarray(pose, dtype=np.float64)
    px = []
    for q in pixels:
        q = {**P_DEFAULT, **q}
        d = rays[q["at"][1], q["at"][0]]
        px.append(dict(at=q["at"], v=q["rng"] * d, n=_tilted(d, q["ntilt"]), label=q["label"], prob=q["prob"]))
    (V, N, S), _ = K.single_pixel_frames(BW, BH, px, (0, 0, 0), (0, 0, 0))
    for q in px:
        S[q["at"][1], q["at"][0], 1:3] = q["at"]
    recs = []
    for k, s in enumerate(surfels):
        s = {**S_DEFAULT, **s}
        d = rays[s["at"][1], s["at"][0]]
        radius = s["radius"] if s["radius"] is not None else s["rscale"] * 1.41 * s["rng"] * UR.consts(p)["pixel_size"]
        r = RH.make_records(((s["rng"] + s["off"]) * d) @ T[:3, :3].T + T[:3, 3], _tilted(d, s["tilt"]) @ T[:3, :3].T, radius,
                            s["creation"], s["ts"], s["conf"])
        r["r"], r["w"], r["weight"] = F32(s["label"] / 255.0) if s["label_raw"] is None else s["label_raw"], s["prob"], s["weight"]
        recs.append(r)
    return scene(sid, p, with_ids(np.concatenate(recs)), [(T, (V, N, S))], expect=expect)


def oracle_run(sc):
    """(result, K9's fp32 terms) of a scene's first update on the oracle.  terms: n x 8 in the order of UR.TERM_FIELDS --
    x01 * W, y01 * H, imz, the front-face product, distance, angle from oracle/debug/o_update_terms.c; new_radius from
    the update's own radius_conf at the texel those coordinates name; the confidence before the cap from the surviving
    records (those below the cap; NaN for a record that did not survive), found by the id in their payload -- so the
    confidence EPS is measured on survivors only, and not at all with use_stability = 0"""
    from oracle import pyoracle
    pyoracle.build()
    o = OracleSide(pyoracle, sc["params"])
    o.load(sc["poses"], sc["records"], sc["timestamp"])
    pose, frame = sc["updates"][0][:2]
    f = o.o.frame()
    f.set(*frame)
    t6 = o.o.debug_update_terms(pose, f)
    res = o.update(pose, frame)
    n, (H, W) = len(sc["records"]), res["mask"].shape
    terms = np.full((n, 8), np.nan, dtype=F32)
    terms[:, :6] = t6
    with np.errstate(invalid="ignore"):
        tx, ty = np.floor(t6[:, 0]), np.floor(t6[:, 1])
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
    terms[ok, 6] = res["radius_conf"][ty[ok].astype(np.int64), tx[ok].astype(np.int64), 0]
    old = res["surfels"][res["surfels"]["b"] == F32(-1.0)]
    below = old["confidence"] < F32(20.0)
    if sc["params"].use_stability:  # without it the update leaves the confidence alone: nothing to measure
        terms[old["g"][below].astype(np.int64), 7] = old["confidence"][below]
    return res, terms


def flip(build, lo, hi, pred):
    """adjacent fp32 values (a, b) in [lo, hi], pred(oracle result of build(a)) false and of build(b) true; the knob is
    positive and pred monotone in it, so the bit patterns are bisected"""
    ia, ib = int(F32(lo).view(np.int32)), int(F32(hi).view(np.int32))
    val = lambda i: np.int32(i).view(F32)  # noqa: E731
    assert not pred(oracle_run(build(val(ia)))[0]) and pred(oracle_run(build(val(ib)))[0])
    while ib - ia > 1:
        m = (ia + ib) // 2
        if pred(oracle_run(build(val(m)))[0]):
            ib = m
        else:
            ia = m
    return val(ia), val(ib)


def _unmatched(res):
    out = res["surfels"]
    return len(out) == 0 or colour_of(out[:1])[0] in (UR.GREY, UR.CYAN)


# name: (scene of the knob, lo, hi, what flips from false to true, column of the oracle's terms, the gate's value)
# (a record stores its position in fp32: a surfel about 9 m from its creation pose moves in steps of 2^-20 m, so the
# distance gate -- and the gates on the range -- can be approached no closer than that)
GATES = {
    "distance": (lambda x: branch_scene("", [dict(off=x)]), 0.1, 0.4, _unmatched, 4, lambda p, k: float(p.map_max_distance)),
    "angle": (lambda x: branch_scene("", [dict(tilt=x)]), 40.0, 50.0, _unmatched, 5, lambda p, k: k["angle_thresh"]),
    "front": (lambda x: branch_scene("", [dict(tilt=x, off=0.0)], [dict(ntilt=60.0)]), 85.0, 95.0, _unmatched, 3, lambda p, k: 0.0),
    "imz-1": (lambda x: branch_scene("", [dict(rng=x)], [dict(rng=x)]), 74.0, 76.0, _unmatched, 2, lambda p, k: 1.0),
    "zclip-0": (lambda x: branch_scene("", [dict(rng=x)], [dict(rng=x)]), 1.9, 2.1, lambda r: bool(r["mask"][BPIX[1], BPIX[0]]), 2,
                lambda p, k: 0.0),
    "log-unstable": (lambda x: branch_scene("", [dict(off=1.0, conf=-x, ts=TIMESTAMP - 1)]), 1e-9, 0.5, lambda r: r["counts"][0] == 0, 7,
                     lambda p, k: k["log_unstable"]),
}
GATE_IDS = [f"gate-{g}-{side}" for g in GATES for side in ("below", "above")]


@lru_cache(maxsize=None)
def gate_knobs(name):
    build, lo, hi, pred = GATES[name][:4]
    return flip(build, lo, hi, pred)


for _g in GATES:
    for _k, _side in enumerate(("below", "above")):
        _SCENES[f"gate-{_g}-{_side}"] = (lambda g, k, side: lambda: {**GATES[g][0](gate_knobs(g)[k]), "id": f"gate-{g}-{side}"})(_g, _k, _side)


def check_gate_rows(results_of, name):
    """the two neighbouring inputs end on different sides of the gate"""
    pred = GATES[name][3]
    assert not pred(results_of(f"gate-{name}-below")[0]) and pred(results_of(f"gate-{name}-above")[0]), name


@pytest.mark.parametrize("name", list(GATES))
def test_gate_rows(oracle_lib, name):
    """precondition: the oracle's fp32 term stands within 8 ulps of the gate's value (8 position steps for the distance)
    at both inputs, which are one ulp of the knob apart"""
    a, b = gate_knobs(name)
    assert np.nextafter(a, F32(np.inf)) == b
    col, thr = GATES[name][4], GATES[name][5]
    for side in ("below", "above"):
        sc = get_scene(f"gate-{name}-{side}")
        term = float(oracle_run(sc)[1][0, col])
        if name == "log-unstable" and side == "above":
            assert np.isnan(term), "the record is deleted: its confidence cannot be read"
            continue
        t = thr(sc["params"], UR.consts(sc["params"]))
        step = 2.0 ** -20 if name == "distance" else max(float(np.spacing(F32(abs(t)))), 2.0 ** -24)
        assert abs(term - t) <= 8 * step, f"{name}-{side}: term {term!r} against {t!r}"
        check_against_fp64(sc["id"], oracle_results(sc["id"]), f"oracle {sc['id']}")
    check_gate_rows(oracle_results, name)


def _k8_radius(rng=BRANGE):
    """the fp32 radius K8 gives the default measurement pixel, read from the oracle"""
    return oracle_run(branch_scene("", [dict()], [dict(rng=rng)]))[0]["radius_conf"][BPIX[1], BPIX[0], 0]


# every integer label L survives float32(L / 255) * 255 in fp32 (checked below), so the label that does not round-trip is
# the stored value next to it: x * 255 = 10.000001 rounds to 10 for the comparison but is not == 10 for the dynamic classes
LABEL_OFF = np.nextafter(F32(10.0 / 255.0), F32(1.0))


EMPTY_PIXEL = (30, 6)  # no measurement there: the surfel is neither matched nor K7-penalised
_up, _down = (lambda x: np.nextafter(F32(x), F32(np.inf))), (lambda x: np.nextafter(F32(x), F32(-np.inf)))
# id: (scene builder, expected colour per input record -- UR.DELETED for a record that must go --, or None)
BRANCHES = {
    "active-99": (lambda: branch_scene("", [dict(creation=TIMESTAMP - 99)]), [UR.MAGENTA]),
    "active-100": (lambda: branch_scene("", [dict(creation=TIMESTAMP - 100)]), [UR.GREEN]),
    "age-2": (lambda: branch_scene("", [dict(at=EMPTY_PIXEL, conf=-0.2, ts=TIMESTAMP - 2)]), [UR.GREY]),
    "age-3": (lambda: branch_scene("", [dict(at=EMPTY_PIXEL, conf=-0.2, ts=TIMESTAMP - 3)]), [UR.DELETED]),
    "threshold-below": (lambda: branch_scene("", [dict(at=EMPTY_PIXEL, conf=_down(0.5))], confidence_threshold=0.5), [UR.DELETED]),
    "threshold-at": (lambda: branch_scene("", [dict(at=EMPTY_PIXEL, conf=0.5)], confidence_threshold=0.5), [UR.GREY]),
    "radius-below": (lambda: branch_scene("", [dict(radius=_down(_k8_radius()))]), [UR.GREEN]),
    "radius-equal": (lambda: branch_scene("", [dict(radius=_k8_radius())]), [UR.GREEN]),
    "radius-above": (lambda: branch_scene("", [dict(radius=_up(_k8_radius()))]), [UR.MAGENTA]),
    "cap-20": (lambda: branch_scene("", [dict(conf=19.9), dict(conf=19.0, at=(25, 6))], [dict(), dict(at=(25, 6))]), [UR.MAGENTA] * 2),
    "max-weight": (lambda: branch_scene("", [dict(weight=19.5), dict(weight=18.5, at=(25, 6))], [dict(), dict(at=(25, 6))],
                                       weighting_scheme=1), [UR.MAGENTA] * 2),
    "penalty-model-label": (lambda: branch_scene("", [dict(label=10.0)], [dict(label=40.0)]), [UR.MAGENTA]),
    "penalty-data-label": (lambda: branch_scene("", [dict(label=40.0)], [dict(label=10.0)]), [UR.MAGENTA]),
    "penalty-equal-labels": (lambda: branch_scene("", [dict(label=10.0)], [dict(label=10.0)]), [UR.MAGENTA]),
    "label-no-roundtrip-differs": (lambda: branch_scene("", [dict(label_raw=LABEL_OFF)], [dict(label=40.0)]), [UR.MAGENTA]),
    "label-no-roundtrip-equals": (lambda: branch_scene("", [dict(label_raw=LABEL_OFF)], [dict(label=10.0)]), [UR.MAGENTA]),
    "winner-first": (lambda: branch_scene("", [dict(off=-1.0), dict(off=1.0)]), [UR.CYAN, UR.GREY]),
    "winner-second": (lambda: branch_scene("", [dict(off=1.0), dict(off=-1.0)]), [UR.GREY, UR.CYAN]),
    "slerp-identical": (lambda: branch_scene("", [dict(tilt=0.0)]), [UR.MAGENTA]),
    "slerp-179": (lambda: branch_scene("", [dict(tilt=0.0)], [dict(ntilt=179.0)]), [UR.MAGENTA]),
    "top-row": (lambda: branch_scene("", [dict(at=(20, 0))], [dict(at=(20, 0))]), [UR.MAGENTA]),
    "bottom-row": (lambda: branch_scene("", [dict(at=(20, BH - 1))], [dict(at=(20, BH - 1))]), [UR.MAGENTA]),
}


def _seam(sign):
    """a surfel a hair to one side of yaw = +-pi, identity poses throughout: +: pixel column 0; -: x01 = 1, outside"""
    def build():
        p = params(BW, BH)
        pt = np.array([-8.0, sign * 1e-30, -1.0])
        row = int(np.floor(UR.R.project(p.data_fov_up, p.data_fov_down, p.min_depth, p.max_depth, pt)[1] * BH))
        V, N, S = empty_frame(p)
        for x in (0, BW - 1):
            V[row, x], N[row, x], S[row, x] = (*pt, 1.0), (1.0, 0.0, 0.0, 1.0), (F32(40.0 / 255.0), x, row, 0.7)
        rec = plain_records(np.ones(1, bool))
        rec["x"], rec["y"], rec["z"], rec["nx"], rec["nz"], rec["radius"], rec["confidence"] = pt[0], pt[1], pt[2], 1.0, 0.0, 1.0, 1.2
        return scene("", p, rec, [(np.eye(4), (V, N, S))])
    return build


def _distance_exact():
    """distance == map_max_distance to the bit (identity poses, everything on the x axis: the surfel at 0.2f, the
    measurement at 2 * 0.2f, their difference and its product with the normal (-1, 0, 0) exact): not compatible"""
    p = params(BW, BH)
    d = F32(p.map_max_distance)
    V, N, S = empty_frame(p)
    V[10, 24], N[10, 24], S[10, 24] = (2 * d, 0.0, 0.0, 1.0), (-1.0, 0.0, 0.0, 1.0), (F32(40.0 / 255.0), 24, 10, 0.7)
    rec = plain_records(np.ones(1, bool))
    rec["x"], rec["y"], rec["z"], rec["nx"], rec["nz"], rec["radius"], rec["confidence"] = d, 0.0, 0.0, -1.0, 0.0, 1.0, 1.2
    return scene("", p, rec, [(np.eye(4), (V, N, S))])


def test_distance_exact_precondition(oracle_lib):
    sc = get_scene("branch-distance-exact")
    assert oracle_run(sc)[1][0, 4] == F32(sc["params"].map_max_distance)


BRANCHES["distance-exact"] = (_distance_exact, [UR.GREY])
BRANCHES["seam-plus"] = (_seam(1.0), [UR.GREEN])
BRANCHES["seam-minus"] = (_seam(-1.0), [UR.GREY])
BRANCH_IDS = [f"branch-{b}" for b in BRANCHES]
for _b in BRANCHES:
    _SCENES[f"branch-{_b}"] = (lambda b: lambda: {**BRANCHES[b][0](), "id": f"branch-{b}", "expect": dict(colours=BRANCHES[b][1])})(_b)


def check_branch_row(sid, got):
    """the stated outcome per input record, then whatever else fp64 decides"""
    sc = get_scene(sid)
    out = got[0]["surfels"]
    old = out[out["b"] == F32(-1.0)]
    have = np.full(len(sc["records"]), UR.DELETED)
    have[old["g"].astype(np.int64)] = colour_of(old)
    assert have.tolist() == list(sc["expect"]["colours"]), f"{sid}: outcomes {have.tolist()}, stated {sc['expect']['colours']}"
    rec = sc["records"]
    name = sid[len("branch-"):]
    if name == "cap-20":
        assert old["confidence"][0] == F32(20.0) and old["confidence"][1] < F32(20.0)
    elif name == "max-weight":
        assert old["weight"].tolist() == [20.0, 19.5]
    elif name.startswith("penalty") or name.startswith("label"):
        gain = float(old["confidence"][0]) - float(rec["confidence"][0])
        assert (gain < -0.5) == (name == "penalty-model-label"), f"{sid}: confidence changed by {gain}"
        V, N, S = sc["updates"][0][1]
        p_data = float(S[BPIX[1], BPIX[0], 3])
        if name in ("label-no-roundtrip-equals", "penalty-equal-labels"):  # equal after round(): the data probability as it is
            assert abs(float(old["w"][0]) - (0.9 * 0.5 + 0.1 * p_data)) < 1e-6
        else:
            assert abs(float(old["w"][0]) - (0.9 * 0.5 + 0.1 * (1 - p_data))) < 1e-6
    elif name == "slerp-identical":
        assert np.max(np.abs(np.stack([old[c] - rec[c] for c in ("nx", "ny", "nz")]))) < 1e-6 and np.isfinite(old["nx"][0])
    elif name == "slerp-179":
        assert old["radius"][0] == 0.0 and got[0]["radius_conf"][BPIX[1], BPIX[0], 3] == 0.0
        n1 = np.array([old[c][0] for c in ("nx", "ny", "nz")], dtype=np.float64)
        n0 = np.array([rec[c][0] for c in ("nx", "ny", "nz")], dtype=np.float64)
        assert abs(np.linalg.norm(n1) - 1) < 1e-6 and abs(np.degrees(np.arccos(n1 @ n0)) - 17.9) < 0.01, "a tenth of the way round"
    elif name.startswith("seam"):
        assert int(got[0]["mask"].sum()) == (1 if name == "seam-plus" else 0) and got[0]["mask"][:, 0].sum() == got[0]["mask"].sum()


@pytest.mark.parametrize("sid", BRANCH_IDS)
def test_branch_rows(oracle_lib, sid):
    got = oracle_results(sid)
    check_branch_row(sid, got)
    check_against_fp64(sid, got, f"oracle {sid}")


# ---- non-finite and zero inputs: nothing faults, the outcomes are the oracle's ---------------------------------------
BAD_VALUES = (np.nan, np.inf, -np.inf, 0.0)


def _bad_records():
    p = params(64, 16, max_surfels=8192)
    base = get_scene("room64x16-default")["records"].copy()
    k = 0
    for fields in (("x",), ("x", "y", "z"), ("nx",), ("nx", "ny", "nz"), ("radius",), ("confidence",), ("weight",), ("w",), ("r",)):
        for v in BAD_VALUES:
            for f in fields:
                base[f][37 + 11 * k] = v
            k += 1
    return scene("bad-records", p, base, get_scene("room64x16-default")["updates"])


def _bad_texels():
    sc = get_scene("room64x16-default")
    V, N, S = (m.copy() for m in sc["updates"][0][1])
    k = 0
    for m in (V, N, S):
        for ch in range(4):
            for v in BAD_VALUES:
                m[(3 + 5 * k) % 16, (7 + 13 * k) % 64, ch] = v
                k += 1
    return scene("bad-texels", sc["params"], sc["records"].copy(), [(POSE_B, (V, N, S))])


_SCENES["bad-records"] = _bad_records
_SCENES["bad-texels"] = _bad_texels
BAD_IDS = ["bad-records", "bad-texels"]


def check_bad_row(sid, got):
    """every record's count stays inside the pose table's domain, and the survivors keep their input order"""
    out = got[0]["surfels"]
    assert np.all((out["count"] >= 0) & (out["count"] < N_POSES) & (out["count"] == np.floor(out["count"])))
    ids = out["g"][out["b"] == F32(-1.0)]
    assert np.all(np.diff(ids) > 0) and len(ids) > 300


@pytest.mark.parametrize("sid", BAD_IDS)
def test_bad_rows(oracle_lib, sid):
    check_bad_row(sid, oracle_results(sid))


def test_count_domain_of_every_scene():
    """suma_map_upload's domain (include/suma_hip.h): every record's `count` is an integer in [0, max_poses)"""
    for sid in ROW_IDS + ROOM_IDS:
        sc = get_scene(sid)
        for rec in [sc["records"]] + [u[2][1] for u in sc["updates"] if len(u) == 3]:
            c = rec["count"]
            assert np.all((c >= 0) & (c < sc["params"].max_poses) & (c == np.floor(c))), sid
            assert len(rec) <= sc["params"].max_surfels


# every row that is compared with the oracle bit for bit on the GPU
ROW_IDS = KEEP_ROW_IDS + GRID_IDS + EPOCH_IDS + ["area-edges"] + EXTRACT_IDS + K10_IDS + GATE_IDS + BRANCH_IDS + BAD_IDS


def test_label_that_does_not_round_trip():
    """precondition of the label rows: every integer label survives float32(L / 255) * 255, the neighbouring stored value
    does not -- it rounds to 10 but is not equal to 10"""
    assert all(F32(L / 255.0) * F32(255.0) == F32(L) for L in range(256))
    lab = LABEL_OFF * F32(255.0)
    assert lab != F32(10.0) and np.floor(lab + F32(0.5)) == 10.0
