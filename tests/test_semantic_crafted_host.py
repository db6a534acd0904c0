"""The semantic front end (k_semantic.hip) and the KNN vote (k_semantic_knn.hip) on crafted scans, CPU side: pins the
host restatements (tests/semantic_shim.c, tests/semantic_knn_shim.c) against a plain fp64 statement of the stages
(tests/semantic_ref.py), proves each row's property, and fixes the inputs that tests/test_gpu_semantic_crafted.py runs
through the kernels.  get_scene(id) builds every scene once; check_projection / check_unproject / check_knn hold a result
(the shim's here, the kernel's there) against fp64 under the margins of semantic_ref.py and against the row's property.

A point or pixel is DECIDED when its margins exceed their bounds (derived in semantic_ref.py's docstring, confirmed here):
the decision -- pixel, winner, label, which voter's prob -- must then equal fp64's exactly, the values within tolerance.
Constructed rows must have 0 undecided, random scenes at most 2 % of the points and 2 % of the pixels (CAP); both are
asserted on the shim here, before a GPU sees the scene.

MEASURED (test_measured_bounds; the largest margin, in units of its derived bound, at which the shim and fp64 decide
differently -- the bound used is max(derived, 2 x measured), so below 0.5 the derived one stands):
    texel 0.098   (four geometries, points swept across column and row boundaries in tenths of the bound, three ranges)
    gap   0.239   (200 directions, range pairs up to six fp32 steps either side of a tie)
    top2  none    (1024 logit pairs, 0 .. 16 fp32 steps apart, either class order: no disagreement at any gap)
    sel   0.202   cut 0.117   (60 off-axis triples, the neighbours' d a quarter step of the range apart / at the cutoff)
  semantic_ref.MEASURED records them rounded up (0.10, 0.24, 0, 0.21, 0.12).  Values on the decided: the planes reach
  0.75 of their derived tolerance, the softmax prob 0.14 of its.
UNDECIDED on the shim, per scene: 0 in every constructed row (centres 32 scenes, straddle 32, zfight 4, specials 1,
  back-projection 20, grid 119, equal 10, mirror 4, tie31 4, emptyvote 16, cuteq 10, negzero 10, cutprob 5, hidden3 5,
  inconsistent 10, outside 4, badproj 3, all81 2); 0 points and 0 pixels in each of the twelve random projection scenes
  and 0 of 400 points in each of the eight random KNN scenes (cap 2 %).  The follow-up back-projections that the
  projection scenes carry (random scores on the projected pixels) have no cap: their generic ranges tie within the
  bound by construction of the centres; fp64 holds what it decides of them.

Scenes.
  projection (PROJ_IDS), W x H in 1x1 1x5 7x1 2x3 33x5 64x16 130x4 257x3, (fov_up, fov_down) in (3, -25) (10, -30)
  (0.5, -0.5) (-5, -25):
    centres    one point in the middle of every pixel, shuffled: every point lands in the pixel it was made for
    straddle   pairs 1/64 pixel on either side of column and row boundaries, of u = 0 | W (the seam) and v = 0 | H (the
               clamp), the seam itself (x < 0, y = +0, -0, +-1e-3), straight up and down, the four axes
    zfight     on the x axis ranges one fp32 step apart (the depth is exact there), the nearest at the HIGHEST index;
               exact duplicates at i, i + 256, i + 512 (the atomicMin of three blocks meet): the lowest index wins and
               plane 4 carries ITS remission
    specials   zero range, NaN, +-inf, overflowing and underflowing ranges (not projected), a subnormal coordinate
               beside a normal one (projected)
    random     n in 0 1 63 64 65 255 256 257 1000 generic points, wider than the field of view
    on every scene: an empty pixel is +0 in all five planes with proj_idx -1; a filled one is within the derived
    tolerance of (v - mean) / std, the depth plane's absolute; proj_idx and pixel name each other.
    SEQUENCES lists the orders the GPU file runs on ONE context: full scan, n = 0, one point, full scan; and
    64x16 -> 7x1 -> 64x16 -> 257x3.
  back-projection (UNPROJ_IDS), C in 1 2 19 20 32 on P = 520 (130x4) and P = 5 (5x1), one case per pixel in turn, the
  pixel array interleaving valid pixels with -1, INT32_MIN, P, P + 1, INT32_MAX inside every wave; label_map holds 259,
  0, a negative id and 16777217 (not a float: the cast rounds to 16777216):
    probabilities  random; the maximum at class 0, at class C - 1, at both (the last wins); all negative; all +0; all
                   -0.0 (the last class, prob -0.0, sign checked); NaN in one plane, in all; +inf; subnormals; all equal
    logits         random x1, x8; all equal (the last class, prob 1 / C); spread above 104 (the others underflow, prob
                   1); +-3e38; one +inf; one -inf among finite; all -inf; one NaN
  KNN (KNN_IDS): the grid (S, k) of GRID on the images 1x1 1x7 7x1 3x3 4x9 24x10 130x4, sigma in 1e-30 0.5 1 1e30, cutoff
  in -5 0 0.5 1 3e38 in rotation, C = 32: on-axis points with exact ranges, empty pixels, hidden points, classes none / 0
  / 1 / 2 / 7 / 31, the bad pixel values; and the rows
    equal        every range equal: all d = 0, the selection is the t rule alone
    mirror       neighbours at ri - D and ri + D tie in d: the lower t is taken
    cuteq        d exactly equal to cutoff = fl(D w[t]), D a power of two: votes; at nextafter(cutoff, 0): does not
    emptyvote    empty neighbours, k = S^2: they vote at cutoff <= 0 and not at cutoff > 0
    outside      out-of-image slots (range 0) nearest to a point at 0.5 m: they carry no class
    all81        one class takes every vote (81 at S = 9: seven bit planes, a full carry chain); class 31 alone
    tie31        four votes each for class 31 and class 1: the lower wins
    negzero      a sole voter with prob -0.0 is reported as -0.0; next to a +0 voter of its class, +0
    cutprob      a cut-off neighbour of the winning class with the largest prob is not reported
    hidden3      three hidden points on one pixel, at different ranges
    badproj      proj_idx in -1, n, INT32_MIN, INT32_MAX: an empty pixel
    inconsistent pixel >= 0 on points whose coordinates are NaN, inf, zero, overflowing or underflowing: (0, 0) by rule 3
                 of the specification.  Before that rule existed the shim reported such a point's pixel class for inf /
                 zero / overflowing ranges but, with a NaN range, (0, 0) at k = 1 (its insertion sort is not an order
                 with a NaN key, the centre does not come first) where the kernel's centre-first form reports the class
    random       24x10, 400 generic points, C = 32, probabilities and logits, judged by margins under the cap
"""
import atexit
import ctypes as C
import functools
import shutil
import tempfile

import numpy as np
import pytest

import semantic_ref as R
from semantic_suma_amd.segmentation import semantic_knn
from test_semantic_host import build_shim, make_params
from test_semantic_host import project as shim_project
from test_semantic_host import unproject as shim_unproject
from test_semantic_knn_host import Scene, build_knn_shim, knn_unproject

F32 = np.float32
CAP = 0.02
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

GEOS = [(1, 1), (1, 5), (7, 1), (2, 3), (33, 5), (64, 16), (130, 4), (257, 3)]
FOVS = [(3.0, -25.0), (10.0, -30.0), (0.5, -0.5), (-5.0, -25.0)]
RANDOM = [(0, (64, 16), 0), (1, (64, 16), 0), (1000, (64, 16), 0), (63, (33, 5), 1), (64, (130, 4), 1),
          (65, (257, 3), 2), (255, (2, 3), 3), (256, (7, 1), 0), (257, (1, 5), 1), (1000, (130, 4), 3), (1, (1, 1), 2),
          (0, (1, 1), 1)]
CLASSES = [1, 2, 19, 20, 32]
GRID = [(1, 1), (3, 1), (3, 2), (3, 8), (3, 9), (5, 1), (5, 4), (5, 5), (5, 6), (5, 25), (7, 2), (7, 25), (7, 49),
        (9, 2), (9, 16), (9, 80), (9, 81)]
SIGMAS = [1e-30, 0.5, 1.0, 1e30]
CUTOFFS = [-5.0, 0.0, 0.5, 1.0, 3e38]
IMAGES = [(1, 1), (1, 7), (7, 1), (3, 3), (4, 9), (24, 10), (130, 4)]
PATHS_FULL = [(3, 9), (5, 5), (5, 25), (7, 49), (9, 81)]  # every kk_points instantiation that has neighbours
LM32 = [259, 77, -7, 16777217, 0] + [10 * j + 3 for j in range(5, 32)]  # 0 at class 4: a label, not "no class"


@functools.lru_cache(maxsize=None)
def shims():
    d = tempfile.mkdtemp(prefix="semantic_crafted")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return build_shim(d), build_knn_shim(d)


def params(W, H, fov=0, n_classes=20, label_map=None):
    lm = LM32[:n_classes] if label_map is None else label_map
    return make_params(width=W, height=H, fov_up=FOVS[fov][0], fov_down=FOVS[fov][1], n_classes=n_classes, label_map=lm)


def point_at(sp, vc, uc, r, rem=0.3):
    """the point at range r whose continuous image coordinates are (uc, vc)"""
    fdown = np.radians(abs(sp.fov_down))
    fov = np.radians(abs(sp.fov_up) + abs(sp.fov_down))
    yaw = (2.0 * uc / sp.width - 1.0) * np.pi
    pitch = (1.0 - vc / sp.height) * fov - fdown
    return [r * np.cos(pitch) * np.cos(-yaw), r * np.cos(pitch) * np.sin(-yaw), r * np.sin(pitch), rem]


def cell(sp, vc, uc):
    return int(np.clip(np.floor(vc), 0, sp.height - 1)) * sp.width + int(np.clip(np.floor(uc), 0, sp.width - 1))


# ---------------------------------------------------------------------------------------------------------------------
# projection scenes
# ---------------------------------------------------------------------------------------------------------------------
def _proj(sp, pts, expect=None, winners=None, random=False):
    pts = np.ascontiguousarray(np.array(pts, F32).reshape(-1, 4))
    expect = np.full(pts.shape[0], -2, np.int64) if expect is None else np.asarray(expect, np.int64)
    return dict(kind="proj", sp=sp, pts=pts, expect=expect, winners=winners or {}, random=random)


def proj_centres(W, H, fov):
    sp = params(W, H, fov)
    order = np.random.default_rng(W * 100 + H).permutation(W * H)
    pts = [point_at(sp, p // W + 0.5, p % W + 0.5, 3.0 + 0.75 * (p % 5), (p % 10) / 10.0) for p in order]
    return _proj(sp, pts, order)


def proj_straddle(W, H, fov):
    sp = params(W, H, fov)
    pts, expect = [], []

    def add(vc, uc):
        pts.append(point_at(sp, vc, uc, 5.0 + 0.61 * len(pts), 0.1 * (len(pts) % 9)))  # no two ranges alike
        expect.append(cell(sp, vc, uc))

    e = 1.0 / 64.0
    for b in sorted({1, W // 2, W - 1} & set(range(1, W))):
        for vc in (0.5, H - 0.5):
            add(vc, b - e), add(vc, b + e)
    for b in sorted({1, H // 2, H - 1} & set(range(1, H))):
        for uc in (0.5, W - 0.5, W / 2.0 + 0.25):
            add(b - e, uc), add(b + e, uc)
    for vc in (-e, e, H - e, H + e, -0.75 * H, 1.75 * H):  # above fov_up clamps to row 0, below fov_down to H - 1
        add(vc, e), add(vc, W - e)  # u at 0 and at W: either side of the seam
    # the seam, the axes, straight up and down.  In the horizontal plane the points are lifted into the middle of row
    # H // 2 (tan of its pitch); on the horizon itself (z = 0) only where that is no row boundary
    mid = point_at(sp, H // 2 + 0.5, 0.5 * W, 1.0)
    lift = mid[2] / np.hypot(mid[0], mid[1])
    v0 = (1.0 - abs(sp.fov_down) / (abs(sp.fov_up) + abs(sp.fov_down))) * H
    flat = [([-40.0, 0.0], 0), ([-41.0, -0.0], 0), ([-42.0, 1e-3], 0), ([-43.0, -1e-3], W - 1), ([44.0, 0.0], W // 2)]
    if W % 4:
        flat += [([0.0, 48.0], W // 4), ([0.0, -49.0], (3 * W) // 4)]
    for (xy, col) in flat:
        pts.append(xy + [lift * np.hypot(*xy), 0.5])
        expect.append((H // 2) * W + col)
        if 0.1 < v0 % 1.0 < 0.9:
            pts.append([1.5 * c for c in xy] + [0.0, 0.4])
            expect.append(int(v0) * W + col)
    for (xyz, col) in (([0.0, 0.0, 45.0], W // 2), ([0.0, 0.0, -46.0], (H - 1) * W + W // 2), ([-0.0, -0.0, 47.0], W // 2)):
        pts.append(xyz + [0.5])
        expect.append(col)  # straight up: row 0; down: row H - 1
    return _proj(sp, pts, expect)


def proj_zfight(W, H):
    sp = params(W, H, 0)
    n = 3 * 256 + 40
    pts = np.zeros((n, 4), F32)  # fillers: zero range, not projected
    pts[:, 3] = 0.9
    winners = {}
    dup = min(W * H, 24)
    for i in range(dup):  # exact duplicates in three blocks
        p = (i * 7) % (W * H)
        if p == cell(sp, *_axis_cell(sp)):
            continue
        q = point_at(sp, p // W + 0.5, p % W + 0.5, 6.0 + i)
        for b in range(3):
            pts[i + 256 * b] = q[:3] + [0.1 + 0.2 * b]
        pts[i + 128] = [2 * c for c in q[:3]] + [0.8]  # farther, a lower index than two of the copies: loses
        winners[p] = i
    # the x axis: exact depths one fp32 step apart, the nearest last
    r = F32(9.0)
    steps = [r + 3 * np.spacing(r), r + 2 * np.spacing(r), r + np.spacing(r), r]
    for j, rr in enumerate(steps):
        pts[300 + 150 * j] = [rr, 0.0, 0.0, 0.2 + 0.1 * j]
    pts[n - 1] = [r, 0.0, 0.0, 0.7]  # and its duplicate later still
    winners[cell(sp, *_axis_cell(sp))] = 300 + 150 * 3
    return _proj(sp, pts, winners=winners)


def _axis_cell(sp):
    """continuous (v, u) of the +x axis"""
    fdown, fov = abs(sp.fov_down), abs(sp.fov_up) + abs(sp.fov_down)
    return (1.0 - fdown / fov) * sp.height, sp.width / 2.0


def proj_specials():
    sp = params(64, 16, 0)
    nan, inf = np.nan, np.inf
    bad = [[0, 0, 0], [nan, 1, 1], [1, nan, 1], [1, 1, nan], [inf, 0, 0], [0, -inf, 0], [1, 2, inf], [3e20, 3e20, 0],
           [3e38, 0, 0], [0, 0, -2e19], [1e-30, 0, 0], [1e-30, -1e-30, 1e-30], [1e-45, 0, 0], [-0.0, 0.0, -0.0]]
    good = [[3.0, 2.0, 1e-40], [-5.0, 1e-42, -0.3], [10.0, 1.0, 0.5], [-4.0, 2.0, -1.5], [1e15, 2e15, -1e14],
            [1e-15, 2e-15, -3e-16]]
    pts = [b + [0.3] for b in bad] + [g + [0.6] for g in good]
    sc = _proj(sp, pts, [-1] * len(bad) + [-2] * len(good))
    sc["projected"] = list(range(len(bad), len(pts)))
    return sc


def proj_random(n, geo, fov):
    sp = params(geo[0], geo[1], fov)
    rng = np.random.default_rng(1000 * n + geo[0])
    up, down = abs(FOVS[fov][0]), abs(FOVS[fov][1])
    yaw = rng.uniform(-np.pi, np.pi, n)
    pitch = np.radians(rng.uniform(-down - 6.0, up + 6.0, n))
    r = np.exp(rng.uniform(np.log(2.0), np.log(60.0), n))
    pts = np.stack([r * np.cos(pitch) * np.cos(yaw), r * np.cos(pitch) * np.sin(yaw), r * np.sin(pitch),
                    rng.uniform(0, 1, n)], 1)
    return _proj(sp, pts, random=True)


# ---------------------------------------------------------------------------------------------------------------------
# back-projection scenes
# ---------------------------------------------------------------------------------------------------------------------
PROB_KINDS = ["random", "max0", "maxlast", "maxboth", "negative", "zero", "negzero", "nan1", "nanall", "inf", "subnormal",
              "equal"]
LOGIT_KINDS = ["random1", "random8", "equal", "spread", "huge", "posinf", "neginf1", "neginfall", "nan1"]


def crafted_pixels(P, n_min=0):
    """valid pixels in order with one bad value after every fourth: never a whole wave of either"""
    bad = [-1, I32_MIN, P, P + 1, I32_MAX]
    out = []
    p = 0
    while p < P or len(out) < n_min:
        out.append(p % P)
        p += 1
        if p % 4 == 0:
            out.append(bad[(p // 4) % 5])
    return np.array(out, np.int32)


def unproj_scene(Cn, big, logits):
    W, H = (130, 4) if big else (5, 1)
    P = W * H
    sp = params(W, H, 0, n_classes=Cn)
    rng = np.random.default_rng(Cn * 10 + big * 2 + logits)
    kinds = LOGIT_KINDS if logits else PROB_KINDS
    s = np.zeros((Cn, P), F32)
    kind = [kinds[(p + p // len(kinds)) % len(kinds)] if big else kinds[(p * 2 + Cn) % len(kinds)] for p in range(P)]
    cls = np.full(P, -2, np.int64)   # the class the row states: -1 none, -2 fp64's to say
    prob = [None] * P
    last = Cn - 1
    for p, kd in enumerate(kind):
        j = p % Cn
        if kd == "random":
            s[:, p] = rng.uniform(-0.2, 1.0, Cn)
        elif kd in ("max0", "maxlast", "maxboth"):
            s[:, p] = rng.uniform(-0.2, 0.8, Cn)
            if kd != "maxlast":
                s[0, p] = 0.9
            if kd != "max0":
                s[last, p] = 0.9
            cls[p], prob[p] = (0 if kd == "max0" else last), F32(0.9)
        elif kd == "negative":
            s[:, p] = -rng.uniform(0.01, 1.0, Cn)
            cls[p], prob[p] = -1, F32(0.0)
        elif kd == "zero":
            cls[p], prob[p] = last, F32(0.0)
        elif kd == "negzero":
            s[:, p] = -0.0
            cls[p], prob[p] = last, F32(-0.0)
        elif kd == "nan1":
            s[:, p] = rng.normal(0, 3, Cn) if logits else rng.uniform(0.0, 1.0, Cn)
            s[j, p] = np.nan
            if logits or Cn == 1:
                cls[p], prob[p] = -1, F32(0.0)
        elif kd == "nanall":
            s[:, p] = np.nan
            cls[p], prob[p] = -1, F32(0.0)
        elif kd == "inf":
            s[:, p] = rng.uniform(0.0, 1.0, Cn)
            s[j, p] = np.inf
            cls[p], prob[p] = j, F32(np.inf)
        elif kd == "subnormal":
            s[:, p] = (rng.permutation(Cn) + 1) * 1.4e-45
            cls[p], prob[p] = int(np.argmax(s[:, p])), F32(Cn * 1.4e-45)
        elif kd == "equal":
            s[:, p] = 1.25 if logits else 0.5
            cls[p], prob[p] = last, (None if logits else F32(0.5))
        elif kd in ("random1", "random8"):
            s[:, p] = rng.normal(0, 3, Cn) * (8.0 if kd == "random8" else 1.0)
        elif kd == "spread":
            s[:, p] = -50.0 - rng.uniform(0, 5, Cn)
            s[j, p] = 60.0
            cls[p], prob[p] = j, F32(1.0)
        elif kd == "huge":
            s[:, p] = -3e38
            s[j, p] = 3e38
            cls[p], prob[p] = j, F32(1.0)
        elif kd == "posinf":
            s[:, p] = rng.normal(0, 3, Cn)
            s[j, p] = np.inf
            cls[p], prob[p] = -1, F32(0.0)
        elif kd == "neginf1":
            s[:, p] = rng.normal(0, 3, Cn)
            s[j, p] = -np.inf
            if Cn == 1:
                cls[p], prob[p] = -1, F32(0.0)
        elif kd == "neginfall":
            s[:, p] = -np.inf
            cls[p], prob[p] = -1, F32(0.0)
    return dict(kind="unproj", sp=sp, scores=s.reshape(Cn, H, W), pixel=crafted_pixels(P, 12), logits=bool(logits),
                row_kind=kind, row_cls=cls, row_prob=prob, random=False)


# ---------------------------------------------------------------------------------------------------------------------
# KNN scenes
# ---------------------------------------------------------------------------------------------------------------------
class Crafted(Scene):
    """Scene of test_semantic_knn_host.py (on-axis points, exact ranges) with 32 classes, the label map above, pixels
    whose only non-negative score is the class's (so a prob of +-0 is the class's too) and crafted pixel / proj_idx"""

    def __init__(self, W, H):
        super().__init__(W, H, 32)
        self.sp = params(W, H, 0, n_classes=32)
        self.scores[:] = -1.0  # no class anywhere until a row says so
        self.expect = []

    def sole_class(self, v, u, cls, prob):
        p = v * self.W + u
        self.scores[:, p] = -1.0
        self.scores[cls, p] = prob

    def raw_point(self, xyz, pixel):
        self.pts.append(list(xyz) + [0.0])
        self.pixel.append(pixel)
        return len(self.pts) - 1

    def done(self, kp, logits=False, random=False):
        pts = np.array(self.pts, F32).reshape(-1, 4)
        return dict(kind="knn", sp=self.sp, kp=kp, pts=pts, scores=self.scores.reshape(self.C, self.H, self.W).copy(),
                    pixel=np.array(self.pixel, np.int64).astype(np.int32), proj_idx=self.proj_idx.copy(), logits=logits,
                    expect=list(self.expect), random=random)


def label_of(cls):
    return float(F32(LM32[cls]))


GRID_RANGES = [4.0, 4.5, 5.0, 6.0, 8.0, 12.0]
GRID_CLASSES = [-1, 0, 1, 2, 31, 31, 1, 7]


def knn_grid(a, b):
    (S, k), (W, H) = GRID[a], IMAGES[b]
    kp = semantic_knn(S, k, SIGMAS[(a + b) % 4], CUTOFFS[(a + 2 * b) % 5])
    rng = np.random.default_rng(100 * a + b)
    s = Crafted(W, H)
    for v in range(H):
        for u in range(W):
            c = GRID_CLASSES[rng.integers(0, 8)]
            if c >= 0:
                s.sole_class(v, u, c, [0.25, 0.5, 0.75, 1.0][rng.integers(0, 4)])
            if rng.integers(0, 8) == 0 and W * H > 1:
                continue  # an empty pixel: it has a class all the same
            r = GRID_RANGES[rng.integers(0, 6)]
            s.point(v, u, r)
            if rng.integers(0, 4) == 0:
                s.point(v, u, r + [0.5, 1.0, 2.0, 16.0][rng.integers(0, 4)], winner=False)
    for j, bad in enumerate([-1, I32_MIN, W * H, W * H + 1, I32_MAX]):
        i = s.raw_point([5.0 + j, 0.0, 0.0], bad)
        s.expect.append((i, 0.0, 0.0))
    return s.done(kp)


def knn_equal(S, k):
    s = Crafted(4, 9)
    for v in range(9):
        for u in range(4):
            s.sole_class(v, u, 1 + (v * 4 + u) % 5, 0.5)
            s.point(v, u, 10.0)
    s.sole_class(4, 1, 6, 0.25)
    if S >= 3 and k == 2:  # the centre and slot t = 0, the pixel up and left by R
        Rr = (S - 1) // 2
        if 4 - Rr >= 0 and 1 - Rr >= 0:
            c0 = 1 + ((4 - Rr) * 4 + (1 - Rr)) % 5
            s.expect.append((4 * 4 + 1, label_of(min(6, c0)), None))
    return s.done(semantic_knn(S, k, 1.0, 0.0))


def knn_mirror(S):
    s = Crafted(7, 1)
    for u, r, c in ((2, 9.0, 3), (3, 10.0, -1), (4, 11.0, 4)):
        if c >= 0:
            s.sole_class(0, u, c, 0.5)
        s.point(0, u, r)
    s.expect.append((1, label_of(3), 0.5))  # d ties: the lower window index, the left neighbour
    return s.done(semantic_knn(S, 2, 1.0, 0.0))


def knn_cuteq(S, k, below):
    D = 2.0
    w = R.knn_weights_fp64(S, 1.0)
    t_left = (S * S - 1) // 2 - 1
    cutoff = F32(D * w[t_left])
    assert float(cutoff) == D * w[t_left]  # a power of two times an fp32 number
    if below:
        cutoff = np.nextafter(cutoff, F32(0.0))
    s = Crafted(7, 1)
    s.sole_class(0, 2, 5, 0.5)
    s.point(0, 2, 10.0)
    i = s.point(0, 3, 8.0)
    s.expect.append((i, 0.0, 0.0) if below else (i, label_of(5), 0.5))
    return s.done(semantic_knn(S, k, 1.0, float(cutoff)))


def knn_emptyvote(S, cutoff):
    s = Crafted(3, 3)
    for v in range(3):
        for u in range(3):
            if (v, u) != (1, 1):
                s.sole_class(v, u, 2, 0.75)
    i = s.point(1, 1, 5.0)
    s.expect.append((i, label_of(2), 0.75) if cutoff <= 0 else (i, 0.0, 0.0))
    return s.done(semantic_knn(S, S * S, 1.0, cutoff))


def knn_outside(S, k):
    s = Crafted(3, 3)
    for v in range(3):
        for u in range(3):
            s.sole_class(v, u, 2 if (v, u) != (0, 0) else 6, 0.5)
            s.point(v, u, 0.5 if (v, u) == (0, 0) else 30.0)
    # the slots outside the image (range 0) are the nearest to the point at 0.5 m and have no class: with k no larger
    # than their number + 1 only the centre votes
    s.expect.append((0, label_of(6), 0.5))
    return s.done(semantic_knn(S, k, 1.0, 0.0))


def knn_all81(cls):
    s = Crafted(24, 10)
    for v in range(10):
        for u in range(24):
            s.sole_class(v, u, cls, 0.5)
            s.point(v, u, 10.0)
    s.sole_class(5, 12, cls, 0.75)
    s.expect.append((5 * 24 + 12, label_of(cls), 0.75))
    s.expect.append((4 * 24 + 4, label_of(cls), 0.5))
    return s.done(semantic_knn(9, 81, 1.0, 0.0))


def knn_tie31(S):
    s = Crafted(3, 3)
    for v in range(3):
        for u in range(3):
            if (v, u) != (1, 1):
                s.sole_class(v, u, 31 if (v * 3 + u) % 2 == 0 else 1, 0.5)
            s.point(v, u, 10.0)
    s.expect.append((4, label_of(1), 0.5))  # 31 at the four corners, 1 at the four edges: equal counts to the lower
    return s.done(semantic_knn(S, S * S, 1.0, 0.0))


def knn_negzero(S, k, plus):
    s = Crafted(7, 1)
    s.sole_class(0, 3, 6, -0.0)
    if plus:
        s.sole_class(0, 2, 6, 0.0)
    for u in range(7):
        s.point(0, u, 10.0)
    s.expect.append((3, label_of(6), 0.0 if plus else -0.0))
    return s.done(semantic_knn(S, k, 1.0, 0.0))


def knn_cutprob(S, k):
    s = Crafted(7, 1)
    for u, r, pr in ((2, 8.5, 0.5), (3, 8.0, 0.25), (4, 20.0, 1.0)):
        s.sole_class(0, u, 3, pr)
        s.point(0, u, r)
    s.expect.append((1, label_of(3), 0.5))
    return s.done(semantic_knn(S, k, 1.0, 1.0))


def knn_hidden3(S, k):
    s = Crafted(7, 5)
    for v in range(5):
        for u in range(7):
            s.sole_class(v, u, 2 if u == 3 else 1, 0.9 if u == 3 else 0.6)
            s.point(v, u, 5.0 if u == 3 else 20.0)
    h = [s.point(2, 3, r, winner=False) for r in (20.0, 12.0, 5.5)]
    if (S, k) == (5, 5):
        s.expect += [(h[0], label_of(1), 0.6), (h[2], label_of(2), 0.9)]
    return s.done(semantic_knn(S, k, 1.0, 1.0))


def knn_badproj(S, k):
    sc = knn_grid(GRID.index((S, k)), IMAGES.index((24, 10)))
    n = sc["pts"].shape[0]
    for j, bad in enumerate([-1, n, I32_MIN, I32_MAX]):
        sc["proj_idx"][17 + 29 * j] = bad
    return sc


def knn_inconsistent(S, k):
    s = Crafted(3, 3)
    for v in range(3):
        for u in range(3):
            s.sole_class(v, u, 1 + (v * 3 + u) % 5, 0.5)
            s.point(v, u, 10.0 + u)
    nan, inf = np.nan, np.inf
    for j, xyz in enumerate([[nan, 0, 0], [0, nan, 1], [inf, 0, 0], [1, -inf, 0], [0, 0, 0], [3e20, 3e20, 0], [3e38, 0, 0],
                             [1e-30, 0, 0], [-0.0, 0.0, 0.0]]):
        i = s.raw_point(xyz, (4 + j) % 9)
        s.expect.append((i, 0.0, 0.0))
    return s.done(semantic_knn(S, k, 1.0, [0.0, 1.0, 3e38][k % 3]))


def knn_random(kpt, logits):
    kp = semantic_knn(*kpt)
    rng = np.random.default_rng(kp.search * 100 + kp.k + int(logits))
    W, H, Cn, n = 24, 10, 32, 400
    sp = params(W, H, 0, n_classes=Cn)
    pts = np.zeros((n, 4), F32)
    pts[:, :3] = rng.normal(0.0, 12.0, (n, 3))
    pixel = rng.integers(0, W * H, n).astype(np.int32)
    pixel[rng.choice(n, 20, replace=False)] = -1
    proj_idx = np.full(W * H, -1, np.int32)
    r = np.sqrt((pts[:, :3].astype(np.float64) ** 2).sum(1))
    for i in np.argsort(-r, kind="stable"):
        if pixel[i] >= 0:
            proj_idx[pixel[i]] = i
    if logits:
        scores = (rng.normal(0.0, 3.0, (Cn, H * W)) * 2.0).astype(F32)
    else:
        scores = rng.uniform(-0.3, 1.0, (Cn, H * W)).astype(F32)
        scores[:, rng.choice(W * H, 15, replace=False)] = -0.5
        scores[0, rng.choice(W * H, 30, replace=False)] = 2.0
    return dict(kind="knn", sp=sp, kp=kp, pts=pts, scores=scores.reshape(Cn, H, W), pixel=pixel, proj_idx=proj_idx,
                logits=bool(logits), expect=[], random=True)


# ---------------------------------------------------------------------------------------------------------------------
# the registry
# ---------------------------------------------------------------------------------------------------------------------
BUILDERS = {}
for _g, (_W, _H) in enumerate(GEOS):
    for _f in range(4):
        BUILDERS[f"centres-{_W}x{_H}-f{_f}"] = functools.partial(proj_centres, _W, _H, _f)
        BUILDERS[f"straddle-{_W}x{_H}-f{_f}"] = functools.partial(proj_straddle, _W, _H, _f)
for _W, _H in ((1, 1), (33, 5), (130, 4), (64, 16)):
    BUILDERS[f"zfight-{_W}x{_H}"] = functools.partial(proj_zfight, _W, _H)
BUILDERS["specials-64x16"] = proj_specials
for _n, _geo, _f in RANDOM:
    BUILDERS[f"random-{_geo[0]}x{_geo[1]}-n{_n}"] = functools.partial(proj_random, _n, _geo, _f)
PROJ_IDS = list(BUILDERS)
SEQUENCES = {"same-size": ["random-64x16-n1000", "random-64x16-n0", "random-64x16-n1", "random-64x16-n1000"],
             "sizes": ["centres-64x16-f0", "centres-7x1-f0", "centres-64x16-f1", "centres-257x3-f0"]}

_n0 = len(BUILDERS)
for _c in CLASSES:
    for _big in (1, 0):
        for _lg in (0, 1):
            BUILDERS[f"unproj-C{_c}-P{520 if _big else 5}-{'logits' if _lg else 'probs'}"] = \
                functools.partial(unproj_scene, _c, _big, _lg)
UNPROJ_IDS = list(BUILDERS)[_n0:]

_n0 = len(BUILDERS)
for _a, (_S, _k) in enumerate(GRID):
    for _b, (_W, _H) in enumerate(IMAGES):
        BUILDERS[f"grid-S{_S}k{_k}-{_W}x{_H}"] = functools.partial(knn_grid, _a, _b)
for _S, _k in ((3, 2), (3, 8), (5, 5), (5, 4), (5, 6), (7, 2), (7, 25), (9, 2), (9, 80), (9, 81)):
    BUILDERS[f"equal-S{_S}k{_k}"] = functools.partial(knn_equal, _S, _k)
for _S in (3, 5, 7, 9):
    BUILDERS[f"mirror-S{_S}"] = functools.partial(knn_mirror, _S)
    BUILDERS[f"tie31-S{_S}"] = functools.partial(knn_tie31, _S)
    for _co in (-5.0, 0.0, 0.5, 3e38):
        BUILDERS[f"emptyvote-S{_S}-c{_co:g}"] = functools.partial(knn_emptyvote, _S, _co)
for _S, _k in PATHS_FULL:
    BUILDERS[f"cuteq-S{_S}k{_k}-at"] = functools.partial(knn_cuteq, _S, _k, False)
    BUILDERS[f"cuteq-S{_S}k{_k}-below"] = functools.partial(knn_cuteq, _S, _k, True)
    BUILDERS[f"negzero-S{_S}k{_k}-sole"] = functools.partial(knn_negzero, _S, _k, False)
    BUILDERS[f"negzero-S{_S}k{_k}-plus"] = functools.partial(knn_negzero, _S, _k, True)
    BUILDERS[f"cutprob-S{_S}k{_k}"] = functools.partial(knn_cutprob, _S, _k)
    BUILDERS[f"hidden3-S{_S}k{_k}"] = functools.partial(knn_hidden3, _S, _k)
    BUILDERS[f"inconsistent-S{_S}k{_k}"] = functools.partial(knn_inconsistent, _S, _k)
for _S, _k in ((1, 1), (3, 1), (5, 4), (7, 2), (9, 16)):
    BUILDERS[f"inconsistent-S{_S}k{_k}"] = functools.partial(knn_inconsistent, _S, _k)
for _S, _k in ((5, 5), (5, 6), (9, 16), (7, 25)):
    BUILDERS[f"outside-S{_S}k{_k}"] = functools.partial(knn_outside, _S, _k)
for _S, _k in ((3, 9), (5, 5), (9, 81)):
    BUILDERS[f"badproj-S{_S}k{_k}"] = functools.partial(knn_badproj, _S, _k)
BUILDERS["all81-c31"] = functools.partial(knn_all81, 31)
BUILDERS["all81-c1"] = functools.partial(knn_all81, 1)
for _kpt in ((5, 5, 1.0, 1.0), (9, 16, 2.0, 0.5), (7, 49, 1.5, 3.0), (3, 2, 0.5, 0.0)):
    for _lg in (0, 1):
        BUILDERS[f"knnrandom-S{_kpt[0]}k{_kpt[1]}-{'logits' if _lg else 'probs'}"] = \
            functools.partial(knn_random, _kpt, _lg)
KNN_IDS = list(BUILDERS)[_n0:]


@functools.lru_cache(maxsize=None)
def get_scene(sid):
    sc = BUILDERS[sid]()
    sc["id"] = sid
    return sc


def _scene(sc):
    return get_scene(sc) if isinstance(sc, str) else sc


def followup_scenes(sid, pixel, proj_idx):
    """what the GPU file back-projects after projecting a scene: plain and KNN, probabilities and logits, on the pixel /
    proj_idx the projection gave"""
    sc = get_scene(sid)
    sp = params(sc["sp"].width, sc["sp"].height, FOVS.index((sc["sp"].fov_up, sc["sp"].fov_down)), n_classes=20)
    P = sp.width * sp.height
    rng = np.random.default_rng(len(sid) + P)
    out = []
    for logits in (False, True):
        s = rng.normal(0, 6, (20, P)).astype(F32) if logits else rng.uniform(-0.2, 1.0, (20, P)).astype(F32)
        s = s.reshape(20, sp.height, sp.width)
        out.append(dict(kind="unproj", id=sid + "+unproject", sp=sp, scores=s, pixel=np.asarray(pixel, np.int32),
                        logits=logits, row_kind=None, random=None))
        out.append(dict(kind="knn", id=sid + "+knn", sp=sp, kp=semantic_knn(), pts=sc["pts"], scores=s,
                        pixel=np.asarray(pixel, np.int32), proj_idx=np.asarray(proj_idx, np.int32).ravel(),
                        logits=logits, expect=[], random=None))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the shims' results and the checks
# ---------------------------------------------------------------------------------------------------------------------
def run_shim(sc, libs=None):
    sc = _scene(sc)
    plain, knn = libs or shims()
    if sc["kind"] == "proj":
        return shim_project(plain, sc["sp"], sc["pts"])
    if sc["kind"] == "unproj":
        return shim_unproject(plain, sc["sp"], sc["scores"], sc["pixel"], logits=sc["logits"])
    return knn_unproject(knn, sc["sp"], sc["kp"], sc["pts"], sc["scores"], sc["pixel"], sc["proj_idx"],
                         logits=sc["logits"])[:2]


@functools.lru_cache(maxsize=None)
def shim_results(sid):
    return run_shim(sid)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def assert_same_bits(got, want, what):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: differs from the host restatement"


@functools.lru_cache(maxsize=None)
def _proj_ref(sid):
    sc = get_scene(sid)
    return R.project_fp64(sc["sp"], sc["pts"])


def _cap(sc, und, total, what):
    if total == 0 or sc["random"] is None:  # a follow-up scene: no cap of its own, fp64 holds what it decides
        return
    if sc["random"]:
        assert und <= CAP * total, f"{sc['id']}: {und} of {total} {what} undecided (cap {CAP:.0%})"
    else:
        assert und == 0, f"{sc['id']}: {und} {what} undecided in a constructed row"


def check_projection(sc, got, who="shim"):
    """got = (input [5, H, W], pixel [n], proj_idx [H, W]) -> (undecided points, undecided pixels)"""
    sc = _scene(sc)
    sid, sp = sc["id"], sc["sp"]
    W, H = sp.width, sp.height
    P, n = W * H, sc["pts"].shape[0]
    inp = np.asarray(got[0], F32).reshape(5, P)
    pixel = np.asarray(got[1], np.int64).reshape(n)
    proj = np.asarray(got[2], np.int64).reshape(P)
    ref = _proj_ref(sid) if isinstance(sid, str) and sid in BUILDERS else R.project_fp64(sp, sc["pts"])
    tag = f"{who} {sid}"
    # whatever fp64 decides
    assert ((pixel >= -1) & (pixel < P)).all(), tag
    filled = proj >= 0
    assert (proj[filled] < n).all() and (proj[~filled] == -1).all(), tag
    assert (pixel[proj[filled]] == np.nonzero(filled)[0]).all(), f"{tag}: proj_idx and pixel do not name each other"
    assert set(np.unique(pixel[pixel >= 0])) == set(np.nonzero(filled)[0]), f"{tag}: a pixel with points has no winner"
    assert (bits(inp[:, ~filled]) == 0).all(), f"{tag}: an empty pixel is not +0 in every plane"
    # the decided
    dp = ref["pt_decided"]
    bad = np.nonzero(dp & (pixel != ref["pixel"]))[0]
    assert bad.size == 0, f"{tag}: point {bad[:5]} in pixel {pixel[bad[:5]]}, fp64 says {ref['pixel'][bad[:5]]} " \
                          f"(margins {ref['m_u'][bad[:5]]}, {ref['m_v'][bad[:5]]})"
    dx = ref["px_decided"]
    bad = np.nonzero(dx & (proj != ref["winner"]))[0]
    assert bad.size == 0, f"{tag}: pixel {bad[:5]} won by {proj[bad[:5]]}, fp64 says {ref['winner'][bad[:5]]}"
    dev = np.abs(inp.astype(np.float64) - ref["planes"])
    over = dx[None] & ~(dev <= ref["tol"])
    assert not over.any(), f"{tag}: plane value off by {dev[over].max():.3g} (tolerance {ref['tol'][over].min():.3g})"
    # the row's own statement
    ex = sc["expect"]
    bad = np.nonzero((ex > -2) & (pixel != ex))[0]
    assert bad.size == 0, f"{tag}: point {bad[:5]} in pixel {pixel[bad[:5]]}, made for {ex[bad[:5]]}"
    for p, i in sc["winners"].items():
        assert proj[p] == i, f"{tag}: pixel {p} won by {proj[p]}, the row says {i}"
        want = (F32(sc["pts"][i, 3]) - F32(sp.means[4])) * F32(1.0 / float(sp.stds[4]))
        assert inp[4, p] == want, f"{tag}: pixel {p} does not carry its winner's remission"
    for i in sc.get("projected", []):
        assert pixel[i] >= 0, f"{tag}: point {i} {sc['pts'][i]} is not projected"
    und_pt, und_px = int((~dp).sum()), int((~dx).sum())
    _cap(sc, und_pt, n, "points")
    _cap(sc, und_px, P, "pixels")
    return und_pt, und_px


def check_unproject(sc, got, who="shim"):
    """got = (labels, probs) -> undecided points"""
    sc = _scene(sc)
    sp, pixel = sc["sp"], np.asarray(sc["pixel"], np.int64)
    labels, probs = np.asarray(got[0], F32), np.asarray(got[1], F32)
    tag = f"{who} {sc['id']}"
    label, prob, tol, dec = R.unproject_fp64(sp, sc["scores"], pixel, sc["logits"])
    P = sp.width * sp.height
    out = (pixel < 0) | (pixel >= P)
    assert (bits(labels[out]) == 0).all() and (bits(probs[out]) == 0).all(), f"{tag}: a point without a pixel is not (0, 0)"
    bad = np.nonzero(dec & (labels.astype(np.float64) != label))[0]
    assert bad.size == 0, f"{tag}: point {bad[:5]} labelled {labels[bad[:5]]}, fp64 says {label[bad[:5]]}"
    if sc["logits"]:
        dev = np.abs(probs.astype(np.float64) - prob)
        over = dec & ~(dev <= tol)
        assert not over.any(), f"{tag}: prob off by {dev[over].max():.3g} (tolerance {tol[over].min():.3g})"
    else:
        bad = np.nonzero(dec & (bits(probs) != bits(prob.astype(F32))))[0]
        assert bad.size == 0, f"{tag}: point {bad[:5]} prob {probs[bad[:5]]}, fp64 says {prob[bad[:5]]} (signs count)"
    if sc["row_kind"] is not None:
        lab = np.array([0.0] + [float(F32(int(sp.label_map[j]))) for j in range(sp.n_classes)])
        for i in np.nonzero(~out)[0]:
            p = pixel[i]
            if sc["row_cls"][p] > -2:
                assert labels[i] == lab[sc["row_cls"][p] + 1], f"{tag}: {sc['row_kind'][p]} pixel {p} labelled {labels[i]}"
            if sc["row_prob"][p] is not None:
                assert bits(probs[i]) == bits(sc["row_prob"][p]), f"{tag}: {sc['row_kind'][p]} pixel {p} prob {probs[i]!r}"
            elif sc["row_kind"][p] == "equal":
                assert abs(float(probs[i]) - 1.0 / sp.n_classes) <= 4 * R.U, f"{tag}: equal logits give {probs[i]!r}"
    und = int((~dec).sum())
    _cap(sc, und, pixel.size, "points")
    return und


def check_knn(sc, got, who="shim"):
    """got = (labels, probs) -> undecided points"""
    sc = _scene(sc)
    labels, probs = np.asarray(got[0], F32), np.asarray(got[1], F32)
    tag = f"{who} {sc['id']}"
    ref = R.knn_fp64(sc["sp"], sc["kp"], sc["pts"], sc["scores"], sc["pixel"], sc["proj_idx"], sc["logits"])
    pixel = np.asarray(sc["pixel"], np.int64)
    out = (pixel < 0) | (pixel >= sc["sp"].width * sc["sp"].height) | ref["own_bad"]
    assert (bits(labels[out]) == 0).all() and (bits(probs[out]) == 0).all(), f"{tag}: a point without a pixel or a range is not (0, 0)"
    dec = ref["decided"]
    bad = np.nonzero(dec & (labels.astype(np.float64) != ref["label"]))[0]
    assert bad.size == 0, f"{tag}: point {bad[:5]} labelled {labels[bad[:5]]}, fp64 says {ref['label'][bad[:5]]} " \
                          f"(sel {ref['sel'][bad[:5]]}, cut {ref['cut'][bad[:5]]})"
    if sc["logits"]:
        dev = np.abs(probs.astype(np.float64) - ref["prob"])
        over = dec & ~(dev <= ref["tol"])
        assert not over.any(), f"{tag}: prob off by {dev[over].max():.3g} (tolerance {ref['tol'][over].min():.3g})"
    else:
        bad = np.nonzero(dec & (bits(probs) != bits(ref["prob"].astype(F32))))[0]
        assert bad.size == 0, f"{tag}: point {bad[:5]} prob {probs[bad[:5]]}, fp64 says {ref['prob'][bad[:5]]}: not the " \
                              f"winner's best voter (signs count)"
    for i, lab, pr in sc["expect"]:
        assert labels[i] == lab, f"{tag}: point {i} labelled {labels[i]}, the row says {lab}"
        if pr is not None:
            assert bits(probs[i]) == bits(F32(pr)), f"{tag}: point {i} prob {probs[i]!r}, the row says {pr!r}"
    und = int((~dec).sum())
    _cap(sc, und, pixel.size, "points")
    return und


CHECKS = dict(proj=check_projection, unproj=check_unproject, knn=check_knn)


# ---------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", PROJ_IDS)
def test_projection_scene(sid):
    got = shim_results(sid)
    und = check_projection(sid, got)
    print(f"{sid}: undecided points {und[0]}, pixels {und[1]}")
    for f in followup_scenes(sid, got[1], got[2]):
        CHECKS[f["kind"]](f, run_shim(f))


@pytest.mark.parametrize("sid", UNPROJ_IDS)
def test_backprojection_scene(sid):
    print(f"{sid}: undecided {check_unproject(sid, shim_results(sid))}")


@pytest.mark.parametrize("sid", KNN_IDS)
def test_knn_scene(sid):
    print(f"{sid}: undecided {check_knn(sid, shim_results(sid))}")


def test_every_parameter_is_covered():
    seen = [get_scene(s)["kp"] for s in KNN_IDS]
    assert {(k.search, k.k) for k in seen} >= set(GRID)
    assert {float(F32(k.sigma)) for k in seen} >= {float(F32(s)) for s in SIGMAS}
    assert {float(F32(k.cutoff)) for k in seen} >= {float(F32(c)) for c in CUTOFFS}
    assert max(get_scene(s)["pts"].shape[0] for s in PROJ_IDS + KNN_IDS) <= 1040  # a point per pixel at the most
    assert max(get_scene(s)["sp"].width * get_scene(s)["sp"].height for s in BUILDERS) <= 1040
    assert {get_scene(s)["pts"].shape[0] for s in PROJ_IDS} >= {0, 1, 63, 64, 65, 255, 256, 257, 1000}


def test_weight_table_of_the_statement_is_the_shims():
    for S in (1, 3, 5, 7, 9):
        for sigma in SIGMAS + [1.5, 2.0]:
            w = np.empty(S * S, F32)
            shims()[1].knn_weights(C.c_uint32(S), C.c_float(sigma), w.ctypes.data_as(C.c_void_p))
            assert w.tobytes() == R.knn_weights_fp64(S, sigma).astype(F32).tobytes(), (S, sigma)


def test_rows_exercise_what_they_claim():
    """the margins that make a row worth running: ties, d = cutoff and one-step gaps really occur"""
    z = _proj_ref("zfight-33x5")
    assert z["px_decided"].all() and len(get_scene("zfight-33x5")["winners"]) >= 20
    x = get_scene("zfight-33x5")["pts"][[300, 450, 600, 750], 0]
    assert (np.diff(x.view(np.uint32).astype(np.int64)) == -1).all()  # one fp32 step apart, the nearest last
    sc = get_scene("cuteq-S5k5-at")
    ref = R.knn_fp64(sc["sp"], sc["kp"], sc["pts"], sc["scores"], sc["pixel"], sc["proj_idx"], False)
    assert ref["cut"][1] == 0.0 and ref["decided"][1]
    sc = get_scene("mirror-S3")
    ref = R.knn_fp64(sc["sp"], sc["kp"], sc["pts"], sc["scores"], sc["pixel"], sc["proj_idx"], False)
    assert ref["sel"][1] == 0.0 and ref["decided"][1]
    und = sum(int((~_proj_ref(s)["pt_decided"]).sum()) for s in PROJ_IDS if s.startswith("random"))
    print("undecided points over the random projection scenes:", und)


def _ratio(margin, bound):
    with np.errstate(all="ignore"):
        return np.where(bound > 0, margin / bound, 0.0)


def measure_bounds(libs=None):
    """-> {kind: the largest margin / derived bound at which the shim and fp64 decide differently}"""
    plain, knn = libs or shims()
    worst = dict(texel=0.0, gap=0.0, top2=0.0, sel=0.0, cut=0.0)
    # points across column and row boundaries in steps of a tenth of the bound
    for (W, H, fov) in ((64, 16, 0), (257, 3, 1), (130, 4, 3), (33, 5, 0)):
        sp = params(W, H, fov)
        e_u, e_v = 6.0 * W * R.U, 40.0 * H * R.U
        k = np.arange(-40, 41) * 0.1
        pts = []
        for b in sorted({1, W // 3, W // 2, W - 1}):
            for r in (3.0, 7.7, 41.0):
                pts += [point_at(sp, 0.4 * H, b + kk * e_u, r) for kk in k]
        for b in sorted({1, H // 2, H - 1}):
            for r in (3.0, 7.7, 41.0):
                pts += [point_at(sp, b + kk * e_v, 0.37 * W, r) for kk in k]
        pts = np.array(pts, F32)
        ref = R.project_fp64(sp, pts)
        _, pixel, _ = shim_project(plain, sp, pts)
        diff = pixel != ref["pixel"]
        assert not (diff & ref["pt_decided"]).any()
        m = np.minimum(_ratio(ref["m_u"], ref["e_u"]), _ratio(ref["m_v"], ref["e_v"]))
        if diff.any():
            worst["texel"] = max(worst["texel"], float(m[diff].max()))
    # range pairs across a tie, in one direction
    sp = params(64, 16, 0)
    rng = np.random.default_rng(5)
    for _ in range(200):
        base = np.array(point_at(sp, rng.uniform(2, 14), rng.uniform(2, 62), rng.uniform(2, 60)), F32)
        pts = []
        for j in range(-6, 7):
            q = base.copy()
            q[:3] = (base[:3].astype(np.float64) * (1.0 + j * 2.0 ** -23)).astype(F32)
            pts.append(q)
        pts = np.array(pts, F32)
        rr, err, _, _ = R.ranges_fp64(pts)
        for j in range(len(pts)):
            pair = np.array([pts[6], pts[j]], F32)  # the base first: it keeps an exact tie
            ref = R.project_fp64(sp, pair)
            _, pixel, proj = shim_project(plain, sp, pair)
            if pixel[0] != pixel[1] or ref["pixel"][0] != ref["pixel"][1]:
                continue
            want = 0 if rr[6] <= rr[j] else 1
            if proj.ravel()[pixel[0]] != want and err[6] + err[j] > 0:
                worst["gap"] = max(worst["gap"], abs(rr[6] - rr[j]) / (err[6] + err[j]))
    # logit pairs across a tie
    sp2 = params(64, 16, 0, n_classes=2)
    base = rng.normal(0, 4, 1024).astype(F32)
    for j in range(0, 17):
        other = (base.astype(np.float64) - j * 2.0 ** -24 * np.maximum(1.0, np.abs(base))).astype(F32)
        for order in (0, 1):
            s = np.stack([base, other][::1 if order == 0 else -1]).reshape(2, 16, 64)
            lab, _ = shim_unproject(plain, sp2, s, np.arange(1024, dtype=np.int32), logits=True)
            label, _, _, _ = R.unproject_fp64(sp2, s, np.arange(1024), True)
            gap = np.abs(base.astype(np.float64) - other)
            diff = lab != label
            if diff.any():
                worst["top2"] = max(worst["top2"], float((gap[diff] / R.TOP2_BOUND).max()))
    # d across the cutoff and across a tie between two neighbours: generic (off-axis) points on a 3 x 1 image
    sp3 = params(3, 1, 0, n_classes=32)
    scores = np.full((32, 1, 3), -1.0, F32)
    scores[3, 0, 0], scores[5, 0, 2] = 0.5, 0.75
    only_right = scores.copy()
    only_right[3, 0, 0] = -1.0
    for trial in range(60):
        ri = rng.uniform(3, 40)
        dl = rng.uniform(0.2, 3.0)
        for j in range(-8, 9):
            dr = dl * (1.0 + j * 0.25 * ri / dl * 2.0 ** -23)
            pts = np.array([point_at(sp3, 0.5, 0.5, ri + dl), point_at(sp3, 0.5, 1.5, ri), point_at(sp3, 0.5, 2.5, ri - dr)],
                           F32)
            pixel, proj = np.array([0, 1, 2], np.int32), np.array([0, 1, 2], np.int32)
            w = R.knn_weights_fp64(3, 1.0)
            rr = R.ranges_fp64(pts)[0]
            for kind, kp, sc_ in (("sel", semantic_knn(3, 2, 1.0, 0.0), scores),
                                  ("cut", semantic_knn(3, 9, 1.0, float(F32(abs(rr[2] - rr[1]) * w[5]))), only_right)):
                lab = knn_unproject(knn, sp3, kp, pts, sc_, pixel, proj)[0]
                ref = R.knn_fp64(sp3, kp, pts, sc_, pixel, proj, False)
                if lab[1] != ref["label"][1]:
                    assert not ref["decided"][1]
                    worst[kind] = max(worst[kind], float(ref[kind][1] / ref[kind + "_err"][1]))
    return worst


def test_measured_bounds():
    """the shim never leaves fp64 on a decided point, and the largest margin at which it does at all is inside the
    recorded figure (semantic_ref.MEASURED), itself below 0.5: the derived bounds stand"""
    worst = measure_bounds()
    print("measured margin / bound at a disagreement:", worst)
    for kind, v in worst.items():
        assert v <= R.MEASURED[kind] < 0.5, (kind, v)
