"""RangeNet++'s KNN post-processing on the host: known answers of its arithmetic specification as restated in
tests/semantic_knn_shim.c (which the GPU tests compare the kernels of csrc/k_semantic_knn.hip with, bit for bit), an
independent vectorised numpy restatement, the layout of suma_semantic_knn in C and ctypes, and parameter validation."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from semantic_suma_amd.segmentation import semantic_knn
from semantic_suma_amd.types import SemanticKnnParams
from test_semantic_host import build_shim as build_plain_shim
from test_semantic_host import make_params
from test_semantic_host import unproject as plain_unproject

HERE = os.path.dirname(os.path.abspath(__file__))


def build_knn_shim(out_dir):
    so = os.path.join(str(out_dir), "semantic_knn_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "semantic_knn_shim.c"), "-o", so, "-lm"])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_knn_shim(tmp_path_factory.mktemp("semantic_knn"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build_plain_shim(tmp_path_factory.mktemp("semantic_knn_plain"))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def knn_unproject(shim, sp, kp, pts, scores, pixel, proj_idx, logits=False):
    """-> labels, probs (n), and the pixel records range, cls, prob (P)"""
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    pixel = np.ascontiguousarray(pixel, dtype=np.int32)
    proj_idx = np.ascontiguousarray(proj_idx, dtype=np.int32)
    n, P = pixel.size, sp.width * sp.height
    labels, probs = np.empty(n, np.float32), np.empty(n, np.float32)
    rng, cls, prob = np.empty(P, np.float32), np.empty(P, np.int32), np.empty(P, np.float32)
    shim.sem_unproject_knn(C.byref(sp), C.byref(kp), vp(pts), vp(scores), C.c_int(int(logits)), vp(pixel), vp(proj_idx),
                           C.c_uint32(n), vp(labels), vp(probs), vp(rng), vp(cls), vp(prob))
    return labels, probs, rng, cls, prob


def weights(shim, S, sigma):
    w = np.empty(S * S, np.float32)
    shim.knn_weights(C.c_uint32(S), C.c_float(sigma), vp(w))
    return w.reshape(S, S)


LM = [0, 10, 20, 30, 40, 50]  # class index -> label


class Scene:
    """a W x H image built pixel by pixel: every pixel gets a winner at a given range (or stays empty) and one-hot
    scores of a given class (-1: all negative, no class wins)"""

    def __init__(self, W, H, C_=6):
        self.W, self.H, self.C = W, H, C_
        self.pts, self.pixel = [], []
        self.proj_idx = np.full(W * H, -1, np.int32)
        self.scores = np.zeros((C_, H * W), np.float32)
        self.sp = make_params(width=W, height=H, n_classes=C_, label_map=LM[:C_])

    def pixel_class(self, v, u, cls, prob=1.0):
        p = v * self.W + u
        self.scores[:, p] = -1.0 if cls < 0 else 0.0
        if cls >= 0:
            self.scores[cls, p] = prob

    def point(self, v, u, r, winner=True):
        i = len(self.pts)
        self.pts.append([r, 0.0, 0.0, 0.0])
        self.pixel.append(v * self.W + u)
        if winner:
            self.proj_idx[v * self.W + u] = i
        return i

    def run(self, shim, kp):
        return knn_unproject(shim, self.sp, kp, np.array(self.pts, np.float32), self.scores.reshape(self.C, self.H, self.W),
                             np.array(self.pixel, np.int32), self.proj_idx)


def test_weight_table_sigma_one_search_five(shim):
    w = weights(shim, 5, 1.0)
    g = [[math.exp(-(dx * dx + dy * dy) / 2.0) for dx in range(-2, 3)] for dy in range(-2, 3)]
    total = sum(sum(row) for row in g)  # row-major: t order
    assert total == pytest.approx((1 + 2 * math.exp(-0.5) + 2 * math.exp(-2.0)) ** 2, rel=1e-14)
    expect = np.array([[np.float32(1.0 - e / total) for e in row] for row in g], np.float32)
    assert w.tobytes() == expect.tobytes()
    assert w[2, 2] == np.float32(1.0 - 1.0 / total) and abs(w[2, 2] - 0.837898) < 1e-5
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1])
    assert w[2, 2] < w[2, 3] < w[3, 3] < w[2, 4] < w[4, 4] < 1.0  # the centre counts the most
    assert weights(shim, 1, 0.3)[0, 0] == 0.0


def test_centre_comes_first_and_k_one_is_the_plain_path(shim, plain):
    rng = np.random.default_rng(0)
    W, H = 12, 5
    s = Scene(W, H)
    for v in range(H):
        for u in range(W):
            s.pixel_class(v, u, int(rng.integers(-1, 6)), float(rng.uniform(0.1, 1.0)))
            s.point(v, u, float(rng.integers(2, 40)))
            s.point(v, u, float(rng.integers(41, 60)), winner=False)  # hidden behind the first
    plain_l, plain_p = plain_unproject(plain, s.sp, s.scores.reshape(6, H, W), np.array(s.pixel, np.int32))
    for kp in (semantic_knn(search=1, k=1), semantic_knn(k=1), semantic_knn(search=9, k=1, sigma=3.0, cutoff=0.0)):
        labels, probs, _, cls, _ = s.run(shim, kp)
        keep = cls[np.array(s.pixel)] >= 1
        assert keep.sum() > 50 and (~keep).sum() > 10
        assert np.array_equal(labels[keep], plain_l[keep]) and np.array_equal(probs[keep], plain_p[keep])
        assert (labels[~keep] == 0).all() and (probs[~keep] == 0).all()  # class 0 and none do not vote


def test_hidden_point_takes_the_background_class(shim):
    """a pole (class 2) at 5 m in front of a wall (class 1) at 20 m: the wall point in the pole's pixel is voted wall"""
    s = Scene(7, 5)
    for v in range(5):
        for u in range(7):
            s.pixel_class(v, u, 2 if u == 3 else 1, 0.9 if u == 3 else 0.6)
            s.point(v, u, 5.0 if u == 3 else 20.0)
    hidden = s.point(2, 3, 20.0, winner=False)
    labels, probs, _, _, _ = s.run(shim, semantic_knn())
    assert labels[hidden] == 10.0 and probs[hidden] == np.float32(0.6)
    pole = 2 * 7 + 3
    assert labels[pole] == 20.0 and probs[pole] == np.float32(0.9)  # the pole keeps its own class
    assert (labels[[v * 7 + u for v in range(5) for u in range(7) if u != 3]] == 10.0).all()


def test_ties_go_to_the_lower_window_index(shim):
    s = Scene(3, 3)
    for v in range(3):
        for u in range(3):
            s.pixel_class(v, u, 1 + (v * 3 + u) % 5)
            s.point(v, u, 10.0)
    s.pixel_class(1, 1, -1)  # the centre has no class: only the neighbours vote
    # all eight neighbours are at d = 0: k = 2 takes t = 0 (class 1), k = 3 adds t = 1 (class 2) -> equal counts
    # go to the lower class, k = 4 adds t = 2 (class 3)
    for k, label in ((2, 10.0), (3, 10.0), (4, 10.0)):
        labels, _, _, _, _ = s.run(shim, semantic_knn(search=3, k=k))
        assert labels[4] == label
    s.pixel_class(0, 0, 4)  # t = 0 now votes class 4; k = 3: classes 4 and 2 one each -> 2
    labels, _, _, _, _ = s.run(shim, semantic_knn(search=3, k=3))
    assert labels[4] == 20.0
    s.pixel_class(0, 2, 4)  # k = 4: class 4 twice (t = 0, 2), class 2 once
    labels, _, _, _, _ = s.run(shim, semantic_knn(search=3, k=4))
    assert labels[4] == 40.0


def test_cutoff(shim):
    s = Scene(3, 3)
    for v in range(3):
        for u in range(3):
            s.pixel_class(v, u, 3)
            s.point(v, u, 12.0)
    s.pixel_class(1, 1, -1)
    s.pts[4][0] = 10.0  # the centre point: every neighbour 2 m away, d = 2 w[t] > 1
    labels, probs, _, _, _ = s.run(shim, semantic_knn(search=3, k=9, cutoff=1.0))
    assert labels[4] == 0.0 and probs[4] == 0.0
    for cutoff in (0.0, -1.0, 2.0):
        labels, probs, _, _, _ = s.run(shim, semantic_knn(search=3, k=9, cutoff=cutoff))
        assert labels[4] == 30.0 and probs[4] == 1.0


def test_class_zero_and_none_do_not_vote_and_no_vote_gives_zero(shim):
    s = Scene(5, 5)
    for v in range(5):
        for u in range(5):
            s.pixel_class(v, u, 0 if (v + u) % 2 else -1)
            s.point(v, u, 7.0)
    labels, probs, _, cls, _ = s.run(shim, semantic_knn(search=5, k=25, cutoff=0.0))
    assert set(cls.tolist()) == {0, -1}
    assert (labels == 0).all() and (probs == 0).all()  # not class 1 as the published argmax over zeros
    s.pixel_class(4, 4, 5, 0.25)  # one voter anywhere in the window decides
    labels, probs, _, _, _ = s.run(shim, semantic_knn(search=5, k=25, cutoff=0.0))
    assert labels[12] == 50.0 and probs[12] == 0.25


def test_image_borders_do_not_wrap(shim):
    W, H = 8, 3
    s = Scene(W, H)
    for v in range(H):
        for u in range(W):
            s.pixel_class(v, u, 4 if u == W - 1 else -1)
            s.point(v, u, 6.0)
    labels, _, _, _, _ = s.run(shim, semantic_knn(search=3, k=9, cutoff=0.0))
    assert (labels[[v * W for v in range(H)]] == 0).all()  # column 0 does not see column W - 1
    assert (labels[[v * W + W - 2 for v in range(H)]] == 40).all()
    # outside the image the range is 0: a point at 0.5 m finds those slots nearest, but they have no class
    s2 = Scene(3, 3)
    for v in range(3):
        for u in range(3):
            s2.pixel_class(v, u, 2)
            s2.point(v, u, 0.5 if (v, u) == (0, 0) else 30.0)
    labels, _, _, _, _ = s2.run(shim, semantic_knn(search=5, k=6, cutoff=0.0))
    assert labels[0] == 20.0  # the centre's own vote; the five out-of-image slots before it do not vote


def numpy_knn(sp, kp, pts, scores, pixel, proj_idx):
    """rules 1 - 8 vectorised over the points (probability scores, no softmax)"""
    W, H, Cn = sp.width, sp.height, sp.n_classes
    S, K, R = kp.search, kp.k, (kp.search - 1) // 2
    tc = (S * S - 1) // 2
    r_pt = np.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2]).astype(np.float32)
    rng = np.where(proj_idx >= 0, r_pt[np.maximum(proj_idx, 0)], np.float32(np.inf)).astype(np.float32)
    sc = scores.reshape(Cn, -1)
    best = np.maximum(sc.max(0), 0.0).astype(np.float32)
    last = Cn - 1 - np.argmax((sc == best)[::-1], axis=0)  # the last maximum
    cls = np.where((sc >= 0).any(0) & ~np.isnan(best), last, -1)
    prob = np.where(cls >= 0, best, 0.0).astype(np.float32)
    dy, dx = np.divmod(np.arange(S * S), S)
    dy, dx = dy - R, dx - R
    e = np.exp(-(dx * dx + dy * dy) / (2.0 * float(np.float32(kp.sigma)) ** 2))
    total = 0.0
    for x in e:
        total += x
    w = (1.0 - e / total).astype(np.float32)
    ok = (pixel >= 0) & (r_pt > 0) & (r_pt <= np.finfo(np.float32).max)  # rule 3: the point's own range in (0, FLT_MAX]
    v, u = np.divmod(pixel[ok], W)
    yy, xx = v[:, None] + dy[None], u[:, None] + dx[None]
    inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    q = np.where(inside, yy * W + xx, 0)
    rt = np.where(inside, rng[q], np.float32(0.0)).astype(np.float32)
    ct = np.where(inside, cls[q], -1)
    pt = np.where(inside, prob[q], np.float32(0.0))
    ri = r_pt[ok][:, None]
    d = (np.abs(rt - ri) * w[None]).astype(np.float32)
    d[:, tc] = 0.0
    t = np.broadcast_to(np.arange(S * S), d.shape)
    order = np.lexsort((t, t != tc, d), axis=-1)[:, :K]
    d_s, c_s, p_s = (np.take_along_axis(a, order, 1) for a in (d, ct, pt))
    votes = (c_s >= 1) & ((kp.cutoff <= 0) | (d_s <= np.float32(kp.cutoff)))
    counts = np.stack([(votes & (c_s == j)).sum(1) for j in range(Cn)], 1)
    win = counts.argmax(1)
    any_vote = counts.max(1) > 0
    p_win = np.where(votes & (c_s == win[:, None]), p_s, -1.0).max(1)
    lm = np.array([sp.label_map[j] for j in range(Cn)], np.float32)
    labels, probs = np.zeros(pixel.size, np.float32), np.zeros(pixel.size, np.float32)
    labels[ok] = np.where(any_vote, lm[win], 0.0)
    probs[ok] = np.where(any_vote, p_win, 0.0)
    return labels, probs


@pytest.mark.parametrize("kp", [(5, 5, 1.0, 1.0), (3, 2, 0.5, 0.0), (9, 16, 2.0, 0.5), (7, 49, 1.5, 3.0)],
                         ids=["default", "3x3k2", "9x9k16", "7x7all"])
def test_shim_agrees_with_numpy(shim, kp):
    kp = semantic_knn(*kp)
    rng = np.random.default_rng(kp.search * 100 + kp.k)
    W, H, Cn, n = 24, 10, 6, 400
    sp = make_params(width=W, height=H, n_classes=Cn, label_map=LM)
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = rng.integers(-30, 31, (n, 3))  # integer coordinates: |p|^2 is exact, only the sqrt rounds
    pts[pts[:, 0] == 0, 0] = 1.0
    pixel = rng.integers(0, W * H, n).astype(np.int32)
    pixel[rng.choice(n, 20, replace=False)] = -1
    proj_idx = np.full(W * H, -1, np.int32)
    r = np.sqrt((pts[:, :3].astype(np.float64) ** 2).sum(1))
    for i in np.argsort(-r, kind="stable"):  # nearest last: the nearest wins its pixel
        if pixel[i] >= 0:
            proj_idx[pixel[i]] = i
    scores = rng.uniform(-0.3, 1.0, (Cn, H * W)).astype(np.float32)
    scores[:, rng.choice(W * H, 15, replace=False)] = -0.5  # no class
    scores[0, rng.choice(W * H, 30, replace=False)] = 2.0  # class 0
    scores = scores.reshape(Cn, H, W)
    labels, probs, _, _, _ = knn_unproject(shim, sp, kp, pts, scores, pixel, proj_idx)
    n_labels, n_probs = numpy_knn(sp, kp, pts, scores, pixel, proj_idx)
    assert labels.tobytes() == n_labels.tobytes()
    assert probs.tobytes() == n_probs.tobytes()
    assert len(set(labels.tolist())) >= 4


def test_semantic_knn_layout_matches_c(shim):
    out = (C.c_uint64 * 5)()
    shim.knn_layout(out)
    assert out[0] == C.sizeof(SemanticKnnParams) == 16
    assert list(out[1:]) == [getattr(SemanticKnnParams, f).offset for f in ("search", "k", "sigma", "cutoff")]
    d = semantic_knn()
    assert (d.search, d.k, d.sigma, d.cutoff) == (5, 5, 1.0, 1.0)


def test_invalid_parameters_are_rejected(shim):
    bad = {1: [(0, 1, 1.0, 1.0), (4, 1, 1.0, 1.0), (11, 1, 1.0, 1.0)],
           2: [(5, 0, 1.0, 1.0), (5, 26, 1.0, 1.0), (1, 2, 1.0, 1.0)],
           3: [(5, 5, 0.0, 1.0), (5, 5, -1.0, 1.0), (5, 5, math.inf, 1.0), (5, 5, math.nan, 1.0)],
           4: [(5, 5, 1.0, math.inf), (5, 5, 1.0, math.nan)]}
    for rule, cases in bad.items():
        for c in cases:
            assert shim.knn_check(C.byref(semantic_knn(*c))) == rule, c
    for c in [(1, 1, 1e-30, 0.0), (9, 81, 1e30, -5.0), (3, 9, 0.5, 0.0), (5, 5, 1.0, 1.0)]:
        assert shim.knn_check(C.byref(semantic_knn(*c))) == 0, c
