"""RangeNet++'s KNN post-processing on the MI355X (csrc/k_semantic_knn.hip): the kernels bit for bit against the host
restatement (tests/semantic_knn_shim.c), k = 1 against the plain back-projection, the occlusion at a depth edge it
exists for, the pipeline's scores_knn entry against the standalone entry + processScanDevice, its device-side ordering
behind a producer stream, and parameter validation."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library: torch and libsuma_hip.so must share one HIP runtime

from semantic_suma_amd import core, kitti
from semantic_suma_amd.segmentation import SemanticFrontEnd, semantic_knn, semantic_params
from semantic_suma_amd.types import params_with_size
from test_gpu_semantic import GEOMETRIES, N_AZ, OneByOne, cuda, random_scores, same_state, scan_points, with_specials
from test_semantic_host import make_params
from test_semantic_knn_host import build_knn_shim, knn_unproject

pytestmark = pytest.mark.gpu

KNN = [(5, 5, 1.0, 1.0), (3, 2, 0.5, 0.0), (9, 16, 2.0, 0.5)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_knn_shim(tmp_path_factory.mktemp("semantic_knn_gpu"))


@pytest.fixture(scope="module")
def ctx():
    return core.Context(params_with_size(N_AZ), device=0)


@pytest.mark.parametrize("kp", KNN, ids=["5x5k5", "3x3k2", "9x9k16"])
@pytest.mark.parametrize("logits", [False, True], ids=["probs", "logits"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=["64x2048", "32x1024"])
def test_knn_bit_equal_to_host(ctx, shim, geo, logits, kp):
    check_knn(ctx, shim, geo, logits, semantic_knn(*kp))


def test_knn_after_its_scratch_grows(shim):
    """a fresh context votes on the smaller image first: the larger one needs a new record image on a used context"""
    ctx = core.Context(params_with_size(N_AZ), device=0)
    for geo in reversed(GEOMETRIES):
        check_knn(ctx, shim, geo, False, semantic_knn(*KNN[0]))


def check_knn(ctx, shim, geo, logits, kp):
    sp = make_params(**geo)
    fe = SemanticFrontEnd(ctx, sp)
    rng = np.random.default_rng(kp.search * 10 + int(logits))
    pts = with_specials(scan_points(1, 2048)[0])
    fe.project(cuda(pts))
    scores = random_scores(rng, 20, geo["height"], geo["width"])
    if logits:
        scores = scores * 8.0
    labels, probs = fe.unproject(cuda(scores)[None], logits=logits, knn=kp)
    torch.cuda.synchronize()
    pixel, proj_idx = fe.pixel.cpu().numpy(), fe.proj_idx.cpu().numpy()
    h_labels, h_probs, _, _, _ = knn_unproject(shim, sp, kp, pts, scores, pixel, proj_idx, logits=logits)
    assert labels.cpu().numpy().tobytes() == h_labels.tobytes()
    assert probs.cpu().numpy().tobytes() == h_probs.tobytes()
    assert (h_labels[pixel < 0] == 0).all() and len(set(h_labels.tolist())) > 5
    # the plain path differs somewhere: the vote is not a no-op
    p_labels, _ = fe.unproject(cuda(scores)[None], logits=logits)
    assert not np.array_equal(p_labels.cpu().numpy(), h_labels)


@pytest.mark.parametrize("kp", [(5, 1, 1.0, 1.0), (1, 1, 1.0, 0.0), (9, 1, 3.0, 0.0)], ids=["5x5", "1x1", "9x9"])
def test_k_one_is_the_plain_backprojection(ctx, shim, kp):
    kp = semantic_knn(*kp)
    sp = make_params(width=2048, height=64)
    fe = SemanticFrontEnd(ctx, sp)
    rng = np.random.default_rng(4)
    pts = with_specials(scan_points(2, 2048)[0])
    fe.project(cuda(pts))
    scores = cuda(random_scores(rng, 20, 64, 2048))[None]
    for logits in (False, True):
        k_labels, k_probs = fe.unproject(scores, logits=logits, knn=kp)
        p_labels, p_probs = fe.unproject(scores, logits=logits)
        torch.cuda.synchronize()
        pixel = fe.pixel.cpu().numpy()
        _, _, _, cls, _ = knn_unproject(shim, sp, kp, pts, scores[0].cpu().numpy(), pixel, fe.proj_idx.cpu().numpy(),
                                        logits=logits)
        keep = np.zeros(pixel.size, bool)
        keep[pixel >= 0] = cls[pixel[pixel >= 0]] >= 1
        assert keep.sum() > 50000
        assert np.array_equal(k_labels.cpu().numpy()[keep], p_labels.cpu().numpy()[keep])
        assert k_probs.cpu().numpy()[keep].tobytes() == p_probs.cpu().numpy()[keep].tobytes()
        assert (k_labels.cpu().numpy()[~keep] == 0).all()


def pixel_centre_point(sp, v, u, r):
    """the point at range r in the middle of pixel (v, u) of RangeNet++'s projection"""
    fov_down = np.radians(abs(sp.fov_down))
    fov = np.radians(abs(sp.fov_up) + abs(sp.fov_down))
    yaw = (2.0 * (u + 0.5) / sp.width - 1.0) * np.pi
    pitch = (1.0 - (v + 0.5) / sp.height) * fov - fov_down
    a = -yaw
    return [r * np.cos(pitch) * np.cos(a), r * np.cos(pitch) * np.sin(a), r * np.sin(pitch), 0.3]


def test_occluded_wall_points_are_not_labelled_pole(ctx):
    """a wall at 20 m (building scores, index 13) behind a two-column pole at 5 m (pole scores, index 18): the wall
    points hidden behind the pole get the pole's label 80 by the plain path and the wall's 50 by the KNN vote"""
    sp = make_params(width=2048, height=64)
    W = sp.width
    rows, cols, pole = range(12, 52), range(990, 1060), (1024, 1025)
    pts, kind = [], []
    for v in rows:
        for u in cols:
            pts.append(pixel_centre_point(sp, v, u, 20.0))
            kind.append("hidden" if u in pole else "wall")
            if u in pole:
                pts.append(pixel_centre_point(sp, v, u, 5.0))
                kind.append("pole")
    pts = np.array(pts, np.float32)
    kind = np.array(kind)
    fe = SemanticFrontEnd(ctx, sp)
    fe.project(cuda(pts))
    torch.cuda.synchronize()
    pixel = fe.pixel.cpu().numpy()
    expect = np.array([v * W + u for v in rows for u in cols for _ in range(2 if u in pole else 1)])
    assert np.array_equal(pixel, expect)  # every point in the pixel it was made for
    scores = np.zeros((20, 64 * W), np.float32)
    scores[13] = 0.7
    pole_px = [v * W + u for v in rows for u in pole]
    scores[13, pole_px] = 0.1
    scores[18, pole_px] = 0.8
    scores = cuda(scores.reshape(20, 64, W))[None]
    assert kitti.LEARNING_MAP_INV[13] == 50 and kitti.LEARNING_MAP_INV[18] == 80
    plain, _ = fe.unproject(scores)
    knn, knn_p = fe.unproject(scores, knn=semantic_knn())
    plain, knn, knn_p = plain.cpu().numpy(), knn.cpu().numpy(), knn_p.cpu().numpy()
    assert (kind == "hidden").sum() == 2 * len(rows)
    assert (plain[kind == "hidden"] == 80).all()
    assert (knn[kind == "hidden"] == 50).all() and (knn_p[kind == "hidden"] == np.float32(0.7)).all()
    assert (knn[kind == "pole"] == 80).all() and (knn_p[kind == "pole"] == np.float32(0.8)).all()
    assert (knn[kind == "wall"] == 50).all() and (plain[kind == "wall"] == 50).all()


def labelled_scans(sp, ctx, count, rng, logits=False):
    """synthetic scans with the scores of a plausible network: the ground-truth class of every pixel's winner ahead of
    uniform noise.  (Random per-pixel classes, smoothed by the vote into patches, are no scene: the semantic ICP's
    weights let such a run diverge on the host oracle as on the device.)"""
    fe = SemanticFrontEnd(ctx, sp)
    scans, scores = [], []
    for k in range(count):
        pts, lab = scan_points(k, N_AZ)
        fe.project(cuda(pts))
        torch.cuda.synchronize()
        proj = fe.proj_idx.cpu().numpy().ravel()
        cls = np.array([kitti.LEARNING_MAP[int(v)] for v in lab], np.int64)
        s = rng.uniform(0.0, 0.5, (20, proj.size)).astype(np.float32)
        won = proj >= 0
        s[cls[proj[won]], np.nonzero(won)[0]] += 0.6
        scans.append(pts)
        scores.append(s.reshape(20, sp.height, sp.width) * (8.0 if logits else 1.0))
    return scans, scores


def run_knn_pipeline(sps, kp, scans, scores, logits):
    """sps: the semantic parameters of every scan"""
    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    for sp, pts, sc in zip(sps, scans, scores):
        fe = SemanticFrontEnd(hp, sp)
        d_pts = cuda(pts)
        fe.project(d_pts)
        d_sc = cuda(sc)
        torch.cuda.synchronize()
        hp.processScanScores(sp, d_pts.data_ptr(), d_sc.data_ptr(), fe.pixel.data_ptr(), pts.shape[0], logits=logits,
                             fixed_iterations=10, knn=kp, d_proj_idx=fe.proj_idx.data_ptr())
        hp.ctx.synchronize()
    return hp


def run_standalone_then_device(sps, kp, ctx, scans, scores, logits):
    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    for sp, pts, sc in zip(sps, scans, scores):
        fe = SemanticFrontEnd(ctx, sp)
        d_pts = cuda(pts)
        fe.project(d_pts)
        labels, probs = fe.unproject(cuda(sc)[None], logits=logits, knn=kp)
        torch.cuda.synchronize()
        hp.processScanDevice(d_pts.data_ptr(), labels.data_ptr(), probs.data_ptr(), pts.shape[0], fixed_iterations=10)
        hp.ctx.synchronize()
    return hp


@pytest.mark.parametrize("side", ["side_stream", "one_stream"])
def test_pipeline_knn_entry_equals_standalone_then_device(ctx, monkeypatch, side):
    if side == "one_stream":
        monkeypatch.setenv("SUMA_NO_SIDE_STREAM", "1")
    sp = make_params(width=1024, height=64)
    kp = semantic_knn()
    for logits in (False, True):
        scans, scores = labelled_scans(sp, ctx, 5, np.random.default_rng(6), logits)
        a = run_knn_pipeline([sp] * len(scans), kp, scans, scores, logits)
        b = run_standalone_then_device([sp] * len(scans), kp, ctx, scans, scores, logits)
        same_state(a, b)
        assert len(np.unique(a.map.getAllSurfels()["r"])) > 2  # the voted labels reached the map


def test_pipeline_knn_entry_after_its_buffers_grow(ctx):
    """a first scan on a narrower image, then a second one with every point twice: the record image and the labels of
    the scores_knn entry grow on a pipeline that has used them"""
    narrow, sp = make_params(width=512, height=64), make_params(width=1024, height=64)
    kp = semantic_knn()
    rng = np.random.default_rng(13)
    scans, scores = labelled_scans(narrow, ctx, 1, rng)
    more = labelled_scans(sp, ctx, 4, rng)
    scans, scores = scans + more[0][1:], scores + more[1][1:]
    scans[1] = np.concatenate([scans[1], scans[1]])
    assert scans[1].shape[0] > scans[0].shape[0] * 5 // 4 + 1024
    sps = [narrow] + [sp] * (len(scans) - 1)
    a = run_knn_pipeline(sps, kp, scans, scores, False)
    b = run_standalone_then_device(sps, kp, ctx, scans, scores, False)
    same_state(a, b)


def test_front_end_process_scan_with_knn_equals_the_manual_path():
    sp = semantic_params(1024, 64, 3.0, -25.0, means=(12.1, 10.9, 0.2, -1.0, 0.2), stds=(12.3, 11.6, 9.0, 0.8, 0.15))
    kp = semantic_knn(search=7, k=9, sigma=1.5, cutoff=2.0)
    model = OneByOne()
    scans = [scan_points(k, N_AZ)[0] for k in range(3)]
    a = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fa = SemanticFrontEnd(a, sp)
    for pts in scans:
        fa.process_scan(None, cuda(pts), model, fixed_iterations=10, logits=True, knn=kp)
    b = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fb = SemanticFrontEnd(b, sp)
    for pts in scans:
        d_pts = cuda(pts)
        inp = fb.project(d_pts)
        labels, probs = fb.unproject(model(inp), logits=True, knn=kp)
        torch.cuda.synchronize()
        b.processScanDevice(d_pts.data_ptr(), labels.data_ptr(), probs.data_ptr(), pts.shape[0], fixed_iterations=10)
        b.ctx.synchronize()
    torch.cuda.synchronize()
    same_state(a, b)


@pytest.mark.parametrize("side", ["side_stream", "one_stream"])
def test_knn_entry_waits_for_the_producer_on_the_device(ctx, monkeypatch, side):
    if side == "one_stream":
        monkeypatch.setenv("SUMA_NO_SIDE_STREAM", "1")
    sp = make_params(width=1024, height=64)
    kp = semantic_knn()
    scans, scores = labelled_scans(sp, ctx, 3, np.random.default_rng(9))
    ref = run_knn_pipeline([sp] * len(scans), kp, scans, scores, False)

    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fe = SemanticFrontEnd(hp, sp)
    producer = torch.cuda.Stream()
    keep = []
    for pts, sc in zip(scans, scores):
        d_pts = cuda(pts)
        fe.project(d_pts)
        real = cuda(sc)
        buf = torch.full_like(real, -1.0)  # sentinel: all negative -> no class anywhere -> label 0, prob 0
        torch.cuda.synchronize()
        with torch.cuda.stream(producer):
            torch.cuda._sleep(100_000_000)  # a long busy kernel in front of the scores
            buf.copy_(real)
            ev = torch.cuda.Event()
            ev.record(producer)
        hp.processScanScores(sp, d_pts.data_ptr(), buf.data_ptr(), fe.pixel.data_ptr(), pts.shape[0],
                             producer_event=ev.cuda_event, fixed_iterations=10, knn=kp,
                             d_proj_idx=fe.proj_idx.data_ptr())
        keep.append((d_pts, real, buf, ev, fe.pixel, fe.proj_idx))
    torch.cuda.synchronize()
    hp.ctx.synchronize()
    same_state(hp, ref)


def test_invalid_knn_params_are_errors(ctx):
    d_pts = cuda(scan_points(0, 64)[0])
    n = d_pts.shape[0]
    sp = make_params(width=64, height=8)
    scores = torch.zeros(20 * 64 * 8, dtype=torch.float32, device="cuda")
    pix = torch.zeros(n, dtype=torch.int32, device="cuda")
    proj = torch.full((64 * 8,), -1, dtype=torch.int32, device="cuda")
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    bad = {"search": [(4, 1, 1.0, 1.0), (11, 1, 1.0, 1.0), (0, 1, 1.0, 1.0)],
           "k": [(5, 0, 1.0, 1.0), (3, 10, 1.0, 1.0)],
           "sigma": [(5, 5, 0.0, 1.0), (5, 5, float("nan"), 1.0), (5, 5, float("inf"), 1.0)],
           "cutoff": [(5, 5, 1.0, float("inf")), (5, 5, 1.0, float("nan"))]}
    L = ctx.L
    for what, cases in bad.items():
        for c in cases:
            kp = semantic_knn(*c)
            rc = L.suma_semantic_unproject_knn(ctx.h, C.byref(sp), C.byref(kp), d_pts.data_ptr(), scores.data_ptr(), 0,
                                               pix.data_ptr(), proj.data_ptr(), n, out.data_ptr(), out.data_ptr())
            msg = L.suma_last_error(ctx.h).decode()
            assert rc == -1 and "suma_semantic_knn" in msg and what in msg, (c, msg)
    rc = L.suma_semantic_unproject_knn(ctx.h, C.byref(sp), None, d_pts.data_ptr(), scores.data_ptr(), 0,
                                       pix.data_ptr(), proj.data_ptr(), n, out.data_ptr(), out.data_ptr())
    assert rc == -1 and "NULL" in L.suma_last_error(ctx.h).decode()
    rc = L.suma_semantic_unproject_knn(ctx.h, C.byref(sp), C.byref(semantic_knn()), d_pts.data_ptr(),
                                       scores.data_ptr(), 0, pix.data_ptr(), None, n, out.data_ptr(), out.data_ptr())
    assert rc == -1 and "NULL buffer" in L.suma_last_error(ctx.h).decode()
    bad_sp = make_params(width=64, height=8, n_classes=0)
    rc = L.suma_semantic_unproject_knn(ctx.h, C.byref(bad_sp), C.byref(semantic_knn()), d_pts.data_ptr(),
                                       scores.data_ptr(), 0, pix.data_ptr(), proj.data_ptr(), n, out.data_ptr(),
                                       out.data_ptr())
    assert rc == -1 and "n_classes" in L.suma_last_error(ctx.h).decode()
    # the pipeline entry refuses them too, and the pipeline goes on with valid ones
    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    with pytest.raises(core.SumaError, match="sigma"):
        hp.processScanScores(sp, d_pts.data_ptr(), scores.data_ptr(), pix.data_ptr(), n, knn=semantic_knn(sigma=-1.0),
                             d_proj_idx=proj.data_ptr())
    with pytest.raises(core.SumaError, match="NULL buffer"):
        hp.processScanScores(sp, d_pts.data_ptr(), scores.data_ptr(), pix.data_ptr(), n, knn=semantic_knn())
    sp = make_params(width=256, height=64)
    fe = SemanticFrontEnd(hp, sp)
    scans, scores = labelled_scans(sp, ctx, 1, np.random.default_rng(1))
    d_pts = cuda(scans[0])
    fe.project(d_pts)
    sc = cuda(scores[0])
    torch.cuda.synchronize()
    hp.processScanScores(sp, d_pts.data_ptr(), sc.data_ptr(), fe.pixel.data_ptr(), d_pts.shape[0],
                         fixed_iterations=10, knn=semantic_knn(), d_proj_idx=fe.proj_idx.data_ptr())
    hp.ctx.synchronize()
    assert hp.L.suma_pipeline_timestamp(hp.h) == 1 and hp.map.size() > 5000
