"""The semantic front end on the MI355X (csrc/k_semantic.hip, semantic_suma_amd/segmentation.py): projection and
back-projection bit for bit against the host restatement (tests/semantic_shim.c), the pipeline's scores entry against
the existing host-label path, its device-side ordering behind a producer stream, and parameter validation."""
import numpy as np
import pytest
import torch  # before the library: torch and libsuma_hip.so must share one HIP runtime

from semantic_suma_amd import core, kitti, synth
from semantic_suma_amd.segmentation import SemanticFrontEnd, semantic_params
from semantic_suma_amd.types import params_with_size
from test_semantic_host import build_shim, make_params
from test_semantic_host import project as host_project
from test_semantic_host import unproject as host_unproject

pytestmark = pytest.mark.gpu

N_AZ = 900  # pipeline scans: 64 x 900 data image (as smoke())


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("semantic_gpu"))


@pytest.fixture(scope="module")
def ctx():
    return core.Context(params_with_size(N_AZ), device=0)


def remission(n):
    return (((np.arange(n, dtype=np.int64) * 2654435761) % 1000) / 1000.0).astype(np.float32)


def scan_points(k, n_azimuth, w="remission"):
    pts, lab, prob, _ = synth.generate_scan(k, n_azimuth=n_azimuth)
    pts = pts.copy()
    if w == "remission":
        pts[:, 3] = remission(pts.shape[0])
    return pts, lab


def with_specials(pts):
    """planted ties (exact duplicates, later in the order), a zero-range point and non-finite coordinates"""
    extra = np.concatenate([pts[::97], pts[5::131]], axis=0).copy()
    extra[:, 3] = 0.5
    bad = np.array([[0, 0, 0, 0.1], [np.nan, 1, 1, 0.1], [np.inf, 0, 0, 0.1], [1, -np.inf, 0, 0.1]], dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([pts, extra, bad], axis=0), dtype=np.float32)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_scores(rng, C, H, W):
    s = rng.uniform(-0.2, 1.0, (C, H, W)).astype(np.float32)
    flat = s.reshape(C, -1)
    P = flat.shape[1]
    idx = rng.choice(P, P // 10, replace=False)
    flat[:, idx[: P // 40]] = -rng.uniform(0.01, 1.0, (C, P // 40))  # all negative
    tie = idx[P // 40: P // 20]
    j = rng.integers(0, C - 1, tie.size)
    flat[j, tie] = 2.0
    flat[j + 1 + rng.integers(0, C - 1 - j), tie] = 2.0  # two equal maxima: the later one wins
    nan = idx[P // 20:]
    flat[rng.integers(0, C, nan.size), nan] = np.nan
    flat[rng.integers(0, C, nan.size), nan] = np.nan
    return s


GEOMETRIES = [dict(width=2048, height=64, fov_up=3.0, fov_down=-25.0),
              dict(width=1024, height=32, fov_up=10.0, fov_down=-30.0)]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=["64x2048", "32x1024"])
def test_projection_bit_equal_to_host(ctx, shim, geo):
    check_projection(ctx, shim, geo)


def test_projection_after_the_z_buffer_grows(shim):
    """a fresh context projects the smaller image first: the larger one needs a new z-buffer on a used context"""
    ctx = core.Context(params_with_size(N_AZ), device=0)
    for geo in reversed(GEOMETRIES):
        check_projection(ctx, shim, geo)


def check_projection(ctx, shim, geo):
    sp = make_params(**geo)
    fe = SemanticFrontEnd(ctx, sp)
    for k in (0, 3):
        pts = with_specials(scan_points(k, 2048)[0])
        inp = fe.project(cuda(pts))
        torch.cuda.synchronize()
        h_inp, h_pixel, h_proj = host_project(shim, sp, pts)
        assert tuple(inp.shape) == (1, 5, geo["height"], geo["width"])
        assert inp[0].cpu().numpy().tobytes() == h_inp.tobytes()
        assert np.array_equal(fe.pixel.cpu().numpy(), h_pixel)
        assert np.array_equal(fe.proj_idx.cpu().numpy(), h_proj)
        assert (h_pixel[-4:] == -1).all() and (h_proj >= 0).sum() > 0.5 * h_proj.size


@pytest.mark.parametrize("logits", [False, True], ids=["probs", "logits"])
def test_backprojection_bit_equal_to_host(ctx, shim, logits):
    sp = make_params(width=2048, height=64)
    fe = SemanticFrontEnd(ctx, sp)
    rng = np.random.default_rng(11)
    pts = with_specials(scan_points(1, 2048)[0])
    fe.project(cuda(pts))
    scores = random_scores(rng, 20, 64, 2048)
    if logits:
        scores = scores * 8.0
    labels, probs = fe.unproject(cuda(scores)[None], logits=logits)
    torch.cuda.synchronize()
    pixel = fe.pixel.cpu().numpy()
    h_labels, h_probs = host_unproject(shim, sp, scores, pixel, logits=logits)
    assert labels.cpu().numpy().tobytes() == h_labels.tobytes()
    assert probs.cpu().numpy().tobytes() == h_probs.tobytes()
    assert (h_labels[pixel < 0] == 0).all() and len(set(h_labels.tolist())) > 5


def test_one_hot_scores_give_back_the_ground_truth(ctx):
    sp = make_params(width=2048, height=64)
    fe = SemanticFrontEnd(ctx, sp)
    pts, lab = scan_points(2, 2048)
    fe.project(cuda(pts))
    torch.cuda.synchronize()
    pixel, proj = fe.pixel.cpu().numpy(), fe.proj_idx.cpu().numpy().ravel()
    winners = proj[proj >= 0]
    cls = np.array([kitti.LEARNING_MAP[int(v)] for v in lab], dtype=np.int64)
    scores = np.zeros((20, proj.size), dtype=np.float32)
    scores[cls[winners], np.nonzero(proj >= 0)[0]] = 1.0
    labels, probs = fe.unproject(cuda(scores.reshape(20, 64, 2048))[None])
    labels, probs = labels.cpu().numpy(), probs.cpu().numpy()
    won = np.zeros(pts.shape[0], dtype=bool)
    won[winners] = True
    assert won.sum() > 50000
    assert np.array_equal(labels[won], kitti.remap_labels(lab.astype(np.int64))[won])
    assert np.array_equal(labels[won], lab[won])  # synth's road / car / building are their own learning_map_inv ids
    assert (probs[won] == 1.0).all()


def run_scores_pipeline(sp, scans, scores, logits, producer=None):
    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fe = SemanticFrontEnd(hp, sp)
    for pts, sc in zip(scans, scores):
        d_pts = cuda(pts)
        fe.project(d_pts)
        d_sc = cuda(sc)
        torch.cuda.synchronize()
        hp.processScanScores(sp, d_pts.data_ptr(), d_sc.data_ptr(), fe.pixel.data_ptr(), pts.shape[0], logits=logits,
                             fixed_iterations=10)
        hp.ctx.synchronize()
    return hp


def run_host_pipeline(sp, ctx, scans, scores, logits, w_one):
    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fe = SemanticFrontEnd(ctx, sp)
    for pts, sc in zip(scans, scores):
        fe.project(cuda(pts))
        labels, probs = fe.unproject(cuda(sc)[None], logits=logits)
        torch.cuda.synchronize()
        host_pts = pts.copy()
        if w_one:
            host_pts[:, 3] = 1.0
        hp.processScan(host_pts, labels.cpu().numpy(), probs.cpu().numpy(), fixed_iterations=10)
    return hp


def same_state(a, b):
    assert np.array_equal(a.getCurrentPose(), b.getCurrentPose())
    assert a.map.size() == b.map.size() > 5000
    assert a.map.getAllSurfels().tobytes() == b.map.getAllSurfels().tobytes()


@pytest.mark.parametrize("side", ["side_stream", "one_stream"])
@pytest.mark.parametrize("w", ["one", "remission"])
def test_pipeline_scores_entry_equals_host_labels(ctx, monkeypatch, side, w):
    if side == "one_stream":
        monkeypatch.setenv("SUMA_NO_SIDE_STREAM", "1")
    sp = make_params(width=1024, height=64)
    rng = np.random.default_rng(5)
    scans = [scan_points(k, N_AZ, w=w)[0] for k in range(5)]
    scores = [random_scores(rng, 20, 64, 1024) for _ in scans]
    for logits in (False, True):
        a = run_scores_pipeline(sp, scans, scores, logits)
        b = run_host_pipeline(sp, ctx, scans, scores, logits, w_one=True)
        same_state(a, b)
        labels = a.map.getAllSurfels()["r"]
        assert len(np.unique(labels)) > 5  # the scores' labels reached the map


def test_pipeline_scores_entry_after_its_labels_grow(ctx):
    """a second scan with every point twice: the scores entry's labels grow on a pipeline that has used them"""
    sp = make_params(width=1024, height=64)
    rng = np.random.default_rng(12)
    scans = [scan_points(k, N_AZ)[0] for k in range(4)]
    scans[1] = np.concatenate([scans[1], scans[1]])
    assert scans[1].shape[0] > scans[0].shape[0] * 5 // 4 + 1024
    scores = [random_scores(rng, 20, 64, 1024) for _ in scans]
    a = run_scores_pipeline(sp, scans, scores, False)
    b = run_host_pipeline(sp, ctx, scans, scores, False, w_one=True)
    same_state(a, b)


@pytest.mark.parametrize("side", ["side_stream", "one_stream"])
def test_scores_entry_waits_for_the_producer_on_the_device(monkeypatch, side):
    if side == "one_stream":
        monkeypatch.setenv("SUMA_NO_SIDE_STREAM", "1")
    sp = make_params(width=1024, height=64)
    rng = np.random.default_rng(9)
    scans = [scan_points(k, N_AZ)[0] for k in range(3)]
    scores = [rng.uniform(0.0, 1.0, (20, 64, 1024)).astype(np.float32) for _ in scans]
    ref = run_scores_pipeline(sp, scans, scores, False)

    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fe = SemanticFrontEnd(hp, sp)
    producer = torch.cuda.Stream()
    keep = []
    for pts, sc in zip(scans, scores):
        d_pts = cuda(pts)
        fe.project(d_pts)
        real = cuda(sc)
        buf = torch.full_like(real, -1.0)  # sentinel: all negative -> label 0, prob 0 everywhere
        torch.cuda.synchronize()
        with torch.cuda.stream(producer):
            torch.cuda._sleep(100_000_000)  # a long busy kernel in front of the scores
            buf.copy_(real)
            ev = torch.cuda.Event()
            ev.record(producer)
        hp.processScanScores(sp, d_pts.data_ptr(), buf.data_ptr(), fe.pixel.data_ptr(), pts.shape[0],
                             producer_event=ev.cuda_event, fixed_iterations=10)
        keep.append((d_pts, real, buf, ev, fe.pixel))
    torch.cuda.synchronize()
    hp.ctx.synchronize()
    same_state(hp, ref)


class OneByOne(torch.nn.Module):
    """a fixed 1 x 1 convolution 5 -> 20, written out per channel (one fixed fp32 operation order)"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.w = torch.randn(20, 5, generator=g).cuda()
        self.b = torch.randn(20, generator=g).cuda()

    def forward(self, x):
        out = self.b[None, :, None, None] + self.w[None, :, 0, None, None] * x[:, 0:1]
        for c in range(1, 5):
            out = out + self.w[None, :, c, None, None] * x[:, c:c + 1]
        return out


def test_front_end_process_scan_equals_the_manual_path():
    sp = semantic_params(1024, 64, 3.0, -25.0, means=(12.1, 10.9, 0.2, -1.0, 0.2), stds=(12.3, 11.6, 9.0, 0.8, 0.15))
    model = OneByOne()
    scans = [scan_points(k, N_AZ)[0] for k in range(4)]
    a = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fa = SemanticFrontEnd(a, sp)
    for pts in scans:
        fa.process_scan(None, cuda(pts), model, fixed_iterations=10, logits=True)
    b = core.SurfelMapping(params_with_size(N_AZ), device=0)
    fb = SemanticFrontEnd(b, sp)
    for pts in scans:
        d_pts = cuda(pts)
        inp = fb.project(d_pts)
        labels, probs = fb.unproject(model(inp), logits=True)
        torch.cuda.synchronize()
        b.processScanDevice(d_pts.data_ptr(), labels.data_ptr(), probs.data_ptr(), pts.shape[0], fixed_iterations=10)
        b.ctx.synchronize()
    torch.cuda.synchronize()
    same_state(a, b)
    assert len(np.unique(a.map.getAllSurfels()["r"])) > 2


def test_invalid_semantic_params_are_errors(ctx):
    import ctypes as C
    d_pts = cuda(scan_points(0, 64)[0])
    n = d_pts.shape[0]
    buf = torch.zeros(32 * 64 * 8 + n, dtype=torch.float32, device="cuda")
    pix = torch.zeros(n, dtype=torch.int32, device="cuda")
    labels = torch.empty(n, dtype=torch.float32, device="cuda")
    bad = {
        "n_classes": make_params(width=64, height=8, n_classes=0),
        "n_classes ": make_params(width=64, height=8, n_classes=33),
        "std": make_params(width=64, height=8, stds=(1.0, 1.0, 0.0, 1.0, 1.0)),
        "overflows": make_params(width=65536, height=65536),
        "empty": make_params(width=0, height=8),
        "fov": make_params(width=64, height=8, fov_up=0.0, fov_down=0.0),
    }
    L = ctx.L
    for what, sp in bad.items():
        rc = L.suma_semantic_project(ctx.h, C.byref(sp), d_pts.data_ptr(), n, buf.data_ptr(), pix.data_ptr(), None)
        assert rc == -1
        msg = L.suma_last_error(ctx.h).decode()
        assert "suma_semantic_params" in msg and what.strip() in msg, msg
        rc = L.suma_semantic_unproject(ctx.h, C.byref(sp), buf.data_ptr(), 0, pix.data_ptr(), n, labels.data_ptr(),
                                       labels.data_ptr())
        assert rc == -1 and what.strip() in L.suma_last_error(ctx.h).decode()
    # the pipeline entry refuses them too, and the pipeline goes on with valid ones
    hp = core.SurfelMapping(params_with_size(N_AZ), device=0)
    with pytest.raises(core.SumaError, match="std"):
        hp.processScanScores(bad["std"], d_pts.data_ptr(), buf.data_ptr(), pix.data_ptr(), n)
    sp = make_params(width=256, height=64)
    fe = SemanticFrontEnd(hp, sp)
    d_pts = cuda(scan_points(0, N_AZ)[0])
    fe.project(d_pts)
    scores = torch.rand((1, 20, 64, 256), device="cuda")
    torch.cuda.synchronize()
    hp.processScanScores(sp, d_pts.data_ptr(), scores.data_ptr(), fe.pixel.data_ptr(), d_pts.shape[0],
                         fixed_iterations=10)
    hp.ctx.synchronize()
    assert hp.L.suma_pipeline_timestamp(hp.h) == 1 and hp.map.size() > 5000
