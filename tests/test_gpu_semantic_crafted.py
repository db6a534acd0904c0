"""The semantic front end (csrc/k_semantic.hip: ks_scatter, ks_resolve, ks_unproject) and the KNN vote
(csrc/k_semantic_knn.hip: kk_pixels and every instantiation of kk_points) on the crafted scenes of
tests/test_semantic_crafted_host.py: every scene through SemanticFrontEnd.project / .unproject (plain and knn=, with the
scene's own pixel / proj_idx where it crafts them), compared bit for bit with the host restatements AND -- whatever fp64
decides -- directly with the fp64 statement of tests/semantic_ref.py under the host file's assertions.  The host file proves
on the CPU that the restatements meet the same assertions, that the caps hold and that every row's property holds; this
file holds no tolerance of its own.  The sequence rows run on ONE context: the z-buffer that ks_resolve re-arms and the
record image of the KNN carry nothing from one call to the next."""
import numpy as np
import pytest
import torch  # before the library: torch and libsuma_hip.so must share one HIP runtime

import test_semantic_crafted_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


@pytest.fixture(scope="module")
def ctx(hip):
    from semantic_suma_amd.types import params_with_size
    return hip.Context(params_with_size(64), device=0)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def front_end(ctx, sp):
    from semantic_suma_amd.segmentation import SemanticFrontEnd
    return SemanticFrontEnd(ctx, sp)


def project(ctx, sc):
    """-> (input [5, H, W], pixel [n], proj_idx [H, W]) as numpy; every buffer is exactly as large as the kernels read"""
    fe = front_end(ctx, sc["sp"])
    inp = fe.project(cuda(sc["pts"]))
    torch.cuda.synchronize()
    return inp[0].cpu().numpy(), fe.pixel.cpu().numpy(), fe.proj_idx.cpu().numpy()


def unproject(ctx, sc):
    """scores C x P, pixel / labels / probs n, proj_idx P, points n x 4"""
    fe = front_end(ctx, sc["sp"])
    kw = {}
    if sc["kind"] == "knn":
        kw = dict(knn=sc["kp"], points=cuda(sc["pts"]), proj_idx=cuda(np.asarray(sc["proj_idx"], np.int32)))
    labels, probs = fe.unproject(cuda(sc["scores"]), logits=sc["logits"], pixel=cuda(np.asarray(sc["pixel"], np.int32)),
                                 **kw)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), probs.cpu().numpy()


_RESULTS = {}


def hip_results(ctx, sid):
    """the kernels' result of a scene, computed once and shared"""
    if sid not in _RESULTS:
        sc = H.get_scene(sid)
        _RESULTS[sid] = project(ctx, sc) if sc["kind"] == "proj" else unproject(ctx, sc)
    return _RESULTS[sid]


@pytest.mark.parametrize("sid", H.PROJ_IDS)
def test_projection_scene(ctx, sid):
    got = hip_results(ctx, sid)
    H.assert_same_bits(got, H.shim_results(sid), sid)
    H.check_projection(sid, got, "kernel")
    # the back-projection of what was projected, plain and voted, probabilities and logits
    for f in H.followup_scenes(sid, got[1], got[2]):
        out = unproject(ctx, f)
        H.assert_same_bits(out, H.run_shim(f), f["id"])
        H.CHECKS[f["kind"]](f, out, "kernel")


@pytest.mark.parametrize("sid", H.UNPROJ_IDS)
def test_backprojection_scene(ctx, sid):
    got = hip_results(ctx, sid)
    H.assert_same_bits(got, H.shim_results(sid), sid)
    H.check_unproject(sid, got, "kernel")


@pytest.mark.parametrize("sid", H.KNN_IDS)
def test_knn_scene(ctx, sid):
    got = hip_results(ctx, sid)
    H.assert_same_bits(got, H.shim_results(sid), sid)
    H.check_knn(sid, got, "kernel")


@pytest.mark.parametrize("name", list(H.SEQUENCES))
def test_sequence_on_one_context(hip, name):
    """full scan, n = 0, one point, the full scan again; and large -> small -> large -> another size: each result equals
    the fresh context's (which equals the host's), the vote that follows each projection included"""
    from semantic_suma_amd.types import params_with_size
    one = hip.Context(params_with_size(64), device=0)
    for step, sid in enumerate(H.SEQUENCES[name]):
        sc = H.get_scene(sid)
        got = project(one, sc)
        H.assert_same_bits(got, H.shim_results(sid), f"{name} step {step}: {sid}")
        H.check_projection(sid, got, f"kernel, {name} step {step}")
        for f in H.followup_scenes(sid, got[1], got[2]):
            H.assert_same_bits(unproject(one, f), H.run_shim(f), f"{name} step {step}: {f['id']}")
