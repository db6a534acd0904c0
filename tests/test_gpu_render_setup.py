"""k_render's per-quad set-up (semantic_suma_amd/csrc/raster_quad.h: phase 1b leaves each quad's areas, orientations and
edge ownership in LDS, phase 2 tests pixels against them) on maps made for it, bit for bit against the oracle: render
(merged and unmerged), render_active with the fused K7 splat, and render_composed, at 48 x 12 and 333 x 10.

The map has 513 surfels, all of them survivors of the new pass from the identity view: one tile of exactly 256 survivors
and 257 more over a tile pair.  Every second normal is tilted to within a few degrees of the viewing ray and its disc made
large, so that the spherical projection turns, folds and crosses the quad: both orientations of each strip triangle occur
independently.  Every fourth surfel is far smaller than a pixel: survivors without a pixel test share a block with
survivors that have some, and a test that read such a survivor's LDS row (which still holds phase 1a's candidate record,
not a set-up) would draw garbage.  That each of these classes is present is asserted from the ORACLE's corners."""
import numpy as np
import pytest

import render_ref as R
import test_render_crafted_host as H
from test_gpu_render_crafted import HipSide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


SIZES = ((48, 12), (333, 10))
N = 513


def setup_scene(W, Hh):
    p = H.params(W, Hh)
    rng = np.random.default_rng(5)
    k = np.arange(N)
    d = H.direction(p, rng.uniform(0.03 * W, 0.97 * W, N), rng.uniform(0.08 * Hh, 0.92 * Hh, N))
    depth = rng.uniform(4.0, 30.0, N)
    side = np.cross(d, rng.normal(size=(N, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    grazing, tiny = k % 2 == 0, k % 4 == 1
    dot = np.where(grazing, rng.uniform(0.02, 0.2, N), rng.uniform(0.6, 1.0, N))  # front-face product; the gate is 0.01
    nrm = dot[:, None] * (-d) + np.sqrt(1.0 - dot ** 2)[:, None] * side
    px = np.where(grazing, rng.uniform(3.0, 40.0, N), rng.uniform(0.3, 6.0, N))
    px = np.where(tiny, rng.uniform(0.02, 0.2, N), px)
    creation = np.asarray(H.CREATION_STAMPS)[rng.integers(0, 4, N)]
    rec = H.make_records(depth[:, None] * d, nrm, 0.5 * px * depth * H.pixel_angle(p), creation, creation + 60)
    view = H.VIEW_I
    calls = [("render", view, view, 0.0), ("render", view, H.nudged(view), 0.0), ("active", view, None, 0.0),
             ("composed", view, H.nudged(view), 0.0)]
    return H.scene(f"setup-{W}x{Hh}", p, rec, calls)


def check_classes(oracle_lib, sc):
    """from the oracle's snapped corners of the new pass: what the docstring promises"""
    p = sc["params"]
    o = oracle_lib.Oracle(p)
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    emitted, corners, _ = o.debug_render_quads(H.VIEW_I, 0.0, R.NEW, 50)
    assert emitted.all() and len(emitted) == N, "every surfel must survive: tiles of 256, 256 and 1 survivors"
    tests, X, Y = H.snapped_boxes(p, corners)
    a1 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])  # E(v0, v1; v2)
    a2 = (X[:, 1] - X[:, 2]) * (Y[:, 3] - Y[:, 2]) - (Y[:, 1] - Y[:, 2]) * (X[:, 3] - X[:, 2])  # E(v2, v1; v3)
    tested = tests > 0
    found = {(s1, s2): int(np.count_nonzero(tested & (np.sign(a1) == s1) & (np.sign(a2) == s2))) for s1 in (1, -1) for s2 in (1, -1)}
    print(f"{sc['id']}: {int(tests.sum())} pixel tests, quads with tests by (sign a1, sign a2): {found}")
    assert min(found.values()) >= 3, f"orientation classes {found}"
    for tile in (slice(0, 256), slice(256, 512)):
        assert np.count_nonzero(tests[tile] == 0) >= 20 and np.count_nonzero(tests[tile] > 0) >= 100, "no-test survivors beside tested ones"
    old = o.debug_render_quads(H.VIEW_I, 0.0, R.OLD, 50)[0].astype(bool)
    assert 50 < old.sum() < N - 50, "render_composed and the unmerged render need an old pass too"


@pytest.mark.parametrize("W,Hh", SIZES)
def test_setup_scene_equals_oracle(hip, oracle_lib, W, Hh):
    sc = setup_scene(W, Hh)
    check_classes(oracle_lib, sc)
    kernel, oracle = HipSide(hip, sc["params"]), H.OracleSide(oracle_lib, sc["params"])
    got, want = H.run_scene(kernel, sc), H.run_scene(oracle, sc)
    H.assert_results_equal(got, want, sc["id"])
    for r in H.written(want, sc["calls"]):  # the comparison is of drawn frames
        assert all(np.count_nonzero(r[nm][0][..., 3]) > 20 for nm in r), "an empty rendering"
    # winners: the semantic payload of a render is the winning surfel's index
    for k in (0, 1):
        for nm in ("old", "new", "out"):
            assert np.array_equal(H.semantic_ids(got[k][nm][2]), H.semantic_ids(want[k][nm][2]))
    # the index map of an update at the pose render_active has just drawn from: K7 rode on that pass
    assert sc["calls"][2][0] == "active"
    kernel.call(sc["calls"][2])
    oracle.call(sc["calls"][2])
    im_got, im_want = kernel.index_map(sc["calls"][2][1]), oracle.index_map(sc["calls"][2][1])
    assert np.count_nonzero(im_want) > 20
    np.testing.assert_array_equal(im_got, im_want, err_msg=f"{sc['id']}: index map differs from the oracle's")
