"""The fixed-function half of the reference's render passes, pinned against a REAL OpenGL implementation.

Rounds 1-3 had to call triangle coverage, the 24-bit depth test and the other GL behaviour around the shaders "the
builder's reading of the specification": neither machine has an X server, EGL or OSMesa.  The image does ship Mesa's DRI
drivers, though, and oracle/glref.py drives swrast_dri.so (llvmpipe, OpenGL 4.5 core) directly through the DRI
software-rasteriser interface.  These tests (CPU only; skipped where Mesa is not installed) run

  * own pass-through shaders fed with the ORACLE'S vertices -- nothing but GL's clipping / rasterisation / depth test
    decides the outcome, so the comparison with oracle/o_map.c is exact up to what the GL specification leaves open
    (a pixel centre lying ON an edge, sub-pixel snapping of the last 1/256 pixel);
  * the reference's OWN render_surfels.{vert,geom,frag} on a map the oracle built: here the driver's atan / asin / FMA
    contraction and its attribute interpolation differ from include/suma_detmath.h in the last ulps, so agreement is
    measured, not demanded: >= 97 % of the texels carry the same surfel.

What the reference's shaders produced in llvmpipe for the tests that need nothing else on the reference side is recorded in
tests/golden/gl_reference_900x64.npz (tests/golden/make_gl_reference_golden.py, where the reference's sources and Mesa
exist), together with a digest of the inputs the oracle gave them; those tests need neither here.  Each GL image is
stored as the XOR of its bits with the oracle's image of the same pass (see `recorded`).
"""
import hashlib
import os

import numpy as np
import pytest

from conftest import get_scan
from semantic_suma_amd.types import params_with_size

W, H = 900, 64
GL_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gl_reference_900x64.npz")


def digest(*arrays):
    """SHA-256 of the bytes of the arrays, in order (the same function as tests/golden/make_gl_reference_golden.py)"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def gl_golden(key, *inputs):
    """the recorded GL outputs, after checking that `inputs` are the ones the recording of `key` was made from"""
    z = np.load(GL_GOLDEN)
    assert str(z[key + "_digest"]) == digest(*inputs), \
        f"{key}: the oracle made other inputs than were recorded; re-record: python tests/golden/make_gl_reference_golden.py"
    return z


def recorded(z, name, oracle_image):
    """GL image `name`, rebuilt bit for bit from its stored XOR with the oracle's image of the same pass -- after checking
    that `oracle_image` is the very image the XOR was taken against, so what comes back is the recorded GL output"""
    oracle_image = np.ascontiguousarray(oracle_image)
    assert digest(oracle_image) == str(z[name + "_oracle_digest"]), \
        f"{name}: the oracle's image is not the recorded one; re-record: python tests/golden/make_gl_reference_golden.py"
    return (oracle_image.view(np.uint32) ^ z[name + "_xor"]).view(oracle_image.dtype)


@pytest.fixture(scope="module")
def gl():
    from oracle import glref
    if not glref.available():
        pytest.skip("no software GL (Mesa swrast_dri.so + DRI headers) on this machine")
    return glref


@pytest.fixture(scope="module")
def scene(oracle_lib):
    """a map after 12 scans + the quads K4's vertex / geometry stage emits for it from the current pose"""
    p = params_with_size(W)
    op = oracle_lib.OraclePipeline(p, threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(12):
        pts, lab, prob, _ = get_scan(k, W, True)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    ctx = op.ctx
    pose = op.pose().astype(np.float32).astype(np.float64)
    ts = ctx.map_timestamp()
    emitted, corners, pn = ctx.debug_render_quads(pose, 0.0, 1, ts - 100)
    ids = np.nonzero(emitted)[0].astype(np.uint32)
    assert ids.size > 30000
    return dict(p=p, op=op, ctx=ctx, pose=pose, ts=ts, corners=corners[ids], ids=ids)


def test_the_context_is_a_real_opengl(gl):
    info = gl.limits()
    assert info["version"].startswith(("3.3", "4.")) and "Core Profile" in info["version"]
    assert info["subpixel_bits"] == 8  # the 1/256-pixel snapping o_map.c assumes (GL requires >= 4)


def edge_distance(c, i, j):
    """distance (in 1/256 pixel) of pixel centre (i, j) from the nearest OUTER edge of quad c[4, 3]"""
    x = np.floor((c[:, 0] * np.float32(W)).astype(np.float32) * np.float32(256.0) + np.float32(0.5)).astype(np.int64)
    y = np.floor((c[:, 1] * np.float32(H)).astype(np.float32) * np.float32(256.0) + np.float32(0.5)).astype(np.int64)
    px, py = 256 * i + 128, 256 * j + 128
    best = np.inf
    for s, t in ((0, 1), (1, 3), (3, 2), (2, 0)):
        w = (x[t] - x[s]) * (py - y[s]) - (y[t] - y[s]) * (px - x[s])
        best = min(best, abs(float(w)) / max(np.hypot(float(x[t] - x[s]), float(y[t] - y[s])), 1e-9))
    return best


def test_triangle_coverage_rule(gl, scene):
    """which pixel centres a quad (two strip triangles) covers: 65 k quads of a real map, no discard, no depth test (the
    last primitive that covers a pixel owns it).  GL and o_raster_tri must agree on every pixel whose centre is not
    within one sub-pixel unit of an outer quad edge -- there the specification lets the implementation decide."""
    cn, ids = scene["corners"], scene["ids"]
    want = scene["ctx"].debug_raster_quads(W, H, cn, ids, use_disc=False, use_depth=False)
    got, _ = gl.QuadRaster(W, H).run(cn, ids, disc=False, depth_test=False)
    assert (want >= 0).sum() > 30000
    row = {int(v): k for k, v in enumerate(ids)}
    jj, ii = np.nonzero(want != got)
    assert jj.size <= 0.0005 * W * H, f"{jj.size} pixels differ"
    for j, i in zip(jj, ii):
        d = min(edge_distance(cn[row[int(q)]], i, j) for q in (want[j, i], got[j, i]) if q >= 0)
        assert d <= 1.0, f"pixel ({i}, {j}): {want[j, i]} vs {got[j, i]}, {d:.2f}/256 px from the nearest edge"


def test_depth_quantisation_rule(gl, oracle_lib):
    """GL_DEPTH24_STENCIL8 + GL_LESS: pairs of pixel-sized quads a few 2^-25 apart in depth, second drawn over first.
    Which one survives depends on how z_w is rounded to 24 bits: o_depth24 (nearest-even of the fp32 product, on
    z_w = 0.5 (2 z01 - 1) + 0.5 as shader and viewport form it) must predict every one of the 16384 outcomes."""
    w, h = 256, 64
    n = w * h
    rng = np.random.default_rng(5)
    za = rng.uniform(0.02, 0.98, n).astype(np.float32)
    zb = (za + (rng.integers(-3, 4, n) * 2.0 ** -25 + rng.uniform(-1, 1, n) * 2.0 ** -26).astype(np.float32)).astype(np.float32)
    ii, jj = (a.ravel() for a in np.meshgrid(np.arange(w), np.arange(h)))

    def squares(z):
        c = np.zeros((n, 4, 3), dtype=np.float32)
        x0, x1, y0, y1 = (ii + 0.25) / w, (ii + 0.75) / w, (jj + 0.25) / h, (jj + 0.75) / h
        for k, (x, y) in enumerate(((x0, y0), (x1, y0), (x0, y1), (x1, y1))):
            c[:, k] = np.stack([x, y, z], 1)
        return c
    cn = np.concatenate([squares(za), squares(zb)])
    win, zwin = gl.QuadRaster(w, h).run(cn, np.arange(2 * n), disc=False, flat_z=True)
    second_wins = win.ravel() >= n

    def zw(z):
        return (np.float32(0.5) * (np.float32(2.0) * z - np.float32(1.0)) + np.float32(0.5)).astype(np.float32)
    ora = oracle_lib.Oracle(params_with_size(W))
    da, db = ora.debug_depth24(zw(za)), ora.debug_depth24(zw(zb))
    assert np.array_equal(db < da, second_wins)
    assert 0.25 < second_wins.mean() < 0.6 and (da == db).mean() > 0.1  # the test does probe ties and near-ties
    assert np.array_equal(zwin.ravel(), zw(np.where(second_wins, zb, za)))  # gl_FragCoord.z is z_w, not z01
    # GL_LEQUAL (render_composed, SurfelMap.cpp:1126): on equal 24-bit depth the LATER primitive replaces the earlier one
    win_le, _ = gl.QuadRaster(w, h).run(cn, np.arange(2 * n), disc=False, flat_z=True, depth_func="LEQUAL")
    assert np.array_equal(db <= da, win_le.ravel() >= n)
    assert (win_le.ravel() >= n).sum() > second_wins.sum()  # the ties changed hands


def test_quads_with_disc_and_depth_test(gl, scene):
    """the same quads with the disc test of render_surfels.frag:22 and the depth test: now the interpolated texture
    coordinate and depth of a fragment matter, which llvmpipe forms from plane equations and o_raster_tri from
    barycentrics of the snapped vertices -- borderline fragments (|tc|^2 ~ 1, depths a few 2^-24 apart) may fall
    either way: measured 0.3 %; bound 1 %."""
    cn, ids = scene["corners"], scene["ids"]
    want = scene["ctx"].debug_raster_quads(W, H, cn, ids, use_disc=True, use_depth=True)
    got, _ = gl.QuadRaster(W, H).run(cn, ids, disc=True)
    assert np.mean(want != got) < 0.01 and np.mean((want >= 0) != (got >= 0)) < 0.004


def test_reference_render_shaders_in_gl(scene):
    """SurfelMap::render_active through the reference's own GLSL in llvmpipe (recorded) against the oracle's rendering of
    the same map: the same surfel wins >= 97 % of the texels (measured 98.1 %; the rest are silhouette texels where the
    driver's atan / asin / FMA choices move a corner across a pixel centre or a disc boundary)."""
    p, ctx, pose, ts = scene["p"], scene["ctx"], scene["pose"], scene["ts"]
    z = gl_golden("scene", ctx.map_surfels(), ctx.map_poses(ts + 1), pose, np.int64(ts))
    out = ctx.frame(model=True)
    ctx.map_render(pose, pose, 0.0, out)
    o = [ctx.map_frame(1).map(m) for m in range(3)]
    g = [recorded(z, name, o[m]) for m, name in enumerate(("render_vertex", "render_normal", "render_semantic"))]
    va, vb = o[0][..., 3] > 0.5, g[0][..., 3] > 0.5
    assert va.sum() > 30000
    same = va & vb & np.all(np.abs(o[0] - g[0]) <= 1e-4 * (1.0 + np.abs(o[0])), axis=-1)
    assert same.sum() >= 0.97 * max(va.sum(), vb.sum())
    assert (va != vb).sum() <= 0.015 * va.sum()
    # where the same surfel won, normal and semantic agree as well (flat attributes of the winner)
    assert np.all(np.abs(o[1][same] - g[1][same]) <= 1e-4) and np.array_equal(o[2][same], g[2][same])


def test_committed_gl_golden_is_reproduced_by_the_oracle():
    """tests/golden/gl_render_450x32.npz (made by tests/golden/make_gl_golden.py with llvmpipe; no GL needed here): the
    oracle renders the stored map and agrees with the stored GL images on >= 97 % of the texels -- the bar the GPU suite
    applies to the HIP path with the same file (tests/test_gpu_gl_golden.py)."""
    from oracle import pyoracle
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "gl_render_450x32.npz"))
    p = params_with_size(int(z["W"]), int(z["H"]))
    ora = pyoracle.Oracle(p)
    ora.map_upload(z["surfels"], int(z["timestamp"]))
    ora.map_update_poses(z["poses"].reshape(-1, 4, 4).transpose(0, 2, 1))
    ora.map_render_active(z["pose"], float(z["conf_threshold"]))
    v = ora.map_frame(1).map(0)
    va, vb = v[..., 3] > 0.5, z["gl_vertex"][..., 3] > 0.5
    same = va & vb & np.all(np.abs(v - z["gl_vertex"]) <= 1e-4 * (1.0 + np.abs(v)), axis=-1)
    assert vb.sum() > 5000 and same.sum() >= 0.97 * max(va.sum(), vb.sum())


def test_reference_jacobian_shaders_in_gl(oracle_lib):
    """Frame2Model::jacobianProducts through the reference's own Frame2Model_jacobians.{vert,geom,frag} in llvmpipe (recorded):
    LINEAR rectangle samplers with CLAMP_TO_BORDER on all six maps, 16 points per geometry-shader invocation blended
    (GL_ONE, GL_ONE) into the 2 x 8 RGB32F target, unpacked as Frame2Model.cpp:214-227.  This pins the conventions the
    oracle's K6 rests on -- texel centres at integer + 0.5, the four-tap weights, border colour 0, the layout of the 48
    floats, Huber from iteration 0 / Tukey from 1 -- against a real GL.  The sums are fp32 and order dependent in GL
    (exact 2^-28 fixed point in the oracle) and a handful of pairs sit on a gate, so: counters within 0.5 %, F within
    1 %, the diagonal of J^T W J within 3e-3 relative (measured 1.5e-3: three of 7797 pairs fall the other side of a gate)."""
    p = params_with_size(W)
    ora = oracle_lib.Oracle(p)
    frames = []
    for k in range(2):
        pts, lab, prob, _ = get_scan(k, W, True)
        frames.append(ora.preprocess(pts, lab, prob, k, ora.frame()))
    T = np.eye(4)
    T[0, 3] = 0.9
    z = gl_golden("jacobian", *[frames[0].map(m) for m in range(3)], *[frames[1].map(m) for m in range(3)], T)
    for iteration in (0, 1):
        b = z["jacobian_b"][iteration]
        F, acc, JtJ, Jtr, st = ora.jacobian_products(frames[1], frames[0], T, iteration)
        valid, Fg, outlier, invalid = b[42], b[43], b[44], b[46]
        assert st.valid > 5000
        assert abs(valid - st.valid) <= 0.005 * st.valid and abs(outlier - st.outlier) <= 0.005 * st.valid
        assert valid + invalid == W * H and abs(invalid - st.invalid) <= 0.005 * st.valid
        assert abs(Fg - F) <= 0.01 * F
        JtJ_gl = b[:36].reshape(6, 6)
        assert np.allclose(np.diag(JtJ_gl), np.diag(JtJ), rtol=3e-3)
        assert np.allclose(JtJ_gl, JtJ, rtol=0, atol=2e-4 * np.abs(JtJ).max())
        assert np.allclose(b[36:42], Jtr, rtol=0, atol=0.01 * np.abs(Jtr).max())


def test_reference_vertexmap_shaders_in_gl(oracle_lib):
    """Preprocessing::process, first pass, through the reference's gen_vertexmap.{vert,frag} in llvmpipe (recorded): size-1 points,
    two colour attachments, DEPTH24_STENCIL8 + GL_LESS, the label / prob attribute pointers 4 / 5 floats into their
    buffers (quirk B-1).  The synthetic scanner fires at exact azimuth steps, so many points sit ON a texel border and the
    driver's atan decides the column: >= 98 % of the 57 600 texels are bit-equal to the oracle's vertex map (measured
    98.8 %), and both validity counts agree to 0.5 % -- before and after the initialisation period (isfirst)."""
    p = params_with_size(W)
    ora = oracle_lib.Oracle(p)
    pts, lab, prob, _ = get_scan(3, W, True)
    z = gl_golden("vertexmap", pts, lab, prob)
    for i, ts in enumerate((3, 20)):
        frame = ora.preprocess(pts, lab, prob, ts, ora.frame())  # owns the memory map(0) views: keep it alive
        ov = frame.map(0)
        gv = recorded(z, f"vertexmap_{i}", ov)
        same = np.all(ov.view(np.uint32) == gv.view(np.uint32), axis=-1)
        assert same.mean() >= 0.98
        assert abs(int((ov[..., 3] > 0.5).sum()) - int((gv[..., 3] > 0.5).sum())) <= 0.005 * (ov[..., 3] > 0.5).sum()


def test_reference_indexmap_shaders_in_gl(oracle_lib):
    """SurfelMap::renderIndexmap (K7) through the reference's gen_indexmap.{vert,frag} in llvmpipe (recorded) against the index map
    the oracle's update made of the same map from the same pose: size-1 points at texel centres, GL_LESS on 24-bit depth,
    the earlier surfel on equal depth.  The shader snaps to texel centres itself, so only the driver's atan / asin can
    move a surfel to the neighbouring texel: >= 97 % of the texels name the same surfel (measured 99.3 % of 57 600)."""
    p = params_with_size(W)
    op = oracle_lib.OraclePipeline(p, threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(12):
        pts, lab, prob, _ = get_scan(k, W, True)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    ctx = op.ctx
    before, ts = ctx.map_surfels().copy(), ctx.map_timestamp()
    pts, lab, prob, _ = get_scan(12, W, True)
    op.process_scan(pts, lab, prob, fixed_iterations=10)
    want = ctx.map_index_map()  # K7 of that update: the map as it was, from the pose the update was given
    pose = op.pose().astype(np.float32)
    R, t = pose[:3, :3], pose[:3, 3]
    inv = np.eye(4, dtype=np.float32)  # the rigid inverse in float, as the HIP path and the oracle form it
    inv[:3, :3] = R.T
    inv[:3, 3] = -(R.T @ t)
    got = recorded(gl_golden("indexmap", before, ctx.map_poses(ts + 1), pose, inv), "indexmap", want)
    assert want.shape == got.shape and (want > 0).sum() > 20000
    same = want == got
    assert same.mean() >= 0.97, same.mean()
    assert abs(int((want > 0).sum()) - int((got > 0).sum())) <= 0.01 * (want > 0).sum()
    assert got.max() <= before.shape[0]


def test_reference_normal_and_floodfill_shaders_in_gl(gl):
    """Preprocessing::process, passes 2 and 3, through the reference's quad.geom + gen_normalmap.frag / floodfill.frag in
    llvmpipe against THE SAME shader text compiled by g++ over oracle/glsl_compat.hpp (the pin of the oracle's K2 / K3,
    tests/test_ref_shaders.py), both fed the vertex map and raw labels GL's own pass 1 made: what is compared is the
    emulation's reading of sampler2DRect with NEAREST + CLAMP_TO_BORDER, of the interpolated texCoords of the full-screen
    quad and of the seam wrap.  Validity flags, eroded and refined labels are equal everywhere; a normal may differ in
    the last ulps (the driver's normalize / cross): measured 75 % of the 57 600 normals bit-equal, the rest within 1.8e-7;
    1162 labels are changed by the flood fill, identically."""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    p = params_with_size(W)
    pts, lab, prob, _ = get_scan(5, W, True)
    gv, gs = gl.VertexMap(p).run(pts, lab, prob, 20)
    gn, ge, gr = gl.NormalsLabels(p).run(gv, gs)
    rn, re_, rr = pyref.Ref(p).normals_and_labels(gv, gs)
    assert (gv[..., 3] > 0.5).sum() > 30000 and (rn[..., 3] > 0.5).sum() > 25000
    assert np.array_equal(gn[..., 3], rn[..., 3]), "normal validity"
    assert np.array_equal(ge, re_), "eroded labels"
    assert np.array_equal(gr, rr), "refined labels"
    assert np.abs(gn[..., :3] - rn[..., :3]).max() <= 2e-6
    assert np.mean(np.all(gn.view(np.uint32) == rn.view(np.uint32), axis=-1)) >= 0.5


def test_reference_update_shaders_with_transform_feedback_in_gl(gl, oracle_lib):
    """SurfelMap::updateSurfels, first draw (K9), through the reference's update_surfels.{vert,geom,frag} in llvmpipe with
    REAL transform feedback, against the same shader text compiled by g++ (oracle/pyref.py, the pin of the oracle's K9) on
    identical inputs: the map before the update of scan 12, the oracle's index map and radius map, the frame's three maps,
    the reference's uniform values.  Pinned here: feedback order = draw order with the dropped primitives closed up, the
    interleaved 64-byte record, MIN NEAREST / MAG LINEAR sampler objects at vertex-stage fetches, texelFetch on the
    pose buffer, the rasterised integration mask.  Measured: 101 255 records on both sides out of 102 453
    surfels, 4 surfels survive on one side only, 99.88 % of the common records agree to 1e-4 (76.6 % bit for bit; the rest
    are borderline associations where the driver's exp / log / atan / acos differ from include/suma_detmath.h in the last
    ulps), 99.88 % of the mask texels agree."""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    p = params_with_size(W)
    op = oracle_lib.OraclePipeline(p, threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(12):
        pts, lab, prob, _ = get_scan(k, W, True)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    ora = op.ctx
    before, t = ora.map_surfels().copy(), 12
    pts, lab, prob, _ = get_scan(t, W, True)
    op.process_scan(pts, lab, prob, fixed_iterations=10)
    cur = op.frame(0)
    frame = (cur.vertex.copy(), cur.normal.copy(), cur.semantic.copy())
    poses = ora.map_poses(t + 2)
    pose = poses[t].reshape(4, 4).T  # poses_[timestamp_] = pose, SurfelMap.cpp:494
    o_idx, o_rc = ora.map_index_map().astype(np.float32), ora.map_radius_conf()
    ref = pyref.Ref(p)
    want, want_mask, want_src = ref.update(before, poses, pose, t, frame, o_rc, o_idx, sources=True)
    got, got_mask, got_src = gl.SurfelUpdate(p, tag_sources=True).run(ref.update_uniforms(pose, t), before, poses, frame, o_rc, o_idx)
    plain, _ = gl.SurfelUpdate(p).run(ref.update_uniforms(pose, t), before, poses, frame, o_rc, o_idx)
    assert np.array_equal(plain.view(np.uint32), got.view(np.uint32)), "the source tag must not change the records"
    want = want.view(np.float32).reshape(-1, 16)
    n = before.shape[0]
    assert n > 100_000 and 0 < want.shape[0] < n, "the update must drop some surfels"
    # feedback order = draw order, the dropped primitives closed up
    assert np.all(np.diff(got_src.astype(np.int64)) > 0) and np.all(np.diff(want_src.astype(np.int64)) > 0)
    kept_g, kept_w = np.zeros(n, bool), np.zeros(n, bool)
    kept_g[got_src], kept_w[want_src] = True, True
    assert (kept_g != kept_w).sum() <= 0.001 * n, f"{(kept_g != kept_w).sum()} surfels survive on one side only"
    both = kept_g & kept_w
    g_, w_ = got[both[got_src]], want[both[want_src]]
    ok = np.isfinite(w_).all(axis=1) & np.isfinite(g_).all(axis=1)  # the slerp NaN of identical normals
    assert ok.mean() > 0.99
    # word 9 is the display colour, pack(vec3) = int(round(c * 255)) per channel (color.glsl): 0.3 * 255 = 76.5 and
    # 0.7 * 255 = 178.5 are ties and GLSL leaves the direction of round() at .5 to the implementation.  llvmpipe rounds to
    # even -- this test found rounds 1-3 of the repository rounding away from zero (C roundf) in include/suma_detmath.h;
    # now both sides pack grey to 0x4C4C4C and green to 0x00B200
    assert set(np.unique(g_[:, 9]).tolist()) <= {5000268.0, 45568.0, 16711935.0, 65535.0, 16711680.0}
    close = np.all(np.abs(g_[ok] - w_[ok]) <= 1e-4 * (1.0 + np.abs(w_[ok])), axis=1)
    exact = np.all(g_[ok].view(np.uint32) == w_[ok].view(np.uint32), axis=1)
    mask_same = np.mean((got_mask > 0.5) == (want_mask[..., 0] > 0.5))
    print(f"K9 in GL: {got.shape[0]} / {want.shape[0]} records of {n}, one-sided {int((kept_g != kept_w).sum())}, "
          f"close {close.mean():.5f}, bit-equal {exact.mean():.5f}, mask {mask_same:.5f}")
    assert close.mean() >= 0.995, close.mean()
    assert exact.mean() >= 0.5, exact.mean()
    assert mask_same >= 0.998


def test_reference_generate_shaders_with_transform_feedback_in_gl(gl, oracle_lib):
    """SurfelMap::updateSurfels, second draw (K10), through the reference's gen_surfels.{vert,geom,frag} in llvmpipe --
    one point per data texel in the x-major order of vbo_img_coords_, GL_RASTERIZER_DISCARD, transform feedback -- against
    the same shader text compiled by g++ on identical inputs (the frame, the oracle's radius map and integration mask of
    scan 12).  The same texels produce a surfel, in the same order; records agree to the last ulps of the driver's
    normalize / asin / atan (the re-centred position).  Measured: 7 046 new surfels on both sides, all within 1e-5, 66 %
    bit for bit, stamps / colour / weight / labels equal."""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    p = params_with_size(W)
    op = oracle_lib.OraclePipeline(p, threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(13):
        pts, lab, prob, _ = get_scan(k, W, True)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    ora, t = op.ctx, 12
    cur = op.frame(0)
    frame = (cur.vertex.copy(), cur.normal.copy(), cur.semantic.copy())
    pose = ora.map_poses(t + 2)[t].reshape(4, 4).T
    o_rc = ora.map_radius_conf()
    mask4 = np.zeros((H, W, 4), np.float32)
    mask4[:, :, 0] = ora.map_integrated() != 0
    ref = pyref.Ref(p)
    want = ref.generate(frame, o_rc, mask4, pose, t).view(np.float32).reshape(-1, 16)
    got = gl.SurfelGenerate(p).run(ref.generate_uniforms(pose, t), frame, o_rc, mask4)
    assert want.shape[0] > 3000
    assert got.shape == want.shape, f"transform feedback wrote {got.shape[0]} new surfels, the compiled shaders {want.shape[0]}"
    exact = np.all(got.view(np.uint32) == want.view(np.uint32), axis=1)
    close = np.all(np.abs(got - want) <= 1e-5 * (1.0 + np.abs(want)), axis=1)
    print(f"K10 in GL: {got.shape[0]} new surfels, close {close.mean():.5f}, bit-equal {exact.mean():.5f}")
    assert close.all()
    assert exact.mean() >= 0.5
    assert np.array_equal(got[:, 8:16].view(np.uint32), want[:, 8:16].view(np.uint32)), "stamps, colour, weight, labels"


def test_reference_copy_and_extract_shaders_with_transform_feedback_in_gl(gl, oracle_lib):
    """SurfelMap::copySurfels (K11) and SurfelMap::extractSurfels (K12) through the reference's copy_surfels.vert /
    extract_surfels.vert + copy_surfels.geom in llvmpipe (transform feedback across two draws, rasteriser discard) on a
    map with small submaps, against the same shader text compiled by g++: the records pass through untouched, so the two
    outputs must be the same bytes -- what is pinned is the area predicate on the pose-table product, the order of the
    two draws in one feedback object, and the feedback layout."""
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    p = params_with_size(W, submap_extent=4.0, submap_dimension=2)
    op = oracle_lib.OraclePipeline(p, threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(0, 40, 5):  # 5.5 m per step: the window shifts, tiles leave
        pts, lab, prob, _ = get_scan(k, W, True)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    ora = op.ctx
    ts = ora.map_timestamp()
    poses = ora.map_poses(ts + 1)
    upd, new = ora.map_updated_surfels(), ora.map_data_surfels()
    assert upd.shape[0] > 20000 and new.shape[0] > 1000 and ora.map_submap_origin() != (0, 0)
    ref = pyref.Ref(p)
    f32 = np.float32
    oi, oj = ora.map_submap_origin()
    center = (f32(2.0 * oi * p.submap_extent), f32(2.0 * oj * p.submap_extent))
    for extent in (f32(2.0) * f32(p.submap_dimension) * f32(p.submap_extent) + f32(p.submap_extent), f32(6.0)):
        want = ref.copy(upd, new, poses, center, extent).view(np.float32).reshape(-1, 16)
        got = gl.SurfelFilter("copy_surfels.vert").run([upd, new], poses, center, extent)
        assert 0 < want.shape[0] < upd.shape[0] + new.shape[0], "the area must drop something"
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"K11, extent {extent}"
    after = ora.map_surfels()
    hits = 0
    for di in (-3, -2, -1, 0, 1):
        c = (f32(2.0 * (oi + di) * p.submap_extent), f32(2.0 * oj * p.submap_extent))
        want = ref.extract(after, poses, c, p.submap_extent).view(np.float32).reshape(-1, 16)
        got = gl.SurfelFilter("extract_surfels.vert").run([after], poses, c, p.submap_extent)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"K12, tile offset {di}"
        hits += want.shape[0]
    assert hits > 1000


def test_reference_radius_and_compose_shaders_in_gl(gl, oracle_lib):
    """K8 (init_radiusConf.{vert,frag}: a point per data texel, two attachments) and K5 (render_compose.frag through
    quad.geom, the map's MIN NEAREST / MAG LINEAR sampler at a 1:1 mapping) in llvmpipe against the same shader text
    compiled by g++ on the oracle's maps: the validity flags and every selected texel are equal; radii agree to the last
    ulps of the driver's division (measured: 96 % of the radii bit for bit)."""
    import math
    from oracle import pyref
    if not pyref.available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    p = params_with_size(W)
    op = oracle_lib.OraclePipeline(p, threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(8):
        pts, lab, prob, _ = get_scan(k, W, True)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    ref = pyref.Ref(p)
    cur = op.frame(0)
    f32 = np.float32
    want = ref.radius_conf(cur.vertex, cur.normal)
    uni = dict(fov_up=float(abs(f32(p.data_fov_up))), fov_down=float(abs(f32(p.data_fov_down))), min_depth=float(f32(p.min_depth)),
               max_depth=float(f32(p.max_depth)), pixel_size=float(ref.pixel_size), confidence_mode=int(p.confidence_mode),
               min_radius=float(f32(p.min_radius)), max_radius=float(f32(p.max_radius)),
               angle_thresh=float(f32(math.cos(float(f32(float(f32(p.max_angle)) * math.pi / 180.0))))))
    got, _ = gl.RadiusConfidence(p).run(uni, cur.vertex, cur.normal)
    assert (want[..., 3] > 0.5).sum() > 15000
    assert np.array_equal(got[..., 1:], want[..., 1:]), "K8 confidence / validity channels"
    assert np.abs(got[..., 0] - want[..., 0]).max() <= 1e-6 * (1.0 + np.abs(want[..., 0]).max())
    k8_exact = float(np.mean(got[..., 0].view(np.uint32) == want[..., 0].view(np.uint32)))
    # K5 on the two map frames of a render from a pose 8 scans back: old and new surfels both present
    ora = op.ctx
    pose = op.pose().astype(np.float32).astype(np.float64)
    out = ora.frame(model=True)
    ora.map_render(pose, pose, -2.0, out)
    old = [ora.map_frame(0).map(m).copy() for m in range(3)]
    new = [ora.map_frame(1).map(m).copy() for m in range(3)]
    old[0][::3, ::5] = new[0][::3, ::5] + np.float32(0.01)  # old frames are empty outside loop closures: plant some texels
    old[0][::3, ::5, 3] = 1.0
    old[1][::3, ::5] = new[1][::3, ::5]
    old[2][::3, ::5] = new[2][::3, ::5]
    wantc = ref.compose(old, new)
    gotc = gl.Compose(p).run(old, new)
    for m in range(3):
        assert np.array_equal(gotc[m].view(np.uint32), wantc[m].view(np.uint32)), f"K5 attachment {m}"
    print(f"K8 in GL: radius bit-equal on {k8_exact:.4f} of the texels; K5 equal on every texel")



def test_reference_render_composed_in_gl(scene, oracle_lib):
    """SurfelMap::render_composed (SurfelMap.cpp:1116-1165: GL_LEQUAL, the old surfels from pose_old, then -- without
    clearing -- the new ones from pose_new into the same depth buffer) through the reference's shaders in llvmpipe (recorded) against
    the oracle's composed frame.  The 12-scan map is given timestamp 106, so that timestamp_ - composeSurfelAge_ = 6 makes
    the surfels of scans 0-5 "old" and those of scans 6-11 "new" and both passes draw: >= 97 % of the texels carry the
    same surfel."""
    p, ctx, pose, ts = scene["p"], scene["ctx"], scene["pose"], 106
    surfels, poses = ctx.map_surfels(), ctx.map_poses(int(scene["ts"]) + 1)
    z = gl_golden("scene", surfels, poses, pose, np.int64(scene["ts"]))
    ora = oracle_lib.Oracle(p)
    ora.map_upload(surfels, ts)
    ora.map_update_poses(poses.reshape(-1, 4, 4).transpose(0, 2, 1))
    pose_old = pose.copy()
    pose_old[0, 3] -= 0.4  # a loop-closure candidate seen from a slightly different place
    ora.map_render_composed(pose_old, pose, 0.0)
    want = [ora.map_frame(2).map(m) for m in range(2)]
    old_only = int(z["composed_old_only_texels"])  # texels the old pass alone drew
    got = [recorded(z, "composed_vertex", want[0]), recorded(z, "composed_normal", want[1])]
    va, vb = want[0][..., 3] > 0.5, got[0][..., 3] > 0.5
    assert va.sum() > 30000 and old_only > 5000 and vb.sum() > old_only + 5000, "both passes must draw"
    same = va & vb & np.all(np.abs(want[0] - got[0]) <= 1e-4 * (1.0 + np.abs(want[0])), axis=-1)
    print(f"render_composed in GL: {same.sum()} of {max(va.sum(), vb.sum())} texels carry the same surfel")
    assert same.sum() >= 0.97 * max(va.sum(), vb.sum())
    assert np.all(np.abs(want[1][same] - got[1][same]) <= 1e-4)
