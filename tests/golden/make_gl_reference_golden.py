#!/usr/bin/env python
"""Generates tests/golden/gl_reference_900x64.npz: what the reference's own GLSL, run by Mesa llvmpipe through
oracle/glref.py, produces on the inputs of the five comparisons in tests/test_gl_reference.py that need nothing but GL
on the reference side -- render_active (K4), render_composed, Frame2Model::jacobianProducts (K6), the vertex map pass of
Preprocessing::process (K1) and renderIndexmap (K7).  The inputs themselves are made by the oracle in the tests, so only
their SHA-256 is stored: a test that finds other inputs asks for a re-recording instead of comparing against GL output
for a different map.  Each GL image is stored as the XOR of its bits with the oracle's image of the same pass, which it
matches on nearly every texel, together with the SHA-256 of that oracle image: a test rebuilds the GL image bit for bit
only after checking that the oracle gave it the same image (tests/test_gl_reference.py::recorded).
The reference's sources and Mesa are only needed here, at generation time.  Run from the repo root:
    python tests/golden/make_gl_reference_golden.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import glref, pyoracle  # noqa: E402
from semantic_suma_amd import synth  # noqa: E402
from semantic_suma_amd.types import params_with_size  # noqa: E402

W, H = 900, 64


def digest(*arrays):
    """SHA-256 of the bytes of the arrays, in order (the same function as tests/test_gl_reference.py::digest)"""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def store(name, gl_image, oracle_image):
    """GL image `name` as its XOR with the oracle's image of the same pass, plus the digest of the latter"""
    out[name + "_oracle_digest"] = digest(oracle_image)
    out[name + "_xor"] = np.ascontiguousarray(gl_image).view(np.uint32) ^ np.ascontiguousarray(oracle_image).view(np.uint32)


def scan(k):
    return synth.generate_scan(k, n_azimuth=W, height=H, semantics=True)


def pipeline(n):
    op = pyoracle.OraclePipeline(params_with_size(W), threads=max(1, min(8, os.cpu_count() or 1)))
    for k in range(n):
        pts, lab, prob, _ = scan(k)
        op.process_scan(pts, lab, prob, fixed_iterations=10)
    return op


assert glref.available(), "needs Mesa (swrast_dri.so + DRI headers)"
p = params_with_size(W)
out = {"W": W, "H": H, "gl_version": glref.limits()["version"], "gl_renderer": glref.limits()["renderer"]}

# the 12-scan map of the `scene` fixture: render_active and render_composed
op = pipeline(12)
ctx = op.ctx
pose = op.pose().astype(np.float32).astype(np.float64)
ts = ctx.map_timestamp()
surfels, poses = ctx.map_surfels(), ctx.map_poses(ts + 1)
out["scene_digest"] = digest(surfels, poses, pose, np.int64(ts))
ctx.map_render(pose, pose, 0.0, ctx.frame(model=True))
R = glref.SurfelRenderer(p)
g = R.render(surfels, poses.reshape(-1, 16), pose, 0.0, ts - 100, False)
for m, name in enumerate(("render_vertex", "render_normal", "render_semantic")):
    store(name, g[m], ctx.map_frame(1).map(m))
ora = pyoracle.Oracle(p)  # render_composed of the same map stamped 106: scans 0-5 "old", 6-11 "new"
ora.map_upload(surfels, 106)
ora.map_update_poses(poses.reshape(-1, 4, 4).transpose(0, 2, 1))
pose_old = pose.copy()
pose_old[0, 3] -= 0.4
ora.map_render_composed(pose_old, pose, 0.0)
tg = R.render_pass(surfels, poses.reshape(-1, 16), pose_old, 0.0, 106 - 100, True, depth_func="LEQUAL")
out["composed_old_only_texels"] = int((tg[0].read()[..., 3] > 0.5).sum())
tg = R.render_pass(surfels, poses.reshape(-1, 16), pose, 0.0, 106 - 100, False, depth_func="LEQUAL", targets=tg,
                   clear_first=False)
for m, name in enumerate(("composed_vertex", "composed_normal")):
    store(name, tg[m].read(), ora.map_frame(2).map(m))

# Frame2Model_jacobians: frames of scans 0 and 1, iterations 0 and 1 (48 floats each, stored as they are)
ora = pyoracle.Oracle(p)
frames = []
for k in range(2):
    pts, lab, prob, _ = scan(k)
    frames.append(ora.preprocess(pts, lab, prob, k, ora.frame()))
maps = [[f.map(m).copy() for m in range(3)] for f in frames]
T = np.eye(4)
T[0, 3] = 0.9
out["jacobian_digest"] = digest(*maps[0], *maps[1], T)
J = glref.Jacobians(p)
out["jacobian_b"] = np.stack([J.run(maps[1], maps[0], T, it) for it in (0, 1)])

# gen_vertexmap: scan 3 at timestamps 3 and 20
pts, lab, prob, _ = scan(3)
out["vertexmap_digest"] = digest(pts, lab, prob)
V = glref.VertexMap(p)
ora = pyoracle.Oracle(p)
for i, t in enumerate((3, 20)):
    gv = V.run(pts, lab, prob, t)[0]
    frame = ora.preprocess(pts, lab, prob, t, ora.frame())
    store(f"vertexmap_{i}", gv, frame.map(0))

# gen_indexmap: the map before the update of scan 12, from the pose that update was given
op = pipeline(12)
ctx = op.ctx
before, ts = ctx.map_surfels().copy(), ctx.map_timestamp()
pts, lab, prob, _ = scan(12)
op.process_scan(pts, lab, prob, fixed_iterations=10)
pose = op.pose().astype(np.float32)
Rt, t = pose[:3, :3], pose[:3, 3]
inv = np.eye(4, dtype=np.float32)
inv[:3, :3] = Rt.T
inv[:3, 3] = -(Rt.T @ t)
poses = ctx.map_poses(ts + 1)
out["indexmap_digest"] = digest(before, poses, pose, inv)
store("indexmap", glref.IndexMap(p).run(before, poses.reshape(-1, 16), pose, inv)[0], ctx.map_index_map())

path = os.path.join(ROOT, "tests", "golden", f"gl_reference_{W}x{H}.npz")
np.savez_compressed(path, **out)
print(f"{path}: {os.path.getsize(path) // 1024} KB, rendered by {out['gl_renderer']}")
