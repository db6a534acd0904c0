#!/usr/bin/env python
"""Writes tests/golden/gl_draw_<W>x<H>.npz: what the reference's own draw_surfels.{vert,geom,frag} draw in a real GL
(Mesa llvmpipe, tests/gl_draw_ref.py) for a synthetic surfel map seen from a perspective camera inside it -- near-plane
clipping active -- in colour modes 0 (Phong), 2 (normals) and 5 (semantic), with everything the drawing took: the
surfel records, the pose table (row-major), the camera (mvp row-major, view position) and the colour map.  The GPU machine
has neither Mesa nor the reference tree; tests/test_gpu_draw.py reads this file instead.
    python tests/golden/make_gl_draw_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import draw_common as dc  # noqa: E402
import gl_draw_ref  # noqa: E402
from semantic_suma_amd import kitti  # noqa: E402

W, H = 256, 160
MODES = (0, 2, 5)


def main():
    if not gl_draw_ref.available():
        sys.exit("needs Mesa llvmpipe and the reference's shader tree")
    s, poses = dc.planar_map(6000, seed=11, extent=15.0)
    mvp, eye = dc.inside_camera([0.5, 0.2, -0.8], 0.3, W, H)
    out = dict(surfels=s.view(np.uint8).reshape(-1, 64), poses=poses, mvp=mvp.astype(np.float64),
               view_pos=np.asarray(eye, dtype=np.float64), color_map=kitti.semantic_color_map(),
               size=np.array([W, H], dtype=np.int32), modes=np.array(MODES, dtype=np.int32))
    for m in MODES:
        out[f"gl_mode{m}"] = gl_draw_ref.gl_draw(s, poses, dc.params(mvp, eye, W, H, m))
    path = os.path.join(HERE, f"gl_draw_{W}x{H}.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
