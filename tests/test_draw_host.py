"""SurfelMap::draw on the host: known answers of the arithmetic specification of csrc/k_draw.hip as restated in
tests/draw_shim.c (which the GPU tests compare the kernels with, bit for bit), the shim against the reference's own
draw_surfels.{vert,geom,frag} in a real GL (llvmpipe; skipped without Mesa or the reference tree), the layout of
suma_draw_params in C and ctypes, and the kernels' resources."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import draw_common as dc
from semantic_suma_amd import core, kitti
from semantic_suma_amd.types import DRAW_COLORS, SURFEL_DTYPE, DrawParams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WHITE = (255, 255, 255, 255)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return dc.build_shim(tmp_path_factory.mktemp("draw"))


def surfels(*rows):
    """rows of dicts -> SURFEL_DTYPE (normal (0, 0, 1), radius 1, confidence 20, label 40 unless given)"""
    s = np.zeros(len(rows), dtype=SURFEL_DTYPE)
    for k, r in enumerate(rows):
        d = dict(nz=1.0, radius=1.0, confidence=20.0, r=40 / 255.0, weight=1.0)
        d.update(r)
        for name, v in d.items():
            s[k][name] = v
    return s


POSES = np.eye(4, dtype=np.float32)[None]


def ortho_top(W=200, H=200, half=10.0):
    """GL camera = map frame (no ROSE2GL): looking down -z onto the plane z = 0, 0.1 map units a pixel"""
    return core.orthographic(-half, half, -half, half, -100.0, 100.0), np.array([0.0, 0.0, 50.0])


def draw(shim, s, mvp, eye, W, H, mode=2, **kw):
    return dc.shim_draw(shim, s, POSES, dc.params(mvp, eye, W, H, mode, **kw))


def test_camera_facing_disc_covers_its_analytic_area(shim):
    mvp, eye = ortho_top()
    r = 3.0
    rgba, ids = draw(shim, surfels(dict(x=0.013, y=0.027, radius=r)), mvp, eye, 200, 200)
    n = int((ids == 0).sum())
    rp = r / 0.1  # 30 pixels
    assert abs(n - math.pi * rp * rp) <= 2 * math.pi * rp, n
    # every covered pixel centre lies within the disc up to one pixel, every pixel one pixel inside it is covered
    j, i = np.mgrid[0:200, 0:200]
    d = np.hypot((i + 0.5) - 100 - 0.13, (j + 0.5) - 100 - 0.27)
    assert np.all(d[ids == 0] <= rp + 1.0) and np.all(ids[d <= rp - 1.0] == 0)
    assert np.all(rgba[ids < 0] == 255)


def test_nearer_surfel_wins_and_equal_depth_goes_to_the_lower_index(shim):
    mvp, eye = ortho_top()
    # the camera looks down -z: larger z is nearer.  The nearer one is drawn whatever its index.
    _, ids = draw(shim, surfels(dict(z=0.0), dict(z=1.0, x=0.5)), mvp, eye, 200, 200)
    assert ids[100, 104] == 1 and ids[100, 92] == 0
    _, ids = draw(shim, surfels(dict(z=1.0, x=0.5), dict(z=0.0)), mvp, eye, 200, 200)
    assert ids[100, 104] == 0 and ids[100, 92] == 1
    # equal depth (the same plane): GL_LESS with in-order primitives keeps the earlier one
    _, ids = draw(shim, surfels(dict(z=0.5), dict(z=0.5, x=0.5)), mvp, eye, 200, 200)
    assert ids[100, 104] == 0 and ids[100, 110] == 1
    _, ids = draw(shim, surfels(dict(z=0.5, x=0.5), dict(z=0.5)), mvp, eye, 200, 200)
    assert ids[100, 104] == 0 and ids[100, 92] == 1


def pixel_rays(W, H, fovy):
    j, i = np.mgrid[0:H, 0:W]
    t = math.tan(math.radians(fovy) / 2)
    return ((2 * (i + 0.5) / W - 1) * t * W / H, (2 * (j + 0.5) / H - 1) * t)


def test_surfel_straddling_the_near_plane_is_clipped(shim):
    W, H = 160, 120
    P = core.perspective(45.0, W / H, 0.1, 10000.0)
    eye = np.zeros(3)
    # a floor disc 1 below the eye (GL camera frame: looking down -z), centred on the eye: half of it lies behind
    s = surfels(dict(x=0.0, y=-1.0, z=0.0, nx=0.0, ny=1.0, nz=0.0, radius=5.0))
    corners = (C.c_float * 24)()
    dp = dc.params(P, eye, W, H, 2)
    shim.draw_shim_corners.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    assert shim.draw_shim_corners(C.byref(dp), s.ctypes.data, POSES.ctypes.data, 1, corners) == 1
    cv = np.array(corners).reshape(4, 6)
    near = cv[:, 2] + cv[:, 3]
    assert (near > 0).any() and (near < 0).any()
    _, ids = dc.shim_draw(shim, s, POSES, dp)
    # analytic: the ray of pixel (i, j) meets the floor y = -1 at distance 1 / -dy ahead; covered iff that point is in
    # front of the near plane and within the radius (one pixel of slack at the disc's rim and at the near cut)
    dx, dy = pixel_rays(W, H, 45.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dy < 0, -1.0 / dy, np.inf)
    px, pz = t * dx, -t
    rho = np.hypot(px, pz)
    inside = (dy < 0) & (rho < 5.0 * 0.97) & (-pz > 0.1 * 1.05)
    outside = (dy >= 0) | (rho > 5.0 * 1.03)
    assert (ids == 0).sum() > 0.3 * W * H / 2
    assert np.all(ids[inside] == 0), int((ids[inside] != 0).sum())
    assert np.all(ids[outside] == -1), int((ids[outside] != -1).sum())  # nothing wrapped into the upper half


def test_geometry_behind_the_camera_gives_no_pixels(shim):
    W, H = 160, 120
    P = core.perspective(45.0, W / H, 0.1, 10000.0)
    s = surfels(dict(z=5.0, radius=3.0), dict(z=0.05, radius=0.02))  # behind, and between the eye and the near plane
    _, ids = dc.shim_draw(shim, s, POSES, dc.params(P, np.zeros(3), W, H, 2))
    assert np.all(ids == -1)


def test_degenerate_normal_draws_nothing(shim):
    mvp, eye = ortho_top()
    # u = normalize(n.y - n.z, -n.x, n.x) has length 0 when n.x = 0 and n.y = n.z: the stated rule drops the surfel
    for n in ((0.0, 0.6, 0.6), (0.0, 0.0, 0.0), (0.0, -0.5, -0.5)):
        _, ids = draw(shim, surfels(dict(nx=n[0], ny=n[1], nz=n[2])), mvp, eye, 200, 200)
        assert np.all(ids == -1), n
    _, ids = draw(shim, surfels(dict(nx=0.0, ny=0.6, nz=0.8)), mvp, eye, 200, 200)
    assert (ids == 0).sum() > 100


def test_label_zero_is_not_drawn_and_uncovers_the_surfel_behind(shim):
    mvp, eye = ortho_top()
    s = surfels(dict(z=1.0, r=0.0), dict(z=0.0, r=40 / 255.0))
    rgba, ids = draw(shim, s, mvp, eye, 200, 200, mode=5)
    assert ids[100, 100] == 1
    assert tuple(rgba[100, 100]) == tuple(kitti.semantic_color_map()[40]) + (255,)
    _, ids2 = draw(shim, s, mvp, eye, 200, 200, mode=2)
    assert ids2[100, 100] == 0  # other modes draw it


def test_mode_2_is_abs_normal_and_mode_5_the_table_colour(shim):
    mvp, eye = ortho_top()
    rgba, ids = draw(shim, surfels(dict(nx=-0.6, ny=0.0, nz=0.8)), mvp, eye, 200, 200, mode=2)
    assert tuple(rgba[100, 100]) == (round(0.6 * 255), 0, round(0.8 * 255), 255)
    table = np.zeros((DRAW_COLORS, 3), dtype=np.uint8)
    table[44] = (7, 77, 177)
    s = surfels(dict(r=44 / 255.0))
    rgba, _ = dc.shim_draw(shim, s, POSES, core.draw_params(mvp, 200, 200, eye, color_mode=5, color_map=table))
    assert tuple(rgba[100, 100]) == (7, 77, 177, 255)


def test_mode_4_alpha_below_half_neither_colours_nor_hides(shim):
    mvp, eye = ortho_top()
    # alpha = 1 - clamp(conf_threshold - c, 0.1, 1): c = 9.0 -> 0 (discarded), c = 9.8 -> 0.8
    s = surfels(dict(z=1.0, confidence=9.0, color=float(0xff0000)), dict(z=0.0, confidence=9.8, color=float(0x00ff00)))
    rgba, ids = draw(shim, s, mvp, eye, 200, 200, mode=4)
    assert ids[100, 100] == 1 and rgba[100, 100, 3] == round(0.8 * 255)
    # the radius of mode 4 is r / sqrt(2): 10 pixels -> 7.07
    n = int((ids == 1).sum())
    assert abs(n - math.pi * 50.0) <= 2 * math.pi * 7.1


def test_empty_map_is_the_clear_colour(shim):
    mvp, eye = ortho_top()
    rgba, ids = dc.shim_draw(shim, np.zeros(0, dtype=SURFEL_DTYPE), POSES,
                             dc.params(mvp, eye, 33, 17, 5, clear_color=(0.2, 0.4, 0.6, 1.0)))
    assert np.all(ids == -1) and np.all(rgba == np.array([51, 102, 153, 255], dtype=np.uint8))


# ---- the shim against the reference's own shaders in a real GL
def gl_or_skip():
    import gl_draw_ref
    if not gl_draw_ref.available():
        pytest.skip("no Mesa llvmpipe or no reference shader tree")
    return gl_draw_ref


CAMERAS = ["chase", "birdseye", "inside"]


def camera(name, poses, W, H):
    if name == "chase":
        return dc.chase_camera(poses[2], W, H)
    if name == "birdseye":
        return dc.birdseye_camera([0.0, 0.0, 0.0], W, H, half=20.0)
    return dc.inside_camera([0.5, 0.2, -0.8], 0.3, W, H)


@pytest.mark.parametrize("mode", [2, 5])
@pytest.mark.parametrize("cam", CAMERAS)
def test_shim_matches_the_reference_shaders_in_gl(shim, cam, mode):
    gr = gl_or_skip()
    s, poses = dc.planar_map(20000)
    W, H = 333, 197
    mvp, eye = camera(cam, poses, W, H)
    dp = dc.params(mvp, eye, W, H, mode)
    a, ids = dc.shim_draw(shim, s, poses, dp)
    b = gr.gl_draw(s, poses, dp)
    frac, n = gr.agreement(a, b, WHITE)
    assert n > 0.3 * W * H
    assert frac >= 0.97, f"{cam} mode {mode}: {frac:.4f} of {n} covered pixels agree"


def test_inside_camera_clips_at_the_near_plane(shim):
    """the perspective case of the GL comparison above really exercises near-plane clipping"""
    s, poses = dc.planar_map(20000)
    mvp, eye = camera("inside", poses, 333, 197)
    dp = dc.params(mvp, eye, 333, 197, 2)
    shim.draw_shim_corners.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    table = dc.cm_poses(poses)
    corners = (C.c_float * 24)()
    straddle = 0
    for k in range(s.shape[0]):
        if shim.draw_shim_corners(C.byref(dp), s[k:k + 1].ctypes.data, table.ctypes.data, table.shape[0], corners):
            cv = np.array(corners).reshape(4, 6)
            near = cv[:, 2] + cv[:, 3]
            straddle += bool((near > 0).any() and (near < 0).any())
    assert straddle >= 3, straddle


# ---- ABI
FIELDS = ["mvp", "view_pos", "width", "height", "color_mode", "conf_threshold", "backface_culling", "use_stability",
          "clear_color", "num_lights", "lights", "mat_ambient", "mat_diffuse", "mat_specular", "mat_emission",
          "mat_shininess", "mat_alpha", "color_map"]


def test_draw_params_layout_matches_c(tmp_path):
    src = tmp_path / "probe.c"
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{ROOT}/include/suma_hip.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(suma_draw_params));',
             'printf("light %zu\\n", sizeof(suma_draw_light));']
    lines += [f'printf("{f} %zu\\n", offsetof(suma_draw_params, {f}));' for f in FIELDS]
    lines += ["return 0; }"]
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", str(src), "-o", str(exe)])
    out = dict(l.split(" ", 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(DrawParams)
    for f in FIELDS:
        assert int(out[f]) == getattr(DrawParams, f).offset, f


LIB = os.path.join(ROOT, "semantic_suma_amd", "libsuma_hip.so")


def test_c_default_state_equals_the_python_default():
    """suma_draw_params_default and core.draw_params give the same lights, material and options (SurfelMap.cpp:195-229)"""
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    L = C.CDLL(LIB)
    L.suma_draw_params_default.argtypes = [C.c_void_p]
    c = DrawParams()
    L.suma_draw_params_default(C.byref(c))
    py = core.draw_params(np.zeros((4, 4)), 0, 0, (0, 0, 0), color_map=np.zeros((DRAW_COLORS, 3), np.uint8),
                          lights=core.DRAW_LIGHTS)
    py.num_lights = 1
    assert bytes(c) == bytes(py)


def test_suma_map_draw_is_exported():
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build())"
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert re.search(r"\bT suma_map_draw$", out, re.M) and re.search(r"\bT suma_draw_params_default$", out, re.M)


def test_semantic_color_map_rule():
    t = kitti.semantic_color_map({7: (1, 2, 3), 300: (9, 9, 9)})
    assert t.shape == (260, 3) and t.dtype == np.uint8
    assert tuple(t[7]) == (3, 2, 1)  # BGR -> RGB
    assert int(t.sum()) == 6  # missing ids are black, ids beyond 259 ignored
    assert kitti.semantic_color_map().shape == (260, 3)


def test_camera_helpers():
    P = core.perspective(90.0, 2.0, 1.0, 3.0)
    v = P @ np.array([2.0, 1.0, -1.0, 1.0])
    assert np.allclose(v[:3] / v[3], [1.0, 1.0, -1.0])
    v = P @ np.array([0.0, 0.0, -3.0, 1.0])
    assert np.isclose(v[2] / v[3], 1.0)
    O = core.orthographic(-1, 3, -2, 2, 0.5, 10.0)
    assert np.allclose(O @ [3, 2, -10, 1], [1, 1, 1, 1])
    V = core.look_at([0, 0, 5], [0, 0, 0], [0, 1, 0])
    assert np.allclose(V @ [0, 0, 0, 1], [0, 0, -5, 1])
    # robot x forward -> GL -z, y left -> GL -x, z up -> GL y
    assert np.allclose(core.ROSE2GL @ [1, 2, 3, 1], [-2, 3, -1, 1])


# ---- resources
def test_draw_kernels_use_no_scratch_and_keep_their_stated_vgprs(tmp_path):
    csrc = os.path.join(ROOT, "semantic_suma_amd", "csrc")
    header = open(os.path.join(csrc, "k_draw.hip")).read().split("*/", 1)[0]
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"\*\s+(kd_\w+)\s.*?(\d+) VGPRs\.", header, re.S)}
    assert set(stated) == {"kd_raster", "kd_big", "kd_resolve"}, stated
    env = dict(os.environ, PATH="/opt/rocm/bin:" + os.environ.get("PATH", ""))
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), "k_draw.hip"],
                             capture_output=True, text=True, timeout=900, env=env)
    except FileNotFoundError:
        pytest.skip("no hipcc")
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"^(?:void )?(\S+)\s+(\d+)\s+(\d+)\s+\|", line)
        if m:
            seen[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    assert set(seen) == set(stated), out.stdout
    for k, (vgpr, sgpr_spill) in seen.items():
        assert vgpr <= stated[k], f"{k}: {vgpr} VGPRs, the header states {stated[k]}"
        assert sgpr_spill == 0, k
    asm = tmp_path / "k_draw.s"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-mllvm", "-amdgpu-kernarg-preload-count=16", "-w", "--cuda-device-only", "-S",
                           "k_draw.hip", "-o", str(asm)], cwd=csrc, env=env)
    text = asm.read_text()
    priv = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(priv) == 3 and all(int(p) == 0 for p in priv), priv
    assert "scratch_" not in text


GL_DRAW_GOLDEN = os.path.join(HERE, "golden", "gl_draw_256x160.npz")


def load_gl_fixture():
    z = np.load(GL_DRAW_GOLDEN)
    s = np.ascontiguousarray(z["surfels"]).view(SURFEL_DTYPE).reshape(-1)
    W, H = (int(v) for v in z["size"])
    return z, s, z["poses"], W, H


@pytest.mark.parametrize("mode", [0, 2, 5])
def test_shim_matches_the_recorded_gl_fixture(shim, mode):
    """tests/golden/gl_draw_256x160.npz (make_gl_draw_golden.py): llvmpipe running the reference's shaders, camera
    inside the map"""
    import gl_draw_ref
    z, s, poses, W, H = load_gl_fixture()
    dp = core.draw_params(z["mvp"], W, H, z["view_pos"], color_mode=mode, color_map=z["color_map"])
    a, _ = dc.shim_draw(shim, s, poses, dp)
    frac, n = gl_draw_ref.agreement(a, z[f"gl_mode{mode}"], WHITE)
    assert n > 0.3 * W * H and frac >= 0.97, (frac, n)
