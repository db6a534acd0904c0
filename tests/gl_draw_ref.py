"""TEST INFRASTRUCTURE: the reference's draw_surfels.{vert,geom,frag} run by a real OpenGL (Mesa llvmpipe, through
oracle/glref.py) with the GL state SurfelMap::draw sets (SurfelMap.cpp:1167-1230): GL_LESS depth test into a 24-bit depth
buffer, no blending, the pose buffer on texture unit 5 and the semantic colour map -- a 260-texel RGB8 1D texture,
NEAREST / CLAMP_TO_BORDER (SurfelMap.cpp:307-309, 1238-1256) -- on unit 7, into an RGBA8 colour buffer read back with
glReadPixels.  Used by tests/test_draw_host.py and tests/golden/make_gl_draw_golden.py only.
"""
import ctypes as C
import os

import numpy as np

from oracle import glref

E = dict(TEXTURE_1D=0x0DE0, RGB8=0x8051, RGB=0x1907, UNSIGNED_BYTE=0x1401, RGBA8=0x8058, UNPACK_ALIGNMENT=0x0CF5,
         PACK_ALIGNMENT=0x0D05)
u32, i32, f32, vp = C.c_uint, C.c_int, C.c_float, C.c_void_p


def available():
    return glref.available() and os.path.exists(os.path.join(glref.SHADER_DIR, "draw_surfels.geom"))


_PROG = []


def _program():
    if not _PROG:
        _PROG.append(glref.Program({"VERTEX_SHADER": "draw_surfels.vert", "GEOMETRY_SHADER": "draw_surfels.geom",
                                    "FRAGMENT_SHADER": "draw_surfels.frag"}))
    return _PROG[0]


def gl_draw(surfels, poses, dp):
    """surfels: SURFEL_DTYPE records, poses [n, 4, 4] row-major float32, dp: types.DrawParams (mvp column-major as the
    C-ABI takes it) -> uint8 [H, W, 4] in glReadPixels order (row 0 = bottom)"""
    g = glref.Context.get()
    GL = glref.GL
    W, H = int(dp.width), int(dp.height)
    prog = _program()
    surfels = np.ascontiguousarray(surfels)
    vbo = glref.Buffer(surfels.view(np.uint8))
    vao = glref.surfel_vao(vbo)
    # poseBuffer: texelFetch(poseBuffer, 4 k + c) is column c of pose k (Eigen's column-major storage)
    cm = np.ascontiguousarray(np.asarray(poses, dtype=np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
    ptex = glref.BufferTexture(cm.reshape(-1, 4))
    # colour map: setColorMap's RGB8 1D texture
    tex = glref.gen("Textures")
    g.fn("glActiveTexture", None, u32)(GL["TEXTURE0"] + 7)
    g.fn("glBindTexture", None, u32, u32)(E["TEXTURE_1D"], tex)
    g.fn("glPixelStorei", None, u32, i32)(E["UNPACK_ALIGNMENT"], 1)
    cmap = np.ctypeslib.as_array(dp.color_map).reshape(260, 3).astype(np.uint8).copy()
    g.fn("glTexImage1D", None, u32, i32, i32, i32, i32, u32, u32, vp)(E["TEXTURE_1D"], 0, E["RGB8"], 260, 0, E["RGB"],
                                                                      E["UNSIGNED_BYTE"], cmap.ctypes.data)
    for pname, val in (("TEXTURE_MIN_FILTER", "NEAREST"), ("TEXTURE_MAG_FILTER", "NEAREST"),
                       ("TEXTURE_WRAP_S", "CLAMP_TO_BORDER")):
        g.fn("glTexParameteri", None, u32, u32, i32)(E["TEXTURE_1D"], GL[pname], GL[val])
    ptex.bind(5)
    # framebuffer: RGBA8 colour + DEPTH24_STENCIL8
    fbo = glref.Framebuffer(W, H)
    rb = glref.gen("Renderbuffers")
    g.fn("glBindRenderbuffer", None, u32, u32)(GL["RENDERBUFFER"], rb)
    g.fn("glRenderbufferStorage", None, u32, u32, i32, i32)(GL["RENDERBUFFER"], E["RGBA8"], W, H)
    fbo.bind()
    g.fn("glFramebufferRenderbuffer", None, u32, u32, u32, u32)(GL["FRAMEBUFFER"], GL["COLOR_ATTACHMENT0"],
                                                                GL["RENDERBUFFER"], rb)
    bufs = (u32 * 1)(GL["COLOR_ATTACHMENT0"])
    g.fn("glDrawBuffers", None, i32, vp)(1, bufs)
    if g.fn("glCheckFramebufferStatus", u32, u32)(GL["FRAMEBUFFER"]) != GL["FRAMEBUFFER_COMPLETE"]:
        raise glref.GLError("draw framebuffer incomplete")
    # uniforms (SurfelMap.cpp:187-229 leaves the lights / material, draw() sets the rest)
    mvp = np.asarray(dp.mvp, dtype=np.float32).reshape(4, 4).T  # column-major -> row-major for Program.set
    u = {"mvp": mvp, "colorMode": int(dp.color_mode), "conf_threshold": float(dp.conf_threshold),
         "view_pos": list(dp.view_pos), "timestamp": 0, "drawCurrentSurfelsOnly": False,
         "backface_culling": bool(dp.backface_culling), "use_stability": bool(dp.use_stability),
         "num_lights": int(dp.num_lights), "poseBuffer": 5, "color_map": 7,
         "material.ambient": list(dp.mat_ambient), "material.diffuse": list(dp.mat_diffuse),
         "material.specular": list(dp.mat_specular), "material.emission": list(dp.mat_emission),
         "material.shininess": float(dp.mat_shininess), "material.alpha": float(dp.mat_alpha)}
    for i in range(10):
        L = dp.lights[i]
        u[f"lights[{i}].position"] = list(L.position)
        u[f"lights[{i}].ambient"] = list(L.ambient)
        u[f"lights[{i}].diffuse"] = list(L.diffuse)
        u[f"lights[{i}].specular"] = list(L.specular)
    prog.set(**u)
    g.fn("glEnable", None, u32)(GL["DEPTH_TEST"])
    g.fn("glDepthFunc", None, u32)(GL["LESS"])
    g.fn("glDisable", None, u32)(GL["BLEND"])
    g.fn("glViewport", None, i32, i32, i32, i32)(0, 0, W, H)
    g.fn("glClearColor", None, f32, f32, f32, f32)(*[float(c) for c in dp.clear_color])
    glref.clear()
    prog.use()
    glref.draw_points(vao, surfels.shape[0])
    g.fn("glFinish", None)()
    g.check("draw_surfels")
    out = np.empty((H, W, 4), dtype=np.uint8)
    g.fn("glReadBuffer", None, u32)(GL["COLOR_ATTACHMENT0"])
    g.fn("glPixelStorei", None, u32, i32)(E["PACK_ALIGNMENT"], 1)
    g.fn("glReadPixels", None, i32, i32, i32, i32, u32, u32, vp)(0, 0, W, H, GL["RGBA"], E["UNSIGNED_BYTE"],
                                                                 out.ctypes.data)
    g.check("glReadPixels")
    for name, ids in (("glDeleteTextures", tex), ("glDeleteRenderbuffers", rb)):
        arr = (u32 * 1)(ids)
        g.fn(name, None, i32, vp)(1, arr)
    return out


def agreement(a, b, clear):
    """fraction of the covered pixels (not the clear colour in at least one image) whose RGBA8 channels all agree
    within 1, and the number of covered pixels"""
    a = a.astype(np.int32)
    b = b.astype(np.int32)
    clear = np.asarray(clear, dtype=np.int32)
    cov = np.any(a != clear, axis=-1) | np.any(b != clear, axis=-1)
    ok = np.all(np.abs(a - b) <= 1, axis=-1)
    n = int(cov.sum())
    return (float((ok & cov).sum()) / n if n else 1.0), n
