"""TEST INFRASTRUCTURE: a plain fp64 evaluation of K6 (Frame2Model::jacobianProducts) and crafted scenes for it.

Nothing here shares code, operation order or number format with oracle/o_icp.c or csrc/k_icp.hip: the stage is written
down from what the shader means (point-to-plane ICP with projective association), in numpy fp64, vectorised over the
pixels.  The only fp32 in it is what the stage is GIVEN in fp32: the maps and the pose (cast once, as the reference
casts it).  numpy only; this is a helper module, not a conftest.

    room_frames(W, H, params, T)                    analytic room scene, one ray per texel centre
    k6_fp64(params, data, model, T, iteration)      the stage; also its counts, max |term| and smallest margins
    gn_fp64(params, data, model, T0, n)             n Gauss-Newton steps on k6_fp64
    single_pixel_frames(...)                        a data frame of listed pixels against one constant model texel
"""
from __future__ import annotations

import numpy as np

DYNAMIC_LABELS = (10, 11, 13, 15, 18, 20, 30, 31, 32)
ROOM = dict(x=5.0, y=5.0, floor=-1.7, ceiling=3.0)
# |label - L| below this counts as "the texel holds label L" (a stored label is float32(L / 255) * 255: off by < 1e-5;
# a bilinear mix of two different labels comes this close only within 0.02 texels of a texel centre)
LABEL_EPS = 0.02


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def pose_from(yaw_deg=0.0, t=(0.0, 0.0, 0.0)):
    """4 x 4 pose (sensor -> world), rotation about z"""
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


def texel_rays(W, H, params):
    """unit directions (H x W x 3, sensor frame) through the texel centres of a W x H range image: the inverse of the
    stage's projection, ix = W/2 (1 - yaw / pi), iy = H (1 - (fov_up - elevation) / fov); row 0 is the lowest beam"""
    fov_up, fov_down = abs(float(params.data_fov_up)), abs(float(params.data_fov_down))
    fov = fov_up + fov_down
    ix = np.arange(W) + 0.5
    iy = np.arange(H) + 0.5
    yaw = np.pi * (1.0 - 2.0 * ix / W)
    elev = np.deg2rad(fov_up - (1.0 - iy / H) * fov)
    ce, se = np.cos(elev)[:, None], np.sin(elev)[:, None]
    d = np.empty((H, W, 3))
    d[..., 0] = ce * np.cos(yaw)[None, :]
    d[..., 1] = ce * np.sin(yaw)[None, :]
    d[..., 2] = se * np.ones(W)[None, :]
    return d


def room_cast(W, H, params, T):
    """ray-cast the room from the sensor pose T: (points, normals, plane id) in the SENSOR frame, fp64.
    plane id: 0 / 1 the walls x = +5 / -5, 2 / 3 the walls y = +5 / -5, 4 the floor, 5 the ceiling"""
    T = np.asarray(T, dtype=np.float64)
    R, o = T[:3, :3], T[:3, 3]
    d = texel_rays(W, H, params)
    dw = d @ R.T
    planes = [(0, ROOM["x"], (-1, 0, 0)), (0, -ROOM["x"], (1, 0, 0)), (1, ROOM["y"], (0, -1, 0)),
              (1, -ROOM["y"], (0, 1, 0)), (2, ROOM["floor"], (0, 0, 1)), (2, ROOM["ceiling"], (0, 0, -1))]
    best = np.full((H, W), np.inf)
    nrm = np.zeros((H, W, 3))
    pid = np.zeros((H, W), dtype=np.int64)
    for k, (axis, c, n) in enumerate(planes):
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (c - o[axis]) / dw[..., axis]
        hit = np.isfinite(s) & (s > 0) & (s < best)
        best = np.where(hit, s, best)
        nrm[hit] = n
        pid[hit] = k
    assert np.all(np.isfinite(best)), "the sensor must sit inside the room"
    return best[..., None] * d, nrm @ R, pid  # n_sensor = R^T n_world


def room_frames(W, H, params, T):
    """(vertex, normal) maps H x W x 4, float32, w = 1, of the room seen from pose T, in the sensor frame at T"""
    p, n, _ = room_cast(W, H, params, T)
    V = np.ones((H, W, 4), dtype=np.float32)
    N = np.ones((H, W, 4), dtype=np.float32)
    V[..., :3] = p
    N[..., :3] = n
    return V, N


def semantic_map(labels, probs):
    """the semantic map K6 reads: x = label / 255, w = probability (y, z are not read by the stage)"""
    labels = np.asarray(labels, dtype=np.float64)
    S = np.zeros(labels.shape + (4,), dtype=np.float32)
    S[..., 0] = (labels / 255.0).astype(np.float32)
    S[..., 3] = np.asarray(probs, dtype=np.float32)
    return S


def single_pixel_frames(W, H, pixels, model_v, model_n, Wm=None, Hm=None, model_label=0.0, model_patch=None):
    """data: invalid (all-zero texels) except the listed pixels; model: one constant valid texel everywhere.

    pixels: list of dict(at=(x, y), v=(3), n=(3), label=float, prob=float); label / prob default to 0.
    model_patch: optional list of (x, y, vertex4 | None, normal4 | None, label | None) texels that replace the constant.
    Returns ((Vd, Nd, Sd), (Vm, Nm, Sm)), all float32."""
    Wm, Hm = Wm or W, Hm or H
    Vd = np.zeros((H, W, 4), dtype=np.float32)
    Nd = np.zeros((H, W, 4), dtype=np.float32)
    Sd = np.zeros((H, W, 4), dtype=np.float32)
    for px in pixels:
        x, y = px["at"]
        Vd[y, x] = (*px["v"], 1.0)
        Nd[y, x] = (*px["n"], 1.0)
        Sd[y, x, 0] = np.float32(px.get("label", 0.0) / 255.0)
        Sd[y, x, 3] = px.get("prob", 0.0)
    Vm = np.zeros((Hm, Wm, 4), dtype=np.float32)
    Nm = np.zeros((Hm, Wm, 4), dtype=np.float32)
    Sm = np.zeros((Hm, Wm, 4), dtype=np.float32)
    Vm[...] = (*model_v, 1.0)
    Nm[...] = (*model_n, 1.0)
    Sm[..., 0] = np.float32(model_label / 255.0)
    for (x, y, v4, n4, lab) in (model_patch or []):
        if v4 is not None:
            Vm[y, x] = v4
        if n4 is not None:
            Nm[y, x] = n4
        if lab is not None:
            Sm[y, x, 0] = np.float32(lab / 255.0)
    return (Vd, Nd, Sd), (Vm, Nm, Sm)


# ---------------------------------------------------------------------------------------------------------------------
# the stage in fp64
# ---------------------------------------------------------------------------------------------------------------------
def _fetch_nearest(m, ix, iy):
    H, W = m.shape[:2]
    x = np.clip(np.floor(ix).astype(np.int64), 0, W - 1)
    y = np.clip(np.floor(iy).astype(np.int64), 0, H - 1)
    return m[y, x]


def _fetch_bilinear(m, ix, iy):
    """GL_LINEAR with a zero border: texel centres at integer + 0.5, all four channels filtered"""
    H, W = m.shape[:2]
    pad = np.zeros((H + 2, W + 2, 4))
    pad[1:-1, 1:-1] = m
    u, v = ix - 0.5, iy - 0.5
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[:, None], (v - fv)[:, None]
    i0 = np.clip(fu.astype(np.int64) + 1, 0, W)  # index into the padded map
    j0 = np.clip(fv.astype(np.int64) + 1, 0, H)
    return ((1 - a) * (1 - b) * pad[j0, i0] + a * (1 - b) * pad[j0, i0 + 1] + (1 - a) * b * pad[j0 + 1, i0] +
            a * b * pad[j0 + 1, i0 + 1])


def _is_dynamic(label):
    """(mask, distance of the decision from LABEL_EPS)"""
    d = np.min(np.abs(label[:, None] - np.asarray(DYNAMIC_LABELS, dtype=np.float64)[None, :]), axis=1)
    return d < LABEL_EPS, np.abs(d - LABEL_EPS)


def k6_fp64(params, data, model, T, iteration=0):
    """data / model: (vertex, normal[, semantic]) float32 maps.  Returns a dict:
    F, JtJ (6 x 6), Jtr (6), counts = (valid, outlier, invalid), max_term (largest |term| of any sum),
    margin (smallest distance by which any comparison was decided), texel_margin (nearest sampling: smallest distance
    of a projected coordinate from a texel edge, in texels)."""
    Vd, Nd = (np.asarray(m, dtype=np.float64) for m in data[:2])
    Vm, Nm = (np.asarray(m, dtype=np.float64) for m in model[:2])
    Sd = np.asarray(data[2], dtype=np.float64) if len(data) > 2 and data[2] is not None else np.zeros_like(Vd)
    Sm = np.asarray(model[2], dtype=np.float64) if len(model) > 2 and model[2] is not None else np.zeros_like(Vm)
    Hm, Wm = Vm.shape[:2]
    P = Vd.shape[0] * Vd.shape[1]
    Vd, Nd, Sd = Vd.reshape(P, 4), Nd.reshape(P, 4), Sd.reshape(P, 4)
    T = np.asarray(T, dtype=np.float64).astype(np.float32).astype(np.float64)  # the pose the shader is handed
    R, t = T[:3, :3], T[:3, 3]
    fov_up, fov_down = abs(float(params.data_fov_up)), abs(float(params.data_fov_down))
    fov = fov_up + fov_down
    dist_thresh = float(params.icp_max_distance)
    cos_thresh = float(np.float32(np.cos(float(params.icp_max_angle) * np.pi / 180.0)))
    factor = float(params.factor)
    wf = int(params.weight_function)
    margins = {}

    e_d = Vd[:, 3] + Nd[:, 3]
    cand = e_d > 1.5
    margins["e_d"] = np.abs(e_d - 1.5)
    v_d = Vd[:, :3] @ R.T + t
    n_d = Nd[:, :3] @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.linalg.norm(v_d, axis=1)
        yaw = np.arctan2(v_d[:, 1], v_d[:, 0])
        pitch = -np.arcsin(v_d[:, 2] / depth)
        ix = 0.5 * (1.0 - yaw / np.pi) * Wm
        iy = (1.0 - (np.rad2deg(pitch) + fov_up) / fov) * Hm
        inside = (ix >= 0) & (ix < Wm) & (iy >= 0) & (iy < Hm)  # False for NaN
    edge = np.minimum(np.minimum(np.abs(ix), np.abs(Wm - ix)), np.minimum(np.abs(iy), np.abs(Hm - iy)))
    margins["image"] = np.where(cand & np.isfinite(edge), edge, np.inf)
    cand = cand & inside
    idx = np.flatnonzero(cand)
    ix, iy, v_d, n_d = ix[idx], iy[idx], v_d[idx], n_d[idx]
    texel_margin = np.inf
    if params.bilinear_sampling:
        vm4, nm4, sm4 = (_fetch_bilinear(m, ix, iy) for m in (Vm, Nm, Sm))
    else:
        vm4, nm4, sm4 = (_fetch_nearest(m, ix, iy) for m in (Vm, Nm, Sm))
        if idx.size:
            fx, fy = ix - np.floor(ix), iy - np.floor(iy)
            texel_margin = float(min(np.min(np.minimum(fx, 1 - fx)), np.min(np.minimum(fy, 1 - fy))))
    e_m = vm4[:, 3] + nm4[:, 3]
    margins["e_m"] = np.abs(e_m - 1.5)
    pair = e_m > 1.5
    v_d, n_d, v_m, n_m = v_d[pair], n_d[pair], vm4[pair, :3], nm4[pair, :3]
    sd4, sm4 = Sd[idx][pair], sm4[pair]

    dist = np.linalg.norm(v_m - v_d, axis=1)
    cosang = np.sum(n_m * n_d, axis=1)
    margins["distance"], margins["angle"] = np.abs(dist - dist_thresh), np.abs(cosang - cos_thresh)
    inlier = ~(dist > dist_thresh) & ~(cosang < cos_thresh)
    r = np.sum(n_m * (v_d - v_m), axis=1)
    J = np.concatenate([n_m, np.cross(v_d, n_m)], axis=1)
    w = np.ones_like(r)
    if wf in (1, 4):  # Huber
        big = np.abs(r) > factor
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(big, factor / np.abs(r), 1.0)
        margins["factor"] = np.abs(np.abs(r) - factor)
    elif wf == 2 and iteration > 0:  # Tukey
        big = np.abs(r) > factor
        w = np.where(big, 0.0, (1.0 - (r / factor) ** 2) ** 2)
        margins["factor"] = np.abs(np.abs(r) - factor)
    # dynamic classes: the data's confidence in the same label, or in a different one
    model_label, data_label, prob = sm4[:, 0] * 255.0, sd4[:, 0] * 255.0, sd4[:, 3]
    dyn, dyn_margin = _is_dynamic(model_label)
    margins["dynamic"] = dyn_margin
    half = lambda l: np.abs(np.abs(l - np.floor(l)) - 0.5)  # distance of a label from the rounding tie
    margins["rounding"] = np.where(dyn, np.minimum(half(model_label), half(data_label)), np.inf)
    same = np.rint(data_label) == np.rint(model_label)
    w = np.where(dyn, w * np.where(same, prob, 1.0 - prob), w)

    wi, ri, Ji = w[inlier], r[inlier], J[inlier]
    JtJ = np.einsum("p,pi,pj->ij", wi, Ji, Ji)
    Jtr = np.einsum("p,p,pi->i", wi, ri, Ji)
    F = float(np.sum(w * r * r))
    terms = [np.abs(w * r * r)]
    if ri.size:
        terms += [np.abs(wi[:, None, None] * Ji[:, :, None] * Ji[:, None, :]).ravel(), np.abs((wi * ri)[:, None] * Ji).ravel()]
    max_term = float(max((np.max(x) for x in terms if x.size), default=0.0))
    n_valid = int(r.size)
    margins = {k: float(np.min(m)) if np.size(m) else np.inf for k, m in margins.items()}
    margin = min(margins.values())
    return dict(F=F, JtJ=JtJ, Jtr=Jtr, counts=(n_valid, int(np.count_nonzero(~inlier)), P - n_valid),
                max_term=max_term, margin=margin, margins=margins, texel_margin=texel_margin)


def se3_exp(x):
    """exp of a twist x = (v, omega) -> 4 x 4, fp64 (Rodrigues; the series below theta = 1e-8)"""
    v, o = np.asarray(x[:3], dtype=np.float64), np.asarray(x[3:], dtype=np.float64)
    K = np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]])
    th = float(np.linalg.norm(o))
    if th < 1e-8:
        A, B, Cc = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        A, B, Cc = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + Cc * (K @ K)) @ v
    return T


def gn_fp64(params, data, model, T0, n):
    """n Gauss-Newton steps on k6_fp64 from T0: the poses [T0, T1, .. Tn]; the iteration counter advances per step"""
    T = np.asarray(T0, dtype=np.float64).copy()
    poses = [T.copy()]
    for k in range(n):
        s = k6_fp64(params, data, model, T, k)
        dx = np.linalg.solve(s["JtJ"], -s["Jtr"])
        T = se3_exp(dx) @ T
        poses.append(T.copy())
    return poses


def pose_delta(Ta, Tb):
    """(metres, radians) between two poses"""
    d = np.linalg.inv(Ta) @ Tb
    return (float(np.linalg.norm(d[:3, 3])),
            float(np.arccos(np.clip(0.5 * (np.trace(d[:3, :3]) - 1.0), -1.0, 1.0))))
