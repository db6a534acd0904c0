"""TEST INFRASTRUCTURE: a plain fp64 statement of Preprocessing::process (K1 .. K3 and the vertex-map filters).

Nothing here shares code, operation order or number format with oracle/o_preprocess.c, csrc/k_preprocess.hip or
csrc/k_filters.hip: every stage is written down from what its shader means (gen_vertexmap.*, gen_normalmap.frag,
floodfill.frag, avg_vertexmap.frag, bilateral_filter.frag; host side Preprocessing.cpp:120-339), in numpy fp64,
vectorised over points and texels.  The only fp32 in it is what the stage is GIVEN in fp32 (points, labels,
probabilities, the parameters, the shaders' literals 0.007 and 1e-7) and what it STORES as a 24-bit depth.  numpy only;
a helper module, not a conftest.

    k1_points(p, pts)                       per point: continuous texel coordinates (u, v), normalised depth, margins
    k1_fp64(p, pts, labels, probs, t)       the z-buffered scatter: winner index, vertex and raw label map, depth gap
    k1_sum_fp64(...) / k1b_fp64 / k1c_fp64  the blended scatter, its average and the bilateral range filter
    fetch_fp64(M, sampling)                 texture(sampler2DRect, integer coordinate) under both texture states
    k2_fp64(V, S) / k3_fp64(V, E)           normals + erosion, flood fill; with every gate's margin

Margins (all "distance from the decision", to be held against a bound measured on the oracle):
    texel   distance of u and of v from the nearest integer, in pixels (the image border is an integer too)
    clip    distance of the normalised depth from 0 and from 1, i.e. of the range from [min_depth, max_depth]; held
            against the measured bound plus two fp32 steps of the point's own range (zn_step)
    gap     depth gap between a texel's winner and its runner-up, in quanta of the 24-bit buffer.  Both sides round
            to the nearest of 2^24 - 1 steps and rounding is monotone, so a gap above 1 + 2 dev (dev: the deviation of
            the window depth, in quanta) leaves the same winner whatever the point order; below that the index may
            decide, in either evaluation
    len     | |un x vn| - 1e-7 |
    fill    | |lp - lq| - 0.007 lp | of every neighbour the fill tested
The `w` channels need no margin: without filters w is 0 or 1; the blended scatter counts points (integers below 2^24),
the GL-initial fetch weighs four texels by exactly 1/4, and n * fl(1 / n) = 1 in binary32 for every count below 41
(checked in the host test), so every w that meets a gate (0, 0.5, 1) is the same number in both evaluations.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U = 2.0 ** -24
DEPTH_STEPS = 16777215.0  # 2^24 - 1: GL_DEPTH24_STENCIL8
DYNAMIC_LABELS = (10, 11, 13, 15, 18, 20, 30, 31, 32)  # gen_vertexmap.vert:95-102
FILL_THRESHOLD = float(F32(0.007))
LEN_GATE = float(F32(0.0000001))
NEAREST, GL_INITIAL = 1, 0  # filter_sampling (suma_types.h)


def consts(p):
    fov_up, fov_down = abs(float(p.data_fov_up)), abs(float(p.data_fov_down))
    return dict(W=int(p.data_width), H=int(p.data_height), fov_up=fov_up, fov=fov_up + fov_down,
                min_depth=float(p.min_depth), max_depth=float(p.max_depth), label_offset=int(p.label_offset),
                prob_offset=int(p.prob_offset))


# ---------------------------------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------------------------------
def k1_points(p, pts):
    """pts: n x 4 float32.  u = W/2 (1 - yaw / pi), v = H (1 - (fov_up - elevation) / fov), zn = (range - min) / (max -
    min).  The yaw is the SPECIFIED atan2 (include/suma_detmath.h): y = -0 counts as +0, so the seam y = 0, x < 0 is
    yaw = +pi, column 0."""
    k = consts(p)
    x, y, z = (np.asarray(pts, dtype=F32)[:, i].astype(np.float64) for i in range(3))
    with np.errstate(all="ignore"):
        rng = np.sqrt(x * x + y * y + z * z)
        yaw = np.arctan2(y + 0.0, x)
        elev = np.arcsin(z / rng)
        u = 0.5 * (1.0 - yaw / np.pi) * k["W"]
        v = (1.0 - (k["fov_up"] - np.rad2deg(elev)) / k["fov"]) * k["H"]
        zn = (rng - k["min_depth"]) / (k["max_depth"] - k["min_depth"])
        finite = np.isfinite(u) & np.isfinite(v) & np.isfinite(zn)
        inside = finite & (u >= 0) & (u < k["W"]) & (v >= 0) & (v < k["H"]) & (zn >= 0) & (zn <= 1)
        m_texel = np.where(finite, np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v))), np.inf)
        m_clip = np.where(finite, np.minimum(np.abs(zn), np.abs(zn - 1.0)), np.inf)
        m_border = np.where(finite, np.minimum(np.minimum(np.abs(u), np.abs(u - k["W"])),
                                               np.minimum(np.abs(v), np.abs(v - k["H"]))), np.inf)
        tx = np.where(inside, np.floor(np.where(finite, u, 0.0)), -1).astype(np.int64)
        ty = np.where(inside, np.floor(np.where(finite, v, 0.0)), -1).astype(np.int64)
        # two fp32 steps of the range itself, in units of zn: what the stage's own fp32 length may be off by at this
        # range, whatever was measured at the ranges of another scene
        zn_step = np.where(finite, 2.0 * np.spacing(np.where(finite, rng, 1.0).astype(F32)).astype(np.float64) /
                           (k["max_depth"] - k["min_depth"]), 0.0)
    return dict(u=u, v=v, zn=zn, range=rng, finite=finite, inside=inside, tx=tx, ty=ty, m_texel=m_texel, m_clip=m_clip,
                m_border=m_border, zn_step=zn_step)


def _attributes(p, n, labels, probs, idx):
    """quirk B-1 (Preprocessing.cpp:142-145): label and probability of point i are read at i + offset, 0 beyond n"""
    k = consts(p)
    lab, prob = np.zeros(idx.shape), np.zeros(idx.shape)
    if labels is not None:
        li = idx + k["label_offset"]
        lab = np.where(li < n, np.asarray(labels, dtype=F32).astype(np.float64)[np.minimum(li, n - 1)], 0.0)
    if probs is not None:
        pi = idx + k["prob_offset"]
        prob = np.where(pi < n, np.asarray(probs, dtype=F32).astype(np.float64)[np.minimum(pi, n - 1)], 0.0)
    return lab, prob


def is_dynamic(label):
    return np.isin(label, np.asarray(DYNAMIC_LABELS, dtype=np.float64))


def k1_fp64(p, pts, labels, probs, timestamp):
    """the depth-tested scatter: per texel the point with the smallest 24-bit depth, then the lowest index.
    Returns V, S (H x W x 4; S = raw labels (l, l, l, prob) with l = label / 255), winner (-1: empty), count (points
    that land in the texel), gap (quanta between winner and runner-up, inf if alone), dropped (the winner is a dynamic
    class of a first scan: vertex zeroed, label kept) and the per-point dict."""
    k = consts(p)
    W, H = k["W"], k["H"]
    pts = np.asarray(pts, dtype=F32).reshape(-1, 4)
    n = pts.shape[0]
    pt = k1_points(p, pts)
    idx = np.flatnonzero(pt["inside"])
    pix = pt["ty"][idx] * W + pt["tx"][idx]
    q = pt["zn"][idx] * DEPTH_STEPS
    d24 = np.rint(q)
    order = np.lexsort((idx, d24, pix))
    idx, pix, q = idx[order], pix[order], q[order]
    head = np.ones(idx.shape, dtype=bool)
    head[1:] = pix[1:] != pix[:-1]
    winner = np.full(W * H, -1, dtype=np.int64)
    winner[pix[head]] = idx[head]
    count = np.bincount(pix, minlength=W * H)
    gap = np.full(W * H, np.inf)
    second = np.flatnonzero(~head & np.r_[False, head[:-1]])
    gap[pix[second]] = np.abs(q[second] - q[second - 1])
    V, S = np.zeros((W * H, 4)), np.zeros((W * H, 4))
    won = np.flatnonzero(winner >= 0)
    wi = winner[won]
    lab, prob = _attributes(p, n, labels, probs, wi)
    drop = is_dynamic(lab) & (timestamp < 10)
    V[won, :3] = np.where(drop[:, None], 0.0, pts[wi, :3].astype(np.float64))
    V[won, 3] = np.where(drop, 0.0, 1.0)
    S[won, :3] = (lab / 255.0)[:, None]
    S[won, 3] = prob
    dropped = np.zeros(W * H, dtype=bool)
    dropped[won] = drop
    sh = (H, W)
    return dict(V=V.reshape(H, W, 4), S=S.reshape(H, W, 4), winner=winner.reshape(sh), count=count.reshape(sh),
                gap=gap.reshape(sh), dropped=dropped.reshape(sh), points=pt)


def k1_decided(p, k1, eps_texel, eps_zn):
    """H x W: no point that could reach the texel sits within eps of a texel edge or of the depth clip (such a point
    taints the 3 x 3 texels around it), and the winner leads its runner-up by more than 1 + eps_zn quanta"""
    k = consts(p)
    W, H = k["W"], k["H"]
    pt = k1["points"]
    with np.errstate(invalid="ignore"):
        ez = eps_zn + pt["zn_step"]
        near = pt["finite"] & (pt["zn"] >= -ez) & (pt["zn"] <= 1 + ez) & (pt["u"] >= -eps_texel) & \
            (pt["u"] <= W + eps_texel) & (pt["v"] >= -eps_texel) & (pt["v"] <= H + eps_texel)
        unsafe = near & ((pt["m_texel"] <= eps_texel) | (pt["m_clip"] <= eps_zn + pt["zn_step"]))
    taint = np.zeros((H, W), dtype=bool)
    for i in np.flatnonzero(unsafe):
        cx, cy = int(np.floor(pt["u"][i])), int(np.floor(pt["v"][i]))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= cy + dy < H:
                    taint[cy + dy, (cx + dx) % W] = True
    return ~taint & (k1["gap"] > 1.0 + eps_zn * DEPTH_STEPS)


# ---------------------------------------------------------------------------------------------------------------------
# the filters
# ---------------------------------------------------------------------------------------------------------------------
def k1_sum_fp64(p, pts, labels, probs, timestamp):
    """the blended scatter (depth test off, GL_ONE / GL_ONE): per texel the sum of its points' (x, y, z, 1) and of
    (l, l, l, prob).  Dynamic points of the first scans are (0, 0, 0, 0): they add nothing, not even to the count.
    Also the sum of |x|, |y|, |z| (for the bound) and the number of points that land."""
    k = consts(p)
    W, H = k["W"], k["H"]
    pts = np.asarray(pts, dtype=F32).reshape(-1, 4)
    n = pts.shape[0]
    pt = k1_points(p, pts)
    idx = np.flatnonzero(pt["inside"])
    pix = pt["ty"][idx] * W + pt["tx"][idx]
    lab, prob = _attributes(p, n, labels, probs, idx)
    keep = ~(is_dynamic(lab) & (timestamp < 10))
    v4 = np.concatenate([pts[idx, :3].astype(np.float64), np.ones((idx.size, 1))], axis=1) * keep[:, None]
    s4 = np.concatenate([np.repeat((lab / 255.0)[:, None], 3, axis=1), prob[:, None]], axis=1)
    vsum, ssum, asum = np.zeros((W * H, 4)), np.zeros((W * H, 4)), np.zeros((W * H, 4))
    np.add.at(vsum, pix, v4)
    np.add.at(ssum, pix, s4)
    np.add.at(asum, pix, np.abs(v4))
    landed = np.bincount(pix, minlength=W * H)
    return dict(vsum=vsum.reshape(H, W, 4), ssum=ssum.reshape(H, W, 4), asum=asum.reshape(H, W, 4),
                landed=landed.reshape(H, W), points=pt)


def fetch_fp64(M, sampling):
    """texture(sampler2DRect, (x, y)) at every integer coordinate.  NEAREST: the texel.  The GL initial state (LINEAR,
    CLAMP_TO_EDGE): an integer coordinate is a texel corner, the result the mean of the four texels around it, indices
    clamped to the edge."""
    M = np.asarray(M, dtype=np.float64)
    if sampling == NEAREST:
        return M
    H, W = M.shape[:2]
    i0 = np.maximum(np.arange(W) - 1, 0)
    j0 = np.maximum(np.arange(H) - 1, 0)
    return 0.25 * (M[j0][:, i0] + M[j0] + M[:, i0] + M)


def k1b_fp64(vsum, sampling):
    """avg_vertexmap.frag:14-21: divide by the count where it exceeds 0.5"""
    f = fetch_fp64(vsum, sampling)
    w = f[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > 0.5, f / w, f)


def k1c_fp64(V, sampling, sigma_space, sigma_range):
    """bilateral_filter.frag:28-83: 13 x 13 window, columns wrap, rows cut at the image; a neighbour's range is
    length(vec4), w included (:64); the pixel distance is taken to the WRAPPED column, as the shader takes it.
    Returns (filtered map, filtered range)."""
    T = fetch_fp64(V, sampling)
    H, W = T.shape[:2]
    ss, sr = float(F32(sigma_space)), float(F32(sigma_range))
    fs, fr = -0.5 / (ss * ss), -0.5 / (sr * sr)
    rng = np.linalg.norm(T[..., :3], axis=-1)
    rng4 = np.linalg.norm(T, axis=-1)
    use = T[..., 3] >= 0.5  # `if (tmp.w < 0.5) continue`
    xs = np.arange(W)
    s1, s2 = np.zeros((H, W)), np.zeros((H, W))
    for dy in range(-6, 7):
        ys = np.arange(H) + dy
        rows = (ys >= 0) & (ys < H)
        yc = np.clip(ys, 0, H - 1)
        for dx in range(-6, 7):
            xx = (xs + dx) % W
            nb_r, nb_use = rng4[yc][:, xx], use[yc][:, xx] & rows[:, None]
            ds2 = ((xs - xx) ** 2)[None, :] + float(dy * dy)
            wgt = np.where(nb_use, np.exp(ds2 * fs + (rng - nb_r) ** 2 * fr), 0.0)
            s1 += nb_r * wgt
            s2 += wgt
    act = T[..., 3] > 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        fr_ = s1 / s2
        out = np.where(act[..., None], np.concatenate([fr_[..., None] * T[..., :3] / rng[..., None], np.ones((H, W, 1))], axis=-1), T)
    return out, np.where(act, fr_, np.nan)


# ---------------------------------------------------------------------------------------------------------------------
# K2, K3
# ---------------------------------------------------------------------------------------------------------------------
def _shift(M, dx, dy):
    """M at (x + dx, y + dy): columns wrap, rows outside the image are the zero border"""
    H = M.shape[0]
    out = np.roll(M, -dx, axis=1)
    if abs(dy) >= H:
        return np.zeros_like(out)
    if dy:
        z = np.zeros_like(out)
        if dy > 0:
            z[:H - dy] = out[dy:]
        else:
            z[-dy:] = out[:H + dy]
        out = z
    return out


def k2_fp64(V, S):
    """gen_normalmap.frag:41-99.  normal = normalize(normalize(u - p) x normalize(v - p)), u the right neighbour, v the
    one above.  Validity on .w: (1) u and v both invalid, (2) s and t both invalid, (3) u or v not above 0.5; then
    w = (len > 1e-7).  Erosion: a label goes to 0 when one of its four neighbours carries another non-zero label.
    Returns normal, eroded (H x W x 4), the rule masks, len, its margin, and bound_terms: the per-component
    sum|terms| of the cross product propagated through the normalisations (see normal_bound)."""
    V, S = np.asarray(V, dtype=np.float64), np.asarray(S, dtype=np.float64)
    H, W = V.shape[:2]
    p, u, v, s, t = V, _shift(V, 1, 0), _shift(V, 0, 1), _shift(V, -1, 0), _shift(V, 0, -1)
    pw = p[..., 3] > 0.0
    r1 = (u[..., 3] < 1.0) & (v[..., 3] < 1.0)
    r2 = (s[..., 3] < 1.0) & (t[..., 3] < 1.0)
    r3 = ~(u[..., 3] > 0.5) | ~(v[..., 3] > 0.5)
    valid = pw & ~r1 & ~r2 & ~r3
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = u[..., :3] - p[..., :3], v[..., :3] - p[..., :3]
        un, vn = a / np.linalg.norm(a, axis=-1, keepdims=True), b / np.linalg.norm(b, axis=-1, keepdims=True)
        w = np.cross(un, vn)
        ln = np.linalg.norm(w, axis=-1)
        nn = w / ln[..., None]
        # |terms| of each component of the cross product
        tx = np.abs(un[..., 1] * vn[..., 2]) + np.abs(un[..., 2] * vn[..., 1])
        ty = np.abs(un[..., 2] * vn[..., 0]) + np.abs(un[..., 0] * vn[..., 2])
        tz = np.abs(un[..., 0] * vn[..., 1]) + np.abs(un[..., 1] * vn[..., 0])
        terms = np.stack([tx, ty, tz], axis=-1)
    normal = np.zeros((H, W, 4))
    normal[..., 3] = np.where(pw, 0.0, 1.0)
    normal[valid, :3] = nn[valid]
    normal[valid, 3] = (ln[valid] > LEN_GATE).astype(np.float64)
    # erosion
    pl = S[..., 0]
    differs = np.zeros((H, W), dtype=bool)
    for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1)):
        nl = _shift(S, dx, dy)[..., 0]
        differs |= (pl != nl) & (nl != 0.0)
    eroded = np.where((pw & ~differs)[..., None], S, np.array([0.0, 0.0, 0.0, 1.0]))
    return dict(normal=normal, eroded=eroded, valid=valid, pw=pw, r1=pw & r1, r2=pw & r2 & ~r3, r3=pw & r3 & ~r1,
                len=ln, m_len=np.where(valid, np.abs(ln - LEN_GATE), np.inf), terms=terms,
                was_eroded=pw & differs & (pl != 0.0))


def normal_bound(k2, c=8.0):
    """c 2^-24 sum|terms| carried through the two normalisations: the cross product's component x is a difference of
    two products of unit-vector components, sum|terms| = T_x; the final normalisation divides by len and adds the
    relative deviation of len (at most sum T / len) on the component itself:
        |n_x - fp64| <= c 2^-24 (T_x + |n_x| (T_x + T_y + T_z)) / len + c 2^-24 |n_x|"""
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.abs(k2["normal"][..., :3])
        T = k2["terms"]
        return c * U * ((T + n * np.sum(T, axis=-1, keepdims=True)) / k2["len"][..., None] + n)


def k3_fp64(V, E):
    """floodfill.frag:34-84 over the ERODED labels: an unlabelled texel takes the label of the first neighbour -- offset
    1 then 2; +x, +y, -x, -y -- that is labelled and whose range lq meets |lp - lq| < 0.007 lp; the probability is
    divided by offset + 1.  Returns refined, fill (0 none, 1, 2), refused (a labelled neighbour failed the range test
    before the texel's fate was settled), all_refused (... and none passed), m_fill."""
    V, E = np.asarray(V, dtype=np.float64), np.asarray(E, dtype=np.float64)
    H, W = V.shape[:2]
    lp = np.linalg.norm(V[..., :3], axis=-1)
    out = E.copy()
    fill = np.zeros((H, W), dtype=np.int64)
    refused = np.zeros((H, W), dtype=bool)
    m_fill = np.full((H, W), np.inf)
    pending = E[..., 0] == 0.0
    for offset in (1, 2):
        for dx, dy in ((offset, 0), (0, offset), (-offset, 0), (0, -offset)):
            q = _shift(E, dx, dy)
            lq = _shift(lp[..., None], dx, dy)[..., 0]
            cand = pending & (q[..., 0] != 0.0)
            diff, thr = np.abs(lp - lq), FILL_THRESHOLD * lp
            ok = cand & (diff < thr)
            m_fill = np.where(cand, np.minimum(m_fill, np.abs(diff - thr)), m_fill)
            refused |= cand & ~ok
            out[ok] = np.concatenate([q[ok][:, :3], q[ok][:, 3:4] / (offset + 1.0)], axis=1)
            fill[ok] = offset
            pending = pending & ~ok
    return dict(refined=out, fill=fill, refused=refused, all_refused=refused & (fill == 0), m_fill=m_fill, lp=lp)


def spread(mask, r):
    """texels within the (2r + 1)^2 window (columns wrap, rows cut) of a set texel"""
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out |= _shift(mask[..., None], dx, dy)[..., 0].astype(bool)
    return out
