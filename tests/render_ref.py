"""TEST INFRASTRUCTURE: a plain fp64 statement of K4 (surfel rendering) + K5 (compose) and the K7 index-map splat.

Nothing here shares code, operation order or number format with oracle/o_map.c or csrc/k_render.hip: the stage is written
down from what render_surfels.vert / .geom / .frag and render_compose.frag mean -- a surfel is a disc of radius r around
p with normal n, drawn as the screen-space quad of its four tangent-plane corners, each projected spherically; a pixel
belongs to the nearest disc that covers its centre -- in numpy fp64, with CONTINUOUS (unsnapped) edge functions.  The
only fp32 in it is what the stage is GIVEN in fp32 (records, pose table, view pose).  numpy only; a helper module, not a
conftest.

    quads_fp64(params, poses, records, view)        per surfel: sensor-frame position / normal, gates, four corners
    selected(params, records, mode, thr, ct)        the stability and age gates (exact: integer / fp32 compares of inputs)
    raster_fp64(W, H, passes)                       winners per pixel centre and the three margins
    compose_fp64(old, new)                          the K5 select on two winner maps
    decided(r, eps_px, eps_z)                       the pixels whose winner no snapping / rounding of size eps can change
    indexmap_fp64(params, poses, records, view)     K7: nearest front-facing surfel per data texel
"""
from __future__ import annotations

import numpy as np

GATE_EPS = 1e-5  # a front-face / centre-in-image gate decided by less than this makes the surfel's whole box undecided
OLD, NEW = 0, 1  # render modes: creation < thr; creation >= thr or timestamp >= thr


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def project(fov_up, fov_down, min_depth, max_depth, p):
    """spherical projection of points (.., 3) -> (x01, y01, z01), yaw 0 at x01 = 0.5, +pi / -pi at x01 = 0 / 1"""
    fov_up, fov_down = abs(float(fov_up)), abs(float(fov_down))
    with np.errstate(all="ignore"):
        depth = np.linalg.norm(p, axis=-1)
        yaw = np.arctan2(p[..., 1], p[..., 0])
        pitch = -np.arcsin(p[..., 2] / depth)
        x = 0.5 * (1.0 - yaw / np.pi)
        y = 1.0 - (np.rad2deg(pitch) + fov_up) / (fov_up + fov_down)
        z = (depth - float(min_depth)) / (float(max_depth) - float(min_depth))
    return np.stack([x, y, z], axis=-1)


def _to_sensor(poses, records, view):
    """(inv(view) * poses[creation]) * (p, 1) and * (n, 0) in fp64, and the sum of |terms| of each component when the
    two chained 4-term products (and the inverse's own -R^T t) are written out"""
    view = _f64(view)
    R, t = view[:3, :3], view[:3, 3]
    inv = np.eye(4)
    inv[:3, :3], inv[:3, 3] = R.T, -R.T @ t
    ainv = np.zeros((4, 4))
    ainv[:3, :3], ainv[:3, 3], ainv[3, 3] = np.abs(R.T), np.abs(R.T) @ np.abs(t), 1.0
    c = records["count"].astype(np.float64).astype(np.int64)
    Ps = _f64(poses)[c]  # n x 4 x 4
    M = inv[None] @ Ps
    aM = ainv[None] @ np.abs(Ps)
    p = np.stack([_f64(records[k]) for k in ("x", "y", "z")], axis=-1)
    n = np.stack([_f64(records[k]) for k in ("nx", "ny", "nz")], axis=-1)
    with np.errstate(all="ignore"):
        pos = np.einsum("nij,nj->ni", M[:, :3, :3], p) + M[:, :3, 3]
        nrm = np.einsum("nij,nj->ni", M[:, :3, :3], n)
        pos_terms = np.einsum("nij,nj->ni", aM[:, :3, :3], np.abs(p)) + aM[:, :3, 3]
        nrm_terms = np.einsum("nij,nj->ni", aM[:, :3, :3], np.abs(n))
    return pos, nrm, pos_terms, nrm_terms


def quads_fp64(params, poses, records, view, data_image=False):
    """per surfel, seen from `view` (4 x 4, sensor -> world):
    pos, nrm (n x 3) and pos_terms, nrm_terms; front = n . (-p / |p|); centre (x01, y01, z01);
    geometric = front-facing by > 0.01, centre inside [0, 1)^3, every corner finite;
    gate_margin = the smallest distance by which one of those comparisons was decided;
    xy (n x 4 x 2) the corners in window pixels, x unwrapped to the centre's side of the seam; z (n x 4) window depth."""
    q = params
    if data_image:
        proj = (q.data_fov_up, q.data_fov_down, q.min_depth, q.max_depth)
        W, H = int(q.data_width), int(q.data_height)
    else:
        proj = (q.model_fov_up, q.model_fov_down, q.model_min_depth, q.model_max_depth)
        W, H = int(q.model_width), int(q.model_height)
    pos, nrm, pos_terms, nrm_terms = _to_sensor(poses, records, view)
    r = _f64(records["radius"])
    with np.errstate(all="ignore"):
        front = np.sum(nrm * (-pos / np.linalg.norm(pos, axis=1, keepdims=True)), axis=1)
        centre = project(*proj, pos)
        u = np.stack([nrm[:, 1] - nrm[:, 2], -nrm[:, 0], nrm[:, 0]], axis=1)
        u = u / np.linalg.norm(u, axis=1, keepdims=True)
        v = np.cross(nrm, u)
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
        ru, rv = r[:, None] * u, r[:, None] * v
        corners = np.stack([pos - ru - rv, pos + ru - rv, pos - ru + rv, pos + ru + rv], axis=1)
        pr = project(*proj, corners)
        x = pr[..., 0]
        x = np.where(centre[:, None, 0] - x > 0.5, x + 1.0, x)
        x = np.where(x - centre[:, None, 0] > 0.5, x - 1.0, x)
        xy = np.stack([x * W, pr[..., 1] * H], axis=-1)
        z = pr[..., 2]
        inside = np.all((centre >= 0.0) & (centre < 1.0), axis=1)
        finite = np.all(np.isfinite(xy), axis=(1, 2)) & np.all(np.isfinite(z), axis=1) & np.isfinite(front)
        geometric = (front > 0.01) & inside & finite
        m = np.minimum(np.abs(front - 0.01), np.min(np.minimum(np.abs(centre), np.abs(1.0 - centre)), axis=1))
    gate_margin = np.where(np.isfinite(m), m, np.inf)  # a NaN compares false everywhere: decided
    return dict(pos=pos, nrm=nrm, pos_terms=pos_terms, nrm_terms=nrm_terms, front=front, centre=centre,
                geometric=geometric, finite=finite, gate_margin=gate_margin, xy=xy, z=z, W=W, H=H)


def selected(params, records, mode, thr, conf_threshold):
    """stability and age gates of render_surfels.geom: comparisons of the inputs as given, nothing to round"""
    creation = records["count"].astype(np.float64).astype(np.int64)
    ts = records["timestamp"].astype(np.int64)
    ts = np.where(ts >= 2 ** 31, ts - 2 ** 32, ts)  # the shader reads a signed int
    with np.errstate(invalid="ignore"):
        stable = (records["confidence"] > np.float32(conf_threshold)) if params.use_stability else np.ones(len(records), bool)
    age = (creation < thr) if mode == OLD else ((creation >= thr) | (ts >= thr))
    return stable & age


def _seg_dist(px, py, a, b):
    """distance of the points (px, py) from the segment a-b"""
    d = b - a
    L2 = float(d @ d)
    if L2 == 0.0:
        return np.hypot(px - a[0], py - a[1])
    s = np.clip(((px - a[0]) * d[0] + (py - a[1]) * d[1]) / L2, 0.0, 1.0)
    return np.hypot(px - (a[0] + s * d[0]), py - (a[1] + s * d[1]))


def _triangle(px, py, A, B, C, attrs):
    """(inside, [attr at the pixels], [|grad attr|], weight of A) of the affine map over triangle A, B, C; attrs: k x 3 corner values"""
    E = np.array([B - A, C - A])
    det = E[0, 0] * E[1, 1] - E[0, 1] * E[1, 0]
    if det == 0.0:
        return None
    Ei = np.array([[E[1, 1], -E[0, 1]], [-E[1, 0], E[0, 0]]]) / det
    dx, dy = px - A[0], py - A[1]
    b1 = dx * Ei[0, 0] + dy * Ei[1, 0]
    b2 = dx * Ei[0, 1] + dy * Ei[1, 1]
    b0 = 1.0 - b1 - b2
    tol = -1e-12  # a centre exactly on the strip's shared diagonal belongs to the quad whatever fp64 rounds the weight to
    inside = (b0 >= tol) & (b1 >= tol) & (b2 >= tol)
    vals, grads = [], []
    for a in attrs:
        vals.append(b0 * a[0] + b1 * a[1] + b2 * a[2])
        grads.append(float(np.linalg.norm(Ei @ np.array([a[1] - a[0], a[2] - a[0]]))))
    return inside, vals, grads, b0


def _narrowest(xy):
    """the quad's smallest extent [px] across a pair of opposite sides (tu or tv runs from -1 to 1 over it): for a
    slanted quad far less than its shortest side"""
    def off(a, b, c):  # distance of c from the line a-b
        d = b - a
        return abs(d[0] * (c[1] - a[1]) - d[1] * (c[0] - a[0])) / max(float(np.hypot(*d)), 1e-300)
    return min(off(xy[0], xy[1], xy[2]), off(xy[0], xy[1], xy[3]), off(xy[2], xy[3], xy[0]), off(xy[2], xy[3], xy[1]),
               off(xy[0], xy[2], xy[1]), off(xy[0], xy[2], xy[3]), off(xy[1], xy[3], xy[0]), off(xy[1], xy[3], xy[2]))


TU = np.array([-1.0, 1.0, -1.0, 1.0])
TV = np.array([-1.0, -1.0, 1.0, 1.0])


Z_CONTEND, PX_CONTEND = 1e-5, 1e-2  # see raster_fp64: every eps_z / eps_px handed to decided() must stay below these


def _quad_fields(xy, z, i0, i1, j0, j1):
    """over the pixel centres of a box: distance from the outline, coverage, and tu^2 + tv^2, z, |grad z| of the strip's
    piecewise affine map -- continued beyond the outline with the triangle on the pixel's side of the shared diagonal"""
    px, py = np.meshgrid(np.arange(i0, i1 + 1) + 0.5, np.arange(j0, j1 + 1) + 0.5)
    e = np.minimum(np.minimum(_seg_dist(px, py, xy[0], xy[1]), _seg_dist(px, py, xy[1], xy[3])),
                   np.minimum(_seg_dist(px, py, xy[3], xy[2]), _seg_dist(px, py, xy[2], xy[0])))
    t1 = _triangle(px, py, xy[0], xy[1], xy[2], (TU[[0, 1, 2]], TV[[0, 1, 2]], z[[0, 1, 2]]))
    t2 = _triangle(px, py, xy[2], xy[1], xy[3], (TU[[2, 1, 3]], TV[[2, 1, 3]], z[[2, 1, 3]]))
    if t1 is None and t2 is None:
        return None
    t1, t2 = t1 or t2, t2 or t1
    first = t1[3] >= 0  # barycentric weight of v0: on the first triangle's side of the diagonal v1-v2
    cov = t1[0] | t2[0]
    pick = lambda a, b: np.where(t1[0] | (first & ~t2[0]), a, b)
    r2 = pick(t1[1][0] ** 2 + t1[1][1] ** 2, t2[1][0] ** 2 + t2[1][1] ** 2)
    zz = pick(t1[1][2], t2[1][2])
    gz = pick(t1[2][2], t2[2][2])
    return e, cov, r2, zz, gz


def raster_fp64(W, H, passes):
    """passes: list of (quads, sel) drawn into ONE depth buffer; sel = selected(): the surfels the pass's stability and
    age gates let through (the geometric gates are in the quads).  Per pixel (H x W):
      winner, winner_pass   id / pass index of the smallest-z fragment, -1 where there is none
      z                     its window depth
      touched               some quad's box (grown by one pixel) holds the pixel centre
      edge                  smallest distance [px] of the centre from an outline edge of a CONTENDING quad
      disc                  smallest |tu^2 + tv^2 - 1| * (narrowest extent [px]) / 6 among the contenders covering the centre:
                            the distance [px] the corners would have to move to flip the disc test.  Moving every corner
                            by d moves tu at a fixed pixel by at most |grad tu| d (the barycentric weights sum to one),
                            |grad tu| <= 2 / extent, so tu^2 + tv^2 moves by at most 4 (|tu| + |tv|) d / extent
                            <= 4 sqrt(2) d / extent at the rim; 6 > 4 sqrt(2)
      zgap                  z of the runner-up (another surfel's fragment) minus z of the winner; also capped by the
                            distance of a contender's fragment from the clip planes z = 0, 1
      zslope                sum over the two of |grad z| per pixel: what a shift of the quads does to the gap
    A quad CONTENDS at a pixel its box touches unless its depth there (the affine map, continued beyond the outline) lies
    behind the winner by more than Z_CONTEND + PX_CONTEND * (sum of the two slopes): whether such a quad covers the
    centre or passes the disc test cannot change the pixel.  Its outline counts only where the disc test is not failed
    by more than PX_CONTEND already (tu^2 + tv^2 is continued across the outline): elsewhere there is no fragment on either
    side of it -- the disc touches the outline at the four side midpoints only.  Without these restrictions no scene with one surfel per texel
    could be 98 % decided: n quads of perimeter p put n * p * 2 EPS_PX pixels within EPS_PX of an outline -- 576 quads of
    12 px on 576 pixels at EPS_PX = 1 / 512 is 4.7 % from the outlines alone, and as much again from the rims."""
    winner = np.full((H, W), -1, dtype=np.int64)
    wpass = np.full((H, W), -1, dtype=np.int64)
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    bslope = np.zeros((H, W))
    sslope = np.zeros((H, W))
    clip = np.full((H, W), np.inf)
    edge = np.full((H, W), np.inf)
    disc = np.full((H, W), np.inf)
    touched = np.zeros((H, W), dtype=bool)
    kept = []
    for k, (Q, sel) in enumerate(passes):
        marginal = sel & Q["finite"] & (Q["gate_margin"] < GATE_EPS)
        draw = sel & Q["geometric"]
        for i in np.flatnonzero(draw | marginal):
            xy, z = Q["xy"][i], Q["z"][i]
            i0, i1 = int(np.floor(xy[:, 0].min() - 1.5)), int(np.ceil(xy[:, 0].max() + 0.5))
            j0, j1 = int(np.floor(xy[:, 1].min() - 1.5)), int(np.ceil(xy[:, 1].max() + 0.5))
            i0, j0, i1, j1 = max(i0, 0), max(j0, 0), min(i1, W - 1), min(j1, H - 1)
            if i0 > i1 or j0 > j1:
                continue
            sl = (slice(j0, j1 + 1), slice(i0, i1 + 1))
            touched[sl] = True
            if marginal[i]:  # whether this surfel is drawn at all hangs on a rounding
                edge[sl] = 0.0
                continue
            f = _quad_fields(xy, z, i0, i1, j0, j1)
            if f is None:
                continue
            e, cov, r2, zz, gz = f
            side = _narrowest(xy)
            kept.append((sl, e, cov, r2, zz, gz, side))
            frag = cov & (r2 <= 1.0) & (zz >= 0.0) & (zz <= 1.0)
            b, s = best[sl], second[sl]
            wins = frag & (zz < b)
            second[sl] = np.where(wins, b, np.where(frag, np.minimum(s, zz), s))
            sslope[sl] = np.where(wins, bslope[sl], np.where(frag & (zz < s), gz, sslope[sl]))
            best[sl] = np.where(wins, zz, b)
            bslope[sl] = np.where(wins, gz, bslope[sl])
            winner[sl] = np.where(wins, i, winner[sl])
            wpass[sl] = np.where(wins, k, wpass[sl])
    for sl, e, cov, r2, zz, gz, side in kept:
        with np.errstate(invalid="ignore"):
            contends = ~(zz - best[sl] > Z_CONTEND + PX_CONTEND * (gz + bslope[sl]))
        rim_near = (r2 - 1.0) * side / 6.0 <= PX_CONTEND  # else: outside the disc on either side of the outline
        edge[sl] = np.where(contends & rim_near, np.minimum(edge[sl], e), edge[sl])
        disc[sl] = np.where(contends & cov, np.minimum(disc[sl], np.abs(r2 - 1.0) * side / 6.0), disc[sl])
        rim = contends & cov & (r2 <= 1.0)
        clip[sl] = np.where(rim, np.minimum(clip[sl], np.minimum(np.abs(zz), np.abs(1.0 - zz))), clip[sl])
    with np.errstate(invalid="ignore"):
        zgap = np.where(np.isfinite(second), second - best, np.inf)
    zgap = np.minimum(zgap, clip)
    return dict(winner=winner, winner_pass=wpass, z=best, touched=touched, edge=edge, disc=disc, zgap=zgap,
                zslope=bslope + np.where(np.isfinite(second), sslope, 0.0))


def decided(r, eps_px, eps_z):
    """a pixel no quad touches is decided (empty); a touched one when all three margins exceed their bounds"""
    assert eps_px < PX_CONTEND and eps_z < Z_CONTEND, "bounds beyond what raster_fp64's contender rule allows for"
    ok = (r["edge"] > eps_px) & (r["disc"] > eps_px) & (r["zgap"] > eps_z + eps_px * r["zslope"])
    return ~r["touched"] | ok


def compose_fp64(old, new):
    """K5 (render_compose.frag) on two raster_fp64 results: the new rendering where it has a surfel, else the old one.
    (vertex.w < 0.5 holds wherever the new rendering is invalid, so the distance test never decides.)
    Returns (winner, source): source 1 = new, 0 = old, -1 = neither; the margins of both renderings apply."""
    take_old = (new["winner"] < 0) & (old["winner"] >= 0)
    winner = np.where(take_old, old["winner"], new["winner"])
    source = np.where(new["winner"] >= 0, 1, np.where(take_old, 0, -1))
    return winner, source


def indexmap_fp64(params, poses, records, view):
    """K7 (gen_indexmap.vert): every front-facing surfel (no stability / age gate) is a point at its centre's data texel;
    the nearest one owns it.  Returns (index map: id + 1 or 0, decided mask): a texel is undecided when a surfel that
    lands in it -- or within `tex_eps` texels of it -- has a marginal gate, sits within tex_eps of a texel edge, or the
    two nearest are closer in depth than 2^-22."""
    Q = quads_fp64(params, poses, records, view, data_image=True)
    W, H = Q["W"], Q["H"]
    tex_eps = 1e-3
    c = Q["centre"]
    with np.errstate(invalid="ignore"):
        fx, fy = c[:, 0] * W, c[:, 1] * H
        ok = (Q["front"] > 0.01) & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H) & (c[:, 2] >= 0) & (c[:, 2] <= 1)
        near_edge = (np.abs(fx - np.rint(fx)) < tex_eps) | (np.abs(fy - np.rint(fy)) < tex_eps) | \
                    (np.abs(Q["front"] - 0.01) < GATE_EPS) | (np.minimum(np.abs(c[:, 2]), np.abs(1 - c[:, 2])) < 1e-6)
    index = np.zeros((H, W), dtype=np.int64)
    best = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    dec = np.ones((H, W), dtype=bool)
    for i in np.flatnonzero(np.isfinite(fx) & np.isfinite(fy) & np.isfinite(Q["front"])):
        x, y = int(np.floor(fx[i])), int(np.floor(fy[i]))
        if near_edge[i]:
            dec[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
        if not ok[i]:
            continue
        z = c[i, 2]
        if z < best[y, x]:
            second[y, x], best[y, x], index[y, x] = best[y, x], z, i + 1
        else:
            second[y, x] = min(second[y, x], z)
    with np.errstate(invalid="ignore"):
        dec &= ~(np.isfinite(second) & (second - best <= 2.0 ** -22))
    return index, dec
