"""TEST INFRASTRUCTURE: a plain fp64 statement of the surfel update, K8 .. K12 (SurfelMap::update).

Nothing here shares code, operation order or number format with oracle/o_map.c or csrc/k_update.hip: the stage is written
down from what update_surfels.vert / .geom / .frag, init_radiusConf.vert, gen_surfels.vert / .geom, copy_surfels.vert
and extract_surfels.vert mean, in numpy fp64, vectorised over the surfels and the pixels.  The only fp32 in it is what
the stage is GIVEN in fp32 (records, pose table, pose, frame, parameters, the shader's literal 0.9 / 0.1) and the two
decisions the shader takes on a single fp32 product of an input: a label is texel.x * 255, compared after round() and,
for the dynamic classes, with ==.  Integer decisions (ages, active_timestamps) and comparisons of input values as they
are given (confidence < confidence_threshold, texel.w > 0.5) are exact.  numpy only; a helper module, not a conftest.

    consts(params)                                      what SurfelMap::setParameters derives
    update_fp64(params, poses, records, timestamp, pose, frame, origin, pending)
                                                        outcome, margins and values per surfel and per measurement pixel
    decide(r, eps)                                      which surfels / mask pixels / K10 pixels no rounding of size eps changes
    tile_fp64(world, world_terms, params, i, j)         K12's predicate on world-frame positions of the map the update leaves

Documented deviation kept: slerp of normals with sin(omega) not > 0 returns v0.
"""
from __future__ import annotations

import numpy as np

import render_ref as R
from k6_ref import DYNAMIC_LABELS

GREY, GREEN, MAGENTA, CYAN, DELETED = 0, 1, 2, 3, 4
OUTCOMES = ("grey", "green", "magenta", "cyan", "deleted")
U = 2.0 ** -24
MARGINS = ("texel", "front", "imz", "zclip", "distance", "angle", "radius", "label", "conf", "winner", "slerp")


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def consts(q):
    vfov = abs(float(q.data_fov_up)) + abs(float(q.data_fov_down))
    pu = 1.0 - float(q.p_stable)
    pp = float(q.p_prior)
    return dict(pixel_size=max(np.tan(0.5 * np.deg2rad(vfov) / q.data_height), np.tan(0.5 * 2 * np.pi / q.data_width)),
                p_unstable=pu, log_prior=np.log(pp / (1 - pp)), log_unstable=np.log(pu / (1 - pu)),
                radconf_thresh=np.cos(np.deg2rad(float(q.max_angle))), angle_thresh=np.sin(np.deg2rad(float(q.map_max_angle))))


def _label(x):
    """texel.x * 255 as the shader forms it: one fp32 product of an input"""
    return (np.asarray(x, dtype=np.float32) * np.float32(255.0)).astype(np.float64)


def _round(x):
    return np.floor(x + 0.5)


def _dynamic(label):
    return np.isin(label, np.asarray(DYNAMIC_LABELS, dtype=np.float64))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _signed(ts):
    ts = np.asarray(ts).astype(np.int64)
    return np.where(ts >= 2 ** 31, ts - 2 ** 32, ts)


def _slerp(v0, v1, weight):
    """update_surfels.vert slerp(): `weight` belongs to v0"""
    omega = np.arccos(np.sum(_unit(v0) * _unit(v1), axis=-1))
    so = np.sin(omega)
    eta = 1.0 / so
    out = (eta * np.sin(weight * omega))[:, None] * v0 + (eta * np.sin((1.0 - weight) * omega))[:, None] * v1
    return np.where((so > 0)[:, None], out, v0)


def area(q, origin, pending):
    """K11's centre and extent (SurfelMap.cpp:667-677); the products are formed in fp32 as the host code forms them"""
    ext, dim = np.float32(q.submap_extent), np.float32(q.submap_dimension)
    E = np.float32(2.0) * dim * ext + ext
    if q.partial_extraction and pending:
        E = E + np.float32(2.0) * ext
    return float(np.float32(2.0 * origin[0] * float(ext))), float(np.float32(2.0 * origin[1] * float(ext))), float(E)


def _area_test(pw, terms, ts, cx, cy, E, with_stamp):
    """(kept, margin, eps): |x - cx| > E or |y - cy| > E drops; eps is the rounding of the fp32 chain that forms
    |x - cx| -- 8 * 2^-24 * (sum|terms| + |c| + E) -- doubled for the comparison's two sides"""
    dx, dy = np.abs(pw[:, 0] - cx), np.abs(pw[:, 1] - cy)
    out = (dx > E) | (dy > E)
    if with_stamp:
        out = out | (ts < 0)
    margin = np.minimum(np.abs(dx - E), np.abs(dy - E))
    margin = np.where(np.isfinite(margin), margin, np.inf)
    eps = 16 * U * (np.maximum(terms[:, 0] + abs(cx), terms[:, 1] + abs(cy)) + E)
    if with_stamp:
        margin = np.where(ts < 0, np.inf, margin)  # the stamp alone decides: exact
    return ~out, margin, eps


def update_fp64(q, poses, rec, timestamp, pose, frame, origin=(0, 0), pending=False):
    """One SurfelMap::update in fp64.  poses: (max_poses, 4, 4); rec: SURFEL_DTYPE records; frame: (vertex, normal,
    semantic) maps H x W x 4; origin / pending: the submap origin and whether an extraction is pending BEFORE the update.
    Returns a dict; per surfel (n): outcome, keep, mark, texel (tx, ty), margins{name: (n)}, pos / nrm / radius /
    confidence / weight / prob / stamp / creation and pos_terms / prob_terms / weight_terms, in_area + area_margin +
    area_eps, world; per pixel (H x W): radius, radius_terms, k8_valid, k8_margin, mask, gen, gen_margin, and the new
    surfels' values new_*; final order: survivors (ids), new (pixels, x-major)."""
    k = consts(q)
    W, H = int(q.data_width), int(q.data_height)
    V, N, S = (_f64(m) for m in frame[:3])
    Sraw = np.asarray(frame[2], dtype=np.float32)
    P = _f64(poses).copy()
    T = _f64(pose)
    if timestamp < len(P):
        P[timestamp] = T
    n = len(rec)
    Rt, tt = T[:3, :3], T[:3, 3]
    out = dict(W=W, H=H, n=n, consts=k, timestamp=timestamp)
    with np.errstate(all="ignore"):
        # ---- K8: the radius a measurement would have as a surfel --------------------------------------------------
        v3, n3 = V[..., :3], N[..., :3]
        d = np.linalg.norm(v3, axis=-1)
        view = -v3 / d[..., None]
        cosang = np.sum(n3 * view, axis=-1)
        w_ok = (V[..., 3] > 0.5) & (N[..., 3] > 0.5)
        k8_valid = w_ok & (cosang > k["radconf_thresh"])
        cl = np.clip(cosang, 0.5, 1.0)
        rad = np.clip(1.41 * d * k["pixel_size"] / cl, float(q.min_radius), float(q.max_radius))
        rad = np.where(k8_valid, rad, 0.0)
        amp = np.where((cosang > 0.5) & (cosang < 1.0), np.sum(np.abs(n3 * view), axis=-1) / cl, 1.0)
        out.update(radius_map=rad, radius_terms=rad * (1.0 + amp), k8_valid=k8_valid,
                   k8_margin=np.where(w_ok & np.isfinite(cosang), np.abs(cosang - k["radconf_thresh"]), np.inf))

        # ---- K7 -----------------------------------------------------------------------------------------------------
        if n:
            index, index_dec = R.indexmap_fp64(q, P, rec, T)
        else:
            index, index_dec = np.zeros((H, W), np.int64), np.ones((H, W), bool)
        out.update(index=index, index_decided=index_dec)

        # ---- K9 -----------------------------------------------------------------------------------------------------
        creation = rec["count"].astype(np.float64).astype(np.int64)
        Ps = P[creation] if n else np.zeros((0, 4, 4))
        Rs, ts_ = Ps[:, :3, :3], Ps[:, :3, 3]
        pl = np.stack([_f64(rec[c]) for c in ("x", "y", "z")], -1).reshape(n, 3)
        nl = np.stack([_f64(rec[c]) for c in ("nx", "ny", "nz")], -1).reshape(n, 3)
        op = np.einsum("nij,nj->ni", Rs, pl) + ts_
        on = np.einsum("nij,nj->ni", Rs, nl)
        op_terms = np.einsum("nij,nj->ni", np.abs(Rs), np.abs(pl)) + np.abs(ts_)
        old_radius, old_conf, old_weight = _f64(rec["radius"]), _f64(rec["confidence"]), _f64(rec["weight"])
        stamp = _signed(rec["timestamp"])
        age = timestamp - stamp
        use_stab = bool(q.use_stability)
        keep = np.ones(n, bool)
        if use_stab:
            keep = np.where(rec["confidence"] < np.float32(q.confidence_threshold), age < int(q.unstable_age), True)

        vertex = (op - tt) @ Rt
        normal = _unit(on @ Rt)
        front = np.sum(normal * (-vertex / np.linalg.norm(vertex, axis=-1, keepdims=True)), axis=-1)
        visible = front > 0.0
        c = R.project(q.data_fov_up, q.data_fov_down, q.min_depth, q.max_depth, vertex)
        fx, fy, imz = c[:, 0] * W, c[:, 1] * H, c[:, 2]
        finite = np.isfinite(fx) & np.isfinite(fy)
        tx = np.where(finite, np.floor(fx), -1).astype(np.int64)
        ty = np.where(finite, np.floor(fy), -1).astype(np.int64)
        in_tex = finite & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        sx, sy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
        dv = np.where(in_tex[:, None], V[sy, sx], 0.0)
        dn = np.where(in_tex[:, None], N[sy, sx], 0.0)
        valid = (dv[:, 3] > 0.5) & (dn[:, 3] > 0.5)
        imx, imy = tx + 0.5, ty + 0.5
        # quirk B-6, as the shader writes it: all(lessThan(img, dim)) && !all(lessThan(img, 0))
        inside = finite & ((imx < W) & (imy < H) & (imz < 1.0)) & ~((imx < 0) & (imy < 0) & (imz < 0))
        reach = valid & inside & visible

        data_label = np.where(in_tex, _label(Sraw[sy, sx, 0]), 0.0)
        data_prob = np.where(in_tex, S[sy, sx, 3], 0.0)
        model_label, model_prob = _label(rec["r"]), _f64(rec["w"])
        differ = _round(data_label) != _round(model_label)
        penalty = np.where(reach & differ & _dynamic(model_label), 1.0, 0.0)

        v, nn = dv[:, :3], dn[:, :3]
        vg = v @ Rt.T + tt
        vg_terms = np.abs(v) @ np.abs(Rt).T + np.abs(tt)
        ng = _unit(nn @ Rt.T)
        view_dir = -v / np.linalg.norm(v, axis=-1, keepdims=True)
        distance = np.abs(np.sum(on * (vg - op), axis=-1))
        angle = np.linalg.norm(np.cross(ng, on), axis=-1)
        new_radius = np.where(in_tex, rad[sy, sx], 0.0)
        match = reach & (distance < float(q.map_max_distance)) & (angle < k["angle_thresh"])
        age_ok = (timestamp - creation) < int(q.active_timestamps)
        averaged = match & (((new_radius < old_radius) & age_ok) | bool(q.update_always))

        ps = np.full(n, float(q.p_stable))
        if q.confidence_mode in (1, 3):
            ps = ps * np.exp(-angle * angle / float(q.sigma_angle) ** 2)
        if q.confidence_mode in (2, 3):
            ps = ps * np.exp(-distance * distance / float(q.sigma_distance) ** 2)
        ps = np.clip(ps, k["p_unstable"], 1.0)
        winner = reach & ~match & (index[sy, sx] - 1 == np.arange(n))
        upd = np.where(match, np.log(ps / (1.0 - ps)), np.where(winner, k["log_unstable"], k["log_prior"])) - penalty
        pre_cap = old_conf + upd - k["log_prior"]
        conf = np.minimum(pre_cap, 20.0) if use_stab else old_conf
        keep = np.where(match, True, keep)
        if use_stab:
            keep = keep & ~(conf < k["log_unstable"])
        colour = np.where(averaged, MAGENTA, np.where(match, GREEN, np.where(winner, CYAN, GREY)))
        outcome = np.where(keep, colour, DELETED)
        mark = match & keep & (imz >= 0.0) & (imz <= 1.0)

        # values
        radius = np.where(match, np.maximum(np.minimum(new_radius, old_radius), 0.0), old_radius)
        new_stamp = np.where(match, timestamp, stamp)
        w1 = np.full(n, float(np.float32(0.9)))
        w2 = np.full(n, float(np.float32(0.1)))
        weight = old_weight.copy()
        weight_terms = np.abs(old_weight)
        if q.weighting_scheme > 0:
            w1 = old_weight
            w2 = np.sum(nn * view_dir, axis=-1) if q.weighting_scheme == 2 else np.ones(n)
            w2_terms = np.sum(np.abs(nn * view_dir), axis=-1) if q.weighting_scheme == 2 else np.ones(n)
            weight = np.where(averaged, np.minimum(float(q.max_weight), w1 + w2), old_weight)
            weight_terms = np.abs(old_weight) + w2_terms
            w1, w2 = w1 / (w1 + w2), w2 / (w1 + w2)
        if q.averaging_scheme == 1:
            avg_p = op + (w2 * distance)[:, None] * on
            avg_terms = op_terms + np.abs(w2 * distance)[:, None] * np.abs(on)
        else:
            avg_p = w1[:, None] * op + w2[:, None] * vg
            avg_terms = np.abs(w1)[:, None] * op_terms + np.abs(w2)[:, None] * vg_terms
        avg_n = _unit(_slerp(on, ng, w1))
        back_p = np.einsum("nji,nj->ni", Rs, avg_p - ts_)
        back_terms = np.einsum("nji,nj->ni", np.abs(Rs), avg_terms + np.abs(ts_))
        back_n = np.einsum("nji,nj->ni", Rs, avg_n)
        pos = np.where(averaged[:, None], back_p, pl)
        pos_terms = np.where(averaged[:, None], back_terms, 0.0)
        nrm = np.where(averaged[:, None], back_n, nl)
        prob_in = np.where(differ, 1.0 - data_prob, data_prob)
        prob = np.where(averaged, w1 * model_prob + w2 * prob_in, model_prob)
        prob_terms = np.where(averaged, np.abs(w1 * model_prob) + np.abs(w2) * (np.abs(data_prob) + differ), 0.0)

        # margins: inf where the decision is not taken (or is exact)
        near = finite & (fx > -1) & (fx < W + 1) & (fy > -1) & (fy < H + 1)
        inf = np.inf
        fr = lambda x: np.abs(x - np.floor(x) - 0.5)  # noqa: E731  distance of a label from the rounding step
        m = dict(
            texel=np.where(near, np.minimum(np.abs(fx - np.rint(fx)), np.abs(fy - np.rint(fy))), inf),
            front=np.where(valid & np.isfinite(front), np.abs(front), inf),
            imz=np.where(valid & visible & np.isfinite(imz), np.abs(imz - 1.0), inf),
            zclip=np.where(match, np.minimum(np.abs(imz), np.abs(1.0 - imz)), inf),
            distance=np.where(reach & np.isfinite(distance), np.abs(distance - float(q.map_max_distance)), inf),
            angle=np.where(reach & np.isfinite(angle), np.abs(angle - k["angle_thresh"]), inf),
            radius=np.where(match & age_ok & (not q.update_always), np.abs(new_radius - old_radius), inf),
            label=np.where(reach, np.minimum(fr(data_label), fr(model_label)), inf),
            conf=np.where(use_stab & np.isfinite(conf), np.abs(conf - k["log_unstable"]), inf),
            winner=np.where(reach & ~match & ~index_dec[sy, sx], 0.0, inf),
            slerp=np.where(averaged, np.arccos(np.clip(np.sum(_unit(on) * ng, axis=-1), -1.0, 1.0)), inf),
        )
        cap_margin = np.where(np.isfinite(pre_cap), np.abs(pre_cap - 20.0), inf)

        # ---- the integration mask and K10 ---------------------------------------------------------------------------
        mask = np.zeros((H, W), bool)
        mask[sy[mark], sx[mark]] = True
        invalid = (V[..., 3] < 1.0) | (N[..., 3] < 1.0) | ~k8_valid
        dot10 = np.sum(n3 * view, axis=-1)
        gen = ~invalid & ~mask & (dot10 > 0.01)
        gen_margin = np.where(invalid & ~((V[..., 3] >= 1.0) & (N[..., 3] >= 1.0)), inf,
                              np.minimum(np.where(np.isfinite(dot10), np.abs(dot10 - 0.01), inf), out["k8_margin"]))
        new_label = _label(Sraw[..., 0])
        new_conf = np.where(_dynamic(new_label), k["log_prior"] - 0.5, k["log_prior"])
        new_world = v3 @ Rt.T + tt
        new_world_terms = np.abs(v3) @ np.abs(Rt).T + np.abs(tt)

        # ---- K11 ----------------------------------------------------------------------------------------------------
        cx, cy, E = area(q, origin, pending)
        world = np.einsum("nij,nj->ni", Rs, pos) + ts_
        world_terms = np.einsum("nij,nj->ni", np.abs(Rs), np.abs(pos) + pos_terms * 8 * U) + np.abs(ts_)
        in_area, area_margin, area_eps = _area_test(world, world_terms, new_stamp, cx, cy, E, True)
        px = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="ij"), -1).reshape(-1, 2)  # x-major
        nw = new_world[px[:, 1], px[:, 0]]
        nwt = new_world_terms[px[:, 1], px[:, 0]]
        new_in, new_margin, new_eps = _area_test(nw, nwt, np.full(len(px), timestamp), cx, cy, E, True)

    out.update(outcome=outcome, keep=keep, mark=mark, match=match, averaged=averaged, winner=winner, reach=reach,
               tx=tx, ty=ty, in_tex=in_tex, fx=fx, fy=fy, imz=imz, front=front, distance=distance, angle=angle,
               new_radius=new_radius, pre_cap=pre_cap, cap_margin=cap_margin, margins=m,
               pos=pos, pos_terms=pos_terms, nrm=nrm, radius=radius, confidence=conf, weight=weight,
               weight_terms=weight_terms, prob=prob, prob_terms=prob_terms, stamp=new_stamp, creation=creation,
               world=world, world_terms=world_terms, in_area=in_area, area_margin=area_margin, area_eps=area_eps,
               mask=mask, gen=gen, gen_margin=gen_margin, new_conf=new_conf, new_normal=_unit_safe(n3),
               pixels=px, new_world=nw, new_world_terms=nwt, new_in_area=new_in, new_area_margin=new_margin,
               new_area_eps=new_eps, area=(cx, cy, E))
    return out


def _unit_safe(v):
    with np.errstate(all="ignore"):
        return _unit(v)


# the debug terms the oracle exports (ora_debug_update_terms), in its column order, against this module's fields
TERM_FIELDS = ("fx", "fy", "imz", "front", "distance", "angle", "new_radius", "pre_cap")
# which measured term bounds which margin
EPS_OF = dict(texel="texel", front="front", imz="imz", zclip="imz", distance="distance", angle="angle", radius="radius",
              label=None, conf="conf", winner=None, slerp=None)


def measure_eps(r, terms):
    """EPS per decision: 2 x the largest |oracle - fp64| of the compared term over the surfels that form it (the factor
    2: the comparison's other side carries an error of the same size); the texel coordinates also get one fp32 ulp of
    the largest coordinate, for the floor.  `terms` is the oracle's export, n x 8."""
    t = np.asarray(terms, dtype=np.float64)
    dev = {}
    for col, name in enumerate(TERM_FIELDS):
        ref = np.asarray(r[name], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            dlt = np.abs(t[:, col] - ref)
        ok = np.isfinite(dlt)
        if name in ("distance", "angle", "new_radius"):
            ok &= r["reach"]
        dev[name] = float(dlt[ok].max()) if ok.any() else 0.0
    ulp = float(np.spacing(np.float32(max(r["W"], r["H"]))))
    return dict(texel=2 * max(dev["fx"], dev["fy"]) + ulp, front=2 * dev["front"], imz=2 * dev["imz"],
                distance=2 * dev["distance"], angle=2 * dev["angle"], radius=2 * dev["new_radius"],
                conf=2 * dev["pre_cap"])


LABEL_EPS = 1e-3   # a label this close to a rounding step would need an error of 16 ulps of 255 in ONE fp32 product
# slerp's sin(omega) > 0 (quirk B-12: v0 otherwise): the fp32 dot of two normalised vectors is off by at most 8 * 2^-24, so it
# stays below 1 -- and omega above 0 -- once 1 - cos(omega) = omega^2 / 2 exceeds that
SLERP_EPS = float(np.sqrt(2 * 8 * U))
K10_EPS = 16 * U   # dot(n, -v/|v|) of inputs of magnitude <= 1: a handful of fp32 roundings, against 0.01 and cos(max_angle)


def decide(r, eps):
    """(surfel decided (n), its final-map membership decided (n), mask pixel decided (H x W), K10 pixel decided (H x W),
    new surfel's membership decided (W * H, x-major))"""
    n, W, H = r["n"], r["W"], r["H"]
    dec = np.ones(n, bool)
    for name, mg in r["margins"].items():
        key = EPS_OF[name]
        bound = LABEL_EPS if name == "label" else SLERP_EPS if name == "slerp" else (0.0 if key is None else eps[key])
        if name == "zclip":
            bound = bound + U  # z_ndc = 2 imz - 1 is rounded once more before it meets +-1: half an ulp of 1, halved again in imz
        dec &= mg > bound
    member = dec & (~r["keep"] | (r["area_margin"] > r["area_eps"]))
    mask_dec = np.ones((H, W), bool)
    tex_bad = ~(r["margins"]["texel"] > eps["texel"])
    for i in np.flatnonzero(~dec & np.isfinite(r["fx"]) & np.isfinite(r["fy"])):
        x, y = int(r["tx"][i]), int(r["ty"][i])
        if tex_bad[i]:
            mask_dec[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = False
        elif r["in_tex"][i]:
            mask_dec[y, x] = False
    gen_dec = mask_dec & (r["gen_margin"] > K10_EPS)
    new_member = gen_dec[r["pixels"][:, 1], r["pixels"][:, 0]] & (r["new_area_margin"] > r["new_area_eps"])
    return dec, member, mask_dec, gen_dec, new_member


def tile_fp64(world, world_terms, q, i, j):
    """K12 (extract_surfels.vert): (in tile, margin, eps) of records at `world` for submap tile (i, j)"""
    ext = float(np.float32(q.submap_extent))
    cx, cy = float(np.float32(2.0 * i * ext)), float(np.float32(2.0 * j * ext))
    return _area_test(world, world_terms, np.zeros(len(world), np.int64), cx, cy, ext, False)
