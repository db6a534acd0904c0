"""TEST INFRASTRUCTURE: a plain fp64 statement of the semantic front end (csrc/k_semantic.hip: ks_scatter, ks_resolve,
ks_unproject) and of RangeNet++'s KNN vote (csrc/k_semantic_knn.hip: kk_pixels, kk_points).

Nothing here shares code or operation order with tests/semantic_shim.c, tests/semantic_knn_shim.c or the kernels: every
stage is written down from what it means (the header comments of the two .hip files, RangeNet++ section III-D, and
KITTIReader.cpp:172-200 of the reference for the argmax rule), in numpy fp64, vectorised over points and pixels.  The only
fp32 in it is what a stage is GIVEN in fp32: points, scores, the parameters, and the KNN weight table, which the host
computes in double and hands to the kernel rounded once (w below is that rounded table, widened again).  numpy only; a
helper module, not a conftest.

    project_fp64(sp, pts)                          per point: range, continuous (u, v), clamped pixel, projected;
                                                   per pixel: winner, runner-up, the five planes; margins
    unproject_fp64(sp, scores, pixel, logits)      label and prob of every point
    pixel_class_fp64(sp, scores, logits)           rule 2 of the KNN: class index and prob of every pixel
    knn_fp64(sp, kp, pts, scores, pixel, proj_idx, logits)   rules 1 - 8

A point or pixel is DECIDED when every margin exceeds its bound, or when the fp32 evaluation is exact for a reason that
fp64 can see (below); then fp32 must take fp64's decision.  What is not decided is compared with the shim only.

Margins and their bounds.  u = 2^-24; a correctly rounded operation is off by at most u relative; tests/test_detmath.py
measures atan2 at 3.5 ulp, asin at 2.30 ulp and exp at 1.0 ulp, an ulp being at most 2 u relative.

  range   depth = sqrt(fma(z, z, fma(y, y, x * x))): three roundings under the root (3 u, halved by it) and the root's
          own: 2.5 u relative, i.e. below RANGE_ULPS = 2.5 fp32 steps of the range.  With two coordinates zero the depth
          is |third| EXACTLY (sqrt(fl(x * x)) = |x| in binary arithmetic): such a range has error 0.
  repr    fp64 has a range where the fp32 squares underflow or overflow.  With the largest |coordinate| in
          [2^-60, 2^60] the largest square is normal and the sum stays below 2^122; what smaller squares lose by
          underflowing is below 2^-149 against 2^-120.  With it below 2^-75 every square rounds to 0 and the specified
          depth is 0; from 2^64 on a square is inf and so is the depth: NOT PROJECTED, stated here as the specification
          states it.  In the two bands between (2^-75 .. 2^-60, 2^60 .. 2^64) the fp32 depth is a subnormal's root or
          may overflow: such points are judged by the shim alone, and so is the whole image they may fall into.
  texel   distance of u from the nearest of 1 .. W-1 and of v from the nearest of 1 .. H-1: the clamp makes 0 and W / H
          harmless, and below 0 and inside [0, 1) are the same pixel.  Bound, per point:
            t = yaw / pi:    |t| (7 u [atan2] + u [pi_f] + u [/])          -- 0 for yaw = 0 (y = 0, x >= 0), exactly
            s = t + 1:       + u |s|  (nothing if t is exact)
            u = 0.5 s W:     W / 2 times that, + u |u| for the product (nothing if s is exact)
            a = z / depth:   |a| (2.5 u + u); 0 for z = 0 and for x = y = 0 (a = +-1 exactly)
            pitch:           asin(min(1, |a| + da)) - asin(|a|)  [asin is convex on [0, 1]]  + 4.6 u |pitch|
            q = (pitch + fdown) / fov:   (dpitch + u fdown + u |pitch + fdown|) / fov + 2 u |q|
            v = (1 - q) H:   H (dq + u |1 - q|) + u |v|
  gap     the winner's range against the runner-up's: decided when the gap exceeds the two range errors, or when the
          two points have the same coordinates (the same fp32 depth: the lower index wins in both), or when both
          ranges are exact.
  top2    logits: the maximum's e is exp(0) = 1; the runner-up takes or ties the maximum only if exp(-gap) (1 + 2 u
          [exp] ) rounds to 1 or above after the division, i.e. gap <= about 3 u.  TOP2_BOUND = 2^-21 (8 u) absolute;
          equal logits (gap 0) are equal operands: e = 1 for both, the last wins in both.
  sel     KNN: the gap between the k-th and the (k + 1)-th d; cut: |d - cutoff| of every selected slot.  Both absolute,
          against the errors of the d involved:  d = |rt - ri| w:  w (err rt + err ri) + u |rt - ri| w + u d.
          rt - ri cancels, so this is in steps of the LARGER range, not of d.  The last two terms vanish when both ranges
          are exact and the difference, resp. the product, is an fp32 number (a correctly rounded operation returns it);
          then d is exact, and a tie or d = cutoff is decided in fp64.  Two slots with the same |rt - ri| and the same
          w have the same d in any arithmetic: the t rule decides in both.

Each bound is multiplied by max(1, 2 x MEASURED), MEASURED being the largest margin, in units of the derived bound, at
which the shim and this file were seen to decide differently (tests/test_semantic_crafted_host.py sweeps points across
column and row boundaries, range pairs and logit pairs across a tie, and d across the cutoff; the figures are in its
docstring).  All are below 0.5, so the derived bounds stand.

Tolerances of the values (decided pixels / points only):
  planes  (v - mean) inv_std: u |v - mean| inv_std + 2 u |result|, for the depth plane + range error x inv_std,
          absolute since depth - mean cancels.
  prob    probabilities: a copy of an fp32 input, exact, the sign of -0 included.  Logits: p = e_max / sum;
          e_j = exp(s_j - m) is off by 2 u + u |s_j - m| relative (the subtraction's rounding goes through exp), the
          sum of C terms by C u, the division by u: p (sum_j p_j (2 u + u |s_j - m|) + (C + 1) u), doubled.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U = 2.0 ** -24
FLT_MAX = float(np.finfo(F32).max)
RANGE_ULPS = 2.5
TOP2_BOUND = 2.0 ** -21
NONE = -1

# the largest margin / derived bound at which the shim and fp64 were seen to differ (host test: test_measured_bounds)
MEASURED = dict(texel=0.10, gap=0.24, top2=0.0, sel=0.21, cut=0.12)


def _scale(kind):
    return max(1.0, 2.0 * MEASURED[kind])


def consts(sp):
    up, down = abs(float(sp.fov_up)), abs(float(sp.fov_down))
    C = int(sp.n_classes)
    return dict(W=int(sp.width), H=int(sp.height), P=int(sp.width) * int(sp.height), C=C,
                fdown=np.radians(down), fov=np.radians(up + down),
                mean=np.array([float(sp.means[c]) for c in range(5)]),
                std=np.array([float(sp.stds[c]) for c in range(5)]),
                # the entry reports the label as a float: (float)label_map[j]
                label=np.array([float(F32(int(sp.label_map[j]))) for j in range(C)]))


def ranges_fp64(pts):
    """-> range, its fp32 error bound (0 where the fp32 depth is exact), valid (finite and > 0), repr_ok"""
    p = np.asarray(pts, dtype=F32).reshape(-1, 4).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rng = np.sqrt(x * x + y * y + z * z)
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        big = np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
        # the fp32 consequence the specification states: every square below 2^-150 rounds to 0 (depth 0), a square of
        # 2^128 or more is inf (depth inf) -- not projected, where fp64 has a range
        valid = finite & (rng > 0) & (big >= 2.0 ** -75) & (big < 2.0 ** 64)
        repr_ok = ~valid | ((big >= 2.0 ** -60) & (big <= 2.0 ** 60))
        on_axis = ((x == 0).astype(int) + (y == 0) + (z == 0)) >= 2
        step = np.spacing(np.where(valid & repr_ok, rng, 1.0).astype(F32)).astype(np.float64)
        err = np.where(on_axis, 0.0, RANGE_ULPS * step)
    return rng, err, valid, repr_ok


def _boundary_margin(c, n):
    """distance of the continuous coordinate c from the nearest of 1 .. n-1"""
    if n <= 1:
        return np.full(c.shape, np.inf)
    return np.abs(c - np.clip(np.rint(c), 1, n - 1))


def _reach(c, err, n):
    """the clamped cells that c +- err may floor to: lo, hi (inclusive)"""
    lo = np.clip(np.floor(c - err), 0, n - 1).astype(np.int64)
    hi = np.clip(np.floor(c + err), 0, n - 1).astype(np.int64)
    return lo, hi


def project_fp64(sp, pts):
    k = consts(sp)
    W, H, P = k["W"], k["H"], k["P"]
    p32 = np.asarray(pts, dtype=F32).reshape(-1, 4)
    p = p32.astype(np.float64)
    n = p.shape[0]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rng, r_err, valid, repr_ok = ranges_fp64(p32)
    with np.errstate(all="ignore"):
        # the SPECIFIED atan2 does not see the sign of a zero: y = -0 is +0 (the seam y = 0, x < 0 is yaw = -pi, column
        # 0), and x = y = 0 (either sign) is yaw 0
        yaw = -np.where((x == 0) & (y == 0), 0.0, np.arctan2(y + 0.0, x))
        a = np.where(valid, z / np.where(valid, rng, 1.0), 0.0)
        pitch = np.arcsin(np.clip(a, -1.0, 1.0))
        t = yaw / np.pi
        u = 0.5 * (t + 1.0) * W
        q = (pitch + k["fdown"]) / k["fov"]
        v = (1.0 - q) * H
        # derived bounds (module docstring)
        e_t = np.abs(t) * 9.0 * U
        e_s = e_t + np.where(e_t > 0, U * np.abs(t + 1.0), 0.0)
        e_u = 0.5 * W * e_s + np.where(e_s > 0, U * np.abs(u), 0.0)
        a_exact = (z == 0) | ((x == 0) & (y == 0))
        da = np.where(a_exact, 0.0, 3.5 * U * np.abs(a))
        e_pitch = (np.arcsin(np.minimum(1.0, np.abs(a) + da)) - np.arcsin(np.abs(a))) + 4.6 * U * np.abs(pitch)
        e_q = (e_pitch + U * k["fdown"] + U * np.abs(pitch + k["fdown"])) / k["fov"] + 2.0 * U * np.abs(q)
        e_v = H * (e_q + U * np.abs(1.0 - q)) + U * np.abs(v)
    ok = valid & repr_ok
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    e_u, e_v = np.where(ok, e_u, 0.0) * _scale("texel"), np.where(ok, e_v, 0.0) * _scale("texel")
    col = np.clip(np.floor(u), 0, W - 1).astype(np.int64)
    row = np.clip(np.floor(v), 0, H - 1).astype(np.int64)
    pixel = np.where(valid, row * W + col, -1)
    m_u, m_v = _boundary_margin(u, W), _boundary_margin(v, H)
    # an exact coordinate (u = W / 2 at yaw 0) floors alike in both, boundary or not
    pt_decided = repr_ok & (~valid | (((m_u > e_u) | (e_u == 0)) & ((m_v > e_v) | (e_v == 0))))

    # per pixel: candidates in (range, index) order; a pixel that an undecided point may fall into is undecided
    px_decided = np.ones(P, bool)
    und = np.nonzero(valid & ~pt_decided)[0]
    for i in und:
        if repr_ok[i]:
            (c0, c1), (r0, r1) = _reach(u[i:i + 1], e_u[i:i + 1], W), _reach(v[i:i + 1], e_v[i:i + 1], H)
            for rr in range(int(r0[0]), int(r1[0]) + 1):
                px_decided[rr * W + int(c0[0]): rr * W + int(c1[0]) + 1] = False
        else:
            px_decided[:] = False  # its direction too is the fp32 arithmetic's alone
    winner, runner = np.full(P, -1, np.int64), np.full(P, -1, np.int64)
    gap = np.full(P, np.inf)
    cand = np.nonzero(valid & pt_decided)[0]
    order = cand[np.lexsort((cand, rng[cand], pixel[cand]))]
    first = np.ones(order.size, bool)
    first[1:] = pixel[order[1:]] != pixel[order[:-1]]
    winner[pixel[order[first]]] = order[first]
    # every other candidate of the pixel against its winner: a copy of the winner (the same coordinates, so the same
    # fp32 depth: the lower index wins in both) is no contest; the runner-up is the nearest that is not one
    wo = winner[pixel[order]]
    copy = (p32[order, :3] == p32[wo, :3]).all(1)
    g = rng[order] - rng[wo]
    exact = (r_err[order] == 0) & (r_err[wo] == 0)
    settled = copy | exact | (g > (r_err[order] + r_err[wo]) * _scale("gap"))
    px_decided[pixel[order[~settled]]] = False
    rivals = order[~copy]
    lead = np.ones(rivals.size, bool)
    lead[1:] = pixel[rivals[1:]] != pixel[rivals[:-1]]
    runner[pixel[rivals[lead]]] = rivals[lead]
    has2 = runner >= 0
    gap[has2] = rng[runner[has2]] - rng[winner[has2]]
    # in steps of the range, for the census
    gap_steps = np.full(P, np.inf)
    gap_steps[has2] = gap[has2] / np.spacing(rng[winner[has2]].astype(F32)).astype(np.float64)

    planes, tol = np.zeros((5, P)), np.zeros((5, P))
    f = winner >= 0
    w_ = winner[f]
    vals = np.stack([rng[w_], p[w_, 0], p[w_, 1], p[w_, 2], p[w_, 3]])
    inv = 1.0 / k["std"][:, None]
    planes[:, f] = (vals - k["mean"][:, None]) * inv
    tol[:, f] = U * np.abs(vals - k["mean"][:, None]) * np.abs(inv) + 2.0 * U * np.abs(planes[:, f])
    tol[0, f] += r_err[w_] * abs(inv[0, 0])
    return dict(range=rng, range_err=r_err, valid=valid, repr_ok=repr_ok, u=u, v=v, e_u=e_u, e_v=e_v, m_u=m_u, m_v=m_v,
                pixel=pixel, pt_decided=pt_decided, px_decided=px_decided, winner=winner, runner=runner, gap=gap,
                gap_steps=gap_steps, planes=planes, tol=tol)


def _softmax_fp64(s):
    """s: C x M float64 of fp32 logits -> p (C x M; NaN where the specified arithmetic gives NaN), its tolerance for the
    maximum, margin top2.  A NaN logit, a +inf (inf - inf) or all -inf (-inf - -inf) make every probability NaN."""
    with np.errstate(all="ignore"):
        m = s.max(0)
        bad = np.isnan(s).any(0) | np.isposinf(m) | np.isneginf(m)
        m_ = np.where(bad, 0.0, m)
        s_ = np.where(bad[None], 0.0, s)
        # s_j - m is an fp32 subtraction: beyond -FLT_MAX it is -inf and e is 0, as it is in fp64 for anything that far
        e = np.exp(s_ - m_[None])
        tot = e.sum(0)
        p = e / tot[None]
        dist = np.where(np.isfinite(s_), np.abs(s_ - m_[None]), 0.0)
        rel = (p * (2.0 * U + U * np.minimum(dist, 200.0))).sum(0) + (s.shape[0] + 1) * U
        tol = 2.0 * p.max(0) * rel
        below = np.where(s_ < m_[None], s_, -np.inf)
        top2 = m_ - below.max(0)  # inf if every logit equals the maximum
        p[:, bad] = np.nan
    return p, np.where(bad, 0.0, tol), np.where(bad, np.inf, top2)


def _last_maximum(s):
    """KITTIReader.cpp:189-200 as a statement: among the scores that are >= 0 (a NaN is not, -0 is) the largest wins, the
    LAST one if several are equal; none >= 0: no class.  -> class index (NONE), prob (the winning score itself, so a -0
    keeps its sign)"""
    C, M = s.shape
    with np.errstate(invalid="ignore"):
        ok = s >= 0
    best = np.where(ok, s, -np.inf).max(0)
    is_best = ok & (s == best[None])
    last = C - 1 - np.argmax(is_best[::-1], axis=0)
    cls = np.where(ok.any(0), last, NONE)
    prob = np.where(cls >= 0, s[np.maximum(cls, 0), np.arange(M)], 0.0)
    return cls, prob


def pixel_class_fp64(sp, scores, logits):
    """-> cls (P; NONE), prob (P, float64), tol (P), decided (P)"""
    k = consts(sp)
    s = np.asarray(scores, dtype=F32).reshape(k["C"], k["P"]).astype(np.float64)
    if not logits:
        cls, prob = _last_maximum(s)
        return cls, prob, np.zeros(k["P"]), np.ones(k["P"], bool)
    p, tol, top2 = _softmax_fp64(s)
    cls, prob = _last_maximum(p)
    return cls, prob, tol, (top2 > TOP2_BOUND * _scale("top2")) | np.isinf(top2)


def unproject_fp64(sp, scores, pixel, logits):
    """-> label, prob, tol, decided per point"""
    k = consts(sp)
    pixel = np.asarray(pixel, dtype=np.int64)
    cls, prob, tol, dec = pixel_class_fp64(sp, scores, logits)
    inside = (pixel >= 0) & (pixel < k["P"])
    q = np.where(inside, pixel, 0)
    has = inside & (cls[q] >= 0)
    label = np.where(has, k["label"][np.maximum(cls[q], 0)], 0.0)
    return label, np.where(has, prob[q], 0.0), np.where(has, tol[q], 0.0), ~inside | dec[q]


def knn_weights_fp64(S, sigma):
    """rule 4; the table the stage is given: rounded once to fp32"""
    R = (S - 1) // 2
    dy, dx = np.divmod(np.arange(S * S), S)
    e = np.exp(-((dx - R) ** 2 + (dy - R) ** 2) / (2.0 * float(F32(sigma)) ** 2))
    return (1.0 - e / np.cumsum(e)[-1]).astype(F32).astype(np.float64)  # cumsum: the sum in t order


def knn_fp64(sp, kp, pts, scores, pixel, proj_idx, logits):
    """rules 1 - 8 -> label, prob, tol, decided, margins sel / cut (per point, absolute, inf where none applies) and the
    point's own fate: `own_bad` marks points with a pixel whose own range is not in (0, FLT_MAX] (rule 3: (0, 0))"""
    k = consts(sp)
    W, H, P = k["W"], k["H"], k["P"]
    S, K = int(kp.search), int(kp.k)
    R, S2 = (S - 1) // 2, S * S
    tc = (S2 - 1) // 2
    cutoff = float(F32(kp.cutoff))
    p32 = np.asarray(pts, dtype=F32).reshape(-1, 4)
    n = p32.shape[0]
    pixel = np.asarray(pixel, dtype=np.int64)
    proj_idx = np.asarray(proj_idx, dtype=np.int64).ravel()
    rng, r_err, valid, repr_ok = ranges_fp64(p32)
    valid = valid & (rng <= FLT_MAX)
    cls, pprob, ptol, pdec = pixel_class_fp64(sp, scores, logits)
    # rule 1: a pixel's range is its winner's, +inf when empty (a winner index outside [0, n) is empty)
    has = (proj_idx >= 0) & (proj_idx < n)
    wi = np.where(has, proj_idx, 0)
    prange = np.where(has, rng[wi] if n else 0.0, np.inf)
    prerr = np.where(has, r_err[wi] if n else 0.0, 0.0)
    pfp32 = has & ~(repr_ok[wi] if n else True)  # the record's range is the fp32 arithmetic's alone
    w = knn_weights_fp64(S, kp.sigma)

    label, prob, tol = np.zeros(n), np.zeros(n), np.zeros(n)
    decided = np.ones(n, bool)
    m_sel, m_cut = np.full(n, np.inf), np.full(n, np.inf)
    e_sel, e_cut = np.zeros(n), np.zeros(n)  # the derived bounds the two margins are held against
    inside = (pixel >= 0) & (pixel < P)
    own_bad = inside & ~valid
    decided &= ~(inside & ~repr_ok)
    act = np.nonzero(inside & valid & repr_ok)[0]
    if act.size == 0:
        return dict(label=label, prob=prob, tol=tol, decided=decided, sel=m_sel, cut=m_cut, sel_err=e_sel,
                    cut_err=e_cut, own_bad=own_bad)
    vv, uu = np.divmod(pixel[act], W)
    dy, dx = np.divmod(np.arange(S2), S)
    yy, xx = vv[:, None] + (dy - R)[None], uu[:, None] + (dx - R)[None]  # columns do not wrap
    inimg = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    q = np.where(inimg, yy * W + xx, 0)
    rt = np.where(inimg, prange[q], 0.0)
    rt_err = np.where(inimg, prerr[q], 0.0)
    ct = np.where(inimg, cls[q], NONE)
    pt = np.where(inimg, pprob[q], 0.0)
    ptl = np.where(inimg, ptol[q], 0.0)
    pdc = np.where(inimg, pdec[q], True)
    murky = np.where(inimg, pfp32[q], False)
    ri, ri_err = rng[act][:, None], r_err[act][:, None]
    with np.errstate(all="ignore"):
        diff = np.abs(rt - ri)
        d = diff * w[None]
        fin = np.isfinite(d)
        in_exact = (rt_err == 0) & (ri_err == 0)
        sub_exact = in_exact & (~fin | (diff.astype(F32).astype(np.float64) == diff))
        mul_exact = sub_exact & (~fin | (d.astype(F32).astype(np.float64) == d))
        d_err = np.where(fin, w[None] * (rt_err + ri_err) + np.where(sub_exact, 0.0, U * diff * w[None]) +
                         np.where(mul_exact, 0.0, U * d), 0.0)
    # the centre: the point's own range, d exactly 0, the pixel's class and prob
    d[:, tc], d_err[:, tc], diff[:, tc] = 0.0, 0.0, 0.0
    murky[:, tc] = False
    tt = np.broadcast_to(np.arange(S2), d.shape)
    order = np.lexsort((tt, tt != tc, d), axis=-1)
    take = lambda a: np.take_along_axis(a, order, 1)
    d_s, e_s, c_s, p_s, t_s, diff_s = take(d), take(d_err), take(ct), take(pt), take(tt), take(diff)
    w_s = w[t_s]
    ok = ~murky.any(1)
    if K < S2:
        with np.errstate(invalid="ignore"):
            g = d_s[:, K] - d_s[:, K - 1]
            g = np.where(np.isnan(g), 0.0, g)  # inf - inf: equal
        same_ops = (diff_s[:, K] == diff_s[:, K - 1]) & (w_s[:, K] == w_s[:, K - 1])
        both_exact = (e_s[:, K] == 0) & (e_s[:, K - 1] == 0)
        m_sel[act], e_sel[act] = g, e_s[:, K] + e_s[:, K - 1]
        ok &= (g > (e_s[:, K] + e_s[:, K - 1]) * _scale("sel")) | same_ops | both_exact
    sel = np.zeros(d.shape, bool)
    sel[:, :K] = True
    voter = sel & (c_s >= 1)
    if cutoff > 0:
        with np.errstate(invalid="ignore"):
            mc = np.where(voter, np.abs(d_s - cutoff), np.inf)
        m_cut[act] = mc.min(1)
        e_cut[act] = np.take_along_axis(e_s, mc.argmin(1)[:, None], 1)[:, 0]
        ok &= ((mc > e_s * _scale("cut")) | (e_s == 0)).all(1)
        voter &= d_s <= cutoff
    # the class of every selected in-image slot must be decided (logits); the centre's included
    ok &= np.where(sel, take(pdc), True).all(1)
    counts = np.stack([(voter & (c_s == j)).sum(1) for j in range(k["C"])], 1)
    win = counts.argmax(1)  # the first of equal counts: the lowest class
    any_vote = counts.max(1) > 0
    mine = voter & (c_s == win[:, None])
    # the largest prob among the winner's voters, -0 below +0
    key = np.where(mine, p_s, -np.inf)
    best = key.max(1)
    plus = (mine & (p_s == best[:, None]) & ~np.signbit(p_s)).any(1)
    best = np.where(best == 0, np.where(plus, 0.0, -0.0), best)
    label[act] = np.where(any_vote, k["label"][win], 0.0)
    prob[act] = np.where(any_vote, best, 0.0)
    tol[act] = np.where(any_vote, np.where(mine, take(ptl), 0.0).max(1), 0.0)
    decided[act] = ok
    return dict(label=label, prob=prob, tol=tol, decided=decided, sel=m_sel, cut=m_cut, sel_err=e_sel, cut_err=e_cut,
                own_bad=own_bad)
