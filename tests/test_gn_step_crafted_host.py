"""The Gauss-Newton step that consumes K6's sums (solve, exp, stopping rules, carry-over) on crafted 6 x 6 systems, CPU
side: pins the oracle (oracle/o_icp.c) against the exact / fp64 reference of tests/gn_step_ref.py and fixes the inputs
that tests/test_gpu_gn_step_crafted.py runs through the HIP kernels.  All frames are 13 x 5 or 48 x 12, every chain has
1 <= max_iterations <= 33.

A. One step on well-posed systems (SYSTEMS_A; max_iterations = 1, T0 = I and TRUE_POSE, weights NONE and HUBER).
B. Prescribed steps through se3_exp (SYSTEMS_B; rows_for_step on seven dyadic, mirrored rows).
   theta in (0, 1e-10] and (1e-10, 1e-8) ARE reachable despite the 2^-28 quantum: with the points 64 m out a residual of
   2^-34 (2^-24) gives the term r * 64 = one (1024) quanta in the rotational half of Jtr, and omega = 2^-40 (2^-30).

   Condition on every system (asserted from the exact words): kappa_2 <= 1e10, every gate decided by >= 0.01.
   Bound on T1 against step_pose(exact_step(words), T0), elementwise:
       B = C * kappa_2 * 2^-53 * max(1, |dx|inf) + 8 * 2^-52      (+ |omega| (1 + |v|) where theta <= 1e-10)
   C = 4 x the largest measured ratio |T1 - ref| / (kappa_2 2^-53 max(1, |dx|inf)), rounded up to a power of two.
   Measured with the CPU oracle (worst system of each family; `pytest -s` prints every system):

       family             systems  max kappa_2  max |dx|inf  max |T1 - ref|  max ratio
       ortho              4        6.83         0.563        1.14e-16        0.151
       lever              4        7.44e+03     0.533        1.17e-15        0.002
       normals-1e-1       4        6.69e+03     6.58         8.49e-15        0.002
       normals-1e-2       4        6.36e+05     65.7         5.13e-14        0.000
       normals-1e-3       4        6.35e+07     659          2.27e-13        0.000
       rows6              4        627          3.47         1.73e-14        0.072
       rows7              4        331          0.659        2.11e-15        0.057
       rows12             4        192          0.723        4.44e-16        0.024
       room48x12          4        20.1         0.31         2.78e-17        0.012
       tiny-0             8        2.46e+04     1.5          0               0.000
       tiny-2^-40         8        2.46e+04     1.5          1.36e-12        0.000   (all of it the dropped rotation)
       tiny-2^-30         8        2.46e+04     1.5          0               0.000
       theta-1e-5         12       6.83         1.5          0               0.000
       theta-1e-2         12       6.83         1.5          1.11e-16        0.146
       theta-0.5          12       6.83         1.5          2.22e-16        0.293
       theta-pi/4-        12       6.83         1.5          1.11e-16        0.146
       theta-pi/4+        12       6.83         1.5          2.22e-16        0.293
       theta-1.5          12       6.83         1.5          2.22e-16        0.293
       theta-3.0          12       6.83         3            2.22e-16        0.169

   Largest ratio 0.293, so C = 2 (4 x 0.293 = 1.17, rounded up to a power of two).  The ratio is far below 1 where
   kappa_2 is large: the unpivoted LDL^T loses much less than kappa_2 * 2^-53 on these systems, and what is left is the
   rounding of exp and of the 4 x 4 product (1 or 2 ulp of 1), which the additive 8 * 2^-52 covers.

C. Each stopping rule alone: :64 on the 48 x 12 room chain; :66 on a crafted 17-row system with Huber outliers, whose
   chain converges linearly, so that the gradient is still 4 x epsilon when the error has stopped moving (in the room
   the chain converges quadratically and :65 always holds where :66 does: `rule66-room` is kept and says so), and
   :66's `err < last_error` half on a chain whose error rises by little; :65 and its quirk (the SIGNED maximum of Jtr)
   on a crafted six-row system; the quirk's mirror; "no rule fires".  Each `fired` triple is asserted from G.stopping.
D. Singular systems: the step is the zero twist (documented deviations), so every pose of the chain is T0.
   The two partial-room systems (rank 3 / rank 5) have exact zero pivots too; pivots at rounding level (-1.6e-7 and
   +6.9e-7 beside pivots of 1 .. 100, finite solution either way) are the two rounding_pivot_cases().

Before the containment rule 23 tests of this file failed on the oracle, most with NaN poses reported converged where
delta > 0: all 16 of test_oracle_singular, both partial-room systems, both rounding-level pivots,
test_solve6_rule_on_stated_matrices and both pipeline runs, e.g.
   test_oracle_singular[empty-data-13x5-default]: final pose [[nan nan nan nan] [nan nan nan nan] [nan nan nan nan]
   [0. 0. 0. 1.]], converged = 1, iterations = 0.

Mutation check on the CPU oracle (each mutant of oracle/o_icp.c built and run against this file; tests that fail):
   the whole containment rule removed             23: the tests named above
   the pivot test dropped (finiteness test kept)   2: test_oracle_rounding_level_pivot[pivot-negative],
                                                      test_solve6_rule_on_stated_matrices (every all-zero case is still
                                                      caught as 0/0 = NaN)
   the finiteness test dropped (pivot test kept)   1: test_solve6_rule_on_stated_matrices
   rule :64 dropped                                3: test_oracle_stopping_rule[rule64-alone], two singular cases
   rule :65 dropped                                1: test_oracle_stopping_rule[rule65-quirk]
   :65 on the largest magnitude of Jtr             1: test_oracle_stopping_rule[rule65-quirk]
   rule :66 dropped                                1: test_oracle_stopping_rule[rule66-alone]
   :66 without `err < last_error`                  1: test_oracle_stopping_rule[rule66-rising]
   the converged step not applied                  4: test_oracle_stopping_rule[rule64-alone | rule66-alone | rule66-room |
                                                      rule65-quirk]
   the theta <= 1e-10 branch dropped (Rodrigues
   at every theta)                                31: test_oracle_one_step[tiny-0-*] (0/0), and every singular case (the
                                                      zero twist itself has theta = 0)
   the branch moved to theta > 0                   1: test_tiny_rotations_reach_both_sides_of_the_threshold
   `D > 0` written `D >= 0` is not a mutant: a zero pivot divides by zero, and the finiteness test catches the result.
"""
from functools import lru_cache
import math

import numpy as np
import pytest

import gn_step_ref as G
import k6_ref as K
import test_k6_crafted_host as H
from semantic_suma_amd.types import default_params

NONE, HUBER, TUKEY = 0, H.HUBER, H.TUKEY
KAPPA_CAP = 1e10
C_BOUND = 2.0  # see the table above
W13, H5 = H.W13, H.H5
F32 = np.float32
TWO_T0 = (("I", np.eye(4)), ("true", H.TRUE_POSE))


def small_params(wf=NONE, **ov):
    kw = dict(data_width=W13, data_height=H5, model_width=W13, model_height=H5, bilinear_sampling=0, weight_function=wf,
              max_iterations=1, stopping_threshold=0.0, delta=0.0)
    kw.update(ov)
    return default_params(**kw)


def room_params(wf=NONE, **ov):
    kw = dict(data_width=48, data_height=12, model_width=48, model_height=12, bilinear_sampling=0, weight_function=wf,
              max_iterations=1, stopping_threshold=0.0, delta=0.0)
    kw.update(ov)
    return default_params(**kw)


def room_frames():
    _, data, model = H.room_scene("room48x12-near-tukey")  # data cast from TRUE_POSE, model from the identity
    return data, model


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------
def dyadic_rows(L):
    """seven mirrored rows on the axes and diagonals of the plane z = 0, normals along axes the point has no component
    on (so v_m = v_d - r n stores r exactly): J = [n, v x n] with entries 0, +-1, +-L"""
    pts = [((0, L, 0), (1, 0, 0)), ((0, -L, 0), (1, 0, 0)), ((L, 0, 0), (0, 1, 0)), ((L, L, 0), (0, 0, 1)),
           ((L, -L, 0), (0, 0, 1)), ((-L, L, 0), (0, 0, 1)), ((-L, -L, 0), (0, 0, 1))]
    p = small_params()
    rows = []
    for v, n in pts:
        ix, iy = G.project(v, W13, H5, p)
        rows.append(dict(at=(int(ix), int(iy)), v=tuple(float(c) for c in v), n=tuple(float(c) for c in n), r=0.0))
    return rows


def ray_rows(seed, n_rows, ranges, normals=None, big_r=2):
    """rows on texel rays: seeded choice of texels, unit normals (random, or cycled through `normals`), residuals within
    +-0.4 and `big_r` of them in +-(0.6 .. 1.4) (beyond the Huber factor, inside the distance gate)"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(W13 * H5)[:n_rows]
    rows = []
    for k, c in enumerate(cells):
        if normals is None:
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
        else:
            n = np.asarray(normals[k % len(normals)], dtype=np.float64)
        r = rng.uniform(-0.4, 0.4)
        if k < big_r:
            r = (1 if k % 2 else -1) * rng.uniform(0.6, 1.4)
        rows.append(dict(at=(int(c % W13), int(c // W13)), n=tuple(n), range=float(ranges[k % len(ranges)]), r=float(r)))
    return rows


def _systems_a():
    out = []
    ortho = dyadic_rows(1.0)
    for row, r in zip(ortho, (0.25, -0.125, 0.375, -0.25, 0.75, 0.125, -0.0625)):
        row["r"] = r
    fam = [("ortho", ortho, True), ("lever", ray_rows(1, 12, np.geomspace(1.0, 60.0, 12)), False)]
    for name, a in (("1e-1", 1e-1), ("1e-2", 1e-2), ("1e-3", 1e-3)):
        fam.append((f"normals-{name}", ray_rows(2, 12, (2.0, 3.0, 5.0, 8.0),
                                                normals=[(1, 0, 0), (math.cos(a), math.sin(a), 0), (0, 0, 1)]), False))
    for n in (6, 7, 12):
        fam.append((f"rows{n}", ray_rows(10 + n, n, (2.0, 3.5, 6.0, 10.0)), False))
    for name, rows, dyadic in fam:
        for tn, T0 in TWO_T0:
            for wn, wf in (("none", NONE), ("huber", HUBER)):
                out.append(dict(id=f"{name}-{tn}-{wn}", rows=rows, T0=T0, wf=wf, dyadic=dyadic and tn == "I", ov={}))
    for tn, T0 in TWO_T0:
        for wn, wf in (("none", NONE), ("huber", HUBER)):
            out.append(dict(id=f"room48x12-{tn}-{wn}", rows=None, T0=T0, wf=wf, dyadic=False, ov={}))
    return out


THETA_TINY = (("0", 0.0), ("2^-40", 2.0 ** -40), ("2^-30", 2.0 ** -30))
THETA = (("1e-5", 1e-5), ("1e-2", 1e-2), ("0.5", 0.5), ("pi/4-", math.pi / 4 - 1e-3), ("pi/4+", math.pi / 4 + 1e-3),
         ("1.5", 1.5), ("3.0", 3.0))
V_LEN = (0.0, 1e-6, 0.1, 1.5)
E = np.eye(3)
D3 = np.ones(3) / math.sqrt(3.0)


def _systems_b():
    out = []

    def add(id, L, v, w, dyadic):
        rows = dyadic_rows(L)
        dx = np.concatenate([v, w])
        for row, r in zip(rows, G.rows_for_step([G.row_jacobian(q, W13, H5, small_params()) for q in rows], dx)):
            row["r"] = float(F32(r))
        out.append(dict(id=id, rows=rows, T0=np.eye(4), wf=NONE, dyadic=dyadic, dx_target=dx, ov=dict(icp_max_distance=16.0)))

    # theta = 0, in (0, 1e-10], in (1e-10, 1e-8): points 64 m out; rotation and translation about the same axis, so
    # that the rows that carry omega hold nothing else (fp32 residuals cannot hold 1.5 + 2^-34)
    for tn, th in THETA_TINY:
        for an, ax in (("z", 2), ("x", 0)):
            for vl in V_LEN:
                add(f"tiny-{tn}-{an}-v{vl:g}", 64.0, vl * E[ax], th * E[ax], True)
    # larger angles: points 1 m out; the translation across the rotation axis, and both along the diagonal
    for tn, th in THETA:
        for k, (an, w, v) in enumerate((("z", E[2], E[0]), ("x", E[0], E[1]), ("d", D3, D3[::-1] * (1, -1, 1)))):
            for vl in V_LEN:
                add(f"theta-{tn}-{an}-v{vl:g}", 1.0, vl * np.asarray(v), th * np.asarray(w), False)
    return out


SYSTEMS_A, SYSTEMS_B = _systems_a(), _systems_b()
SYSTEMS = {s["id"]: s for s in SYSTEMS_A + SYSTEMS_B}
A_IDS, B_IDS = [s["id"] for s in SYSTEMS_A], [s["id"] for s in SYSTEMS_B]


@lru_cache(maxsize=None)
def system(sid):
    """(params, data, model, T0, fp64 evaluation at T0) of a system; built once, read-only"""
    s = SYSTEMS[sid]
    if s["rows"] is None:
        p = room_params(s["wf"], **s["ov"])
        data, model = room_frames()
        # the system is changed, not the bound: data texels that T0 projects within 0.02 texels of the image border
        # or of a texel edge (nearest sampling) are invalidated
        Vd = data[0].astype(np.float64)
        T32 = s["T0"].astype(np.float32).astype(np.float64)
        q = Vd[..., :3] @ T32[:3, :3].T + T32[:3, 3]
        ix, iy = G.project(np.moveaxis(q, -1, 0), 48, 12, p)
        fx, fy = ix - np.floor(ix), iy - np.floor(iy)
        close = (np.minimum(np.minimum(fx, 1 - fx), np.minimum(fy, 1 - fy)) < 0.02) | (ix < 0.02) | (ix > 47.98) | \
                (iy < 0.02) | (iy > 11.98)
        assert np.count_nonzero(close) <= 48
        data = tuple(np.where(close[..., None], 0, m).astype(np.float32) for m in data)
        for m in data:
            m.setflags(write=False)
    else:
        p = small_params(s["wf"], **s["ov"])
        data, model = G.system_frames(s["rows"], W13, H5, p, s["T0"])
        for m in data + model:
            m.setflags(write=False)
    return p, data, model, s["T0"], K.k6_fp64(p, data, model, s["T0"], 0)


def hand_words(s, p):
    """the words a dyadic system must give: J, weight and residual of every row as stated"""
    words = [0] * 32
    for row in s["rows"]:
        J = G.row_jacobian(row, W13, H5, p)
        r = float(F32(row["r"]))
        w = float(F32(p.factor) / F32(abs(r))) if (p.weight_function == HUBER and abs(r) > p.factor) else 1.0
        for k, v in enumerate(H.pair_words(J, w, r, True)):
            words[k] += v
    words[29], words[30], words[31] = len(s["rows"]), 0, W13 * H5 - len(s["rows"])
    return words


def step_bound(kappa, dx):
    """B of the docstring, and the allowance for the rotation that se3_exp drops at theta <= 1e-10"""
    b = C_BOUND * kappa * 2.0 ** -53 * max(1.0, float(np.max(np.abs(dx)))) + 8 * 2.0 ** -52
    th = float(np.linalg.norm(dx[3:]))
    return b + (th * (1.0 + float(np.linalg.norm(dx[:3]))) if th <= 1e-10 else 0.0)


def assert_step(sid, acc, T1, what):
    """conditions on the system (from the exact words), then T1 within B of the exact reference; returns the ratio"""
    p, data, model, T0, ref = system(sid)
    dx, kappa = G.exact_step(acc)
    assert kappa <= KAPPA_CAP, f"{sid}: kappa_2 = {kappa:.3g}"
    assert ref["margin"] >= H.MIN_MARGIN, f"{sid}: margins {ref['margins']}"
    if not SYSTEMS[sid]["rows"] is None:
        assert ref["counts"] == (len(SYSTEMS[sid]["rows"]), 0, W13 * H5 - len(SYSTEMS[sid]["rows"])), f"{sid}: {ref['counts']}"
    want = G.step_pose(dx, T0)
    th = float(np.linalg.norm(dx[3:]))
    drop = th * (1.0 + float(np.linalg.norm(dx[:3]))) if th <= 1e-10 else 0.0
    err = float(np.max(np.abs(T1 - want)))
    ratio = max(0.0, err - drop) / (kappa * 2.0 ** -53 * max(1.0, float(np.max(np.abs(dx)))))
    print(f"{what} {sid}: kappa_2 {kappa:.3g}, |dx|inf {np.max(np.abs(dx)):.3g}, theta {th:.3g}, |T1 - ref| {err:.3g}, "
          f"ratio {ratio:.3g}")
    assert np.all(np.isfinite(T1)) and err <= step_bound(kappa, dx), f"{what} {sid}: |T1 - ref| = {err}, B = {step_bound(kappa, dx)}"
    return ratio, dx


def oracle_step(oracle_lib, sid):
    p, data, model, T0, ref = system(sid)
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    F, acc, JtJ, Jtr, st = ora.jacobian_products(fd, fm, T0, 0)
    T1, hist, mst = ora.minimize(fd, fm, T0)
    return (F, acc, JtJ, Jtr, st), (T1, hist, mst)


@pytest.mark.parametrize("sid", A_IDS + B_IDS)
def test_oracle_one_step(oracle_lib, sid):
    s = SYSTEMS[sid]
    p, data, model, T0, ref = system(sid)
    (F, acc, JtJ, Jtr, st), (T1, hist, mst) = oracle_step(oracle_lib, sid)
    if s["dyadic"]:
        got, want = [int(x) for x in acc], hand_words(s, p)
        assert got == want, f"words differ at {[k for k in range(32) if got[k] != want[k]]}"
    else:
        H.assert_within_fp64(ref, F, JtJ, Jtr, (st.valid, st.outlier, st.invalid), f"oracle {sid}")
    assert hist.shape[0] == 2 and np.array_equal(hist[0], T0) and np.array_equal(hist[1], T1)
    assert mst.iterations == 1 and mst.converged == 0
    _, dx = assert_step(sid, acc, T1, "oracle")
    if "dx_target" in s:  # the prescribed step came out (fp32 residuals, 2^-28 words)
        assert np.max(np.abs(dx - s["dx_target"])) <= 1e-6 * max(1.0, float(np.max(np.abs(s["dx_target"])))), f"{dx}"


def test_tiny_rotations_reach_both_sides_of_the_threshold(oracle_lib):
    """theta = 0 exactly, in (0, 1e-10] and in (1e-10, 1e-8), from the exact words; the rotational half of Jtr of the
    dyadic rows is exact: only the component about the chosen axis is non-zero, and it is -4 L^2 omega (x) or
    -3 L^2 omega (z)"""
    for tn, th in THETA_TINY:
        for an, ax in (("z", 2), ("x", 0)):
            for vl in V_LEN:
                sid = f"tiny-{tn}-{an}-v{vl:g}"
                (_, acc, _, _, _), (T1, _, _) = oracle_step(oracle_lib, sid)
                dx, _ = G.exact_step(acc)
                # which side of lie_algebra.cpp's `theta > 1e-10` the step fell on: at or below it the rotation is
                # dropped altogether (the block is the identity in bits), above it omega shows in the off-diagonal
                assert np.array_equal(T1[:3, :3], np.eye(3)) == (th <= 1e-10), f"{sid}: {T1[:3, :3]}"
                got = float(np.linalg.norm(dx[3:]))
                rot = [int(acc[21 + 3 + k]) for k in range(3)]
                n_rows = 4 if an == "x" else 3
                assert rot[ax] == -round(n_rows * 64.0 * 64.0 * th * 2 ** 28) and not any(rot[k] for k in range(3) if k != ax)
                if th == 0.0:
                    assert got == 0.0
                elif th < 1e-10:
                    assert 0.0 < got <= 1e-10, got
                else:
                    assert 1e-10 < got < 1e-8, got


# ---------------------------------------------------------------------------------------------------------------------
# C. stopping rules
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_START = np.eye(4)
START_66 = K.pose_from(15.0, (0.8, -0.17, 0.04))
GAP = 4.0


@lru_cache(maxsize=None)
def room_chain():
    """fp64 quantities of the 48 x 12 room chain (nearest sampling, Huber) from the identity, 8 steps"""
    data, model = room_frames()
    return G.chain_quantities(room_params(HUBER, max_iterations=8), data, model, CHAIN_START, 8)


def _f32(x):
    return float(F32(x))


def huber_rows(seed):
    """10 .. 23 rows on texel rays at 3 .. 12 m with random unit normals; the first 2 .. 7 are Huber outliers (|r| in
    0.7 .. 1.5, inside the distance gate), the rest lie within +-0.15"""
    rng = np.random.default_rng(seed)
    n_rows, n_out = int(rng.integers(10, 24)), int(rng.integers(2, 8))
    cells = rng.permutation(W13 * H5)[:n_rows]
    rows = []
    for k, c in enumerate(cells):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        r = rng.uniform(-0.15, 0.15) if k >= n_out else rng.choice([-1, 1]) * rng.uniform(0.7, 1.5)
        rows.append(dict(at=(int(c % W13), int(c // W13)), n=tuple(n), range=float(rng.uniform(3, 12)), r=float(r)))
    return rows


@lru_cache(maxsize=None)
def rule_cases():
    """dict id -> dict(params, frames, T0, expect...) of section C; every condition the issue states is asserted here"""
    poses, q = room_chain()
    cases = {}
    data, model = room_frames()
    # :64 alone: delta between |dx|inf of iterations k* - 1 and k*, epsilon = 0
    ks = next(k for k in range(1, 8) if q[k - 1]["dx_inf"] >= GAP * q[k]["dx_inf"])
    assert all(q[j]["dx_inf"] > q[ks - 1]["dx_inf"] / 1.0001 for j in range(ks)), "an earlier step is smaller"
    delta = _f32(math.sqrt(q[ks - 1]["dx_inf"] * q[ks]["dx_inf"]))
    cases["rule64-alone"] = dict(p=room_params(HUBER, max_iterations=8, stopping_threshold=0.0, delta=delta), data=data, model=model,
                                 T0=CHAIN_START, converged=1, iterations=ks, fired=(True, False, False))
    # :66 ALONE, on a crafted system: 17 rows on texel rays, three of them Huber outliers (|r| in 0.7 .. 1.5).  The
    # reweighting makes the chain converge linearly, so the gradient is still large when the error has stopped moving:
    # fp64 shows max Jtr = 2.6, 0.26, 0.097 and |dF| = 3.4e38, 0.024, 0.0012.  epsilon is the geometric mean of the last
    # two |dF|; :65 is silent by 4x at EVERY iteration up to and including k*, :64 is off (delta = 0).
    p66 = small_params(HUBER, max_iterations=8)
    d66, m66 = G.system_frames(huber_rows(88), W13, H5, p66, np.eye(4))
    _, qh = G.chain_quantities(p66, d66, m66, np.eye(4), 8)
    kh = next(k for k in range(1, 8) if qh[k - 1]["dF"] >= GAP * qh[k]["dF"] and
              all(abs(qh[j]["max_jtr"]) >= GAP * math.sqrt(qh[k - 1]["dF"] * qh[k]["dF"]) for j in range(k + 1)))
    epsh = _f32(math.sqrt(qh[kh - 1]["dF"] * qh[kh]["dF"]))
    assert qh[kh]["F"] < qh[kh - 1]["F"] and qh[kh]["dF"] > 1e-5, "the gap must stand above fp32 rounding of F"
    assert all(abs(qh[j]["max_jtr"]) >= GAP * epsh for j in range(kh + 1)), [qh[j]["max_jtr"] for j in range(kh + 1)]
    assert all(qh[j]["dF"] >= 2 * epsh for j in range(kh)) and 2 * qh[kh]["dF"] <= epsh
    assert all(x["margin"] >= H.MIN_MARGIN and x["counts"] == (17, 0, 48) for x in qh[:kh + 1])
    cases["rule66-alone"] = dict(p=small_params(HUBER, max_iterations=8, stopping_threshold=epsh, delta=0.0), data=d66, model=m66,
                                 T0=np.eye(4), converged=1, iterations=kh, fired=(False, False, True))
    # :66's other half (`err < last_error`): 19 such rows whose error RISES at the second iteration, by a quarter of
    # epsilon, while :65 is silent by 4x -- nothing fires and the chain runs out of iterations.
    dr, mr = G.system_frames(huber_rows(70), W13, H5, p66, np.eye(4))
    _, qr = G.chain_quantities(p66, dr, mr, np.eye(4), 2)
    epsr = _f32(GAP * qr[1]["dF"])
    assert qr[1]["F"] > qr[0]["F"] and qr[1]["dF"] > 1e-5 and all(abs(x["max_jtr"]) >= GAP * epsr for x in qr)
    assert all(x["margin"] >= H.MIN_MARGIN and x["counts"] == (19, 0, 46) for x in qr)
    cases["rule66-rising"] = dict(p=small_params(HUBER, max_iterations=2, stopping_threshold=epsr, delta=0.0), data=dr, model=mr,
                                  T0=np.eye(4), converged=0, iterations=2, fired=None)
    # :66 on the 48 x 12 room, as far as the room goes: epsilon between |dF| of iterations k* - 1 and k*, delta = 0; :65
    # silent by 4x at every EARLIER iteration.  From the identity the room gives no such iteration (max Jtr = 38, 0.86
    # against 4 epsilon = 1.95), so the chain starts 15 degrees and 0.5 m off.  AT k* rule :65 holds as well (the chain
    # converges quadratically: dF_k ~ |Jtr_k-1|^2 while Jtr_k itself has already collapsed), so this case alone would
    # not notice a missing :66 -- the crafted case above does.
    poses66, q66 = G.chain_quantities(room_params(HUBER, max_iterations=8), data, model, START_66, 8)
    ke = next(k for k in range(1, 8) if q66[k - 1]["dF"] >= GAP * q66[k]["dF"] and q66[k]["F"] < q66[k - 1]["F"] and
              all(abs(q66[j]["max_jtr"]) >= GAP * math.sqrt(q66[k - 1]["dF"] * q66[k]["dF"]) for j in range(k)))
    eps = _f32(math.sqrt(q66[ke - 1]["dF"] * q66[ke]["dF"]))
    assert q66[ke - 1]["dF"] >= GAP * q66[ke]["dF"] and q66[ke]["dF"] > 1e-5, "the gap must stand above fp32 rounding of F"
    assert all(abs(q66[j]["max_jtr"]) >= GAP * eps for j in range(ke)), [q66[j]["max_jtr"] for j in range(ke)]
    assert all(q66[j]["dF"] >= 2 * eps for j in range(ke)) and all(q66[j]["dx_inf"] > 0 for j in range(ke + 1))
    cases["rule66-room"] = dict(p=room_params(HUBER, max_iterations=8, stopping_threshold=eps, delta=0.0), data=data, model=model,
                                T0=START_66, converged=1, iterations=ke, fired=(False, True, True))
    # no rule fires in three iterations: both thresholds 4x below everything the chain shows
    eps3 = _f32(min(min(abs(q[j]["max_jtr"]), q[j]["dF"]) for j in range(3)) / GAP)
    del3 = _f32(min(q[j]["dx_inf"] for j in range(3)) / GAP)
    assert eps3 > 0 and del3 > 0
    cases["no-rule-fires"] = dict(p=room_params(HUBER, max_iterations=3, stopping_threshold=eps3, delta=del3), data=data, model=model,
                                  T0=CHAIN_START, converged=0, iterations=3, fired=None)
    # :65 and its quirk: Jtr = s (-1, -1, -1, -1, -1, +1e-6) on six rows (J invertible: r = J^-T Jtr)
    s, eps65, del65 = 0.125, 1e-5, 1e-6
    for name, last in (("rule65-quirk", 1e-6), ("rule65-mirror", 1.0)):
        rows = dyadic_rows(1.0)[:6]
        p = small_params(NONE, max_iterations=1, stopping_threshold=eps65, delta=del65)
        J = np.array([G.row_jacobian(r, W13, H5, p) for r in rows])
        target = s * np.array([-1, -1, -1, -1, -1, last])
        for row, r in zip(rows, np.linalg.solve(J.T, target)):
            row["r"] = float(F32(r))
        d, m = G.system_frames(rows, W13, H5, p, np.eye(4))
        ref = K.k6_fp64(p, d, m, np.eye(4), 0)
        dx = G.contained_step(ref["JtJ"], ref["Jtr"])
        assert ref["margin"] >= H.MIN_MARGIN and ref["counts"] == (6, 0, 59)
        assert np.min(ref["Jtr"]) <= -1000 * eps65 and np.max(np.abs(dx)) >= 1000 * del65
        if last < 1:
            assert abs(np.max(ref["Jtr"])) < eps65 / 4 and np.argmax(ref["Jtr"]) == 5
        else:
            assert np.max(ref["Jtr"]) >= 1000 * eps65
        cases[name] = dict(p=p, data=d, model=m, T0=np.eye(4), converged=int(last < 1), iterations=0 if last < 1 else 1,
                           fired=(False, True, False) if last < 1 else None)
    return cases


RULE_IDS = ["rule64-alone", "rule66-alone", "rule66-rising", "rule66-room", "no-rule-fires", "rule65-quirk", "rule65-mirror"]


def assert_rule_case(cid, T, hist, converged, iterations, what):
    """converged / iterations / history length as the rules say, every pose within POSE_BAR of fp64 at its iteration"""
    c = rule_cases()[cid]
    want = G.expected_chain(c["p"], c["data"], c["model"], c["T0"], c["p"].max_iterations,
                            float(c["p"].stopping_threshold), float(c["p"].delta))
    assert (want["converged"], want["iterations"]) == (c["converged"], c["iterations"]), "test setup"
    if c["fired"] is not None:
        assert want["fired"] == c["fired"], f"test setup: {want['fired']}"
    assert (converged, iterations) == (c["converged"], c["iterations"]), f"{what} {cid}: {converged}, {iterations}"
    assert hist.shape[0] == len(want["history"]) == c["iterations"] + 1
    for k, (a, b) in enumerate(zip(list(hist) + [T], want["history"] + [want["final"]])):
        t, r = K.pose_delta(a, b)
        print(f"{what} {cid}: pose {k}: {t:.3g} m, {r:.3g} rad from fp64")
        assert t <= H.POSE_BAR[0] and r <= H.POSE_BAR[1], f"{what} {cid}: pose {k}: {t} m, {r} rad"
    if c["converged"]:  # the converged step is applied, and not pushed
        assert K.pose_delta(T, hist[-1])[0] > 0.0


@pytest.mark.parametrize("cid", RULE_IDS)
def test_oracle_stopping_rule(oracle_lib, cid):
    c = rule_cases()[cid]
    ora = oracle_lib.Oracle(c["p"])
    fd, fm = H.oracle_frames(ora, c["data"], c["model"])
    T, hist, st = ora.minimize(fd, fm, c["T0"])
    assert_rule_case(cid, T, hist, st.converged, st.iterations, "oracle")


# ---------------------------------------------------------------------------------------------------------------------
# D. singular systems
# ---------------------------------------------------------------------------------------------------------------------
FAR_START = K.pose_from(1.5, (1000.0, 0.31, 0.04))


@lru_cache(maxsize=None)
def singular_cases():
    """id -> (params overrides, size, data, model, T0, iteration0)"""
    cases = {}
    zero = lambda W, Hh: tuple(np.zeros((Hh, W, 4), dtype=np.float32) for _ in range(3))
    rd, rm = room_frames()
    small = G.system_frames([dict(dyadic_rows(2.0)[k], r=0.25) for k in range(6)], W13, H5, small_params(), np.eye(4))
    cases["empty-data-13x5"] = (dict(), (W13, H5), zero(W13, H5), small[1], np.eye(4), 0)
    cases["empty-data-48x12"] = (dict(), (48, 12), zero(48, 12), rm, H.TRUE_POSE, 0)
    cases["empty-model"] = (dict(), (48, 12), rd, zero(48, 12), np.eye(4), 0)
    # every pair 4 m apart: valid, none an inlier
    far = [dict(r, r=4.0) for r in dyadic_rows(2.0)]
    cases["all-outliers"] = (dict(), (W13, H5), *G.system_frames(far, W13, H5, small_params(), np.eye(4)), np.eye(4), 0)
    tk = [dict(r, r=0.75) for r in dyadic_rows(2.0)]  # inside the distance gate, beyond the Tukey factor
    cases["tukey-all-zero"] = (dict(weight_function=TUKEY), (W13, H5), *G.system_frames(tk, W13, H5, small_params(), np.eye(4)),
                               np.eye(4), 1)
    p = small_params()
    one = [dict(at=(6, 4), v=(2.0, 0.0, 0.0), n=(1.0, 0.0, 0.0), r=0.25)]
    cases["one-pixel"] = (dict(), (W13, H5), *G.system_frames(one, W13, H5, p, np.eye(4)), np.eye(4), 0)
    # eight points on the plane x = 2 mirrored in y AND in z: J = (1, 0, 0, 0, z, -y), so JtJ = diag(8, 0, 0, 0, sum z^2,
    # sum y^2).  Points above the horizon need a field of view that is symmetric about it: +-14 degrees here.
    sym = dict(data_fov_up=14.0, data_fov_down=-14.0, model_fov_up=14.0, model_fov_down=-14.0)
    ps = small_params(**sym)
    plane = []
    for y, z in ((1.0, 0.25), (2.0, 0.5)):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                v = (2.0, sy * y, sz * z)
                ix, iy = G.project(v, W13, H5, ps)
                plane.append(dict(at=(int(ix), int(iy)), v=v, n=(1.0, 0.0, 0.0), r=0.25))
    cases["one-plane-dyadic"] = (sym, (W13, H5), *G.system_frames(plane, W13, H5, ps, np.eye(4)), np.eye(4), 0)
    cases["far-start"] = (dict(), (48, 12), rd, rm, FAR_START, 0)
    return cases


SINGULAR_IDS = ["empty-data-13x5", "empty-data-48x12", "empty-model", "all-outliers", "tukey-all-zero", "one-pixel",
                "one-plane-dyadic", "far-start"]
MODES = {"fixed": dict(stopping_threshold=0.0, delta=0.0, max_iterations=3), "default": dict(max_iterations=5)}


def singular_case(cid, mode):
    ov, (W, Hh), data, model, T0, it0 = singular_cases()[cid]
    kw = dict(data_width=W, data_height=Hh, model_width=W, model_height=Hh, bilinear_sampling=0)
    kw.update(ov)
    kw.update(MODES[mode])
    return default_params(**kw), data, model, T0, it0


def singular_expectation(cid, mode):
    """written from the rule: the poses are T0; with delta > 0 rule :64 ends the chain at its first step (|0| < delta),
    with delta = 0 it runs all its iterations unconverged.  Counts: k6_fp64's."""
    p, data, model, T0, it0 = singular_case(cid, mode)
    ref = K.k6_fp64(p, data, model, T0, it0)
    piv = G.ldlt_pivots_fp64(ref["JtJ"])
    assert not all(d > 0.0 for d in piv), f"test setup: {cid} is not singular: {piv}"
    if cid == "all-outliers":
        assert ref["counts"][0] == ref["counts"][1] == 7
    if cid == "tukey-all-zero":  # inliers, every one with weight zero
        assert ref["counts"][:2] == (7, 0) and not np.any(ref["JtJ"]) and ref["F"] == 0.0
    if cid in ("empty-data-13x5", "empty-data-48x12", "empty-model"):
        assert ref["counts"][0] == 0
    if cid == "far-start":
        assert ref["counts"][0] == ref["counts"][1], "no inlier 1000 m away"
    if cid == "one-pixel":
        assert np.array_equal(ref["JtJ"], np.diag([1.0, 0, 0, 0, 0, 0]))
    if cid == "one-plane-dyadic":
        assert np.array_equal(ref["JtJ"], np.diag(np.diag(ref["JtJ"]))) and sum(d == 0.0 for d in np.diag(ref["JtJ"])) == 3
    if p.delta > 0:
        return dict(n_hist=1, converged=1, iterations=0, counts=ref["counts"])
    return dict(n_hist=p.max_iterations + 1, converged=0, iterations=p.max_iterations, counts=ref["counts"])


def assert_singular(cid, mode, T, hist, st, info, what):
    """info: (JtJ, Jtr) of the chain's last evaluation"""
    p, data, model, T0, it0 = singular_case(cid, mode)
    want = singular_expectation(cid, mode)
    assert np.all(np.isfinite(T)), f"{what} {cid}-{mode}: final pose {T}, converged = {st.converged}, iterations = {st.iterations}"
    assert np.array_equal(T, T0) and hist.shape[0] == want["n_hist"] and all(np.array_equal(h, T0) for h in hist)
    assert (st.converged, st.iterations) == (want["converged"], want["iterations"])
    assert (st.valid, st.outlier, st.invalid) == want["counts"]
    assert np.isfinite(st.error) and all(np.all(np.isfinite(m)) for m in info)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cid", SINGULAR_IDS)
def test_oracle_singular(oracle_lib, cid, mode):
    p, data, model, T0, it0 = singular_case(cid, mode)
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    T, hist, st = ora.minimize(fd, fm, T0, iteration0=it0)
    _, _, JtJ, Jtr, _ = ora.jacobian_products(fd, fm, T, it0)
    assert_singular(cid, mode, T, hist, st, (JtJ, Jtr), "oracle")


@lru_cache(maxsize=None)
def noise_cases():
    """one wall (rank 3) and two walls plus floor (rank 5) of the 48 x 12 room, all else invalidated.  J is built from
    the MODEL normal, and the model was cast from the identity: its normals are exact axes, so whole columns of J are
    exactly zero and these systems have exact zero pivots, like section D (only the data side is rotated).  Pivots that
    are really at rounding level are in rounding_pivot_cases() below."""
    (Vd, Nd, Sd), model = room_frames()
    _, _, plane = K.room_cast(48, 12, room_params(), H.TRUE_POSE)
    out = {}
    for name, keep in (("one-wall", (0,)), ("two-walls-and-floor", (0, 1, 4))):
        mask = np.isin(plane, keep)[..., None]
        out[name] = ((np.where(mask, Vd, 0).astype(np.float32), np.where(mask, Nd, 0).astype(np.float32), Sd), model)
    return out


NOISE_IDS = ["one-wall", "two-walls-and-floor"]


@pytest.mark.parametrize("cid", NOISE_IDS)
def test_oracle_noise_level_systems_stay_finite(oracle_lib, cid):
    data, model = noise_cases()[cid]
    p = room_params(HUBER, max_iterations=3)
    ref = K.k6_fp64(p, data, model, np.eye(4), 0)
    assert np.linalg.matrix_rank(ref["JtJ"], tol=1e-6 * np.max(ref["JtJ"])) == (3 if cid == "one-wall" else 5)
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    T, hist, st = ora.minimize(fd, fm, np.eye(4))
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(hist))


NULL_DIRECTION = np.array([1.0, 0.5, 0.25]) / np.linalg.norm([1.0, 0.5, 0.25])
ROUNDING_PIVOT_IDS = ["pivot-negative", "pivot-tiny-positive"]


@lru_cache(maxsize=None)
def rounding_pivot_cases():
    """12 rows on texel rays whose normals are all perpendicular to one oblique direction: no row sees a translation
    along it, so JtJ has rank 5 in exact arithmetic and no zero column.  The 2^-28 rounding of each term makes the third
    pivot of the unpivoted LDL^T about +-1e-7 beside pivots of 1 .. 100 -- negative for one seed, positive for the
    other -- and the solution is finite either way.  Only the pivot test of the containment rule tells them apart."""
    out = {}
    for name, seed in (("pivot-negative", 1000), ("pivot-tiny-positive", 1001)):
        rng = np.random.default_rng(seed)
        rows = []
        for c in rng.permutation(W13 * H5)[:12]:
            n = rng.normal(size=3)
            n -= NULL_DIRECTION * (n @ NULL_DIRECTION)
            n /= np.linalg.norm(n)
            rows.append(dict(at=(int(c % W13), int(c // W13)), n=tuple(n), range=float(rng.uniform(2, 8)),
                             r=float(rng.uniform(-0.3, 0.3))))
        p = small_params(NONE, max_iterations=3)
        out[name] = (p, *G.system_frames(rows, W13, H5, p, np.eye(4)))
    return out


def assert_rounding_pivot(cid, JtJ, Jtr, T, hist, st, what):
    """JtJ / Jtr: the first evaluation's (exact images of the fixed-point words, so the pivots computed here in the
    stated operation order are the ones the solve meets)"""
    piv = G.ldlt_pivots_fp64(JtJ)
    free = np.linalg.solve(JtJ, -Jtr)  # what the system gives without the rule: finite, not small
    print(f"{what} {cid}: pivots {piv}, |unconstrained step|inf {np.max(np.abs(free)):.3g}")
    assert all(d > 0.5 for k, d in enumerate(piv) if k != 2) and abs(piv[2]) < 1e-5 and np.all(np.isfinite(free))
    assert np.max(np.abs(free)) > 1e-2
    assert np.all(np.isfinite(T)) and hist.shape[0] == 4 and (st.converged, st.iterations) == (0, 3)
    if cid == "pivot-negative":  # the step is the zero twist although the solution is finite
        assert piv[2] < 0.0 and all(np.array_equal(P, np.eye(4)) for P in list(hist) + [T])
        assert (st.valid, st.outlier) == (12, 0)
    else:  # a tiny POSITIVE pivot is not contained: the first step is the system's own, exp(dx) of the contained solve
        assert piv[2] > 0.0 and np.max(np.abs(hist[1] - np.eye(4))) > 1e-3
        want = G.step_pose(G.contained_step(JtJ, Jtr), np.eye(4))
        assert np.max(np.abs(hist[1] - want)) <= 1e-6 * max(1.0, np.max(np.abs(free))), "numpy's solve of the same system"


@pytest.mark.parametrize("cid", ROUNDING_PIVOT_IDS)
def test_oracle_rounding_level_pivot(oracle_lib, cid):
    p, data, model = rounding_pivot_cases()[cid]
    ora = oracle_lib.Oracle(p)
    fd, fm = H.oracle_frames(ora, data, model)
    _, _, JtJ, Jtr, _ = ora.jacobian_products(fd, fm, np.eye(4), 0)
    T, hist, st = ora.minimize(fd, fm, np.eye(4))
    assert_rounding_pivot(cid, JtJ, Jtr, T, hist, st, "oracle")


def test_solve6_rule_on_stated_matrices(oracle_lib):
    """ora_solve6 itself: zero, negative and NaN pivots and a non-finite solution give the zero twist; a healthy system
    is what numpy says"""
    rng = np.random.default_rng(5)
    J = rng.normal(size=(12, 6))
    A, b = J.T @ J, rng.normal(size=6)
    assert np.allclose(oracle_lib.solve6(A, b), np.linalg.solve(A, -b), rtol=1e-10, atol=0)
    bad = [np.zeros((6, 6)), np.diag([1.0, 0, 0, 0, 0, 0]), np.diag([1.0, 1, 1, -1, 1, 1]), np.diag([1.0, 1, np.nan, 1, 1, 1]),
           np.diag([1.0, 1, 1, 1, 1, 1e-320])]
    rhs = [b, b, b, b, np.full(6, 1e300)]
    for M, r in zip(bad, rhs):
        assert G.contained_step(M, r).tolist() == [0.0] * 6
        assert np.asarray(oracle_lib.solve6(M, r)).tolist() == [0.0] * 6, M


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline across an empty scan
# ---------------------------------------------------------------------------------------------------------------------
PIPELINE_SIZE = (360, 32)
PIPELINE_MODES = {"fixed": 5, "default": 0}  # fixed_iterations; 0 = the stopping tests of the parameters
EMPTY_AT = 3
TRACK_BOUND = (0.05, 0.005)  # metres, radians: the last pose with and without the empty scan


def pipeline_scans(with_empty=True):
    """six scans of one drive; with_empty: the fourth is a sensor blackout (no points) instead.  The run it is compared
    with is the same drive with that scan intact -- leaving the scan out altogether would compare against a run that
    has driven one scan's motion less.  Measured with the CPU oracle: 0.013 m / 0.0008 rad (fixed) and 0.0088 m /
    0.0025 rad (default) between the two last poses."""
    from conftest import get_scan
    W, Hh = PIPELINE_SIZE
    scans = [get_scan(k, W, True, height=Hh)[:3] for k in range(6)]  # (points, labels, probabilities)
    if with_empty:
        scans[EMPTY_AT] = (np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32))
    return scans


def assert_pipeline_across_empty_scan(poses, increments, last_without, what):
    """poses[k] / increments[k]: pose and last increment after scan k.  Finite; the empty scan's chain keeps the start
    it was given (the previous increment); tracking goes on"""
    assert all(np.all(np.isfinite(P)) for P in poses) and all(np.all(np.isfinite(P)) for P in increments), what
    want = poses[EMPTY_AT - 1] @ increments[EMPTY_AT - 1]
    assert np.max(np.abs(poses[EMPTY_AT] - want)) <= 1e-12, f"{what}: {np.max(np.abs(poses[EMPTY_AT] - want))}"
    t, r = K.pose_delta(poses[-1], last_without)
    print(f"{what}: last pose {t:.3g} m, {r:.3g} rad from the run without the empty scan")
    assert t <= TRACK_BOUND[0] and r <= TRACK_BOUND[1], f"{what}: {t} m, {r} rad"


@pytest.mark.parametrize("mode", list(PIPELINE_MODES))
def test_oracle_pipeline_across_an_empty_scan(oracle_lib, mode):
    from semantic_suma_amd.types import params_with_size
    p = params_with_size(*PIPELINE_SIZE)
    runs = {}
    for with_empty in (True, False):
        op = oracle_lib.OraclePipeline(p)
        poses, incs = [], []
        for pts, lab, prob in pipeline_scans(with_empty):
            op.process_scan(pts, lab, prob, fixed_iterations=PIPELINE_MODES[mode])
            poses.append(op.pose().copy())
            incs.append(op.last_increment().copy())
        runs[with_empty] = (poses, incs)
    assert_pipeline_across_empty_scan(*runs[True], runs[False][0][-1], f"oracle pipeline {mode}")
