"""Maps made for k_render's tile groups (semantic_suma_amd/csrc/k_render.hip, -DSUMA_RENDER_GROUP: a block runs phase 1a
on several consecutive 256-record tiles, appends their candidates to one list and rasterises the list once it is full
enough, the next tile would not fit, or the group ends), and the proof -- with the oracle, on the CPU -- that every map
has the per-tile candidate counts it claims.  tests/test_gpu_render_group.py runs the same scenes through the kernel.

The kernel takes its tiles from the END of the record array, so "tile 0" of a scene here is the LAST 256 records, tile 1
the 256 before them, and block 0's group is tiles 0 .. G - 1.  A candidate is what the oracle's geometry stage emits:
stable, selected by the pass, front facing, centre inside the image and the depth range.

   sizes   S in SIZES records of one ordinary shell: partial last tile, odd tile count, a group of one tile
   pairs   two tiles with nA and nB candidates (PAIRS_A x PAIRS_B): plain append, exact fit (nA + nB = 256), overflow
           by one and by many (the tile's second run of phase 1a), both sides of any flush threshold that is a multiple
           of 32; the records that are no candidates are spread over the four reasons there are: unstable, back facing,
           outside the field of view, beyond the depth range
   quads   four tiles: sparse-sparse-sparse-dense, dense first, and orders that flush in the middle of a group; all
           stamps new (the counts hold for render, render_active and the new pass of the others) or "mixed": the
           candidates cycle through new only / old only / old by creation and new by stamp, so that one list carries
           rows for the old z-buffer, the new one and both -- there the counts are those of the merged render
   twins   pairs of records that are the same to the bit, in DIFFERENT tiles of one group, alone at their pixels
   carry   two different maps one after the other on one context, the second smaller
"""
from functools import lru_cache

import numpy as np
import pytest

import render_ref as R
import test_render_crafted_host as H

W, HH = 48, 12  # the smallest image of the crafted suites
THR = H.TIMESTAMP - 100
SIZES = (1, 255, 256, 257, 511, 512, 513, 769, 1025)
PAIRS_A = (0, 1, 64, 96, 127, 128, 129, 160, 255, 256)
PAIRS_B = (0, 1, 96, 128, 160, 256)
QUADS = {"sparse3-dense": (20, 30, 40, 250), "dense-first": (250, 20, 30, 40), "fill-exactly": (64, 64, 64, 64),
         "flush-in-the-middle": (100, 100, 100, 100), "overflow-twice": (120, 200, 100, 250), "empty-between": (0, 200, 0, 90),
         "all-empty": (0, 0, 0, 0), "all-full": (256, 256, 256, 256)}
REASONS = ("unstable", "back-facing", "out-of-view", "too-far")


def calls():
    """merged render, render_active (the fused K7 splat rides on it before an update), unmerged render, render_composed"""
    v = H.VIEW_I
    return [("render", v, v, 0.0), ("active", v, None, 0.0), ("render", v, H.nudged(v), 0.0), ("composed", v, H.nudged(v), 0.0)]


def tile_records(counts, seed, mixed=False, columns=(0.04, 0.96), poses=None, with_flags=False):
    """len(counts) tiles of 256 records; tile t (in the kernel's order: from the end of the array) has counts[t] candidates
    from the identity view, at random places among the tile's records"""
    p = H.params(W, HH)
    rng = np.random.default_rng(seed)
    n = 256 * len(counts)
    cand = np.zeros(n, bool)
    for t, c in enumerate(counts):
        lo = n - 256 * (t + 1)
        cand[lo + rng.permutation(256)[:c]] = True
    k = np.arange(n)
    reason = np.where(cand, -1, k % 4)
    x, y = rng.uniform(columns[0] * W, columns[1] * W, n), rng.uniform(0.1 * HH, 0.9 * HH, n)
    y = np.where(reason == 2, np.where(k % 8 < 4, -0.4 * HH, 1.4 * HH), y)  # above / below the field of view
    d = H.direction(p, x, y)
    depth = np.where(reason == 3, rng.uniform(80.0, 100.0, n), rng.uniform(4.0, 30.0, n))  # model_max_depth is 75 m
    tilt = rng.normal(size=(n, 3)) * 0.3
    nrm = -d + tilt - np.sum(tilt * d, axis=1, keepdims=True) * d
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where((reason == 1)[:, None], -nrm, nrm)
    conf = np.where(reason == 0, -1.0, 1.0)
    px = np.where(k % 5 == 0, rng.uniform(0.05, 0.3, n), rng.uniform(1.0, 5.0, n))  # every fifth quad has no pixel test
    if mixed:  # new only (mask 2), old only (mask 1), old by creation and new by stamp (mask 3)
        creation = np.choose(k % 3, [60, 3, 40])
        ts = np.choose(k % 3, [70, 8, 110])
    else:
        creation = np.where(k % 2 == 0, 60, 120)
        ts = creation + 10
    rec = H.make_records(depth[:, None] * d, nrm, 0.5 * px * depth * H.pixel_angle(p), creation, ts, conf, poses=poses)
    return (rec, cand) if with_flags else rec


def tiles_scene(name, counts, seed, mixed=False):
    return H.scene(name, H.params(W, HH), tile_records(counts, seed, mixed), calls(), counts=tuple(counts), mixed=mixed)


# The list is flushed once it holds MORE rows than the threshold: 40 + 40 candidates stay together in one list for every
# threshold from 40 on (the default is 96) at a group size of 2 (tiles 0 | 1, 2 | 3) and of 4 (all four up to 120 rows).
TWIN_COUNTS = (40, 40, 40, 40)
TWINS = (("new-new", 1, 0, False, False, (6.5, 6.5)), ("old-old", 0, 1, True, True, (14.5, 5.5)),
         ("old-high-new-low", 3, 2, False, True, (22.5, 6.5)), ("old-low-new-high", 3, 2, True, False, (30.5, 5.5)))


@lru_cache(maxsize=None)
def twin_records():
    """1024 records, four tiles of 40 candidates each: ordinary ones in the right-hand part of the image, four pairs of
    twins alone on the left.  The twins of a pair take the places of candidates in two DIFFERENT tiles (kernel order, named
    in TWINS) whose candidates share one list, so that they meet in one phase 2.  As in the tie scene of the crafted suite,
    creation stamps 3 and 60 share ONE pose, so that an old record and a new one coincide, and the second twin's normal is
    the first one's times two: the same quad to the bit (the tangent frame is normalised), but a frame's normal map shows
    which of the two was drawn.  Returns the records, the poses and [(name, id a, id b, a old, b old, pixel)]."""
    p = H.params(W, HH)
    poses = H.pose_table()
    poses[60] = poses[3]
    rec, cand = tile_records(TWIN_COUNTS, 43, columns=(0.75, 0.97), poses=poses, with_flags=True)
    n, taken, pairs = len(rec), set(), []
    for name, ta, tb, a_old, b_old, (x, y) in TWINS:
        d = H.direction(p, x, y)
        one = H.make_records(8.0 * d, -d, 0.5 * 3.4 * 8.0 * H.pixel_angle(p), 3, 8, poses=poses)[0]
        ids = []
        for t, old, scale in ((ta, a_old, 1.0), (tb, b_old, 2.0)):
            idx = next(i for i in range(n - 256 * (t + 1), n - 256 * t) if cand[i] and i not in taken)
            taken.add(idx)
            r = one.copy()
            r["count"], r["timestamp"] = (3.0, 8) if old else (60.0, 70)
            r["nx"], r["ny"], r["nz"] = H.F32(scale) * one["nx"], H.F32(scale) * one["ny"], H.F32(scale) * one["nz"]
            rec[idx] = r
            ids.append(idx)
        pairs.append((name, ids[0], ids[1], a_old, b_old, (x, y)))
    return H.number(rec), poses, tuple(pairs)


def twins_scene():
    rec, poses, _ = twin_records()
    rec = rec.copy()
    v = H.VIEW_I
    return H.scene("group-twins", H.params(W, HH), rec, [("render", v, v, 0.0), ("active", v, None, 0.0),
                                                          ("inactive", v, None, 0.0), ("composed", v, v, 0.0)], poses=poses)


def twin_expectations():
    """[(call index, frame, (x, y), winner id, length of the winner's normal)]: GL_LESS keeps the earlier primitive of a tie
    -- the lower id -- in render, render_active and render_inactive; render_composed draws with GL_LEQUAL, the later
    primitive of the later pass wins (that call runs two slot passes per tile, so never the grouped kernel)"""
    out = []
    for _, a, b, a_old, b_old, (x, y) in twin_records()[2]:
        at = (int(x), int(y))
        scale = {a: 1.0, b: 2.0}
        olds = [i for i, o in ((a, a_old), (b, b_old)) if o]
        news = [i for i, o in ((a, a_old), (b, b_old)) if not o]
        if news:
            out += [(0, "new", at, min(news), scale[min(news)]), (1, "new", at, min(news), scale[min(news)])]
        if olds:
            out += [(0, "old", at, min(olds), scale[min(olds)]), (2, "old", at, min(olds), scale[min(olds)])]
        comp = max(news) if news else max(olds)
        out.append((3, "composed", at, comp, scale[comp]))
    return out


def check_twins(results, records):
    """the winner's identity in every call: the length of the drawn normal (1 or 2) says which twin won; render also
    writes the payload (the record's own index), the single-target calls leave the semantic map alone"""
    for k, frame, (x, y), want, want_scale in twin_expectations():
        V, N, S = results[k][frame]
        assert V[y, x, 3] == 1.0, f"twins: call {k} {frame} ({x}, {y}) is empty"
        assert abs(np.linalg.norm(N[y, x, :3]) - want_scale) < 1e-3, \
            f"twins: call {k} {frame} ({x}, {y}): normal {N[y, x, :3]} is not the one of record {want} (length {want_scale})"
        if k == 0:
            assert int(round(float(S[y, x, 0]))) == want, f"twins: call {k} {frame} ({x}, {y}): id {S[y, x, 0]} != {want}"


@lru_cache(maxsize=None)
def get_scene(sid):
    kind, _, rest = sid.partition(":")
    if kind == "size":
        S = int(rest)
        p = H.params(W, HH)
        return H.scene(sid, p, H.shell(p, 1025, 17)[:S].copy(), H.usual_calls(H.VIEW_I))
    if kind == "pair":
        nA, nB = (int(v) for v in rest.split("+"))
        return tiles_scene(sid, (nA, nB), 1000 + 7 * nA + nB)
    if kind == "quad":
        return tiles_scene(sid, QUADS[rest], 2000 + len(rest))
    if kind == "mixed":
        return tiles_scene(sid, QUADS[rest], 3000 + len(rest), mixed=True)
    assert sid == "group-twins"
    return twins_scene()


SIZE_IDS = [f"size:{S}" for S in SIZES]
PAIR_IDS = [f"pair:{a}+{b}" for a in PAIRS_A for b in PAIRS_B]
QUAD_IDS = [f"quad:{q}" for q in QUADS] + [f"mixed:{q}" for q in ("sparse3-dense", "dense-first", "overflow-twice", "fill-exactly")]
COUNTED_IDS = PAIR_IDS + QUAD_IDS
CARRY = ("quad:overflow-twice", "pair:129+128", "size:257")  # 1024, 512 and 257 records on one context


def candidates(oracle_lib, sc, mode):
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    return o.debug_render_quads(H.VIEW_I, 0.0, mode, THR)[0].astype(bool)


def per_tile(flags):
    """counts per 256-record tile, in the kernel's order (last records first)"""
    n = len(flags)
    return tuple(int(flags[max(0, n - 256 * (t + 1)):n - 256 * t].sum()) for t in range((n + 255) // 256))


def fused_index_map(side, sc):
    """On a context that has made no other call: load, ONE render_active, then the index map of an update at the very
    pose it has drawn from.  That is the sequence in which the kernel's K7 splat, fused into the render pass, is what the
    update consumes (a second render_active before the update would find the first splat unconsumed, clear it and switch
    the fusion off: the index map would then come from a K7 pass of its own and show nothing of k_render)."""
    c = next(c for c in sc["calls"] if c[0] == "active")
    side.load(sc["poses"], sc["records"], sc["timestamp"])
    side.call(c)
    return side.index_map(c[1])


@lru_cache(maxsize=None)
def oracle_run(sid):
    """(frames after every call, index map behind one render_active) of the oracle, computed once and shared"""
    from oracle import pyoracle
    pyoracle.build()
    sc = get_scene(sid)
    return H.run_scene(H.OracleSide(pyoracle, sc["params"]), sc), fused_index_map(H.OracleSide(pyoracle, sc["params"]), sc)


def oracle_results(sid):
    return oracle_run(sid)[0]


def check_carry(side_factory, reference):
    """every scene of CARRY in turn on ONE context (1024, 512, 257 records), then the first again: each run equals the
    scene's own reference in bits -- no row, count or z-buffer entry of the larger map survives into the smaller one"""
    side = side_factory(get_scene(CARRY[0])["params"])
    for sid in CARRY + CARRY[:1]:
        sc = get_scene(sid)
        H.assert_results_equal(H.written(H.run_scene(side, sc), sc["calls"]), H.written(reference(sid), sc["calls"]), f"carry {sid}")


# ---------------------------------------------------------------------------------------------------------------------
# the claims, proved with the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", COUNTED_IDS)
def test_tiles_have_the_candidate_counts_they_claim(oracle_lib, sid):
    sc = get_scene(sid)
    new, old = candidates(oracle_lib, sc, R.NEW), candidates(oracle_lib, sc, R.OLD)
    assert per_tile(new | old) == sc["counts"], "candidates of the merged render, per tile"
    if sc["mixed"]:
        if sum(sc["counts"]) >= 12:
            assert (new & ~old).sum() > 0 and (old & ~new).sum() > 0 and (new & old).sum() > 0, "rows for the old z-buffer, the new one and both"
    else:
        assert per_tile(new) == sc["counts"] and not old.any(), "all stamps are new: render_active sees the same counts"
    # what is no candidate is spread over the four reasons, a quarter each
    rec = sc["records"]
    n = len(rec)
    cand = new | old
    k = np.arange(n)
    for r, name in enumerate(REASONS):
        mine = ~cand & (k % 4 == r)
        if (~cand).sum() >= 8:
            assert mine.sum() > 0, name
        assert not (cand & (rec["confidence"] < 0)).any()
    assert np.array_equal(rec["confidence"] < 0, ~cand & (k % 4 == 0)), "the unstable ones"


def test_pairs_cover_the_paths():
    """plain append, exact fit, overflow by one and by many, and both sides of every flush threshold that is a multiple
    of 32 (nA on either side with a second tile behind it)"""
    sums = {a + b for a in PAIRS_A for b in PAIRS_B}
    assert 256 in sums and 257 in sums and max(sums) == 512 and 0 in sums
    assert any(a + b <= 256 and a and b for a in PAIRS_A for b in PAIRS_B)
    for T in range(32, 256, 32):
        assert any(a <= T for a in PAIRS_A if a) and any(a > T for a in PAIRS_A)
    for T in (64, 96, 128, 160):  # the thresholds that were measured: the neighbours of each are there
        assert {T, T + 1} & set(PAIRS_A) or {T - 1, T} & set(PAIRS_A)
    assert {127, 128, 129} <= set(PAIRS_A)


@pytest.mark.parametrize("sid", SIZE_IDS)
def test_size_scene(oracle_lib, sid):
    sc = get_scene(sid)
    assert len(sc["records"]) == int(sid.split(":")[1])
    new, old = candidates(oracle_lib, sc, R.NEW), candidates(oracle_lib, sc, R.OLD)
    print(f"{sid}: candidates per tile (merged) {per_tile(new | old)}")
    if len(new) >= 255:
        assert (new | old).sum() >= 0.8 * len(new), "an ordinary shell: nearly every record is a candidate"
        assert np.count_nonzero(oracle_results(sid)[0]["out"][0][..., 3]) > 20, "an empty rendering"


def test_twins_tie_in_different_tiles_of_a_group(oracle_lib):
    sc = get_scene("group-twins")
    o = oracle_lib.Oracle(sc["params"])
    o.map_update_poses(sc["poses"])
    o.map_upload(sc["records"], sc["timestamp"])
    n = len(sc["records"])
    pairs = twin_records()[2]
    new, old = candidates(oracle_lib, sc, R.NEW), candidates(oracle_lib, sc, R.OLD)
    assert per_tile(new | old) == TWIN_COUNTS, "sparse tiles: the candidates of two of them fit into one list"
    for name, a, b, a_old, b_old, _ in pairs:
        ca = o.debug_render_quads(H.VIEW_I, 0.0, R.OLD if a_old else R.NEW, THR)
        cb = o.debug_render_quads(H.VIEW_I, 0.0, R.OLD if b_old else R.NEW, THR)
        assert ca[0][a] and cb[0][b], name
        assert ca[1][a].tobytes() == cb[1][b].tobytes(), f"{name}: the quads differ"
        zw = lambda c: H.F32(0.5) * (H.F32(2.0) * c[:, 2] - H.F32(1.0)) + H.F32(0.5)
        assert np.array_equal(o.debug_depth24(zw(ca[1][a])), o.debug_depth24(zw(cb[1][b]))), name
        ta, tb = (n - 1 - a) // 256, (n - 1 - b) // 256  # tiles in the kernel's order
        assert ta != tb and ta // 2 == tb // 2, "different tiles of one group of two (and so of four)"
    assert any(a > b for _, a, b, *_ in pairs) and any(a < b for _, a, b, *_ in pairs), "the lower id in the earlier tile and in the later one"
    check_twins(oracle_results("group-twins"), sc["records"])


def test_carry_nothing_over(oracle_lib):
    assert [len(get_scene(s)["records"]) for s in CARRY] == [1024, 512, 257]
    check_carry(lambda p: H.OracleSide(oracle_lib, p), oracle_results)
