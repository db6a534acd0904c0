"""suma_localizer_relocalize (csrc/suma_localize.hip) over the CPU oracle: tests/localize_host.py's HostLocalizer for
K1-K3 and every candidate's set_pose + scan, tests/place_shim.c for the descriptor, the search, the top-K and the pose
hypothesis -- the same steps in the same order as the library, so that the library's result must equal it to the bit."""
import numpy as np

import place_common as pc


class HostPlaces:
    """a place index on the host: cells (N, S, R), ids, one pose per entry"""

    def __init__(self, shim, pp, cells, ids, poses):
        self.shim, self.pp = shim, pp
        self.cells = np.ascontiguousarray(cells, dtype=np.float32).reshape(-1, pp.sectors, pp.rings)
        self.ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self.poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        assert len(self.cells) == len(self.ids) == len(self.poses)

    def query(self, vertex, semantic, k, exclude=None):
        q = pc.shim_describe(self.shim, vertex, semantic, self.pp)
        if not len(self.cells):
            return []
        dist, shift = pc.shim_search(self.shim, self.cells, q)
        return pc.shim_topk(self.shim, dist, shift, self.ids, k, self.pp.sectors, exclude)


def _state(h):
    keys = ("pose", "increment", "have_pose", "first", "origin", "n_window", "rebuilds", "window")
    return {k: (np.array(getattr(h, k), copy=True) if isinstance(getattr(h, k, None), np.ndarray) else getattr(h, k, None))
            for k in keys}


def _restore(h, s):
    if s["have_pose"] and (h.origin != s["origin"] or not h.have_pose):
        h._gather(*s["origin"])
    for k, v in s.items():
        setattr(h, k, v)


def relocalize(h, places: HostPlaces, points, labels, probs, max_candidates, fixed_iterations=0):
    """h: a HostLocalizer with a map.  -> dict as core.Localizer.relocalize gives it"""
    assert h.map is not None and 1 <= max_candidates <= 32
    # 1. K1-K3 at T_loc
    h.ora.preprocess(points, labels, probs, h.t_loc, h.frame)
    # 2. the candidate places
    matches = places.query(h.frame.vertex, h.frame.semantic, max_candidates)
    saved = _state(h)
    # 3. each candidate is a start pose and one scan
    tried, best, best_score = [], -1, 0.0
    for k, m in enumerate(matches):
        h.set_pose(pc.shim_hypothesis(places.shim, places.poses[m["index"]], m["yaw"]))
        r = h.process_scan(points, labels, probs, fixed_iterations)
        tried.append(dict(match=m, result=r))
        if not r["tracked"]:
            continue
        score = float(r["stats"]["error"]) / float(r["stats"]["valid"])
        if best < 0 or score < best_score:
            best, best_score = k, score
    # 4.
    if best < 0:
        _restore(h, saved)
        return dict(found=False, n_tried=len(tried), winner=-1, match=None, result=None, candidates=tried)
    w = tried[best]["result"]
    if best + 1 != len(matches):
        if h.origin != w["origin"]:
            h._gather(*w["origin"])
        h.pose, h.increment, h.first = w["pose"].copy(), w["increment"].copy(), False
    return dict(found=True, n_tried=len(tried), winner=best, match=tried[best]["match"], result=w, candidates=tried)


def relocalized_equal(a, b, where=""):
    """two relocalisation dicts (core.Localizer.relocalize / relocalize above) equal to the bit"""
    from localize_host import results_equal
    assert (a["found"], a["n_tried"], a["winner"]) == (b["found"], b["n_tried"], b["winner"]), (where, a["winner"], b["winner"])
    pc.matches_equal([c["match"] for c in a["candidates"]], [c["match"] for c in b["candidates"]], where)
    for k, (x, y) in enumerate(zip(a["candidates"], b["candidates"])):
        results_equal(x["result"], y["result"], (where, "candidate", k))
    if a["found"]:
        pc.matches_equal([a["match"]], [b["match"]], where)
        results_equal(a["result"], b["result"], (where, "winner"))
