"""Shared by the tests of the tracks (test_abi_tracks.py, test_tracks_host.py, test_gpu_tracks*.py): the host restatement
tests/track_shim.c of csrc/k_tracks.hip, a plain Python statement of it (the join by breadth-first search, the
association as a sort of all gated pairs taken greedily, sums in Python integers), the named cases on every boundary of
the specification, random sequences, and the measurements of DESIGN.md 21 on DESIGN.md 19's scenario."""
import ctypes as C
import os
import subprocess
from collections import deque

import numpy as np

from semantic_suma_amd.types import (OBJECT_TRACK_DTYPE, SCAN_OBJECT_DTYPE, TRACK_COUNTS, TrackCounts, TrackParams)

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_FLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off"]
NONE = 0xffffffff
f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "track_shim.so")
    subprocess.check_call(["gcc"] + SHIM_FLAGS + ["-fPIC", "-shared", os.path.join(HERE, "track_shim.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, u32 = C.c_void_p, C.c_uint32
    L.track_shim_update.argtypes = [vp, u32, u32, C.POINTER(TrackParams), vp, C.POINTER(u32), C.POINTER(u32), vp,
                                    C.POINTER(u32), vp, vp, C.POINTER(TrackCounts)]
    for k in ("object", "params", "track", "counts"):
        getattr(L, "track_shim_sizeof_" + k).restype = C.c_size_t
    return L


def objects(rows):
    """rows of (label, min3, max3[, centroid3[, n_texels[, n_dynamic[, r_min]]]]) -> SCAN_OBJECT_DTYPE records; the
    centroid defaults to the box's middle"""
    rec = np.zeros(len(rows), dtype=SCAN_OBJECT_DTYPE)
    for i, row in enumerate(rows):
        row = list(row) + [None] * (7 - len(row))
        r = rec[i]
        r["root"], r["label"], r["prob"] = i, row[0], 1.0
        r["min"], r["max"] = row[1], row[2]
        r["centroid"] = (np.asarray(row[1], dtype=f32) + np.asarray(row[2], dtype=f32)) * f32(0.5) if row[3] is None else row[3]
        r["n_texels"] = 10 if row[4] is None else row[4]
        r["n_dynamic"] = 0 if row[5] is None else row[5]
        r["r_min"] = 5.0 if row[6] is None else row[6]
    return rec


def points(xyz, label=10, half=0.125):
    """one small box of one class around each position: detections that joining leaves alone when they are apart"""
    xyz = np.asarray(xyz, dtype=f32).reshape(-1, 3)
    return objects([(label, p - f32(half), p + f32(half), p) for p in xyz])


class ShimTracker:
    """the tracker's state on the host, updated by tests/track_shim.c"""

    def __init__(self, shim, tp: TrackParams = None):
        self.shim = shim
        self.tp = TrackParams.defaults() if tp is None else tp
        self.clear()

    def clear(self):
        self.slots = np.zeros(int(self.tp.max_tracks), dtype=OBJECT_TRACK_DTYPE)
        self.last_stamp, self.next_id = 0, 1

    def set_state(self, slots, last_stamp, next_id):
        self.slots = np.ascontiguousarray(slots, dtype=OBJECT_TRACK_DTYPE).copy()
        self.last_stamp, self.next_id = last_stamp, next_id

    def update(self, rec, scan_id):
        """-> None when the stamp is refused, else (tracks, object_tracks, counts dict, object_detections)"""
        rec = np.ascontiguousarray(rec, dtype=SCAN_OBJECT_DTYPE).reshape(-1)
        n = rec.shape[0]
        out = np.zeros(int(self.tp.max_tracks), dtype=OBJECT_TRACK_DTYPE)
        ot, od = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        last, nxt, n_out, cnt = C.c_uint32(self.last_stamp), C.c_uint32(self.next_id), C.c_uint32(0), TrackCounts()
        rc = self.shim.track_shim_update(rec.ctypes.data, n, scan_id, C.byref(self.tp), self.slots.ctypes.data, C.byref(last),
                                         C.byref(nxt), out.ctypes.data, C.byref(n_out), ot.ctypes.data, od.ctypes.data,
                                         C.byref(cnt))
        if rc:
            return None
        self.last_stamp, self.next_id = last.value, nxt.value
        return out[:n_out.value].copy(), ot[:n].copy(), cnt.as_dict(), od[:n].copy()


# ---- the specification once more in plain Python.  fp32 by numpy; a fused multiply-add is the exact fp64 product plus the
# addend rounded to odd in fp64 (Boldo-Melquiond), which rounds to the correct fp32
def _fma(a, b, c):
    with np.errstate(all="ignore"):
        p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
        c = np.asarray(c, dtype=np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def _len3(x, y, z):
    with np.errstate(all="ignore"):
        x, y, z = (np.asarray(v, dtype=np.float32) for v in (x, y, z))
        return np.sqrt(_fma(z, z, _fma(y, y, x * x)))


def _fmax(a, b):
    return np.where(a < b, b, a).astype(np.float32)


def _ordered(v):
    b = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, (~b) & 0xffffffff, b | 0x80000000)


def python_join(rec, join_dist):
    """-> (detections as dicts, obj_det)"""
    n = len(rec)
    jd = f32(join_dist)
    adj = np.zeros((n, n), dtype=bool)
    if n and not jd < 0:
        mn, mx = rec["min"].astype(np.float32), rec["max"].astype(np.float32)
        ok = np.isfinite(mn).all(axis=1) & np.isfinite(mx).all(axis=1)
        for i0 in range(0, n, 256):               # rows b = i0 .., columns a: the pair is (a, b) with a < b
            b = slice(i0, min(i0 + 256, n))
            with np.errstate(all="ignore"):
                g = [_fmax(_fmax(f32(0.0), mn[None, :, k] - mx[b, None, k]), mn[b, None, k] - mx[None, :, k]) for k in range(3)]
                near = _len3(*g) <= jd
            adj[b] = near & (rec["label"][b, None] == rec["label"][None, :]) & ok[b, None] & ok[None, :]
        adj = np.tril(adj, -1)
        adj |= adj.T
    det_of, dets = np.full(n, NONE, dtype=np.int64), []
    for first in range(n):
        if det_of[first] != NONE:
            continue
        det_of[first] = len(dets)
        queue, members = deque([first]), []
        while queue:
            i = queue.popleft()
            members.append(i)
            for j in np.nonzero(adj[i] & (det_of == NONE))[0]:
                det_of[j] = len(dets)
                queue.append(int(j))
        m = rec[members]
        d = dict(label=int(rec["label"][first]), n_objects=len(members),
                 n_texels=min(sum(int(x) for x in m["n_texels"]), NONE), n_dynamic=min(sum(int(x) for x in m["n_dynamic"]), NONE))
        w = [min(max(int(x), 1), 1 << 22) for x in m["n_texels"]]
        lo, hi, cen = [], [], []
        for k in range(3):
            lo.append(m["min"][:, k][np.argmin(_ordered(m["min"][:, k]))])
            hi.append(m["max"][:, k][np.argmax(_ordered(m["max"][:, k]))])
            with np.errstate(all="ignore"):
                q = m["centroid"][:, k].astype(np.float32) * f32(1024.0)
            q = np.where(q < f32(-16777216.0), f32(-16777216.0), q)
            q = np.where(q > f32(16777216.0), f32(16777216.0), q)
            q = np.where(np.isnan(q), f32(0.0), q)
            S = sum(wi * int(np.rint(qi)) for wi, qi in zip(w, q))
            cen.append(f32(float(S) / (float(sum(w)) * 1024.0)))
        d.update(min=np.array(lo, dtype=f32), max=np.array(hi, dtype=f32), centroid=np.array(cen, dtype=f32),
                 r_min=m["r_min"][np.argmin(_ordered(m["r_min"]))])
        dets.append(d)
    return dets, det_of.astype(np.uint32)


class CapReached(Exception):
    """the plain statement has no cap: the rounds the association needs exceed max_rounds"""


class PyTracker:
    """the plain statement: greedy matching over the sorted gated pairs -- equal to the rounds while max_rounds is not
    reached, which ``update`` asserts"""

    def __init__(self, tp: TrackParams = None):
        self.tp = TrackParams.defaults() if tp is None else tp
        self.slots = np.zeros(int(self.tp.max_tracks), dtype=OBJECT_TRACK_DTYPE)
        self.last_stamp, self.next_id = 0, 1

    def set_state(self, slots, last_stamp, next_id):
        self.slots = np.ascontiguousarray(slots, dtype=OBJECT_TRACK_DTYPE).copy()
        self.last_stamp, self.next_id = last_stamp, next_id

    def update(self, rec, scan_id):
        tp, sl = self.tp, self.slots
        s = (scan_id + 1) & 0xffffffff
        if not s > self.last_stamp:
            return None
        rec = np.ascontiguousarray(rec, dtype=SCAN_OBJECT_DTYPE).reshape(-1)
        dets, obj_det = python_join(rec, tp.join_dist)
        D, T = len(dets), len(sl)
        cnt = dict.fromkeys(TRACK_COUNTS, 0)
        cnt.update(n_objects=len(rec), n_detections=D, n_joined=len(rec) - D)
        dt = f32(s - self.last_stamp)
        live = np.nonzero(sl["state"] != 0)[0]
        cnt["n_tracks_before"] = len(live)
        with np.errstate(all="ignore"):
            pred = (sl["position"] + sl["velocity"] * dt).astype(np.float32)
            gate = (f32(tp.gate_base) + f32(tp.gate_speed) * (s - sl["last_matched"].astype(np.int64)).astype(np.float32)).astype(np.float32)
        pairs = []
        if D and len(live):
            cen = np.array([d["centroid"] for d in dets], dtype=np.float32)
            with np.errstate(all="ignore"):
                dist = _len3(*[cen[None, :, k] - pred[live, None, k] for k in range(3)])
                ok = dist <= gate[live, None]
            for a, d in zip(*np.nonzero(ok)):
                pairs.append((int(dist[a, d].view(np.uint32)), int(live[a]), int(d)))
        pairs.sort()
        trk_det, det_trk = {}, {}
        for _, t, d in pairs:
            if t not in trk_det and d not in det_trk:
                trk_det[t], det_trk[d] = d, t
        det_track = {}
        for t in live:
            k = sl[t]
            if t in trk_det:
                d = dets[trk_det[t]]
                with np.errstate(all="ignore"):
                    res = (d["centroid"] - pred[t]).astype(np.float32)
                    if k["hits"] == 1:
                        k["position"], k["velocity"] = d["centroid"], res / dt
                    else:
                        gain = f32(tp.beta) / dt
                        k["position"] = pred[t] + f32(tp.alpha) * res
                        k["velocity"] = k["velocity"] + gain * res
                k["hits"] = min(int(k["hits"]) + 1, 65535) if k["hits"] < 65535 else k["hits"]
                k["missed"], k["last_matched"], k["detection"] = 0, s, trk_det[t]
                for key in ("label", "n_texels", "n_dynamic", "n_objects", "min", "max", "r_min"):
                    k[key] = d[key]
                if k["hits"] >= tp.confirm_hits:
                    k["state"] = 2
                det_track[trk_det[t]] = int(k["id"])
                cnt["n_matched"] += 1
            else:
                k["position"], k["detection"] = pred[t], NONE
                k["missed"] += 1
                cnt["n_missed"] += 1
                if k["missed"] > tp.max_missed:
                    sl[t] = np.zeros((), dtype=OBJECT_TRACK_DTYPE)
                    cnt["n_expired"] += 1
        free = [t for t in range(T) if sl["state"][t] == 0]
        for d in range(D):
            if d in det_trk:
                continue
            if cnt["n_born"] == len(free):
                det_track[d] = 0
                cnt["n_dropped"] += 1
                continue
            t = free[cnt["n_born"]]
            sl[t] = np.zeros((), dtype=OBJECT_TRACK_DTYPE)
            k, dd = sl[t], dets[d]
            k["id"], k["slot"], k["state"] = (self.next_id + cnt["n_born"]) & 0xffffffff, t, 2 if tp.confirm_hits <= 1 else 1
            k["hits"], k["first_stamp"], k["last_matched"], k["detection"] = 1, s, s, d
            k["position"] = k["origin"] = dd["centroid"]
            for key in ("label", "n_texels", "n_dynamic", "n_objects", "min", "max", "r_min"):
                k[key] = dd[key]
            det_track[d] = int(k["id"])
            cnt["n_born"] += 1
        self.next_id = (self.next_id + cnt["n_born"]) & 0xffffffff
        self.last_stamp = s
        out = sl[sl["state"] != 0].copy()
        cnt["n_confirmed"] = int((out["state"] == 2).sum())
        # greedy in ascending key order is what the rounds give when they are not cut short: the number of rounds the
        # rounds take is found by playing them on the pair list
        cnt["rounds"] = python_rounds(pairs)
        if cnt["rounds"] > tp.max_rounds:
            raise CapReached(cnt["rounds"])
        ot = np.array([det_track[int(d)] for d in obj_det], dtype=np.uint32)
        return out, ot, cnt, obj_det


def python_rounds(pairs):
    """the rounds of step 3 on the sorted list of gated pairs -> how many of them match something"""
    left, rounds = list(pairs), 0
    while left:
        bt, bd = {}, {}
        for key in left:
            bt.setdefault(key[1], key)
            bd.setdefault(key[2], key)
        hit = {k for k in left if bt[k[1]] == k and bd[k[2]] == k}
        ts, ds = {k[1] for k in hit}, {k[2] for k in hit}
        left = [k for k in left if k[1] not in ts and k[2] not in ds]
        rounds += 1
    return rounds


def check_counts(c, tp, live_after):
    """the identities of suma_track_counts"""
    assert c["n_objects"] == c["n_detections"] + c["n_joined"], c
    assert c["n_detections"] == c["n_matched"] + c["n_born"] + c["n_dropped"], c
    assert c["n_tracks_before"] == c["n_matched"] + c["n_missed"] and c["n_expired"] <= c["n_missed"], c
    assert live_after == c["n_tracks_before"] - c["n_expired"] + c["n_born"] and c["n_confirmed"] <= live_after, c
    assert c["rounds"] <= tp.max_rounds and (c["n_unresolved"] == 0 or c["rounds"] == tp.max_rounds), c


def same(a, b, what):
    """two updates' results, byte for byte"""
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a[2] == b[2], (what, a[2], b[2])
    assert a[0].tobytes() == b[0].tobytes(), (what, a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes(), (what, a[1], b[1])


# ---- sequences: lists of steps; a step is ("update", records, scan_id), ("state", slots, last_stamp, next_id) or
# ("clear",).  run() plays one on anything with update / set_state / clear
def run(tracker, steps):
    out = []
    for st in steps:
        if st[0] == "update":
            out.append(tracker.update(st[1], st[2]))
        elif st[0] == "state":
            tracker.set_state(st[1], st[2], st[3])
        else:
            tracker.clear()
    return out


def track_slot(slot, tid, pos, vel=(0, 0, 0), hits=2, missed=0, first=1, last=1, state=1, label=10):
    k = np.zeros((), dtype=OBJECT_TRACK_DTYPE)
    k["id"], k["slot"], k["state"], k["label"], k["hits"], k["missed"] = tid, slot, state, label, hits, missed
    k["first_stamp"], k["last_matched"], k["position"], k["velocity"], k["origin"] = first, last, pos, vel, pos
    k["detection"] = NONE
    return k


def table(T, tracks):
    sl = np.zeros(T, dtype=OBJECT_TRACK_DTYPE)
    for k in tracks:
        sl[int(k["slot"])] = k
    return sl


def grid_points(n, pitch=4.0, label=10):
    """n detections on a grid, pitch apart: nothing joins, nothing is gated to a neighbour's track"""
    i = np.arange(n)
    return points(np.stack([(i % 64) * pitch, (i // 64) * pitch, np.zeros(n)], axis=1), label)


def shrinking_line(n=40, ratio=0.95):
    """tracks at x_k, detections at x_k + a_k, the next track at x_k + a_k + b_k with a_0 > b_0 > a_1 > b_1 > ...: every
    detection but the last is nearer to the next track than to its own, every track nearest to its own detection, so
    that only the last pair is mutual and each round resolves exactly one pair, from the far end.  From a_0 = 8 m the
    ratio 0.95 leaves neighbouring distances 7 mm apart at the far end; everything is a multiple of 1/1024 m, the step of
    a detection's centroid"""
    x, a, tr, de = 0.0, 8.0, [], []
    for k in range(n):
        tr.append(x)
        de.append(x + a)
        x, a = x + a + a * ratio, a * ratio * ratio
    return np.round(np.array(tr) * 1024.0) / 1024.0, np.round(np.array(de) * 1024.0) / 1024.0


def named_cases():
    """-> list of (name, TrackParams, steps): each on a rule of the specification (the issue's list)"""
    out = []
    P = TrackParams.defaults

    def add(name, tp, steps):
        out.append((name, tp, steps))

    for n in (0, 1, 63, 64, 65, 1025, 4096):
        for T in (1, 2, 64, 65, 1024):
            rec = grid_points(n)
            moved = rec.copy()
            moved["centroid"][:, 0] += f32(0.25)
            add("count_%d_tracks_%d" % (n, T), P(max_tracks=T), [("update", rec, 0), ("update", moved[::-1].copy(), 1),
                                                                   ("update", rec[: n // 2], 3)])
    # ties: the index decides
    add("two_detections_one_track", P(join_dist=-1.0), [("update", points([[0, 0, 0]]), 0),
                                                        ("update", points([[1, 0, 0], [-1, 0, 0], [0, 1, 0]]), 1)])
    add("two_tracks_one_detection", P(join_dist=-1.0), [("update", points([[1, 0, 0], [-1, 0, 0]]), 0),
                                                        ("update", points([[0, 0, 0]]), 1)])
    # the gate: 1.5 + 0.5 * 1 = 2 and 1.5 + 0.5 * 3 = 3, at and one ulp beyond.  A detection's centroid is a multiple of
    # 1/1024 m, so the ulp is put on the track's side: an uploaded track at -2^-22 m
    for gap, g in ((1, 2.0), (3, 3.0)):
        for name, x0 in (("at", 0.0), ("beyond", -2.0 ** -22)):
            add("gate_%s_gap_%d" % (name, gap), P(max_tracks=4), [("state", table(4, [track_slot(0, 1, (x0, 0, 0))]), 1, 2),
                                                                  ("update", points([[g, 0, 0]]), gap)])
    tr, de = shrinking_line(40)
    slots = table(64, [track_slot(k, k + 1, (x, 0, 0)) for k, x in enumerate(tr)])
    for name, rounds in (("need", 40), ("one_below", 39), ("one", 1)):
        add("line_rounds_" + name, P(max_tracks=64, max_rounds=rounds, gate_base=16.0, join_dist=-1.0),
            [("state", slots, 1, 41), ("update", points(np.stack([de, 0 * de, 0 * de], axis=1), half=2.0 ** -20), 1)])
    add("births_exceed_free_slots", P(max_tracks=3), [("update", grid_points(2), 0), ("update", grid_points(7), 1)])
    # a slot freed and taken again in one update; ids go on across expiries
    add("slot_reused_same_update", P(max_tracks=2, max_missed=0),
        [("update", grid_points(2), 0), ("update", points([[100, 0, 0], [200, 0, 0], [300, 0, 0]]), 1),
         ("update", points([[100, 0, 0]]), 2), ("update", points([[100, 0, 0], [0, 0, 0]]), 5)])
    for mm in (0, 1, 3):
        add("expiry_at_max_missed_%d" % mm, P(max_missed=mm),
            [("update", points([[0, 0, 0]]), 0)] + [("update", points([]), 1 + k) for k in range(mm + 1)] + [("update", points([[0, 0, 0]]), 9)])
        add("rematch_at_max_missed_%d" % mm, P(max_missed=mm, gate_speed=0.0),
            [("update", points([[0, 0, 0]]), 0)] + [("update", points([]), 1 + k) for k in range(mm)] +
            [("update", points([[0.5, 0, 0]]), 1 + mm), ("update", points([[1.0, 0, 0]]), 2 + mm)])
    for ch in (1, 2, 3):
        add("confirm_hits_%d" % ch, P(confirm_hits=ch), [("update", points([[0.25 * k, 0, 0]]), k) for k in range(4)])
    for dt in (1, 4):
        add("velocity_rules_dt_%d" % dt, P(gate_base=8.0),
            [("update", points([[0, 0, 0]]), 0), ("update", points([[0.75, 0.5, -0.25]]), dt), ("update", points([[1.75, 1.0, 0.0]]), 2 * dt),
             ("update", points([[2.0, 1.0, 0.125]]), 3 * dt)])
    add("hits_saturate", P(max_tracks=4), [("state", table(4, [track_slot(1, 7, (0, 0, 0), hits=65534, state=2),
                                                               track_slot(2, 3, (9, 0, 0), hits=65535, state=2)]), 5, 9),
                                           ("update", points([[0, 0, 0], [9, 0, 0]]), 5), ("update", points([[0, 0, 0], [9, 0, 0]]), 6)])
    bad = [track_slot(0, 1, (INF, 0, 0)), track_slot(1, 2, (0, NAN, 0)), track_slot(2, 3, (0, 0, 0), vel=(0, -INF, 0)),
           track_slot(3, 4, (1, 0, 0), vel=(NAN, 0, 0)), track_slot(5, 5, (3, 0, 0))]
    add("non_finite_tracks", P(max_tracks=8, max_missed=1), [("state", table(8, bad), 1, 6)] +
        [("update", points([[0, 0, 0], [3, 0, 0]]), k) for k in (1, 2, 3)])
    # joining
    chain = objects([(50, (k * 1.0, 0, 0), (k * 1.0 + 0.5, 1, 1)) for k in range(300)])
    add("join_chain_300", P(), [("update", chain, 0), ("update", chain[::-1].copy(), 1)])
    jd = f32(0.5)
    add("join_gap_at_and_beyond", P(join_dist=0.5), [("update", objects([(50, (0, 0, 0), (1, 1, 1)), (50, (f32(1) + jd, 0, 0), (3, 1, 1)),
                                                            (50, (10, 0, 0), (11, 1, 1)),
                                                            (50, (np.nextafter(f32(11) + jd, INF), 0, 0), (13, 1, 1))]), 0)])
    add("join_touching_dist_0", P(join_dist=0.0), [("update", objects([(50, (0, 0, 0), (1, 1, 1)), (50, (1, 1, 1), (2, 2, 2)),
                                                                       (50, (2.0625, 0, 0), (3, 1, 1))]), 0)])
    add("join_equal_boxes_other_labels", P(), [("update", objects([(50, (0, 0, 0), (1, 1, 1)), (10, (0, 0, 0), (1, 1, 1)),
                                                                   (50, (0, 0, 0), (1, 1, 1))]), 0)])
    add("join_off", P(join_dist=-1.0), [("update", objects([(50, (0, 0, 0), (1, 1, 1))] * 5), 0)])
    one = objects([(50, ((k % 64) * 0.25, (k // 64) * 0.25, 0), ((k % 64) * 0.25 + 0.25, (k // 64) * 0.25 + 0.25, 1), None, 1 + k % 7, k % 3)
                   for k in range(4096)])
    add("join_4096_in_one", P(), [("update", one, 0), ("update", one, 1)])
    add("join_signed_zero_box", P(), [("update", objects([(50, (0.0, -0.0, 0.0), (0.0, 0.0, -0.0)), (50, (-0.0, 0.0, 0.0), (-0.0, -0.0, 0.0)),
                                                          (50, (0.0, 0.0, -0.0), (0.0, 0.0, 0.0))]), 0)])
    add("join_non_finite_boxes", P(), [("update", objects([(50, (0, 0, 0), (1, 1, 1)), (50, (0, NAN, 0), (1, 1, 1), (0.5, 0.5, 0.5)),
                                                           (50, (0, 0, 0), (INF, 1, 1), (0.5, 0.5, 0.5)), (50, (0.5, 0, 0), (1, 1, 1)),
                                                           (50, (0, 0, 0), (1, 1, 1), (NAN, INF, -INF), 0)]), 0)])
    # the stamp rule: equal and lower stamps are refused, the state stays
    add("stamp_refusals", P(), [("update", points([[0, 0, 0]]), 4), ("update", points([[1, 0, 0]]), 4), ("update", points([[1, 0, 0]]), 2),
                                ("update", points([[1, 0, 0]]), 0xffffffff), ("update", points([[0.5, 0, 0]]), 5)])
    return out


def random_sequence(seed, n_objects, T=64):
    """eight updates over about n_objects objects: dyadic coordinates (multiples of 1/16 m), four labels, a drift per
    label, boxes that often touch, skipped scan ids, and an uploaded state with non-finite tracks in the middle"""
    rng = np.random.RandomState(seed)
    tp = TrackParams.defaults(max_tracks=T, max_rounds=64, join_dist=(0.5, 0.25, -1.0, 1.0)[seed % 4], max_missed=1 + seed % 3,
                              confirm_hits=1 + seed % 3)
    base = rng.randint(0, 64 * 16, (n_objects, 3)) / 16.0
    base[:, 2] = rng.randint(0, 32, n_objects) / 16.0
    labels = rng.choice([10, 50, 50, 71], n_objects)
    steps, scan = [], 0
    for u in range(8):
        keep = rng.rand(n_objects) < 0.85
        lo = base[keep] + u * np.array([0.25, 0.0625, 0.0]) * (labels[keep, None] == 10) + rng.randint(-2, 3, (int(keep.sum()), 3)) / 16.0
        size = rng.randint(1, 24, lo.shape) / 16.0
        cen = lo + size * rng.randint(0, 5, lo.shape) / 4.0
        rec = objects([(int(l), a, a + s, c, int(rng.randint(0, 40)), int(rng.randint(0, 3)), float(rng.randint(1, 99)) / 4.0)
                       for l, a, s, c in zip(labels[keep], lo, size, cen)])
        if u == 4:
            sl = np.zeros(T, dtype=OBJECT_TRACK_DTYPE)
            for t in range(0, T, 3):
                sl[t] = track_slot(t, 1 + t, base[t % max(n_objects, 1)] if n_objects else (0, 0, 0), vel=(0.25, 0, 0), hits=1 + t % 3,
                                   first=scan, last=scan)
            sl["position"][0, 0], sl["velocity"][min(3, T - 1), 1] = INF, NAN
            steps.append(("state", sl, scan, T + 5))
        steps.append(("update", rec, scan))
        scan += 1 + (u % 3 == 1) * 2
    return tp, steps


# ---- the scenario of DESIGN.md 19 / 21: per scan the objects, tracked with the defaults
def cube_box(scan, k=19):
    """(centre, half extents, yaw) of the moving cube at a scan, as synth._boxes gives it"""
    from semantic_suma_amd import synth
    c, h, yaw, _ = synth._boxes(scan)
    return c[k], h[k], yaw[k]


def scenario_measure(per_scan_objects, first_scan, update):
    """plays ``update(records, k) -> (tracks, object_tracks, counts, ...)`` over the scenario's objects, scan first_scan + k,
    and measures the quantities (a) .. (d) of DESIGN.md 21 -> dict"""
    import object_common as oc
    cube_object_scans, used, history, still, confirmed = [], {}, {}, 0.0, []
    for k, rec in enumerate(per_scan_objects):
        tracks, ot = update(rec, k)[:2]
        cube = cube_box(first_scan + k)
        has_object = bool(len(rec)) and bool((oc.inside_box(rec["centroid"], cube, 1.0) & (rec["label"] == 10)).any())
        if has_object:
            cube_object_scans.append(first_scan + k)
        confirmed.append(int((tracks["state"] == 2).sum()))
        for t in tracks:
            history.setdefault(int(t["id"]), []).append(t.copy())
            age = int(t["last_matched"]) - int(t["first_stamp"])
            mine = rec[ot == t["id"]]
            if has_object and t["label"] == 10 and t["detection"] != NONE and len(mine):
                w = np.maximum(mine["n_texels"].astype(np.float64), 1.0)
                c = (mine["centroid"].astype(np.float64) * w[:, None]).sum(axis=0) / w.sum()
                if oc.inside_box(c, cube, 1.0)[0]:
                    used.setdefault(int(t["id"]), []).append(first_scan + k)
            if t["label"] == 50 and t["state"] == 2 and age >= 8:
                net = (t["position"].astype(np.float64) - t["origin"]) / age
                still = max(still, float(np.linalg.norm(net)))
    out = dict(cube_object_scans=cube_object_scans, cube_track_scans=len({k for v in used.values() for k in v}), cube_ids=len(used),
               still_speed=still, net_error=None, velocity_error=None, net_velocity=None, cube_id=None, cube_id_scans=None,
               max_confirmed=max(confirmed) if confirmed else 0)
    if used:
        best = max(used, key=lambda i: len(history[i]))
        truth, errs, net = synth_step_in_map(), [], None
        for t in history[best]:
            age = int(t["last_matched"]) - int(t["first_stamp"])
            if age:
                net = (t["position"].astype(np.float64) - t["origin"]) / age if t["detection"] != NONE else net
            if t["state"] == 2 and t["detection"] != NONE:
                errs.append(float(np.linalg.norm(t["velocity"].astype(np.float64) - truth)))
        out.update(net_velocity=None if net is None else [float(x) for x in net],
                   net_error=None if net is None else float(np.linalg.norm(net - truth)),
                   velocity_error=max(errs) if errs else None, cube_id=best, cube_id_scans=used[best])
    return out


def synth_step_in_map():
    """the cube's true step per scan, (0.5, 0, 0) m in the world, turned into the map frame (the frame of pose 0)"""
    from semantic_suma_amd import synth
    T0 = synth.trajectory_pose(0)
    return np.linalg.inv(T0[:3, :3]) @ np.array([0.5, 0.0, 0.0])


# what tests/track_shim.c measured with the default parameters on the CPU restatement of the localiser
# (a) of the 18 scans in which cube 19 yields an object, those in which a class-10 track is matched to (or founded by) a
# detection whose centroid lies in the cube's true box grown by 1 m; (b) the distinct ids among them; (c) for the
# longest-lived of them, the error of its net displacement per scan against (0.5, 0, 0) m, and the largest error of its
# filtered velocity once confirmed; (d) the largest net speed of a confirmed class-50 track at least 8 scans old; (e) the
# control run's largest number of confirmed tracks in a scan
MEASURED = dict(cube_track_scans=18, cube_ids=2, net_error=0.041313, velocity_error=0.485095, still_speed=0.197391,
                control_confirmed=1)


def check_measured(cube_track_scans, cube_ids, net_error, velocity_error, still_speed, control_confirmed, net_velocity):
    """the issue's conditions: factor-two margins about the measured values, and the sanity condition"""
    M = MEASURED
    assert cube_track_scans > 0 and cube_track_scans >= 0.5 * M["cube_track_scans"], (cube_track_scans, M)
    assert cube_ids <= 2 * M["cube_ids"], (cube_ids, M)
    assert net_error <= 2 * M["net_error"] and velocity_error <= 2 * M["velocity_error"], (net_error, velocity_error, M)
    assert still_speed <= 2 * M["still_speed"], (still_speed, M)
    assert control_confirmed <= max(2 * M["control_confirmed"], 5), (control_confirmed, M)
    step = synth_step_in_map() / 0.5                                   # the unit vector of +x in the map frame
    along = float(np.dot(net_velocity, step))
    assert along > 0 and along > np.linalg.norm(np.asarray(net_velocity) - along * step), net_velocity
    assert still_speed < 0.25, still_speed
