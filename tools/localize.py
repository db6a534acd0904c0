#!/usr/bin/env python
"""Localisation in a finished map (core.Localizer, csrc/k_localize.hip): maps a synthetic sequence
(semantic_suma_amd/synth.py) or a KITTI directory (velodyne/*.bin, optionally labels/*.label) with SurfelMapping,
exports the map in the world frame (optionally voxel-fused) and localises a range of the same or of later scans in it --
or takes the map from a PLY written by tools/export_map.py (--map).  The map is never changed.  Prints one line per scan
(position, the two gate ratios, tracked, window rebuilds; the distance to the mapping pose of the same scan where one
exists) and a JSON summary.  --timing keeps the scans on the device and reports localisation scans/s beside the mapping
pipeline's scans/s over the same scans in the same run, and the cost of one window rebuild.  --relocalize starts without
a start pose; --evidence collects change evidence per map record while the scans are localised (csrc/k_change.hip), prints
every scan's totals and, with --prune-out, writes the map without the records the default rule removes (--without takes
objects out of the synthetic world the localised scans see).  --novel collects the surfaces no record of the map explains
(csrc/k_novel.hip), prints every scan's counts and, with --update-out, writes the updated map: the records the rule keeps
(all of them without --evidence) followed by the fused new ones (--map-without takes objects out of the world the mapping
run sees).  --objects (with --novel) segments each scan's unexplained texels into objects (csrc/k_objects.hip) and prints,
per scan, their number and each one's class, size, centroid and nearest range; --objects-out writes them as JSON.
--tracks (with --objects) follows the objects across the scans (csrc/k_tracks.hip) and prints, per scan, the confirmed
tracks: id, class, position, velocity, net velocity since birth, age and fragments; --tracks-out writes all tracks as JSON.  --deskew motion compensates the localised scans with the localiser's last increment (csrc/k_deskew.hip), for
sensors that deliver raw sweeps.  --live-grid GRID.npz (with --novel) switches the live obstacle layer on (csrc/k_live.hip) over
the traversability grid in GRID.npz (mapio.write_grid; a file that does not exist is made from the map as mapped, at
--grid-cell metres, and written), prints every scan's counts and live cells and, with --goal X Y, the path cost from the
robot's cell to the goal on the static grid and on the live one; --live-out writes the last composed grid.  With --relocalize the first scan goes through Localizer.relocalize against a place index (core.PlaceIndex) -- the mapping
run's own scans, or with --map the file tools/export_map.py --places wrote (--places).  Needs a GPU.
    python tools/localize.py [--map-scans 80] [--first 10] [--scans 60] [--voxel 0.1] [--width 2048] [--kitti sequences/08]
    python tools/localize.py --map map.ply --start 12.0 0.5 0.0 3.0 --first 11 --scans 20
    python tools/localize.py --timing                       # 64 x 2048, the 300-scan map, 60 scans
    python tools/localize.py --relocalize [--candidates 8]  # no setPose: the start comes from place recognition
    python tools/localize.py --map map.ply --places map.places.npz --relocalize --first 11 --scans 20
    python tools/localize.py --evidence --without 2 41 --prune-out pruned.ply   # cube 2 and a building are gone
    python tools/localize.py --map-without 2 41 --novel --update-out new.ply    # cube 2 and a building have arrived
    python tools/localize.py --map-without 2 41 --novel --objects [--objects-out objects.json]   # ... as objects, per scan
    python tools/localize.py --map-without 2 41 --novel --objects --live-grid grid.npz --goal 60 -8   # ... in the planner's grid
    python tools/localize.py --map-without 2 41 --novel --objects --tracks [--tracks-out tracks.json]   # ... followed across scans
    python tools/localize.py --kitti raw/sequence --deskew   # raw (uncompensated) sweeps: corrected in front of K1
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_suma_amd import core, kitti, mapio, places, synth  # noqa: E402
from semantic_suma_amd.types import LocalizerParams, PlaceParams, params_with_size  # noqa: E402


def read_scan(args, k, without=()):
    if args.kitti:
        bins = sorted(f for f in os.listdir(os.path.join(args.kitti, "velodyne")) if f.endswith(".bin"))
        pts = kitti.read_velodyne(os.path.join(args.kitti, "velodyne", bins[k]))
        lp = os.path.join(args.kitti, "labels", bins[k][:-4] + ".label")
        lab, prob = kitti.read_labels(lp, pts.shape[0]) if os.path.exists(lp) else (None, None)
        return pts, lab, prob
    return synth.generate_scan(k, n_azimuth=args.width, height=args.height, without=without)[:3]


def resident(ctx, scan):
    pts, lab, prob = (None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in scan)
    n = pts.reshape(-1, 4).shape[0]
    return ctx.device_array(pts), 0 if lab is None else ctx.device_array(lab), 0 if prob is None else ctx.device_array(prob), n


def event_ms(ctx, enqueue, repeats=10, warmup=3):
    """event times of `enqueue()` on the ctx stream, in ms"""
    import torch
    st = torch.cuda.ExternalStream(ctx.stream) if ctx.stream else torch.cuda.current_stream()
    out = []
    with torch.cuda.stream(st):
        for k in range(warmup + repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            enqueue()
            b.record(st)
            b.synchronize()
            if k >= warmup:
                out.append(a.elapsed_time(b))
    return out


def observe_timing(loc, scan, pose, n_window):
    """kc_observe's event time (suma_profile, one observation at a time) against an event-timed device-to-device copy of
    the bytes it touches: 64 a window record (48 of the record, 16 of its evidence) and the frame's three maps"""
    ctx, p = loc.ctx, loc.params
    frame = core.Frame(ctx, p.data_width, p.data_height)
    core.Preprocessing(ctx).process(scan[0], frame, scan[1], scan[2], p.active_timestamps + 10)
    ctx.profile(1)
    kernel = []
    for k in range(13):
        ctx.profile_reset()
        loc.observeFrame(frame, pose)
        ms = {r["name"]: r["total_ms"] for r in ctx.profile_get()}["change_observe"]
        if k >= 3:
            kernel.append(ms)
    ctx.profile(0)
    nbytes = 64 * n_window + 48 * p.data_width * p.data_height
    src, dst = ctx.device_array(np.zeros(nbytes, dtype=np.uint8)), ctx.device_array(np.zeros(nbytes, dtype=np.uint8))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    copy = event_ms(ctx, lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, C.c_void_p(ctx.stream)))
    ctx.device_free(src)
    ctx.device_free(dst)
    k, c = float(np.median(kernel)), float(np.median(copy))
    return dict(bytes=nbytes, kc_observe_us_median10=round(1e3 * k, 2), d2d_copy_us_median10=round(1e3 * c, 2),
                observe_over_copy=round(k / c, 3), samples=dict(kc_observe_ms=kernel, d2d_copy_ms=copy))


def collect_timing(loc, scan, pose, n_window, scan_id=0):
    """kn_mark's and kn_collect + kn_emit's event times (suma_profile, one collection at a time) against event-timed
    device-to-device copies of the bytes they touch: 32 a window record (16 of its position, 16 of the vertex texel) for
    the marks; the frame's three maps, nine mark bytes and a flag byte a texel for the collection.  ``scan_id``: the first of
    the collections' ids, which count up (the live layer wants them above the run's)"""
    ctx, p = loc.ctx, loc.params
    frame = core.Frame(ctx, p.data_width, p.data_height)
    core.Preprocessing(ctx).process(scan[0], frame, scan[1], scan[2], p.active_timestamps + 10)
    held = loc.novelCandidates(allow_overflow=True)
    ctx.profile(1)
    mark, collect = [], []
    for k in range(13):
        ctx.profile_reset()
        loc.collectFrame(frame, pose, scan_id + k)
        ms = {r["name"]: r["total_ms"] for r in ctx.profile_get()}
        if k >= 3:
            mark.append(ms["novel_mark"])
            collect.append(ms["novel_collect"])
    ctx.profile(0)
    loc.setNovelCandidates(held)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = {}
    for name, nbytes, kernel in (("kn_mark", 32 * n_window, mark), ("kn_collect", 58 * p.data_width * p.data_height, collect)):
        src, dst = ctx.device_array(np.zeros(nbytes, dtype=np.uint8)), ctx.device_array(np.zeros(nbytes, dtype=np.uint8))
        copy = event_ms(ctx, lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, C.c_void_p(ctx.stream)))
        ctx.device_free(src)
        ctx.device_free(dst)
        k, c = float(np.median(kernel)), float(np.median(copy))
        out[name] = dict(bytes=nbytes, kernel_us_median10=round(1e3 * k, 2), d2d_copy_us_median10=round(1e3 * c, 2),
                         kernel_over_copy=round(k / c, 3), samples=dict(kernel_ms=kernel, d2d_copy_ms=copy))
    return out


def objects_timing(loc, scan, pose, scan_id=0, tracked=False):
    """the event times of one segmentation's two kernel groups (suma_profile: kob_init + kob_merge + kob_flatten, and
    kob_vote + kob_emit + kob_ids) over the flags of one collection, each against an event-timed device-to-device copy of
    the bytes it touches (about 150 and 40 a texel: the vertex and semantic texels, the labels, the vote table, the ids; 96
    more per member for its accumulator are left out), and the host route timed in the same run: the flag, vertex and
    semantic images downloaded, then tests/object_shim.c (gcc -O2, one thread) over them.  ``tracked``: the tracks are on,
    every segmentation is followed by their update and wants a scan id of its own"""
    import subprocess
    import tempfile
    from semantic_suma_amd.types import ObjectCounts, ObjectParams, SCAN_OBJECT_DTYPE
    ctx, p = loc.ctx, loc.params
    W, H = p.data_width, p.data_height
    frame = core.Frame(ctx, W, H)
    core.Preprocessing(ctx).process(scan[0], frame, scan[1], scan[2], p.active_timestamps + 10)
    held = loc.novelCandidates(allow_overflow=True)
    loc.collectFrame(frame, pose, scan_id)
    loc.setNovelCandidates(held)
    flags = loc.novelFlags()
    ctx.profile(1)
    label, reduce_ = [], []
    for k in range(13):
        ctx.profile_reset()
        counts = loc.segmentFlags(frame, pose, flags, scan_id + 1 + k if tracked else 0)
        ms = {r["name"]: r["total_ms"] for r in ctx.profile_get()}
        if k >= 3:
            label.append(ms["objects_label"])
            reduce_.append(ms["objects_reduce"])
    ctx.profile(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = dict(counts=counts)
    for name, nbytes, kernel in (("label", 150 * W * H, label), ("reduce", 40 * W * H, reduce_)):
        src, dst = ctx.device_array(np.zeros(nbytes, dtype=np.uint8)), ctx.device_array(np.zeros(nbytes, dtype=np.uint8))
        copy = event_ms(ctx, lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, C.c_void_p(ctx.stream)))
        ctx.device_free(src)
        ctx.device_free(dst)
        k, c = float(np.median(kernel)), float(np.median(copy))
        out[name] = dict(launches=3, bytes=nbytes, kernel_us_median10=round(1e3 * k, 2), d2d_copy_us_median10=round(1e3 * c, 2),
                         kernel_over_copy=round(k / c, 3), samples=dict(kernel_ms=kernel, d2d_copy_ms=copy))
    # the host route
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "object_shim.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared",
                               os.path.join(root, "tests", "object_shim.c"), "-o", so, "-lm"])
        shim = C.CDLL(so)
        shim.object_shim_segment.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_int32, C.c_void_p, C.POINTER(ObjectParams),
                                                                 C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(ObjectCounts)]
        shim.object_shim_segment.restype = None
        op, cnt = ObjectParams.defaults(), ObjectCounts()
        rec, ids = np.zeros(op.max_objects, dtype=SCAN_OBJECT_DTYPE), np.zeros(W * H, dtype=np.uint32)
        Tc = np.ascontiguousarray(np.asarray(pose, dtype=np.float64).T)
        download, host = [], []
        for k in range(13):
            ctx.synchronize()
            t0 = time.perf_counter()
            fl, V, S = loc.novelFlags(), frame.download(0), frame.download(2)
            t1 = time.perf_counter()
            shim.object_shim_segment(V.ctypes.data, S.ctypes.data, fl.ctypes.data, W, H, Tc.ctypes.data, C.byref(op), 0,
                                     rec.ctypes.data, ids.ctypes.data, C.byref(cnt))
            t2 = time.perf_counter()
            if k >= 3:
                download.append(1e3 * (t1 - t0))
                host.append(1e3 * (t2 - t1))
        same = cnt.as_dict() == counts and rec[:cnt.stored].tobytes() == loc.objects(allow_overflow=True)[0].tobytes()
    out["host_route"] = dict(download_us_median10=round(1e3 * float(np.median(download)), 2),
                             shim_us_median10=round(1e3 * float(np.median(host)), 2), equals_device=bool(same),
                             samples=dict(download_ms=download, shim_ms=host))
    return out


def live_timing(loc, scan, pose, live):
    """the event times of the live layer's three kernels (suma_profile: klv_hit, klv_carve, klv_compose) over the flags of
    one collection -- each update with a stamp of its own on the state the run left --, each against an event-timed
    device-to-device copy of the bytes it touches (hit: the vertex texel, the flag and the id, 21 a texel; carve: the
    vertex texel, 16 a texel, and what the rays read, which depends on the scene and is left out; compose: 48 + 16 read and
    48 + 1 written a cell), and the host route timed in the same run: the flag, vertex and id images downloaded, then
    tests/live_shim.c (gcc -O2, one thread) over them"""
    import subprocess
    import tempfile
    from semantic_suma_amd.types import LIVE_CELL_DTYPE, LiveCounts, LiveParams
    ctx, p = loc.ctx, loc.params
    W, H = p.data_width, p.data_height
    gp = live["gp"]
    n_cells = int(gp.width) * int(gp.height)
    frame = core.Frame(ctx, W, H)
    core.Preprocessing(ctx).process(scan[0], frame, scan[1], scan[2], p.active_timestamps + 10)
    flags = loc.novelFlags()
    d_cells = ctx.device_array(np.zeros(n_cells * 48, dtype=np.uint8))
    base = 1 << 20                                     # scan ids far above the run's
    ctx.profile(1)
    hit, carve, compose = [], [], []
    for k in range(13):
        ctx.profile_reset()
        counts = loc.liveUpdateFlags(frame, pose, flags, base + k)
        stats = loc.liveCells(out=d_cells)[2]
        ms = {r["name"]: r["total_ms"] for r in ctx.profile_get()}
        if k >= 3:
            hit.append(ms["live_hit"])
            carve.append(ms.get("live_carve", 0.0))
            compose.append(ms["live_compose"])
    ctx.profile(0)
    ctx.device_free(d_cells)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = dict(counts=counts, stats=stats, cells=n_cells)
    for name, nbytes, kernel in (("hit", 21 * W * H, hit), ("carve", 16 * W * H, carve), ("compose", 113 * n_cells, compose)):
        src, dst = ctx.device_array(np.zeros(nbytes, dtype=np.uint8)), ctx.device_array(np.zeros(nbytes, dtype=np.uint8))
        copy = event_ms(ctx, lambda: hip.hipMemcpyAsync(dst, src, nbytes, 3, C.c_void_p(ctx.stream)))
        ctx.device_free(src)
        ctx.device_free(dst)
        k, c = float(np.median(kernel)), float(np.median(copy))
        out[name] = dict(bytes=nbytes, kernel_us_median10=round(1e3 * k, 2), d2d_copy_us_median10=round(1e3 * c, 2),
                         kernel_over_copy=round(k / c, 3), samples=dict(kernel_ms=kernel, d2d_copy_ms=copy))
    # the host route: one more update on the device and on the host from the same state
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import live_common as lv
    with tempfile.TemporaryDirectory() as tmp:
        shim = lv.build_shim(tmp)
        download, host = [], []
        same = True
        for k in range(13):
            layer = lv.ShimLayer(shim, live["static"], gp, live["lp"])
            layer.set_state(loc.liveState(), base + 12 + k)
            ctx.synchronize()
            t0 = time.perf_counter()
            fl, V = loc.novelFlags(), frame.download(0)
            ids = loc.objectIds() if live["objects"] else None
            t1 = time.perf_counter()
            layer.update(V, fl, pose, base + 13 + k, ids)
            comp = layer.compose()
            t2 = time.perf_counter()
            loc.liveUpdateFlags(frame, pose, flags, base + 13 + k)
            got = loc.liveCells()
            same = same and got[0].tobytes() == comp[0].tobytes() and loc.liveState().tobytes() == layer.state().tobytes()
            if k >= 3:
                download.append(1e3 * (t1 - t0))
                host.append(1e3 * (t2 - t1))
    out["host_route"] = dict(download_us_median10=round(1e3 * float(np.median(download)), 2),
                             shim_us_median10=round(1e3 * float(np.median(host)), 2), equals_device=bool(same),
                             samples=dict(download_ms=download, shim_ms=host))
    return out


def tracks_timing(loc, base):
    """the event times of one tracker update's two kernel groups (suma_profile: ktr_init + ktr_join + ktr_reduce, and
    ktr_track) over the records of the last segmentation, each update with a stamp of its own on the state the run left,
    and the host route timed in the same run: the object records downloaded, then tests/track_shim.c (gcc -O2, one
    thread) over them from the same state"""
    import tempfile
    ctx = loc.ctx
    rec = loc.objects(allow_overflow=True)[0]
    ctx.profile(1)
    join, update = [], []
    for k in range(13):
        ctx.profile_reset()
        counts = loc.trackObjects(rec, base + k)
        ms = {r["name"]: r["total_ms"] for r in ctx.profile_get()}
        if k >= 3:
            join.append(ms["tracks_join"])
            update.append(ms["tracks_update"])
    ctx.profile(0)
    out = dict(counts=counts, objects=int(len(rec)),
               join=dict(launches=3, kernel_us_median10=round(1e3 * float(np.median(join)), 2), samples=dict(kernel_ms=join)),
               update=dict(launches=1, kernel_us_median10=round(1e3 * float(np.median(update)), 2), samples=dict(kernel_ms=update)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    import track_common as tc
    with tempfile.TemporaryDirectory() as tmp:
        shim = tc.build_shim(tmp)
        download, host, same = [], [], True
        for k in range(13):
            want = tc.ShimTracker(shim, loc._track_params)
            want.set_state(*loc.trackState())
            ctx.synchronize()
            t0 = time.perf_counter()
            got = loc.objects(allow_overflow=True)[0]
            t1 = time.perf_counter()
            w = want.update(got, base + 13 + k)
            t2 = time.perf_counter()
            loc.trackObjects(rec, base + 13 + k)
            same = same and loc.tracks(allow_overflow=True)[0].tobytes() == w[0].tobytes() and \
                loc.trackState()[0].tobytes() == want.slots.tobytes()
            if k >= 3:
                download.append(1e3 * (t1 - t0))
                host.append(1e3 * (t2 - t1))
    out["host_route"] = dict(download_us_median10=round(1e3 * float(np.median(download)), 2),
                             shim_us_median10=round(1e3 * float(np.median(host)), 2), equals_device=bool(same),
                             samples=dict(download_ms=download, shim_ms=host))
    return out


def added_footprints(gp, boxes):
    """bool per cell: the centre lies inside the x / y extent of one of synth._boxes(0)'s ``boxes`` (the grid's frame is
    that of scan 0)"""
    c, h, yaw, _ = synth._boxes(0)
    T0 = synth.trajectory_pose(0)
    ix, iy = np.meshgrid(np.arange(gp.width), np.arange(gp.height))
    xyz = np.stack([gp.origin_x + (ix + 0.5) * gp.cell_size, gp.origin_y + (iy + 0.5) * gp.cell_size, np.zeros(ix.shape)],
                   -1).reshape(-1, 3) @ T0[:3, :3].T + T0[:3, 3]
    out = np.zeros(len(xyz), dtype=bool)
    for b in boxes:
        cs, sn = np.cos(yaw[b]), np.sin(yaw[b])
        q = (xyz - c[b]) @ np.array([[cs, sn, 0], [-sn, cs, 0], [0, 0, 1]]).T
        out |= np.all(np.abs(q[:, :2]) <= h[b][:2], axis=1)
    return out


def pose_from(x, y, z, yaw_deg):
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = x, y, z
    return T


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map", default=None, help="a PLY of tools/export_map.py / mapio.write_ply instead of a mapping run")
    ap.add_argument("--map-scans", type=int, default=None, help="scans the mapping run integrates (default 80; --timing: 300)")
    ap.add_argument("--first", type=int, default=None, help="first scan to localise (default: 20 scans before the end of the map)")
    ap.add_argument("--scans", type=int, default=60, help="scans to localise")
    ap.add_argument("--kitti", default=None, help="a sequences/XX directory")
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--voxel", type=float, default=0.0, help="voxel size of the exported map in metres; 0: one record per surfel")
    ap.add_argument("--extent", type=float, default=None, help="submap_extent")
    ap.add_argument("--dimension", type=int, default=None, help="submap_dimension")
    ap.add_argument("--iterations", type=int, default=0, help="fixed Gauss-Newton iterations; 0: until convergence")
    ap.add_argument("--no-motion-model", action="store_true", help="guess = the last pose (constant_velocity = 0)")
    ap.add_argument("--start", type=float, nargs=4, metavar=("X", "Y", "Z", "YAW_DEG"), default=None,
                    help="start pose (default: the mapping pose of scan --first; identity with --map)")
    ap.add_argument("--save-map", default=None, help="write the exported map as a PLY")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--relocalize", action="store_true", help="no start pose: the first scan is relocalised in a place index")
    ap.add_argument("--places", default=None, help="with --map: the place index tools/export_map.py --places wrote")
    ap.add_argument("--candidates", type=int, default=8, help="places a relocalisation tries (1 .. 32)")
    ap.add_argument("--place-range", type=float, default=80.0, help="max_range of the place descriptor in metres")
    ap.add_argument("--evidence", action="store_true", help="collect change evidence per map record and print every scan's totals")
    ap.add_argument("--prune-out", default=None, metavar="FILE.ply", help="with --evidence: write the map the default rule keeps")
    ap.add_argument("--without", type=int, nargs="*", default=[], metavar="BOX",
                    help="synthetic scans: boxes of synth._boxes the localised scans do not see (0-22 cubes, 23.. buildings)")
    ap.add_argument("--deskew", action="store_true",
                    help="the localised scans are raw sweeps: motion compensate them with the last increment (azimuth time, "
                         "counter-clockwise, t_ref 0.5)")
    ap.add_argument("--novel", action="store_true", help="collect the surfaces no map record explains and print every scan's counts")
    ap.add_argument("--update-out", default=None, metavar="FILE.ply",
                    help="with --novel: write the updated map (what the rule keeps, then the fused new records)")
    ap.add_argument("--objects", action="store_true",
                    help="with --novel: segment each scan's unexplained texels into objects and print them")
    ap.add_argument("--objects-out", default=None, metavar="FILE.json", help="with --objects: write every scan's objects")
    ap.add_argument("--map-without", type=int, nargs="*", default=[], metavar="BOX",
                    help="synthetic scans: boxes of synth._boxes the mapping run does not see")
    ap.add_argument("--tracks", action="store_true",
                    help="with --objects: track the objects across the scans and print every scan's confirmed tracks")
    ap.add_argument("--tracks-out", default=None, metavar="FILE.json", help="with --tracks: write every scan's tracks")
    ap.add_argument("--live-grid", default=None, metavar="GRID.npz",
                    help="with --novel: the live obstacle layer over this traversability grid (made from the map and written "
                         "when the file does not exist)")
    ap.add_argument("--grid-cell", type=float, default=0.2, help="cell size of a grid --live-grid makes, in metres")
    ap.add_argument("--live-out", default=None, metavar="FILE.npz", help="with --live-grid: write the last composed grid")
    ap.add_argument("--goal", type=float, nargs=2, metavar=("X", "Y"), default=None,
                    help="with --live-grid: print per scan the path cost from the robot's cell to this world position on "
                         "the static grid and on the live one (unknown cells count as traversable)")
    args = ap.parse_args()
    if args.live_grid and not args.novel:
        ap.error("--live-grid needs --novel")
    if (args.live_out or args.goal) and not args.live_grid:
        ap.error("--live-out and --goal need --live-grid")
    if args.prune_out and not args.evidence:
        ap.error("--prune-out needs --evidence")
    if args.update_out and not args.novel:
        ap.error("--update-out needs --novel")
    if args.objects and not args.novel:
        ap.error("--objects needs --novel")
    if args.objects_out and not args.objects:
        ap.error("--objects-out needs --objects")
    if args.tracks and not args.objects:
        ap.error("--tracks needs --objects")
    if args.tracks_out and not args.tracks:
        ap.error("--tracks-out needs --tracks")
    over = {k: v for k, v in (("submap_extent", args.extent), ("submap_dimension", args.dimension)) if v is not None}
    p = params_with_size(args.width, args.height, **over)
    n_map = args.map_scans if args.map_scans is not None else (300 if args.timing else 80)
    first = args.first if args.first is not None else (0 if args.map else max(0, n_map - args.scans - 20))
    ks = list(range(first, first + args.scans))
    res = dict(width=args.width, height=args.height, first=first, scans=args.scans, voxel_size=args.voxel,
               fixed_iterations=args.iterations, constant_velocity=int(not args.no_motion_model))

    map_poses = {}
    index, entry_poses = None, None
    if args.relocalize and args.map and not args.places:
        ap.error("--relocalize with --map needs --places")
    if args.map:
        records, _ = mapio.read_ply(args.map)
        res["map"] = args.map
        if args.relocalize:
            index, entry_poses = places.load(args.places)
    else:
        pipe = core.SurfelMapping(p)
        if args.relocalize:
            index = core.PlaceIndex(PlaceParams.defaults(max_range=args.place_range), capacity=n_map)
        mapping_s, timed = 0.0, 0
        for k in range(n_map):
            sc = read_scan(args, k, tuple(args.map_without))
            if args.timing and k in ks and k > 0:  # the mapping rate over the scans that are localised below, resident
                d = resident(pipe.ctx, sc)
                pipe.ctx.synchronize()
                t = time.perf_counter()
                pipe.processScanDevice(*d, fixed_iterations=args.iterations)
                pipe.ctx.synchronize()
                mapping_s += time.perf_counter() - t
                timed += 1
                for a in d[:3]:
                    if a:
                        pipe.ctx.device_free(a)
            else:
                pipe.processScan(*sc, fixed_iterations=args.iterations)
            map_poses[k] = pipe.getCurrentPose()
            if index is not None:
                index.addFrame(pipe.ctx, pipe.frame(0), k)
        if index is not None:
            entry_poses = np.stack([map_poses[k] for k in range(n_map)])
        t = time.perf_counter()
        records, st = pipe.map.export_world(voxel_size=args.voxel, stats=True)
        res.update(map_scans=n_map, export_ms=round(1e3 * (time.perf_counter() - t), 3), export=st)
        if timed:
            res["mapping_scans_per_s"] = round(timed / mapping_s, 2)
        if args.save_map:
            mapio.write_ply(args.save_map, records)
        pipe.close()

    loc = core.Localizer(p, LocalizerParams.defaults(p, constant_velocity=int(not args.no_motion_model)))
    if args.evidence:
        loc.enableEvidence()
    if args.novel:
        loc.enableNovelty()
    if args.objects:
        loc.enableObjects()
    if args.tracks:
        loc.enableTracks()
    if args.deskew:
        loc.enableDeskew()
        res["deskew"] = True
    live = None
    if args.live_grid:
        from semantic_suma_amd.types import LiveParams, PlanParams
        if os.path.exists(args.live_grid):
            cells, gp = mapio.read_grid(args.live_grid)
        else:
            cells, gp, _ = core.world_grid(loc.ctx, records, cell_size=args.grid_cell)
            mapio.write_grid(args.live_grid, cells, gp)
        loc.enableLiveGrid(cells, gp)
        live = dict(gp=gp, static=cells, lp=LiveParams.defaults(), objects=bool(args.objects), per_scan=[], d_cells=loc.ctx.device_array(np.zeros(cells.size * 48, dtype=np.uint8)))
        res["live_grid"] = dict(file=args.live_grid, width=int(gp.width), height=int(gp.height), cell_size=float(gp.cell_size))
        if args.goal:
            live["pp"] = PlanParams.defaults(unknown_blocked=False)
            live["goal"] = core.grid_cell_index(gp, *args.goal)
            if live["goal"] < 0:
                ap.error("--goal lies outside the grid")
            live["static_field"] = core.grid_plan(loc.ctx, cells, gp, [live["goal"]], live["pp"])[0]
            live["added"] = added_footprints(gp, args.map_without) if args.map_without and not args.kitti else None
    t = time.perf_counter()
    dropped = loc.setMap(records)
    res.update(map_records=int(len(records)), dropped=dropped, set_map_ms=round(1e3 * (time.perf_counter() - t), 3))
    start = pose_from(*args.start) if args.start else map_poses.get(first, np.eye(4))
    if not args.relocalize:
        loc.setPose(start)
    scans = [read_scan(args, k, tuple(args.without)) for k in ks]
    host_scans = scans
    observations, collections, objects, tracks = [], [], [], []
    if args.timing:
        scans = [resident(loc.ctx, sc) for sc in scans]
        loc.ctx.synchronize()
    out = []
    t = time.perf_counter()
    for k, sc in zip(ks, scans):
        try:
            if args.relocalize and not out:  # the first scan: no pose yet
                t_rel = time.perf_counter()
                rel = (loc.relocalizeDevice if args.timing else loc.relocalize)(
                    index, entry_poses, *sc, max_candidates=args.candidates, fixed_iterations=args.iterations)
                res["relocalisation"] = dict(found=rel["found"], n_tried=rel["n_tried"], winner=rel["winner"],
                                             match=rel["match"], ms=round(1e3 * (time.perf_counter() - t_rel), 3),
                                             tried=[dict(c["match"], tracked=c["result"]["tracked"]) for c in rel["candidates"]])
                if not rel["found"]:
                    res.update(lost_at_scan=k, error="the relocalisation found no place")
                    break
                start = rel["result"]["pose"]
                out.append(rel["result"])
                continue
            out.append(loc.processScanDevice(*sc, fixed_iterations=args.iterations) if args.timing
                       else loc.processScan(*sc, fixed_iterations=args.iterations))
            if args.evidence:
                observations.append(loc.lastObservation())
            if args.novel and not args.timing:  # the counts wait for the device: a timed run asks once, at the end
                collections.append(loc.lastCollection(allow_overflow=True))
            if args.objects and not args.timing:
                objects.append(loc.objects(allow_overflow=True))
            if args.tracks and not args.timing:
                tracks.append(loc.tracks(allow_overflow=True))
            if live and not args.timing:
                gp, T = live["gp"], out[-1]["pose"]
                entry = dict(scan=k, counts=loc.liveCounts())
                _, mask, entry["stats"] = loc.liveCells(out=live["d_cells"])
                if args.goal:
                    start = core.grid_cell_index(gp, float(T[0, 3]), float(T[1, 3]))
                    field = core.grid_plan(loc.ctx, live["d_cells"], gp, [live["goal"]], live["pp"])[0]
                    if start >= 0:
                        entry["static_cost"] = int(live["static_field"].reshape(-1)["cost"][start])
                        entry["live_cost"] = int(field.reshape(-1)["cost"][start])
                        pres, prow = core.grid_paths(loc.ctx, field, gp, [start])
                        path = prow[0, :min(int(pres["length"][0]), prow.shape[1])]
                        entry["path_cells"] = int(len(path))
                        if live["added"] is not None:
                            entry["path_cells_in_added_boxes"] = int(live["added"][path].sum())
                live["per_scan"].append(entry)
        except core.SumaError as e:  # a run that has left the map ends on a pose that is no longer finite
            res.update(lost_at_scan=k, error=str(e))
            break
    loc.ctx.synchronize()
    wall = time.perf_counter() - t
    worst = 0.0
    for k, r in zip(ks, out):
        T = r["pose"]
        err = float(np.linalg.norm(T[:3, 3] - map_poses[k][:3, 3])) if k in map_poses else float("nan")
        worst = max(worst, err) if err == err else worst
        if "first_beyond_half_a_metre" not in res and err > 0.5:
            res["first_beyond_half_a_metre"] = k
        print(f"scan {k:5d}  xyz {T[0, 3]:10.3f} {T[1, 3]:10.3f} {T[2, 3]:8.3f}  valid {r['valid_ratio']:.3f} "
              f"outlier {r['outlier_ratio']:.3f}  tracked {int(r['tracked'])}  rebuilt {int(r['window_rebuilt'])}  "
              f"origin {r['origin']}  window {r['n_window']}  to mapping pose {err:.3f} m")
    if args.evidence:
        for k, (cnt, observed) in zip(ks[len(ks) - len(observations):] if args.relocalize else ks, observations):
            print(f"scan {k:5d}  observed {int(observed)}  " + "  ".join(f"{n} {v}" for n, v in cnt.items()))
        ev = loc.evidence()
        kept, keep = core.pruned_map(records, ev)
        res["evidence"] = dict({f: int(ev[f].sum()) for f in ev.dtype.names}, observed_scans=sum(o for _, o in observations),
                               records_with_misses=int((ev["misses"] > 0).sum()), pruned=int((~keep).sum()), kept=int(len(kept)))
        if args.prune_out:
            mapio.write_ply(args.prune_out, kept)
            res["pruned_map"] = args.prune_out
    if args.novel:
        for k, (cnt, collected) in zip(ks[len(ks) - len(collections):] if args.relocalize else ks, collections):
            print(f"scan {k:5d}  collected {int(collected)}  " + "  ".join(f"{n} {v}" for n, v in cnt.items()))
        fused, views, st = loc.novel(allow_overflow=True, stats=True)
        res["novel"] = dict(st, candidates_per_scan=round(st["n_candidates"] / max(1, len(out)), 1),
                            candidate_bytes=48 * st["n_candidates"],
                            per_scan=[c["stored"] for c, _ in collections] if collections else None,
                            max_views=int(views.max()) if len(views) else 0)
        if args.update_out:
            upd = np.concatenate([core.pruned_map(records, loc.evidence())[0] if args.evidence else records, fused])
            mapio.write_ply(args.update_out, upd)
            res.update(updated_map=args.update_out, updated_records=int(len(upd)))
    if args.objects:
        listing = []
        for k, got in zip(ks[len(ks) - len(objects):] if args.relocalize else ks, objects):
            rec, cnt = got if got is not None else ((), dict(n_objects=0, n_small=0, n_members=0))
            print(f"scan {k:5d}  objects {cnt['n_objects']}  small {cnt['n_small']}  members {cnt['n_members']}")
            for o in rec:
                size = o["max"] - o["min"]
                print(f"            class {int(o['label']):3d} ({float(o['prob']):.2f})  texels {int(o['n_texels']):5d}  "
                      f"dynamic {int(o['n_dynamic']):4d}  size {size[0]:6.2f} {size[1]:6.2f} {size[2]:6.2f}  "
                      f"centroid {o['centroid'][0]:9.3f} {o['centroid'][1]:9.3f} {o['centroid'][2]:7.3f}  "
                      f"nearest {float(o['r_min']):7.3f} m")
            listing.append(dict(scan=k, counts=cnt, objects=[
                dict(root=int(o["root"]), n_texels=int(o["n_texels"]), label=int(o["label"]), prob=float(o["prob"]),
                     n_dynamic=int(o["n_dynamic"]), min=[float(v) for v in o["min"]], max=[float(v) for v in o["max"]],
                     centroid=[float(v) for v in o["centroid"]], r_min=float(o["r_min"])) for o in rec]))
        last = loc.objects(allow_overflow=True)
        res["objects"] = dict(per_scan=[e["counts"]["n_objects"] for e in listing] if listing else None,
                              last_scan=None if last is None else last[1])
        if args.objects_out:
            with open(args.objects_out, "w") as f:
                json.dump(listing, f)
            res["objects_file"] = args.objects_out
    if args.tracks:
        from semantic_suma_amd.types import ObjectTrack
        listing = []
        for k, got in zip(ks[len(ks) - len(tracks):] if args.relocalize else ks, tracks):
            rec, cnt = got if got is not None else ((), dict(n_detections=0, n_matched=0, n_born=0, n_expired=0))
            conf = [ObjectTrack(r) for r in rec if r["state"] == 2]
            print(f"scan {k:5d}  tracks {len(rec)}  confirmed {len(conf)}  detections {cnt['n_detections']}  matched "
                  f"{cnt['n_matched']}  born {cnt['n_born']}  expired {cnt['n_expired']}")
            for t in conf:
                v, nv = t.velocity, t.net_velocity
                print(f"            id {t.id:4d}  class {t.label:3d}  position {t.position[0]:9.3f} {t.position[1]:9.3f} "
                      f"{t.position[2]:7.3f}  velocity {v[0]:6.2f} {v[1]:6.2f} {v[2]:6.2f}  net {nv[0]:6.2f} {nv[1]:6.2f} {nv[2]:6.2f} "
                      f"({float(np.linalg.norm(nv)):.3f} a scan)  age {t.age:3d}  missed {t.missed}  fragments {t.n_objects}")
            listing.append(dict(scan=k, counts=cnt, tracks=[ObjectTrack(r).as_dict() for r in rec]))
        last = loc.tracks(allow_overflow=True)
        res["tracks"] = dict(confirmed_per_scan=[sum(1 for t in e["tracks"] if t["confirmed"]) for e in listing] if listing else None,
                             last_scan=None if last is None else last[1], ids_given=loc.trackState()[2] - 1)
        if args.tracks_out:
            with open(args.tracks_out, "w") as f:
                json.dump(listing, f)
            res["tracks_file"] = args.tracks_out
    if live:
        for e in live["per_scan"]:
            c, st = e["counts"] or {}, e["stats"]
            line = (f"scan {e['scan']:5d}  live {st['n_live']}  pending {st['n_pending']}  expired {st['n_expired']}  carved "
                    f"{st['n_carved']}  hit texels {c.get('n_hit_texels', 0)}  hit cells {c.get('n_hit_cells', 0)}  cleared "
                    f"{c.get('n_cleared', 0)}")
            if "live_cost" in e:
                line += f"  path cost static {e['static_cost']}  live {e['live_cost']}  cells {e['path_cells']}"
                if "path_cells_in_added_boxes" in e:
                    line += f"  of them in the added boxes {e['path_cells_in_added_boxes']}"
            print(line)
        comp, mask, st = loc.liveCells()
        res["live"] = dict(last=st, per_scan=[e["stats"]["n_live"] for e in live["per_scan"]] or None)
        if args.live_out:
            mapio.write_grid(args.live_out, comp, live["gp"])
            res["live_file"] = args.live_out
    origin, n_window, rebuilds = loc.window()
    res.update(tracked=sum(r["tracked"] for r in out), window_rebuilds=sum(r["window_rebuilt"] for r in out),
               n_window=n_window, worst_distance_to_mapping_pose_m=round(worst, 4))
    if args.timing and out:
        res["localisation_scans_per_s"] = round(len(out) / wall, 2)
        # one window rebuild: the gather of setPose at the pose the run ended on, behind a synchronisation
        T, times = (start if "lost_at_scan" in res or "first_beyond_half_a_metre" in res else out[-1]["pose"]), []
        for _ in range(5):
            loc.ctx.synchronize()
            t = time.perf_counter()
            loc.setPose(T)
            loc.ctx.synchronize()
            times.append(time.perf_counter() - t)
        res["window_rebuild_ms"] = [round(1e3 * x, 3) for x in times]
        if args.evidence and "lost_at_scan" not in res:
            res["observe"] = observe_timing(loc, host_scans[len(out) - 1], out[-1]["pose"], loc.window()[1])
        if args.novel and "lost_at_scan" not in res:
            res["collect"] = collect_timing(loc, host_scans[len(out) - 1], out[-1]["pose"], loc.window()[1], (1 << 18) if live or args.tracks else 0)
        if args.objects and "lost_at_scan" not in res:
            res["segment"] = objects_timing(loc, host_scans[len(out) - 1], out[-1]["pose"], (1 << 19) if live or args.tracks else 0, tracked=args.tracks)
        if live and "lost_at_scan" not in res:
            res["live_timing"] = live_timing(loc, host_scans[len(out) - 1], out[-1]["pose"], live)
        if args.tracks and "lost_at_scan" not in res:
            res["tracks_timing"] = tracks_timing(loc, 1 << 21)
    loc.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
