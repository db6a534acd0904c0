#!/usr/bin/env python
"""The finished map as a point cloud: runs a synthetic sequence (semantic_suma_amd/synth.py) or a KITTI directory
(velodyne/*.bin, optionally labels/*.label) through SurfelMapping, optionally closing loops, then exports the whole map
-- active surfels and every parked submap tile -- in the world frame on the GPU (SurfelMap.export_world,
csrc/k_world.hip) and writes it as a binary PLY (semantic_suma_amd/mapio.py).  Prints the export's stats and the wall
time of the export alone; --compare also times the host route (getAllSurfels + per-tile downloads + a numpy transform).
--places FILE adds every scan's frame to a place index (core.PlaceIndex, csrc/k_place.hip) right behind the scan and
writes it with the final trajectory -- the pose table, i.e. with loop closing the poses after integration -- for
tools/localize.py --relocalize (semantic_suma_amd/places.py).
--grid FILE.npz also writes the map's 2.5-D traversability grid for a planner (SurfelMap.export_grid, csrc/k_grid.hip;
mapio.write_grid), --grid-png a picture of its cell states (white unknown, green free, red obstacle, grey no ground);
with --compare the grid's device time is printed next to a numpy binning of the downloaded records.  Needs a GPU.
    python tools/export_map.py --out map.ply [--scans 40] [--kitti sequences/08] [--voxel 0.2] [--min-confidence 0]
                               [--close-loops] [--width 2048] [--compare] [--places map.places.npz]
                               [--grid map.grid.npz [--grid-cell 0.2] [--grid-png map.grid.png]]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_suma_amd import core, kitti, mapio, places, synth  # noqa: E402
from semantic_suma_amd.types import SURFEL_DTYPE, LoopParams, PlaceParams, params_with_size  # noqa: E402


def scans(args):
    if args.kitti:
        bins = sorted(f for f in os.listdir(os.path.join(args.kitti, "velodyne")) if f.endswith(".bin"))[:args.scans]
        for b in bins:
            pts = kitti.read_velodyne(os.path.join(args.kitti, "velodyne", b))
            lp = os.path.join(args.kitti, "labels", b[:-4] + ".label")
            lab, prob = kitti.read_labels(lp, pts.shape[0]) if os.path.exists(lp) else (None, None)
            yield pts, lab, prob
    else:
        for k in range(args.scans):
            pts, lab, prob, _ = synth.generate_scan(k, n_azimuth=args.width, height=64)
            yield pts, lab, prob


def host_route(smap, max_poses):
    """what a consumer had to do before: download every source record and redo the pose lookup in numpy (fp64 here: a
    host has no reason to restate the fma chain) -- the positions only, no filter, no voxels"""
    parts = [smap.getAllSurfels()]
    for i, j in smap.cached_tiles():
        parts.append(np.ascontiguousarray(smap.cached_tile(i, j)).view(SURFEL_DTYPE).reshape(-1))
    s = np.concatenate(parts)
    table = np.tile(np.eye(4), (max_poses, 1, 1))
    poses = smap.poses()
    table[:len(poses)] = poses
    c = s["count"]
    k = np.where(c >= 0, np.where(c < max_poses, np.nan_to_num(c, nan=0.0), max_poses - 1), 0).astype(np.int64)
    M = table[k]
    p = np.einsum("nij,nj->ni", M[:, :3, :3], np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float64)) + M[:, :3, 3]
    return p.astype(np.float32)


GRID_STATE_RGBA = np.array([[255, 255, 255, 255], [60, 170, 80, 255], [200, 40, 40, 255], [128, 128, 128, 255]], np.uint8)


def numpy_grid_route(world, gp):
    """the host route to a grid: the downloaded records binned in numpy -- the cell index, the occupancy and the lowest
    and highest z per cell only; no vote, no ground rule, no fill.  -> (occupied cells, z_min, z_max per cell)"""
    fx = np.floor((world["x"] - np.float32(gp.origin_x)) / np.float32(gp.cell_size))
    fy = np.floor((world["y"] - np.float32(gp.origin_y)) / np.float32(gp.cell_size))
    ok = np.isfinite(world["z"]) & (fx >= 0) & (fx < gp.width) & (fy >= 0) & (fy < gp.height)
    c = (fy[ok].astype(np.int64) * gp.width + fx[ok].astype(np.int64))
    z = world["z"][ok]
    lo = np.full(gp.width * gp.height, np.inf, np.float32)
    hi = np.full(gp.width * gp.height, -np.inf, np.float32)
    np.minimum.at(lo, c, z)
    np.maximum.at(hi, c, z)
    return int(np.count_nonzero(np.bincount(c, minlength=gp.width * gp.height))), lo, hi


def export_grid(args, pipe, res):
    """--grid: the grid from the device, its file and picture, the timings"""
    from draw_map import write_png
    smap, ctx = pipe.map, pipe.ctx
    times = []
    for _ in range(max(1, args.repeat)):
        t = time.perf_counter()
        cells, gp, gst = smap.export_grid(cell_size=args.grid_cell, min_confidence=args.min_confidence, fit_margin=1)
        times.append(time.perf_counter() - t)
    mapio.write_grid(args.grid, cells, gp)
    res.update(grid=args.grid, grid_stats=gst, grid_size=[gp.width, gp.height], grid_cell=args.grid_cell,
               grid_export_wall_ms=[round(1e3 * x, 3) for x in times])
    if args.grid_png:
        write_png(args.grid_png, GRID_STATE_RGBA[cells["state"][::-1]])  # row 0 of the picture is the greatest y
    if args.compare:
        world = smap.export_world(min_confidence=args.min_confidence)
        d = ctx.device_array(world)
        try:
            wall = []
            for rep in range(3):  # the last run with the ctx's kernel timers on
                ctx.profile(rep == 2)
                ctx.profile_reset()
                t = time.perf_counter()
                core.world_grid(ctx, d, len(world), cell_size=args.grid_cell, fit_margin=1)
                wall.append(round(1e3 * (time.perf_counter() - t), 3))
            res["grid_kernels_us"] = {k["name"]: round(1e3 * k["total_ms"], 1) for k in ctx.profile_get()
                                      if k["name"].startswith("grid_")}
            ctx.profile(0)
        finally:
            ctx.device_free(d)
        res["grid_device_call_wall_ms"] = wall  # fit + grid + the cells' download, from records on the device
        t = time.perf_counter()
        world = smap.export_world(min_confidence=args.min_confidence)
        occupied = numpy_grid_route(world, gp)[0]
        res["grid_numpy_route_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
        res["grid_numpy_route_occupied"] = occupied
        t = time.perf_counter()
        vox, vst = smap.export_world(voxel_size=args.grid_cell, min_confidence=args.min_confidence, stats=True)
        res["voxel_export_same_cell_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
        res["voxel_export_same_cell_out"] = vst["n_out"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="map.ply")
    ap.add_argument("--scans", type=int, default=40)
    ap.add_argument("--kitti", default=None, help="a sequences/XX directory")
    ap.add_argument("--width", type=int, default=2048, help="data image width (64 rows)")
    ap.add_argument("--voxel", type=float, default=0.0, help="voxel size in metres; 0: one record per surfel")
    ap.add_argument("--min-confidence", type=float, default=None)
    ap.add_argument("--close-loops", action="store_true")
    ap.add_argument("--repeat", type=int, default=3, help="timed exports (the first one allocates the scratch)")
    ap.add_argument("--compare", action="store_true", help="also time the host route")
    ap.add_argument("--places", default=None, help="write a place index of every scan with the final trajectory (.npz)")
    ap.add_argument("--place-range", type=float, default=80.0, help="max_range of the place descriptor in metres")
    ap.add_argument("--grid", default=None, help="also write the traversability grid (.npz, mapio.write_grid)")
    ap.add_argument("--grid-cell", type=float, default=0.2, help="cell size of the grid in metres")
    ap.add_argument("--grid-png", default=None, help="a picture of the grid's cell states")
    args = ap.parse_args()
    p = params_with_size(args.width, 64)
    pipe = core.SurfelMapping(p, loop_params=LoopParams.defaults() if args.close_loops else None)
    index = core.PlaceIndex(PlaceParams.defaults(max_range=args.place_range), capacity=args.scans) if args.places else None
    for k, (pts, lab, prob) in enumerate(scans(args)):
        pipe.processScan(pts, lab, prob)
        if index is not None:
            index.addFrame(pipe.ctx, pipe.frame(0), k)
    smap = pipe.map
    times = []
    for _ in range(max(1, args.repeat)):
        t = time.perf_counter()
        world, st = smap.export_world(voxel_size=args.voxel, min_confidence=args.min_confidence, stats=True)
        times.append(time.perf_counter() - t)
    mapio.write_ply(args.out, world)
    res = dict(stats=st, voxel_size=args.voxel, export_wall_ms=[round(1e3 * x, 3) for x in times], out=args.out,
               bytes=os.path.getsize(args.out))
    if index is not None:
        places.save(args.places, index, np.asarray(smap.poses(), dtype=np.float64)[:index.size()])
        res.update(places=args.places, place_entries=index.size())
    if args.compare:
        t = time.perf_counter()
        pts = host_route(smap, p.max_poses)
        res["host_route_wall_ms"] = round(1e3 * (time.perf_counter() - t), 3)
        res["host_route_points"] = int(pts.shape[0])
    if args.grid:
        export_grid(args, pipe, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
