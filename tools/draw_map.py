#!/usr/bin/env python
"""Pictures of the map while it is built: runs a synthetic sequence (semantic_suma_amd/synth.py) or a KITTI directory
(velodyne/*.bin, optionally labels/*.label) through SurfelMapping and, every k scans, writes two PNGs drawn on the GPU
by SurfelMap.draw (csrc/k_draw.hip): a bird's-eye semantic view over the trajectory and a chase camera behind the sensor.
PNG is written with the standard library (zlib + struct).  Needs a GPU.
    python tools/draw_map.py --out pics [--scans 40] [--every 10] [--kitti sequences/08] [--mode 5] [--size 1280x720]
"""
import argparse
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from semantic_suma_amd import core, kitti, synth  # noqa: E402
from semantic_suma_amd.types import params_with_size  # noqa: E402


def write_png(path, rgba):
    """uint8 [H, W, 4], row 0 at the top"""
    h, w, _ = rgba.shape
    raw = b"".join(b"\x00" + np.ascontiguousarray(rgba[y]).tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def chase(pose, W, H):
    eye = (pose @ np.array([-15.0, 0.0, 8.0, 1.0]))[:3]
    target = (pose @ np.array([10.0, 0.0, 0.0, 1.0]))[:3]
    V = core.look_at(core.ROSE2GL[:3, :3] @ eye, core.ROSE2GL[:3, :3] @ target, [0.0, 1.0, 0.0])
    return core.perspective(45.0, W / H, 0.1, 10000.0) @ V @ core.ROSE2GL, eye


def birdseye(traj, W, H):
    c = traj[:, :3, 3].mean(0)
    span = np.ptp(traj[:, :2, 3], axis=0).max() / 2 + 40.0
    eye = c + np.array([0.0, 0.0, 200.0])
    V = core.look_at(core.ROSE2GL[:3, :3] @ eye, core.ROSE2GL[:3, :3] @ c, core.ROSE2GL[:3, :3] @ np.array([1.0, 0.0, 0.0]))
    a = W / H
    return core.orthographic(-span * a, span * a, -span, span, 0.1, 1000.0) @ V @ core.ROSE2GL, eye


def scans(args):
    if args.kitti:
        bins = sorted(f for f in os.listdir(os.path.join(args.kitti, "velodyne")) if f.endswith(".bin"))[:args.scans]
        for b in bins:
            pts = kitti.read_velodyne(os.path.join(args.kitti, "velodyne", b))
            lp = os.path.join(args.kitti, "labels", b[:-4] + ".label")
            if os.path.exists(lp):
                lab, prob = kitti.read_labels(lp, pts.shape[0])
            else:
                lab = prob = None
            yield pts, lab, prob
    else:
        for k in range(args.scans):
            pts, lab, prob, _ = synth.generate_scan(k, n_azimuth=args.width, height=64)
            yield pts, lab, prob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="draw_map_out")
    ap.add_argument("--scans", type=int, default=40)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--kitti", default=None, help="a sequences/XX directory")
    ap.add_argument("--width", type=int, default=2048, help="data image width (64 rows)")
    ap.add_argument("--mode", type=int, default=5, help="colour mode of the chase view (0..5)")
    ap.add_argument("--size", default="1280x720")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    os.makedirs(args.out, exist_ok=True)
    pipe = core.SurfelMapping(params_with_size(args.width, 64))
    traj = []
    for k, (pts, lab, prob) in enumerate(scans(args)):
        pipe.processScan(pts, lab, prob)
        traj.append(pipe.getCurrentPose().copy())
        if (k + 1) % args.every == 0:
            t = np.array(traj)
            mvp, eye = birdseye(t, W, H)
            write_png(os.path.join(args.out, f"birdseye_{k + 1:05d}.png"), pipe.map.draw(mvp, W, H, eye, color_mode=5))
            mvp, eye = chase(t[-1], W, H)
            write_png(os.path.join(args.out, f"chase_{k + 1:05d}.png"), pipe.map.draw(mvp, W, H, eye, color_mode=args.mode))
            print(f"scan {k + 1}: {pipe.map.size()} surfels -> {args.out}", flush=True)


if __name__ == "__main__":
    main()
