#!/usr/bin/env python3
"""Measures what DESIGN.md section 16 reports about the motion compensation and writes profiles/deskew_timing.json.
Needs a GPU.

    python tools/deskew_timing.py [--out profiles/deskew_timing.json] [--scans 60]

  kd_deskew     131 072 points (64 x 2048), a general motion, azimuth time, out of place: the library's own HIP events
                (suma_profile_enable) around the launch of one suma_deskew_points_device after suma_profile_reset; 3
                untimed calls, then the median of 10.  The same with the `times` source.
  copy          hipMemcpyAsync device to device of the same 2 MiB of points (2 MiB read + 2 MiB written, as the kernel),
                HIP events around each copy; 3 untimed, then the median of 10.
  processScan   the blocking host-vector entry over the first --scans scans of the synthetic sequence at 64 x 2048,
                wall clock from the first call to a final synchronisation, correction off and on, twice each in turn
                (the scans are the generator's instantaneous ones: the rate does not depend on what the points hold).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402 -- before the library: torch and libsuma_hip.so must share one HIP runtime

from semantic_suma_amd import core, synth  # noqa: E402
from semantic_suma_amd.types import DESKEW_TIME_TIMES, DeskewParams, params_with_size  # noqa: E402

N = 64 * 2048


def kernel_ms(ctx, d_in, d_out, d_times, motion, dp):
    out = []
    for k in range(13):
        ctx.profile_reset()
        core.deskew_points_device(ctx, d_in, motion, N, d_out, dp, d_times)
        ctx.synchronize()
        rec = {r["name"]: r["total_ms"] for r in ctx.profile_get()}
        if k >= 3:
            out.append(rec["kd_deskew"])
    return out


def d2d_copy_ms(d_in, d_out, nbytes):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for k in range(13):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = hip.hipMemcpyAsync(C.c_void_p(d_out.data_ptr()), C.c_void_p(d_in.data_ptr()), nbytes, 3, stream)  # 3 = device to device
        b.record()
        b.synchronize()
        assert rc == 0, rc
        if k >= 3:
            out.append(a.elapsed_time(b))
    return out


def scan_rate(p, scans, deskew):
    pipe = core.SurfelMapping(p)
    if deskew:
        pipe.enableDeskew()
    pipe.processScan(*scans[0])  # the first scan allocates and has no pose update
    pipe.ctx.synchronize()
    t = time.perf_counter()
    for s in scans[1:]:
        pipe.processScan(*s)
    pipe.ctx.synchronize()
    dt = time.perf_counter() - t
    pipe.close()
    return (len(scans) - 1) / dt


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew_timing.json"))
    ap.add_argument("--scans", type=int, default=60)
    args = ap.parse_args()
    p = params_with_size(2048, 64)
    ctx = core.Context(p)
    rng = np.random.default_rng(5)
    az, r = rng.uniform(-np.pi, np.pi, N), rng.uniform(2.0, 80.0, N)
    pts = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.0, 3.0, N), np.ones(N)], 1).astype(np.float32)
    d_in, d_out = torch.from_numpy(pts).cuda(), torch.zeros((N, 4), dtype=torch.float32).cuda()
    d_times = torch.from_numpy(rng.uniform(0.0, 1.0, N).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    a = 0.07
    motion = np.eye(4)
    motion[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    motion[:3, 3] = [1.1, 0.04, -0.01]
    ctx.profile(1)
    k_az = kernel_ms(ctx, d_in, d_out, None, motion, DeskewParams.defaults())
    k_tm = kernel_ms(ctx, d_in, d_out, d_times, motion, DeskewParams.defaults(time_source=DESKEW_TIME_TIMES))
    ctx.profile(0)
    copy = d2d_copy_ms(d_in, d_out, pts.nbytes)
    out = dict(points=N, bytes_read_and_written=2 * pts.nbytes,
               kd_deskew_azimuth_us_median10=1e3 * statistics.median(k_az),
               kd_deskew_times_us_median10=1e3 * statistics.median(k_tm),
               d2d_copy_us_median10=1e3 * statistics.median(copy),
               samples=dict(kd_deskew_azimuth_ms=k_az, kd_deskew_times_ms=k_tm, d2d_copy_ms=copy))
    out["azimuth_over_copy"] = out["kd_deskew_azimuth_us_median10"] / out["d2d_copy_us_median10"]
    scans = [synth.generate_scan(k, n_azimuth=2048, height=64)[:3] for k in range(args.scans)]
    rates = dict(off=[], on=[])
    for _ in range(2):
        for name in ("off", "on"):
            rates[name].append(scan_rate(p, scans, name == "on"))
    out["process_scan"] = dict(scans=args.scans, size="64 x 2048", scans_per_s_off=rates["off"], scans_per_s_on=rates["on"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "samples"}))


if __name__ == "__main__":
    main()
