#!/usr/bin/env python3
"""Measures what DESIGN.md section 11 reports about a pipeline checkpoint and writes profiles/checkpoint_timing.json.
Needs a GPU.

    python tools/checkpoint_timing.py [--out profiles/checkpoint_timing.json] [--bench-scans 300]

Two maps: (a) the benchmark's sequence (synth.generate_scan, 2048 x 64, default parameters, 10 fixed iterations) after
--bench-scans scans, the map bench.py's timed steps start from; (b) the circle scenario of tests/test_gpu_checkpoint.py (360 x 32,
submap_extent 4, submap_dimension 2) after 70 scans.  Per map:

  save / load   host clock (perf_counter) around suma_pipeline_checkpoint_save / _load alone, into / from a numpy buffer
                that exists before the clock starts; one untimed call first (it grows the staging block), then the
                median of 5.  Both calls are blocking, so the clock sees the whole of the work, the copy of the image
                between host memory and HBM included.
  kc_pack       the library's own HIP events (suma_profile_enable) around the launches of one save, after
                suma_profile_reset: 4 launches, their time summed; median of 5 saves.
  copy          hipMemcpyAsync device to device of as many bytes as kc_pack moved (the four device-resident sections),
                between two blocks of suma_device_alloc, HIP events (torch.cuda.Event on the current stream) around each
                copy; 3 untimed, then the median of 10.  ratio = kc_pack / copy.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402 -- before the library: torch and libsuma_hip.so must share one HIP runtime

from semantic_suma_amd import checkpoint as ck  # noqa: E402
from semantic_suma_amd import core, synth  # noqa: E402
from semantic_suma_amd.types import params_with_size  # noqa: E402

DEVICE_SECTIONS = ("POSES", "ACTIVE", "FRAME", "TILES")


def measure(name, pipe):
    L, h = pipe.L, pipe.h
    n = C.c_uint64()
    pipe.ctx.check(L.suma_pipeline_checkpoint_size(h, C.byref(n)), "size")
    buf = np.empty(n.value, dtype=np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)

    def save():
        t = time.perf_counter()
        rc = L.suma_pipeline_checkpoint_save(h, ptr, n.value, C.byref(n))
        dt = time.perf_counter() - t
        pipe.ctx.check(rc, "save")
        return 1e3 * dt

    save()
    save_ms = [save() for _ in range(5)]
    img = buf.tobytes()
    secs = ck.read(img)
    info = core.checkpoint_info(img)
    pipe.ctx.profile(1)
    pack_ms, launches = [], 0
    for _ in range(5):
        pipe.ctx.profile_reset()
        save()
        rec = [r for r in pipe.ctx.profile_get() if r["name"] == "kc_pack"]
        assert len(rec) == 1, "the profile has no kc_pack record"
        pack_ms.append(rec[0]["total_ms"])
        launches = rec[0]["launches"]
    pipe.ctx.profile(0)
    assert buf.tobytes() == img, "two saves of one state differ"

    def load():
        t = time.perf_counter()
        rc = L.suma_pipeline_checkpoint_load(h, img, len(img))
        dt = time.perf_counter() - t
        pipe.ctx.check(rc, "load")
        return 1e3 * dt

    load()
    load_ms = [load() for _ in range(5)]

    nbytes = sum(len(secs[s]["data"]) for s in DEVICE_SECTIONS)
    src, dst = C.c_void_p(), C.c_void_p()
    pipe.ctx.check(L.suma_device_alloc(pipe.ctx.h, nbytes, C.byref(src)), "suma_device_alloc")
    pipe.ctx.check(L.suma_device_alloc(pipe.ctx.h, nbytes, C.byref(dst)), "suma_device_alloc")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    copy_ms = []
    for k in range(13):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = hip.hipMemcpyAsync(dst, src, nbytes, 3, stream)  # 3 = hipMemcpyDeviceToDevice
        b.record()
        b.synchronize()
        assert rc == 0, rc
        if k >= 3:
            copy_ms.append(a.elapsed_time(b))
    pipe.ctx.device_free(src.value)
    pipe.ctx.device_free(dst.value)
    pack, copy = statistics.median(pack_ms), statistics.median(copy_ms)
    return dict(name=name, image_bytes=len(img), n_active=info["n_active"], n_parked=info["n_parked"],
                n_tiles=info["n_tiles"], timestamp=info["timestamp"], save_ms_host_clock_median5=statistics.median(save_ms),
                load_ms_host_clock_median5=statistics.median(load_ms), kc_pack_launches=launches,
                kc_pack_ms_hip_events_median5=pack, device_section_bytes=nbytes,
                d2d_copy_ms_hip_events_median10=copy, kc_pack_over_copy=pack / copy,
                samples=dict(save_ms=save_ms, load_ms=load_ms, kc_pack_ms=pack_ms, d2d_copy_ms=copy_ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_timing.json"))
    ap.add_argument("--bench-scans", type=int, default=300)
    args = ap.parse_args()
    import loop_scenario as ls
    out = []
    pipe = core.SurfelMapping(params_with_size(2048, 64))
    for k in range(args.bench_scans):
        pipe.processScan(*synth.generate_scan(k, n_azimuth=2048, height=64)[:3], fixed_iterations=10)
    out.append(measure(f"bench sequence, 2048 x 64, after {args.bench_scans} scans", pipe))
    pipe.close()
    pipe = core.SurfelMapping(params_with_size(360, 32, submap_extent=4.0, submap_dimension=2))
    for k in range(70):
        pipe.processScan(*ls.scan(k, 360, 32), fixed_iterations=6)
    out.append(measure("circle scenario, 360 x 32, after 70 scans", pipe))
    pipe.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for r in out:
        print(json.dumps({k: v for k, v in r.items() if k != "samples"}))


if __name__ == "__main__":
    main()
