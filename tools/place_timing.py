#!/usr/bin/env python3
"""Measures what DESIGN.md section 13 reports about the place index and writes profiles/place_timing.json.  Needs a GPU.

    python tools/place_timing.py [--out profiles/place_timing.json] [--entries 1000 4541 20000]

One 64 x 2048 frame (synth.generate_scan(0), K1-K3), the default descriptor (20 rings x 60 sectors):

  add_frame     the library's own HIP events (suma_profile_enable) around the launches of one suma_place_index_add_frame
                -- the memset of the entry, kp_describe, kp_norms -- after suma_profile_reset; one untimed call, then the
                median of 10.
  query_frame   per database size: the same events around kp_search alone ("place_search"), around kp_topk alone
                ("place_topk", k = 8) and around the query's own descriptor ("place_describe"); one untimed call, then
                the median of 10.  The databases are random crafted entries (30 % empty cells, 20 % empty columns).
  copy          hipMemcpyAsync device to device of the database's bytes (entries x 1260 floats) between two blocks of
                suma_device_alloc, HIP events (torch.cuda.Event on the current stream) around each copy; 3 untimed, then
                the median of 10.  ratio = place_search / copy: the search reads the database once.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402 -- before the library: torch and libsuma_hip.so must share one HIP runtime

from semantic_suma_amd import core, synth  # noqa: E402
from semantic_suma_amd.types import PlaceParams, params_with_size  # noqa: E402

SCAN_STEP_US = 313.0  # one scan of the flagship pipeline


def profiled(ctx, call, names):
    """one call between suma_profile_reset and suma_profile_get -> {name: ms}"""
    ctx.profile_reset()
    call()
    ctx.synchronize()
    rec = {r["name"]: r["total_ms"] for r in ctx.profile_get()}
    return {n: rec[n] for n in names}


def d2d_copy_ms(ctx, nbytes):
    L = ctx.L
    src, dst = C.c_void_p(), C.c_void_p()
    ctx.check(L.suma_device_alloc(ctx.h, nbytes, C.byref(src)), "suma_device_alloc")
    ctx.check(L.suma_device_alloc(ctx.h, nbytes, C.byref(dst)), "suma_device_alloc")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for k in range(13):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = hip.hipMemcpyAsync(dst, src, nbytes, 3, stream)  # 3 = hipMemcpyDeviceToDevice
        b.record()
        b.synchronize()
        assert rc == 0, rc
        if k >= 3:
            out.append(a.elapsed_time(b))
    ctx.device_free(src.value)
    ctx.device_free(dst.value)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_timing.json"))
    ap.add_argument("--entries", type=int, nargs="+", default=[1000, 4541, 20000])
    args = ap.parse_args()
    p = params_with_size(2048, 64)
    ctx = core.Context(p)
    frame = core.Frame(ctx, 2048, 64)
    pts, lab, prob, _ = synth.generate_scan(0, n_azimuth=2048, height=64)
    core.Preprocessing(ctx).process(pts, frame, lab, prob, 20)
    ctx.synchronize()
    pp = PlaceParams.defaults()
    S, R = pp.sectors, pp.rings
    ctx.profile(1)

    idx = core.PlaceIndex(pp, capacity=16)
    idx.addFrame(ctx, frame, 0)
    add_ms = [profiled(ctx, lambda: idx.addFrame(ctx, frame, 1), ["place_describe"])["place_describe"] for _ in range(10)]
    idx.close()
    out = dict(frame="64 x 2048", rings=R, sectors=S, entry_bytes=4 * (S * R + S),
               add_frame_us_hip_events_median10=1e3 * statistics.median(add_ms), scan_step_us=SCAN_STEP_US,
               samples=dict(add_frame_ms=add_ms), query=[])
    out["add_frame_over_scan_step"] = out["add_frame_us_hip_events_median10"] / SCAN_STEP_US

    rng = np.random.RandomState(3)
    for n in args.entries:
        cells = rng.uniform(0.05, 30.0, (n, S, R)).astype(np.float32)
        cells[rng.uniform(size=(n, S, R)) < 0.3] = 0.0
        cells[rng.uniform(size=(n, S)) < 0.2] = 0.0
        idx = core.PlaceIndex(pp, capacity=n)
        idx.upload(cells, np.arange(n, dtype=np.uint32))
        names = ["place_describe", "place_search", "place_topk"]
        idx.queryFrame(ctx, frame, 8)
        runs = [profiled(ctx, lambda: idx.queryFrame(ctx, frame, 8), names) for _ in range(10)]
        nbytes = n * 4 * (S * R + S)
        copy = d2d_copy_ms(ctx, nbytes)
        med = {k: statistics.median(r[k] for r in runs) for k in names}
        c = statistics.median(copy)
        total = sum(med.values())
        out["query"].append(dict(entries=n, database_bytes=nbytes, describe_us=1e3 * med["place_describe"],
                                 search_us=1e3 * med["place_search"], topk_us=1e3 * med["place_topk"],
                                 query_device_us=1e3 * total, d2d_copy_us=1e3 * c, search_over_copy=med["place_search"] / c,
                                 query_over_scan_step=1e3 * total / SCAN_STEP_US,
                                 samples=dict(query_ms=runs, d2d_copy_ms=copy)))
        idx.close()
    ctx.profile(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    slim = {k: v for k, v in out.items() if k != "samples"}
    slim["query"] = [{k: v for k, v in q.items() if k != "samples"} for q in out["query"]]
    print(json.dumps(slim))


if __name__ == "__main__":
    main()
