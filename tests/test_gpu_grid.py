"""suma_world_grid / suma_world_grid_fit on the MI355X (csrc/k_grid.hip, core.world_grid, SurfelMap.export_grid): cells and
stats byte for byte against the host restatement (tests/grid_shim.c) -- sizes around every boundary, rasters from one cell
up, fill radii, run extremes, cell edges, non-finite fields, ties, thresholds, the fit, validation, determinism, no side
effects, and a real pipeline's map."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import grid_common as gc
import loop_scenario as ls
from semantic_suma_amd import core
from semantic_suma_amd.types import (GRID_CELL_DTYPE, GRID_FREE, GRID_NO_GROUND, GRID_OBSTACLE, GRID_UNKNOWN, GridParams,
                                     GridStats, params_with_size)

pytestmark = pytest.mark.gpu
one = gc.one


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return gc.build_shim(tmp_path_factory.mktemp("grid_gpu"))


@pytest.fixture(scope="module")
def ctx():
    return core.Context(params_with_size(900, 64))


def check(shim, ctx, rec, gp, where=""):
    """the grid of the device equals the shim's on (rec, gp): cells and every stat; returns (cells, stats)"""
    got, gp2, st = core.world_grid(ctx, rec, params=gp)
    want, wst = gc.shim_grid(shim, rec, gp)
    assert bytes(gp2) == bytes(gp)
    assert st == wst, (where, st, wst)
    assert got.dtype == GRID_CELL_DTYPE and got.shape == (gp.height, gp.width)
    if got.tobytes() != want.tobytes():
        bad = [f for f in GRID_CELL_DTYPE.names if got[f].tobytes() != want[f].tobytes()]
        raise AssertionError((where, bad, int((got.view(np.uint8) != want.view(np.uint8)).sum())))
    return got, st


RASTERS = {"1x1": gc.params(1, 1, 32.0, origin=(-8.0, -16.0)),            # every record in the one cell
           "1x70": gc.params(1, 70, 0.25, origin=(3.0, -1.5)),            # most records outside
           "65x3": gc.params(65, 3, 0.25, origin=(-1.5, 2.0)),
           "257x129": gc.params(257, 129, 0.0703125, origin=(-1.03, -1.01))}


@pytest.mark.parametrize("raster", list(RASTERS))
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_sizes_and_rasters(shim, ctx, n, raster):
    got, st = check(shim, ctx, gc.scene(n), RASTERS[raster], raster)
    assert st["n_records"] == n == st["n_dropped"] + st["n_outside"] + st["n_binned"]
    assert int(got["support"].sum()) == st["n_binned"] and (n < 1023 or st["n_binned"] > 0)
    if raster == "1x1":
        assert st["n_binned"] == n
    if raster == "1x70" and n >= 1023:
        assert st["n_outside"] > n // 2


@pytest.mark.parametrize("fill", [0, 1, 3, 8])
def test_fill_radius(shim, ctx, fill):
    got, st = check(shim, ctx, gc.scene(600), gc.params(80, 50, 0.25, origin=(-2.0, -2.0), fill_radius=fill), fill)
    assert (fill == 0) == (st["n_filled"] == 0)
    assert st["n_free"] > 0 and st["n_obstacle"] > 0 and (fill > 1 or st["n_no_ground"] > 0)
    assert np.any((got["state"] == GRID_UNKNOWN) & (got["ground_source"] == 2)) == (fill > 0)


def test_run_extremes(shim, ctx):
    rec = gc.scene(3000)
    rec["x"], rec["y"] = 0.01 * np.arange(3000), 2.0                         # one cell holds all 3000
    got, st = check(shim, ctx, rec, gc.params(3, 3, 100.0, origin=(-100.0, -100.0)), "one cell")
    assert st["n_occupied"] == 1 and got[1, 1]["support"] == 3000
    rec["x"], rec["y"] = 0.5 * np.arange(3000) + 0.25, 0.25                  # every record in a cell of its own
    got, st = check(shim, ctx, rec, gc.params(3000, 1, 0.5), "own cells")
    assert st["n_occupied"] == 3000 and np.all(got["support"] == 1)


def test_cell_edges_and_a_negative_origin(shim, ctx):
    gp = gc.params(6, 4, 0.25, origin=(-1.0, -0.5))
    k = np.arange(-1, 8)
    xs, ys = np.meshgrid(gp.origin_x + k * 0.25, gp.origin_y + k * 0.25)      # on every edge, the far one (fx == width) too
    rec = np.concatenate([one(x, y, -1.75) for x, y in zip(xs.ravel(), ys.ravel())])
    got, st = check(shim, ctx, rec, gp)
    assert st["n_binned"] == 6 * 4 and st["n_outside"] == len(rec) - 24 and np.all(got["support"] == 1)
    rec["x"] += np.float32(-1e-6)                                            # just below the edges: one column fewer
    got, st = check(shim, ctx, rec, gp)
    assert np.array_equal(gc.cell_of(rec, gp) >= 0, (rec["x"] >= -1.0) & (rec["x"] < 0.5) & (rec["y"] >= -0.5) & (rec["y"] < 0.5))


@pytest.mark.parametrize("field", ["x", "y", "z", "nz", "prob", "confidence", "label"])
def test_edge_values_in_every_field(shim, ctx, field):
    rec = gc.scene(400)
    gp = gc.params(30, 18, 0.75, origin=(-2.0, -2.0))
    if field == "label":
        rec["label"][5:400:7] = [260, 300, 0xffffffff] * 19                 # >= 260 reads as 0
    else:
        rec[field][5:400:7] = [np.nan, np.inf, -np.inf] * 19
    _, st = check(shim, ctx, rec, gp, field)
    assert st["n_dropped"] == (57 if field in "xyz" else 0)
    # a cell whose every member carries the value
    cell = np.concatenate([one(0.1, 0.1, -1.75), one(0.2, 0.1, -1.5), one(0.3, 0.2, 0.0, label=10)])
    for v in ([260, 300, 0xffffffff] if field == "label" else [np.nan, np.inf, -np.inf]):
        cell[field] = v
        check(shim, ctx, cell, gc.params(2, 2, 1.0), (field, v))


def test_ties_and_membership(shim, ctx):
    gp = gc.params(1, 1, 1.0)
    rec = np.concatenate([
        one(0.5, 0.5, 1.0, conf=np.nan), one(0.5, 0.5, 2.0, conf=3.0), one(0.5, 0.5, 3.0, conf=3.0),
        one(0.5, 0.5, 4.0, conf=9.0, label=10), one(0.5, 0.5, 5.0, conf=9.0, nz=0.69), one(0.5, 0.5, 6.0, conf=9.0, nz=np.nan),
        one(0.5, 0.5, 0.5, conf=-np.inf, nz=-0.7)])
    got, _ = check(shim, ctx, rec, gp)
    assert (got[0, 0]["n_ground"], got[0, 0]["ground_z"], got[0, 0]["ground_rough"]) == (4, 2.0, 2.5)
    got, _ = check(shim, ctx, rec[::-1].copy(), gp)                          # the other order: the tie goes the other way
    assert got[0, 0]["ground_z"] == 3.0
    got, _ = check(shim, ctx, rec[[0, 3]], gp)
    assert got[0, 0]["ground_z"] == 1.0
    v = np.concatenate([one(0.5, 0.5, 0.0, label=48, prob=0.5), one(0.5, 0.5, 0.0, label=40, prob=0.5)])
    got, _ = check(shim, ctx, v, gp)                                         # equal vote sums: the smaller id
    assert (got[0, 0]["label"], got[0, 0]["prob"]) == (40, 0.5)
    v["prob"], v["confidence"] = 0.0, [5.0, 1.0]
    got, _ = check(shim, ctx, v, gp)                                         # no weight: the most confident member's label
    assert (got[0, 0]["label"], got[0, 0]["prob"]) == (48, 0.0)
    v["confidence"] = 5.0
    got, _ = check(shim, ctx, v, gp)                                         # equal confidences: the smaller source index
    assert got[0, 0]["label"] == 48
    z = np.concatenate([one(0.5, 0.5, 0.0, label=72), one(0.5, 0.5, -0.0), one(0.5, 0.5, 0.0)])
    got, _ = check(shim, ctx, z, gp)                                         # -0 below +0 whatever the members' order
    assert np.signbit(got[0, 0]["z_min"]) and not np.signbit(got[0, 0]["z_max"])


def test_fill_ties_and_borders(shim, ctx):
    heights = {(2, 1): 1.0, (1, 2): 2.0, (3, 2): 3.0, (2, 3): 4.0}           # the four neighbours of the centre
    rec = np.concatenate([one(ix + 0.5, iy + 0.5, z) for (ix, iy), z in heights.items()] + [one(2.5, 2.5, 2.5, label=10)])
    got, st = check(shim, ctx, rec, gc.params(5, 5, 1.0, fill_radius=1))
    assert (got[2, 2]["ground_z"], got[2, 2]["ground_source"], got[2, 2]["state"]) == (1.0, 2, GRID_OBSTACLE)
    assert got[1, 1]["ground_z"] == 1.0 and got[3, 3]["ground_z"] == 3.0 and st["n_filled"] == 17
    got, _ = check(shim, ctx, rec[1:], gc.params(5, 5, 1.0, fill_radius=1))
    assert got[2, 2]["ground_z"] == 2.0
    got, st = check(shim, ctx, rec, gc.params(5, 5, 1.0, fill_radius=8))     # the window clipped at every border
    assert st["n_filled"] == 21 and got[0, 0]["ground_z"] == 1.0 and got[4, 4]["ground_z"] == 3.0
    got, st = check(shim, ctx, rec, gc.params(5, 5, 1.0, fill_radius=0))
    assert st["n_filled"] == 0 and got[2, 2]["state"] == GRID_NO_GROUND
    rec = np.concatenate([one(0.5, 0.5, 1.0), one(3.5, 2.5, 2.0)])
    got, _ = check(shim, ctx, rec, gc.params(5, 5, 1.0, fill_radius=2))
    assert got[2, 2]["ground_z"] == 2.0 and got[1, 1]["ground_z"] == 1.0 and got[4, 0]["ground_source"] == 0


def test_thresholds_are_strict(shim, ctx):
    gp = gc.params(1, 1, 1.0, step_height=0.25, clearance=2.0)
    rec = np.concatenate([one(0.5, 0.5, -1.75), one(0.5, 0.5, -1.5, label=10), one(0.5, 0.5, 0.25, label=10),
                          one(0.5, 0.5, 0.5, label=10)])                       # h = 0.25, 2.0, 2.25
    got, _ = check(shim, ctx, rec, gp)
    c = got[0, 0]
    assert (c["n_obstacle"], c["n_overhang"], c["obstacle_z"], c["state"]) == (1, 1, 0.25, GRID_OBSTACLE)
    got, _ = check(shim, ctx, rec[[0, 1, 3]], gp)
    assert (got[0, 0]["n_obstacle"], got[0, 0]["n_overhang"], got[0, 0]["state"]) == (0, 1, GRID_FREE)
    got, _ = check(shim, ctx, rec[1:], gp)
    assert got[0, 0]["state"] == GRID_NO_GROUND


def fit(ctx, d_rec, n, cell_size, margin):
    gp = GridParams.defaults(cell_size=cell_size)
    rc = ctx.L.suma_world_grid_fit(ctx.h, C.c_void_p(d_rec) if d_rec else None, n, margin, C.byref(gp))
    return rc, gp


def test_fit_against_numpy(shim, ctx):
    rec = gc.scene(5000, lo=(-37.3, 2.2), hi=(11.9, 40.1))
    rec["x"][::9], rec["y"][1::9], rec["z"][2::9] = np.nan, np.inf, -np.inf
    rec["x"][2::9] = 1e6                                                     # a non-finite z: its x does not count
    d = ctx.device_array(rec)
    try:
        for n, cs, margin in ((5000, 0.2, 0), (5000, 0.2, 1), (5000, 0.75, 3), (1025, 0.1, 2), (4, 0.2, 0)):
            rc, gp = fit(ctx, d, n, cs, margin)
            assert rc == 0 and (gp.origin_x, gp.origin_y, gp.width, gp.height) == gc.fit_of(rec[:n], cs, margin), (n, cs, margin)
            check(shim, ctx, rec[:n], gp, ("fitted", n, cs, margin))
        cells, gp2, st = core.world_grid(ctx, rec, cell_size=0.2, fit_margin=1)  # a margin of one cell holds every record
        finite = np.isfinite(rec["x"]) & np.isfinite(rec["y"]) & np.isfinite(rec["z"])
        assert st["n_outside"] == 0 and st["n_dropped"] == int((~finite).sum()) > 1000 and cells.shape == (gp2.height, gp2.width)
        # a single record
        rc, gp = fit(ctx, d + 48 * 4, 1, 0.25, 0)
        assert rc == 0 and (gp.width, gp.height) == (1, 1) and (gp.origin_x, gp.origin_y, 1, 1) == gc.fit_of(rec[4:5], 0.25, 0)
        # no finite record: invalid; the parameters stay
        bad = rec[:64].copy()
        bad["z"] = np.nan
        d_bad = ctx.device_array(bad)
        try:
            for n in (64, 0):
                rc, gp = fit(ctx, d_bad, n, 0.2, 1)
                assert rc == -1 and "no finite record" in ctx.L.suma_last_error(ctx.h).decode()
                assert bytes(gp) == bytes(GridParams.defaults(cell_size=0.2))
        finally:
            ctx.device_free(d_bad)
        # more cells than the limit: capacity; the parameters stay
        for cs in (1e-3, 1e-30):
            rc, gp = fit(ctx, d, 5000, cs, 1)
            assert rc == -3 and "2^26" in ctx.L.suma_last_error(ctx.h).decode()
            assert bytes(gp) == bytes(GridParams.defaults(cell_size=cs))
        for cs in (0.0, -1.0, float("nan"), float("inf")):
            rc, gp = fit(ctx, d, 5000, cs, 1)
            assert rc == -1 and "cell_size" in ctx.L.suma_last_error(ctx.h).decode()
    finally:
        ctx.device_free(d)


SENTINEL = 0x7fc00001
BAD = [("cell_size", 0.0, "cell_size"), ("cell_size", -1.0, "cell_size"), ("cell_size", float("nan"), "cell_size"),
       ("cell_size", float("inf"), "cell_size"), ("origin_x", float("nan"), "origin"), ("origin_y", float("inf"), "origin"),
       ("width", 0, "width"), ("height", 0, "width"), ("width", 1 << 25, "width"), ("min_normal_z", float("nan"), "min_normal_z"),
       ("step_height", float("nan"), "step_height"), ("step_height", float("inf"), "step_height"),
       ("clearance", 0.2, "clearance"), ("clearance", float("inf"), "clearance"), ("clearance", float("nan"), "clearance"),
       ("fill_radius", 9, "fill_radius"),
       ("gp", None, "parameters"), ("stats", None, "stats"), ("cells", None, "cells"), ("records", None, "records"),
       ("n", 1 << 31, "n ="), ("misaligned", None, "aligned")]


@pytest.mark.parametrize("field,value,needle", BAD)
def test_invalid_calls_launch_nothing(shim, ctx, field, value, needle):
    rec = gc.scene(500)
    gp, st = gc.params(16, 8, 1.0), GridStats()
    records = torch.from_numpy(rec.view(np.int32).copy()).cuda()
    cells = torch.full((16 * 8 * 12,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    a_gp, a_st, a_cells, a_rec, n = C.byref(gp), C.byref(st), C.c_void_p(cells.data_ptr()), C.c_void_p(records.data_ptr()), 500
    if field == "gp":
        a_gp = None
    elif field == "stats":
        a_st = None
    elif field == "cells":
        a_cells = None
    elif field == "records":
        a_rec = None
    elif field == "n":
        n = value
    elif field == "misaligned":
        a_rec = C.c_void_p(records.data_ptr() + 4)
    else:
        setattr(gp, field, value)
    rc = ctx.L.suma_world_grid(ctx.h, a_gp, a_rec, n, a_cells, a_st)
    msg = ctx.L.suma_last_error(ctx.h).decode()
    assert rc == -1 and needle in msg, (rc, msg)
    ctx.synchronize()
    assert bool(torch.all(cells == SENTINEL)), "an invalid call wrote cells"
    assert records.cpu().numpy().tobytes() == rec.tobytes()
    check(shim, ctx, rec, gc.params(16, 8, 1.0))  # a valid call still works


def test_determinism_and_the_record_buffer(shim, ctx):
    rec = gc.scene(5000)
    gp, st1, st2 = RASTERS["257x129"], GridStats(), GridStats()
    records = torch.from_numpy(rec.view(np.int32).copy()).cuda()
    a = torch.full((257 * 129 * 12,), SENTINEL, dtype=torch.int32, device="cuda")
    b = torch.full((257 * 129 * 12,), 0, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(ctx.L.suma_world_grid(ctx.h, C.byref(gp), C.c_void_p(records.data_ptr()), 5000, C.c_void_p(a.data_ptr()), C.byref(st1)))
    ctx.check(ctx.L.suma_world_grid(ctx.h, C.byref(gp), C.c_void_p(records.data_ptr()), 5000, C.c_void_p(b.data_ptr()), C.byref(st2)))
    assert bool(torch.equal(a, b)) and st1.as_dict() == st2.as_dict()   # every cell is written, whatever the buffer held
    want, wst = gc.shim_grid(shim, rec, gp)
    assert a.cpu().numpy().tobytes() == want.tobytes() and st1.as_dict() == wst
    assert records.cpu().numpy().tobytes() == rec.tobytes()            # the records are read only
    cells, _, st = core.world_grid(ctx, records, 5000, gp)              # a torch tensor as the device address
    assert cells.tobytes() == want.tobytes() and st == wst


W, H = 360, 32


def test_no_side_effects_on_a_pipeline():
    p = params_with_size(W, H, submap_extent=4.0, submap_dimension=2)
    a, b = core.SurfelMapping(p), core.SurfelMapping(p)
    cells = 0
    for k in range(30):
        sc = ls.scan(k, W, H)
        a.processScan(*sc, fixed_iterations=6)
        b.processScan(*sc, fixed_iterations=6)
        if k % 5 == 4:
            cells += b.map.export_grid(cell_size=0.5)[0].size
        assert np.array_equal(a.getCurrentPose(), b.getCurrentPose()), k
    assert cells > 1000
    assert a.map.getAllSurfels().tobytes() == b.map.getAllSurfels().tobytes()
    assert a.map.poses().tobytes() == b.map.poses().tobytes()
    assert a.map.counts() == b.map.counts() and a.map.cache_stats() == b.map.cache_stats()
    assert a.map.cached_tiles() == b.map.cached_tiles()
    for ij in a.map.cached_tiles():
        assert a.map.cached_tile(*ij).tobytes() == b.map.cached_tile(*ij).tobytes()


def test_export_grid_of_a_pipeline_equals_the_shim_on_its_world_export(shim):
    p = params_with_size(W, H, submap_extent=4.0, submap_dimension=2)
    pipe = core.SurfelMapping(p)
    for k in range(12):
        pipe.processScan(*ls.scan(k, W, H), fixed_iterations=6)
    for kw in (dict(), dict(min_confidence=0.0, keep_labels=[40, 48, 50])):
        world = pipe.map.export_world(**kw)
        assert len(world) > (0 if kw else 3000)
        cells, gp, st = pipe.map.export_grid(cell_size=0.25, fit_margin=1, fill_radius=3, **kw)
        assert (gp.origin_x, gp.origin_y, gp.width, gp.height) == gc.fit_of(world, 0.25, 1) and gp.fill_radius == 3
        want, wst = gc.shim_grid(shim, world, gp)
        assert st == wst and cells.tobytes() == want.tobytes()
        assert st["n_binned"] == len(world) and (kw or st["n_free"] > 100)
    # a raster given in full is taken as it is
    gp = gc.params(40, 30, 0.5, origin=(-10.0, -7.5))
    cells, gp2, st = pipe.map.export_grid(params=gp)
    want, wst = gc.shim_grid(shim, pipe.map.export_world(), gp)
    assert bytes(gp2) == bytes(gp) and st == wst and cells.tobytes() == want.tobytes() and st["n_outside"] > 0


def test_export_map_tool_writes_a_grid(tmp_path):
    """tools/export_map.py --grid end to end on three small scans: the file holds the cells its stats count"""
    import json
    import os
    import subprocess
    import sys
    from semantic_suma_amd import mapio
    from test_gpu_cpp import ROOT
    out, grid, png = str(tmp_path / "map.ply"), str(tmp_path / "map.grid.npz"), str(tmp_path / "map.grid.png")
    line = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "export_map.py"), "--out", out, "--scans", "3",
                                    "--width", "360", "--repeat", "1", "--grid", grid, "--grid-cell", "0.5", "--grid-png", png,
                                    "--compare"], timeout=120).decode().strip().splitlines()[-1]
    res = json.loads(line)
    cells, gp = mapio.read_grid(grid)
    st = res["grid_stats"]
    assert [gp.width, gp.height] == res["grid_size"] and cells.shape == (gp.height, gp.width)
    assert int((cells["support"] > 0).sum()) == st["n_occupied"] == res["grid_numpy_route_occupied"] > 100
    assert int(cells["support"].sum()) == st["n_binned"] == res["stats"]["n_out"]
    assert {"grid_classify", "grid_sort", "grid_reduce", "grid_finish", "grid_fit"} <= set(res["grid_kernels_us"])
    assert open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
