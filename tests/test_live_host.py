"""The live obstacle layer on the host (no GPU): the restatement tests/live_shim.c against a plain Python statement of
csrc/k_live.hip's specification (live_common.PyLayer) on crafted and random sequences with dyadic coordinates, NaN and
infinite points; the named cases give what the specification says; the shim as a program of its own under the address and
undefined-behaviour sanitizers; and the semantic check of DESIGN.md 20 on DESIGN.md 19's scenario."""
import os
import subprocess

import numpy as np
import pytest

import live_common as lv
from semantic_suma_amd.types import LiveParams

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return lv.build_shim(tmp_path_factory.mktemp("live_host"))


CASES = lv.named_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_named_cases(shim, case):
    """the shim equals the Python statement, and both give what the specification says"""
    a, b = lv.ShimLayer(shim, case.cells, case.gp, case.lp), lv.PyLayer(case.cells, case.gp, case.lp)
    ca, cb = case.run(a), case.run(b)
    assert ca == cb, (ca, cb)
    lv.same_layer(a, b, case.name)
    for c in ca:
        assert c["n_members"] == c["n_outside"] + c["n_no_ground"] + c["n_low"] + c["n_high"] + c["n_hit_texels"], c
    case.expect(ca, a)
    case.expect(cb, b)


@pytest.mark.parametrize("W,H,gw,gh", [(70, 3, 7, 5), (130, 4, 65, 33), (257, 1, 257, 3), (1, 5, 1, 1), (70, 3, 1, 1)])
def test_random_sequences(shim, W, H, gw, gh):
    """six updates of random frames on one layer, compared after every update; with an id image on every other one"""
    gp, cells, lp, steps = lv.random_sequence(W, H, gw, gh, seed=W + gw)
    a, b = lv.ShimLayer(shim, cells, gp, lp), lv.PyLayer(cells, gp, lp)
    rng = np.random.RandomState(3)
    seen = dict.fromkeys(lv.ZERO, 0)
    stats = dict(n_live=0, n_pending=0, n_expired=0, n_carved=0)
    for k, (V, fl, T, sid) in enumerate(steps):
        ids = None if k % 2 == 0 else np.where(rng.rand(H, W) < 0.2, lv.NONE, 5).astype(np.uint32)
        ca, cb = a.update(V, fl, T, sid, ids), b.update(V, fl, T, sid, ids)
        assert ca == cb, (k, ca, cb)
        _, _, st = lv.same_layer(a, b, (W, H, gw, gh, k))
        for key in seen:
            seen[key] += ca[key]
        for key in stats:
            stats[key] += st[key]
    print(seen, stats)
    if W * H >= 200 and gw * gh > 1:      # the sequence reaches every class of the hit rule and every class of a cell
        assert all(seen[key] > 0 for key in seen), seen
        # (on the strip 257 texels meet 771 cells: two hits in a row in one cell, which live takes, do not occur)
        assert all(stats[key] > 0 for key in stats if key != "n_live" or gw <= 4 * gh), stats


def test_update_order_does_not_matter(shim):
    """the texels of a frame in reverse order give the same state: what the atomics of the library rely on"""
    gp, cells, lp, steps = lv.random_sequence(70, 3, 7, 5, seed=9)
    a, b = lv.ShimLayer(shim, cells, gp, lp), lv.ShimLayer(shim, cells, gp, lp)
    for V, fl, T, sid in steps:
        ca = a.update(V, fl, T, sid)
        cb = b.update(V.reshape(-1, 4)[::-1].reshape(V.shape), fl.reshape(-1)[::-1].reshape(fl.shape), T, sid)
        assert ca == cb
        lv.same_layer(a, b, sid)


def test_write_grid_keeps_the_composed_cells(shim, tmp_path):
    """mapio.write_grid / read_grid: a composed grid goes through like a static one, live obstacles included"""
    from semantic_suma_amd import mapio
    gp, cells, lp, steps = lv.random_sequence(70, 3, 7, 5, seed=1)
    a = lv.ShimLayer(shim, cells, gp, LiveParams.defaults(min_hits=1))
    for V, fl, T, sid in steps[:2]:
        a.update(V, fl, T, sid)
    comp, mask, st = a.compose()
    assert st["n_live"] > 0 and comp.tobytes() != a.cells.tobytes()
    mapio.write_grid(str(tmp_path / "live.npz"), comp, gp)
    back, gp2 = mapio.read_grid(str(tmp_path / "live.npz"))
    assert back.tobytes() == comp.tobytes() and bytes(gp2) == bytes(gp)
    assert (back["state"][mask == 1] == 2).all()


def test_shim_under_sanitizers(tmp_path):
    """tests/live_shim.c as a program of its own (its main runs nine updates and composes), -fsanitize=address,undefined"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.call(["gcc"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0 or \
            subprocess.call([str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("the compiler cannot link the sanitizers")
    exe = str(tmp_path / "live_shim_san")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off"] + flags +
                          ["-DLIVE_SHIM_MAIN", os.path.join(HERE, "live_shim.c"), "-o", exe, "-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-4000:])
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 9 and "live" in lines[-1], lines


# ---- the semantic check: DESIGN.md 19's scenario through the CPU restatement of the localiser, the grid and plan shims
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    import novel_common as nc
    tmp = tmp_path_factory.mktemp("live_scene")
    shims = lv.scenario_shims(tmp)
    return shims, tmp, lv.scenario_run(shims, tmp, nc.ADDED)


def test_the_added_building_becomes_live_obstacles(scene):
    """Measured on this restatement with the default parameters (live_common.MEASURED): after 24 of the 25
    scans -- all but the first, which can only make cells pending -- a live cell lies inside building 41's footprint; at
    least 0.879 of the live cells lie inside the footprint grown by one cell (the others are returns the map as mapped
    does not explain elsewhere); the control run, the same world mapped and localised, never has a live cell."""
    import novel_common as nc
    shims, tmp, run = scene
    hits, share, _ = lv.scenario_measure(run)
    control = lv.scenario_run(shims, tmp, ())
    control_live = lv.scenario_measure(control)[2]
    print("scans with a live cell in the building %d, smallest share %.6f, control live cells %d" % (hits, share, control_live))
    print([st["n_live"] for st in run["stats"]], [c["n_cleared"] for c in run["counts"]])
    assert len(run["masks"]) == nc.LAST - nc.FIRST + 1
    assert hits == lv.MEASURED["scans_with_building"] and abs(share - lv.MEASURED["min_share"]) < 1e-6
    assert control_live == lv.MEASURED["control_live"]
    lv.check_measured(hits, share, control_live)


def test_the_path_goes_round_the_building(scene):
    """a start and a goal on opposite sides of building 41: on the static grid the path crosses the footprint; on the
    composed grid after the scan MEASURED names (and after the last one) no cell of it lies inside, and it costs more"""
    import object_common as oc
    shims, tmp, run = scene
    gp = run["gp"]
    fin = lv.footprint(gp, oc.building_box(), 0.0).reshape(-1)
    res, cells = lv.scenario_path(shims, gp, run["cells"], lv.PATH_START, lv.PATH_GOAL)
    assert res["status"] == 0 and fin[cells].sum() > 10 and res["cost"] == lv.MEASURED["static_cost"], (res, fin[cells].sum())
    assert lv.MEASURED["path_from"] in lv.KEEP
    for k in lv.KEEP:
        res_k, cells_k = lv.scenario_path(shims, gp, run["composed"][k], lv.PATH_START, lv.PATH_GOAL)
        print(k, res_k, int(fin[cells_k].sum()))
        assert res_k["status"] == 0 and not fin[cells_k].any() and res_k["cost"] > res["cost"], (k, res_k)
    assert lv.scenario_path(shims, gp, run["composed"][lv.MEASURED["path_from"]], lv.PATH_START, lv.PATH_GOAL)[0]["cost"] == \
        lv.MEASURED["live_cost"]
    # the robot's own start: the cell of the run's first pose
    P = run["poses"][0]
    start = (int((P[0, 3] - gp.origin_x) / gp.cell_size), int((P[1, 3] - gp.origin_y) / gp.cell_size))
    res0 = lv.scenario_path(shims, gp, run["cells"], start, lv.ROBOT_GOAL)
    res4 = lv.scenario_path(shims, gp, run["composed"][4], start, lv.ROBOT_GOAL)
    assert fin[res0[1]].any() and not fin[res4[1]].any() and res4[0]["cost"] > res0[0]["cost"], (res0[0], res4[0])


def test_what_has_gone_stops_being_live_sooner_with_carving(scene):
    """The scenario gives the layer no moving car to follow (away from the two added boxes a single cell becomes live in
    the whole run), so what goes is the building: from scan index 10 on the scans are those of the world without it.  With carving
    the last live cell of its grown footprint is gone 1 scan later, without carving after 9 (hold_scans - 1)."""
    import novel_common as nc
    import object_common as oc
    shims, tmp, run = scene
    fgrow = lv.footprint(run["gp"], oc.building_box(), run["gp"].cell_size)
    took = {}
    for name, lp in (("on", LiveParams.defaults()), ("off", LiveParams.defaults(carve_range=0.0))):
        r = lv.scenario_run(shims, tmp, nc.ADDED, lp, gone_from=lv.TRAIL_GONE, gone_without=(23 + 18,))
        live = [int(((m == 1) & fgrow).sum()) for m in r["masks"]]
        print(name, live)
        assert live[lv.TRAIL_GONE - 1] > 20
        took[name] = next(k for k in range(lv.TRAIL_GONE, len(live)) if live[k] == 0) - lv.TRAIL_GONE
    assert took == dict(on=lv.MEASURED["trail_carve_on"], off=lv.MEASURED["trail_carve_off"]), took
    assert took["on"] < took["off"]
