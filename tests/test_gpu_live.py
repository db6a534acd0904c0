"""The live obstacle layer on the MI355X (csrc/k_live.hip, suma_localizer_*live*, core.Localizer): state, composed cells,
mask, counts and stats byte for byte against the host restatement (tests/live_shim.c) through liveUpdateFlags, on a
localiser with a one-record map: every named case of live_common (the hit rule, the sequences, the carve rule), random
sequences at every frame and raster shape, objects on and off, the refusals, and two runs giving the same bytes.  The
rasters are crafted cells uploaded for the call; no grid is computed."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library: torch and libsuma_hip.so must share one HIP runtime

import live_common as lv
import object_common as oc
from semantic_suma_amd import core
from semantic_suma_amd.types import (GRID_CELL_DTYPE, LiveParams, NovelParams, ObjectParams, WORLD_SURFEL_DTYPE,
                                     params_with_size)

pytestmark = pytest.mark.gpu

# W x H: 210 texels (no multiple of the wave), 520 (three blocks of 256), 257 x 1 (two blocks), 1 x 5
FRAMES = [(70, 3), (130, 4), (257, 1), (1, 5)]
# cells: one; 35 (no multiple of the wave); 2145 (nine blocks of 256, the last one partly filled); a strip of 771
RASTERS = [(1, 1), (7, 5), (65, 33), (257, 3)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return lv.build_shim(tmp_path_factory.mktemp("live_gpu"))


class Rig:
    """a localiser with a one-record map and novelty on, and one data-sized frame; layer() switches the live layer on over
    crafted cells and gives it the interface of live_common.ShimLayer"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.loc = core.Localizer(params_with_size(W, H, submap_extent=10.0, submap_dimension=2))
        rec = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
        rec["nz"], rec["radius"], rec["confidence"] = 1.0, 0.1, 5.0
        self.loc.setMap(rec)
        self.loc.enableNovelty(NovelParams.defaults(max_candidates=1024))
        self.frame = core.Frame(self.loc.ctx, W, H)
        self.S = np.zeros((H, W, 4), dtype=np.float32)

    def layer(self, cells, gp, lp=None):
        self.gp, self.lp = gp, LiveParams.defaults() if lp is None else lp
        self.loc.enableLiveGrid(np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE), gp, self.lp)
        self.now = 0
        return self

    def update(self, V, flags, T, scan_id, ids=None):
        assert ids is None
        self.frame.set(V, np.zeros_like(V), self.S)
        counts = self.loc.liveUpdateFlags(self.frame, T, flags, scan_id)
        assert self.loc.liveCounts() == counts
        self.now = scan_id + 1
        return counts

    def state(self):
        return self.loc.liveState()

    def set_state(self, state, last_stamp):
        self.loc.setLiveState(state, last_stamp)
        self.now = last_stamp

    def compose(self):
        return self.loc.liveCells()

    def close(self):
        self.loc.close()


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = Rig(W, H)
        return made[(W, H)]

    yield get
    for r in made.values():
        r.close()


# ---- 1. every named case: the hit rule, the sequences on one layer, the carve rule
CASES = lv.named_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_named_cases_equal_shim(shim, rigs, case):
    want = lv.ShimLayer(shim, case.cells, case.gp, case.lp)
    got = rigs(lv.W0, lv.H0).layer(case.cells, case.gp, case.lp)
    cw, cg = case.run(want), case.run(got)
    assert cg == cw, (cg, cw)
    lv.same_layer(got, want, case.name)
    case.expect(cg, got)


# ---- 2. every frame shape on every raster: six updates on one layer, compared after each
@pytest.mark.parametrize("W,H", FRAMES)
def test_random_sequences_equal_shim(shim, rigs, W, H):
    rig = rigs(W, H)
    for gw, gh in RASTERS:
        gp, cells, lp, steps = lv.random_sequence(W, H, gw, gh, seed=W + gw)
        want, got = lv.ShimLayer(shim, cells, gp, lp), rig.layer(cells, gp, lp)
        assert got.compose()[2] == dict(n_live=0, n_pending=0, n_expired=0, n_carved=0) and rig.loc.liveCounts() is None
        for k, (V, fl, T, sid) in enumerate(steps):
            cw, cg = want.update(V, fl, T, sid), got.update(V, fl, T, sid)
            assert cg == cw, (W, H, gw, gh, k, cg, cw)
            lv.same_layer(got, want, (W, H, gw, gh, k))
        print(W, H, gw, gh, cw, want.compose()[2])


# ---- 3. clear zeroes; a new map does too; the stamps start again
def test_clear_zeroes(shim, rigs):
    rig = rigs(70, 3)
    gp, cells, lp, steps = lv.random_sequence(70, 3, 7, 5, seed=2)
    want, got = lv.ShimLayer(shim, cells, gp, lp), rig.layer(cells, gp, lp)
    for V, fl, T, sid in steps[:3]:
        want.update(V, fl, T, sid), got.update(V, fl, T, sid)
    assert got.state().view(np.uint8).any()
    static = np.ascontiguousarray(cells, dtype=GRID_CELL_DTYPE).reshape(gp.height, gp.width)
    for how in ("clear", "set_map"):
        if how == "clear":
            rig.loc.clearLiveGrid()
        else:
            rec = np.zeros(1, dtype=WORLD_SURFEL_DTYPE)
            rec["nz"], rec["radius"], rec["confidence"] = 1.0, 0.1, 5.0
            rig.loc.setMap(rec)
        assert not got.state().view(np.uint8).any() and rig.loc.liveCounts() is None
        out, mask, st = got.compose()
        assert out.tobytes() == static.tobytes() and not mask.any() and st == dict(n_live=0, n_pending=0, n_expired=0, n_carved=0)
        want.clear()
        for V, fl, T, sid in steps[:2]:                     # scan ids 0, 1 again: the last stamp went back to 0
            assert got.update(V, fl, T, sid) == want.update(V, fl, T, sid)
        lv.same_layer(got, want, how)


# ---- 4. objects: with them on, components below min_texels do not hit; with them off, they do
def test_objects_filter_the_hits(shim, rigs, tmp_path_factory):
    W, H = 70, 3
    rig = rigs(W, H)
    oshim = oc.build_shim(tmp_path_factory.mktemp("live_gpu_objects"))
    V, S, fl, pose, op = oc.sized_components(W, H, 5)            # runs of 4, 5 and 6 texels in row 0
    # loop_frame at oc.POSE: world x = 2 - y, world y = x - 3, world z = z + 0.5 = -0.5: the ground at -1 makes them hits
    gp = lv.grid_params(8, 16, cell_size=0.25, origin=(1.0, 5.0))
    cells = lv.flat_cells(gp, -1.0)
    lp = LiveParams.defaults(min_hits=1)
    _, ids, ocnt = oc.shim_segment(oshim, V, S, fl, pose, op, 0)
    assert ocnt["n_small"] == 1 and ocnt["n_objects"] == 2
    on, off = lv.ShimLayer(shim, cells, gp, lp), lv.ShimLayer(shim, cells, gp, lp)
    c_on, c_off = on.update(V, fl, pose, 0, ids), off.update(V, fl, pose, 0)
    assert (c_on["n_members"], c_off["n_members"]) == (11, 15) and c_on["n_hit_texels"] == 11 and c_off["n_hit_texels"] == 15
    rig.S = S
    try:
        rig.loc.enableObjects(op)
        got = rig.layer(cells, gp, lp)
        assert got.update(V, fl, pose, 0) == c_on
        lv.same_layer(got, on, "objects on")
        assert rig.loc.objects()[1] == ocnt and rig.loc.objectIds().tobytes() == ids.tobytes()
        rig.loc.disableObjects()
        got = rig.layer(cells, gp, lp)
        assert got.update(V, fl, pose, 0) == c_off
        lv.same_layer(got, off, "objects off")
    finally:
        rig.loc.disableObjects()
        rig.S = np.zeros((H, W, 4), dtype=np.float32)


# ---- 5. refusals launch nothing: the state stays as it was
def test_refusals(shim, rigs):
    rig = rigs(70, 3)
    gp, cells, lp, steps = lv.random_sequence(70, 3, 7, 5, seed=4)
    got = rig.layer(cells, gp, lp)
    loc = rig.loc
    V, fl, T, _ = steps[0]
    got.update(V, fl, T, 5)
    before = got.state().tobytes()
    for sid in (5, 4, 0, 0xffffffff):                       # stamps 6, 5, 1 and 0: none above the last one's
        with pytest.raises(core.SumaError, match="stamp"):
            loc.liveUpdateFlags(rig.frame, T, fl, sid)
    with pytest.raises(ValueError, match="one byte per texel"):
        loc.liveUpdateFlags(rig.frame, T, fl.reshape(-1)[:-1], 6)
    with pytest.raises(core.SumaError, match="non-finite"):
        loc.liveUpdateFlags(rig.frame, np.full((4, 4), np.nan), fl, 6)
    with pytest.raises(core.SumaError, match="data image"):
        loc.liveUpdateFlags(core.Frame(loc.ctx, 70, 4), T, fl, 6)
    d = torch.zeros(35 * 12 + 8, dtype=torch.int32, device="cuda")
    with pytest.raises(core.SumaError, match="aligned"):
        loc.liveCells(out=d.data_ptr() + 4)
    assert not d.cpu().numpy().any()
    assert loc.L.suma_localizer_live_cells_device(loc.h, None, None, None) == -1
    assert got.state().tobytes() == before and loc.liveCounts()["n_texels"] == 210
    # the composed cells on the device equal the downloaded ones, and nothing beyond them is written
    cells_h, mask, st = loc.liveCells()
    _, mask_d, st_d = loc.liveCells(out=d)
    back = d.cpu().numpy()
    assert back[:35 * 12].tobytes() == cells_h.tobytes() and not back[35 * 12:].any() and mask_d.tobytes() == mask.tobytes()
    assert st_d == st
    # enabling: parameters, raster, alignment, novelty
    for bad, what in ((dict(hold_scans=0), "hold_scans"), (dict(min_hits=65536), "min_hits"),
                      (dict(carve_range=float("nan")), "carve_range"), (dict(carve_margin=-1.0), "carve_margin")):
        with pytest.raises(core.SumaError, match=what):
            loc.enableLiveGrid(cells, gp, LiveParams.defaults(**bad))
    for bad, what in ((dict(cell_size=0.0), "cell_size"), (dict(step_height=float("inf")), "step_height"),
                      (dict(clearance=0.1), "clearance"), (dict(fill_radius=9), "fill_radius")):
        kw = dict(cell_size=1.0, width=7, height=5, step_height=0.25, clearance=2.0)
        kw.update(bad)
        from semantic_suma_amd.types import GridParams
        with pytest.raises(core.SumaError, match=what):
            loc.enableLiveGrid(cells, GridParams.defaults(**kw), lp)
    with pytest.raises(ValueError, match="cells against a raster"):
        loc.enableLiveGrid(cells[:-1], gp, lp)
    dc = torch.zeros(35 * 12 + 8, dtype=torch.int32, device="cuda")
    with pytest.raises(core.SumaError, match="aligned"):
        loc.enableLiveGrid(dc.data_ptr() + 4, gp, lp)
    assert got.state().tobytes() == before                  # a refused enable leaves the layer
    other = core.Localizer(params_with_size(70, 3, submap_extent=10.0, submap_dimension=2))
    with pytest.raises(core.SumaError, match="novelty is off"):
        other.enableLiveGrid(cells, gp, lp)
    other.enableNovelty(NovelParams.defaults(max_candidates=64))
    assert other.L.suma_localizer_live_counts(other.h, None, None) == -1
    assert "live layer is off" in other.L.suma_last_error(other.ctx.h).decode()
    other.enableLiveGrid(cells, gp, lp)
    assert other.liveCounts() is None
    other.disableNovelty()                                  # takes the layer with it
    assert other.L.suma_localizer_clear_live_grid(other.h) == -1
    other.close()


# ---- 6. two runs give the same bytes; a second compose does too
def test_repeatability(shim, rigs):
    rig = rigs(130, 4)
    gp, cells, lp, steps = lv.random_sequence(130, 4, 65, 33, seed=6)
    runs = []
    for _ in range(2):
        got = rig.layer(cells, gp, lp)
        per = []
        for V, fl, T, sid in steps:
            c = got.update(V, fl, T, sid)
            out, mask, st = got.compose()
            again = got.compose()
            assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == mask.tobytes() and again[2] == st
            per.append((c, got.state().tobytes(), out.tobytes(), mask.tobytes(), st))
        runs.append(per)
    assert runs[0] == runs[1]
