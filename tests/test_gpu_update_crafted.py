"""K8 .. K12 (k_update.hip) on the crafted maps of tests/test_update_crafted_host.py: every room scene and every row
through SurfelMap.updatePoses / upload / update, compared bit for bit with the oracle (surfel buffer, radius_conf, index
map, integration mask, counts, cached tiles, origin after every update) AND -- the room scenes and the geometric rows --
directly with the fp64 statement of tests/update_ref.py on what fp64 decides.  The host file proves on the CPU that the
oracle meets the same bounds and that every row's precondition holds."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import test_update_crafted_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


@contextmanager
def environ(env):
    """variables the product reads while an update runs, set for that call only"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class HipSide:
    """the kernel behind the interface of H.OracleSide"""

    def __init__(self, hip, p):
        self.hip, self.p = hip, p
        self.ctx = hip.Context(p)
        self.map = hip.SurfelMap(self.ctx)

    def load(self, poses, records, timestamp):
        self.map.updatePoses(poses)
        self.map.upload(records, timestamp)

    def run(self, pose, frame, env=None):
        f = self.hip.Frame(self.ctx, self.p.data_width, self.p.data_height)
        f.set(*frame)
        with environ(env):
            self.map.update(pose, f)

    def update(self, pose, frame, env=None):
        self.run(pose, frame, env)
        s, d, _, origin = self.map.counts()
        tiles = {ij: np.ascontiguousarray(self.map.cached_tile(*ij)).view(np.uint32) for ij in self.map.cached_tiles()}
        return dict(surfels=self.map.getAllSurfels(), radius_conf=self.map.radius_conf(), index=self.map.index_map(),
                    mask=self.map.integrated(), counts=(s, d), size=self.map.size(), origin=origin, tiles=tiles)


_RESULTS = {}


def hip_results(hip, sid):
    """the kernel's results of a scene, computed once and shared"""
    if sid not in _RESULTS:
        sc = H.get_scene(sid)
        _RESULTS[sid] = H.run_scene(HipSide(hip, sc["params"]), sc)
    return _RESULTS[sid]


@pytest.mark.parametrize("sid", H.ROOM_IDS)
def test_room_scene(hip, oracle_lib, sid):
    got = hip_results(hip, sid)
    fig = H.check_against_fp64(sid, got, f"kernel {sid}")
    print(f"{sid}: worst |kernel - fp64| / (2^-24 sum|terms|) = {fig['worst']:.2f}, normal {fig['normal']:.3g}, conf {fig['conf']:.3g}")
    H.assert_results_equal(got, H.oracle_results(sid), sid)


@pytest.mark.parametrize("sid", [s for s in H.ROW_IDS if s not in H.GRID_IDS])
def test_row_equals_oracle(hip, oracle_lib, sid):
    H.assert_results_equal(hip_results(hip, sid), H.oracle_results(sid), sid)


@pytest.mark.parametrize("sid", H.KEEP_ROW_IDS)
def test_keep_rows(hip, sid):
    H.check_keep_row(sid, hip_results(hip, sid))


@pytest.mark.parametrize("sid", H.GRID_IDS)
def test_grid_rows(hip, oracle_lib, sid):
    """263 169 and 524 295 records: more tiles than blocks, so blocks draw a second and a third ticket"""
    sc = H.get_scene(sid)
    got = H.run_scene(HipSide(hip, sc["params"]), sc)
    H.check_grid_row(sid, got, hip_results(hip, H.GRID_BASE))
    H.assert_results_equal(got, H.oracle_results(sid), sid)
    H.oracle_results.cache_clear()


def test_epochs(hip, oracle_lib):
    """status words keep stale epochs, group halves alternate and a third launch shifts the parity: every step on the
    one context equals a fresh context, and the run with a standalone K12 between the steps equals the oracle's"""
    H.check_epochs(lambda p: HipSide(hip, p))


def test_area_edges(hip):
    H.check_area_edges(hip_results(hip, "area-edges"))


def test_extraction_rows(hip, oracle_lib):
    H.check_extraction(lambda sid: hip_results(hip, sid))


@pytest.mark.parametrize("sid", H.K10_IDS)
def test_k10_rows(hip, oracle_lib, sid):
    got = hip_results(hip, sid)
    H.check_k10_row(sid, got)
    H.check_against_fp64(sid, got, f"kernel {sid}")


@pytest.mark.parametrize("name", list(H.GATES))
def test_gate_rows(hip, oracle_lib, name):
    H.check_gate_rows(lambda sid: hip_results(hip, sid), name)
    for side in ("below", "above"):
        H.check_against_fp64(f"gate-{name}-{side}", hip_results(hip, f"gate-{name}-{side}"), f"kernel gate-{name}-{side}")


@pytest.mark.parametrize("sid", H.BRANCH_IDS)
def test_branch_rows(hip, oracle_lib, sid):
    got = hip_results(hip, sid)
    H.check_branch_row(sid, got)
    H.check_against_fp64(sid, got, f"kernel {sid}")


@pytest.mark.parametrize("sid", H.BAD_IDS)
def test_bad_rows(hip, sid):
    H.check_bad_row(sid, hip_results(hip, sid))


@pytest.mark.parametrize("sid", H.CAPACITY_IDS)
def test_capacity_rows(hip, oracle_lib, sid):
    """max_surfels reached: size() reports it; the truncated buffer, read with suma_map_download, is the oracle's"""
    import ctypes as C
    from semantic_suma_amd.types import SURFEL_DTYPE
    sc = H.get_scene(sid)
    side = HipSide(hip, sc["params"])
    side.load(sc["poses"], sc["records"], sc["timestamp"])
    side.run(*sc["updates"][0][:2])
    with pytest.raises(hip.SumaError, match="max_surfels"):
        side.map.size()
    cap = sc["params"].max_surfels
    out, n = np.zeros(cap, dtype=SURFEL_DTYPE), C.c_uint32(0)
    side.ctx.check(side.ctx.L.suma_map_download(side.ctx.h, hip._ptr(out), cap, C.byref(n)), "suma_map_download")
    assert n.value == cap
    want = H.oracle_results(sid)[0]
    assert out.tobytes() == want["surfels"].tobytes(), f"{sid}: the truncated map differs from the oracle's"
    H.check_capacity_row(sid, [dict(surfels=out)])
