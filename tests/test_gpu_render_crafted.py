"""K4 / K5 / the fused K7 splat (k_render.hip) on the crafted maps of tests/test_render_crafted_host.py: every room scene
and every structural row bit for bit against the oracle (all three maps of the old, new, composed and output frames
after every call) AND directly against the fp64 statement of tests/render_ref.py -- winner ids read from the semantic
payload, positions and normals within 8 * 2^-24 * sum|terms| -- on the pixels fp64 decides.  The host file proves on the
CPU that the oracle meets the same bounds and that every row's precondition holds."""
import numpy as np
import pytest

import test_render_crafted_host as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


class HipSide:
    """the kernel behind the interface of H.OracleSide"""

    def __init__(self, hip, p):
        self.hip, self.p = hip, p
        self.ctx = hip.Context(p)
        self.map = hip.SurfelMap(self.ctx)

    def load(self, poses, records, timestamp):
        self.map.updatePoses(poses)
        self.map.upload(records, timestamp)

    def call(self, c):
        kind, a, b, ct = c
        out = None
        if kind == "render":
            out = self.map.render(a, b, self.hip.Frame(self.ctx, self.p.model_width, self.p.model_height), ct)
        elif kind == "active":
            self.map.render_active(a, ct)
        elif kind == "inactive":
            self.map.render_inactive(a, ct)
        else:
            self.map.render_composed(a, b, ct)
        res = {nm: np.stack([self.map._frame(w).download(m) for m in range(3)]) for w, nm in enumerate(H.FRAMES)}
        if out is not None:
            res["out"] = np.stack([out.download(m) for m in range(3)])
        return res

    def index_map(self, pose):
        self.map.update(pose, self.hip.Frame(self.ctx, self.p.data_width, self.p.data_height))
        return self.map.index_map()


_RESULTS = {}


def hip_results(hip, sid):
    """the kernel's frames of a scene, computed once and shared"""
    if sid not in _RESULTS:
        sc = H.get_scene(sid)
        _RESULTS[sid] = H.run_scene(HipSide(hip, sc["params"]), sc)
    return _RESULTS[sid]


@pytest.mark.parametrize("sid", H.ROOM_IDS)
def test_room_scene(hip, oracle_lib, sid):
    got = hip_results(hip, sid)
    worst = H.check_against_fp64(sid, got, f"kernel {sid}")
    print(f"{sid}: worst |kernel - fp64| / (2^-24 sum|terms|) = {worst:.2f}")
    H.assert_results_equal(got, H.oracle_results(sid), sid)
    if H.get_scene(sid)["params"].compose_rendering:  # K5's three branches at their named pixels
        ids = H.semantic_ids(got[0]["out"][2])
        winner, _ = H.fp64_call(sid, 0)["out"]
        for nm, (x, y) in H.K5_PIXELS[sid].items():
            assert ids[y, x] == winner[y, x], f"K5 pixel {nm} at ({x}, {y})"


@pytest.mark.parametrize("sid", H.ROW_IDS)
def test_row_equals_oracle(hip, oracle_lib, sid):
    H.assert_results_equal(hip_results(hip, sid), H.oracle_results(sid), sid)


@pytest.mark.parametrize("sid", H.FP64_ROW_IDS)
def test_row_against_fp64(hip, oracle_lib, sid):
    H.check_against_fp64(sid, hip_results(hip, sid), f"kernel {sid}")


@pytest.mark.parametrize("W", (2047, 2048))
def test_big_box(hip, oracle_lib, W):
    """2047 x 1024: the reciprocal row / column split at the largest test index the geometry allows; 2048 x 1024: BIG"""
    sid = f"big-box-{W}x1024"
    sc = H.get_scene(sid)
    got = H.run_scene(HipSide(hip, sc["params"]), sc)
    H.assert_results_equal(got, H.run_scene(H.OracleSide(oracle_lib, sc["params"]), sc), sid)
    H.check_big_box(sid, got, f"kernel {sid}")
    H.fp64_call.cache_clear()
    H._quads.cache_clear()


def test_size_rows(hip, oracle_lib):
    H.check_size_rows(lambda sid: hip_results(hip, sid))


def test_empty_map_between(hip):
    H.check_empty_map_between(lambda p: HipSide(hip, p))


def test_tiles_rows(hip, oracle_lib):
    H.check_tiles_rows(lambda sid: hip_results(hip, sid))


def test_tie_rows(hip, oracle_lib):
    H.check_tie_rows(hip_results(hip, "tie"))


def test_diagonal_rows(hip, oracle_lib):
    H.check_diagonal_rows(lambda sid: hip_results(hip, sid))


def test_rim_row(hip, oracle_lib):
    assert H.check_rim_row(hip_results(hip, "rim-exact")) == H.check_rim_row(H.oracle_results("rim-exact"))


def test_seam_rows(hip, oracle_lib):
    H.check_seam_rows(hip_results(hip, "seam"))


def test_gate_rows(hip, oracle_lib):
    H.check_gate_rows(lambda sid: hip_results(hip, sid))


def test_bad_rows(hip, oracle_lib):
    H.check_bad_rows(lambda sid: hip_results(hip, sid))


def test_carry_nothing_over(hip, oracle_lib):
    """the repeats equal the first run in bits, and the first run equals the oracle's"""
    H.check_carry_nothing_over(lambda p: HipSide(hip, p))
    H.assert_results_equal(hip_results(hip, H.CARRY[0]), H.oracle_results(H.CARRY[0]), H.CARRY[0])


@pytest.mark.parametrize("sid,data_size", H.INDEX_MAP_SCENES)
def test_index_map(hip, oracle_lib, sid, data_size):
    """K7 fused into the render pass: equal to the oracle's index map everywhere, to fp64's on decided texels"""
    got = H.check_index_map(lambda p: HipSide(hip, p), sid, data_size, f"kernel {sid}")
    want = H.check_index_map(lambda p: H.OracleSide(oracle_lib, p), sid, data_size, f"oracle {sid}")
    np.testing.assert_array_equal(got, want, err_msg=f"{sid}: index map differs from the oracle's")
