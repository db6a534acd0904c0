"""k_render's tile groups (semantic_suma_amd/csrc/k_render.hip: the candidates of several consecutive tiles share one
list and one 1b -> prefix -> 2 chain) on the maps of tests/test_render_group_host.py, bit for bit against the oracle:
every map of the old, new, composed and output frames after every call -- merged render, render_active, the unmerged
render and render_composed -- and, on a context of its own, the index map of an update right behind ONE render_active,
whose K7 splat rides on that pass: the kernel-time table must show the fused pass and no K7 pass of the update's own.
The host file proves on the CPU that each map has the per-tile candidate counts it claims; whatever group size and flush
threshold the library was built with, the results are the oracle's."""
import numpy as np
import pytest

import test_render_crafted_host as H
import test_render_group_host as G
from test_gpu_render_crafted import HipSide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from semantic_suma_amd import core
    core.lib()  # raises if libsuma_hip.so is missing: no silent fallback
    return core


_RUNS = {}


def fused_index_map(hip, sc):
    """G.fused_index_map on the kernel, with the proof that the update consumed k_render's splat"""
    side = HipSide(hip, sc["params"])
    side.ctx.profile(1)
    im = G.fused_index_map(side, sc)
    side.ctx.synchronize()
    launches = {k["name"]: k["launches"] for k in side.ctx.profile_get()}
    assert launches.get("k4k7_render_indexmap") == 1 and not launches.get("k7_indexmap"), \
        f"{sc['id']}: the index map is not the fused splat's: {launches}"
    return im


def hip_run(hip, sid):
    """(frames after every call, index map behind one render_active) of the kernel, computed once and shared"""
    if sid not in _RUNS:
        sc = G.get_scene(sid)
        _RUNS[sid] = H.run_scene(HipSide(hip, sc["params"]), sc), fused_index_map(hip, sc)
    return _RUNS[sid]


def check_scene(hip, sid):
    (got, got_im), (want, want_im) = hip_run(hip, sid), G.oracle_run(sid)
    H.assert_results_equal(got, want, sid)
    np.testing.assert_array_equal(got_im, want_im, err_msg=f"{sid}: index map differs from the oracle's")
    return want_im


@pytest.mark.parametrize("sid", G.SIZE_IDS)
def test_sizes(hip, oracle_lib, sid):
    check_scene(hip, sid)


@pytest.mark.parametrize("nA", G.PAIRS_A)
def test_pairs(hip, oracle_lib, nA):
    """one case per nA, every nB inside it: 60 small scenes"""
    drawn = 0
    for nB in G.PAIRS_B:
        drawn += np.count_nonzero(check_scene(hip, f"pair:{nA}+{nB}"))
    assert drawn > 20, "the index maps are empty"


@pytest.mark.parametrize("sid", G.QUAD_IDS)
def test_groups_of_four(hip, oracle_lib, sid):
    sc = G.get_scene(sid)
    want = check_scene(hip, sid)
    if sum(sc["counts"]):
        assert np.count_nonzero(want) > 20 and np.count_nonzero(G.oracle_results(sid)[0]["out"][0][..., 3]) > 20, "an empty rendering"


def test_twins(hip, oracle_lib):
    sid = "group-twins"
    check_scene(hip, sid)
    G.check_twins(hip_run(hip, sid)[0], G.get_scene(sid)["records"])


def test_carry_nothing_over(hip, oracle_lib):
    G.check_carry(lambda p: HipSide(hip, p), G.oracle_results)
