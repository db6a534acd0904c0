"""The world export's specification on the host (tests/world_shim.c, the yardstick of test_gpu_world.py): the label
rule, and properties of the shim's output on a synthetic map that an independent numpy formulation confirms; the PLY
round trip of semantic_suma_amd.mapio."""
import numpy as np
import pytest

import draw_common as dc
import world_common as wc
from semantic_suma_amd import kitti, mapio
from semantic_suma_amd.types import WORLD_SURFEL_DTYPE

N_POSES = 16


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return wc.build_shim(tmp_path_factory.mktemp("world_host"))


@pytest.fixture(scope="module")
def planar():
    return dc.planar_map(5000)


def test_label_rule_inverts_l_over_255(shim):
    for l in range(260):
        r = np.float32(l) / np.float32(255.0)
        assert shim.world_shim_label(float(r)) == l
        assert wc.labels_of(np.array([(r,)], dtype=[("r", "<f4")]))[0] == l
    for r in (np.nan, np.inf, -np.inf, -1.0, 260.0 / 255.0 + 1e-3, 1e30):
        assert shim.world_shim_label(float(r)) == 0, r
    assert shim.world_shim_weight(float("nan")) == 0 and shim.world_shim_weight(2.0) == 65535
    assert shim.world_shim_weight(-1.0) == 0 and shim.world_shim_weight(0.5) == 32768  # rint(32767.5): to even


def test_flat_mode_is_the_transform_of_each_kept_source_in_order(shim, planar):
    s, poses = planar
    p, n = wc.shim_transform(shim, s, poses, N_POSES)
    # the fma chain against fp64: a rigid pose of a point within 100 m, error far below a millimetre
    k = s["count"].astype(int)
    want = np.einsum("nij,nj->ni", poses[k].astype(np.float64),
                     np.stack([s["x"], s["y"], s["z"], np.ones(len(s))], 1).astype(np.float64))
    assert np.abs(p - want).max() < 1e-4
    keep = [10, 40, 44, 48]
    out, st, _ = wc.shim_export(shim, s, poses, N_POSES, min_confidence=3.0, keep_labels=keep)
    sel = (s["confidence"] > np.float32(3.0)) & np.isin(wc.labels_of(s), keep)
    assert 0 < sel.sum() < len(s)
    assert st == dict(n_passed=int(sel.sum()), n_dropped=0, n_out=int(sel.sum()))
    assert out["x"].tobytes() == p[sel, 0].tobytes() and out["y"].tobytes() == p[sel, 1].tobytes()
    assert out["z"].tobytes() == p[sel, 2].tobytes() and out["nz"].tobytes() == n[sel, 2].tobytes()
    assert out["nx"].tobytes() == n[sel, 0].tobytes() and out["ny"].tobytes() == n[sel, 1].tobytes()
    for a, b in (("radius", "radius"), ("confidence", "confidence"), ("prob", "w"), ("timestamp", "timestamp")):
        assert out[a].tobytes() == s[b][sel].tobytes(), a
    assert np.array_equal(out["label"], wc.labels_of(s)[sel]) and np.all(out["support"] == 1)


@pytest.mark.parametrize("voxel", [0.25, 1.0, 8.0])
def test_voxel_mode_properties(shim, planar, voxel):
    s, poses = planar
    out, st, keys = wc.shim_export(shim, s, poses, N_POSES, voxel_size=voxel)
    assert int(out["support"].sum()) == st["n_passed"] - st["n_dropped"] == len(s)
    assert st["n_out"] == len(out) and np.all(np.diff(keys.astype(np.int64)) > 0)
    # every output lies in its own voxel
    ijk = wc.voxel_index(np.stack([out["x"], out["y"], out["z"]], 1), voxel)
    assert np.array_equal(wc.key_of(ijk), keys)
    # an independent vote: numpy over the members of each voxel, the integer weights summed in fp64 (exact: < 2^53)
    p, _ = wc.shim_transform(shim, s, poses, N_POSES)
    skey = wc.key_of(wc.voxel_index(p[:, :3], voxel))
    L, q = wc.labels_of(s), wc.weights_of(s).astype(np.float64)
    order = {int(k): i for i, k in enumerate(keys)}
    sums = np.zeros((len(keys), 260))
    np.add.at(sums, ([order[int(k)] for k in skey], L), q)
    assert np.array_equal(out["label"], sums.argmax(1))  # argmax: the first (smallest) id on a tie
    best = sums.max(1)
    assert np.array_equal(out["prob"], (best.astype(np.float32) / sums.sum(1).astype(np.float32)))
    # representative: the greatest confidence of the voxel; timestamp: the latest
    conf = np.full(len(keys), -np.inf)
    np.maximum.at(conf, [order[int(k)] for k in skey], s["confidence"].astype(np.float64))
    assert np.array_equal(out["confidence"].astype(np.float64), conf)
    stamp = np.zeros(len(keys), dtype=np.int64)
    np.maximum.at(stamp, [order[int(k)] for k in skey], s["timestamp"].astype(np.int64))
    assert np.array_equal(out["timestamp"], stamp)


def test_a_smaller_kept_set_never_adds_voxels(shim, planar):
    s, poses = planar
    prev = None
    for mc in (-np.inf, 0.0, 5.0, 10.0):
        _, st, keys = wc.shim_export(shim, s, poses, N_POSES, voxel_size=1.0, min_confidence=mc)
        if prev is not None:
            assert set(keys.tolist()) <= prev and len(keys) < len(prev)
        prev = set(keys.tolist())


def test_capacity_gives_the_prefix(shim, planar):
    s, poses = planar
    for voxel in (0.0, 1.0):
        full, st, _ = wc.shim_export(shim, s, poses, N_POSES, voxel_size=voxel)
        half, st2, _ = wc.shim_export(shim, s, poses, N_POSES, voxel_size=voxel, capacity=st["n_out"] // 2)
        assert st2 == st and half.tobytes() == full[:st["n_out"] // 2].tobytes()


def test_ply_round_trip(tmp_path, shim, planar):
    s, poses = planar
    out, _, _ = wc.shim_export(shim, s, poses, N_POSES, voxel_size=0.5)
    out = out.copy()
    out["label"][:3] = (259, 0, 300)  # 300: outside the colour map -> black
    path = str(tmp_path / "map.ply")
    mapio.write_ply(path, out)
    back, rgb = mapio.read_ply(path)
    assert back.dtype == WORLD_SURFEL_DTYPE and len(back) == len(out)
    for f in ("x", "y", "z", "nx", "ny", "nz", "radius", "confidence", "label", "prob", "support"):
        assert back[f].tobytes() == out[f].tobytes(), f
    cmap = kitti.semantic_color_map()
    assert np.array_equal(rgb[3:], cmap[out["label"][3:]]) and np.all(rgb[2] == 0)
    assert open(path, "rb").read(64).startswith(b"ply\nformat binary_little_endian 1.0\n")
    mapio.write_ply(path, out[:0])
    assert len(mapio.read_ply(path)[0]) == 0
