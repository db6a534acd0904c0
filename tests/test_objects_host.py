"""The per-scan objects' specification on the host (tests/object_shim.c, the yardstick of test_gpu_objects.py): the shim
-- a flood fill over a stack -- against a plain Python statement of every rule -- breadth-first search over the link
graph, sums in Python integers -- on random flag images and crafted ones; the shim under the address and
undefined-behaviour sanitizers as a stand-alone program; and one semantic check without a GPU: DESIGN.md 15's scenario
through the CPU restatement of the localiser, where the added building must come out as objects and the control run as
next to none."""
import subprocess

import numpy as np
import pytest

import object_common as oc
from semantic_suma_amd.types import ObjectParams


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return oc.build_shim(tmp_path_factory.mktemp("object_host"))


def equal(a, b, what):
    assert a[2] == b[2], (what, a[2], b[2])
    assert a[0].tobytes() == b[0].tobytes(), (what, a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes(), what


@pytest.mark.parametrize("W,H", [(13, 4), (70, 3), (9, 1), (1, 5), (2, 4)])
def test_shim_equals_python_on_crafted_frames(shim, W, H):
    for k, (name, V, S, fl, pose, op) in enumerate(oc.crafted_cases(W, H)):
        a = oc.shim_segment(shim, V, S, fl, pose, op, k)
        equal(a, oc.python_segment(V, S, fl, pose, op, k), (W, H, name))
        c = a[2]
        assert c["n_small"] + c["n_objects"] == c["n_components"] and c["stored"] == min(c["n_objects"], op.max_objects)
        assert c["n_members"] <= int(np.count_nonzero(fl)) and c["n_texels"] == W * H


def test_shim_equals_python_on_random_frames(shim):
    """dyadic coordinates (multiples of 1/64 m) at several densities of points and flags, with dv.w = 0 texels, infinite
    and NaN points among them; thresholds that cut the distances that occur"""
    rng = np.random.RandomState(11)
    for trial in range(24):
        W, H = [(17, 5), (24, 3), (6, 6), (40, 2)][trial % 4]
        V, S = np.zeros((H, W, 4), dtype=np.float32), np.zeros((H, W, 4), dtype=np.float32)
        V[..., :3] = rng.randint(-64, 65, (H, W, 3)) / 64.0 + np.array([4.0, 0.0, 0.0])
        V[..., 3] = rng.rand(H, W) < 0.9
        for bad in (np.nan, np.inf, -np.inf):
            V[rng.randint(H), rng.randint(W), rng.randint(3)] = bad
        S[..., 0] = rng.choice([0, 10, 13, 40, 50, 259, 300], (H, W)).astype(np.float32) / np.float32(255.0)
        S[..., 3] = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 1.5, -1.0, np.nan], dtype=np.float32), (H, W))
        fl = (rng.rand(H, W) < (0.5, 0.8, 1.0)[trial % 3]) * rng.randint(1, 256, (H, W))
        op = ObjectParams.defaults(link_base=(0.5, 0.75, 1.0, 0.0)[trial % 4], link_slope=(0.0, 0.0625, 0.125)[trial % 3],
                                   min_texels=1 + trial % 4, max_objects=(4096, 2)[trial % 2])
        pose = np.eye(4)
        pose[:3, 3] = rng.randint(-8, 9, 3) / 4.0
        if trial % 2:
            pose[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
        a = oc.shim_segment(shim, V, S, fl, pose, op, trial)
        equal(a, oc.python_segment(V, S, fl, pose, op, trial), trial)
        assert a[2]["n_components"] >= 1


def test_crafted_frames_meet_their_rules(shim):
    """the named cases give what the specification says, at 70 x 3"""
    W, H, P = 70, 3, 210
    got = {name: oc.shim_segment(shim, V, S, fl, pose, op, 0) for name, V, S, fl, pose, op in oc.crafted_cases(W, H)}
    assert got["all_flags_one_component"][2] == dict(n_texels=P, n_members=P, n_components=1, n_small=0, n_objects=1, stored=1)
    r = got["all_flags_one_component"][0][0]
    assert r["root"] == 0 and r["n_texels"] == P and r["r_min"] == np.sqrt(np.float32(64.0 + 0.75 * 0.75))   # (8, 0, -0.75), row 2 of column 0
    assert got["all_flags_zero"][2] == dict(oc.ZERO, n_texels=P) and np.all(got["all_flags_zero"][1] == oc.NONE)
    assert got["all_flags_no_link"][2]["n_components"] == P
    assert np.array_equal(got["all_flags_no_link"][0]["root"], np.arange(P))
    assert got["min_texels_above_image"][2]["n_small"] == 1 and len(got["min_texels_above_image"][0]) == 0
    assert got["serpentine"][2]["n_components"] == 1 and got["spiral"][2]["n_components"] == 1
    assert got["checkerboard"][2] == dict(n_texels=P, n_members=P // 2, n_components=1, n_small=0, n_objects=1, stored=1)
    assert got["across_the_seam"][2]["n_components"] == 1 and got["across_the_seam"][0]["n_texels"][0] == 4
    assert got["around_the_turn"][0]["n_texels"][0] == W
    assert got["flagged_non_members"][2]["n_members"] == P - 5
    assert got["pose_overflow"][2] == dict(oc.ZERO, n_texels=P)
    c = got["random_sparse"][2]
    assert c["n_objects"] > c["stored"] == 3 and set(np.unique(got["random_sparse"][1])) == {0, 1, 2, oc.NONE}
    box = got["signed_zero_box"][0][0]
    assert np.signbit(box["min"][0]) and not np.signbit(box["max"][0]) and box["min"][0] == 0 == box["max"][0]
    for near in (True, False):
        V, S, fl, pose, op = oc.threshold_case(W, H, near)
        a = oc.shim_segment(shim, V, S, fl, pose, op, 0)
        equal(a, oc.python_segment(V, S, fl, pose, op, 0), near)
        assert list(a[0]["n_texels"]) == [6, 3, 3], near
    for m in (1, 5, 9):
        V, S, fl, pose, op = oc.sized_components(W, H, m)
        a = oc.shim_segment(shim, V, S, fl, pose, op, 0)
        equal(a, oc.python_segment(V, S, fl, pose, op, 0), m)
        assert list(a[0]["n_texels"]) == [m, m + 1]


SANITIZER_MAIN = r"""
#include <stdio.h>
#include "object_shim.c"

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }

static int run(int32_t W, int32_t H, uint32_t density, uint32_t min_texels, uint32_t max_objects, float base) {
  const uint32_t P = (uint32_t)W * (uint32_t)H;
  float* V = (float*)malloc((size_t)P * 4 * sizeof(float));
  float* S = (float*)malloc((size_t)P * 4 * sizeof(float));
  uint8_t* flag = (uint8_t*)malloc(P);
  uint32_t* ids = (uint32_t*)malloc((size_t)P * sizeof(uint32_t));
  object_t* out = (object_t*)malloc((size_t)max_objects * sizeof(object_t));
  uint32_t seed = 7u * (uint32_t)W + (uint32_t)H;
  for (uint32_t t = 0; t < P; ++t) {
    V[4 * t] = 5.0f + (float)(lcg(&seed) >> 24) / 256.0f;
    V[4 * t + 1] = (float)(t % (uint32_t)W) / 8.0f;
    V[4 * t + 2] = (float)(t / (uint32_t)W) / 8.0f;
    V[4 * t + 3] = (lcg(&seed) >> 28) ? 1.0f : 0.0f;
    if ((lcg(&seed) >> 26) == 0) V[4 * t + (t % 3)] = (t & 1) ? NAN : INFINITY;
    S[4 * t] = (float)((lcg(&seed) >> 24) % 60u) / 255.0f, S[4 * t + 1] = S[4 * t + 2] = 0.0f;
    S[4 * t + 3] = (float)(lcg(&seed) >> 24) / 200.0f - 0.1f;
    flag[t] = (uint8_t)(((lcg(&seed) >> 24) % 100u) < density);
  }
  const double T[16] = {0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 2.5, -3.0, 1e39 * (W == 3), 1};
  const oparams_t op = {base, 0.03f, min_texels, max_objects};
  ocounts_t c;
  object_shim_segment(V, S, flag, W, H, T, &op, 3u, out, ids, &c);
  uint32_t with_id = 0, members = 0;
  for (uint32_t t = 0; t < P; ++t) with_id += ids[t] != 0xffffffffu;
  for (uint32_t k = 0; k < c.stored; ++k) members += out[k].n_texels;
  printf("%d x %d: members %u components %u small %u objects %u stored %u\n", W, H, c.n_members, c.n_components, c.n_small,
         c.n_objects, c.stored);
  free(V), free(S), free(flag), free(ids), free(out);
  return (c.n_small + c.n_objects == c.n_components && with_id == members && c.n_texels == P) ? 0 : 1;
}
int main(void) {
  return run(70, 3, 60, 3, 4096, 0.3f) | run(1, 9, 100, 1, 2, 0.3f) | run(2, 5, 90, 1, 1, 0.3f) | run(257, 1, 80, 2, 65536, 0.2f) |
         run(3, 3, 100, 1, 8, 0.3f) | run(64, 32, 100, 5000, 16, 1.0f);
}
"""


def test_shim_under_sanitizers(tmp_path):
    """object_shim.c with a main of its own, compiled with -fsanitize=address,undefined and run: host C only"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.call(["gcc"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0 or \
            subprocess.call([str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("the compiler cannot link the sanitizers")
    src = tmp_path / "san_main.c"
    src.write_text(SANITIZER_MAIN)
    exe = tmp_path / "san_main"
    subprocess.check_call(["gcc"] + oc.SHIM_FLAGS + flags + ["-I", oc.HERE, str(src), "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0, out.stdout.decode()
    assert out.stdout.decode().count("\n") == 6


# ---- the semantic check: DESIGN.md 15's scenario through the CPU restatement of the localiser
def host_objects(shim, tmp, without):
    """-> per scan (records, ids, counts, vertex image, flags, pose) of the shim over novel_common.host_run's frames"""
    import change_common as cc
    import localize_common as lc
    import novel_common as nc
    import novel_host as nh

    lshim, cshim, nshim = lc.build_shim(tmp), cc.build_shim(tmp), nc.build_shim(tmp)
    p, poses, records = nc.map_on_oracle(tmp, without)
    per_scan = []

    class Recording(nh.HostNovelLocalizer):
        def process_scan(self, *scan):
            r = super().process_scan(*scan)
            assert r["collected"] and r["tracked"]
            f = self.frame
            V, S = np.array(f.vertex, dtype=np.float32), np.array(f.semantic, dtype=np.float32)
            flags = (self.col.category == 5).astype(np.uint8)          # novel: what kn_collect flags
            k = len(per_scan)
            per_scan.append(oc.shim_segment(shim, V, S, flags, r["pose"], None, k) + (V, flags, np.array(r["pose"])))
            return r

    h = Recording(p, lshim, cshim, nshim)
    h.set_map(records)
    h.set_pose(poses[nc.FIRST])
    for s in nc.localise_scans():
        h.process_scan(*s)
    return per_scan


def test_the_added_building_comes_out_as_objects(shim, tmp_path):
    """Measured on this restatement with the default parameters (object_common.MEASURED): every one of the
    25 scans has an object whose centroid lies in building 41's box grown by 0.3 m; the largest such object holds at least
    0.172 of the novel texels in that box (the synthetic scan leaves every fifth column or so of the wall without a
    return, which cuts the wall into strips no link parameter can join); the control has at most 2 objects a scan."""
    import novel_common as nc
    added = host_objects(shim, tmp_path, nc.ADDED)
    assert len(added) == nc.LAST - nc.FIRST + 1
    hits, shares = 0, []
    box = oc.building_box()
    for k, (rec, ids, cnt, V, flags, pose) in enumerate(added):
        hit, share = oc.scan_measure(rec, ids, V, flags, pose)
        print("scan", nc.FIRST + k, cnt, "building", hit, share)
        hits += bool(hit)
        if hit:
            shares.append(share)
            # the hand-over a planner wants: such an object's box lies within the building's, grown by 0.3 m
            inside = oc.inside_box(rec["centroid"], box, 0.3)
            for r in rec[inside]:
                corners = np.array([[r[a][0], r[b][1], r[c][2]] for a in ("min", "max") for b in ("min", "max")
                                    for c in ("min", "max")])
                assert oc.inside_box(corners, box, 0.3).all(), (k, r)
    control = [c[2]["n_objects"] for c in host_objects(shim, tmp_path, ())]
    print("scans with the building %d, smallest share %.6f, control objects per scan %s" % (hits, min(shares), control))
    assert hits == oc.MEASURED["scans_with_building"] and abs(min(shares) - oc.MEASURED["min_share"]) < 1e-6
    assert max(control) == oc.MEASURED["control_objects"]
    oc.check_measured(hits, min(shares), max(control))
