"""The tracks' specification on the host (tests/track_shim.c, the yardstick of test_gpu_tracks*.py): the shim -- a flood
fill and two loops a round -- against a plain Python statement of every rule -- breadth-first search, a sort of all gated
pairs taken greedily, sums in Python integers -- on the named cases and on random sequences; what the named cases must
give by the specification; the detections in reverse input order; the shim under the address and undefined-behaviour
sanitizers as a stand-alone program; and the semantic check without a GPU: DESIGN.md 19's scenario through the CPU
restatement of the localiser, segmented by tests/object_shim.c and tracked by the shim with the default parameters."""
import subprocess

import numpy as np
import pytest

import track_common as tc
from semantic_suma_amd.types import TrackParams

NONE = tc.NONE


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return tc.build_shim(tmp_path_factory.mktemp("track_host"))


@pytest.fixture(scope="module")
def named(shim):
    """name -> (params, steps, the shim's result per update, the shim tracker afterwards)"""
    out = {}
    for name, tp, steps in tc.named_cases():
        t = tc.ShimTracker(shim, tp)
        out[name] = (tp, steps, tc.run(t, steps), t)
    return out


def test_shim_equals_python_on_the_named_cases(shim, named):
    for name, (tp, steps, got, tracker) in named.items():
        if name.startswith("count_") and int(name.split("_")[1]) > 65 and int(name.split("_")[3]) not in (2, 1024):
            continue                      # the plain statement is slow on thousands of objects: two table sizes of each
        py = tc.PyTracker(tp)
        try:
            want = tc.run(py, steps)
        except tc.CapReached as e:
            assert name in ("line_rounds_one_below", "line_rounds_one") and e.args[0] == 40, name
            continue
        for u, (a, b) in enumerate(zip(got, want)):
            tc.same(a, b, (name, u))
            if a is not None:
                tc.check_counts(a[2], tp, len(a[0]))
                assert a[3].tobytes() == b[3].tobytes(), (name, u)
        assert tracker.slots.tobytes() == py.slots.tobytes(), name
        assert (tracker.last_stamp, tracker.next_id) == (py.last_stamp, py.next_id), name


@pytest.mark.parametrize("n_objects", [0, 1, 5, 70, 300])
def test_shim_equals_python_on_random_sequences(shim, n_objects):
    for seed in range(3):
        tp, steps = tc.random_sequence(seed + 10 * n_objects, n_objects)
        a, b = tc.ShimTracker(shim, tp), tc.PyTracker(tp)
        for u, (x, y) in enumerate(zip(tc.run(a, steps), tc.run(b, steps))):
            tc.same(x, y, (n_objects, seed, u))
            tc.check_counts(x[2], tp, len(x[0]))
        assert a.slots.tobytes() == b.slots.tobytes() and (a.last_stamp, a.next_id) == (b.last_stamp, b.next_id)


def test_named_cases_meet_their_rules(named):
    """what the specification says of each"""
    def res(name, u=-1):
        return named[name][2][u]

    for n in (0, 1, 63, 64, 65, 1025, 4096):
        for T in (1, 2, 64, 65, 1024):
            first, second, third = named["count_%d_tracks_%d" % (n, T)][2]
            kept = min(n, T)
            assert first[2]["n_born"] == kept and first[2]["n_dropped"] == n - kept and len(first[0]) == kept, (n, T)
            assert list(first[0]["id"]) == list(range(1, kept + 1)) and list(first[0]["slot"]) == list(range(kept))
            # the same things 0.25 m on, in reverse order: the kept ones are matched, the rest dropped again
            assert second[2]["n_matched"] == kept and second[2]["n_born"] == 0 and second[2]["rounds"] == (1 if kept else 0), (n, T)
            assert np.array_equal(second[1][::-1][:kept], np.arange(1, kept + 1)) and not second[1][::-1][kept:].any()
            assert third[2]["n_matched"] == min(n // 2, T) and third[2]["n_missed"] == kept - min(n // 2, T)
    # ties
    t, ot, c, _ = res("two_detections_one_track")
    assert c["n_matched"] == 1 and t[0]["detection"] == 0 and list(ot) == [1, 2, 3]
    t, ot, c, _ = res("two_tracks_one_detection")
    assert c["n_matched"] == 1 and c["n_missed"] == 1 and t[0]["detection"] == 0 and t[1]["detection"] == NONE and list(ot) == [1]
    for gap in (1, 3):
        assert res("gate_at_gap_%d" % gap)[2]["n_matched"] == 1 and res("gate_beyond_gap_%d" % gap)[2]["n_matched"] == 0
        assert res("gate_beyond_gap_%d" % gap)[2]["n_born"] == 1
    # the line: one pair a round
    c = res("line_rounds_need")[2]
    assert c["n_matched"] == 40 and c["rounds"] == 40 and c["n_unresolved"] == 0
    assert list(res("line_rounds_need")[0]["detection"][:40]) == list(range(40))
    c = res("line_rounds_one_below")[2]
    assert c["n_matched"] == 39 and c["rounds"] == 39 and c["n_unresolved"] == 1 and c["n_born"] == 1
    c = res("line_rounds_one")[2]
    assert c["n_matched"] == 1 and c["rounds"] == 1 and c["n_unresolved"] == 39 and c["n_born"] == 24 and c["n_dropped"] == 15
    assert res("line_rounds_one")[0]["detection"][39] == 39
    # capacity
    t, ot, c, _ = res("births_exceed_free_slots")
    assert c["n_matched"] == 2 and c["n_born"] == 1 and c["n_dropped"] == 4 and list(ot) == [1, 2, 3, 0, 0, 0, 0] and len(t) == 3
    # a slot freed and taken again in one update; ids are not reused
    got = named["slot_reused_same_update"][2]
    assert got[1][2]["n_expired"] == 2 and got[1][2]["n_born"] == 2 and got[1][2]["n_dropped"] == 1
    assert list(got[1][0]["id"]) == [3, 4] and list(got[1][0]["slot"]) == [0, 1] and list(got[1][1]) == [3, 4, 0]
    assert list(got[2][0]["id"]) == [3] and list(got[3][0]["id"]) == [3, 5] and list(got[3][0]["slot"]) == [0, 1]
    for mm in (0, 1, 3):
        got = named["expiry_at_max_missed_%d" % mm][2]
        assert [g[2]["n_expired"] for g in got] == [0] * (mm + 1) + [1, 0] and len(got[mm][0]) == 1 and len(got[mm + 1][0]) == 0
        assert got[-1][0]["id"][0] == 2
        got = named["rematch_at_max_missed_%d" % mm][2]
        assert got[mm][0]["missed"][0] == mm and got[mm + 1][2]["n_matched"] == 1 and got[mm + 1][0]["id"][0] == 1
        assert got[mm + 1][0]["missed"][0] == 0
    for ch in (1, 2, 3):
        got = named["confirm_hits_%d" % ch][2]
        assert [int(g[0]["state"][0]) for g in got] == [2 if k + 1 >= ch else 1 for k in range(4)], ch
        assert [g[2]["n_confirmed"] for g in got] == [1 if k + 1 >= ch else 0 for k in range(4)]
    for dt in (1, 4):
        got = named["velocity_rules_dt_%d" % dt][2]
        f = np.float32
        assert np.array_equal(got[1][0]["position"][0], f([0.75, 0.5, -0.25]))
        v1 = f([0.75, 0.5, -0.25]) / f(dt)
        assert np.array_equal(got[1][0]["velocity"][0], v1)
        pred = f([0.75, 0.5, -0.25]) + v1 * f(dt)
        r = f([1.75, 1.0, 0.0]) - pred
        assert np.array_equal(got[2][0]["position"][0], pred + f(0.5) * r)
        assert np.array_equal(got[2][0]["velocity"][0], v1 + (f(0.2) / f(dt)) * r)
        assert got[2][0]["hits"][0] == 3 and np.array_equal(got[2][0]["origin"][0], f([0, 0, 0]))
    got = named["hits_saturate"][2]
    assert list(got[0][0]["hits"]) == [65535, 65535] and list(got[1][0]["hits"]) == [65535, 65535]
    got = named["non_finite_tracks"][2]
    assert got[0][2]["n_matched"] == 1 and got[0][2]["n_missed"] == 4 and got[0][2]["n_born"] == 1
    assert got[1][2]["n_expired"] == 4 and sorted(got[2][0]["id"]) == [5, 6]
    # joining
    for u in (0, 1):
        t, ot, c, od = res("join_chain_300", u)
        assert c["n_detections"] == 1 and c["n_joined"] == 299 and t[0]["n_objects"] == 300 and not od.any()
        assert t[0]["min"][0] == 0 and t[0]["max"][0] == 299.5 and t[0]["n_texels"] == 3000
    t, ot, c, od = res("join_gap_at_and_beyond")
    assert list(od) == [0, 0, 1, 2] and c["n_joined"] == 1
    assert list(res("join_touching_dist_0")[3]) == [0, 0, 1]
    assert list(res("join_equal_boxes_other_labels")[3]) == [0, 1, 0]
    assert list(res("join_off")[3]) == [0, 1, 2, 3, 4]
    t, ot, c, od = res("join_4096_in_one")
    assert c["n_detections"] == 1 and c["n_matched"] == 1 and t[0]["n_objects"] == 4096 and (ot == 1).all()
    assert t[0]["n_texels"] == sum(1 + k % 7 for k in range(4096)) and t[0]["n_dynamic"] == sum(k % 3 for k in range(4096))
    t = res("join_signed_zero_box")[0][0]
    assert np.signbit(t["min"]).all() and not np.signbit(t["max"]).any() and t["n_objects"] == 3
    t, ot, c, od = res("join_non_finite_boxes")
    assert list(od) == [0, 1, 2, 0, 0] and c["n_detections"] == 3
    # the stamp rule
    got = named["stamp_refusals"][2]
    assert [g is None for g in got] == [False, True, True, True, False]
    assert got[4][2]["n_matched"] == 1 and got[4][0]["id"][0] == 1 and named["stamp_refusals"][3].last_stamp == 6


def test_reversed_input_gives_the_same_tracks(shim):
    """the objects of every update in reverse order: detections are renumbered by their smallest object, which the reversal
    turns round per update; a second pair of runs over well separated detections, where no tie is broken by an index and
    every birth order is set to agree, must give the same tracks but for the detection numbers"""
    rng = np.random.RandomState(5)
    base = np.stack([np.arange(40) * 8.0, rng.randint(0, 64, 40) / 8.0, np.zeros(40)], axis=1)
    a, b = tc.ShimTracker(shim), tc.ShimTracker(shim)
    # the first update founds the tracks in input order: give both runs the same state, then reverse the inputs
    first = tc.points(base)
    a.update(first, 0), b.update(first, 0)
    for u in range(1, 6):
        pts = base + u * np.array([0.25, 0.0, 0.0]) + rng.randint(-2, 3, base.shape) / 16.0
        halves = tc.objects([(10, p - 0.25, p + np.array([0.0, 0.25, 0.25]), p - 0.125) for p in pts] +
                            [(10, p - np.array([0.0, 0.25, 0.25]), p + 0.25, p + 0.125) for p in pts])  # two fragments each
        keep = rng.rand(80) < 0.9
        keep[:40] |= ~keep[40:]                       # at least one fragment of each stays: no births
        rec = halves[keep]
        x, y = a.update(rec, u), b.update(rec[::-1].copy(), u)
        n = x[2]["n_detections"]
        assert x[2] == y[2] and x[2]["n_born"] == 0 and x[2]["n_joined"] == len(rec) - 40
        assert np.array_equal(x[1], y[1][::-1])                       # per object the same track
        ya = y[0].copy()
        # expected renumbering: detection d of the forward run is the one whose smallest object is i; in the reversed run
        # that detection's smallest object is len - 1 - (its largest forward object)
        largest = {int(d): int(np.nonzero(x[3] == d)[0].max()) for d in range(n)}
        order = sorted(range(n), key=lambda d: len(rec) - 1 - largest[d])
        renumber = {d: k for k, d in enumerate(order)}
        assert [renumber[int(d)] for d in x[0]["detection"]] == [int(d) for d in ya["detection"]]
        ya["detection"] = x[0]["detection"]
        assert ya.tobytes() == x[0].tobytes(), u


def test_shim_under_sanitizers(tmp_path):
    """track_shim.c with its own main (-DTRACK_SHIM_MAIN), compiled with -fsanitize=address,undefined and run: host C only"""
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.call(["gcc"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0 or \
            subprocess.call([str(tmp_path / "probe")], stderr=subprocess.DEVNULL) != 0:
        pytest.skip("the compiler cannot link the sanitizers")
    exe = tmp_path / "san_main"
    subprocess.check_call(["gcc"] + tc.SHIM_FLAGS + flags + ["-DTRACK_SHIM_MAIN", tc.HERE + "/track_shim.c", "-o", str(exe), "-lm"])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().startswith("track_shim ok"), out.stdout.decode()


# ---- the semantic check: DESIGN.md 19's scenario, segmented by object_shim.c, tracked by track_shim.c
def host_tracks(shim, tmp, without, tp=None):
    import novel_common as nc
    import object_common as oc
    import test_objects_host as toh
    per_scan = [s[0] for s in toh.host_objects(oc.build_shim(tmp), tmp, without)]
    t = tc.ShimTracker(shim, tp)
    return tc.scenario_measure(per_scan, nc.FIRST, t.update), per_scan


def test_the_moving_car_keeps_its_track(shim, tmp_path):
    """Measured on this restatement with the default parameters (track_common.MEASURED)."""
    import novel_common as nc
    m, _ = host_tracks(shim, tmp_path, nc.ADDED)
    control, _ = host_tracks(shim, tmp_path, ())
    print("added:", m)
    print("control:", control)
    M = tc.MEASURED
    assert m["cube_track_scans"] == M["cube_track_scans"] and m["cube_ids"] == M["cube_ids"]
    assert abs(m["net_error"] - M["net_error"]) < 1e-6 and abs(m["velocity_error"] - M["velocity_error"]) < 1e-6
    assert abs(m["still_speed"] - M["still_speed"]) < 1e-6 and control["max_confirmed"] == M["control_confirmed"]
    tc.check_measured(m["cube_track_scans"], m["cube_ids"], m["net_error"], m["velocity_error"], m["still_speed"],
                      control["max_confirmed"], m["net_velocity"])
