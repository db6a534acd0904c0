"""The semantic front end on the host: known answers of its arithmetic specification as restated in
tests/semantic_shim.c (which the GPU tests compare the kernels of csrc/k_semantic.hip with, bit for bit), the layout of
suma_semantic_params in C and ctypes, and kitti.read_velodyne_raw."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from semantic_suma_amd import kitti
from semantic_suma_amd.types import SEM_CHANNELS, SEM_MAX_CLASSES, SemanticParams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_shim(out_dir):
    so = os.path.join(str(out_dir), "semantic_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(HERE, "semantic_shim.c"), "-o", so, "-lm"])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("semantic"))


def make_params(width=2048, height=64, fov_up=3.0, fov_down=-25.0, means=(12.1, 10.9, 0.2, -1.0, 0.2),
                stds=(12.3, 11.6, 9.0, 0.8, 0.15), n_classes=20, label_map=None):
    sp = SemanticParams(width=width, height=height, fov_up=fov_up, fov_down=fov_down, n_classes=n_classes)
    for c in range(SEM_CHANNELS):
        sp.means[c], sp.stds[c] = means[c], stds[c]
    lm = [kitti.LEARNING_MAP_INV[j] for j in range(20)] if label_map is None else label_map
    for j, v in enumerate(lm):
        sp.label_map[j] = v
    return sp


def project(shim, sp, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
    P = sp.width * sp.height
    inp = np.empty((SEM_CHANNELS, sp.height, sp.width), dtype=np.float32)
    pixel = np.empty(pts.shape[0], dtype=np.int32)
    proj_idx = np.empty((sp.height, sp.width), dtype=np.int32)
    shim.sem_project(C.byref(sp), pts.ctypes.data_as(C.c_void_p), C.c_uint32(pts.shape[0]),
                     inp.ctypes.data_as(C.c_void_p), pixel.ctypes.data_as(C.c_void_p),
                     proj_idx.ctypes.data_as(C.c_void_p))
    assert P == proj_idx.size
    return inp, pixel, proj_idx


def unproject(shim, sp, scores, pixel, logits=False):
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    pixel = np.ascontiguousarray(pixel, dtype=np.int32)
    labels = np.empty(pixel.size, dtype=np.float32)
    probs = np.empty(pixel.size, dtype=np.float32)
    shim.sem_unproject(C.byref(sp), scores.ctypes.data_as(C.c_void_p), C.c_int(int(logits)),
                       pixel.ctypes.data_as(C.c_void_p), C.c_uint32(pixel.size), labels.ctypes.data_as(C.c_void_p),
                       probs.ctypes.data_as(C.c_void_p))
    return labels, probs


def test_point_straight_ahead_lands_in_the_middle_column(shim):
    sp = make_params()
    _, pixel, proj_idx = project(shim, sp, [[10.0, 0.0, 0.0, 0.5]])
    row = math.floor((1.0 - 25.0 / 28.0) * 64)  # pitch 0: v = (1 - |fov_down| / fov) H = 6.86
    assert row == 6
    assert pixel[0] == row * 2048 + 1024
    assert proj_idx[row, 1024] == 0 and (proj_idx >= 0).sum() == 1


def test_yaw_runs_right_to_left_and_row_zero_is_the_top(shim):
    sp = make_params(width=8, height=4)
    # +y (yaw = -pi/2) is a quarter of the width left of the centre; just above fov_up clamps to row 0
    up = math.tan(math.radians(4.0))
    _, pixel, _ = project(shim, sp, [[0.0, 10.0, 0.0, 0.0], [0.0, -10.0, 0.0, 0.0], [10.0, 0.0, 10.0 * up, 0.0]])
    assert pixel[0] % 8 == 2 and pixel[1] % 8 == 6
    assert pixel[2] // 8 == 0


def test_points_outside_the_fov_clamp_to_the_first_and_last_row(shim):
    sp = make_params(width=64, height=16)
    pts = [[10.0, 0.0, 10.0, 0.0],    # 45 degrees up: far above fov_up
           [10.0, 0.0, -10.0, 0.0],   # 45 degrees down: below fov_down
           [0.0, 0.0, 5.0, 0.0],      # straight up
           [0.0, 0.0, -5.0, 0.0],     # straight down
           [-10.0, -1e-3, 0.0, 0.0],  # yaw just below +pi: the last column
           [-10.0, -0.0, 0.0, 0.0]]   # sdm_atan2 does not see the sign of a zero: yaw = -pi, the first column
    _, pixel, _ = project(shim, sp, pts)
    assert pixel[0] // 64 == 0 and pixel[2] // 64 == 0
    assert pixel[1] // 64 == 15 and pixel[3] // 64 == 15
    assert pixel[4] % 64 == 63 and pixel[5] % 64 == 0
    assert (pixel >= 0).all() and (pixel < 64 * 16).all()


def test_nearest_wins_and_equal_ranges_go_to_the_lowest_index(shim):
    sp = make_params(width=32, height=8)
    pts = [[10.0, 0.0, 0.0, 0.1],   # 0: far
           [5.0, 0.0, 0.0, 0.2],    # 1: nearer, same pixel -> wins
           [5.0, 0.0, 0.0, 0.3],    # 2: same range as 1 -> loses to the lower index
           [-5.0, 0.0, 0.0, 0.4],   # 3: behind, its own pixel
           [-5.0, 0.0, 0.0, 0.5]]   # 4: same as 3
    inp, pixel, proj_idx = project(shim, sp, pts)
    assert pixel[0] == pixel[1] == pixel[2] and pixel[3] == pixel[4] != pixel[0]
    flat = proj_idx.ravel()
    assert flat[pixel[0]] == 1 and flat[pixel[3]] == 3
    # the winner's remission, normalised
    r = inp[4].ravel()[pixel[0]]
    assert r == np.float32((np.float32(0.2) - np.float32(0.2)) * np.float32(1.0 / 0.15))
    rng_plane = inp[0].ravel()
    assert rng_plane[pixel[0]] == (np.float32(5.0) - np.float32(12.1)) * np.float32(1.0 / 12.3)


def test_empty_pixels_are_zero_in_every_channel_and_bad_points_are_not_projected(shim):
    sp = make_params(width=64, height=16)
    pts = np.array([[10.0, 1.0, 0.5, 0.3], [0.0, 0.0, 0.0, 0.3], [np.nan, 1.0, 1.0, 0.3], [np.inf, 0.0, 0.0, 0.3],
                    [3e20, 3e20, 0.0, 0.3], [-4.0, 2.0, -1.5, 0.7]], dtype=np.float32)
    inp, pixel, proj_idx = project(shim, sp, pts)
    assert pixel[1] == pixel[2] == pixel[3] == pixel[4] == -1  # zero range, NaN, inf, range overflows fp32
    assert pixel[0] >= 0 and pixel[5] >= 0
    empty = proj_idx < 0
    assert empty.sum() == 64 * 16 - 2
    assert (inp[:, empty] == 0.0).all()  # not -mean / std
    assert (inp[:, ~empty] != 0.0).all()


def test_argmax_rule_of_the_reference(shim):
    C_ = 4
    sp = make_params(width=4, height=1, n_classes=C_, label_map=[7, 11, 13, 17])
    nan = np.nan
    # one pixel per case; scores planar [C, 1, 4]
    cases = np.array([[0.2, 0.5, 0.5, 0.1],       # last maximum wins -> class 2
                      [-0.1, -2.0, -0.5, -0.3],   # all negative -> (0, 0)
                      [nan, 0.3, nan, 0.1],       # NaN never wins -> class 1
                      [0.0, 0.0, 0.0, 0.0]],      # all zero: prob <= 0 holds every time -> the LAST class, prob 0
                     dtype=np.float32)
    scores = np.ascontiguousarray(cases.T.reshape(C_, 1, 4))
    pixel = np.array([0, 1, 2, 3, -1, 4], dtype=np.int32)  # -1: not projected; 4: outside the image
    labels, probs = unproject(shim, sp, scores, pixel)
    assert labels.tolist() == [13.0, 0.0, 11.0, 17.0, 0.0, 0.0]
    assert probs.tolist() == [np.float32(0.5), 0.0, np.float32(0.3), 0.0, 0.0, 0.0]


def test_logits_mode_is_a_softmax_then_the_same_rule(shim):
    sp = make_params(width=16, height=8, n_classes=20)
    rng = np.random.default_rng(3)
    logits = rng.normal(0.0, 3.0, (20, 8, 16)).astype(np.float32)
    pixel = np.arange(128, dtype=np.int32)
    labels, probs = unproject(shim, sp, logits, pixel, logits=True)
    x = logits.reshape(20, -1).astype(np.float64)
    p = np.exp(x - x.max(0)) / np.exp(x - x.max(0)).sum(0)
    assert np.allclose(probs, p.max(0), rtol=1e-5)
    lm = np.array([kitti.LEARNING_MAP_INV[j] for j in range(20)], dtype=np.float32)
    assert np.array_equal(labels, lm[p.argmax(0)])
    # a NaN logit makes the whole softmax NaN: no class wins
    logits[5, 0, 0] = np.nan
    labels, probs = unproject(shim, sp, logits, pixel[:1], logits=True)
    assert labels[0] == 0.0 and probs[0] == 0.0


def test_semantic_params_layout_matches_c(shim):
    out = (C.c_uint64 * 9)()
    shim.sem_layout(out)
    fields = ["width", "height", "fov_up", "fov_down", "means", "stds", "n_classes", "label_map"]
    assert out[0] == C.sizeof(SemanticParams) == 4 * (4 + 2 * SEM_CHANNELS + 1 + SEM_MAX_CLASSES)
    assert list(out[1:]) == [getattr(SemanticParams, f).offset for f in fields]


def test_read_velodyne_raw_keeps_remission(tmp_path):
    pts = np.array([[1.0, 2.0, 3.0, 0.25], [4.0, 5.0, 6.0, 0.75]], dtype="<f4")
    f = tmp_path / "000000.bin"
    pts.tofile(f)
    raw = kitti.read_velodyne_raw(str(f))
    assert raw.dtype == np.float32 and np.array_equal(raw, pts)
    assert kitti.read_velodyne(str(f))[:, 3].tolist() == [1.0, 1.0]  # unchanged: rv::Point3f (x, y, z, 1)
    (tmp_path / "bad.bin").write_bytes(b"\0" * 12)
    with pytest.raises(ValueError):
        kitti.read_velodyne_raw(str(tmp_path / "bad.bin"))
