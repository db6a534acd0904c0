"""C-ABI checks of the collection of newly seen surfaces that need no GPU: the header's new symbols are exported and
bound, the ctypes mirrors have the C layouts, the defaults are as the header states, NULL handles are refused before any
device exists, and the fusion of the host restatement (tests/novel_shim.c) equals a plain numpy restatement on crafted
candidates."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_novel_params_default", "suma_novel_fuse_params_default", "suma_localizer_enable_novelty",
       "suma_localizer_disable_novelty", "suma_localizer_collect_frame", "suma_localizer_last_collection",
       "suma_localizer_novel_candidates", "suma_localizer_novel_candidates_device", "suma_localizer_set_novel_candidates",
       "suma_localizer_novel", "suma_localizer_novel_device", "suma_localizer_novel_marks", "suma_localizer_clear_novelty"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from semantic_suma_amd import core
    return core


def test_new_symbols_are_declared_and_exported(built):
    L = C.CDLL(built.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "suma_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(L, name), name
        assert hasattr(built.lib(), name) and getattr(built.lib(), name).argtypes is not None, name
    for m in ("enableNovelty", "disableNovelty", "collectFrame", "lastCollection", "novelCandidates", "novel",
              "clearNovelty", "updatedMap"):
        assert hasattr(built.Localizer, m), m
    adapter = open(os.path.join(ROOT, "include", "suma_adapter.hpp")).read()
    for m in ("enableNovelty", "novel(", "updatedMap("):
        assert m in adapter, m


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import (LocalizerParams, LocalizerResult, NOVEL_COUNTS, NovelCounts, NovelFuseParams,
                                         NovelParams, NovelStats, WORLD_SURFEL_DTYPE)
    structs = {"suma_novel_params": NovelParams, "suma_novel_fuse_params": NovelFuseParams,
               "suma_novel_counts": NovelCounts, "suma_novel_stats": NovelStats}
    body = []
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    body += ['printf("%zu\\n", sizeof(suma_localizer_params));', 'printf("%zu\\n", sizeof(suma_localizer_result));',
             'printf("%zu\\n", sizeof(suma_world_surfel));']
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = []
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    want += [C.sizeof(LocalizerParams), C.sizeof(LocalizerResult), WORLD_SURFEL_DTYPE.itemsize]
    assert v == want
    assert C.sizeof(NovelParams) == 16 and C.sizeof(NovelFuseParams) == 12 and C.sizeof(NovelCounts) == 28
    assert C.sizeof(NovelStats) == 20 and C.sizeof(LocalizerParams) == 16
    assert NOVEL_COUNTS == ("n_texels", "no_return", "out_of_range", "grazing", "explained", "novel", "stored")


def test_defaults(built):
    from semantic_suma_amd.types import NovelFuseParams, NovelParams, default_params
    L = built.lib()
    q = NovelParams(9.0, 9.0, 7, 7)
    L.suma_novel_params_default(C.byref(q))
    assert (q.agree_margin, q.max_range, q.tracked_only, q.max_candidates) == (0.5, 50.0, 1, 4194304)
    assert q.max_candidates * 48 == 201326592  # the header's 201 MB
    assert bytes(q) == bytes(NovelParams.defaults())
    p = default_params()
    for thr in (0.0, 2.5, -1.25):
        p.confidence_threshold = thr
        fp = NovelFuseParams(9.0, 9, 9.0)
        L.suma_novel_fuse_params_default(C.byref(p), C.byref(fp))
        assert fp.voxel_size == C.c_float(0.2).value and fp.min_views == 2 and fp.confidence == thr + 1.0
        assert bytes(fp) == bytes(NovelFuseParams.defaults(p))
    fp = NovelFuseParams(9.0, 9, 9.0)
    L.suma_novel_fuse_params_default(None, C.byref(fp))
    assert fp.confidence == 1.0 and bytes(fp) == bytes(NovelFuseParams.defaults())
    L.suma_novel_params_default(None)
    L.suma_novel_fuse_params_default(None, None)
    assert NovelParams.defaults(agree_margin=1.5).agree_margin == 1.5
    with pytest.raises(KeyError):
        NovelParams.defaults(no_such_field=1)
    with pytest.raises(KeyError):
        NovelFuseParams.defaults(None, no_such_field=1)


def test_refusals_without_a_device(built):
    """nothing here reaches a device: a NULL localiser"""
    L = built.lib()
    n = C.c_uint32(7)
    assert L.suma_localizer_enable_novelty(None, None) == -1 and L.suma_localizer_disable_novelty(None) == -1
    assert L.suma_localizer_collect_frame(None, None, None, 0, None) == -1
    assert L.suma_localizer_last_collection(None, None, None) == -1
    assert L.suma_localizer_novel_candidates(None, None, 0, C.byref(n)) == -1 and n.value == 7
    assert L.suma_localizer_novel_candidates_device(None, None, 0, C.byref(n)) == -1
    assert L.suma_localizer_set_novel_candidates(None, None, 0) == -1
    assert L.suma_localizer_novel(None, None, None, None, 0, None) == -1
    assert L.suma_localizer_novel_device(None, None, None, None, 0, None) == -1
    assert L.suma_localizer_novel_marks(None, None, 0, C.byref(n)) == -1
    assert L.suma_localizer_clear_novelty(None) == -1


@pytest.fixture(scope="module")
def nshim(tmp_path_factory):
    import novel_common as nc
    return nc.build_shim(tmp_path_factory.mktemp("novel_abi"))


def test_shim_fusion_equals_numpy(nshim):
    import novel_common as nc
    from semantic_suma_amd.types import NovelFuseParams
    cand, names = nc.crafted_candidates()
    sets = [cand, cand[:0], cand[:1], cand[:2], cand[::-1].copy(), nc.random_candidates(600)]
    for fp in (NovelFuseParams(0.2, 2, 1.0), NovelFuseParams(0.2, 1, -3.5), NovelFuseParams(0.2, 3, 1.0),
               NovelFuseParams(0.5, 2, 1.0), NovelFuseParams(0.2, 4, 1.0)):
        for c in sets:
            a, b = nc.shim_fuse(nshim, c, fp), nc.numpy_fuse(c, fp)
            assert a[2] == b[2], (fp.voxel_size, fp.min_views, len(c), a[2], b[2])
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            assert len(a[0]) == 0 or (np.all(a[1] >= fp.min_views) and np.all(a[0]["confidence"] == np.float32(fp.confidence)))


def test_crafted_candidates_meet_their_rules(nshim):
    """every named group gives what the specification says, at voxel_size 0.2 and min_views 2"""
    import novel_common as nc
    from semantic_suma_amd.types import NovelFuseParams
    f32 = np.float32
    cand, names = nc.crafted_candidates()
    rec, views, st = nc.shim_fuse(nshim, cand, NovelFuseParams(0.2, 2, 1.0))
    assert st == dict(n_dropped=6, n_voxels=15, n_out=13)

    def voxel(name):
        x, y, z = names[name]
        k = np.nonzero((np.floor(rec["x"] / f32(0.2)) == np.floor(f32(x + 0.02) / f32(0.2))) &
                       (np.floor(rec["y"] / f32(0.2)) == np.floor(f32(y + 0.05) / f32(0.2))))[0]
        assert len(k) <= 1, name
        return (rec[k[0]], int(views[k[0]])) if len(k) else None

    r, v = voxel("radius_tie")           # two members of radius 0.125: the one created first
    first = min(i for i in range(len(cand)) if cand["radius"][i] == f32(0.125) and abs(cand["x"][i] - 1.0) < 0.2)
    assert r["radius"] == f32(0.125) and r["x"] == cand["x"][first] and v == 3 and r["support"] == 3 and r["timestamp"] == 2
    assert voxel("radius_nan")[0]["radius"] == f32(0.5)
    assert np.isnan(voxel("radius_all_nan")[0]["radius"])
    r, v = voxel("vote_tie")             # 0.5 for label 9 against 0.25 + 0.25 for label 3: the smaller id
    assert r["label"] == 3 and r["prob"] == f32(0.5)
    r, v = voxel("vote_weights")
    assert r["label"] == 9 and 0.53 < r["prob"] < 0.54
    r, v = voxel("vote_all_zero")        # no weight at all: the representative's label, prob 0
    assert r["label"] == 7 and r["prob"] == 0 and r["radius"] == f32(0.1)
    assert voxel("prob_nan")[0]["label"] == 7 and voxel("prob_nan")[0]["prob"] == 1.0
    assert voxel("prob_above_one")[0]["label"] == 7   # 7.0 counts as 1.0 against 0.75 + 0.75
    assert voxel("label_300")[0]["label"] == 0        # a label beyond 259 votes as 0
    assert voxel("views_one_short") is None and voxel("single") is None
    assert voxel("views_enough")[1] == 2
    r, v = voxel("three_scans")
    assert v == 3 and r["support"] == 4 and r["timestamp"] == 9
    assert voxel("stamps_not_in_order")[1] == 2
    assert voxel("edge_inside") is not None and voxel("edge_positive") is None
    assert np.all(np.isfinite(rec["x"])) and np.all(np.diff(views.astype(np.int64)) > -99)
    # one view is enough with min_views = 1: every voxel comes out
    assert nc.shim_fuse(nshim, cand, NovelFuseParams(0.2, 1, 1.0))[2]["n_out"] == 15
