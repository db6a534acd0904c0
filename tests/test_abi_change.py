"""C-ABI checks of the change evidence that need no GPU: the header's new symbols are exported and bound, the ctypes
mirrors have the C layouts, the defaults are as the header states, bad parameters are refused before any device exists,
and suma_change_prune_mask -- the rule's one home -- equals a numpy restatement on boundary evidence."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["suma_change_params_default", "suma_change_rule_default", "suma_localizer_enable_evidence",
       "suma_localizer_disable_evidence", "suma_localizer_observe_frame", "suma_localizer_last_observation",
       "suma_localizer_evidence", "suma_localizer_evidence_device", "suma_localizer_clear_evidence",
       "suma_change_prune_mask"]


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
    for m in ("enableEvidence", "disableEvidence", "observeFrame", "lastObservation", "evidence", "clearEvidence",
              "prunedMap"):
        assert hasattr(built.Localizer, m), m


def test_layouts_match_c(built, tmp_path):
    from semantic_suma_amd.types import (ChangeCounts, ChangeParams, ChangeRule, EVIDENCE_DTYPE, LocalizerParams,
                                         LocalizerResult)
    structs = {"suma_change_params": ChangeParams, "suma_change_counts": ChangeCounts, "suma_change_rule": ChangeRule}
    body = ['printf("%zu\\n", sizeof(suma_change_evidence));']
    body += [f'printf("%zu\\n", offsetof(suma_change_evidence, {f}));' for f in EVIDENCE_DTYPE.names]
    for cname, T in structs.items():
        body.append(f'printf("%zu\\n", sizeof({cname}));')
        body += [f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in T._fields_]
    body += ['printf("%zu\\n", sizeof(suma_localizer_params));', 'printf("%zu\\n", sizeof(suma_localizer_result));']
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "suma_hip.h"\nint main(){' + "".join(body) +
                   "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [EVIDENCE_DTYPE.itemsize] + [EVIDENCE_DTYPE.fields[f][1] for f in EVIDENCE_DTYPE.names]
    for T in structs.values():
        want += [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_]
    want += [C.sizeof(LocalizerParams), C.sizeof(LocalizerResult)]  # the localiser's own structures keep their layouts
    assert v == want
    assert EVIDENCE_DTYPE.itemsize == 16 and C.sizeof(ChangeParams) == 16 and C.sizeof(ChangeCounts) == 36
    assert C.sizeof(ChangeRule) == 8 and C.sizeof(LocalizerParams) == 16


def test_defaults(built):
    from semantic_suma_amd.types import ChangeParams, ChangeRule
    L = built.lib()
    cp = ChangeParams(9.0, 9.0, 9.0, 7)
    L.suma_change_params_default(C.byref(cp))
    assert (cp.free_margin, cp.max_range, cp.tracked_only) == (0.5, 50.0, 1) and cp.min_view_cos == C.c_float(0.3).value
    assert bytes(cp) == bytes(ChangeParams.defaults())
    rule = ChangeRule(99, 99.0)
    L.suma_change_rule_default(C.byref(rule))
    assert (rule.min_misses, rule.miss_ratio) == (3, 2.0) and bytes(rule) == bytes(ChangeRule.defaults())
    L.suma_change_params_default(None)
    L.suma_change_rule_default(None)
    assert ChangeParams.defaults(free_margin=1.5).free_margin == 1.5
    with pytest.raises(KeyError):
        ChangeParams.defaults(no_such_field=1)


def test_refusals_without_a_device(built):
    """nothing here reaches a device: a NULL localiser, and the prune mask's NULL arrays"""
    from semantic_suma_amd.types import ChangeParams
    L = built.lib()
    cp = ChangeParams.defaults(free_margin=float("nan"))
    assert L.suma_localizer_enable_evidence(None, C.byref(cp)) == -1
    assert L.suma_localizer_disable_evidence(None) == -1 and L.suma_localizer_clear_evidence(None) == -1
    assert L.suma_localizer_observe_frame(None, None, None, None) == -1
    assert L.suma_localizer_last_observation(None, None, None) == -1
    n = C.c_uint32(7)
    assert L.suma_localizer_evidence(None, None, 0, C.byref(n)) == -1 and n.value == 7
    assert L.suma_localizer_evidence_device(None, None, 0, C.byref(n)) == -1
    keep = np.ones(4, dtype=np.uint8)
    assert L.suma_change_prune_mask(None, 4, None, keep.ctypes.data, None) == -1
    assert "NULL array" in L.suma_last_error(None).decode()
    assert L.suma_change_prune_mask(None, 0, None, None, C.byref(n)) == 0 and n.value == 0


def boundary_evidence(rule):
    """every combination of misses around min_misses and hits around misses / miss_ratio, the exact tie included"""
    from semantic_suma_amd.types import EVIDENCE_DTYPE
    mm, ratio = int(rule.min_misses), float(rule.miss_ratio)
    rows = []
    for misses in sorted({min(m, 0xffffffff) for m in (0, 1, max(mm, 1) - 1, mm, mm + 1, 2 * mm, 2 * mm + 1, 7, 8, 64, 1 << 24,
                                                        (1 << 24) + 1, 0xffffffff)}):
        ties = [] if not np.isfinite(ratio) or ratio <= 0 else [int(misses / ratio)]
        for hits in sorted({0, 1, 2, 3, 4, misses, 0xffffffff} | {max(t + d, 0) for t in ties for d in (-1, 0, 1)}):
            rows.append((min(hits, 0xffffffff), misses))
    ev = np.zeros(len(rows), dtype=EVIDENCE_DTYPE)
    ev["hits"], ev["misses"] = [r[0] for r in rows], [r[1] for r in rows]
    ev["occluded"] = np.arange(len(rows)) * 7          # reported, and do not enter the rule
    ev["label_changes"] = ev["hits"] // 2
    return ev


def test_prune_mask_equals_numpy(built, tmp_path):
    import change_common as cc
    from semantic_suma_amd.types import ChangeRule, EVIDENCE_DTYPE
    shim = cc.build_shim(tmp_path)
    rules = [None, ChangeRule.defaults(), ChangeRule(1, 0.0), ChangeRule(0, 1.0), ChangeRule(5, 0.5), ChangeRule(3, 3.0),
             ChangeRule(3, float("inf")), ChangeRule(3, float("nan")), ChangeRule(3, -1.0), ChangeRule(0xffffffff, 2.0)]
    for rule in rules:
        ev = boundary_evidence(ChangeRule.defaults() if rule is None else rule)
        want = cc.numpy_prune(ev, rule)
        got = built.prune_mask(ev, rule)
        assert got.dtype == bool and np.array_equal(got, want), rule and (rule.min_misses, rule.miss_ratio)
        assert np.array_equal(cc.shim_prune(shim, ev, rule), want)
        removed = C.c_uint32(0)
        keep = np.full(len(ev), 9, dtype=np.uint8)
        assert built.lib().suma_change_prune_mask(ev.ctypes.data, len(ev), None if rule is None else C.byref(rule),
                                                  keep.ctypes.data, C.byref(removed)) == 0
        assert removed.value == int((~want).sum()) and set(np.unique(keep)) <= {0, 1}
    # the named boundaries with the default rule (3, 2.0): one miss short, exactly enough, and the exact tie
    ev = np.zeros(5, dtype=EVIDENCE_DTYPE)
    ev["misses"], ev["hits"] = [2, 3, 4, 4, 5], [0, 0, 2, 1, 2]
    assert built.prune_mask(ev).tolist() == [True, False, True, False, False]
    records = np.arange(5)
    kept, keep = built.pruned_map(records, ev)
    assert kept.tolist() == [0, 2] and keep.tolist() == [True, False, True, False, False]
    with pytest.raises(ValueError):
        built.pruned_map(records[:4], ev)
    assert built.prune_mask(np.zeros(0, dtype=EVIDENCE_DTYPE)).shape == (0,)
