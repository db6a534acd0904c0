"""The localiser with change evidence over the CPU oracle: tests/localize_host.py's HostLocalizer, which ends every
scan as csrc/suma_localize.hip does -- with one observation (tests/change_shim.c) of the scan's own frame at the final
pose, unless the window is empty or tracked_only && !tracked.  The library must equal it to the byte."""
import numpy as np

import change_common as cc
import localize_host as lh
from semantic_suma_amd.types import ChangeParams, EVIDENCE_DTYPE


class HostChangeLocalizer(lh.HostLocalizer):
    def __init__(self, params, shim, change_shim, loc_params=None, change_params: ChangeParams = None, threads: int = 8):
        super().__init__(params, shim, loc_params, threads)
        self.cshim = change_shim
        self.cp = ChangeParams.defaults() if change_params is None else change_params
        self.evidence = None
        self.last = (None, False)

    def set_map(self, records):
        dropped = super().set_map(records)
        self.evidence = np.zeros(len(self.map.records), dtype=EVIDENCE_DTYPE)
        self.last = (None, False)
        return dropped

    def clear_evidence(self):
        self.evidence[...] = np.zeros((), dtype=EVIDENCE_DTYPE)

    def observe_frame(self, maps, T):
        """maps = (vertex, normal, semantic) of a data-sized frame"""
        win = cc.window_sources(self.map, self.origin[0], self.origin[1], self.p.submap_dimension) if self.have_pose \
            else np.zeros(0, dtype=np.uint32)
        assert len(win) == self.n_window
        return cc.shim_observe(self.cshim, self.map.records, win, maps, self.p, T, self.cp, self.evidence)

    def process_scan(self, points, labels, probs, fixed_iterations=0):
        r = super().process_scan(points, labels, probs, fixed_iterations)
        zero = dict.fromkeys(cc.CATEGORIES + ("label_changes",), 0)
        if self.n_window and (r["tracked"] or not self.cp.tracked_only) and np.all(np.isfinite(r["pose"])):
            f = self.frame
            self.last = (self.observe_frame((f.vertex, f.normal, f.semantic), r["pose"]), True)
        else:
            self.last = (zero, False)
        r["observation"], r["observed"] = self.last
        return r
