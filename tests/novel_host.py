"""The localiser with change evidence and the collection of newly seen surfaces over the CPU oracle:
tests/change_host.py's HostChangeLocalizer, which ends every scan as csrc/suma_localize.hip does -- after the observation,
one collection (tests/novel_shim.c) of the scan's own frame at the final pose, unless the window is empty, tracked_only &&
!tracked, or the pose is not finite; the scan's number counts from 0 at every set_map whether or not it collected.  The
library must equal it to the byte."""
import numpy as np

import change_common as cc
import change_host as ch
import novel_common as nc
from semantic_suma_amd.types import NOVEL_COUNTS, NovelFuseParams, NovelParams


class HostNovelLocalizer(ch.HostChangeLocalizer):
    def __init__(self, params, shim, change_shim, novel_shim, loc_params=None, change_params=None,
                 novel_params: NovelParams = None, threads: int = 8):
        super().__init__(params, shim, change_shim, loc_params, change_params, threads)
        self.col = nc.ShimCollector(novel_shim, params, novel_params)
        self.scan_count = 0
        self.last_collection = (dict.fromkeys(NOVEL_COUNTS, 0), False)

    def set_map(self, records):
        dropped = super().set_map(records)
        self.col.clear()
        self.scan_count = 0
        self.last_collection = (dict.fromkeys(NOVEL_COUNTS, 0), False)
        return dropped

    def collect_frame(self, maps, T, scan_id):
        win = cc.window_sources(self.map, self.origin[0], self.origin[1], self.p.submap_dimension) if self.have_pose \
            else np.zeros(0, dtype=np.uint32)
        assert len(win) == self.n_window
        return self.col.collect(self.map.records, win, maps, T, scan_id)

    def process_scan(self, points, labels, probs, fixed_iterations=0):
        r = super().process_scan(points, labels, probs, fixed_iterations)
        scan_id = self.scan_count
        self.scan_count += 1
        if self.n_window and (r["tracked"] or not self.col.np.tracked_only) and np.all(np.isfinite(r["pose"])):
            f = self.frame
            self.last_collection = (self.collect_frame((f.vertex, f.normal, f.semantic), r["pose"], scan_id), True)
        else:
            self.last_collection = (dict.fromkeys(NOVEL_COUNTS, 0), False)
        r["collection"], r["collected"] = self.last_collection
        return r

    def candidates(self):
        return self.col.candidates()

    def novel(self, fuse_params: NovelFuseParams = None):
        return self.col.fuse(fuse_params)

    def updated_map(self, records, rule=None, fuse_params=None):
        """the records the prune rule keeps, then the fused novel records"""
        keep = cc.shim_prune(self.cshim, self.evidence, rule)
        return np.concatenate([np.asarray(records)[keep], self.novel(fuse_params)[0]])
