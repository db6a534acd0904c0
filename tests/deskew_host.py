"""The pipeline and the localiser with motion compensation on, over the CPU oracle: the shim's correction
(tests/deskew_shim.c) with the previous scan's increment as the motion, then OraclePipeline.process_scan /
HostLocalizer.process_scan -- the same order as csrc/suma_api.hip (pipeline_begin_scan_impl) and
csrc/suma_localize.hip, so that the library must equal it to the bit.  Precedent: localize_host.py."""
import numpy as np

import deskew_common as dc
import localize_host as lh
import novel_host as nh
from oracle import pyoracle
from semantic_suma_amd.types import DESKEW_MOTION_INCREMENT, DESKEW_MOTION_NONE, DESKEW_MOTION_OVERRIDE, DeskewParams


class _Switch:
    """suma_*_enable_deskew / _disable_deskew / _set_deskew_motion / _deskew_motion"""

    def _init_switch(self, shim):
        self.dk_shim, self.dk_on, self.dk_params = shim, False, None
        self.dk_override, self.dk_last, self.dk_source = None, np.eye(4), DESKEW_MOTION_NONE

    def enable_deskew(self, dp: DeskewParams = None):
        self.dk_on, self.dk_params = True, DeskewParams.defaults() if dp is None else dp

    def disable_deskew(self):
        self.dk_on, self.dk_override = False, None

    def set_deskew_motion(self, motion):
        assert self.dk_on
        self.dk_override = np.asarray(motion, dtype=np.float64).copy()

    def deskew_motion(self):
        return self.dk_last.copy(), self.dk_source

    def _corrected(self, points, increment):
        if not self.dk_on:
            return points
        motion, self.dk_source = (increment, DESKEW_MOTION_INCREMENT) if self.dk_override is None else \
            (self.dk_override, DESKEW_MOTION_OVERRIDE)
        self.dk_last, self.dk_override = np.asarray(motion, dtype=np.float64).copy(), None
        return dc.shim_points(self.dk_shim, points, self.dk_last, self.dk_params)


class HostPipeline(_Switch):
    def __init__(self, params, shim, threads: int = 8):
        pyoracle.build()
        self.op = pyoracle.OraclePipeline(params, threads=threads)
        self._init_switch(shim)

    def process_scan(self, points, labels, probs, fixed_iterations=0):
        self.op.process_scan(self._corrected(points, self.op.last_increment()), labels, probs, fixed_iterations)

    def pose(self):
        return self.op.pose().copy()

    def last_increment(self):
        return self.op.last_increment().copy()

    def stats(self):
        return self.op.last_stats().as_dict()

    def frame_maps(self, which):
        f = self.op.frame(which)
        return [f.map(m).copy() for m in range(3)]


class HostLocalizer(lh.HostLocalizer, _Switch):
    def __init__(self, params, shim, deskew_shim, loc_params=None, threads: int = 8):
        lh.HostLocalizer.__init__(self, params, shim, loc_params, threads)
        self._init_switch(deskew_shim)

    def process_scan(self, points, labels, probs, fixed_iterations=0):
        # the increment of the previous scan's step 7; the identity after set_pose
        return lh.HostLocalizer.process_scan(self, self._corrected(points, self.increment), labels, probs, fixed_iterations)


class HostMaintLocalizer(nh.HostNovelLocalizer, _Switch):
    """the same over the localiser with change evidence and novelty: both read the frame the localiser holds, which is
    made from the corrected points"""

    def __init__(self, params, shim, change_shim, novel_shim, deskew_shim, **kw):
        nh.HostNovelLocalizer.__init__(self, params, shim, change_shim, novel_shim, **kw)
        self._init_switch(deskew_shim)

    def process_scan(self, points, labels, probs, fixed_iterations=0):
        return nh.HostNovelLocalizer.process_scan(self, self._corrected(points, self.increment), labels, probs,
                                                  fixed_iterations)
