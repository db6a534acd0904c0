#!/usr/bin/env python
"""Generates tests/golden/se3_log_200.npz: SE3::log of the reference's lie_algebra.cpp (oracle/_ref, compiled by
oracle/ref_build.py where the reference's sources exist) on the 200 poses of
tests/test_pipeline_phases.py::test_se3_log_is_the_reference_function, so that the test needs no oracle/_ref.
Run from the repo root:  python tests/golden/make_se3_log_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyoracle, pyref  # noqa: E402

assert pyref.available(), "oracle/_ref not built (python oracle/ref_build.py)"
pyoracle.build()
rng = np.random.default_rng(5)
Ts = []
for k in range(200):
    x = rng.uniform(-1, 1, 6) * (1e-6 if k % 10 == 0 else 1.0)
    x[3:] *= 0.5 if k % 3 else 3.0
    Ts.append(pyoracle.se3_exp(x))
T = np.stack(Ts)
path = os.path.join(ROOT, "tests", "golden", "se3_log_200.npz")
np.savez_compressed(path, T=T, log=np.stack([pyref.se3_log(t) for t in T]))
print(f"{path}: {os.path.getsize(path) // 1024} KB")
