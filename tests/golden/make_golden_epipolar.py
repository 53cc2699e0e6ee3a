#!/usr/bin/env python
"""Fixture of the epipolar geometry, from the upstream reference imported read-only from /root/reference.  Runs ONLY in the
build container.

    python tests/golden/make_golden_epipolar.py [OUT.npz]     # writes tests/golden/epipolar_F.npz (a second)

Calls the reference's own summary/inspect_epipolar_geometry.py:two_view_geometry the way inspect() does (K1 = the intrinsics of
context view 1, K2 = those of view 0) on four synthetic pairs (tests/epipolar_ref.golden_inputs: coponerf_amd.synthetic's wide
rig).  `cv2` is ref_shim's empty stand-in, as in make_golden_summaries.py: two_view_geometry is numpy only.  Stored: the inputs
and the E, F, E_gt, F_gt it returns.  Data only.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import ref_shim  # noqa: E402
from tests import epipolar_ref as er  # noqa: E402


def compute():
    ref_shim.install()
    from summary import inspect_epipolar_geometry as ref
    K, rel, gt = er.golden_inputs()
    E, F, _, E_gt, F_gt, _ = ref.two_view_geometry(K[:, 1], K[:, 0], rel, gt)
    return {"intrinsics": K.numpy(), "rel_pose": rel.numpy(), "gt_rel_pose": gt.numpy(), "E": np.asarray(E, dtype=np.float64),
            "F": np.asarray(F, dtype=np.float64), "E_gt": np.asarray(E_gt, dtype=np.float64), "F_gt": np.asarray(F_gt, dtype=np.float64)}


def main():
    out = compute()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "epipolar_F.npz")
    np.savez_compressed(path, **out)
    for k, v in out.items():
        print("%-12s %-14s %s" % (k, v.shape, v.dtype))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
