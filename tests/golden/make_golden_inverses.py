#!/usr/bin/env python
"""Generate tests/golden/inter_inverses.npz: every 4x4 inverse the oracle asks LAPACK for in the `inter` case of
make_golden.py, input and result, as the upstream reference received them when inter.npz was made (float32 bits of
MKL's AVX2 / AVX-512 kernels on an Intel host; the inputs are the case's cameras, so no reference import is needed).

MKL's generic path (x86 CPUs of other vendors) rounds the inverse of one context camera differently in the last bit,
and the case's near-parallel ray intersections amplify that to 5e-2 in `pt`.  tests/test_oracle_golden.py hands the
oracle these bits, so that it judges the oracle's own arithmetic on every host.

    python tests/golden/make_golden_inverses.py        # on a host whose MKL takes its AVX2 / AVX-512 path
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from coponerf_amd import synthetic as syn  # noqa: E402
from oracle import render_ref as orc  # noqa: E402
from tests.helpers import case_inputs  # noqa: E402


def main():
    cfg = ast.literal_eval(str(np.load(os.path.join(HERE, "inter.npz"))["cfg"]))
    inp, z, rel, flow = case_inputs(cfg)
    calls, real = [], torch.inverse

    def inverse(a):
        r = real(a)
        calls.append((a.detach().clone(), r.detach().clone()))
        return r
    torch.inverse = inverse
    try:
        with torch.no_grad():
            orc.forward(inp, z, rel, flow, cfg["val"], syn.make_render_weights(), npoints=cfg["S"], keep=True)
    finally:
        torch.inverse = real
    blob = {"n": np.array(len(calls))}
    for i, (a, r) in enumerate(calls):
        blob[f"in{i}"], blob[f"out{i}"] = a.numpy(), r.numpy()
    np.savez_compressed(os.path.join(HERE, "inter_inverses.npz"), **blob)
    print("inter_inverses", len(calls), [tuple(a.shape) for a, _ in calls])


if __name__ == "__main__":
    main()
