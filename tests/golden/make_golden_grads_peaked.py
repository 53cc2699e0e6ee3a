#!/usr/bin/env python
"""Gradient fixture of the training path at SHARP attention, from the upstream reference imported read-only from
/root/reference.  Runs ONLY in the build container.

    python tests/golden/make_golden_grads_peaked.py        # writes tests/golden/grads_peaked.npz

The case of make_golden_grads.py (B=2, H=64, R=80, S=32, val=False, narrow rig, same seeds, same loss and stored fields)
with the attention sharpened as in peaked_val: key_map_2 / query_embed_2 / query_repeat_embed_2 scaled by 64
(synthetic.peaked_weights) and the latents at get_z's per-level statistics (synthetic.latents_at_getz_statistics).  The
reference's joint softmax on this case has a median largest weight of 0.88; 89 % of the rays are above 0.5.  Stored: for
each render parameter and each feature map the gradient's L2 norm, max |g| and a strided sample (every 61st element) - data
only.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import ref_shim  # noqa: E402
from coponerf_amd import synthetic as syn  # noqa: E402

CFG = dict(B=2, H=64, R=80, S=32, wseed=17, iseed=51, zseed=52, cseed=53, wtseed=54, stride=61, peak=64.0)


def main():
    c = CFG
    weights = syn.peaked_weights(syn.make_render_weights(seed=c["wseed"]), c["peak"])
    model = ref_shim.build_reference_model(weights, npoints=c["S"], H=c["H"])
    model.train()
    inp = syn.make_inputs(c["B"], c["H"], c["H"], c["R"], seed=c["iseed"])
    z, rel, flow = syn.make_latents(c["B"], c["H"], c["H"], seed=c["zseed"])
    z = syn.latents_at_getz_statistics(z)
    coef = syn.normal((c["B"], 1, c["R"], 3), seed=c["cseed"])
    cw = syn.normal((2 * c["B"], c["R"], c["S"]), seed=c["wtseed"]) * 0.3
    z = [t.clone().requires_grad_(True) for t in z]
    out = model(inp, z=z, rel_pose=rel, val=False, flow=flow)
    loss = (out["rgb"] * coef).sum() + (out["at_wt"] * cw).sum()
    loss.backward()
    wmax = out["at_wt"].detach().view(c["B"], 2, c["R"], c["S"]).permute(0, 2, 1, 3).reshape(-1, 2 * c["S"]).amax(1)
    rec = {"loss": np.float64(loss.item()), "stride": np.int64(c["stride"])}
    params = dict(model.named_parameters())
    for name in weights:
        g = params[name].grad
        assert g is not None, name
        flat = g.detach().reshape(-1)
        rec[f"{name}|norm"] = np.float64(flat.double().norm().item())
        rec[f"{name}|max"] = np.float32(flat.abs().max().item())
        rec[f"{name}|sample"] = flat[:: c["stride"]].numpy().astype(np.float32)
    for i, t in enumerate(z):
        flat = t.grad.detach().reshape(-1)
        rec[f"z{i}|norm"] = np.float64(flat.double().norm().item())
        rec[f"z{i}|max"] = np.float32(flat.abs().max().item())
        rec[f"z{i}|sample"] = flat[:: c["stride"]].numpy().astype(np.float32)
    path = os.path.join(HERE, "grads_peaked.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB, loss", loss.item(),
          "| largest softmax weight per ray: median %.3f, above 0.5: %.0f %%" % (float(wmax.median()), 100 * float((wmax > 0.5).float().mean())))


if __name__ == "__main__":
    main()
