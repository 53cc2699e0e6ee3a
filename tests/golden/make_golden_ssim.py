#!/usr/bin/env python
"""Fixture of the flow-warp SSIM term (`train.py --ssim`), from the upstream reference imported read-only from /root/reference.
Runs ONLY in the build container.

    python tests/golden/make_golden_ssim.py        # writes tests/golden/ssim.npz (a few seconds)

The term is computed by the reference's own LFLoss.__call__ with ssim=True (models/loss_function.py:105-120) on the CPU.  The
object is created without running __init__, and so is its SSIM module: both constructors need a CUDA tensor type
(loss_function.py:20, 53); `.window` is filled here by the same formula (loss_function.py:19-27).  `model_out` is hand-made:
{'rgb', 'flow': [f0, f1]} - the flows get_z produces on synthetic weights are not cycle-consistent, so upstream's masks would
switch the term off (step.npz records cycle_loss == 0 for that reason).

Case (tests/ssim_ref.case, seed 81): two 256 x 256 pairs, flows 64 x 64.  Stored: ssim_loss, the two validity masks (packed
bits, read out of the reference's own call), d ssim_loss / d f0 and / d f1 in fp32.  Data only.
"""
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import ref_shim  # noqa: E402
from tests import ssim_ref  # noqa: E402


def main():
    ref_shim.install()
    for name in ("lietorch", "lpips"):                     # imported at module level by loss_function.py, unused by this term
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["lietorch"].SE3 = None
    from models import loss_function as lf

    rgb, f0, f1 = ssim_ref.case()
    f0.requires_grad_(True)
    f1.requires_grad_(True)
    loss_fn = object.__new__(lf.LFLoss)
    loss_fn.depth = loss_fn.pose = loss_fn.cycle = False
    loss_fn.ssim = True
    loss_fn.w1, loss_fn.w2, loss_fn.w3 = 0.01, 1.0, 1.0
    ssim = object.__new__(lf.SSIM)
    torch.nn.Module.__init__(ssim)
    ssim.window_size, ssim.channel = 11, 3
    g = torch.Tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])      # loss_function.py:20-21
    g = (g / g.sum()).unsqueeze(1)
    ssim.window = g.mm(g.t()).unsqueeze(0).unsqueeze(0).expand(3, 1, 11, 11).contiguous()           # loss_function.py:24-27
    loss_fn.ssim_loss = ssim
    # the masks are locals of LFLoss.__call__: read them where the SSIM module receives them
    seen = []
    inner = lf._ssim
    lf._ssim = lambda i1, i2, w, ws, ch, mask: (seen.append(mask.detach().clone()), inner(i1, i2, w, ws, ch, mask))[1]
    B = rgb.shape[0]
    model_out = {"rgb": torch.zeros(B, 1, 4, 3), "flow": [f0, f1]}
    losses, _ = loss_fn({"context": {"rgb": rgb}}, model_out, {"rgb": torch.zeros(B, 1, 4, 3)}, ITER=0)
    lf._ssim = inner
    loss = losses["ssim_loss"]
    loss.backward()
    m0, m1 = (m[:, 0].bool() for m in seen)
    rec = {
        "ssim_loss": np.float64(loss.item()),
        "mask0": ssim_ref.pack_mask(m0), "mask1": ssim_ref.pack_mask(m1),
        "dflow0": f0.grad.numpy().astype(np.float32), "dflow1": f1.grad.numpy().astype(np.float32),
    }
    nz = [float((g != 0).float().mean()) for g in (f0.grad, f1.grad)]
    print("ssim_loss %.9f, masks %.1f %% / %.1f %% full, gradient non-zero on %.1f %% / %.1f %% of the cells"
          % (loss.item(), 100 * m0.float().mean(), 100 * m1.float().mean(), 100 * nz[0], 100 * nz[1]))
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
