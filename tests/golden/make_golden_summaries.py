#!/usr/bin/env python
"""Fixture of the validation log, from the upstream reference imported read-only from /root/reference.  Runs ONLY in the
build container.

    python tests/golden/make_golden_summaries.py        # writes tests/golden/summaries.npz (a few seconds)

Runs the reference's own summary/summaries.py:img_summaries on the CPU with a recording writer.  Besides ref_shim's stand-ins,
three inert ones are installed here, because the libraries are not available: `torchvision.utils.make_grid` returns its input
unchanged and records the `normalize` / `scale_each` it was given (the grid's rules are pinned by tests/test_summaries_ref.py
instead); `cv2.findContours` finds nothing and `cv2.drawContours` draws nothing, so overlay_semantic_mask leaves out its
1-pixel contour; and with the otherwise empty `cv2`, inspect() returns (None, None) through its own `except`, so the two
epipolar images are not written.

Case (tests/summaries_ref.inputs, seed 97): two 256 x 256 pairs, flows 64 x 64.  The inputs are pure functions of seeds and are
not stored.  Stored: every scalar; per image tag its shape, the two grid flags, the minimum and maximum of the batch and of
every image, and the values at a seeded sample of 16 384 element positions (summaries_ref.positions).  Data only.
"""
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
from tests import summaries_ref as sr  # noqa: E402


class Recorder:
    def __init__(self, flags):
        self.flags, self.images, self.scalars = flags, {}, {}

    def add_image(self, tag, img, step):
        self.images[tag] = (np.asarray(img), self.flags.pop())

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = float(value)


def main():
    ref_shim.install()
    flags = []

    def make_grid(tensor, normalize=False, scale_each=False, **kw):
        assert not kw, kw                                   # nrow, padding, pad_value stay at torchvision's defaults
        flags.append((bool(normalize), bool(scale_each)))
        return tensor

    tv = sys.modules["torchvision"]
    tv.utils = types.ModuleType("torchvision.utils")
    tv.utils.make_grid = make_grid
    sys.modules["torchvision.utils"] = tv.utils
    cv2 = sys.modules["cv2"]
    cv2.RETR_TREE = cv2.CHAIN_APPROX_SIMPLE = 0
    cv2.findContours = lambda *a, **k: ([], None)
    cv2.drawContours = lambda *a, **k: None
    from summary import summaries as ref
    import matplotlib

    # the closed form the product builds its table from is matplotlib's own (integers index the lookup table directly)
    lut = matplotlib.colormaps["jet"](np.arange(256))[:, :3]
    assert np.abs(lut - sr.jet_table()).max() < 1e-15, np.abs(lut - sr.jet_table()).max()

    model_input, model_output = sr.inputs()
    S = sr.FIXTURE["S"]
    rec = Recorder(flags)
    with torch.no_grad():
        ref.img_summaries(None, model_input, None, None, model_output, rec, 0, img_shape=(S, S))
    assert not flags and sorted(rec.images) == sorted(sr.IMAGE_TAGS), sorted(rec.images)
    out = {"scalar_" + k: np.float64(v) for k, v in rec.scalars.items()}
    for tag, (img, (normalize, scale_each)) in rec.images.items():
        assert img.dtype == np.float32 and img.ndim == 4, (tag, img.dtype, img.shape)
        out[tag + "_shape"] = np.array(img.shape, dtype=np.int64)
        out[tag + "_flags"] = np.array([normalize, scale_each])
        out[tag + "_range"] = np.array([img.min(), img.max()], dtype=np.float32)
        out[tag + "_range_each"] = np.stack([img.min(axis=(1, 2, 3)), img.max(axis=(1, 2, 3))], -1).astype(np.float32)
        out[tag + "_values"] = img.reshape(-1)[sr.positions(tag, img.size)]
        print("%-24s %-18s normalize %d scale_each %d  range %.4f .. %.4f" % (tag, img.shape, normalize, scale_each, img.min(), img.max()))
    for k, v in rec.scalars.items():
        print("%-28s %.9g" % (k, v))
    path = os.path.join(HERE, "summaries.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
