"""coponerf_amd.evaluate.image_metrics (csrc/image_metrics.hip) and pose_metrics on the MI355X against the float64 restatement
of tests/metrics_ref.py (`pytest -m gpu`).

Bars, each against float64 on the same fp32 inputs:
  ssim   |d| <= 5e-5: half a unit of the fourth decimal the evaluation prints; an indexing, weight, crop or reflection mistake
         moves these small images by more than 1e-3.  On the flat and bright cases, where fp32 itself costs 2e-5 .. 6e-5 in
         `E[x^2] - E[x]^2`, the bar is max(5e-5, 2 x |straight fp32 - float64|) of that case, computed here.
  mse    relative 1e-6: fp32 per-sample terms, fixed-order fp32 partials per 16 x 32 tile, float64 finish:
         (3 + log2(16 * 32 * 3)) * 2^-24 = 8e-7.
  psnr   1e-5 dB: the mse bar through 10 / ln 10 (4.3e-6 dB) plus the fp32 rounding of a value below 64 dB (1.9e-6).
Every case prints its distances (and those of straight fp32) before it asserts; DESIGN.md §4.8 quotes them.
"""
import functools

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu

SSIM_BAR, MSE_REL, PSNR_DB = 5e-5, 1e-6, 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(name, N, H, W):
    """Inputs and float64 results of one case, computed once and shared (read-only)."""
    pred, target = mr.make_case(name, N, H, W)
    mse = mr.mse64(pred, target)
    ref = {"pred": pred, "target": target, "mse": mse, "psnr": mr.psnr64(mse), "ssim": mr.ssim64(pred, target),
           "ssim32": mr.ssim32_straight(pred, target)}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def run(pred, target, dev, image_shape=None):
    from coponerf_amd.evaluate import image_metrics
    out = image_metrics(torch.from_numpy(np.ascontiguousarray(pred)).to(dev), torch.from_numpy(np.ascontiguousarray(target)).to(dev),
                        image_shape)
    return out.cpu()


@pytest.mark.parametrize("cid,name,N,H,W", mr.cases(), ids=[c[0] for c in mr.cases()])
def test_image_metrics_against_float64(cid, name, N, H, W, dev):
    ref = reference(name, N, H, W)
    got = run(ref["pred"], ref["target"], dev).double().numpy()
    assert got.shape == (N, 3)
    d_ssim = np.abs(got[:, 2] - ref["ssim"])
    d_32 = np.abs(ref["ssim32"] - ref["ssim"])
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_mse = np.where(ref["mse"] == 0, np.abs(got[:, 0]), np.abs(got[:, 0] - ref["mse"]) / ref["mse"])
        d_psnr = np.where(np.isinf(ref["psnr"]), np.where(got[:, 1] == ref["psnr"], 0.0, np.inf), np.abs(got[:, 1] - ref["psnr"]))
    print(f"{cid}: ssim64 {ref['ssim'].round(6).tolist()} |kernel - f64| {d_ssim.max():.2e} (straight fp32: {d_32.max():.2e})  "
          f"mse rel {rel_mse.max():.2e}  psnr {d_psnr.max():.2e} dB")
    bar = np.maximum(SSIM_BAR, 2 * d_32) if name in ("flat", "bright") else np.full(N, SSIM_BAR)
    assert np.all(d_ssim <= bar), (d_ssim, bar)
    assert np.all(rel_mse <= MSE_REL), rel_mse
    assert np.all(d_psnr <= PSNR_DB), d_psnr
    if name == "identical":
        assert np.all(got[:, 2] == 1.0) and np.all(got[:, 0] == 0.0) and np.all(np.isposinf(got[:, 1]))


def test_nan_stays_in_its_image(dev):
    ref = reference("textured", 3, 41, 75)
    clean = run(ref["pred"], ref["target"], dev)
    pred = ref["pred"].copy()
    pred[1, 20, 33, 2] = np.nan
    got = run(pred, ref["target"], dev)
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])
    # a NaN in a corner still reaches the cropped map (through the window of pixel (5, 5)) and the squared error
    pred = ref["pred"].copy()
    pred[1, 0, 0, 0] = np.nan
    assert bool(torch.isnan(run(pred, ref["target"], dev)[1]).all())


@pytest.mark.parametrize("name,H,W", [("textured", 41, 75), ("out_of_range", 64, 48)])
def test_bit_reproducible_and_independent_of_batch(name, H, W, dev):
    ref = reference(name, 3, H, W) if (3, H, W) in mr.SHAPES else None
    pred, target = (ref["pred"], ref["target"]) if ref else mr.make_case(name, 3, H, W)
    a, b = run(pred, target, dev), run(pred, target, dev)
    assert torch.equal(a, b)
    singles = torch.cat([run(pred[n:n + 1], target[n:n + 1], dev) for n in range(3)])
    assert torch.equal(a, singles)
    # the (B, 1, H*W, 3) view that forward(val=True)['rgb'] holds is the same memory
    flat = run(pred.reshape(3, 1, H * W, 3), target.reshape(3, 1, H * W, 3), dev, image_shape=(H, W))
    assert torch.equal(a, flat)


def test_rejected_inputs(dev):
    from coponerf_amd import _hip
    from coponerf_amd.evaluate import image_metrics
    x = torch.zeros(1, 16, 16, 3, device=dev)
    with pytest.raises(ValueError, match="11"):
        image_metrics(torch.zeros(1, 10, 16, 3, device=dev), torch.zeros(1, 10, 16, 3, device=dev))
    with pytest.raises(ValueError, match="11"):
        image_metrics(torch.zeros(1, 16, 10, 3, device=dev), torch.zeros(1, 16, 10, 3, device=dev))
    # the library itself refuses it too, as a status (skimage raises for a window larger than the image)
    out, part = torch.zeros(1, 3, device=dev), torch.zeros(64, device=dev)
    small = torch.zeros(1, 10, 16, 3, device=dev)
    with pytest.raises(RuntimeError, match="cpn_image_metrics"):
        _hip.call("cpn_image_metrics", small.data_ptr(), small.data_ptr(), 1, 10, 16, part.data_ptr(), out.data_ptr(), 0)
    assert _hip.lib().cpn_image_metrics_scratch(1, 10, 16) == 0
    assert _hip.lib().cpn_image_metrics_scratch(2, 41, 75) == 2 * 3 * 3 * 2
    with pytest.raises(ValueError, match="fp32"):
        image_metrics(x.half(), x.half())
    with pytest.raises(ValueError, match="fp32"):
        image_metrics(x, x.double())
    with pytest.raises(ValueError, match="contiguous"):
        image_metrics(torch.zeros(1, 3, 16, 16, device=dev).permute(0, 2, 3, 1), x)
    with pytest.raises(ValueError, match="contiguous"):
        image_metrics(x, torch.zeros(1, 16, 32, 3, device=dev)[:, :, ::2])
    with pytest.raises(ValueError):
        image_metrics(x, torch.zeros(2, 16, 16, 3, device=dev))
    with pytest.raises(ValueError, match="image_shape"):
        image_metrics(x.view(1, 256, 3), x.view(1, 256, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        image_metrics(x.cpu(), x.cpu())


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis /= np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def _poses(angles, t_pred, t_gt):
    B = len(angles)
    rel, gt = np.tile(np.eye(4), (B, 1, 1)), np.tile(np.eye(4), (B, 1, 1))
    for b, a in enumerate(angles):
        base = _rot([0.3, -0.5 + 0.2 * b, 0.8], 0.4 + 0.3 * b)
        gt[b, :3, :3] = base
        rel[b, :3, :3] = _rot([1.0 - 0.3 * b, 0.2, 0.1 * b - 0.4], a) @ base
        rel[b, :3, 3], gt[b, :3, 3] = t_pred[b], t_gt[b]
    return rel.astype(np.float32), gt.astype(np.float32)


def test_pose_metrics_against_float64(dev):
    from coponerf_amd.evaluate import pose_metrics
    angles = [0.05, 0.3, 1.2, 2.5, 3.0]
    t_gt = np.array([[0.3, 0.0, 0.1], [-0.2, 0.4, 1.0], [1.5, -0.5, 0.2], [0.0, 0.0, 2.0], [0.7, 0.7, -0.1]])
    t_pred = np.stack([_rot([0.1, 1.0, 0.2], a) @ t * s for a, t, s in zip([0.1, 0.4, 1.0, 2.5, 3.0], t_gt, [1.0, 1.1, 0.7, 1.0, 2.0])])
    rel, gt = _poses(angles, t_pred, t_gt)
    want = mr.pose64(rel, gt)
    got = pose_metrics(torch.from_numpy(rel).to(dev), torch.from_numpy(gt).to(dev)).cpu().double().numpy()
    assert got.shape == (5, 3)
    d = np.abs(got - want)
    print(f"rot {want[:, 0].round(4).tolist()} |d| {d[:, 0].max():.2e}; angle {want[:, 2].round(4).tolist()} |d| {d[:, 2].max():.2e}; "
          f"trans rel {(d[:, 1] / want[:, 1]).max():.2e}")
    assert np.all(want[:, 0] >= 0.05 - 1e-6) and np.all(want[:, 2] >= 0.05) and np.all(want[:, [0, 2]] <= 3.05)
    assert np.all(np.abs(want[:, 0] - np.array(angles)) <= 1e-5)            # radians, whatever the reference calls it
    assert np.all(d[:, 0] <= 1e-5) and np.all(d[:, 2] <= 1e-5)
    assert np.all(d[:, 1] <= 1e-6 * want[:, 1])


def test_identical_poses_are_clamped_not_nan(dev):
    from coponerf_amd.evaluate import pose_metrics
    t = np.array([[0.3, 0.0, 0.1], [-0.2, 0.4, 1.0], [1.5, -0.5, 0.2]])
    rel, _ = _poses([0.7, 1.9, 3.0], t, t)
    p = torch.from_numpy(rel).to(dev)
    got = pose_metrics(p, p.clone()).cpu()
    assert bool(torch.isfinite(got).all())
    assert bool((got[:, 0] <= 1e-3).all()) and bool((got[:, 2] <= 1e-3).all()) and bool((got[:, 1] == 0).all())
