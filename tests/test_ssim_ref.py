"""The yardsticks of the flow-warp SSIM tests hold against upstream's own numbers, without a GPU: tests/ssim_ref.py's float64
reference, fed the fp32 coordinates ATen computes on the CPU (what upstream ran), against tests/golden/ssim.npz; and the
stock-op terms of coponerf_amd.losses against the restatement the step fixtures were checked with (tests/step_case.py).

Bars: loss to 2^-22; each dflow to a relative L2 of 2^-18 = 64 fp32 roundings of 2^-24, the count on one pixel's path (two
11-term window sums per moment, the quotient, the adjoint sums, the taps).  Measured: 4.3e-7, a tenth of that."""
import os

import numpy as np
import pytest
import torch

from coponerf_amd import _hip, losses
from tests import ssim_ref as R
from tests import step_case as sc
from tests.helpers import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "ssim.npz"))


@pytest.fixture(scope="module")
def case():
    return R.case()


def test_case_masks_are_upstreams(fx, case):
    rgb, f0, f1 = case
    B, _, H, W, _ = rgb.shape
    for d, m in enumerate(R.masks_of(f0, f1, H, W)):
        assert torch.equal(m, R.unpack_mask(fx[f"mask{d}"], (B, H, W)))
        assert 0.5 < float(m.float().mean()) < 0.9


def test_float64_reference_at_lifted_coordinates_matches_upstream(fx, case):
    rgb, f0, f1 = case
    B, _, H, W, _ = rgb.shape
    total = 0.0
    for d, f in enumerate((f0, f1)):
        mask = R.unpack_mask(fx[f"mask{d}"], (B, H, W))
        coords = R.unnormalised_coords(R.upsample(f, H, W))                 # fp32, ATen on the CPU: what upstream sampled at
        loss, g = R.ref64_loss(rgb, f, mask, d, coords)
        total += float(loss) / 2
        want = 2 * torch.from_numpy(fx[f"dflow{d}"]).double()               # the fixture differentiates (L0 + L1) / 2
        e = R.rel_l2(g, want)
        print(f"d{d}: loss {float(loss):.9f}, dflow relL2 {e:.2e}, worst {R.rel_max(g, want):.2e}")
        assert e <= 2.0 ** -18
        assert float((want != 0).double().mean()) > 0.9
    print(f"ssim_loss {total:.9f} vs upstream {float(fx['ssim_loss']):.9f}")
    assert abs(total - float(fx["ssim_loss"])) <= 2.0 ** -22


def test_stock_composition_is_upstreams_on_the_cpu(fx, case):
    """The fp32 yardstick the GPU test measures its gap with is the computation the fixture recorded."""
    rgb, f0, f1 = case
    B, _, H, W, _ = rgb.shape
    total = 0.0
    for d, f in enumerate((f0, f1)):
        leaf = f.clone().requires_grad_(True)
        loss = R.stock_loss(rgb, leaf, R.unpack_mask(fx[f"mask{d}"], (B, H, W)), d)
        g, = torch.autograd.grad(loss, leaf)
        total += float(loss.detach()) / 2
        assert R.rel_l2(g, 2 * torch.from_numpy(fx[f"dflow{d}"])) <= 2.0 ** -18
    assert abs(total - float(fx["ssim_loss"])) <= 2.0 ** -22


def test_loss_config_defaults():
    cfg = losses.LossConfig()
    assert (cfg.cycle, cfg.pose, cfg.ssim) == (False, False, False)
    assert losses.LossConfig(ssim=True) != cfg and losses.LossConfig() == cfg
    import inspect
    from coponerf_amd.train_step import TrainStep
    assert inspect.signature(TrainStep.__init__).parameters["loss"].default == cfg
    assert torch.equal(losses.gaussian_window(), R.window1d())


def _hand_made_out(seed=5):
    from coponerf_amd import synthetic as syn
    B, Rn = 2, 37
    t1 = syn.uniform((B, Rn, 2), seed, 0.0, 255.0, stream=1)
    off = syn.normal((B, Rn, 2), seed, std=8.0, stream=2)                    # some pairs beyond the 20 px validity radius
    rel = torch.eye(4).repeat(B, 1, 1)
    gt = torch.eye(4).repeat(B, 1, 1)
    ang = syn.uniform((B,), seed, -0.2, 0.2, stream=3)
    rel[:, 0, 0], rel[:, 0, 2], rel[:, 2, 0], rel[:, 2, 2] = ang.cos(), ang.sin(), -ang.sin(), ang.cos()
    rel[:, :3, 3] = syn.normal((B, 3), seed, std=0.3, stream=4)
    gt[:, :3, 3] = syn.normal((B, 3), seed, std=0.3, stream=5)
    return {
        "rgb": syn.uniform((B, 1, Rn, 3), seed, -1.0, 1.0, stream=6).requires_grad_(True),
        "T_to_C1_pts": t1.requires_grad_(True), "C2_pts_to_C1": (t1.detach() + off).requires_grad_(True),
        "mask_c2": syn.uniform((B, Rn), seed, stream=7) > 0.2, "matchability_cycle_mask": syn.uniform((B, Rn), seed, stream=8) > 0.3,
        "rel_pose": rel.requires_grad_(True), "gt_rel_pose": gt,
    }


def test_cycle_and_pose_terms_match_the_step_fixtures_restatement():
    out = _hand_made_out()
    gt = torch.zeros_like(out["rgb"]).detach() + 0.25
    want = sc.loss_terms("full", out, gt)
    got = losses.loss_terms(losses.LossConfig(cycle=True, pose=True), {}, out, gt)
    assert set(got) == set(want) == {"img_loss", "cycle_loss", "pose_loss"}
    assert float(want["cycle_loss"]) > 0 and float(want["pose_loss"]) > 0
    leaves = [out[k] for k in ("rgb", "T_to_C1_pts", "C2_pts_to_C1", "rel_pose")]
    for name in want:
        assert torch.equal(got[name], want[name]), name
        for a, b in zip(torch.autograd.grad(got[name], leaves, allow_unused=True, retain_graph=True),
                        torch.autograd.grad(want[name], leaves, allow_unused=True, retain_graph=True)):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), name
    only_img = losses.loss_terms(losses.LossConfig(), {}, out, gt)
    assert list(only_img) == ["img_loss"]
    nan_gt = gt.clone()
    nan_gt[0, 0, 0, 0] = float("nan")                                       # loss_function.py:66-69: NaNs count as zero
    assert torch.isfinite(losses.loss_terms(losses.LossConfig(), {}, out, nan_gt)["img_loss"])


def test_new_symbols_are_declared_and_exported():
    names = {"cpn_ssim_warp", "cpn_ssim_warp_bwd", "cpn_ssim_warp_blocks"}
    assert names <= set(_hip.declared_symbols()) and names <= set(_hip.SIGNATURES)
    lib = _hip.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.cpn_ssim_warp_blocks(256, 256) == 16 * 8 and lib.cpn_ssim_warp_blocks(8, 12) == 1
    # pointer and shape checks come before any launch (no GPU here)
    assert lib.cpn_ssim_warp(*([None] * 5), 1, 8, 8, 8, 8, *([None] * 7)) == -1 and b"null" in lib.cpn_last_error()
    assert lib.cpn_ssim_warp(*([16] * 5), 1, 48, 48, 16, 16, *([16] * 6), None) == -2 and b"scale 3" in lib.cpn_last_error()
    assert lib.cpn_ssim_warp(*([16] * 5), 1, 48, 64, 24, 16, *([16] * 6), None) == -2
    assert lib.cpn_ssim_warp_bwd(*([16] * 6), 1, 48, 48, 3, 3, 16, 16, None) == -2 and b"scale 16" in lib.cpn_last_error()
    assert lib.cpn_ssim_warp_bwd(*([16] * 6), 1, 48, 48, 24, 24, None, 16, None) == -1


def test_ssim_term_needs_the_device():
    rgb, f0, f1 = R.case(1, 8, 12, 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        losses.ssim_warp_loss(rgb, f0, f1, torch.ones(1, 2, 8, 12, dtype=torch.bool))
