"""The host side of the LPIPS training term: shards.BatchAssembler(lpips=True) draws what the reference's loaders draw
(data/realestate10k_dataio.py:364-385), losses.patch_from_rays rebuilds a patch from rays in any order, and LossConfig gains a
weight that defaults to 0."""
import types

import numpy as np
import pytest
import torch

from coponerf_amd import losses, shards

HS, WS, SIDE, PATCH = 64, 80, 64, 32
CPU = torch.device("cpu")


def scene(n=4, seed=5):
    rng = np.random.default_rng(seed)
    c2w = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    intr = np.tile(np.array([0.5, 0.89, 0.5, 0.5], dtype=np.float64), (n, 1))
    return types.SimpleNamespace(frames=rng.integers(0, 256, size=(n, HS, WS, 3), dtype=np.uint8), c2w=c2w, intrinsics=intr)


def test_both_branches_as_the_reference_draws_them():
    sh = scene()
    asm = shards.BatchAssembler(1, HS, WS, PATCH * PATCH, CPU, lpips=True)
    assert asm.side == SIDE
    rng, twin = np.random.default_rng(17), np.random.default_rng(17)
    seen = {0: 0, 1: 0}
    for _ in range(64):
        asm.fill(0, sh, (0, 1, 2), rng)
        pix = asm.ray_pix[0].numpy().astype(np.int64)
        bit = int(twin.integers(0, 2))                                  # one bit first
        assert int(asm.mask[0]) == bit
        seen[bit] += 1
        if bit:
            x0, y0 = int(twin.integers(0, SIDE - PATCH)), int(twin.integers(0, SIDE - PATCH))
            assert 0 <= x0 < SIDE - PATCH and 0 <= y0 < SIDE - PATCH
            ys, xs = (pix // SIDE).reshape(PATCH, PATCH), (pix % SIDE).reshape(PATCH, PATCH)
            assert np.array_equal(ys, np.broadcast_to(y0 + np.arange(PATCH)[:, None], (PATCH, PATCH)))      # row-major
            assert np.array_equal(xs, np.broadcast_to(x0 + np.arange(PATCH)[None, :], (PATCH, PATCH)))
            assert ys.max() < SIDE and xs.max() < SIDE                  # inside the crop
        else:
            assert np.array_equal(pix, twin.permutation(SIDE * SIDE)[:PATCH * PATCH])
            assert len(np.unique(pix)) == PATCH * PATCH and pix.min() >= 0 and pix.max() < SIDE * SIDE
    assert seen[0] >= 16 and seen[1] >= 16
    assert asm.mask.dtype == torch.int64 and tuple(asm.mask.shape) == (1,) and not asm.mask.is_cuda


def test_ray_count_must_be_the_patch():
    with pytest.raises(ValueError, match="patch"):
        shards.BatchAssembler(1, HS, WS, 1000, CPU, lpips=True)
    with pytest.raises(ValueError, match="patch"):
        shards.BatchAssembler(1, HS, WS, 256, CPU, lpips=True, patch=32)
    shards.BatchAssembler(1, HS, WS, 256, CPU, lpips=True, patch=16)
    with pytest.raises(ValueError, match="does not fit"):
        shards.BatchAssembler(1, HS, WS, SIDE * SIDE, CPU, lpips=True, patch=SIDE)
    shards.BatchAssembler(1, HS, WS, 1000, CPU)                         # without lpips any count, as before


def test_without_lpips_the_generator_is_consumed_as_before():
    sh = scene()
    R = 300
    asm = shards.BatchAssembler(2, HS, WS, R, CPU)
    rng, twin = np.random.default_rng(3), np.random.default_rng(3)
    for b in (0, 1, 0):
        asm.fill(b, sh, (0, 1, 2), rng)
        assert np.array_equal(asm.ray_pix[b].numpy(), twin.permutation(SIDE * SIDE)[:R].astype(np.int32))
    assert rng.integers(0, 1 << 30) == twin.integers(0, 1 << 30)        # nothing else was drawn
    assert asm.mask is None                                             # the mask exists with lpips=True only


def test_patch_from_rays_ignores_the_order_of_the_rays():
    g = torch.Generator().manual_seed(2)
    B = 3
    x0, y0 = torch.tensor([0, 7, 31]), torch.tensor([31, 2, 0])
    ys, xs = torch.meshgrid(torch.arange(PATCH), torch.arange(PATCH), indexing="ij")
    uv = torch.stack((xs.reshape(-1)[None] + x0[:, None], ys.reshape(-1)[None] + y0[:, None]), -1).float()      # (B, R, 2)
    rgb = torch.rand(B, PATCH * PATCH, 3, generator=g)
    want = rgb.view(B, PATCH, PATCH, 3).permute(0, 3, 1, 2)
    assert torch.equal(losses.patch_from_rays(rgb, uv, PATCH), want)
    for _ in range(3):
        perm = torch.stack([torch.randperm(PATCH * PATCH, generator=g) for _ in range(B)])
        take = lambda t: torch.gather(t, 1, perm[..., None].expand(-1, -1, t.shape[-1]))
        assert torch.equal(losses.patch_from_rays(take(rgb), take(uv), PATCH), want)
    src = rgb.clone().requires_grad_(True)                              # differentiable: every ray gets its pixel's gradient
    wgt = torch.rand(B, 3, PATCH, PATCH, generator=g)
    perm = torch.stack([torch.randperm(PATCH * PATCH, generator=g) for _ in range(B)])
    take = lambda t: torch.gather(t, 1, perm[..., None].expand(-1, -1, t.shape[-1]))
    (losses.patch_from_rays(take(src), take(uv), PATCH) * wgt).sum().backward()
    assert torch.equal(src.grad, wgt.permute(0, 2, 3, 1).reshape(B, -1, 3))
    with pytest.raises(ValueError, match="patch_from_rays"):
        losses.patch_from_rays(rgb[:, :100], uv[:, :100], PATCH)
    # rays that cover no window (a wrong mask): every index stays inside the patch - a meaningless image, no out-of-range write
    wild = torch.randint(0, 256, (B, PATCH * PATCH, 2), generator=g).float()
    got = losses.patch_from_rays(rgb, wild, PATCH)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())


def test_loss_config_default_is_todays():
    cfg = losses.LossConfig()
    assert (cfg.cycle, cfg.pose, cfg.ssim) == (False, False, False) and cfg.lpips == 0.0
    assert cfg == losses.LossConfig(cycle=False, pose=False, ssim=False)
    assert losses.LossConfig(lpips=0.5).lpips == 0.5
    for bad in (-0.1, float("nan")):                                    # a weight that would switch the term off unnoticed
        with pytest.raises(ValueError, match="weight >= 0"):
            losses.LossConfig(lpips=bad)


def test_the_term_asks_for_its_network_and_a_host_mask():
    cfg = losses.LossConfig(lpips=1.0)
    rgb = torch.zeros(1, 1, PATCH * PATCH, 3)
    uv = torch.zeros(1, 1, PATCH * PATCH, 2)
    with pytest.raises(ValueError, match="perceptual"):
        losses.loss_terms(cfg, {"query": {"uv": uv, "mask": torch.ones(1, dtype=torch.int64)}}, {"rgb": rgb}, rgb)
    with pytest.raises(ValueError, match="mask"):
        losses.loss_terms(cfg, {"query": {"uv": uv}}, {"rgb": rgb}, rgb, perceptual=object())
    zero = losses.lpips_patch_loss(object(), rgb, rgb, uv, torch.zeros(1, dtype=torch.int64))      # no patch pair: the network is not called
    assert zero.item() == 0.0 and not zero.requires_grad
    assert set(losses.loss_terms(losses.LossConfig(), {"query": {"uv": uv}}, {"rgb": rgb}, rgb)) == {"img_loss"}
