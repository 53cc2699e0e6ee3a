"""The reference's training loss, every flag (models/loss_function.py:89-137 of the reference, `train.py --cycle --pose --ssim`).

  img_loss    |gt - rgb|.mean() with NaNs zeroed (loss_function.py:65-71)                          always
  cycle_loss  0.01 x masked Huber of the two reprojections (loss_function.py:122-130)               LossConfig.cycle
  pose_loss   geodesic rotation distance + translation distance (loss_function.py:74-86, 132-134)  LossConfig.pose
  ssim_loss   the flow-warp SSIM of both directions (loss_function.py:19-60, 109-120)              LossConfig.ssim
  lpips_loss  weight x mean LPIPS of the rendered 32 x 32 patches against the true ones              LossConfig.lpips
              (not in the reference's loss: its loaders draw the patches with lpips=True, loss_function.py:11 imports `lpips`
              and never calls it; the definition here is this package's)

The cycle and pose terms are stock ops on (B, R, 2) and (B, 3, 3) tensors.  The SSIM term is csrc/ssim_warp.hip: 2 launches
forward and 2 backward for both directions of every pair, differentiable in the two flows.  Nothing here reads a device value
on the host or copies pageable host memory to the device: a step's loss stays as asynchronous as the step.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from . import _hip

W_CYCLE, W_SSIM, W_POSE = 0.01, 1.0, 1.0          # LFLoss.w1, w2, w3
WINDOW_SIZE, WINDOW_SIGMA = 11, 1.5


@dataclasses.dataclass(frozen=True)
class LossConfig:
    """Which terms join the image loss: the reference's `--cycle --pose --ssim` switches, and the patch LPIPS term's weight."""
    cycle: bool = False
    pose: bool = False
    ssim: bool = False
    lpips: float = 0.0                                # weight of the patch LPIPS term; the reference has none to copy

    def __post_init__(self):
        if not self.lpips >= 0:                         # a negative weight, or NaN
            raise ValueError(f"LossConfig: lpips is a weight >= 0 (0 switches the term off), got {self.lpips}")


def gaussian_window(size: int = WINDOW_SIZE, sigma: float = WINDOW_SIGMA) -> torch.Tensor:
    """loss_function.gaussian: fp32 exp values, normalised in fp32 (CPU tensor)."""
    g = torch.tensor([math.exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)], dtype=torch.float32)
    return g / g.sum()


_WINDOWS: Dict[str, torch.Tensor] = {}


def _window(device) -> torch.Tensor:
    key = str(device)
    w = _WINDOWS.get(key)
    if w is None:                                   # a constant: once per device, from pinned memory
        host = gaussian_window()
        w = _WINDOWS[key] = host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host
    return w


def _check(ctx_rgb, flow0, flow1, masks):
    if not ctx_rgb.is_cuda:
        raise RuntimeError("ssim_warp_loss runs on the HIP device only (coponerf_amd has no non-HIP compute path)")
    B, V, H, W, C = ctx_rgb.shape
    if V != 2 or C != 3:
        raise ValueError(f"ssim_warp_loss: context rgb must be (B, 2, H, W, 3), got {tuple(ctx_rgb.shape)}")
    if flow0.shape != flow1.shape or flow0.dim() != 4 or flow0.shape[0] != B or flow0.shape[1] != 2:
        raise ValueError(f"ssim_warp_loss: flows must both be (B, 2, h, w), got {tuple(flow0.shape)} and {tuple(flow1.shape)}")
    if tuple(masks.shape) != (B, 2, H, W) or masks.dtype != torch.bool:
        raise ValueError(f"ssim_warp_loss: masks must be bool (B, 2, H, W), got {masks.dtype} {tuple(masks.shape)}")
    for t in (ctx_rgb, flow0, flow1):
        if t.dtype != torch.float32:
            raise ValueError("ssim_warp_loss: fp32 tensors only")


class _SsimWarp(torch.autograd.Function):
    """loss (2,): per direction, sum_b sum (1 - ssim) mask / sum_b sum mask / 3.  Differentiable in flow0 and flow1."""

    @staticmethod
    def forward(ctx, ctx_rgb, flow0, flow1, masks):
        rgb, f0, f1, mk = ctx_rgb.contiguous(), flow0.contiguous(), flow1.contiguous(), masks.contiguous()
        B, _, H, W, _ = rgb.shape
        h, w = f0.shape[2:]
        dev = rgb.device
        f32 = torch.float32
        nblk = _hip.lib().cpn_ssim_warp_blocks(H, W)
        coords = torch.empty(2 * B, 2, H, W, dtype=f32, device=dev)
        maps = torch.empty(2 * B, 9, H, W, dtype=f32, device=dev)
        partial = torch.empty(2 * B, max(nblk, 1), 2, dtype=f32, device=dev)
        sums = torch.empty(2 * B, 2, dtype=f32, device=dev)
        loss = torch.empty(2, dtype=f32, device=dev)
        inv = torch.empty(2, dtype=f32, device=dev)
        win = _window(dev)
        _hip.call("cpn_ssim_warp", rgb.data_ptr(), f0.data_ptr(), f1.data_ptr(), mk.data_ptr(), win.data_ptr(), B, H, W, h, w,
                  coords.data_ptr(), maps.data_ptr(), partial.data_ptr(), sums.data_ptr(), loss.data_ptr(), inv.data_ptr(),
                  _hip.stream_handle())
        ctx.save_for_backward(rgb, coords, maps, inv, win)
        ctx.low = (h, w)
        ctx.mark_non_differentiable(coords, sums)
        return loss, coords, sums

    @staticmethod
    def backward(ctx, gloss, _gc, _gs):
        rgb, coords, maps, inv, win = ctx.saved_tensors
        B, _, H, W, _ = rgb.shape
        h, w = ctx.low
        g = gloss.contiguous().float()
        gup = torch.empty(2 * B, 2, H, W, dtype=torch.float32, device=rgb.device)
        dflow = torch.empty(B, 2, 2, h, w, dtype=torch.float32, device=rgb.device)          # (pair, direction, xy, h, w)
        _hip.call("cpn_ssim_warp_bwd", rgb.data_ptr(), coords.data_ptr(), maps.data_ptr(), win.data_ptr(), g.data_ptr(),
                  inv.data_ptr(), B, H, W, h, w, gup.data_ptr(), dflow.data_ptr(), _hip.stream_handle())
        return None, dflow[:, 0], dflow[:, 1], None


def ssim_warp_terms(ctx_rgb: torch.Tensor, flow0: torch.Tensor, flow1: torch.Tensor, masks: torch.Tensor):
    """(loss (2,) per direction, coords (2B, 2, H, W), sums (2B, 2)) of cpn_ssim_warp; masks (B, 2, H, W) bool.  Item 2 b + d
    warps view 1 - d by flow_d[b] and compares it with view d under masks[b, d]."""
    _check(ctx_rgb, flow0, flow1, masks)
    return _SsimWarp.apply(ctx_rgb, flow0, flow1, masks)


def ssim_warp_loss(ctx_rgb: torch.Tensor, flow0: torch.Tensor, flow1: torch.Tensor,
                   masks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """loss_function.py:109-120: w2 (L0 + L1) / 2, L_d the masked SSIM loss of view 1 - d warped by flow_d against view d.
    masks (B, 2, H, W) bool or None: then the cycle-consistency x in-image masks of the flows themselves
    (aux_outputs.cycle_masks, = upstream's cyclic_consistency_error * get_gt_correspondence_mask), without gradient."""
    if masks is None:
        from .aux_outputs import cycle_masks
        if tuple(ctx_rgb.shape[2:4]) != (256, 256):
            raise ValueError("ssim_warp_loss: the flows' own masks are defined at 256 x 256 (CoPoNeRF.py:230-236); pass `masks`")
        with torch.no_grad():
            m1, m2 = cycle_masks((flow0.detach(), flow1.detach()), flow0.shape[2])
            masks = torch.stack((m1, m2), 1)
    loss = ssim_warp_terms(ctx_rgb, flow0, flow1, masks)[0]
    return W_SSIM * (loss[0] + loss[1]) / 2


def _geodesic(m1: torch.Tensor, m2: torch.Tensor) -> torch.Tensor:
    """loss_function.py:76-86."""
    m = torch.bmm(m1, m2.transpose(1, 2))
    cos = (m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2
    cos = torch.max(torch.min(cos, torch.ones_like(cos)), -torch.ones_like(cos))
    return torch.acos(cos).mean()


def image_loss(out_rgb: torch.Tensor, gt_rgb: torch.Tensor) -> torch.Tensor:
    zero = lambda t: torch.where(torch.isnan(t), torch.zeros_like(t), t)      # loss_function.py:66-69
    return (zero(gt_rgb) - zero(out_rgb)).abs().mean()


def patch_from_rays(rgb: torch.Tensor, uv: torch.Tensor, patch: int) -> torch.Tensor:
    """rgb (B, R, 3) and uv (B, R, 2) pixel coordinates (x, y) of R = patch^2 rays that cover a patch x patch window, in ANY
    order -> (B, 3, patch, patch).  Ray r goes to row y - min y, column x - min x of its own pair: the result does not depend
    on the order of the rays (TrainStep sorts them by tile).  Stock ops on B patch^2 elements, differentiable in rgb.
    PRECONDITION: the rays of every pair do cover such a window (what mask = 1 says).  The host cannot check that without
    reading uv back; for rays that do not, the index is clamped into the patch, so the result is a meaningless image (rays
    overwrite each other, pixels stay 0) and never an out-of-range write."""
    B, R, _ = rgb.shape
    if R != patch * patch or tuple(uv.shape) != (B, R, 2):
        raise ValueError(f"patch_from_rays: {patch} x {patch} patches need rgb (B, {patch * patch}, 3) and uv (B, {patch * patch}, 2), "
                         f"got {tuple(rgb.shape)} and {tuple(uv.shape)}")
    x, y = uv[..., 0].floor().long(), uv[..., 1].floor().long()
    idx = (y - y.min(1, keepdim=True).values) * patch + (x - x.min(1, keepdim=True).values)      # (B, R): a permutation
    idx = idx.clamp(0, R - 1)                                                   # no effect on a window; see the precondition
    out = torch.zeros_like(rgb).scatter(1, idx[..., None].expand(-1, -1, 3), rgb)
    return out.view(B, patch, patch, 3).permute(0, 3, 1, 2)


def lpips_patch_loss(perceptual, rgb: torch.Tensor, gt_rgb: torch.Tensor, uv: torch.Tensor, mask,
                     patch: Optional[int] = None) -> torch.Tensor:
    """mean over the pairs with mask == 1 of perceptual.differentiable(patch of rgb, patch of gt_rgb); rgb, gt_rgb (B, 1, R, 3)
    or (B, R, 3), uv likewise with 2.  mask (B,) lives on the HOST (shards.BatchAssembler drew it there): which pairs are
    patches decides shapes, and a device mask would have to be read back.  No patch pair: an exact zero without a graph.
    patch=None: the side whose square is the ray count (32 for the reference's 1 024 rays; BatchAssembler insists on
    rays == patch^2)."""
    if not torch.is_tensor(mask) or mask.is_cuda:
        raise ValueError("lpips_patch_loss: query['mask'] must be a host tensor - keep it on the host, where the loader drew it "
                         "(a device mask would cost a read-back every step)")
    rows = [b for b, m in enumerate(mask.reshape(-1).tolist()) if m]
    if not rows:
        return torch.zeros((), dtype=torch.float32, device=rgb.device)
    B = rgb.shape[0]
    flat = lambda t: t.reshape(B, -1, t.shape[-1])
    rgb, gt_rgb, uv = flat(rgb), flat(gt_rgb), flat(uv)
    if patch is None:
        patch = math.isqrt(rgb.shape[1])
    if len(rows) != B:
        rgb, gt_rgb, uv = (torch.stack([t[b] for b in rows]) for t in (rgb, gt_rgb, uv))      # rows are host integers
    return perceptual.differentiable(patch_from_rays(rgb, uv, patch), patch_from_rays(gt_rgb.detach(), uv, patch)).mean()


def loss_terms(cfg: LossConfig, model_input: Dict, out: Dict, gt_rgb: torch.Tensor, perceptual=None) -> Dict[str, torch.Tensor]:
    """The terms `cfg` switches on, by the reference's names; the step's loss is their sum (wrapper.py:109-123).
    perceptual: the lpips.LPIPS of the `lpips` term."""
    terms = {"img_loss": image_loss(out["rgb"], gt_rgb)}
    if cfg.ssim:
        flow: Sequence[torch.Tensor] = out["flow"]
        terms["ssim_loss"] = ssim_warp_loss(model_input["context"]["rgb"], flow[0], flow[1])
    if cfg.cycle:
        a, b = out["T_to_C1_pts"], out["C2_pts_to_C1"]
        dist = torch.norm(a - b, dim=-1, keepdim=True)
        valid = dist.detach().le(20).float() * out["mask_c2"].unsqueeze(-1) * out["matchability_cycle_mask"].unsqueeze(-1)
        hub = F.huber_loss(a, b, reduction="none")
        terms["cycle_loss"] = W_CYCLE * ((hub * valid).sum() / (valid.sum() + 1e-6))
    if cfg.pose:
        rel, gt = out["rel_pose"], out["gt_rel_pose"]
        terms["pose_loss"] = W_POSE * (_geodesic(rel[:, :3, :3], gt[:, :3, :3])
                                       + torch.norm(rel[:, :3, 3] - gt[:, :3, 3], dim=-1).mean())
    if cfg.lpips > 0:
        q = model_input["query"]
        if perceptual is None:
            raise ValueError("LossConfig.lpips > 0 needs the network: TrainStep(..., perceptual=LPIPS...)")
        if "mask" not in q:
            raise ValueError("LossConfig.lpips > 0 needs query['mask'] (shards.BatchAssembler(lpips=True) makes it)")
        terms["lpips_loss"] = cfg.lpips * lpips_patch_loss(perceptual, out["rgb"], gt_rgb, q["uv"], q["mask"])
    return terms
