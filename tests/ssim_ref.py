"""Yardsticks of the flow-warp SSIM term (coponerf_amd/losses.py, csrc/ssim_warp.hip) and the inputs of its tests.

  case(...)        the synthetic inputs of tests/golden/ssim.npz (make_golden_ssim.py) and of the smaller GPU cases
  stock_loss(...)  the stock fp32 composition: F.interpolate, grid_sample and conv2d, as upstream's LFLoss writes it
                   (models/loss_function.py:19-60, 109-120; utils_training/utils.py:642-671)
  ref64_loss(...)  float64, with an explicit four-tap sampler whose sampling coordinates are GIVEN in fp32 and lifted: their
                   value is the lifted number, their derivative the analytic W/(W-1) d up / d flow.  A coordinate within an ulp
                   of an integer picks another tap pair in float64 than in fp32 - one such pixel moves a dflow entry by 4e-2 of
                   the largest - so a float64 run on its own coordinates is no yardstick for an fp32 one; on lifted ones it is.

A direction d of a batch: view 1 - d warped by flow_d against view d, normalised over the batch as upstream does.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from coponerf_amd import synthetic as syn

SEED = 81
FIXTURE = dict(B=2, H=256, W=256, s=4)


def window1d(dtype=torch.float32):
    """loss_function.gaussian(11, 1.5) on the CPU."""
    g = torch.tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return (g / g.sum()).to(dtype)


def window2d(dtype=torch.float32):
    """create_window(11, 3): the fp32 outer product, (3, 1, 11, 11)."""
    w = window1d().unsqueeze(1)
    return w.mm(w.t())[None, None].expand(3, 1, 11, 11).contiguous().to(dtype)


def case(B=FIXTURE["B"], H=FIXTURE["H"], W=FIXTURE["W"], s=FIXTURE["s"], seed=SEED):
    """(rgb (B, 2, H, W, 3), f0, f1 (B, 2, H/s, W/s)) fp32, pure functions of the arguments.  Images: 0.6 x the mean of four
    low-frequency sinusoids + 0.4 x U[-1, 1).  Flows in low-resolution pixels: f0 = (3, -1.5) + smooth + N(0, 0.2^2),
    f1 = -(3, -1.5) - smooth + ramp(x: 0 -> 4) N(0, 1): consistent on the left, inconsistent towards the right edge."""
    h, w = H // s, W // s
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ph = syn.uniform((B, 2, 3, 4, 3), seed, 0.0, 1.0, stream=1).double()           # per image, channel, wave: fx, fy, phase
    img = torch.zeros(B, 2, 3, H, W, dtype=torch.float64)
    for k in range(4):
        fx, fy, p0 = (ph[..., k, i][..., None, None] for i in range(3))
        img += torch.sin(2 * math.pi * ((0.5 + 2.5 * fx) * xs / W + (0.5 + 2.5 * fy) * ys / H + p0))
    img = 0.6 * (img / 4) + 0.4 * syn.uniform((B, 2, 3, H, W), seed, -1.0, 1.0, stream=2).double()
    rgb = img.permute(0, 1, 3, 4, 2).contiguous().float()
    yl, xl = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    smooth = torch.stack((0.8 * torch.sin(2 * math.pi * yl / max(h, 2)) + 0.5 * torch.cos(2 * math.pi * xl / max(w, 2)),
                          0.6 * torch.cos(2 * math.pi * (xl + yl) / max(h + w, 2))))[None]
    base = torch.tensor([3.0, -1.5], dtype=torch.float64).view(1, 2, 1, 1)
    ramp = (4.0 * xl / max(w - 1, 1))[None, None]
    f0 = base + smooth + syn.normal((B, 2, h, w), seed, std=0.2, stream=3).double()
    f1 = -base - smooth + ramp * syn.normal((B, 2, h, w), seed, std=1.0, stream=4).double()
    return rgb, f0.float().contiguous(), f1.float().contiguous()


def views(rgb, d):
    """(source, target) of direction d as (B, 3, H, W) views."""
    return rgb[:, 1 - d].permute(0, 3, 1, 2), rgb[:, d].permute(0, 3, 1, 2)


def _grid(H, W, like):
    ys, xs = torch.meshgrid(torch.arange(H, device=like.device), torch.arange(W, device=like.device), indexing="ij")
    return torch.stack((xs, ys), 0).to(like.dtype)[None]


def upsample(flow, H, W):
    """loss_function.py:112-113 (the factor is H / h as 256 / h there)."""
    return F.interpolate(flow, (H, W), mode="bilinear") * (H / flow.shape[2])


def unnormalised_coords(up):
    """utils.warp's normalisation followed by grid_sample's unnormalisation (align_corners=False), in the tensor's own
    precision: (B, 2, H, W) pixel coordinates (ix, iy)."""
    B, _, H, W = up.shape
    v = _grid(H, W, up) + up
    gx = 2.0 * v[:, 0] / max(W - 1, 1) - 1.0
    gy = 2.0 * v[:, 1] / max(H - 1, 1) - 1.0
    return torch.stack((((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2), 1)


def warp(x, up):
    """utils_training/utils.py:642-671."""
    B, _, H, W = x.shape
    v = _grid(H, W, up) + up
    gx = 2.0 * v[:, 0] / max(W - 1, 1) - 1.0
    gy = 2.0 * v[:, 1] / max(H - 1, 1) - 1.0
    return F.grid_sample(x, torch.stack((gx, gy), -1), align_corners=False)


def ssim_masked(img1, img2, window, mask):
    """loss_function._ssim: mask (B, 1, H, W) in the images' dtype."""
    conv = lambda t: F.conv2d(t, window, padding=5, groups=3)
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = conv(img1 * img1) - mu1_sq
    s2 = conv(img2 * img2) - mu2_sq
    s12 = conv(img1 * img2) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return torch.sum((1 - m) * mask) / torch.sum(mask) / 3


def stock_loss(rgb, flow, mask, d, window=None):
    """Direction d in stock fp32 ops on rgb's device; flow (B, 2, h, w) may require grad; mask (B, H, W) bool; window: create_window's
    tensor already on the device (a timing loop must not copy it from the host every step)."""
    src, tgt = views(rgb, d)
    H, W = rgb.shape[2:4]
    up = upsample(flow, H, W)
    window = window2d().to(rgb.device) if window is None else window
    return ssim_masked(warp(src, up), tgt, window, mask.unsqueeze(1).to(rgb.dtype))


def masks_of(f0, f1, H, W):
    """loss_function.py:115-118 in stock ops: (m0, m1) (B, H, W) bool."""
    u0, u1 = upsample(f0, H, W), upsample(f1, H, W)
    inside = lambda u: (lambda m: m[:, 0].ge(0) & m[:, 0].le(W - 1) & m[:, 1].ge(0) & m[:, 1].le(H - 1))(u + _grid(H, W, u))
    m0 = torch.norm(u0 + warp(u1, u0), dim=1).le(10) * inside(u0)
    m1 = torch.norm(u1 + warp(u0, u1), dim=1).le(10) * inside(u1)
    return m0, m1


def sample_taps(x, ix, iy):
    """Four zero-padded bilinear taps of x (B, C, H, W) at pixel coordinates ix, iy (B, H, W); differentiable in ix, iy through
    the weights, as grid_sample's backward is."""
    B, C, H, W = x.shape
    x0, y0 = torch.floor(ix.detach()), torch.floor(iy.detach())
    out = x.new_zeros(B, C, H, W)
    flat = x.reshape(B, C, H * W)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wx = (ix - x0) if dx else (x0 + 1 - ix)
            wy = (iy - y0) if dy else (y0 + 1 - iy)
            ok = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(B, 1, H * W).expand(-1, C, -1)
            val = torch.gather(flat, 2, idx).reshape(B, C, H, W)
            out = out + torch.where(ok, wx * wy, torch.zeros_like(wx)).unsqueeze(1) * val
    return out


def ref64_loss(rgb, flow, mask, d, coords32):
    """Direction d in float64 on the CPU at the GIVEN fp32 coordinates coords32 (B, 2, H, W).  Returns (loss, dflow) float64."""
    src, tgt = views(rgb.detach().cpu().double(), d)
    B, _, H, W = src.shape
    f = flow.detach().cpu().double().requires_grad_(True)
    up = upsample(f, H, W)
    c = coords32.detach().cpu().double()
    # value: the lifted coordinate; derivative: d ix / d up_x = (W / 2) (2 / max(W - 1, 1))
    ix = c[:, 0] + (W / max(W - 1, 1)) * (up[:, 0] - up[:, 0].detach())
    iy = c[:, 1] + (H / max(H - 1, 1)) * (up[:, 1] - up[:, 1].detach())
    loss = ssim_masked(sample_taps(src, ix, iy), tgt, window2d(torch.float64), mask.cpu().unsqueeze(1).double())
    g, = torch.autograd.grad(loss, f)
    return loss.detach(), g


def pack_mask(m):
    return np.packbits(m.cpu().numpy().astype(np.uint8))


def unpack_mask(p, shape):
    return torch.from_numpy(np.unpackbits(p)[: int(np.prod(shape))].reshape(shape).astype(bool))


def rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm())


def rel_max(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / want.abs().max())
