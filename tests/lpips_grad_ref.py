"""Float64 yardstick for the LPIPS training term (helper, no tests of its own: tests/test_lpips_grad_ref.py pins it).

Gradients come from float64 autograd through the functions of tests/lpips_ref.py (imported, not edited): `head64` for the
distance head, `scale64` / `features64` for the stem and the whole network.  Next to them stands a float64 closed-form
restatement of the two adjoints that csrc/lpips.hip implements (include/coponerf_hip.h states them), which also carries the one
rule autograd does not give: at a pixel whose prediction vector is all zeros the head's gradient is 0 (autograd: NaN, from the
root's derivative at 0).  The closed forms return, per element, the sum of the absolute values of the element's terms: what the
bounds of tests/test_gpu_lpips_grad.py are relative to.

`defect=` applies one seeded mistake to a closed form; tests/test_lpips_grad_ref.py shows that each one exceeds the GPU test's
bounds at least 100 times on that test's own cases (built here, once, and shared read-only).
"""
import functools

import torch
import torch.nn.functional as F

from coponerf_amd import synthetic as syn
from coponerf_amd.lpips import parse_state_dict, synthetic_state_dict
from tests import lpips_ref as lr

U = 2.0 ** -24
SEED = 3                                                    # LPIPS.synthetic(SEED), as tests/test_gpu_lpips.py

# Bounds of tests/test_gpu_lpips_grad.py, counted from the kernels' operation sequences in units of one rounding u = 2^-24
# (that test's docstring writes the counts out)
K_HEAD_BWD = 132
K_STEM_BWD = 20

HEAD_DEFECTS = ("no_projection", "no_pixel_mean")
STEM_DEFECTS = ("relu_mask_from_dy", "no_clamp_mask", "kernel_not_flipped", "no_scale")

HEAD_C = (64, 512)
HEAD_HW = ((1, 1), (2, 2), (5, 7), (16, 16))
HEAD_N = (1, 3)
HEAD_KINDS = ("unit", "large", "tiny", "zeros")
STEM_HW = ((16, 16), (16, 40), (24, 16))


# --------------------------------------------------------------------------------------------------------------- head
@functools.lru_cache(maxsize=None)
def head_case(N, C, h, w, kind="unit"):
    """(maps (2N, h, w, C) fp32, lin (C), g (N) fp32) - the maps of tests/test_gpu_lpips.py's head cases; g of both signs.
    `zeros`: pixel 0 of image 0 is zero in both maps, pixel P // 2 of image 0 in the prediction only, the last pixel of the
    last image in the target only."""
    scale = {"unit": 1.0, "large": 1e4, "tiny": 1e-12, "zeros": 1.0}[kind]
    feat, lin = lr.make_maps(N, C, h, w, seed=1000 * C + 10 * h + w + N, scale=scale)
    if kind == "zeros":
        f = feat.view(2 * N, h * w, C)
        f[0, 0] = 0.0
        f[N, 0] = 0.0
        f[0, (h * w) // 2] = 0.0
        f[2 * N - 1, h * w - 1] = 0.0
    g = (syn.uniform((N,), 7 + N, 0.5, 1.5, stream=6) * torch.tensor([1.0, -1.0, 1.0][:N])).float()
    return feat, lin.float(), g


def zero_pixels(N, h, w):
    """(image, pixel) of the prediction vectors a `zeros` case sets to 0."""
    return sorted({(0, 0), (0, (h * w) // 2)})


def head_grad_autograd(feat, lin, N, g):
    """d sum_n g_n d_n / d f_pred through lpips_ref.head64, float64, (N, h, w, C).  NaN at a zero prediction vector."""
    f = feat.double().permute(0, 3, 1, 2)
    fp = f[:N].clone().requires_grad_(True)
    d, _ = lr.head64(fp, f[N:], lin.double())
    (d * g.double()).sum().backward()
    return fp.grad.permute(0, 2, 3, 1)


def head_grad_closed(feat, lin, N, g, defect=None):
    """The adjoint as the header states it, float64: (df (N, h, w, C), per element r |u_j| + (sum_c |u_c| |f_c|) r^2 |f_j| / s
    with |u_c| = lin_c (|a_c| + |b_c|) 2 |g_n| / P).  s == 0: df = 0 and the terms are 0."""
    f = feat.double()
    fp, ft = f[:N], f[N:]
    P = fp.shape[1] * fp.shape[2]
    s = fp.pow(2).sum(-1, keepdim=True).sqrt()
    r = 1.0 / (s + lr.EPS)
    a = fp * r
    b = ft / (ft.pow(2).sum(-1, keepdim=True).sqrt() + lr.EPS)
    coef = 2.0 * g.double().view(N, 1, 1, 1) / (1.0 if defect == "no_pixel_mean" else P)
    w = lin.double().view(1, 1, 1, -1)
    u = w * (a - b) * coef
    u_abs = w * (a.abs() + b.abs()) * coef.abs()
    live = s > 0
    s1 = torch.where(live, s, torch.ones_like(s))
    proj = (u * fp).sum(-1, keepdim=True) * r * r / s1 * fp
    df = r * u - (0.0 if defect == "no_projection" else proj)
    terms = r * u_abs + (u_abs * fp.abs()).sum(-1, keepdim=True) * r * r / s1 * fp.abs()
    return torch.where(live, df, torch.zeros_like(df)), torch.where(live, terms, torch.zeros_like(terms))


# --------------------------------------------------------------------------------------------------------------- stem
def stem_weights():
    w, b, _ = parse_state_dict(synthetic_state_dict(SEED))
    return w[0].contiguous(), b[0].contiguous()


@functools.lru_cache(maxsize=None)
def stem_case(N, H, W):
    """(pred (N, H, W, 3), y (N, H, W, 64), dy (N, H, W, 64)), fp32.  pred leaves [-1, 1] in places and holds values at exactly
    +1 and -1 and two NaNs (one on a border); y is relu1_1 of pred (float64, rounded: zero where the ReLU is off, NaN round a
    NaN pixel) with one block set to 0 on top; dy is noise of both signs."""
    p, t = lr.make_images(N, H, W, seed=21, target_gain=1.5)
    p = (1.5 * p).permute(0, 2, 3, 1).contiguous()         # a good part of it beyond +-1
    p[0, 3, 4, 0], p[0, 3, 5, 1], p[N - 1, H - 1, W - 2, 2] = 1.0, -1.0, 1.0
    p[0, 0, 7, 1] = float("nan")
    p[N - 1, 9, W - 3, 0] = float("nan")
    w, b = stem_weights()
    y = lr.stem64(p, p, w, b)[0][:N].float().contiguous()
    y[:, 5:11, 2:9] = 0.0
    dy = syn.normal((N, H, W, 64), 100 * H + W + N, 1.0, stream=8).float().contiguous()
    return p, y, dy


def _stem_masks(pred, y, dy, defect):
    relu = (dy > 0) if defect == "relu_mask_from_dy" else (y > 0)
    clamp = torch.ones_like(pred, dtype=torch.bool) if defect == "no_clamp_mask" else (pred >= -1.0) & (pred <= 1.0)
    return relu, clamp


def stem_grad_autograd(pred, y, dy, w):
    """d sum(dy [y > 0] z) / d pred, float64, with z = conv1_1(scaling layer(clamp(pred))) through lpips_ref.scale64: the ReLU's
    mask is taken from the given stem output y, as the kernel takes it.  A NaN in pred is replaced by 0 before the clamp
    (torch's clamp passes no gradient to a NaN; the convolution is linear, so its gradient does not depend on the value)."""
    nan = torch.isnan(pred)
    p = torch.where(nan, torch.zeros_like(pred), pred).double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    z = F.conv2d(F.pad(lr.scale64(p.clamp(-1.0, 1.0)), (1, 1, 1, 1)), w.double())
    (z * (dy.double() * (y > 0)).permute(0, 3, 1, 2)).sum().backward()
    return torch.where(nan, torch.zeros_like(pred, dtype=torch.float64), p.grad.permute(0, 2, 3, 1))


def stem_grad_closed(pred, y, dy, w, defect=None):
    """The adjoint as the header states it, float64: (dpred (N, H, W, 3), per element sum |w| |dy'| / scale)."""
    relu, clamp = _stem_masks(pred, y, dy, defect)
    d = (dy.double() * relu).permute(0, 3, 1, 2)
    w64 = w.double()
    if defect == "kernel_not_flipped":
        w64 = w64.flip(2, 3)
    full = F.conv_transpose2d(d, w64, padding=1)
    mag = F.conv_transpose2d(d.abs(), w64.abs(), padding=1)
    scale = 1.0 if defect == "no_scale" else lr.SCALE32.double().view(1, 3, 1, 1)
    full, mag = (full / scale).permute(0, 2, 3, 1), (mag / scale).permute(0, 2, 3, 1)
    return torch.where(clamp, full, torch.zeros_like(full)), torch.where(clamp, mag, torch.zeros_like(mag))


# -------------------------------------------------------------------------------------------------------- end to end
def lpips_grad64(p, t, seed):
    """(lpips (N), d sum_n lpips_n / d p (N, 3, H, W), per-element bound term) in float64 on the fp32 images: the network of
    lpips_ref (inputs32, scale64, features64, head64) with the prediction's fp32 round-tripped VALUE and the clamp's gradient.
    The bound term is the stem adjoint's sum |w| |dy'| / scale on the float64 gradient of relu1_1."""
    weights, biases, lins = lr.weights64(seed)
    N = p.shape[0]
    xp32, xt32 = lr.inputs32(p, t)
    p64 = p.double().clone().requires_grad_(True)
    pc = p64.clamp(-1.0, 1.0)
    xp = xp32.double() + (pc - pc.detach())                 # the value the kernel sees; the derivative of clamp + round trip
    x = F.pad(lr.scale64(torch.cat((xp, xt32.double()))), (1, 1, 1, 1))
    z = F.conv2d(x, weights[0], biases[0])
    z.retain_grad()
    y = F.relu(z)
    taps, n = [], 1
    for j, block in enumerate(lr.BLOCKS):
        if j:
            y = F.max_pool2d(y, 2, 2)
        for q, _ in enumerate(block):
            if j == 0 and q == 0:
                continue
            y = F.relu(F.conv2d(y, weights[n], biases[n], padding=1))
            n += 1
        taps.append(y)
    total = sum(lr.head64(f[:N], f[N:].detach(), w)[0] for f, w in zip(taps, lins))
    total.sum().backward()
    mag = F.conv_transpose2d(z.grad[:N].abs(), weights[0].abs(), padding=1) / lr.SCALE32.double().view(1, 3, 1, 1)
    return total.detach(), p64.grad, mag
