"""Float64 yardstick for coponerf_amd.lpips (helper, no tests of its own: tests/test_lpips_ref.py pins it).

The `lpips` package is not a dependency, so LPIPS(net='vgg', version='0.1', lpips=True, spatial=False, normalize=False) is
restated here from its published definition, in torch float64 on the CPU:

  1. test.py:227-229, 258-259: the prediction clamped to [-1, 1]; both images through x01 = (x + 1) * 0.5, x = (x01 - 0.5) * 2,
     every operation rounded to fp32 (done in fp32 here, before anything is widened);
  2. the scaling layer (x - shift) / scale, shift (-.030, -.088, -.188), scale (.458, .448, .450) - fp32 constants, widened;
  3. torchvision's vgg16().features: 3 x 3 convolutions (stride 1, zero padding 1 AFTER the scaling, bias, ReLU) at indices
     0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, 2 x 2 max pools (stride 2, floor) before blocks 2 .. 5, taps after relu1_2,
     relu2_2, relu3_3, relu4_3, relu5_3;
  4. per tap a = f_p / (sqrt(sum_c f_p^2) + 1e-10), b likewise; d_k[n] = mean_pixels sum_c w_k[c] (a_c - b_c)^2;
  5. lpips[n] = sum_k d_k[n].

`defect=` applies one seeded mistake to the restatement; tests/test_lpips_ref.py uses them to show that the bars of
tests/test_gpu_lpips.py are far below what any of them costs.
"""
import functools

import torch
import torch.nn.functional as F

from coponerf_amd import synthetic as syn
from coponerf_amd.lpips import parse_state_dict, synthetic_state_dict

# torchvision's vgg16().features, written out here so that the restatement shares no structure with the module under test: the
# indices of the convolutions block by block; a 2 x 2 max pool (indices 4, 9, 16, 23) stands before every block but the
# first, a ReLU after every convolution, and the taps are the blocks' last ReLUs (indices 3, 8, 15, 22, 29).
BLOCKS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))

SHIFT32 = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float32)
SCALE32 = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float32)
EPS = 1e-10
U = 2.0 ** -24
DEFECTS = ("pad_before_scale", "shift_sign", "tap_early", "channel_mean", "mis_split", "ceil_pool", "clamp_target")


@functools.lru_cache(maxsize=None)
def weights64(seed):
    """(conv weights, biases, lin weights) of LPIPS.synthetic(seed), widened to float64."""
    w, b, l = parse_state_dict(synthetic_state_dict(seed))
    return [x.double() for x in w], [x.double() for x in b], [x.double() for x in l]


def round_trip32(x):
    """test.py:227-229 then :258-259 on an fp32 tensor: every operation rounded to fp32."""
    assert x.dtype == torch.float32
    x01 = (x + 1.0) * 0.5
    return (x01 - 0.5) * 2.0


def inputs32(p, t, defect=None):
    """p, t (N, 3, H, W) fp32 -> the fp32 images the scaling layer sees; only the prediction is clamped."""
    p = p.clamp(-1.0, 1.0)
    if defect == "clamp_target":
        t = t.clamp(-1.0, 1.0)
    return round_trip32(p), round_trip32(t)


def scale64(x32, defect=None):
    shift = SHIFT32.double().view(1, 3, 1, 1) * (-1.0 if defect == "shift_sign" else 1.0)
    return (x32.double() - shift) / SCALE32.double().view(1, 3, 1, 1)


def features64(x32, weights, biases, defect=None):
    """The five tapped maps (2N, C, h, w) float64 of fp32 round-tripped images x32 (2N, 3, H, W)."""
    if defect == "pad_before_scale":
        x = scale64(F.pad(x32, (1, 1, 1, 1)), defect)
    else:
        x = F.pad(scale64(x32, defect), (1, 1, 1, 1))
    taps, n = [], 0
    for j, block in enumerate(BLOCKS):
        if j:
            x = F.max_pool2d(x, 2, 2, ceil_mode=defect == "ceil_pool")
        for q, _ in enumerate(block):
            if defect == "tap_early" and q == len(block) - 1:
                taps.append(x)
            x = F.relu(F.conv2d(x, weights[n], biases[n], padding=0 if n == 0 else 1))
            n += 1
        if defect != "tap_early":
            taps.append(x)
    return taps


def head64(fp, ft, w, defect=None):
    """fp, ft (N, C, h, w) float64, w (C) -> (d (N), bound term (N) = mean_pixels sum_c w_c (|a_c| + |b_c|)^2)."""
    a = fp / (fp.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    b = ft / (ft.pow(2).sum(1, keepdim=True).sqrt() + EPS)
    wv = (torch.full_like(w, 1.0 / w.numel()) if defect == "channel_mean" else w).view(1, -1, 1, 1)
    d = (wv * (a - b).pow(2)).sum(1).mean(dim=(1, 2))
    term = (wv * (a.abs() + b.abs()).pow(2)).sum(1).mean(dim=(1, 2))
    return d, term


def lpips64(p, t, seed, defect=None):
    """p, t (N, 3, H, W) fp32 in [-1, 1] (and beyond) -> (lpips (N), per layer (N, 5), bound terms (N, 5)), float64."""
    weights, biases, lins = weights64(seed)
    N = p.shape[0]
    xp, xt = inputs32(p, t, defect)
    taps = features64(torch.cat((xp, xt)), weights, biases, defect)
    layers, terms = [], []
    for f, w in zip(taps, lins):
        fp, ft = (f[0::2], f[1::2]) if defect == "mis_split" else (f[:N], f[N:])
        d, term = head64(fp, ft, w, defect)
        layers.append(d)
        terms.append(term)
    layers, terms = torch.stack(layers, 1), torch.stack(terms, 1)
    return layers.sum(1), layers, terms


def stem64(p, t, w, b):
    """relu1_1 of both images, float64 on the fp32 round-tripped input: ((2N, H, W, 64) values, the same shape of
    |b| + sum |w| |x| and of sum |w| |x| for the bound of tests/test_gpu_lpips.py).  p, t (N, H, W, 3) fp32; w, b fp32."""
    xp, xt = inputs32(p.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2))
    x = F.pad(scale64(torch.cat((xp, xt))), (1, 1, 1, 1))
    y = F.relu(F.conv2d(x, w.double(), b.double()))
    mag = F.conv2d(x.abs(), w.double().abs())
    full = mag + b.double().abs().view(1, -1, 1, 1)
    return y.permute(0, 2, 3, 1), full.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


# the end-to-end cases of tests/test_gpu_lpips.py: name -> (H, W, make_images keywords).  16 x 16 takes every map down to
# 1 x 1 and is a low-contrast grey pair: there the scaled zero a wrong padding order would put round the image
# (0.07 .. 0.42) is as large as the signal, which is what makes that defect visible in the distance at all (on a
# full-contrast pair it moves LPIPS by 1e-4 .. 2e-3 only).  20 x 28 pools in floor mode twice and has a target three times out of
# range, so that a clamp of the target would show.
CASES = {"16x16": (16, 16, {"low_contrast": True}), "20x28": (20, 28, {"target_gain": 3.0}), "64x48": (64, 48, {})}


def make_images(N, H, W, seed=0, identical=None, low_contrast=False, target_gain=1.0):
    """(p, t) (N, 3, H, W) fp32: a smooth pattern plus noise as the target, a damped and re-noised copy that leaves [-1, 1] in
    places as the prediction (low_contrast: a grey pair of amplitude 0.05 round -0.1 with noise 0.05 in both).  target_gain
    takes the target out of range.  `identical`: that image's prediction is its target, and the target is in range.
    Pure functions of the seed."""
    ys = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xs = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = syn.uniform((N, 3, 1, 1), seed, 0.0, 6.28, stream=1)
    pattern = torch.sin(7.0 * xs + 5.0 * ys + ph) * torch.cos(3.0 * ys - 2.0 * xs + 0.5 * ph)
    if low_contrast:
        t = 0.05 * pattern - 0.1 + syn.normal((N, 3, H, W), seed, 0.05, stream=2)
        p = t + syn.normal((N, 3, H, W), seed, 0.05, stream=3)
    else:
        t = (0.6 * pattern + syn.normal((N, 3, H, W), seed, 0.15, stream=2)).clamp(-1.0, 1.0)
        p = 1.15 * (0.9 * t + syn.normal((N, 3, H, W), seed, 0.1, stream=3))
    t = t * target_gain
    if identical is not None:
        t[identical] = t[identical].clamp(-1.0, 1.0)
        p[identical] = t[identical]
    return p.float().contiguous(), t.float().contiguous()


def make_maps(N, C, h, w, seed, scale=1.0):
    """Synthetic feature maps (2N, h, w, C) fp32 (predictions first; the targets are damped, re-noised predictions) and a
    non-negative lin weight (C)."""
    f = syn.normal((2 * N, h, w, C), seed, 1.0, stream=4)
    f[N:] = 0.8 * f[:N] + 0.3 * f[N:]
    return (f * scale).float().contiguous(), syn.uniform((C,), seed, stream=5)


def head64_nhwc(feat, lin, N):
    """head64 on a (2N, h, w, C) fp32 map as the kernel takes it."""
    f = feat.double().permute(0, 3, 1, 2)
    return head64(f[:N], f[N:], lin.double())
