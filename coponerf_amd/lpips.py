"""LPIPS (VGG) of the reference's evaluation script (test.py:149, 258-263), on the device and without the network.

test.py builds `lpips.LPIPS(net='vgg')` - the `lpips` package 0.1.x with version='0.1', lpips=True, spatial=False,
normalize=False - calls it per image and reads every value with `.item()`.  The package needs torchvision and fetches the
VGG16 weights when it is constructed.  Here

  LPIPS.from_files / from_state_dict   load the weights from files the USER owns: torchvision's `vgg16` state dict plus the
                                       package's `vgg.pth`, or one `lpips.LPIPS(net='vgg').state_dict()`.  Nothing is fetched;
                                       neither `lpips` nor torchvision is imported.
  LPIPS.synthetic(seed)                deterministic stand-in weights for tests and timing (no real weights ship with this
                                       package, and every number this repository quotes is on these)
  LPIPS.forward(p, t) -> (N,)          p, t (N, 3, H, W) in [-1, 1], as `Evaluator(extra={"lpips": lp})` hands them over

For images p, t:  p is clamped to [-1, 1]; both take the fp32 round trip (x + 1) * 0.5, (x01 - 0.5) * 2 of test.py:227-229,
258-259; the scaling layer (x - shift) / scale; torchvision's vgg16().features with taps after relu1_2, relu2_2, relu3_3,
relu4_3, relu5_3; per tap a = f_p / (sqrt(sum_c f_p^2) + 1e-10), b likewise, d_k = mean_pixels sum_c w_k[c] (a_c - b_c)^2;
the result is sum_k d_k.

  csrc/lpips.hip  cpn_lpips_stem   clamp, round trip, scaling layer, conv1_1 + bias + ReLU: one launch, NHWC out
  library ops                      conv1_2 .. conv5_3 and the four pools in fp32 on the 2N batch (predictions and targets
                                   together), in NCHW memory: one copy of relu1_1 in, one channels-last copy of each of the
                                   five tapped maps out (`get_z` keeps the library on its deterministic
                                   algorithms during inference, and for channels_last those are 130 x slower than these)
  csrc/lpips.hip  cpn_lpips_head   the whole distance head, all five layers and all images: two launches

`forward` runs under `torch.no_grad()`, reads nothing on the host and touches no global backend flag.

  LPIPS.differentiable(p, t) -> (N,)   the same distance as a training term: the gradient flows to p only.
                                       The stem and the head are autograd Functions over cpn_lpips_stem / cpn_lpips_stem_bwd and
                                       cpn_lpips_head / cpn_lpips_head_bwd; between them the library's convolutions and pools
                                       run under autograd on the N predictions (data gradients only: the weights are buffers)
                                       and under no_grad on the N targets.  A pixel of a tapped map whose channels are all 0
                                       gets gradient 0 (this package's rule; float64 autograd of normalize_tensor gives NaN).
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _hip
from . import synthetic as syn

CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)        # the convolutions of vgg16().features
CONV_CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
                 (512, 512), (512, 512), (512, 512))
BLOCKS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))     # a 2 x 2 max pool before every block but the first
TAP_CHANNELS = (64, 128, 256, 512, 512)                                # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LAYERS = _hip.LPIPS_LAYERS
MIN_SIDE = 16                                                          # four pools must leave a pixel


def _slice_of(i: int) -> int:
    """The package's `net.slice{j}` that holds index i of `features` (slices end after 3, 8, 15, 22, 29)."""
    return 1 + sum(i > end for end in (3, 8, 15, 22))


def synthetic_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Stand-in weights in torchvision's key layout plus the `lin` layers: convolutions N(0, 2 / (9 Cin)), biases N(0, 0.05^2),
    `lin` uniform in [0, 1) as (1, C, 1, 1) (real ones are non-negative; this puts the distances near 0.1, where real LPIPS
    values lie).  A pure function of the seed (coponerf_amd.synthetic), shared with the float64 restatement of the tests."""
    sd: Dict[str, torch.Tensor] = {}
    for n, (i, (cin, cout)) in enumerate(zip(CONV_INDICES, CONV_CHANNELS)):
        sd[f"features.{i}.weight"] = syn.normal((cout, cin, 3, 3), seed, math.sqrt(2.0 / (9 * cin)), stream=2 * n)
        sd[f"features.{i}.bias"] = syn.normal((cout,), seed, 0.05, stream=2 * n + 1)
    for k, c in enumerate(TAP_CHANNELS):
        sd[f"lin{k}.model.1.weight"] = syn.uniform((1, c, 1, 1), seed, stream=100 + k)
    return sd


def _tensor(sd: Dict, key: str, shape: Tuple[int, ...]) -> torch.Tensor:
    if key not in sd:
        raise ValueError(f"LPIPS: the state dict has no {key!r}")
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != shape:
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"LPIPS: {key!r} must have shape {shape}, got {got}")
    return t.detach().to(torch.float32)


def parse_state_dict(vgg: Dict, lin: Optional[Dict] = None) -> Tuple[List[torch.Tensor], List[torch.Tensor], List[torch.Tensor]]:
    """(conv weights (Cout, Cin, 3, 3), conv biases, lin weights (C,)) as fp32 CPU tensors from either accepted layout:
    torchvision's `features.{i}.weight/bias` with the package's `lin{k}.model.1.weight` (in `lin`, or in `vgg` itself), or the
    package's own `net.slice{j}.{i}.weight/bias` + `lin{k}.model.1.weight`.  `lins.{k}.*` (the same tensors under a second name)
    and `scaling_layer.*` (constants) are ignored."""
    full = any(str(k).startswith("net.slice") for k in vgg)
    lin = vgg if lin is None else lin
    weights, biases, lins = [], [], []
    for i, (cin, cout) in zip(CONV_INDICES, CONV_CHANNELS):
        stem = f"net.slice{_slice_of(i)}.{i}" if full else f"features.{i}"
        weights.append(_tensor(vgg, stem + ".weight", (cout, cin, 3, 3)))
        biases.append(_tensor(vgg, stem + ".bias", (cout,)))
    for k, c in enumerate(TAP_CHANNELS):
        key = f"lin{k}.model.1.weight"
        if key in lin and torch.is_tensor(lin[key]) and tuple(lin[key].shape) == (c,):
            lins.append(_tensor(lin, key, (c,)))
        else:
            lins.append(_tensor(lin, key, (1, c, 1, 1)).reshape(c))
    return weights, biases, lins


class LPIPS(torch.nn.Module):
    """`fn(p, t) -> (N,)` for `Evaluator(extra={"lpips": fn})`; see the module docstring.  The weights are buffers: `.to(dev)`
    moves them, nothing trains."""

    def __init__(self, weights: List[torch.Tensor], biases: List[torch.Tensor], lins: List[torch.Tensor]):
        super().__init__()
        if len(weights) != len(CONV_INDICES) or len(biases) != len(CONV_INDICES) or len(lins) != LAYERS:
            raise ValueError("LPIPS: 13 convolution weights, 13 biases and 5 lin weights")
        self.register_buffer("stem_weight", weights[0].contiguous().clone())
        self.register_buffer("stem_bias", biases[0].contiguous().clone())
        for i, w, b in zip(CONV_INDICES[1:], weights[1:], biases[1:]):
            self.register_buffer(f"w{i}", w.contiguous().clone())
            self.register_buffer(f"b{i}", b.contiguous().clone())
        for k, l in enumerate(lins):
            self.register_buffer(f"lin{k}", l.contiguous().clone())

    # ------------------------------------------------------------------------------------------------------- loading
    @classmethod
    def from_state_dict(cls, vgg: Dict, lin: Optional[Dict] = None) -> "LPIPS":
        return cls(*parse_state_dict(vgg, lin))

    @classmethod
    def from_files(cls, vgg_path: str, lin_path: Optional[str] = None) -> "LPIPS":
        """vgg_path: torchvision's vgg16 state dict (then lin_path: the package's weights/v0.1/vgg.pth), or the state dict of
        a whole lpips.LPIPS(net='vgg').  Local files only."""
        vgg = torch.load(vgg_path, weights_only=True, map_location="cpu")
        lin = torch.load(lin_path, weights_only=True, map_location="cpu") if lin_path is not None else None
        return cls.from_state_dict(vgg, lin)

    @classmethod
    def synthetic(cls, seed: int = 0) -> "LPIPS":
        return cls.from_state_dict(synthetic_state_dict(seed))

    # ------------------------------------------------------------------------------------------------------- forward
    @staticmethod
    def _channels_last(x: torch.Tensor) -> torch.Tensor:
        """(N, 3, H, W) -> its (N, H, W, 3) memory: the hook's permuted view as it is, anything else through one copy."""
        return x.permute(0, 2, 3, 1).contiguous()           # no copy when the view is contiguous already

    def trunk(self, x: torch.Tensor) -> List[torch.Tensor]:
        """relu1_1 (2N, 64, H, W), in the channels_last memory the stem leaves it in (or any other) -> the five tapped maps as
        contiguous (2N, h, w, C).  The convolutions run in NCHW: one copy of relu1_1 on the way in, one channels-last copy of
        every tapped map on the way out."""
        return [f.permute(0, 2, 3, 1).contiguous() for f in self._trunk_nchw(x)]

    def _trunk_nchw(self, x: torch.Tensor) -> List[torch.Tensor]:
        """The five tapped maps as the convolutions leave them, (n, C, h, w) contiguous.  Runs under autograd as it stands: every
        in-place ReLU acts on a convolution's fresh output."""
        x = x.contiguous()
        taps = []
        for j, block in enumerate(BLOCKS):
            if j:
                x = F.max_pool2d(x, 2, 2)
            for i in block:
                if i == 0:
                    continue                                # conv1_1 is the stem kernel's
                x = F.relu_(F.conv2d(x, getattr(self, f"w{i}"), getattr(self, f"b{i}"), padding=1))
            taps.append(x)
        return taps

    def stem(self, p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """p, t (N, H, W, 3) contiguous -> relu1_1 of both as (2N, 64, H, W), a view of the kernel's (2N, H, W, 64) output."""
        N, H, W, _ = p.shape
        out = torch.empty(2 * N, H, W, 64, dtype=torch.float32, device=p.device)
        _hip.call("cpn_lpips_stem", p.data_ptr(), t.data_ptr(), self.stem_weight.data_ptr(), self.stem_bias.data_ptr(), N, H, W,
                  out.data_ptr(), _hip.stream_handle())
        return out.permute(0, 3, 1, 2)

    def head(self, taps: List[torch.Tensor], N: int, per_layer: bool = False):
        """taps[k] (2N, h_k, w_k, C_k) fp32, predictions first -> (N,), and (N, 5) with per_layer."""
        return lpips_head(taps, [getattr(self, f"lin{k}") for k in range(len(taps))], N, per_layer)

    def _check(self, p: torch.Tensor, t: torch.Tensor) -> None:
        if not (torch.is_tensor(p) and torch.is_tensor(t)):
            raise TypeError("LPIPS: p and t must be tensors")
        if not (p.is_cuda and t.is_cuda):
            raise RuntimeError("LPIPS runs on the HIP device only (coponerf_amd has no non-HIP compute path)")
        if p.device != t.device or p.device != self.stem_weight.device:
            raise ValueError(f"LPIPS: p on {p.device}, t on {t.device}, weights on {self.stem_weight.device}")
        if p.dtype != torch.float32 or t.dtype != torch.float32:
            raise ValueError(f"LPIPS: fp32 tensors only, got {p.dtype} and {t.dtype}")
        if p.dim() != 4 or p.shape[1] != 3 or p.shape != t.shape or p.shape[0] < 1:
            raise ValueError(f"LPIPS: two (N, 3, H, W) batches, got {tuple(p.shape)} and {tuple(t.shape)}")
        N, _, H, W = p.shape
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"LPIPS: four 2 x 2 pools need H, W >= {MIN_SIDE}, got {H} x {W}")

    @torch.no_grad()
    def forward(self, p: torch.Tensor, t: torch.Tensor, per_layer: bool = False):
        self._check(p, t)
        with torch.cuda.device(p.device):
            x = self.stem(self._channels_last(p), self._channels_last(t))
            return self.head(self.trunk(x), p.shape[0], per_layer)

    # ------------------------------------------------------------------------------------------------ as a training term
    def differentiable(self, p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """forward's inputs, checks and values (within its float64 bounds; not its bits: the library may pick another
        algorithm for N images than for 2N) with a gradient to p.  t gets none.  Reads nothing on the host."""
        self._check(p, t)
        with torch.cuda.device(p.device):
            yp, yt = _Stem.apply(self._channels_last(p), self._channels_last(t.detach()), self.stem_weight, self.stem_bias)
            taps_p = self._trunk_nchw(yp.permute(0, 3, 1, 2))
            with torch.no_grad():
                taps_t = self._trunk_nchw(yt.permute(0, 3, 1, 2))
            return _Head.apply([getattr(self, f"lin{k}") for k in range(LAYERS)], taps_t, *taps_p)


def _head_args(who: str, taps: List[torch.Tensor], lins: List[torch.Tensor], N: int):
    """The checks and the host arrays the head and its adjoint share: (layers, device, the pointer-array type, (C, h, w) int arrays)."""
    L = len(taps)
    if not 1 <= L <= LAYERS or len(lins) != L:
        raise ValueError(f"{who}: 1 .. {LAYERS} maps and as many lin weights, got {L} and {len(lins)}")
    dev = taps[0].device
    for k, (f, l) in enumerate(zip(taps, lins)):
        if not (f.is_cuda and l.is_cuda) or f.device != dev or l.device != dev:
            raise RuntimeError(f"{who} runs on one HIP device only (coponerf_amd has no non-HIP compute path)")
        if f.dtype != torch.float32 or l.dtype != torch.float32 or f.dim() != 4 or f.shape[0] != 2 * N or not f.is_contiguous():
            raise ValueError(f"{who}: map {k} must be a contiguous fp32 (2N, h, w, C), got {tuple(f.shape)} {f.dtype}")
        if tuple(l.shape) != (f.shape[3],) or not l.is_contiguous():
            raise ValueError(f"{who}: lin {k} must be ({f.shape[3]},), got {tuple(l.shape)}")
    ints = ctypes.c_int * L
    return L, dev, ctypes.c_void_p * L, tuple(ints(*[f.shape[d] for f in taps]) for d in (3, 1, 2))


def lpips_head(taps: List[torch.Tensor], lins: List[torch.Tensor], N: int, per_layer: bool = False):
    """csrc/lpips.hip's distance head alone: taps[k] (2N, h_k, w_k, C_k) contiguous fp32 on the device, predictions first,
    lins[k] (C_k).  Returns (N,) fp32, and the (N, 5) per-layer terms with per_layer.  Two launches, no host read."""
    L, dev, ptrs, (cs, hs, ws) = _head_args("lpips_head", taps, lins, N)
    n = _hip.lib().cpn_lpips_head_scratch(N, L, hs, ws)
    if n <= 0:
        raise ValueError(f"lpips_head: {N} images with maps {[tuple(f.shape[1:3]) for f in taps]} are not one launch")
    partial = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    layers = torch.empty(N, LAYERS, dtype=torch.float32, device=dev) if per_layer else None
    with torch.cuda.device(dev):
        _hip.call("cpn_lpips_head", ptrs(*[f.data_ptr() for f in taps]), ptrs(*[l.data_ptr() for l in lins]), cs, hs, ws, L, N,
                  partial.data_ptr(), out.data_ptr(), layers.data_ptr() if per_layer else None, _hip.stream_handle())
    return (out, layers) if per_layer else out


class _Stem(torch.autograd.Function):
    """cpn_lpips_stem on (N, H, W, 3) channels-last images -> relu1_1 of the predictions and of the targets, both (N, H, W, 64)
    halves of the kernel's one output.  Differentiable in the predictions (cpn_lpips_stem_bwd)."""

    @staticmethod
    def forward(ctx, p, t, weight, bias):
        N, H, W, _ = p.shape
        out = torch.empty(2 * N, H, W, 64, dtype=torch.float32, device=p.device)
        _hip.call("cpn_lpips_stem", p.data_ptr(), t.data_ptr(), weight.data_ptr(), bias.data_ptr(), N, H, W, out.data_ptr(),
                  _hip.stream_handle())
        yp, yt = out[:N], out[N:]
        ctx.save_for_backward(p, yp, weight)
        ctx.mark_non_differentiable(yt)
        return yp, yt

    @staticmethod
    def backward(ctx, dyp, _dyt):
        p, yp, weight = ctx.saved_tensors
        N, H, W, _ = p.shape
        dy = dyp.contiguous()
        dp = torch.empty_like(p)
        with torch.cuda.device(p.device):
            _hip.call("cpn_lpips_stem_bwd", dy.data_ptr(), yp.data_ptr(), p.data_ptr(), weight.data_ptr(), N, H, W, dp.data_ptr(),
                      _hip.stream_handle())
        return dp, None, None, None


class _Head(torch.autograd.Function):
    """(N,) distances of the tapped maps as the convolutions leave them: taps_p[k], taps_t[k] (N, C_k, h_k, w_k).  Forward: one
    channels-last (2N, h, w, C) buffer per layer, filled by one copy per half, and cpn_lpips_head; backward: cpn_lpips_head_bwd,
    its channels-last result copied to the convolutions' layout.  Differentiable in taps_p only."""

    @staticmethod
    def forward(ctx, lins, taps_t, *taps_p):
        N = taps_p[0].shape[0]
        both = []
        for fp, ft in zip(taps_p, taps_t):
            f = torch.empty(2 * N, fp.shape[2], fp.shape[3], fp.shape[1], dtype=torch.float32, device=fp.device)
            f[:N].copy_(fp.permute(0, 2, 3, 1))
            f[N:].copy_(ft.permute(0, 2, 3, 1))
            both.append(f)
        ctx.save_for_backward(*both, *lins)
        return lpips_head(both, list(lins), N)

    @staticmethod
    def backward(ctx, g):
        L = len(ctx.saved_tensors) // 2
        both, lins = ctx.saved_tensors[:L], ctx.saved_tensors[L:]
        return (None, None) + tuple(d.permute(0, 3, 1, 2).contiguous() for d in lpips_head_bwd(both, lins, g))


def lpips_head_bwd(taps: List[torch.Tensor], lins: List[torch.Tensor], g: torch.Tensor) -> List[torch.Tensor]:
    """csrc/lpips.hip's adjoint of the distance head alone: taps and lins as lpips_head takes them, g (N,) the gradient of
    every image's distance.  Returns the gradients of the prediction halves, (N, h_k, w_k, C_k) fp32.  One launch, no host read.
    A pixel whose prediction vector is all zeros gets 0 (include/coponerf_hip.h)."""
    N = g.shape[0]
    L, dev, ptrs, (cs, hs, ws) = _head_args("lpips_head_bwd", taps, lins, N)
    g = g.contiguous()
    if not g.is_cuda or g.device != dev or g.dtype != torch.float32 or g.dim() != 1:
        raise ValueError(f"lpips_head_bwd: g must be fp32 (N,) on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
    grads = [torch.empty(N, *f.shape[1:], dtype=torch.float32, device=dev) for f in taps]
    with torch.cuda.device(dev):
        _hip.call("cpn_lpips_head_bwd", ptrs(*[f.data_ptr() for f in taps]), ptrs(*[l.data_ptr() for l in lins]), cs, hs, ws, L, N,
                  g.data_ptr(), ptrs(*[d.data_ptr() for d in grads]), _hip.stream_handle())
    return grads
