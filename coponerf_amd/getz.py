"""get_z: image encoder -> UFC joint feature / 4-D cost-volume aggregation -> pose head.

Restates `CoPoNeRF.get_z` (/root/reference models/CoPoNeRF.py:159-206) with the reference's parameter names
(checkpoint contract):

  encoder.*                   ResNet-34 trunk, no first max-pool (models/backbone.py:10-102)          stock ops
  conv_map                    7x7 conv on the normalised image (CoPoNeRF.py:69,187)                    HIP (cpn_conv_map7x7)
  feature_cost_aggregation.*  UFC (models/aggregation.py:146-562, models/conv4d.py:57-163)            in scope (§8 a22-a29)
  cross_attention.*           CrossBlock / "fundamental-matrix" attention (models/backbone.py:280-428) stock ops
  pose/rotation/translation_regressor                                                               stock ops

The 4-D operators that dominate UFC (Conv4d + GroupNorm + ReLU, cosine correlation, soft-argmax) go through an
`ops` object: `HipOps` binds the gfx950 kernels of libcoponerf_hip.so, and the test oracle binds its own CPU
restatement (oracle/ufc_ref.py) to pin this glue code against fixtures of the upstream model.  Everything else is
plain PyTorch-ROCm module code, exactly the kind of op the reference itself calls.  256x256 inputs only, like the
reference (UFC feat_size 16/32/64, learned pos_embed, pose head input size).
"""
from __future__ import annotations

import math
import os
from typing import Sequence, Tuple

import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import stream_handle as _stream_handle

from .ufc_ops import Linear as _Linear, linear as _linear      # nn.Linear / F.linear with the training dW on cpn_wgrad_f32


# ----------------------------------------------------------------------------------------------
# ResNet-34 trunk with torchvision-compatible parameter names (encoder.model.*)
# ----------------------------------------------------------------------------------------------
class _TrunkBatchNorm(nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters, buffers and training-mode arithmetic) whose `num_batches_tracked` counter is not
    bumped layer by layer: in training each bump is a launch of its own (36 per trunk pass); inside SpatialEncoder.forward
    the modules that ran are noted (per thread) and `flush_counters()` advances all their counters with ONE multi-tensor add."""
    _tls = threading.local()            # per thread: replicas driven from several threads keep their own lists

    def forward(self, x):
        if not (self.training and self.track_running_stats) or self.momentum is None:
            return super().forward(x)
        pend = getattr(_TrunkBatchNorm._tls, "pending", None)
        if pend is None:                # used outside SpatialEncoder.forward (nobody would flush): the stock behaviour
            return super().forward(x)
        pend.append(self.num_batches_tracked)
        return F.batch_norm(x, self.running_mean, self.running_var, self.weight, self.bias, True, self.momentum, self.eps)

    @staticmethod
    def collect_counters():
        """Start noting the counters of the modules that run on this thread (SpatialEncoder.forward, training mode)."""
        _TrunkBatchNorm._tls.pending = []

    @staticmethod
    def flush_counters():
        pend, _TrunkBatchNorm._tls.pending = getattr(_TrunkBatchNorm._tls, "pending", None), None
        if pend:
            with torch.no_grad():
                torch._foreach_add_(pend, 1)


class TrunkBackward:
    """Training: data and weight gradient of the trunk's 3x3 / 1x1 convolutions with fp16 operands (fp32 accumulation in the
    library's implicit-GEMM kernels), every layer's incoming gradient scaled by a power of two found on the device
    (cpn_scale_to_f16).  The forward stays fp32.  tools/conv_bwd_precision_bench.py, 8 images of 256 x 256: 6.8 -> 4.6 ms
    for the 36 layers including the casts; each layer's dx / dw within 8e-4 / 1.4e-3 (relative L2) of the fp32 kernels' — a
    tenth of what the forward's fp16 operands already leave upstream of z (tests/test_gpu_step.py).

    One per SpatialEncoder, shared by its blocks.  enabled: this backward (CPN_TRUNK_BWD_F16=0: the library's fp32 one);
    target: where each layer's largest |dy| lands, moved by `after_step`; trace: set to a list to collect (x shape,
    max |dx16|, max |dw16|) per layer (device scalars, no sync)."""

    def __init__(self):
        self.enabled = os.environ.get("CPN_TRUNK_BWD_F16", "1") != "0"
        self.target = 4.0
        self.trace = None

    def after_step(self, stepped: bool) -> None:
        """Called with the outcome of every optimizer step (coponerf_amd.train_step): non-finite gradients quarter the target
        (an overflowing dw / dx would otherwise repeat for ever), a finite step doubles it back towards 4."""
        # floor 2^-4: 64 x more room than the 146 x of target 4 — beyond that an overflow here is not what made the step
        # non-finite, and a smaller target only pushes the small entries of dy into fp16's subnormals
        self.target = min(4.0, self.target * 2.0) if stepped else max(2.0 ** -4, self.target * 0.25)


class _ScaleSlots:
    """[amax bits, scale, 1 / scale] triples for cpn_scale_to_f16, zero when handed out: one fill per 128 layers."""
    _pools = {}

    @classmethod
    def take(cls, dev):
        pool = cls._pools.get(dev)
        if pool is None or pool[1] == 128:
            pool = cls._pools[dev] = [torch.zeros(128, 4, dtype=torch.float32, device=dev), 0]
        pool[1] += 1
        return pool[0][pool[1] - 1]


class _ConvF16BwdFn(torch.autograd.Function):
    """F.conv2d(x, w, None, stride, padding) whose backward runs on fp16 operands (see TrunkBackward)."""

    @staticmethod
    def forward(ctx, x, w, stride, padding, state: TrunkBackward):
        ctx.save_for_backward(x, w)
        ctx.geo, ctx.state = (int(stride), int(padding)), state
        return F.conv2d(x, w, None, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        from ._hip import call
        x, w = ctx.saved_tensors
        st, pd = ctx.geo
        # (in training the trunk runs channels-last: the stem's input is an NHWC-strided view of the images.  The scale + cast
        # pass is elementwise over dense memory, whichever of the two layouts it is)
        if not (dy.is_contiguous() or dy.is_contiguous(memory_format=torch.channels_last)):
            dy = dy.contiguous()
        if dy.numel() % 4:                                     # cpn_scale_to_f16 works on 16-byte pieces
            return tuple(torch.ops.aten.convolution_backward(dy, x, w, None, [st, st], [pd, pd], [1, 1], False, [0, 0], 1,
                                                             [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False])[:2]) + (None,) * 3
        slot = _ScaleSlots.take(dy.device)
        dy16 = torch.empty_like(dy, dtype=torch.float16)       # keeps dy's layout
        # the largest |dy| lands in [target / 2, target]: dx and dw come back as fp16 tensors, and dw sums dy . x over up to
        # 131 072 positions per image batch — at target 64 its largest entry reached 7 160 of fp16's 65 504 on the synthetic
        # step (tools/trunk_bwd_headroom.py); at 4 there are two decades of room, and entries down to 1.5e-5 of the largest
        # keep all their bits.  A skipped step backs the target off further (TrunkBackward.after_step, called by TrainStep).
        call("cpn_scale_to_f16", dy.data_ptr(), dy.numel(), float(ctx.state.target), slot.data_ptr(), dy16.data_ptr(),
             slot[1:].data_ptr(), _stream_handle())
        need = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], False]
        dx16, dw16, _ = torch.ops.aten.convolution_backward(dy16, x.half(), w.half(), None, [st, st], [pd, pd], [1, 1], False,
                                                            [0, 0], 1, need)
        if ctx.state.trace is not None:                        # tests / tools: the largest fp16 entries, still on the device
            ctx.state.trace.append((tuple(x.shape), dx16.abs().max() if need[0] else None, dw16.abs().max() if need[1] else None))
        inv = slot[2:3]                                        # 1-d fp32: the product is fp32
        dw = None
        if need[1]:
            # the library returns dw in the activations' layout (channels-last in training): the parameter's gradient is
            # written contiguous, or the norm / clip / Adam passes over the gradients fall off their multi-tensor paths
            dw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
            torch.mul(dw16, inv, out=dw)
        return (dx16 * inv if need[0] else None), dw, None, None, None


def _conv(conv: nn.Conv2d, x, state: TrunkBackward):
    if (state.enabled and x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled() and conv.bias is None
            and x.numel() % 4 == 0 and (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last))):
        return _ConvF16BwdFn.apply(x, conv.weight, conv.stride[0], conv.padding[0], state)
    return conv(x)


class _BasicBlock(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int, trunk_bwd: TrunkBackward):
        super().__init__()
        self.trunk_bwd = trunk_bwd
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = _TrunkBatchNorm(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = _TrunkBatchNorm(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), _TrunkBatchNorm(cout))

    def forward(self, x):
        st = self.trunk_bwd
        idt = x if self.downsample is None else self.downsample[1](_conv(self.downsample[0], x, st))
        out = self.bn2(_conv(self.conv2, self.relu(self.bn1(_conv(self.conv1, x, st))), st))
        return self.relu(out + idt)


class _ResNet34Trunk(nn.Module):
    def __init__(self, trunk_bwd: TrunkBackward):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = _TrunkBatchNorm(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for i, (cout, n, s) in enumerate([(64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)], start=1):
            setattr(self, f"layer{i}", nn.Sequential(*[_BasicBlock(cin if j == 0 else cout, cout, s if j == 0 else 1, trunk_bwd)
                                                       for j in range(n)]))
            cin = cout
        self.avgpool = nn.Sequential()      # the reference replaces both by empty Sequentials (backbone.py:56-57)
        self.fc = nn.Sequential()


def _bn_act(x, bn, relu: bool, res=None):
    """Inference BatchNorm (+ residual) (+ ReLU) in place on the convolution's output: cpn_bn_act (csrc/encoder.hip)."""
    from ._hip import call
    N, C, H, W = x.shape
    if not x.is_contiguous() or (H * W) % 4 or (res is not None and not res.is_contiguous()):
        y = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)   # e.g. channels-last
        y = y if res is None else y + res
        return F.relu(y) if relu else y
    call("cpn_bn_act", x.data_ptr(), 0 if res is None else res.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
         bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), N, C, H * W, int(relu), x.data_ptr(),
         _stream_handle())
    return x


def _trunk_conv(xh, conv, bn, relu: bool, res=None, want_nchw: bool = False):
    """conv (3x3 / 1x1, no bias) + inference batch norm (+ residual) (+ ReLU) on an NHWC fp32 map: cpn_trunk_conv_bn_act
    (csrc/trunk_conv.hip).  Returns the NHWC result and, if asked for, the NCHW copy the same epilogue writes."""
    from ._hip import call, lib
    N, H, W, Cin = xh.shape
    Cout, k, s = conv.out_channels, conv.kernel_size[0], conv.stride[0]
    w = conv.weight
    pack = conv.__dict__.get("_cpn_pack")
    if pack is None or pack[0] != (w._version, w.data_ptr()):
        wp = torch.empty(k * k, Cin, Cout, dtype=torch.float32, device=xh.device)
        call("cpn_pack_conv_weight", w.detach().contiguous().data_ptr(), Cout, Cin, k, wp.data_ptr(),
             _stream_handle())
        pack = conv.__dict__["_cpn_pack"] = ((w._version, w.data_ptr()), wp)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    out = torch.empty(N, Ho, Wo, Cout, dtype=torch.float32, device=xh.device)
    nchw = torch.empty(N, Cout, Ho, Wo, dtype=torch.float32, device=xh.device) if want_nchw else None
    scratch = torch.empty(lib().cpn_trunk_conv_scratch_floats(N, H, W, Cin, Cout, k, s), dtype=torch.float32, device=xh.device)
    call("cpn_trunk_conv_bn_act", xh.data_ptr(), pack[1].data_ptr(), N, H, W, Cin, Cout, k, s, bn.running_mean.data_ptr(),
         bn.running_var.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps),
         0 if res is None else res.data_ptr(), int(relu), out.data_ptr(), 0 if nchw is None else nchw.data_ptr(),
         scratch.data_ptr(), _stream_handle())
    return out, nchw


class SpatialEncoder(nn.Module):
    """backbone.py:10-102 with use_first_pool=False, num_layers=5: returns [512@H/16, 256@H/8, 128@H/4, 64@H/2, 64@H/2]."""

    def __init__(self):
        super().__init__()
        self.trunk_bwd = TrunkBackward()            # not a parameter or buffer: state_dict is unchanged
        self.model = _ResNet34Trunk(self.trunk_bwd)

    def _forward_infer(self, x):
        """eval() + no_grad on the GPU: library convolutions, each followed by ONE pass for batch norm, residual and ReLU
        (the library takes three launches: 85 -> 36 per get_z)."""
        m = self.model
        x = _bn_act(m.conv1(x), m.bn1, True)
        lat = [x]
        xh = None                                        # NHWC copy of x once the own kernels take over
        for name in ("layer1", "layer2", "layer3", "layer4"):
            blocks = list(getattr(m, name))
            own = (HIP_TRUNK_TAIL and name in ("layer3", "layer4")
                   and x.shape[0] * (x.shape[2] // 2) * (x.shape[3] // 2) <= HIP_TRUNK_MAX_POSITIONS)
            if own and xh is None:
                xh = x.permute(0, 2, 3, 1).contiguous()
            for i, blk in enumerate(blocks):
                if own:
                    # split-K implicit GEMMs with the normalisation in their epilogue (csrc/trunk_conv.hip)
                    idt = xh
                    if blk.downsample is not None:
                        idt, _ = _trunk_conv(xh, blk.downsample[0], blk.downsample[1], False)
                    out, _ = _trunk_conv(xh, blk.conv1, blk.bn1, True)
                    xh, xn = _trunk_conv(out, blk.conv2, blk.bn2, True, res=idt, want_nchw=i == len(blocks) - 1)
                    x = xn if xn is not None else x
                    continue
                xh = None
                idt = x
                if blk.downsample is not None:
                    idt = _bn_act(blk.downsample[0](x), blk.downsample[1], False)
                out = _bn_act(blk.conv1(x), blk.bn1, True)
                x = _bn_act(blk.conv2(out), blk.bn2, True, res=idt)
            lat.append(x)
        return lat[::-1]

    def forward(self, x):
        m = self.model
        if (not torch.is_grad_enabled() and not self.training and x.is_cuda and x.dtype == torch.float32
                and x.is_contiguous() and FUSED_TRUNK):
            return self._forward_infer(x)
        _TrunkBatchNorm.collect_counters()
        try:
            x = m.relu(m.bn1(m.conv1(x)))
            lat = [x]
            for name in ("layer1", "layer2", "layer3", "layer4"):
                x = getattr(m, name)(x)
                lat.append(x)
        finally:
            _TrunkBatchNorm.flush_counters()
        return lat[::-1]


# ----------------------------------------------------------------------------------------------
# 4-D operators: parameter containers + dispatch to `ops`
# ----------------------------------------------------------------------------------------------
class Conv4d(nn.Module):
    """Parameters of conv4d.Conv4d (conv4d.py:57-135): two 2-D kernels, one over the query pair of dims, one over
    the support pair; with stride > 1 the other pair is max-pooled (kernel = stride, ceil_mode)."""

    def __init__(self, cin: int, cout: int, k: int, s: int, p: int):
        super().__init__()
        self.query_conv = nn.Conv2d(cin, cout, (k, k), stride=(s, s), padding=(p, p))
        self.supp_conv = nn.Conv2d(cin, cout, (k, k), stride=(s, s), padding=(p, p))
        self.k, self.s, self.p = k, s, p


class Encoder4D(nn.Module):
    """conv4d.Encoder4D (conv4d.py:138-163): [Conv4d -> GroupNorm(1 group) -> ReLU] x n."""

    def __init__(self, levels: Sequence[int], k: int = 3, s: int = 1, p: int = 1):
        super().__init__()
        self.conv4d = nn.ModuleList([
            nn.Sequential(Conv4d(levels[i], levels[i + 1], k, s, p), nn.GroupNorm(1, levels[i + 1]), nn.ReLU())
            for i in range(len(levels) - 1)])

    def forward(self, x, ops, residual=None):
        """residual: what the caller adds to the stack's output (`x + Encoder4D(x)`), handed to the last block so that
        operators that can fold it into their normalisation pass do."""
        last = len(self.conv4d) - 1
        for i, blk in enumerate(self.conv4d):
            c4, gn = blk[0], blk[1]
            args = (x, c4.query_conv.weight, c4.query_conv.bias, c4.supp_conv.weight, c4.supp_conv.bias, c4.k, c4.s, c4.p,
                    gn.weight, gn.bias, gn.eps)
            x = ops.conv4d_gn_relu(*args, residual=residual) if (i == last and residual is not None) else ops.conv4d_gn_relu(*args)
        return x


class _DWConv(nn.Module):
    def __init__(self, dim: int, size: int):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)
        self.size = size

    def forward(self, x):                       # (B, L, C) tokens
        B, L, C = x.shape
        if x.is_cuda and x.dtype == torch.float32 and C % 4 == 0:
            from .ufc_ops import DwConvTokensFn            # the convolution on the token layout itself (csrc/ufc_wgrad.hip)
            return DwConvTokensFn.apply(x, self.dwconv.weight, self.dwconv.bias, self.size)
        xm = x.transpose(1, 2).reshape(B, C, self.size, self.size)
        y = self.dwconv(xm)
        return y.flatten(2).transpose(1, 2)


TWO_STREAMS = os.environ.get("CPN_GETZ_TWO_STREAMS", "1") != "0"
# source and target passes of every UFC layer as one batched pass (UFCLayer._forward_views_batched); 0 = one after the other
BATCH_VIEWS = os.environ.get("CPN_GETZ_BATCH_VIEWS", "1") != "0"
# inference trunk: batch norm + residual + ReLU behind every convolution as one kernel (SpatialEncoder._forward_infer)
FUSED_TRUNK = os.environ.get("CPN_GETZ_FUSED_TRUNK", "1") != "0"
# ... and layer3 / layer4 on the package's own split-K convolution (cpn_trunk_conv_bn_act) while the maps are small enough for
# the library's kernels to leave the chip idle: output positions of the layer over all images (one 256 x 256 pair: 2 048 at
# layer3, 512 at layer4; tools/trunk_conv_bench.py: at 4 096 positions the library's 3x3 stride-1 kernel is ahead)
HIP_TRUNK_TAIL = os.environ.get("CPN_GETZ_HIP_TRUNK_TAIL", "1") != "0"
# inference: positional encodings of the pose head and its regressor tail as one kernel each (csrc/pose.hip)
FUSED_POSE_ENDS = os.environ.get("CPN_GETZ_FUSED_POSE_ENDS", "1") != "0"
HIP_TRUNK_MAX_POSITIONS = int(os.environ.get("CPN_GETZ_HIP_TRUNK_MAX_POSITIONS", "2048"))
# training: the final correlation on cpn_corr_mean3 with its own adjoint (ufc_ops._CorrMean3Fn); 0 = composed resize ops
CORR_MEAN3_TRAIN = os.environ.get("CPN_CORR_MEAN3_TRAIN", "1") != "0"
_SIDE_STREAMS = {}


def _side_stream(device):
    st = _SIDE_STREAMS.get(device)
    if st is None:
        st = _SIDE_STREAMS[device] = torch.cuda.Stream(device=device)
    return st


def _tokens_to_map(x, h):
    B, L, C = x.shape
    return x.transpose(1, 2).reshape(B, C, h, L // h)


def _map_to_tokens(x):
    return x.flatten(2).transpose(1, 2)


def _corr_to_maps(corr):
    """(B,H,Hs,Ws,Ht,Wt) -> (B, H*Ht*Wt, Hs, Ws)."""
    B, H, Hs, Ws, Ht, Wt = corr.shape
    from .ufc_ops import swap_pairs
    return swap_pairs(corr).reshape(B, H * Ht * Wt, Hs, Ws)


class UFCLayer(nn.Module):
    """aggregation.UFCLayer (aggregation.py:146-356)."""

    def __init__(self, fs: int, f2c: Tuple[int, int, int], nhead: int = 8, d: int = 256):
        super().__init__()
        self.fs, self.nhead, self.dim = fs, nhead, d // nhead
        self.q_proj = _Linear(d + 256 * nhead, d)
        self.k_proj = _Linear(d + 256 * nhead, d)
        self.v_proj = _Linear(d, d)
        self.v_proj_corr = Encoder4D((nhead, nhead))
        self.mlp = nn.Sequential(_Linear(d, 4 * d), _DWConv(4 * d, fs), nn.GELU(), _Linear(4 * d, d))
        self.mlp_corr = Encoder4D((nhead, 4 * nhead, nhead))
        self.mlp_cross = nn.Sequential(_Linear(d, 4 * d), _DWConv(4 * d, fs), nn.GELU(), _Linear(4 * d, d))
        self.mlp_refine_corr = Encoder4D((nhead, 4 * nhead, nhead))
        self.mlp_refine_corr2 = Encoder4D((nhead, 4 * nhead, nhead))
        self.feat_to_corr1 = Encoder4D((1, nhead), *f2c)
        self.feat_to_corr2 = Encoder4D((1, nhead), *f2c)
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.v_cross = _Linear(d, d)
        self.norm_cross1, self.norm_cross2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.pos_embed = nn.Parameter(torch.zeros(1, fs * fs, 1, self.dim))
        nn.init.trunc_normal_(self.pos_embed, std=.02)

    def _feed_forward(self, seq, x):
        """Linear -> DWConv 3x3 -> GELU -> Linear (aggregation.py:176-182).  Inference: the GELU rides in the DWConv
        kernel's epilogue (one launch less per block, 20 per get_z)."""
        if torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32:
            return seq(x)
        from ._hip import call
        h = seq[0](x)
        B, L, C = h.shape
        dw = seq[1]
        if C % 4 or not h.is_contiguous():
            return seq[3](seq[2](dw(h)))
        y = torch.empty_like(h)
        call("cpn_dwconv3x3_tokens", h.data_ptr(), dw.dwconv.weight.detach().reshape(C, 9).data_ptr(),
             dw.dwconv.bias.detach().data_ptr(), B, dw.size, dw.size, C, 2, y.data_ptr(),
             _stream_handle())
        return seq[3](y)

    def _qk_weights(self, ncc: int):
        """[q_proj | k_proj] split by input: the cost-volume columns (2d, ncc), the feature columns (2d, d), the biases (2d)
        and the positional table (L, dim).  Under no_grad the concatenations are cached on the parameters' versions."""
        ps = (self.q_proj.weight, self.k_proj.weight, self.q_proj.bias, self.k_proj.bias, self.pos_embed)
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in ps)
        key = tuple((p.data_ptr(), p._version) for p in ps) + (ncc,)
        c = self.__dict__.get("_qk_cache")
        if not grad and c is not None and c[0] == key:
            return c[1]
        Wq, Wk = ps[0], ps[1]
        # (one split node per weight instead of two slices: under autograd a slice's backward is a zero fill + a copy + an add)
        (Wq_c, Wq_f), (Wk_c, Wk_f) = Wq.split((ncc, Wq.shape[1] - ncc), 1), Wk.split((ncc, Wk.shape[1] - ncc), 1)
        out = (torch.cat((Wq_c, Wk_c), 0), torch.cat((Wq_f, Wk_f), 0), torch.cat((ps[2], ps[3]), 0),
               self.pos_embed.reshape(-1, self.dim))
        if not grad:
            out = tuple(t.detach().contiguous() for t in out)
            self.__dict__["_qk_cache"] = (key, out)
        return out

    def _queries_keys(self, corr, feat_n, ops):
        """aggregation.py:274-281: q/k = Linear(cat(interp(corr maps, fs), norm1(feat))) + pos_embed.  The Linear layer
        acts on channels, the bilinear interpolation on positions: the 2048 cost-volume channels are projected at their
        native Hs x Ws positions and the 2 x 256 projected channels are upsampled (exact in real arithmetic; at fs = 64
        the two projections drop from 2 x 4.8 to 0.8 GFLOP per call)."""
        B, H, Hs, Ws, Ht, Wt = corr.shape
        fs, d = self.fs, self.nhead * self.dim
        Wc, Wf, bqk, pos = self._qk_weights(H * Ht * Wt)
        low = torch.matmul(Wc, _corr_to_maps(corr).flatten(2)).view(B, 2 * d, Hs, Ws)      # (B, 2d, Hs, Ws): IS the map layout
        lin = _linear(feat_n, Wf, bqk)                                                    # (B, L, 2d)
        if torch.is_grad_enabled() and (lin.requires_grad or low.requires_grad) or not lin.is_cuda:
            qk = (lin + _map_to_tokens(ops.resize_bilinear(low, fs))).view(B, -1, 2, self.nhead, self.dim) + pos[None, :, None, None, :]
            return qk.unbind(2)
        from ._hip import call
        q = torch.empty(B, fs * fs, self.nhead, self.dim, dtype=torch.float32, device=lin.device)
        k = torch.empty_like(q)
        call("cpn_qk_assemble", lin.data_ptr(), low.data_ptr(), pos.data_ptr(), B, fs, Hs, Ws, self.nhead, self.dim,
             q.data_ptr(), k.data_ptr(), _stream_handle())
        return q, k

    def _attention(self, corr, feat, ops):              # aggregation.py:269-310
        B, H, Hs, Ws, Ht, Wt = corr.shape
        fs = self.fs
        feat_r = feat
        feat = self.norm1(feat)
        q, k = self._queries_keys(corr, feat, ops)
        vf = self.v_proj(feat).view(B, -1, self.nhead, self.dim)
        msg_feat = ops.linear_attention(q, k, vf).view(B, -1, self.nhead * self.dim)
        # cost-volume values: corr + interp(LinearAttention(q, k, interp(v_proj_corr(corr), fs)), Hs), aggregation.py:283-301,
        # evaluated at the volume's own resolution (ops.cost_volume_attention): no (B, 2048, fs, fs) tensor is formed
        msg_corr = ops.cost_volume_attention(q, k, self.v_proj_corr(corr, ops), fs, residual=corr)
        msg_feat = feat_r + msg_feat
        msg_feat = msg_feat + self._feed_forward(self.mlp, self.norm2(msg_feat))
        msg_corr = self.mlp_corr(msg_corr, ops, residual=msg_corr)
        return msg_corr, msg_feat

    def _cross(self, corr, src, trg, ops):              # aggregation.py:312-340
        B, H, Hs, Ws, Ht, Wt = corr.shape
        fs = self.fs
        c = corr.reshape(B, H, Hs * Ws, Ht * Wt)
        pool = lambda t, hh: _map_to_tokens(F.avg_pool2d(_tokens_to_map(t, fs), fs // hh))
        trg_v = self.v_cross(self.norm_cross1(pool(trg, Ht))).view(B, -1, self.nhead, self.dim)
        src_v = self.v_cross(self.norm_cross1(pool(src, Hs))).view(B, -1, self.nhead, self.dim)
        src_attn, trg_attn = ops.cross_attention(c, src_v, trg_v)
        src_attn = src_attn.reshape(B, -1, self.nhead * self.dim)
        trg_attn = trg_attn.reshape(B, -1, self.nhead * self.dim)
        up = lambda t, hh: _map_to_tokens(_tokens_to_map(t, hh).repeat_interleave(fs // hh, 2)
                                          .repeat_interleave(fs // hh, 3))
        src = src + up(src_attn, Hs)
        trg = trg + up(trg_attn, Ht)
        src = src + self._feed_forward(self.mlp_cross, self.norm_cross2(src))
        trg = trg + self._feed_forward(self.mlp_cross, self.norm_cross2(trg))
        return src, trg

    def _cross_views(self, corr, x2, ops):              # aggregation.py:312-340 with [src; trg] stacked along dim 0
        B, H, Hs, Ws, Ht, Wt = corr.shape
        fs, d = self.fs, self.nhead * self.dim
        c = corr.reshape(B, H, Hs * Ws, Ht * Wt)
        pooled = _map_to_tokens(F.avg_pool2d(_tokens_to_map(x2, fs), fs // Hs))
        v = self.v_cross(self.norm_cross1(pooled)).view(2 * B, -1, self.nhead, self.dim)
        v_src, v_trg = v.chunk(2, 0)
        src_attn, trg_attn = ops.cross_attention(c, v_src, v_trg)
        attn = torch.cat((src_attn.reshape(B, -1, d), trg_attn.reshape(B, -1, d)), 0)
        r = fs // Hs
        x2 = x2 + _map_to_tokens(_tokens_to_map(attn, Hs).repeat_interleave(r, 2).repeat_interleave(r, 3))
        return x2 + self._feed_forward(self.mlp_cross, self.norm_cross2(x2))

    def _forward_views_batched(self, corr, src, trg, ops):
        """forward() with the source pass and the target pass — same weights, independent samples — as ONE pass over
        [corr ; corr^T] and [src ; trg] stacked along the batch axis: half the launches of the token side, and the 16^4
        volumes' kernels (a few hundred workgroups per pair) fill twice as much of the chip."""
        t4 = lambda x: x.permute(0, 1, 4, 5, 2, 3)
        from .ufc_ops import swap_pairs as _swap
        B = corr.shape[0]
        corr2 = torch.cat((corr, _swap(corr)), 0)
        msg2, x2 = self._attention(corr2, torch.cat((src, trg), 0), ops)
        # halves taken ONCE per tensor with chunk (a view of the same storage: the correlation kernel still sees its two
        # operands as adjacent halves of one buffer); every `x[:B]` is a slice node of its own under autograd, whose
        # backward is a zero fill + a copy + an add into the other half's - 14 of them per layer before
        msg_s, msg_t = msg2.chunk(2, 0)
        xs, xt = x2.chunk(2, 0)
        corr_r = msg_s + t4(msg_t)
        corr_r = self.feat_to_corr1(ops.correlation_tokens(xs, xt, self.fs), ops, residual=corr_r)
        corr_r = self.mlp_refine_corr(corr_r, ops, residual=corr_r)
        x2 = self._cross_views(corr_r, x2, ops)
        xs, xt = x2.chunk(2, 0)
        corr_r = self.feat_to_corr2(ops.correlation_tokens(xs, xt, self.fs), ops, residual=corr_r)
        corr_r = self.mlp_refine_corr2(corr_r, ops, residual=corr_r)
        return corr_r, xs, xt

    def forward(self, corr, src, trg, ops):             # aggregation.py:342-356
        if BATCH_VIEWS and corr.shape[2:4] == corr.shape[4:6] and src.shape == trg.shape:
            return self._forward_views_batched(corr, src, trg, ops)
        t4 = lambda x: x.permute(0, 1, 4, 5, 2, 3)
        from .ufc_ops import swap_pairs as _swap              # t4(x).contiguous() as one transpose kernel
        if corr.is_cuda and TWO_STREAMS and torch.cuda.is_current_stream_capturing():
            # Inside a HIP-graph capture (coponerf_amd/graphs.py) the source and target attention passes — independent,
            # and made of kernels that each fill a fraction of the chip (16^4 volumes, a few hundred workgroups) — are
            # forked onto a second stream: the replay runs them side by side (14.1 vs 15.1 ms per pair).  Not in eager
            # mode: there the host launch rate is the limit anyway, and blocks that change streams make the caching
            # allocator fall back to hipMalloc in the next call (a serial get_z -> render loop got 35 % slower).
            cur = torch.cuda.current_stream()
            side = _side_stream(corr.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                corr_trg, trg_r = self._attention(_swap(corr), trg, ops)
            corr_src, src_r = self._attention(corr, src, ops)
            cur.wait_stream(side)
            corr_trg.record_stream(cur)
            trg_r.record_stream(cur)
        else:
            corr_src, src_r = self._attention(corr, src, ops)
            corr_trg, trg_r = self._attention(_swap(corr), trg, ops)
        corr_r = corr_src + t4(corr_trg)
        corr_r = self.feat_to_corr1(ops.correlation_tokens(src_r, trg_r, self.fs), ops, residual=corr_r)
        corr_r = self.mlp_refine_corr(corr_r, ops, residual=corr_r)
        src_r, trg_r = self._cross(corr_r, src_r, trg_r, ops)
        corr_r = self.feat_to_corr2(ops.correlation_tokens(src_r, trg_r, self.fs), ops, residual=corr_r)
        corr_r = self.mlp_refine_corr2(corr_r, ops, residual=corr_r)
        return corr_r, src_r, trg_r


def _interp_tokens(x, size, ops):                        # aggregation.py:58-63
    h = int(math.isqrt(x.shape[1]))
    return _map_to_tokens(ops.resize_bilinear(_tokens_to_map(x, h), size))


def _interp4d(x, n, ops):                                # aggregation.py:49-56, x (B,1,h,h,h,h) -> (B,1,n,n,n,n)
    B, C, Hs, Ws, Ht, Wt = x.shape
    if Hs == n and Ht == n:
        return x
    y = ops.resize_bilinear(x.reshape(B, C * Hs * Ws, Ht, Wt), n)
    y = y.reshape(B, C, Hs, Ws, n, n).permute(0, 1, 4, 5, 2, 3).reshape(B, C * n * n, Hs, Ws)
    y = ops.resize_bilinear(y, n)
    return y.reshape(B, C, n, n, n, n).permute(0, 1, 4, 5, 2, 3)


_GRID_CONSTS = {}


def _mapping_to_flow(m):                                 # aggregation.py:30-48
    """flow = (mapping + 1) * (size - 1) / 2 - pixel grid.  The pixel grid and the two scale factors are constants of
    (H, W, device): cached, so the call is 2 launches instead of 11 (two aranges, six pointwise ops, a cat ...)."""
    B, _, H, W = m.shape
    key = (H, W, str(m.device))
    c = _GRID_CONSTS.get(key)
    if c is None:
        xs = torch.arange(W, device=m.device, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W)
        ys = torch.arange(H, device=m.device, dtype=torch.float32).view(1, 1, H, 1).expand(1, 1, H, W)
        c = _GRID_CONSTS[key] = (torch.cat((xs, ys), 1).contiguous(),
                                 torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0], device=m.device).view(1, 2, 1, 1))
    grid, half = c
    return (m[:, :2].float() + 1) * half - grid          # same operation order per element as the reference


class UFC(nn.Module):
    """aggregation.UFC (aggregation.py:358-562): coarse-to-fine schedule [2, 2, 1] layers at 16^2 / 32^2 / 64^2 tokens."""

    def __init__(self, nhead: int = 8):
        super().__init__()
        cfg = [(16, (3, 1, 1), 2), (32, (3, 2, 1), 2), (64, (5, 4, 2), 1)]
        self.layers = nn.ModuleList([nn.ModuleList([UFCLayer(fs, f2c, nhead) for _ in range(n)]) for fs, f2c, n in cfg])
        self.embedding = nn.ModuleList([Encoder4D((1, nhead), *f2c) for _, f2c, _ in cfg])
        self.proj_feat = nn.ModuleList([nn.Sequential(_Linear(c, 256), nn.ReLU()) for c in (512, 256, 128)])

    def forward(self, feat: Sequence[torch.Tensor], nview: int, ops):
        B2 = feat[0].shape[0]
        B = B2 // nview
        # proj_feat of both views in one call per level: (B*nview, L, 256) -> view v of every pair
        proj = [self.proj_feat[i](_map_to_tokens(feat[i])) for i in range(3)]
        proj = [p.view(B, nview, *p.shape[1:]) for p in proj]
        src_f = [p[:, 0] for p in proj]
        trg_f = [p[:, 1] for p in proj]
        feats, corrs = [], []
        corr = src = trg = None
        for lvl, fs in enumerate((16, 32, 64)):
            emb = self.embedding[lvl](ops.correlation_tokens(src_f[lvl], trg_f[lvl], fs), ops, residual=corr)
            if lvl == 0:
                corr, src, trg = emb, src_f[0], trg_f[0]
            else:
                corr = emb
                src = _interp_tokens(src, fs, ops) + src_f[lvl]
                trg = _interp_tokens(trg, fs, ops) + trg_f[lvl]
            for layer in self.layers[lvl]:
                corr, src, trg = layer(corr, src, trg, ops)
            feats.append(_tokens_to_map(torch.stack((src, trg), dim=1).flatten(0, 1), fs))
            corrs.append(ops.correlation_tokens(src, trg, fs))
        fused_ok = CORR_MEAN3_TRAIN or not (torch.is_grad_enabled() and corrs[2].requires_grad)
        if len(corrs) == 3 and hasattr(ops, "corr_mean3") and corrs[2].shape[-1] == 64 and fused_ok:
            c = ops.corr_mean3(corrs)                               # both interpolate4d's, the adds and the / 3 in one pass
        else:
            up = [_interp4d(x, 64, ops) for x in corrs]
            c = ((up[0] + up[1]) + up[2]) / len(corrs)              # sum(...) / 3 without the 0 + x pass; (B,1,64,64,64,64)
        t_to_s, s_to_t = ops.soft_argmax_pair(c)                                      # (B,2,64,64) each
        return feats, (_mapping_to_flow(t_to_s), _mapping_to_flow(s_to_t), t_to_s, s_to_t), c


# ----------------------------------------------------------------------------------------------
# pose head (out of the render/aggregation scope; stock ops) — backbone.py:209-428
# ----------------------------------------------------------------------------------------------
def positional_encodings(fx, fy, cx, cy, n: int = 64):
    """(x^2, y^2, xy, x, y, 1) of K^-1-normalised pixel coordinates, index = col*n + row.
    Closed form of the 4096-iteration Python loop of backbone.get_positional_encodings (backbone.py:209-278)."""
    B = fx.shape[0]
    dev = fx.device
    hp, wp = cy * 2, cx * 2
    # K = [[a,0,c],[0,b,d],[0,0,1]] in normalised coordinates; K^-1 applied to the grid point (x, y, 1) is
    # ((x - c) / a, (y - d) / b, 1) in closed form (the library inverse synchronises with the host, which also rules out
    # HIP-graph capture of get_z; a (B,3,3) @ (3, n*n) product for it is a dozen tiny launches)
    a = (fx / wp) * 2                                   # (B,1)
    b = (fy / hp) * 2
    c = (cx / wp) * 2 - 1
    d = (cy / hp) * 2 - 1
    key = ("pe", n, str(dev))
    g = _GRID_CONSTS.get(key)
    if g is None:
        lin = torch.linspace(-1, 1, steps=n, device=dev)
        g = _GRID_CONSTS[key] = (lin.repeat_interleave(n)[None].contiguous(), lin.repeat(n)[None].contiguous(),
                                 torch.ones(1, n * n, device=dev))
    xs, ys, ones = g                                    # index k*n + j -> xs[k], ys[j]
    p4 = (xs - c) / a                                   # (B, n*n)
    p3 = (ys - d) / b
    return torch.stack((p3 * p3, p4 * p4, p3 * p4, p3, p4, ones.expand(B, -1)), dim=2)  # (B, n*n, 6)


class _Mlp(nn.Module):
    def __init__(self, d: int, hidden: int):
        super().__init__()
        self.fc1, self.act, self.fc2 = _Linear(d, hidden), nn.GELU(), _Linear(hidden, d)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _CrossAttention(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.qkv = _Linear(dim, dim * 3, bias=False)          # unused upstream too (backbone.py:296); checkpoint key
        self.proj_fundamental = _Linear(dim + 6, dim)

    def forward(self, x1, x2, corr, intr, ops):
        B = x1.shape[0]
        a1 = corr.reshape(B, corr.shape[-4] * corr.shape[-3], -1)                       # (B, src, trg)
        f1 = ops.dual_softmax(a1)                                  # a1.softmax(-1) * a1.softmax(-2)
        f2 = f1.transpose(-2, -1)          # == a2.softmax(-1) * a2.softmax(-2) with a2 = a1^T: two softmaxes, not four
        n = int(math.isqrt(x1.shape[1]))
        if isinstance(intr[0], str):                              # ("raw", intrinsics of the input dict, H): one kernel
            pos = ops.pose_positional(intr[1], intr[2], n).to(x1.dtype)
        else:
            pos = positional_encodings(*intr, n=n).to(x1.dtype)
        v1, v2 = torch.cat([x1, pos], dim=2), torch.cat([x2, pos], dim=2)
        F1 = ((v1.transpose(-2, -1) @ f1) @ v1).transpose(-2, -1)
        F2 = ((v2.transpose(-2, -1) @ f2) @ v2).transpose(-2, -1)
        return self.proj_fundamental(F2), self.proj_fundamental(F1)


class CrossBlock(nn.Module):
    def __init__(self, dim: int = 256):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.cross_attn = _CrossAttention(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim, 4 * dim)
        self.norm = nn.LayerNorm(dim)

    def forward(self, x, corr, intr, ops):
        b_s, hw, nf = x.shape
        x = x.reshape(-1, 2, hw, nf)
        fa, fb = self.cross_attn(self.norm1(x[:, 0]), self.norm1(x[:, 1]), corr, intr, ops)
        f = torch.cat([fa.unsqueeze(1), fb.unsqueeze(1)], dim=1).reshape(b_s, -1, nf)
        f = f + self.mlp(self.norm2(f))
        return self.norm(f)


def r6d_to_matrix(d6):
    """Zhou et al. 6-D rotation -> rows of R (CoPoNeRF.py:106-126)."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


_CONSTS = {}


def _const(device, values):
    """Small constant tensors, uploaded once per device (a host->device copy inside get_z would also make the call
    impossible to capture into a HIP graph)."""
    key = (str(device), tuple(values))
    if key not in _CONSTS:
        _CONSTS[key] = torch.tensor(values, dtype=torch.float32, device=device)
    return _CONSTS[key]


def imagenet_normalise(x):
    mean = _const(x.device, (0.485, 0.456, 0.406)).view(1, 3, 1, 1)
    std = _const(x.device, (0.229, 0.224, 0.225)).view(1, 3, 1, 1)
    return (x - mean) / std


def make_pose_heads():
    mlp = lambda dims: [m for i in range(len(dims) - 1) for m in (nn.ReLU(), _Linear(dims[i], dims[i + 1]))]
    pose = nn.Sequential(_Linear((16 * 16 + 6) * 256 * 2, 512), nn.ReLU(), _Linear(512, 256), nn.ReLU(),
                         _Linear(256, 128 * 2), nn.ReLU())
    return pose, nn.Sequential(*mlp([128, 64, 32, 6])), nn.Sequential(*mlp([128, 64, 32, 3]))


_DET_OWNED = [False]


def _conv_determinism(want: bool) -> None:
    """Inference: restrict the convolution library to deterministic algorithms (ResNet trunk: +0.15 ms per pair on MI355X)
    so that get_z as a whole is bit-reproducible — with val=True its pose decides the view-2 sample coordinates.  The
    switch is process-wide and changing it makes the library re-select its kernels (~0.3 s), so it is flipped only when
    the mode changes (inference <-> training), never per call, and only if this module was the one that set it."""
    cd = torch.backends.cudnn
    if want and not cd.deterministic:
        cd.deterministic = True
        _DET_OWNED[0] = True
    elif not want and _DET_OWNED[0] and cd.deterministic:
        cd.deterministic = False
        _DET_OWNED[0] = False


def get_z(model, input, ops):
    """Body of CoPoNeRF.get_z (CoPoNeRF.py:159-206) on the sub-modules of `model`."""
    rgb = input["context"]["rgb"]
    B, V, H, W, _ = rgb.shape
    if (H, W) != (256, 256):
        raise ValueError("get_z supports 256x256 context images only, like the reference (SURVEY.md §0)")
    model.H, model.W = H, W
    x = imagenet_normalise((rgb.flatten(0, 1).permute(0, 3, 1, 2) + 1) / 2.)
    det = not torch.is_grad_enabled() and getattr(model, "deterministic_get_z", True)
    _conv_determinism(det)
    # x is an NHWC-strided view of the input image; the library's deterministic choice for the 7x7 stem in that layout is
    # a 300 ms kernel on MI355X, in NCHW it is the usual one
    z = model.encoder(x.contiguous() if det else x)[:3]
    # conv_map straight from the (N,H,W,3) image (normalisation fused); on the inference path the kernel also emits the
    # NHWC fp16 copy of this level, which the render engine adopts instead of re-laying the map out
    infer = not torch.is_grad_enabled()
    z_conv, z_conv_nhwc16 = ops.conv_map(rgb.flatten(0, 1), model.conv_map.weight, model.conv_map.bias, want_nhwc16=infer)
    if z_conv_nhwc16 is not None and hasattr(model, "_engine"):
        model._engine.adopt_level3(z_conv, z_conv_nhwc16)
    feats, flows, c = model.feature_cost_aggregation(z, model.n_view, ops)
    fused_pose = infer and FUSED_POSE_ENDS and hasattr(ops, "pose_tail") and rgb.is_cuda
    if fused_pose:
        # the launch-bound ends of the pose head as two kernels (csrc/pose.hip): the K^-1 grid, and everything behind the
        # first Linear of the regressor (~70 launches of 2-5 us kernels otherwise)
        intr = ("raw", input["context"]["intrinsics"], H)
    else:
        Kn = input["context"]["intrinsics"].clone()
        Kn[:, :, :2, :] = Kn[:, :, :2, :] / H
        intr = (Kn[:, 0, 0, 0, None], Kn[:, 0, 1, 1, None], Kn[:, 0, 0, 2, None], Kn[:, 0, 1, 2, None])
    pose_feat = model.cross_attention(feats[-1].flatten(-2, -1).transpose(-1, -2), c, intr, ops).reshape(B, -1)
    if fused_pose:
        rel_pose = ops.pose_tail(pose_feat, model.pose_regressor, model.rotation_regressor, model.translation_regressor)
        return feats + [z_conv], rel_pose, flows
    lat = model.pose_regressor(pose_feat)[:, :128]
    R = r6d_to_matrix(model.rotation_regressor(lat))[:, :3, :3]
    t = model.translation_regressor(lat)
    bottom = _const(t.device, (0., 0., 0., 1.)).expand(B, 1, -1)
    rel_pose = torch.cat((torch.cat((R, t.unsqueeze(-1)), dim=-1), bottom), dim=1)
    return feats + [z_conv], rel_pose, flows
