"""Autograd nodes of RenderEngine.train_precision = "f32": render_train's per-sample stages in the reference's arithmetic.

The forward is the inference f32 mode's (render_f32.py, csrc/encode_f32.hip) over all rays of the call: fp32
node tables, the first layer into `hs` (rows, 3328) fp16 = [hi_own | hi_other | lo_own | lo_other] (hid = hi + lo to 22 bits),
the folded key layer against (hi, lo) weights (exact products, fp32 accumulation), the 128-wide layers and the folded value
projection on the exact fp32 MFMA (cpn_linear_f32), both attention rounds on hi + lo in fp32.  The graph has the shape of the
f16 default's (train_fns.py); the nodes hand each other the same BackwardPass.

`hs` travels through autograd as its hi half, a (rows, 1664) view with row stride 3328: the gradient of hid = hi + lo is the
gradient of either half, and it has the layout of the f16 path's hid2 gradient, so the table-form backward of the first layer
(EncodeFn._backward_tables) takes it unchanged.

Backward precision.  The attention sums, the 128-wide per-sample layers, the value projection and everything per ray are
fp32.  hs's gradient (the key layer's data gradient plus the parked attention parts, masked by hi > 0) is the scaled fp16 of
the f16 path (cpn_gemm_f16_combine_hs), the key layer's weight gradient sums exact hi and lo products of that fp16 gradient,
and the first layer's table-form backward keeps its fp16 operands: ~3e-4 relative rounding, no flipped ReLU masks."""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import render_f32
from ._hip import call
from .train_fns import (BackwardPass, EncodeFn, LinearF32Fn, _colsum_f32, _data_grad, _stream, _wgrad_tall)

HS_LD = 3328                                # hs row: hi (1664) | lo (1664)


def _hs(hi: torch.Tensor) -> torch.Tensor:
    """The whole (rows, 3328) hs behind its hi-half view."""
    assert hi.shape[1] == HS_LD // 2 and hi.stride() == (HS_LD, 1), (hi.shape, hi.stride())
    return hi.as_strided((hi.shape[0], HS_LD), (HS_LD, 1))


class EncodeF32Fn(Function):
    """hi view of hs (rows, 3328) fp16 = the first layer's ReLU output as (hi, lo) pairs, from the fp32 node tables
    (render_f32.node_tables) and cpn_encode_hidden_f32.  Its backward is EncodeFn's table form, fed the combined gradient
    cpn_gemm_f16_combine_hs handed over; the fp16 operands that form needs are rounded from the fp32 ones here."""

    @staticmethod
    def forward(ctx, z0, z1, z2, z3, W, b, pixel_val, sec_grid, pe6, dims, HW, bp: BackwardPass):
        B, V, R, S = dims
        H, Wd = HW
        s = _stream()
        dev = z0.device
        W1 = W.detach().float().contiguous()                                         # (832, 835)
        w = {"tab.w": W1[:, :768].contiguous()}
        tab, map3, feat = render_f32.node_tables((z0, z1, z2, z3), w, H, Wd, s, keep_feat=True)
        k80t = torch.cat((W1[:, 768:835].t(), b.detach().float()[None]), 0).contiguous()  # (68, 832), bias as its last row
        nrays = B * R
        hs = torch.empty(nrays * V * S, HS_LD, dtype=torch.float16, device=dev)
        call("cpn_encode_hidden_f32", tab.data_ptr(), map3.data_ptr(), H, Wd, pixel_val.data_ptr(), sec_grid.data_ptr(),
             pe6.data_ptr(), k80t.data_ptr(), B, V, R, S, 0, nrays, hs.data_ptr(), s)
        del tab
        W16 = torch.zeros(832, 896, dtype=torch.float16, device=dev)      # fp16 image of W, K padded (level-3 columns 768..831)
        call("cpn_pack_weight_f16", W1.data_ptr(), 832, W1.shape[1], W16.data_ptr(), 896, s)
        ctx.save_for_backward(map3.half(), pixel_val, sec_grid, pe6, W16, hs, feat.half(), w["tab.w"].half())
        ctx.dims, ctx.HW, ctx.bp, ctx.K = dims, HW, bp, W1.shape[1]
        ctx.shapes = [tuple(t.shape) for t in (z0, z1, z2, z3)]
        return hs[:, :HS_LD // 2]

    @staticmethod
    def backward(ctx, dC):
        hs = ctx.saved_tensors[5]
        B, V, R, S = ctx.dims
        bp = ctx.bp
        if not bp.parts and bp.take("combined", dC):
            d16 = dC.view(-1, 832)          # the key layer's data-gradient GEMM added the parked parts and applied the mask
        else:
            # the mask in the layout cpn_hid_grad_combine reads (a copy of the hi half: only a gradient the key layer did not
            # hand over takes this branch)
            d = bp.scaled16(dC.contiguous()).to(torch.float16)
            d16 = torch.empty(hs.shape[0] * 2, 832, dtype=torch.float16, device=hs.device)
            call("cpn_hid_grad_combine", d.data_ptr(), hs[:, :HS_LD // 2].contiguous().data_ptr(), *bp.part_ptrs(), B, V, R, S,
                 0, B * R, d16.data_ptr(), _stream())
            bp.parts = []
        return EncodeFn._backward_tables(ctx, d16)[:12]


class KeyLayerF32Fn(Function):
    """kh (rows, 128) fp32 = ReLU([hi | lo] . [W_hi | W_hi]^T + hi . W_lo^T + c) with the (hi, lo) split of the folded fp32 key
    matrix W (128, 1664) formed each call (the two cpn_gemm_f16 launches of render_f32.per_sample).  In the backward it is the
    last consumer of hs autograd runs: it fixes the pass's gradient scale, scales the parts the attention sums parked, and
    hands EncodeF32Fn the combined, masked gradient (cpn_gemm_f16_combine_hs)."""

    @staticmethod
    def forward(ctx, hi, W, b, dims, bp: BackwardPass):
        hs = _hs(hi)
        s = _stream()
        rows = hs.shape[0]
        Wc = W.detach().float().contiguous()
        W_hi = Wc.half()
        W_lo = (Wc - W_hi.float()).half().contiguous()
        W_1 = torch.cat((W_hi, W_hi), 1).contiguous()                     # against [hi | lo]
        bc = b.detach().float().contiguous()
        zero = torch.zeros(W.shape[0], dtype=torch.float32, device=hi.device)
        kh = torch.empty(rows, W.shape[0], dtype=torch.float32, device=hi.device)
        call("cpn_gemm_f16", hs.data_ptr(), HS_LD, W_1.data_ptr(), HS_LD, bc.data_ptr(), kh.data_ptr(), kh.shape[1], rows,
             kh.shape[1], HS_LD, 0, 1, s)
        call("cpn_gemm_f16", hs.data_ptr(), HS_LD, W_lo.data_ptr(), HS_LD // 2, zero.data_ptr(), kh.data_ptr(), kh.shape[1],
             rows, kh.shape[1], HS_LD // 2, 1, 2, s)
        ctx.save_for_backward(hi, W_hi, kh)
        ctx.dims, ctx.bp = dims, bp
        return kh

    @staticmethod
    def backward(ctx, dkh):
        hi, W_hi, kh = ctx.saved_tensors
        hs = _hs(hi)
        bp = ctx.bp
        B, V, R, S = ctx.dims
        d = torch.ops.aten.threshold_backward(dkh.float().contiguous(), kh, 0)     # true gradient where kh > 0
        # the pass's scale, fixed here: the largest entry of hs's gradient (|d| . |W| column sums + the parked parts, w <= 1)
        # and of d itself land below the target
        dmax = d.abs().amax()
        bound = torch.maximum(dmax, dmax * W_hi.float().abs().sum(0).amax() + sum(dh.abs().amax() for _, dh in bp.parts))
        s = bp.ensure(bound.reshape(1))
        bp.parts = [(w, dh * s) for w, dh in bp.parts]                  # parked unscaled by AttendHiddenF32Fn
        d16 = (d * s).to(torch.float16)
        K = d16.shape[1]
        dA = None
        if ctx.needs_input_grad[0] and bp.parts and S % 16 == 0 and K % 32 == 0:
            Wt = W_hi.t().contiguous()                                   # (1664, K)
            dA = bp.hand_over("combined", torch.empty(hs.shape[0], HS_LD // 2, dtype=torch.float16, device=hs.device))
            call("cpn_gemm_f16_combine_hs", d16.data_ptr(), K, Wt.data_ptr(), K, hs.data_ptr(), *bp.part_ptrs(), B, V, R, S, 0,
                 B * R, K, dA.data_ptr(), _stream())
            bp.parts = []
        elif ctx.needs_input_grad[0]:
            dA = _data_grad(d16, W_hi)                                   # EncodeF32Fn adds the parts and masks
        dW = db = None
        if ctx.needs_input_grad[1]:
            # hs^T . d16 on the transposed tall problem (N = 3328): hi and lo products are exact, their halves summed
            dWt = _wgrad_tall(hs, d16, s)                                # (3328, K)
            dW = (dWt[:HS_LD // 2] + dWt[HS_LD // 2:]).t()
        if ctx.needs_input_grad[2]:
            db = _colsum_f32(d)
        return dA, dW, db, None, None


class AttendHiddenF32Fn(Function):
    """(hbar (rays, 1664) fp32, w (N, R, S) fp32) = cpn_attend_hidden_f32(qa, qb, hs): the joint softmax and the weighted sum
    of hi + lo.  Both rounds keep their weights for the backward (cpn_attend_hidden_bwd_f32, fp32 throughout).  hs's gradient
    w (x) dhbar is parked unscaled in the pass for KeyLayerF32Fn; qb_last as in train_fns.AttendHiddenFn."""

    @staticmethod
    def forward(ctx, qa, qb, hi, dims, bp: BackwardPass, qb_last=None):
        B, V, R, S = dims
        hs = _hs(hi)
        nrays = B * R
        hbar = torch.empty(nrays, HS_LD // 2, dtype=torch.float32, device=qa.device)
        w = torch.empty(B * V, R, S, dtype=torch.float32, device=qa.device)
        call("cpn_attend_hidden_f32", qa.data_ptr(), qb.data_ptr(), hs.data_ptr(), B, V, R, S, 0, nrays, hbar.data_ptr(),
             w.data_ptr(), _stream())
        ctx.save_for_backward(qa, qb, hi, w)
        ctx.dims, ctx.bp, ctx.qb_last = dims, bp, qb_last
        return hbar, w

    @staticmethod
    def backward(ctx, dhbar, dw):
        qa, qb, hi, w = ctx.saved_tensors
        hs = _hs(hi)
        B, V, R, S = ctx.dims
        nrays = B * R
        bp = ctx.bp
        dh = dhbar.float().contiguous()
        dwc = None if dw is None else dw.float().contiguous()
        dqa, dqb = torch.empty_like(qa), torch.empty_like(qb)
        dqb = bp.shared_qb_grad(ctx.qb_last, dqb, lambda acc: call(
            "cpn_attend_hidden_bwd_f32", qa.data_ptr(), qb.data_ptr(), hs.data_ptr(), w.data_ptr(), dh.data_ptr(),
            0 if dwc is None else dwc.data_ptr(), B, V, R, S, 0, nrays, dqa.data_ptr(), dqb.data_ptr(), acc, _stream()))
        bp.parts.append((w, dh))            # unscaled: KeyLayerF32Fn fixes the pass's scale
        return dqa, dqb, None, None, None, None


def render_samples(P, mat, bias, z, g, key, value, dims, HW, bp: BackwardPass):
    """(z_local (rays, 416) fp32, round-1 softmax weights (N, R, S)) of render_train in the reference's arithmetic: the graph of
    the f16 default with each per-sample stage in its f32 form.  key / value = the differentiable fp32 folds (W, c)."""
    B, V, R, S = dims
    T = V * S
    Wkf, ckf = key
    Wvf, cvf = value
    hi = EncodeF32Fn.apply(z[0], z[1], z[2], z[3], mat("query_encode_latent", 832), bias("query_encode_latent"),
                           g["pixel_val"], g["sec_grid"], g["pe6"], dims, HW, bp)
    kh = KeyLayerF32Fn.apply(hi, Wkf, ckf, dims, bp)
    key2 = LinearF32Fn.apply(kh, mat("key_map_2", 128), bias("key_map_2"), None, False, False)
    lc = render_f32.loc16(g["loc8"], g["coords9"], B, R, S)                         # (rows, 16) local_coords, row order
    hq = LinearF32Fn.apply(lc, mat("query_embed", 128), bias("query_embed"), None, False, True)
    ce = LinearF32Fn.apply(hq, mat("query_embed_2", 128), bias("query_embed_2"), None, False, False)
    hbar1, w1 = AttendHiddenF32Fn.apply(key2, ce, hi, dims, bp, True)          # coords_embed is shared by the two rounds
    z1 = LinearF32Fn.apply(hbar1, Wvf, cvf, None, False, False)
    ze = LinearF32Fn.apply(z1, mat("encode_latent", 128), bias("encode_latent"), None, False, False)
    Wr_z, Wr_l = mat("query_repeat_embed", 128).split((128, 16), 1)
    aq = LinearF32Fn.apply(ze, Wr_z.contiguous(), None, None, False, False)
    q2h = LinearF32Fn.apply(lc, Wr_l.contiguous(), bias("query_repeat_embed"), aq.repeat_interleave(T, dim=0), False, True)
    q2 = LinearF32Fn.apply(q2h, mat("query_repeat_embed_2", 128), bias("query_repeat_embed_2"), None, False, False)
    hbar2, _ = AttendHiddenF32Fn.apply(q2, ce, hi, dims, bp, False)
    zs = LinearF32Fn.apply(hbar2, Wvf, cvf, None, False, False)
    return zs + float(V) * z1, w1                                            # CoPoNeRF.py:481-485
