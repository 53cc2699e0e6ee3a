"""Launches of the reference-arithmetic formulation of the per-sample stages (precision "f32", and the rays "auto" flags;
csrc/encode_f32.hip), as functions without state: RenderEngine keeps every cache and setting and hands in
the weight entry, the fp32 node tables, the call's geometry (the dict of RenderEngine._geometry), `buf` and the stream."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import _hip
from ._hip import call

V = 2


def linear_f32(s, x, ldx, wt, bias, y, ldy, m, n, k, relu, res=None) -> None:
    """y = x wt^T (+ bias) (+ res) with the output ReLU if `relu`, on cpn_linear_f32 in blocks of 128 output columns"""
    for n0 in range(0, n, 128):
        nb = min(128, n - n0)
        call("cpn_linear_f32", x.data_ptr(), ldx, wt.data_ptr() + n0 * wt.shape[1] * 4, wt.shape[1],
             0 if bias is None else bias.data_ptr() + n0 * 4, 0 if res is None else res.data_ptr() + n0 * 4,
             0 if res is None else res.shape[1], y.data_ptr() + n0 * 4, ldy, m, nb, k, 0, int(relu), s)


def loc16(loc8, coords9, B, R, S, rays: Optional[torch.Tensor] = None) -> torch.Tensor:
    """local_coords (16 channels, CoPoNeRF.py:411-445) of every sample in row order: [ctx ray dir 3 | 0 0 0 | query dir 3 |
    tanh(depth x {1, .1, .01, .001}) 4 | query origin 3] from the per-sample / per-ray pieces cpn_sample_geometry wrote;
    rays (int64 device indices b * R + r): the rows of the listed rays only, in list order"""
    l8 = loc8.view(B, V, R, S, 8).permute(0, 2, 1, 3, 4)                  # (B,R,V,S,8)
    c9 = coords9.view(B, V, R, 1, 9).permute(0, 2, 1, 3, 4)              # (B,R,V,1,9)
    if rays is not None:
        l8, c9 = l8.reshape(B * R, V, S, 8)[rays], c9.reshape(B * R, V, 1, 9)[rays]
    c9 = c9.expand(*l8.shape[:-1], 9)
    out = torch.cat((l8[..., 0:3], torch.zeros_like(l8[..., 0:3]), c9[..., 0:3], l8[..., 3:7], c9[..., 6:9]), dim=-1)
    return out.reshape(-1, 16).contiguous()


def weights(w: Dict[str, torch.Tensor], params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Adds this formulation's section to the engine's weight entry `w` (RenderEngine._weights) unless it is there: the table
    projection, the K = 68 block (k-major, bias as its last row), the three 128-wide layers in fp32 and the folded key matrix
    as an fp16 (hi, lo) pair.  The rest it reads from the entry as _weights built it."""
    if "k80t" in w:
        return w
    w1 = params["query_encode_latent.weight"].detach().reshape(832, -1).float().contiguous()        # (832, 835)
    w["tab.w"] = w1[:, :768].contiguous()                                                          # (832, 768)
    w["k80t"] = torch.cat((w1[:, 768:835].t(), w["query_encode_latent.b"][None]), 0).contiguous()  # (68, 832)
    for name in ("key_map_2", "query_embed_2", "query_repeat_embed_2"):
        w[name + ".w"] = params[name + ".weight"].detach().reshape(128, -1).float().contiguous()
    hi = w["key_fold.w"].half()
    lo = (w["key_fold.w"] - hi.float()).half()
    w["key_fold.w1"] = torch.cat((hi, hi), 1).contiguous()                                         # against [hid_hi | hid_lo]
    w["key_fold.w2"] = lo.contiguous()                                                             # against hid_hi
    return w


def node_tables(z, w: Dict[str, torch.Tensor], H: int, W: int, s, keep_feat: bool = False) -> Tuple[torch.Tensor, ...]:
    """(tab, map3): the three coarse levels sampled at every node of the common grid in fp32 and projected through the first
    layer's column blocks, and the full-resolution level as NHWC fp32; keep_feat: (tab, map3, feat), feat = the sampled
    (nodes, 768) fp32 rows the projection read (train_precision="f32" keeps them for the weight gradient)"""
    maps = [t.detach().float().permute(0, 2, 3, 1).contiguous() for t in z]                          # NHWC fp32
    nimg = maps[0].shape[0]
    nodes = nimg * int(_hip.lib().cpn_encode_table_nodes(H, W))
    feat = torch.empty(nodes, 768, dtype=torch.float32, device=maps[0].device)
    call("cpn_node_features_f32", maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), H, W, nimg, feat.data_ptr(), s)
    tab = torch.empty(nodes, _hip.TAB_LD, dtype=torch.float32, device=feat.device)
    linear_f32(s, feat, 768, w["tab.w"], None, tab, _hip.TAB_LD, nodes, _hip.TAB_LD, 768, False)
    return (tab, maps[3], feat) if keep_feat else (tab, maps[3])


def per_sample(w, tables, g, zl, at_wt, dims, chunk: int, buf, s, rays: Optional[torch.Tensor] = None, nsel: int = 0) -> None:
    """zl, at_wt of a call in the reference's arithmetic, in the formulation of the fp16 default (csrc/encode_f32.hip): fp32 node tables, the first layer as 4 fp32 table taps + an fp32 K = 68 block, hid as fp16 (hi, lo) pairs, the folded key
    layer on cpn_gemm_f16 against (hi, lo) weights (exact products, fp32 accumulation), both attention rounds on the
    hidden activations, the folded value projection per ray in exact fp32.  dims = (B, R, S, H, W), `chunk` rays per chunk.
    rays (int32 device list, precision="auto"), nsel: only the first nsel listed rays - the per-sample kernels take their
    _rays forms, the per-ray rows are compact in list order and land in zl by one index_copy_; at_wt is written in place."""
    B, R, S, H, W = dims
    tab, map3 = tables
    f32, f16 = torch.float32, torch.float16
    T = V * S
    t = lambda name, shape, dt=f32: buf("f32t." + name, shape, dt, zl.device)
    if rays is None:
        nray, listed, form, out = B * R, (), "", zl
    else:
        idx = rays[:nsel].long()
        nray, listed, form, out = nsel, (rays.data_ptr(),), "_rays", t("zc", (nsel, 416))
    lc_all = loc16(g["loc8"], g["coords9"], B, R, S, None if rays is None else idx)
    C = min(chunk, nray)
    lin = lambda *a, **k: linear_f32(s, *a, **k)
    att = lambda q, wt: call("cpn_attend_hidden_f32" + form, q.data_ptr(), ce.data_ptr(), hs.data_ptr(), B, V, R, S, *listed,
                             ray0, n, hbar.data_ptr(), wt, s)
    for ray0 in range(0, nray, C):
        n = min(C, nray - ray0)
        rows = n * T
        hs = t("hs", (rows, 3328), f16)
        call("cpn_encode_hidden_f32" + form, tab.data_ptr(), map3.data_ptr(), H, W, g["pixel_val"].data_ptr(),
             g["sec_grid"].data_ptr(), g["pe6"].data_ptr(), w["k80t"].data_ptr(), B, V, R, S, *listed, ray0, n, hs.data_ptr(), s)
        kh, key2 = t("kh", (rows, 128)), t("key2", (rows, 128))
        call("cpn_gemm_f16", hs.data_ptr(), 3328, w["key_fold.w1"].data_ptr(), 3328, w["key_fold.b"].data_ptr(), kh.data_ptr(),
             128, rows, 128, 3328, 0, 1, s)
        call("cpn_gemm_f16", hs.data_ptr(), 3328, w["key_fold.w2"].data_ptr(), 1664, w["enc.zero_bias"].data_ptr(),
             kh.data_ptr(), 128, rows, 128, 1664, 1, 2, s)
        lin(kh, 128, w["key_map_2.w"], w["key_map_2.b"], key2, 128, rows, 128, 128, False)
        lc = lc_all[ray0 * T:(ray0 + n) * T]
        hq, ce = t("hq", (rows, 128)), t("ce", (rows, 128))
        lin(lc, 16, w["query_embed.w"], w["query_embed.b"], hq, 128, rows, 128, 16, True)
        lin(hq, 128, w["query_embed_2.w"], w["query_embed_2.b"], ce, 128, rows, 128, 128, False)
        hbar, z1, ze, aq = t("hbar", (n, 1664)), t("z1", (n, 416)), t("ze", (n, 128)), t("aq", (n, 128))
        att(key2, at_wt.data_ptr())
        lin(hbar, 1664, w["value_fold.w"], w["value_fold.b"], z1, 416, n, 416, 1664, False)
        lin(z1, 416, w["encode_latent.w"], w["encode_latent.b"], ze, 128, n, 128, 416, False)
        lin(ze, 128, w["query_repeat_embed.w_z"], None, aq, 128, n, 128, 128, False)
        aq_rows = aq[:n].repeat_interleave(T, dim=0)                                     # the ray's vector on each of its samples
        q2 = key2                                                                        # (the key is spent)
        lin(lc, 16, w["query_repeat_embed.w_l"], w["query_repeat_embed.b"], hq, 128, rows, 128, 16, True, res=aq_rows)
        lin(hq, 128, w["query_repeat_embed_2.w"], w["query_repeat_embed_2.b"], q2, 128, rows, 128, 128, False)
        att(q2, 0)
        zs = t("zs", (n, 416))
        lin(hbar, 1664, w["value_fold.w"], w["value_fold.b"], zs, 416, n, 416, 1664, False)
        # the round-1 vector sits in both view slots when the views are summed (CoPoNeRF.py:481-485): + V * z1
        torch.add(zs[:n], z1[:n], alpha=float(V), out=out[ray0:ray0 + n])
    if rays is not None:
        zl.index_copy_(0, idx, out)

