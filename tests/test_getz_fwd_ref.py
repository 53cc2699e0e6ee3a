"""The float64 references of tests/getz_fwd_ref.py pinned and calibrated on the CPU, so that tests/test_gpu_getz_f64.py compares
with something that was itself checked.  For every reference:

  pin        against an independent statement in float64 - F.interpolate(align_corners=True) and its autograd, oracle.ufc_ref's
             TorchOps.correlation_tokens and cost_volume_attention, getz.positional_encodings, a stock nn.Linear chain with
             getz.r6d_to_matrix.  A resize reference is pinned in two steps: with the resize matrix F.interpolate itself has
             (its image of the identity) in place of tap_matrix the reference equals the independent statement to float64
             rounding; and tap_matrix differs from that matrix by no more than the fp32 rounding of the fraction, 2 u f per row
             (the quotient's and the product's rounding) - also where the two pick different taps at an integer coordinate,
             because the blend is continuous there.
  emulate    the kernel's fp32 operation order in torch float32 on every case of the GPU tests: max err/bound <= 1, so the
             bounds are not too tight; the figures are printed.
  defect     one plausible defect injected into the emulation leaves the bound: the bounds are not vacuous.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ufc_ref as oracle
from tests import getz_fwd_ref as ref
from tests.attend_ref import ratio
from tests.test_ufc_bwd_ref import seq_sum, strided_sums, tree_halving, wave_sum64

F32 = torch.float32
U = ref.U


def worst(got, want, terms):
    return float(ratio(got, want, ref.total(terms).expand_as(want)).max())


def inside(what, got, want, terms):
    return ref.report(what, got, want, terms)


def outside(what, got, want, terms):
    w = worst(got, want, terms)
    print(f"{what}: the defect reaches err/bound = {w:.1f}")
    assert w > 1, what


# ------------------------------------------------------------------------------------------------------------------
# taps
# ------------------------------------------------------------------------------------------------------------------
def torch_matrix(n_fine, h):
    """The (n_fine, h) matrix of F.interpolate(align_corners=True) along one axis in float64: its image of the identity."""
    eye = torch.eye(h, dtype=torch.float64).view(1, h, h, 1)                            # (1, channel j, axis, 1)
    return F.interpolate(eye, size=(n_fine, 1), mode="bilinear", align_corners=True)[0, :, :, 0].T.contiguous()


def taps32(n_fine, h):
    i0, i1, l, f = ref.axis_taps(n_fine, h)
    return i0, i1, l.float(), f.float()


def _axis_pairs():
    pairs = set()
    for planes, h, w, H, W in ref.RESIZE_CASES:
        pairs |= {(H, h), (W, w)}
    for B, h0, h1, n in ref.MEAN3_CASES:
        pairs |= {(n, h0), (n, h1)}
    for B, fs, h, w, nhead, dim in ref.QK_CASES:
        pairs |= {(fs, h), (fs, w)}
    for B, fs, H, hs, Dv in ref.CVA_CASES:
        pairs |= {(fs, hs), (hs, fs)}
    return sorted(pairs)


@pytest.mark.parametrize("n_fine,h", _axis_pairs() + [(130, 33), (64, 16), (64, 32), (33, 33)])
def test_tap_matrix_is_the_float64_resize_matrix_up_to_the_fraction_rounding(n_fine, h):
    W, T = ref.tap_matrix(n_fine, h), torch_matrix(n_fine, h)
    f = ref.axis_taps(n_fine, h)[3]
    assert torch.equal(W.sum(1), torch.ones(n_fine, dtype=torch.float64)) and bool((W >= 0).all())
    assert bool(((W - T).abs() <= (2 * U * f + 1e-15).unsqueeze(1)).all()), float((W - T).abs().max())
    D = ref.tap_matrix(n_fine, h, derivative=True)
    assert bool((D.sum(1) == 0).all())
    if n_fine == h:
        assert torch.equal(W, torch.eye(h, dtype=torch.float64))


def close64(what, a, b, scale=None):
    tol = 1e-12 * float((a.abs().max() if scale is None else scale) + 1e-300)
    err = float((a - b).abs().max())
    assert err <= tol, (what, err, tol)


# ------------------------------------------------------------------------------------------------------------------
# resize and adjoint
# ------------------------------------------------------------------------------------------------------------------
def mix(a, b, l):
    return a * (1.0 - l) + b * l


def emu_resize(x, H, W, defect=False):
    planes, h, w = x.shape
    y0, y1, ly, _ = taps32(H, h)
    x0, x1, lx, _ = taps32(W, w)
    if defect:                                                    # the second column tap one to the left
        x1 = torch.clamp(x1 - 1, min=0)
    g = lambda yi, xi: x[:, yi][:, :, xi]
    top, bot = mix(g(y0, x0), g(y0, x1), lx), mix(g(y1, x0), g(y1, x1), lx)
    return mix(top, bot, ly[:, None])


def weights32(n_fine, h):
    """(n_fine, h) fp32: (t == i0 ? fl(1 - l) : 0) + (t == i1 ? l : 0), as the adjoint and the Kd gather form them."""
    i0, i1, l, _ = taps32(n_fine, h)
    t = torch.arange(h)
    return torch.where(t[None] == i0[:, None], (1.0 - l)[:, None], torch.zeros((), dtype=F32)) + \
        torch.where(t[None] == i1[:, None], l[:, None], torch.zeros((), dtype=F32))


def emu_adjoint(g, h, w, defect=False):
    planes, H, W = g.shape
    wy, wx = weights32(H, h), weights32(W, w)
    row = torch.zeros(planes, H, w, dtype=F32)
    for X in range(W - (1 if defect else 0)):                     # defect: the window ends one fine column early
        row = row + wx[X][None, None, :] * g[:, :, X, None]
    acc = torch.zeros(planes, h, w, dtype=F32)
    for Y in range(H):
        acc = acc + wy[Y][None, :, None] * row[:, Y, None, :]
    return acc


@pytest.mark.parametrize("case", ref.RESIZE_CASES, ids=ref.case_id)
def test_resize_references(case):
    planes, h, w, H, W = case
    x = ref.make_resize_inputs(case)
    xd = x["x"].double().requires_grad_(True)
    up = F.interpolate(xd[None], size=(H, W), mode="bilinear", align_corners=True)[0]
    (gin,) = torch.autograd.grad(up, xd, x["g"].double())
    mats = (torch_matrix(H, h), torch_matrix(W, w))
    close64("resize", ref.resize_ref(x["x"], H, W, mats)[0], up.detach())
    close64("adjoint", ref.resize_adjoint_ref(x["g"], h, w, mats)[0], gin)
    want, terms = ref.resize_ref(x["x"], H, W)
    inside("resize emulation " + ref.case_id(case), emu_resize(x["x"], H, W), want, terms)
    if case == ref.RESIZE_IDENTITY:
        assert torch.equal(emu_resize(x["x"], H, W), x["x"]) and torch.equal(want, x["x"].double())
    wa, ta = ref.resize_adjoint_ref(x["g"], h, w)
    inside("adjoint emulation " + ref.case_id(case), emu_adjoint(x["g"], h, w), wa, ta)
    if case == (2, 3, 5, 8, 6):
        outside("resize, second tap one to the left", emu_resize(x["x"], H, W, True), want, terms)
        outside("adjoint, last fine column dropped", emu_adjoint(x["g"], h, w, True), wa, ta)


# ------------------------------------------------------------------------------------------------------------------
# final correlation
# ------------------------------------------------------------------------------------------------------------------
def emu_interp4d(x, n):
    h = x.shape[-1]
    i0, i1, l, _ = taps32(n, h)

    def pass2d(t):                                                # the last two dims: blend4(p00, p01, p10, p11, l_last, l_first)
        g = lambda a, b: t[..., a, :][..., b]
        return mix(mix(g(i0, i0), g(i0, i1), l), mix(g(i1, i0), g(i1, i1), l), l[:, None])
    y = pass2d(x).permute(0, 3, 4, 1, 2)                          # (B, i, j, I, J)
    return pass2d(y).permute(0, 3, 4, 1, 2)


def emu_mean3(c0, c1, c2, defect=False):
    n = c2.shape[-1]
    u0, u1 = emu_interp4d(c0, n), emu_interp4d(c1, n)
    third = torch.tensor(1.0, dtype=F32) / torch.tensor(3.0, dtype=F32)
    if defect:                                                    # 1/3 applied before the second addition
        return (u0 + u1) * third + c2
    return ((u0 + u1) + c2) * third


def interp4d_torch(x, n):                                         # aggregation.py:49-56 on (B, h, h, h, h)
    B, h = x.shape[0], x.shape[-1]
    y = F.interpolate(x.reshape(B, h * h, h, h), size=(n, n), mode="bilinear", align_corners=True)
    y = y.reshape(B, h, h, n, n).permute(0, 3, 4, 1, 2).reshape(B, n * n, h, h)
    y = F.interpolate(y, size=(n, n), mode="bilinear", align_corners=True)
    return y.reshape(B, n, n, n, n).permute(0, 3, 4, 1, 2)


@pytest.mark.parametrize("case", ref.MEAN3_CASES, ids=ref.case_id)
def test_corr_mean3_reference(case):
    B, h0, h1, n = case
    assert ref.corr_mean3_arm(B, h0, h1) == ref.MEAN3_ARMS[case]
    x = ref.make_mean3_inputs(case)
    c0, c1, c2 = x["c0"], x["c1"], x["c2"]
    stock = (interp4d_torch(c0.double(), n) + interp4d_torch(c1.double(), n) + c2.double()) * ref.THIRD
    close64("mean3", ref.corr_mean3_ref(c0, c1, c2, (torch_matrix(n, h0), torch_matrix(n, h1)))[0], stock)
    want, terms = ref.corr_mean3_ref(c0, c1, c2)
    inside("mean3 emulation " + ref.case_id(case), emu_mean3(c0, c1, c2), want, terms)
    if case == (2, 3, 5, 7):
        outside("mean3, 1/3 before the second addition", emu_mean3(c0, c1, c2, True), want, terms)
    if h1 == n:
        assert torch.equal(emu_interp4d(c1, n), c1)


def test_corr_mean3_both_arms_shape():
    B, h0, h1, n = ref.MEAN3_BOTH
    assert ref.corr_mean3_arm(B, h0, h1) == "thread" and ref.corr_mean3_arm(B - 1, h0, h1) == "planes"


# ------------------------------------------------------------------------------------------------------------------
# correlation
# ------------------------------------------------------------------------------------------------------------------
def emu_l2norm(x, eps=1e-5):
    ss = wave_sum64(x * x)
    d = torch.sqrt(ss) + torch.tensor(eps, dtype=F32)
    return x / d.unsqueeze(-1)


def emu_gemm(sn, tn, drop_tail=False):
    """The MFMA's k order: block kb, then e = 0..3, each step adding k = kb + 4 fg + e for fg = 0..3."""
    B, L, K = sn.shape
    acc = torch.zeros(B, L, L, dtype=F32)
    blocks = list(range(0, K, 16))
    if drop_tail and len(blocks) % 2 == 1:                        # the odd K / 16 tail step forgotten
        blocks = blocks[:-1]
    for kb in blocks:
        for e in range(4):
            for fg in range(4):
                kk = kb + 4 * fg + e
                acc = acc + sn[:, :, None, kk] * tn[:, None, :, kk]
    return acc


@pytest.mark.parametrize("case", ref.CORR_CASES, ids=ref.case_id)
def test_correlation_references(case):
    """The GEMM's emulation runs on the first 4 samples of a case (they are independent and walk the same code)."""
    B, L, C = case
    assert ref.correlation_arm(B, L) == ref.CORR_ARMS[case]
    x = ref.make_corr_inputs(case)
    r = ref.correlation_ref(x["src"], x["trg"])
    s64, t64 = x["src"].double(), x["trg"].double()
    close64("src_n", r["src_n"], oracle.l2_normalise_tokens(s64))
    close64("corr", r["corr"], torch.einsum("bsc,btc->bst", oracle.l2_normalise_tokens(s64), oracle.l2_normalise_tokens(t64)), 1.0)
    fs = math.isqrt(L)
    if fs * fs == L:
        close64("corr tokens", r["corr"].reshape(B, 1, fs, fs, fs, fs), oracle.TorchOps.correlation_tokens(s64, t64, fs), 1.0)
    sn, tn = emu_l2norm(x["src"]), emu_l2norm(x["trg"])
    what = "correlation emulation " + ref.case_id(case)
    inside(what + " src_n", sn, r["src_n"], r["src_n_terms"])
    inside(what + " trg_n", tn, r["trg_n"], r["trg_n_terms"])
    nb = min(B, 4)
    want, terms = ref.correlation_gemm_ref(sn[:nb], tn[:nb])
    inside(what + " corr", emu_gemm(sn[:nb], tn[:nb]), want, terms)
    if case == ref.CORR_ZERO_ROW:
        assert bool((sn[1, 3] == 0).all()) and bool((want[1, 3] == 0).all()) and bool((want[0, :, 0] == 0).all())
        assert bool((terms["chain"][1, 3] == 0).all())
    if case == (1, 100, 48):
        outside("correlation, odd K/16 tail step dropped", emu_gemm(sn, tn, True), want, terms)


# ------------------------------------------------------------------------------------------------------------------
# q / k assembly
# ------------------------------------------------------------------------------------------------------------------
def emu_qk(lin, low, pos, fs, h, w, nhead, dim, contract=False, defect=False):
    B, L, d2 = lin.shape
    d = nhead * dim
    y0, y1, ly, fy = taps32(fs, h)
    x0, x1, lx, fx = taps32(fs, w)
    if defect:                                                    # the column tap's border test against h instead of w
        x1 = x0 + (x0 < h - 1)
    if contract:                                                  # l = fma(scale, I, -i0): the product enters unrounded
        frac = lambda n_in, i0: ((torch.tensor(n_in - 1, dtype=F32) / torch.tensor(max(fs - 1, 1), dtype=F32)).double()
                                 * torch.arange(fs, dtype=torch.float64) - i0.double()).float()
        ly, lx = frac(h, y0), frac(w, x0)
    g = lambda yi, xi: low[:, :, yi][:, :, :, xi]
    top, bot = mix(g(y0, x0), g(y0, x1), lx), mix(g(y1, x0), g(y1, x1), lx)
    up = mix(top, bot, ly[:, None]).permute(0, 2, 3, 1).reshape(B, L, d2)
    v = (lin + up) + pos[:, torch.arange(d2) % dim].unsqueeze(0)
    return v[..., :d].contiguous(), v[..., d:].contiguous()


@pytest.mark.parametrize("case", ref.QK_CASES, ids=ref.case_id)
def test_qk_assemble_reference(case):
    B, fs, h, w, nhead, dim = case
    x = ref.make_qk_inputs(case)
    d = nhead * dim
    up = F.interpolate(x["low"].double(), size=(fs, fs), mode="bilinear", align_corners=True)
    stock = x["lin"].double() + up.permute(0, 2, 3, 1).reshape(B, fs * fs, 2 * d) + x["pos"].double().repeat(1, 2 * nhead)
    q64, k64, _, _ = ref.qk_assemble_ref(x["lin"], x["low"], x["pos"], fs, h, w, nhead, dim, (torch_matrix(fs, h), torch_matrix(fs, w)))
    close64("q", q64, stock[..., :d])
    close64("k", k64, stock[..., d:])
    qw, kw, qt, kt = ref.qk_assemble_ref(x["lin"], x["low"], x["pos"], fs, h, w, nhead, dim)
    for contract in (False, True):
        q, k = emu_qk(x["lin"], x["low"], x["pos"], fs, h, w, nhead, dim, contract)
        what = f"qk emulation {ref.case_id(case)} contract={contract}"
        inside(what + " q", q, qw, qt)
        inside(what + " k", k, kw, kt)
    if case == (2, 5, 3, 4, 2, 3):
        q, k = emu_qk(x["lin"], x["low"], x["pos"], fs, h, w, nhead, dim, defect=True)
        outside("qk, column border tested against h", q, qw, qt)
        outside("qk (k half), column border tested against h", k, kw, kt)


# ------------------------------------------------------------------------------------------------------------------
# cost-volume attention
# ------------------------------------------------------------------------------------------------------------------
def elu1(x):
    return torch.where(x > 0, x + 1.0, torch.exp(torch.clamp(x, max=0.0)))


def emu_cva(q, k, v, res, fs, old_window=False):
    """cva_kd_kernel and cva_out_kernel in fp32.  old_window: the gather window before this fix - for hs == 1 it was formed with
    one token per low-resolution step and ended at token 2."""
    B, L, H, D = q.shape
    P, Dv = v.shape[2], v.shape[3]
    hs = math.isqrt(P)
    eps = torch.tensor(1e-6, dtype=F32)
    K = elu1(k)
    nblk = ref.cdiv(P, 16)
    Lb = ref.cdiv(L, nblk)
    ksum = torch.zeros(B, H, D, dtype=F32)
    for blk in range(nblk):
        tok = K[:, blk * Lb:min(L, blk * Lb + Lb)]                # (B, n, H, 32)
        if tok.shape[1] == 0:
            continue
        ksum = ksum + seq_sum(strided_sums(tok.permute(0, 2, 3, 1), 8), -1)
    wg = weights32(fs, hs)                                        # (fs, hs)
    last = min(fs - 1, 2) if (old_window and hs == 1) else fs - 1
    Kmap = K.view(B, fs, fs, H, D)
    row = torch.zeros(B, fs, hs, H, D, dtype=F32)
    for X in range(last + 1):
        row = row + wg[X].view(1, 1, hs, 1, 1) * Kmap[:, :, X, None]
    kd = torch.zeros(B, hs, hs, H, D, dtype=F32)
    for Y in range(last + 1):
        kd = kd + wg[Y].view(1, hs, 1, 1, 1) * row[:, Y, None]
    kd = kd.reshape(B, P, H, D).permute(0, 2, 1, 3)               # (B, H, P, 32)
    M = torch.zeros(B, H, D, Dv, dtype=F32)
    for blk in range(nblk):
        m = torch.zeros(B, H, D, Dv, dtype=F32)
        for p in range(blk * 16, min(P, blk * 16 + 16)):
            m = m + kd[:, :, p, :, None] * v[:, :, p, None, :]
        M = M + m
    y0, y1, ly, _ = taps32(hs, fs)
    p = torch.arange(P)
    py, px = p // hs, p % hs
    idx = (y0[py] * fs + y0[px], y0[py] * fs + y1[px], y1[py] * fs + y0[px], y1[py] * fs + y1[px])
    wts = ((1.0 - ly[px]) * (1.0 - ly[py]), ly[px] * (1.0 - ly[py]), (1.0 - ly[px]) * ly[py], ly[px] * ly[py])
    qd = torch.zeros(B, P, H, D, dtype=F32)
    for t in range(4):
        qv = elu1(q[:, idx[t]])                                   # (B, P, H, 32)
        dot = tree_halving(qv * ksum[:, None])
        qd = qd + wts[t].view(1, P, 1, 1) * qv / (dot.unsqueeze(-1) + eps)
    qd = qd.permute(0, 2, 1, 3)                                   # (B, H, P, 32)
    a = torch.zeros(B, H, P, Dv, dtype=F32)
    for dd in range(D):
        a = a + qd[..., dd, None] * M[:, :, None, dd, :]
    return a if res is None else res + a


def as_volume(t, hs, Dv):
    """(B, H, P, Dv) -> (B, H, hs, hs, Dv, 1): the oracle's (B, H, Hs, Ws, Ht, Wt) with Ht Wt = Dv."""
    return t.reshape(t.shape[0], t.shape[1], hs, hs, Dv, 1)


@pytest.mark.parametrize("with_res", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("case", ref.CVA_CASES, ids=ref.case_id)
def test_cva_reference(case, with_res):
    B, fs, H, hs, Dv = case
    x = ref.make_cva_inputs(case)
    res = x["res"] if with_res else None
    stock = oracle.TorchOps.cost_volume_attention(x["q"].double(), x["k"].double(), as_volume(x["v"].double(), hs, Dv), fs,
                                                  residual=None if res is None else as_volume(res.double(), hs, Dv), eps=ref.EPS_LA)
    pinned = ref.cva_ref(x["q"], x["k"], x["v"], res, fs, mats=(torch_matrix(fs, hs), torch_matrix(hs, fs)))[0]
    close64("cva", pinned, stock.reshape(B, H, hs * hs, Dv))
    want, terms = ref.cva_ref(x["q"], x["k"], x["v"], res, fs)
    what = f"cva emulation {ref.case_id(case)} {'residual' if with_res else 'plain'}"
    inside(what, emu_cva(x["q"], x["k"], x["v"], res, fs), want, terms)
    if case in ref.CVA_ONE_POINT:
        outside(what + ", tokens past the third dropped (the kernel before the fix)", emu_cva(x["q"], x["k"], x["v"], res, fs, True),
                want, terms)
    else:
        assert torch.equal(emu_cva(x["q"], x["k"], x["v"], res, fs, True), emu_cva(x["q"], x["k"], x["v"], res, fs))


def test_cva_gather_window_is_complete_except_for_one_low_point():
    """cva_kd_kernel's window [Y0, Y1] restated in fp32: for every 1 <= hs <= 33, hs <= fs < 130 it holds every token whose
    tap touches the position - except, before the fix, for hs == 1 and fs >= 4, where it ended at token 2."""
    import numpy as np
    f32 = np.float32
    for hs in range(1, 34):
        for fs in range(hs, 130):
            inv_s = f32(fs - 1) / f32(hs - 1) if fs > 1 and hs > 1 else f32(1.0)
            i0, i1, l, _ = (t.numpy() for t in ref.axis_taps(fs, hs))
            for y in range(hs):
                touch = ((i0 == y) & (l < 1)) | ((i1 == y) & (l > 0))
                lo, hi = int(touch.nonzero()[0].min()), int(touch.nonzero()[0].max())
                Y0 = max(0, int(np.floor(f32(y - 1) * inv_s)) - 1)
                Y1 = min(fs - 1, int(np.ceil(f32(y + 1) * inv_s)) + 1)
                if hs == 1:
                    assert (Y0 <= lo and hi <= Y1) == (fs < 4), (hs, fs)
                    Y0, Y1 = 0, fs - 1                              # the fix
                assert Y0 <= lo and hi <= Y1, (hs, fs, y)


class _Fp32Ops:
    """The two resize operators cost_volume_attention_torch asks of its `ops`, on the fp32 emulations."""

    @staticmethod
    def resize_bilinear(x, size):
        N, C, h, w = x.shape
        return emu_resize(x.reshape(N * C, h, w), size, size).reshape(N, C, size, size)

    @staticmethod
    def resize_bilinear_adjoint(x, size):
        N, C, H, W = x.shape
        return emu_adjoint(x.reshape(N * C, H, W), size, size).reshape(N, C, size, size)


@pytest.mark.parametrize("case", ref.CVA_ONE_POINT + [(1, 7, 2, 3, 300)], ids=ref.case_id)
def test_cva_stock_form_in_fp32(case):
    """cost_volume_attention_torch itself on fp32 CPU tensors inside the stock form's bound (its elu term included)."""
    from coponerf_amd.ufc_ops import cost_volume_attention_torch
    B, fs, H, hs, Dv = case
    x = ref.make_cva_inputs(case)
    vol = lambda t: t.reshape(B, H, hs, hs, Dv, 1)
    got = cost_volume_attention_torch(_Fp32Ops, x["q"], x["k"], vol(x["v"]), fs, vol(x["res"]), 1e-6)
    inside("cva stock form " + ref.case_id(case), got.reshape(B, H, hs * hs, Dv), *ref.cva_ref(x["q"], x["k"], x["v"], x["res"], fs, stock=True))


def test_cva_stock_form_one_low_point():
    """cost_volume_attention_torch's association, Qd (Kd^T v) with Kd through the resize ADJOINT, in float64 on the hs == 1
    cases: equal to cva_ref (the reference's order) to float64 rounding - the training form never had the window."""
    for case in ref.CVA_ONE_POINT:
        B, fs, H, hs, Dv = case
        x = ref.make_cva_inputs(case)
        want, _ = ref.cva_ref(x["q"], x["k"], x["v"], x["res"], fs)
        Q, K = ref._phi(x["q"].double()), ref._phi(x["k"].double())
        Z = 1 / (torch.einsum("blhd,bhd->blh", Q, K.sum(1)) + ref.EPS_LA)
        as_map = lambda t: t.permute(0, 2, 3, 1).reshape(B * H * 32, fs, fs)
        Qd = ref.resize_ref(as_map(Q * Z[..., None]), hs, hs)[0].reshape(B, H, 32, hs * hs)
        Kd = ref.resize_adjoint_ref(as_map(K), hs, hs)[0].reshape(B, H, 32, hs * hs)
        got = x["res"].double() + Qd.transpose(-1, -2) @ (Kd @ x["v"].double())
        close64("stock association", got, want)


# ------------------------------------------------------------------------------------------------------------------
# pose head
# ------------------------------------------------------------------------------------------------------------------
def emu_pospos(K, H, lin, defect=False):
    B, n = K.shape[0], lin.shape[0]
    H = torch.tensor(H, dtype=F32)
    Kb = K[:, 0]
    fx, fy, cx, cy = (Kb[:, 0, 0] / H).view(B, 1), (Kb[:, 1, 1] / H).view(B, 1), (Kb[:, 0, 2] / H).view(B, 1), (Kb[:, 1, 2] / H).view(B, 1)
    hp, wp = cy * 2.0, cx * 2.0
    a, bb = (fx / wp) * 2.0, (fy / hp) * 2.0
    c, d = (cx / wp) * 2.0 - 1.0, (cy / hp) * 2.0 - 1.0
    xs, ys = lin.repeat_interleave(n).view(1, -1), lin.repeat(n).view(1, -1)
    if defect:                                                    # the grid transposed: index = row n + col
        xs, ys = ys, xs
    p4, p3 = (xs - c) / a, (ys - d) / bb
    return torch.stack((p3 * p3, p4 * p4, p3 * p4, p3, p4, torch.ones_like(p3)), 2)


@pytest.mark.parametrize("case", ref.POSPOS_CASES, ids=ref.case_id)
def test_pose_positional_reference(case):
    from coponerf_amd import getz
    B, V, n = case
    x = ref.make_pospos_inputs(case)
    K, H = x["K"], x["H"]
    assert bool((K[:, 0, 0, 0] != K[:, 0, 1, 1]).all()) and bool((K[:, 0, 0, 2] != K[:, 0, 1, 2]).all())
    want, terms = ref.pose_positional_ref(K, H, x["lin"])
    Kn = K.double() / H
    getz._GRID_CONSTS.pop(("pe", n, "cpu"), None)                 # the cached fp32 grid of another test must not be used in float64
    stock = getz.positional_encodings(Kn[:, 0, 0, 0, None], Kn[:, 0, 1, 1, None], Kn[:, 0, 0, 2, None], Kn[:, 0, 1, 2, None], n=n)
    getz._GRID_CONSTS.pop(("pe", n, "cpu"), None)
    close64("positional", want, stock.double())                   # both read the same fp32 linspace
    if V > 1:
        other = K.clone()
        other[:, 1] = other[:, 1] * 1.5
        assert torch.equal(ref.pose_positional_ref(other, H, x["lin"])[0], want)
    inside("positional emulation " + ref.case_id(case), emu_pospos(K, H, x["lin"]), want, terms)
    if n > 1:
        outside("positional, grid transposed", emu_pospos(K, H, x["lin"], True), want, terms)


def emu_gemv(x, W, nsplit, defect=False):
    B, K = x.shape
    O = W.shape[0]
    out = torch.zeros(B, O, nsplit, dtype=F32)
    for c, (lo, hi) in enumerate(ref.gemv_chunks(K, nsplit)):
        if defect and hi == K:                                    # the ragged last chunk loses its last 16-byte group
            hi -= 4
        if hi <= lo:
            continue
        xv, wv = x[:, None, lo:hi].reshape(B, 1, -1, 4), W[None, :, lo:hi].reshape(1, O, -1, 4)
        g = (wv[..., 0] * xv[..., 0] + wv[..., 1] * xv[..., 1]) + (wv[..., 2] * xv[..., 2] + wv[..., 3] * xv[..., 3])
        r = tree_halving(strided_sums(g, 256).reshape(B, O, 4, 64))
        out[:, :, c] = (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])
    return out


@pytest.mark.parametrize("case", ref.GEMV_CASES, ids=ref.case_id)
def test_pose_gemv_reference(case):
    B, K, O, nsplit = case
    x = ref.make_gemv_inputs(case)
    want, terms = ref.pose_gemv_ref(x["x"], x["W"], nsplit)
    full = x["x"].double() @ x["W"].double().T
    close64("gemv", want.sum(-1), full, float(full.abs().max()) + math.sqrt(K))
    chunks = ref.gemv_chunks(K, nsplit)
    assert chunks[0][0] == 0 and max(hi for _, hi in chunks) == K and all(a[1] == b[0] or b[0] == b[1] for a, b in zip(chunks, chunks[1:]))
    for c, (lo, hi) in enumerate(chunks):
        if hi == lo:
            assert bool((want[:, :, c] == 0).all()) and bool((terms["chain"][:, :, c] == 0).all())
    if case == (3, 160, 7, 64):
        assert [hi - lo for lo, hi in chunks] == [4] * 40 + [0] * 24
    if case == (2, 1028, 5, 8):
        assert chunks[-1] == (924, 1028) and chunks[0] == (0, 132)
    inside("gemv emulation " + ref.case_id(case), emu_gemv(x["x"], x["W"], nsplit), want, terms)
    if K > 4:
        outside("gemv, last group of the last chunk dropped", emu_gemv(x["x"], x["W"], nsplit, True), want, terms)


def emu_dense(x, W, b, relu=True):
    xv = torch.relu(x) if relu else x
    return tree_halving(strided_sums(xv[:, None, :] * W[None], 64)) + b


def emu_tail(h, nsplit, bias0, weights, defect=None):
    w2, b2, w3, b3, r1, rb1, r2, rb2, r3, rb3, t1, tb1, t2, tb2, t3, tb3 = weights
    if nsplit > 0:
        v = h[..., 0]
        for c in range(1, nsplit - (1 if defect == "last chunk" else 0)):
            v = v + h[..., c]
        s0 = v if defect == "bias" else v + bias0
    else:
        s0 = h
    s1 = emu_dense(s0, w2, b2)
    s2 = emu_dense(s1, w3, b3, relu=defect != "relu")
    lat = s2[:, :128]
    o6 = emu_dense(emu_dense(emu_dense(lat, r1, rb1), r2, rb2), r3, rb3)
    o3 = emu_dense(emu_dense(emu_dense(lat, t1, tb1), t2, tb2), t3, tb3)
    tiny = torch.tensor(1e-12, dtype=F32)
    a1, a2 = o6[:, :3], o6[:, 3:]
    n1 = torch.maximum(torch.sqrt(a1[:, 0] * a1[:, 0] + a1[:, 1] * a1[:, 1] + a1[:, 2] * a1[:, 2]), tiny).unsqueeze(1)
    b1 = a1 / n1
    dt = (b1[:, 0] * a2[:, 0] + b1[:, 1] * a2[:, 1] + b1[:, 2] * a2[:, 2]).unsqueeze(1)
    u = a2 - dt * b1
    n2 = torch.maximum(torch.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]), tiny).unsqueeze(1)
    bb2 = u / n2
    out = torch.zeros(h.shape[0], 4, 4, dtype=F32)
    out[:, 0, :3], out[:, 1, :3], out[:, 2, :3], out[:, :3, 3], out[:, 3, 3] = b1, bb2, ref._cross(b1, bb2), o3, 1.0
    return out


@functools.lru_cache(maxsize=None)
def _tail_inputs(case):
    return ref.make_tail_inputs(case)


@pytest.mark.parametrize("case", ref.TAIL_CASES, ids=ref.case_id)
def test_pose_tail_reference(case):
    from coponerf_amd import getz
    B, nsplit, kind = case
    x = _tail_inputs(case)
    w = x["weights"]
    want, terms = ref.pose_tail_ref(x["h"], nsplit, x["bias0"], w)
    # the stock chain in float64
    d = [t.double() for t in w]
    s0 = x["h"].double().sum(-1) + x["bias0"].double() if nsplit else x["h"].double()
    lin = lambda t, i: F.linear(t, d[i], d[i + 1])
    lat = torch.relu(lin(torch.relu(lin(torch.relu(s0), 0)), 2))[:, :128]               # pose_regressor: Linear ReLU Linear ReLU Linear ReLU
    rot = lin(torch.relu(lin(torch.relu(lin(torch.relu(lat), 4)), 6)), 8)
    tra = lin(torch.relu(lin(torch.relu(lin(torch.relu(lat), 10)), 12)), 14)
    a1, a2 = rot[:, :3], rot[:, 3:]
    if kind == "plain":
        R = getz.r6d_to_matrix(rot)
        close64("rotation", want[:, :3, :3], R)
        assert float(a1.norm(dim=1).min()) > 0.25 and float((a2 - (R[:, 0] * a2).sum(1, keepdim=True) * R[:, 0]).norm(dim=1).min()) > 0.25
    else:
        assert bool((a1 == 0).all()) and bool((want[:, 0, :3] == 0).all()) and bool((want[:, 2, :3] == 0).all())
        close64("b2", want[:, 1, :3], a2 / a2.norm(dim=1, keepdim=True))
        assert bool((ref.total(terms)[:, 0, :3] == 0).all()) and bool((ref.total(terms)[:, 2, :3] == 0).all())
    close64("translation", want[:, :3, 3], tra)
    assert torch.equal(want[:, 3], torch.tensor([0., 0., 0., 1.], dtype=torch.float64).expand(B, 4))
    assert bool((ref.total(terms)[:, 3] == 0).all())
    what = "tail emulation " + ref.case_id(case)
    got = emu_tail(x["h"], nsplit, x["bias0"], w)
    inside(what, got, want, terms)
    assert torch.equal(got[:, 3], torch.tensor([0., 0., 0., 1.]).expand(B, 4))
    if kind == "degenerate":
        assert bool((got[:, 0, :3] == 0).all()) and bool((got[:, 2, :3] == 0).all())
    if kind == "plain" and B == 3:
        defects = ("relu", "bias", "last chunk") if nsplit else ("relu",)
        for defect in defects:
            outside(f"{what}, defect: {defect}", emu_tail(x["h"], nsplit, x["bias0"], w, defect), want, terms)
