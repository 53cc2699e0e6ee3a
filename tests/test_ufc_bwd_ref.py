"""The float64 references of tests/ufc_bwd_ref.py pinned on the CPU - every backward, fed the exact float64 forward outputs,
against float64 autograd through the matching oracle.ufc_ref.TorchOps operator (or the one-line torch statement) - and their
bounds calibrated from both sides with each kernel's arithmetic written in fp32 torch in the kernel's own order (two-pass and
online softmaxes with their group merges, split partials, wave trees, fp32 casts of float64 statistics): the plain emulation
stays inside every bound on every case the GPU tests use, and for every kernel a seeded defect of the kind the bound exists
for leaves it.  So tests/test_gpu_ufc_f64.py compares with something that was itself checked."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ufc_ref as oracle
from tests import ufc_bwd_ref as ref

F32 = torch.float32
BETA32 = torch.tensor(0.02, dtype=F32)
INF = float("inf")


# ------------------------------------------------------------------------------------------------------------------
# building blocks of the emulations
# ------------------------------------------------------------------------------------------------------------------
def tree_halving(x):
    """Sum of the last dim (a power of two) as lane 0 of an xor butterfly with offsets n/2 ... 1 forms it."""
    n = x.shape[-1]
    while n > 1:
        n //= 2
        x = x[..., :n] + x[..., n:2 * n]
    return x[..., 0]


def tree_adjacent(x):
    """The same for offsets 1, 2, 4, ...: neighbours first."""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def strided_sums(x, stride):
    """(..., n) -> (..., stride): thread i adds elements i, i + stride, ... in that order."""
    n = x.shape[-1]
    pad = ref.cdiv(n, stride) * stride - n
    x = F.pad(x, (0, pad)).reshape(*x.shape[:-1], -1, stride)
    acc = torch.zeros_like(x[..., 0, :])
    for i in range(x.shape[-2]):
        acc = acc + x[..., i, :]
    return acc


def block_sum256(x):
    """A 256-thread block's sum of the last dim: strided per thread, a wave tree, (w0 + w1) + (w2 + w3)."""
    w = tree_halving(strided_sums(x, 256).reshape(*x.shape[:-1], 4, 64))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def wave_sum64(x):
    return tree_halving(strided_sums(x, 64))


def seq_sum(x, dim):
    acc = torch.zeros_like(x.select(dim, 0))
    for i in range(x.shape[dim]):
        acc = acc + x.select(dim, i)
    return acc


def online_groups(a, payload, groups, beta=None):
    """The online softmax down the rows of a (N, S, T): thread (group g, column t) walks s = g, g + groups, ... with a running
    max, a sum and a payload accumulator (payload (N, S, K) or None), rescaling by expf((m_old - m_new) [/ beta]) when the
    max moves.  -> per-group (m, se (N, groups, T), acc (N, groups, T, K) or None)."""
    N, S, T = a.shape
    m = torch.full((N, groups, T), -INF, dtype=F32)
    se = torch.zeros(N, groups, T, dtype=F32)
    acc = torch.zeros(N, groups, T, payload.shape[-1], dtype=F32) if payload is not None else None
    sc = (lambda x: x / beta) if beta is not None else (lambda x: x)
    for i in range(ref.cdiv(S, groups)):
        rows = a[:, i * groups:(i + 1) * groups]
        g = rows.shape[1]
        mm = m[:, :g]
        up = rows > mm
        r = torch.where(up, torch.exp(sc(mm - rows)), torch.ones((), dtype=F32))
        mnew = torch.where(up, rows, mm)
        e = torch.exp(sc(rows - mnew))
        se[:, :g] = se[:, :g] * r + e
        if acc is not None:
            acc[:, :g] = acc[:, :g] * r.unsqueeze(-1) + e.unsqueeze(-1) * payload[:, i * groups:(i + 1) * groups].unsqueeze(2)
        m[:, :g] = mnew
    return m, se, acc


def merge_groups(m, se, acc, beta=None, skip_last=False):
    """The groups' partials merged in group order: M = max, r_q = 0 for an empty group or expf((m_q - M) [/ beta])."""
    G = m.shape[1] - (1 if skip_last else 0)
    sc = (lambda x: x / beta) if beta is not None else (lambda x: x)
    M = m[:, :G].max(1).values
    E = torch.zeros_like(M)
    A = torch.zeros_like(acc[:, 0]) if acc is not None else None
    for q in range(G):
        r = torch.where(m[:, q] == -INF, torch.zeros((), dtype=F32), torch.exp(sc(m[:, q] - M)))
        E = E + se[:, q] * r
        if acc is not None:
            A = A + acc[:, q] * r.unsqueeze(-1)
    return M, E, A


def lin11_f32(h):
    return -1.0 + (torch.tensor(2.0, dtype=F32) / torch.tensor(float(h - 1), dtype=F32)) * torch.arange(h, dtype=F32)


def coords_f32(h, swap=False):
    t = torch.arange(h * h)
    l = lin11_f32(h)
    return torch.stack((l[t // h], l[t % h]) if swap else (l[t % h], l[t // h]), 1)


# ------------------------------------------------------------------------------------------------------------------
# K8 emulation
# ------------------------------------------------------------------------------------------------------------------
def emu_argmax_fwd(c, h, defect=None):
    B, T, _ = c.shape
    xy = coords_f32(h)
    m = c.max(-1, keepdim=True).values
    e = torch.exp((c - m) / BETA32)
    tot = block_sum256(e)
    t_to_s = torch.stack([block_sum256(e * xy[:, i]) / tot for i in (0, 1)], 1)
    pm, pe, pa = online_groups(c, xy.expand(B, T, 2), ref.CR_GROUPS, BETA32)
    M, E, A = merge_groups(pm, pe, pa, BETA32, skip_last=defect == "last row group skipped")
    return t_to_s, (A / E.unsqueeze(-1)).transpose(1, 2).contiguous()


def emu_argmax_bwd(c, h, t_to_s, s_to_t, g1, g2, defect=None):
    B, T, _ = c.shape
    xy = coords_f32(h)
    m = c.max(-1, keepdim=True).values
    inv = 1.0 / (block_sum256(torch.exp((c - m) / BETA32)) * BETA32)
    p = torch.exp((c - m) / BETA32) * inv.unsqueeze(-1)
    br = lambda o, g, xy: (g[:, 0].unsqueeze(-1) * (xy[:, 0] - o[:, 0].unsqueeze(-1)) + g[:, 1].unsqueeze(-1) * (xy[:, 1] - o[:, 1].unsqueeze(-1)))
    dc = p * br(t_to_s, g1, xy)
    pm, pe, _ = online_groups(c, None, 4, BETA32)
    M = pm.max(1).values
    E = seq_sum(pe * torch.exp((pm - M.unsqueeze(1)) / BETA32), 1)
    inv = 1.0 / (E * BETA32)
    if defect == "1/beta once":                                       # the column direction forgets the derivative's 1 / beta
        inv = 1.0 / E
    q = torch.exp((c - M.unsqueeze(1)) / BETA32) * inv.unsqueeze(1)        # (B, S, T): column t's softmax over s
    xs = coords_f32(h, swap=defect == "x and y swapped in the column direction")
    return dc + q * br(s_to_t, g2, xs).transpose(1, 2)


# ------------------------------------------------------------------------------------------------------------------
# dual softmax emulation
# ------------------------------------------------------------------------------------------------------------------
def emu_dual_fwd(a, defect=None):
    B, L, M = a.shape
    rm = a.max(-1).values
    rs = wave_sum64(torch.exp(a - rm.unsqueeze(-1)))
    pm, pe, _ = online_groups(a, None, ref.CR_GROUPS)
    cm, cs, _ = merge_groups(pm, pe, None, skip_last=defect == "last row group skipped")
    rstat, cstat = torch.stack((rm, rs), -1), torch.stack((cm, cs), -1)
    f = (torch.exp(a - rm.unsqueeze(2)) / rs.unsqueeze(2)) * (torch.exp(a - cm.unsqueeze(1)) / cs.unsqueeze(1))
    return rstat, cstat, f


def emu_dual_bwd(a, rstat, cstat, f, df, defect=None):
    B, L, M = a.shape
    fd = f * df
    srow = wave_sum64(fd)
    part = strided_sums(fd.transpose(1, 2), ref.CR_GROUPS)                             # (B, M, groups)
    scol = seq_sum(part[..., :ref.CR_GROUPS - 1] if defect == "last row group skipped" else part, 2)
    r = torch.exp(a - rstat[..., 0].unsqueeze(2)) / rstat[..., 1].unsqueeze(2)
    c = torch.exp(a - cstat[..., 0].unsqueeze(1)) / cstat[..., 1].unsqueeze(1)
    return 2.0 * r * c * df - r * srow.unsqueeze(2) - c * scol.unsqueeze(1)


# ------------------------------------------------------------------------------------------------------------------
# K10 emulation
# ------------------------------------------------------------------------------------------------------------------
def _bh(x):
    """(B, n, H, C) -> (B H, n, C)"""
    B, n, H, C = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * H, n, C)


def _un_bh(x, B):
    BH, n, C = x.shape
    return x.reshape(B, BH // B, n, C).permute(0, 2, 1, 3).contiguous()


def emu_cross_fwd(corr, src_v, trg_v):
    B, H, S, T = corr.shape
    c, sv, tv = corr.reshape(B * H, S, T), _bh(src_v), _bh(trg_v)
    e = torch.exp(c - c.max(-1, keepdim=True).values)
    z = wave_sum64(e)
    prod = (e.unsqueeze(-1) * tv.unsqueeze(1)).transpose(2, 3)                          # (BH, S, C, T)
    halves = strided_sums(prod, 2)
    src = (halves[..., 0] + halves[..., 1]) / z.unsqueeze(-1)
    pm, pe, pa = online_groups(c, sv, ref.XC_GROUPS)
    M, Z, A = merge_groups(pm, pe, pa)
    return _un_bh(src, B), _un_bh(A * (1.0 / Z).unsqueeze(-1), B)


def emu_cross_bwd(corr, src_v, trg_v, src_attn, trg_attn, g_src, g_trg, defect=None):
    B, H, S, T = corr.shape
    c, sv, tv, sa, ta, g1, g2 = (corr.reshape(B * H, S, T), _bh(src_v), _bh(trg_v), _bh(src_attn), _bh(trg_attn), _bh(g_src), _bh(g_trg))
    m1 = c.max(-1).values
    iz1 = 1.0 / wave_sum64(torch.exp(c - m1.unsqueeze(-1)))
    r1 = tree_halving(g1 * sa)
    pm, pz, _ = online_groups(c, None, 8)
    m2, Z2, _ = merge_groups(pm, pz, None)
    iz2 = 1.0 / Z2
    r2 = seq_sum(g2 * ta, 2)
    if defect == "tail rows take the clamped row's r1" and S % 16:
        r1 = r1.clone()
        r1[:, S - S % 16:] = r1[:, S - 1:S]
    p1 = torch.exp(c - m1.unsqueeze(-1)) * iz1.unsqueeze(-1)
    p2 = torch.exp(c - m2.unsqueeze(1)) * iz2.unsqueeze(1)
    d1 = seq_sum(g1.unsqueeze(2) * tv.unsqueeze(1), 3)
    d2 = seq_sum(sv.unsqueeze(2) * g2.unsqueeze(1), 3)
    dc = p1 * (d1 - r1.unsqueeze(-1)) + p2 * (d2 - r2.unsqueeze(1))
    dsv = tree_adjacent(strided_sums((p2.unsqueeze(-1) * g2.unsqueeze(1)).transpose(2, 3), 16))       # (BH, S, C)
    dtv = seq_sum(strided_sums((p1.unsqueeze(-1) * g1.unsqueeze(2)).permute(0, 2, 3, 1), 16), 3)      # (BH, T, C)
    return dc.reshape(B, H, S, T), _un_bh(dsv, B), _un_bh(dtv, B)


# ------------------------------------------------------------------------------------------------------------------
# K9 emulation
# ------------------------------------------------------------------------------------------------------------------
def _elu1(x):
    return torch.where(x > 0, x + 1.0, torch.exp(torch.clamp(x, max=0.0)))


def _split_reduce(kphi, vals, wt, nsplit, drop_last=False):
    """sum over tokens of kphi_l (x) vals_l and of kphi_l wt_l: each split adds its lper tokens in order, the splits are added
    in order.  kphi (B, L, H, 32), vals (B, L, H, Dv) already scaled, wt (B, L, H) or None -> (B, H, 32, Dv), (B, H, 32)."""
    B, L, H, D = kphi.shape
    lper = ref.cdiv(L, nsplit)
    pad = nsplit * lper - L
    if drop_last:                                                  # the last token of every split contributes nothing
        keep = torch.ones(nsplit * lper, dtype=F32)
        keep[lper - 1::lper] = 0.0
        keep = keep[:L].view(1, L, 1, 1)
        kphi = kphi * keep
    w = kphi if wt is None else kphi * wt.unsqueeze(-1)
    pd = lambda x: F.pad(x, (0, 0, 0, 0, 0, pad)).reshape(B, nsplit, lper, H, -1)
    k5, v5, w5 = pd(kphi), pd(vals), pd(w)
    kv = torch.zeros(B, nsplit, H, D, vals.shape[-1], dtype=F32)
    ks = torch.zeros(B, nsplit, H, D, dtype=F32)
    for i in range(lper):
        kv = kv + k5[:, :, i].unsqueeze(-1) * v5[:, :, i].unsqueeze(-2)
        ks = ks + w5[:, :, i]
    return seq_sum(kv, 1), seq_sum(ks, 1)


def emu_linear_fwd(q, k, v, cm, nsplit, defect=None):
    vv = v.permute(0, 3, 1, 2) if cm else v
    B, L, H, Dv = vv.shape
    fL = torch.tensor(float(L), dtype=F32)
    kv, ks = _split_reduce(_elu1(k), vv * (1.0 / fL), None, nsplit, drop_last=defect == "last token of a split dropped")
    P = _elu1(q)
    z = 1.0 / (torch.einsum("blhd,bhd->blh", P, ks) + torch.tensor(1e-6, dtype=F32))
    out = torch.einsum("blhd,bhdv->blhv", P, kv) * z.unsqueeze(-1) * fL
    return ref._la_layout(out, cm)


def emu_linear_bwd(q, k, v, dout, cm, nsplit, defect=None):
    vv, g = (v.permute(0, 3, 1, 2), dout.permute(0, 3, 1, 2)) if cm else (v, dout)
    B, L, H, Dv = vv.shape
    fL = torch.tensor(float(L), dtype=F32)
    invL = 1.0 / fL
    drop = defect == "last token of a split dropped"
    P, N = _elu1(q), _elu1(k)
    kv, ks = _split_reduce(N, vv * invL, None, nsplit)
    T_ = torch.einsum("blhv,bhdv->blhd", g, kv)
    at = (P * T_).sum(-1)
    z = 1.0 / ((P * ks.unsqueeze(1)).sum(-1) + torch.tensor(1e-6, dtype=F32))
    dden = -fL * at * z * z
    dq = ((fL * z).unsqueeze(-1) * T_ + dden.unsqueeze(-1) * ks.unsqueeze(1)) * torch.where(q > 0, torch.ones((), dtype=F32), P)
    dkv, dks = _split_reduce(P, g * (fL * z).unsqueeze(-1), dden, nsplit, drop_last=drop)
    dphi_k = torch.ones_like(N) if defect == "phi' of a negative k taken as 1" else torch.where(k > 0, torch.ones((), dtype=F32), N)
    dk = (torch.einsum("bshv,bhdv->bshd", vv, dkv) * invL + dks.unsqueeze(1)) * dphi_k
    dv = torch.einsum("bshd,bhdv->bshv", N, dkv) * invL
    return dq, dk, ref._la_layout(dv, cm)


# ------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU, Conv4d data gradient, row normalisation
# ------------------------------------------------------------------------------------------------------------------
def _gn_f32_stats(stats, n):
    m = stats[:, 0] / n
    var = stats[:, 1] / n - m * m
    return m.float().view(-1, 1, 1), (1.0 / torch.sqrt(var + float(torch.tensor(1e-5, dtype=F32)))).float().view(-1, 1, 1)


def emu_gn_fwd(y, stats, w, b):
    mean, rstd = _gn_f32_stats(stats, y.shape[1] * y.shape[2])
    return torch.relu((y - mean) * rstd * w.view(1, -1, 1) + b.view(1, -1, 1))


def emu_gn_bwd(y, out, dout, stats, w, defect=None):
    B, C, npos = y.shape
    n = C * npos
    mean, rstd = _gn_f32_stats(stats, n)
    g = w.view(1, -1, 1)
    dz = torch.where(out > 0, dout, torch.zeros((), dtype=F32))
    yh = (y - mean) * rstd
    if npos % 4 == 0:                                              # fp32 sums of the four elements of a 16-byte load
        four = lambda x: seq_sum(x.reshape(B, C, npos // 4, 4), 3)
        s0, s1 = four(dz), four(dz * yh)
        a = [(s0 * g).double().sum(2), (s1 * g).double().sum(2), s1.double().sum(2), s0.double().sum(2)]
    else:
        a = [(dz * g).double().sum(2), (dz * g * yh).double().sum(2), (dz * yh).double().sum(2), dz.double().sum(2)]
    div = npos if defect == "npos where C npos belongs" else n
    m1, m2 = (a[0].sum(1) / div).float().view(-1, 1, 1), (a[1].sum(1) / div).float().view(-1, 1, 1)
    return rstd * (dz * g - m1 - yh * m2), a[2].sum(0).float(), a[3].sum(0).float()


def emu_dgrad(dy, wq, ws, defect=None):
    if defect == "one tap of the last channel dropped":
        ws = ws.clone()
        ws[-1, :, 0, 0] = 0.0
    B, Co, Hq, Wq, Hs, Ws = dy.shape
    Ci = wq.shape[1]
    a = F.conv_transpose2d(dy.permute(0, 4, 5, 1, 2, 3).reshape(B * Hs * Ws, Co, Hq, Wq), wq, padding=1)
    b = F.conv_transpose2d(dy.permute(0, 2, 3, 1, 4, 5).reshape(B * Hq * Wq, Co, Hs, Ws), ws, padding=1)
    return a.reshape(B, Hs, Ws, Ci, Hq, Wq).permute(0, 3, 4, 5, 1, 2) + b.reshape(B, Hq, Wq, Ci, Hs, Ws).permute(0, 3, 1, 2, 4, 5)


def emu_l2_fwd(x):
    return x / (torch.sqrt(wave_sum64(x * x)) + torch.tensor(1e-5, dtype=F32)).unsqueeze(1)


def emu_l2_bwd(x, y, dy, defect=None):
    r = torch.sqrt(wave_sum64(x * x))
    dot = wave_sum64(y * dy)
    inv = 1.0 / (r if defect == "eps dropped" else r + torch.tensor(1e-5, dtype=F32))
    k = dot / torch.clamp(r, min=1e-30)
    return dy * inv.unsqueeze(1) - y * k.unsqueeze(1)


# ------------------------------------------------------------------------------------------------------------------
# shared, cached: inputs, emulated forwards, references
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _argmax(case):
    x = ref.make_argmax_inputs(case)
    fwd = emu_argmax_fwd(x["c"], case[0])
    return x, fwd, ref.argmax_bwd_ref(x["c"], case[0], fwd[0], fwd[1], x["g1"], x["g2"])


@functools.lru_cache(maxsize=None)
def _dual(case):
    x = ref.make_dual_inputs(case)
    fwd = emu_dual_fwd(x["a"])
    return x, fwd, ref.dual_bwd_ref(x["a"], fwd[0], fwd[1], fwd[2], x["df"])


@functools.lru_cache(maxsize=None)
def _cross(case):
    x = ref.make_cross_inputs(case)
    return x, emu_cross_fwd(x["corr"], x["src_v"], x["trg_v"])


@functools.lru_cache(maxsize=None)
def _linear(case):
    x = ref.make_linear_inputs(case)
    return x, ref.linear_bwd_ref(x["q"], x["k"], x["v"], x["dout"], case[4], case[5])


@functools.lru_cache(maxsize=None)
def _gn(case):
    x = ref.make_gn_inputs(case)
    stats = ref.gn_moments(x["y"])[0]
    out = emu_gn_fwd(x["y"], stats, x["gn_w"], x["gn_b"])
    return x, stats, out, ref.gn_bwd_ref(x["y"], out, x["dout"], x["gn_w"])


@functools.lru_cache(maxsize=None)
def _dgrad(case):
    x = ref.make_dgrad_inputs(case)
    return x, ref.conv4d_dgrad_ref(x["dy"], x["wq"], x["ws"])


@functools.lru_cache(maxsize=None)
def _l2(case):
    x = ref.make_l2_inputs(case)
    y = emu_l2_fwd(x["x"])
    return x, y, ref.l2norm_bwd_ref(x["x"], y, x["dy"])


def _inside(what, got, want, terms):
    return ref.report(what, got, want, terms)


def _outside(what, got, want, terms):
    """A seeded defect: at least one element leaves the bound; prints how far the result moved on the scale of the output."""
    r = ref.ratio(got, want, ref.total(terms).expand_as(want))
    moved = float((got.double() - want).abs().max() / want.abs().max())
    print(f"{what}: worst err/bound {float(r.max()):.1f}, moved by {moved:.2e} of the largest entry")
    assert float(r.max()) > 1.0, what


rel = lambda a, b: float((a - b).abs().max() / b.abs().max())


def _pinned(what, got, grad, terms, ill_conditioned=False):
    """A reference against float64 autograd: 1e-12 of the largest entry.  Three kinds of case are ill-conditioned IN FLOAT64 -
    the whole gradient is a difference of terms many orders larger than itself, on autograd's side as on the reference's: the
    peaked soft-argmax (p ~ 1: every entry of dc below 1e-11, x - o cancels to 1e-14), the linear attention at L = 1 (out does
    not depend on q but through eps) and the row normalisation at C = 1 (dx = dy eps / (|x| + eps)^2).  No float64 arbiter
    resolves those to 1e-12 of their largest entry; for them, and element by element, the tolerance is that plus the reference's
    own bound - the sum of absolute values of the element's terms times its operation count - at float64's unit roundoff."""
    err = (got - grad).abs()
    slack = 1e-12 * grad.abs().max() + ref.total(terms).expand_as(got) * (2.0 ** -53 / ref.U)
    assert bool((err <= slack).all()), (what, float((err / slack).max()))
    if not ill_conditioned:
        assert rel(got, grad) <= 1e-12, (what, rel(got, grad))


@contextlib.contextmanager
def _float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


# ------------------------------------------------------------------------------------------------------------------
# 1. the references are pinned to float64 autograd
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.ARGMAX_CASES, ids=ref.case_id)
def test_argmax_references_are_float64_autograd_of_the_oracle(case):
    """TorchOps._soft_argmax in both directions as TorchOps.soft_argmax_pair calls it, with the fp32 value of beta the kernel
    is handed and float64 coordinates."""
    h, B, _ = case
    x = ref.make_argmax_inputs(case)
    c = x["c"].double().requires_grad_(True)
    with _float64_default():
        c6 = c.view(B, 1, h, h, h, h)
        gx, gy = oracle.TorchOps._soft_argmax(c6.permute(0, 1, 4, 5, 2, 3).flatten(1, 3), beta=ref.BETA)
        t_to_s = torch.cat((gx, gy), 1).reshape(B, 2, h * h)
        gx, gy = oracle.TorchOps._soft_argmax(c6.flatten(1, 3), beta=ref.BETA)
        s_to_t = torch.cat((gx, gy), 1).reshape(B, 2, h * h)
    ((t_to_s * x["g1"].double()).sum() + (s_to_t * x["g2"].double()).sum()).backward()
    fwd = ref.argmax_fwd_ref(x["c"], h)
    assert rel(fwd["t_to_s"], t_to_s.detach()) <= 1e-12 and rel(fwd["s_to_t"], s_to_t.detach()) <= 1e-12
    dc, terms = ref.argmax_bwd_ref(x["c"], h, t_to_s.detach(), s_to_t.detach(), x["g1"], x["g2"])
    _pinned("dc", dc, c.grad, terms, ill_conditioned=case[2] == "peaked")


@pytest.mark.parametrize("case", ref.DUAL_CASES, ids=ref.case_id)
def test_dual_softmax_references_are_float64_autograd(case):
    x = ref.make_dual_inputs(case)
    a = x["a"].double().requires_grad_(True)
    f = oracle.TorchOps.dual_softmax(a)
    (f * x["df"].double()).sum().backward()
    st = ref.dual_stats_ref(x["a"])
    rstat, cstat = torch.stack((st["rmax"], st["rsum"]), -1), torch.stack((st["cmax"], st["csum"]), -1)
    assert rel(ref.dual_f_ref(x["a"], rstat, cstat)[0], f.detach()) <= 1e-12
    assert rel(ref.dual_bwd_ref(x["a"], rstat, cstat, f.detach(), x["df"])[0], a.grad) <= 1e-12


@pytest.mark.parametrize("case", [c for c in ref.CROSS_CASES if c != ref.CROSS_BIG], ids=ref.case_id)
def test_cross_attention_references_are_float64_autograd_of_the_oracle(case):
    x = ref.make_cross_inputs(case)
    c, sv, tv = (x[k].double().requires_grad_(True) for k in ("corr", "src_v", "trg_v"))
    sa, ta = oracle.TorchOps.cross_attention(c, sv, tv)
    ((sa * x["g_src"].double()).sum() + (ta * x["g_trg"].double()).sum()).backward()
    fwd = ref.cross_fwd_ref(x["corr"], x["src_v"], x["trg_v"])
    assert rel(fwd["src_attn"], sa.detach()) <= 1e-12 and rel(fwd["trg_attn"], ta.detach()) <= 1e-12
    got = ref.cross_bwd_ref(x["corr"], x["src_v"], x["trg_v"], sa.detach(), ta.detach(), x["g_src"], x["g_trg"])
    if case[2] * case[3] > 1:                                       # one row and one column: dcorr is identically 0
        assert rel(got["dcorr"], c.grad) <= 1e-12
    else:
        assert float(got["dcorr"].abs().max()) <= 1e-12 and float(c.grad.abs().max()) <= 1e-12
    assert rel(got["dsrc_v"], sv.grad) <= 1e-12 and rel(got["dtrg_v"], tv.grad) <= 1e-12


@pytest.mark.parametrize("case", [c for c in ref.LINEAR_CASES if c != ref.LINEAR_BIG], ids=ref.case_id)
def test_linear_attention_references_are_float64_autograd_of_the_oracle(case):
    B, L, H, Dv, cm, nsplit, gain = case
    x = ref.make_linear_inputs(case)
    q, k, v = (x[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    out = oracle.TorchOps.linear_attention(q, k, v, channel_major=bool(cm), eps=ref.EPS_LA)
    (out * x["dout"].double()).sum().backward()
    assert rel(ref.linear_fwd_ref(x["q"], x["k"], x["v"], cm, nsplit)[0], out.detach()) <= 1e-12
    got = ref.linear_bwd_ref(x["q"], x["k"], x["v"], x["dout"], cm, nsplit)
    assert bool((x["q"] == 0).any()) and bool((x["k"] == 0).any())
    for name, grad in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        _pinned(name, got[name], grad, got[name + "_terms"], ill_conditioned=L == 1)


@pytest.mark.parametrize("case", ref.GN_CASES, ids=ref.case_id)
def test_gn_relu_references_are_float64_autograd(case):
    x = ref.make_gn_inputs(case)
    y, w, b = (x[n].double().requires_grad_(True) for n in ("y", "gn_w", "gn_b"))
    out = F.relu(F.group_norm(y, 1, w, b, ref.EPS_GN))
    (out * x["dout"].double()).sum().backward()
    assert rel(ref.gn_fwd_ref(x["y"], x["gn_w"], x["gn_b"])[0], out.detach()) <= 1e-12
    got = ref.gn_bwd_ref(x["y"], out.detach(), x["dout"].double(), x["gn_w"])
    assert rel(got["dy"], y.grad) <= 1e-12 and rel(got["dgn_w"], w.grad) <= 1e-12 and rel(got["dgn_b"], b.grad) <= 1e-12
    assert case[1] == 1 or (bool((x["gn_w"] < 0).any()) and bool((x["gn_w"] > 0).any()))


@pytest.mark.parametrize("case", ref.DGRAD_CASES, ids=ref.case_id)
def test_conv4d_dgrad_reference_is_float64_autograd_of_the_oracle(case):
    B, Co, Ci, Hq, Wq, Hs, Ws = case
    x = ref.make_dgrad_inputs(case)
    xin = torch.zeros(B, Ci, Hq, Wq, Hs, Ws, dtype=torch.float64, requires_grad=True)
    zero = torch.zeros(Co, dtype=torch.float64)
    y = oracle.conv4d(xin, x["wq"].double(), zero, x["ws"].double(), zero, 3, 1, 1)
    (y * x["dy"].double()).sum().backward()
    assert rel(ref.conv4d_dgrad_ref(x["dy"], x["wq"], x["ws"])[0], xin.grad) <= 1e-12


@pytest.mark.parametrize("case", ref.L2_CASES, ids=ref.case_id)
def test_l2norm_references_are_float64_autograd(case):
    """Autograd through x / (|x| + eps) on the rows that are not exactly 0 (the inputs of the `zero` kind without row 1: norm's
    gradient at 0 is NaN); on that row the closed form dy / eps."""
    x = ref.make_l2_inputs(case)
    keep = [i for i in range(case[0]) if not (case[2] == "zero" and i == 1)]
    xs = x["x"][keep].double().requires_grad_(True)
    y = oracle.l2_normalise_tokens(xs, eps=ref.EPS_NORM)
    (y * x["dy"][keep].double()).sum().backward()
    assert rel(ref.l2norm_fwd_ref(x["x"][keep])[0], y.detach()) <= 1e-12
    dx, terms = ref.l2norm_bwd_ref(x["x"][keep], y.detach(), x["dy"][keep])
    _pinned("dx", dx, xs.grad, terms, ill_conditioned=case[1] == 1)
    if case[2] == "zero":
        z = torch.zeros(1, case[1])
        assert rel(ref.l2norm_bwd_ref(z, z, x["dy"][1:2])[0], x["dy"][1:2].double() / ref.EPS_NORM) <= 1e-15


# ------------------------------------------------------------------------------------------------------------------
# 2. the emulations stay inside every bound on every GPU case
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.ARGMAX_CASES, ids=ref.case_id)
def test_argmax_emulation_is_inside_the_bounds(case):
    x, fwd, (want, terms) = _argmax(case)
    f = ref.argmax_fwd_ref(x["c"], case[0])
    _inside("t_to_s", fwd[0], f["t_to_s"], f["t_to_s_terms"])
    _inside("s_to_t", fwd[1], f["s_to_t"], f["s_to_t_terms"])
    _inside("dc", emu_argmax_bwd(x["c"], case[0], fwd[0], fwd[1], x["g1"], x["g2"]), want, terms)
    if case[2] == "tied":
        c = x["c"]
        assert bool(((c[:, 1] == c[:, 1].max(-1, keepdim=True).values).sum(-1) == 2).all())
        assert bool(((c[:, :, 2] == c[:, :, 2].max(-1, keepdim=True).values).sum(-1) == 2).all())
    if case[2] == "peaked":
        assert float(torch.softmax(x["c"].double() / ref.BETA, -1).max(-1).values.min()) > 0.99


@pytest.mark.parametrize("case", ref.DUAL_CASES, ids=ref.case_id)
def test_dual_softmax_emulation_is_inside_the_bounds(case):
    x, (rstat, cstat, f), (want, terms) = _dual(case)
    st = ref.dual_stats_ref(x["a"])
    assert torch.equal(rstat[..., 0].double(), st["rmax"]) and torch.equal(cstat[..., 0].double(), st["cmax"])
    _inside("rsum", rstat[..., 1], st["rsum"], st["rsum_terms"])
    _inside("csum", cstat[..., 1], st["csum"], st["csum_terms"])
    _inside("f", f, *ref.dual_f_ref(x["a"], rstat, cstat))
    _inside("da", emu_dual_bwd(x["a"], rstat, cstat, f, x["df"]), want, terms)


def _cross_grads(x, variant):
    g1 = torch.zeros_like(x["g_src"]) if variant == "g_src=0" else x["g_src"]
    g2 = torch.zeros_like(x["g_trg"]) if variant == "g_trg=0" else x["g_trg"]
    return g1, g2


# (the 512 x 512 case runs once on the CPU)
@pytest.mark.parametrize("case,variant", [(c, v) for c in ref.CROSS_CASES for v in ref.CROSS_VARIANTS if c != ref.CROSS_BIG or v == "both"],
                         ids=lambda p: p if isinstance(p, str) else ref.case_id(p))
def test_cross_attention_emulation_is_inside_the_bounds(case, variant):
    x, (sa, ta) = _cross(case)
    if variant == "both":
        f = ref.cross_fwd_ref(x["corr"], x["src_v"], x["trg_v"])
        _inside("src_attn", sa, f["src_attn"], f["src_attn_terms"])
        _inside("trg_attn", ta, f["trg_attn"], f["trg_attn_terms"])
    g1, g2 = _cross_grads(x, variant)
    want = ref.cross_bwd_ref(x["corr"], x["src_v"], x["trg_v"], sa, ta, g1, g2)
    got = emu_cross_bwd(x["corr"], x["src_v"], x["trg_v"], sa, ta, g1, g2)
    for name, t in zip(("dcorr", "dsrc_v", "dtrg_v"), got):
        _inside(name, t, want[name], want[name + "_terms"])


@pytest.mark.parametrize("case", ref.LINEAR_CASES, ids=ref.case_id)
def test_linear_attention_emulation_is_inside_the_bounds(case):
    B, L, H, Dv, cm, nsplit, gain = case
    x, want = _linear(case)
    _inside("out", emu_linear_fwd(x["q"], x["k"], x["v"], cm, nsplit), *ref.linear_fwd_ref(x["q"], x["k"], x["v"], cm, nsplit))
    for name, t in zip(("dq", "dk", "dv"), emu_linear_bwd(x["q"], x["k"], x["v"], x["dout"], cm, nsplit)):
        _inside(name, t, want[name], want[name + "_terms"])


@pytest.mark.parametrize("case", ref.GN_CASES, ids=ref.case_id)
def test_gn_relu_emulation_is_inside_the_bounds(case):
    x, stats, out, want = _gn(case)
    _inside("out", out, *ref.gn_fwd_ref(x["y"], x["gn_w"], x["gn_b"]))
    for name, t in zip(("dy", "dgn_w", "dgn_b"), emu_gn_bwd(x["y"], out, x["dout"], stats, x["gn_w"])):
        _inside(name, t, want[name], want[name + "_terms"])


@pytest.mark.parametrize("case", ref.DGRAD_CASES, ids=ref.case_id)
def test_conv4d_dgrad_emulation_is_inside_the_bound(case):
    x, (want, terms) = _dgrad(case)
    _inside("dx", emu_dgrad(x["dy"], x["wq"], x["ws"]), want, terms)


@pytest.mark.parametrize("case", ref.L2_CASES, ids=ref.case_id)
def test_l2norm_emulation_is_inside_the_bounds(case):
    x, y, (want, terms) = _l2(case)
    _inside("y", y, *ref.l2norm_fwd_ref(x["x"]))
    _inside("dx", emu_l2_bwd(x["x"], y, x["dy"]), want, terms)


# ------------------------------------------------------------------------------------------------------------------
# 3. seeded defects leave the bounds
# ------------------------------------------------------------------------------------------------------------------
def test_seeded_defects_leave_the_argmax_bounds():
    case = (9, 1, "realistic")
    x, fwd, (want, terms) = _argmax(case)
    f = ref.argmax_fwd_ref(x["c"], 9)
    _outside("s_to_t, last row group skipped", emu_argmax_fwd(x["c"], 9, "last row group skipped")[1], f["s_to_t"], f["s_to_t_terms"])
    for defect in ("x and y swapped in the column direction", "1/beta once"):
        _outside("dc, " + defect, emu_argmax_bwd(x["c"], 9, fwd[0], fwd[1], x["g1"], x["g2"], defect), want, terms)


def test_seeded_defects_leave_the_dual_softmax_bounds():
    case = (2, 70, 130, 2)
    x, (rstat, cstat, f), (want, terms) = _dual(case)
    st = ref.dual_stats_ref(x["a"])
    _outside("csum, last row group skipped", emu_dual_fwd(x["a"], "last row group skipped")[1][..., 1], st["csum"], st["csum_terms"])
    _outside("da, last row group skipped", emu_dual_bwd(x["a"], rstat, cstat, f, x["df"], "last row group skipped"), want, terms)


def test_seeded_defect_leaves_the_cross_attention_bound():
    case = (2, 3, 40, 56, 3)
    x, (sa, ta) = _cross(case)
    want = ref.cross_bwd_ref(x["corr"], x["src_v"], x["trg_v"], sa, ta, x["g_src"], x["g_trg"])
    got = emu_cross_bwd(x["corr"], x["src_v"], x["trg_v"], sa, ta, x["g_src"], x["g_trg"], "tail rows take the clamped row's r1")
    _outside("dcorr, tail rows take the clamped row's r1", got[0], want["dcorr"], want["dcorr_terms"])


def test_seeded_defects_leave_the_linear_attention_bounds():
    case = (2, 100, 3, 40, 0, 3, 0.7)
    B, L, H, Dv, cm, nsplit, gain = case
    x, want = _linear(case)
    got = emu_linear_bwd(x["q"], x["k"], x["v"], x["dout"], cm, nsplit, "phi' of a negative k taken as 1")
    _outside("dk, phi' of a negative k taken as 1", got[1], want["dk"], want["dk_terms"])
    got = emu_linear_bwd(x["q"], x["k"], x["v"], x["dout"], cm, nsplit, "last token of a split dropped")
    _outside("dv, last token of a split dropped", got[2], want["dv"], want["dv_terms"])
    fw, ft = ref.linear_fwd_ref(x["q"], x["k"], x["v"], cm, nsplit)
    _outside("out, last token of a split dropped", emu_linear_fwd(x["q"], x["k"], x["v"], cm, nsplit, "last token of a split dropped"), fw, ft)


def test_seeded_defects_leave_the_gn_dgrad_and_l2norm_bounds():
    x, stats, out, want = _gn((2, 5, 625, 0.0))
    _outside("dy, npos where C npos belongs", emu_gn_bwd(x["y"], out, x["dout"], stats, x["gn_w"], "npos where C npos belongs")[0],
             want["dy"], want["dy_terms"])
    x, (want, terms) = _dgrad((2, 8, 8, 8, 8, 8, 8))
    _outside("dx, one tap of the last channel dropped", emu_dgrad(x["dy"], x["wq"], x["ws"], "one tap of the last channel dropped"), want, terms)
    x, y, (want, terms) = _l2((4, 64, "tiny"))
    _outside("dx, eps dropped", emu_l2_bwd(x["x"], y, x["dy"], "eps dropped"), want, terms)
