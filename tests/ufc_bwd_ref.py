"""Float64 references, with element-wise error bounds, of the fp32 kernels behind the training backward of get_z - the
soft-argmax pair, the dual softmax, the cost-volume cross attention, the linear attention, GroupNorm + ReLU, the Conv4d data
gradient, the row normalisation's VJP (csrc/ufc_match.hip, csrc/ufc_conv4d.hip, csrc/ufc_corr.hip, csrc/ufc_attn.hip) - and the case lists, for tests/test_ufc_bwd_ref.py
(CPU) and tests/test_gpu_ufc_f64.py (GPU).  Helpers, not tests.

Every reference takes the values a kernel READS (fp32 bits converted to float64; a backward that is handed forward outputs or
statistics gets exactly those) and forms in float64 what include/coponerf_hip.h says the entry computes.  Every bound is first
order in u = 2^-24 and comes from the kernel's operation count:

    gam(n) = n u / (1 - n u)   times the float64 SUM OF ABSOLUTE VALUES of the element's terms (never |want|), n = the longest
                               chain of additions of the element plus its element-wise roundings;
    an expf                    is taken as exact to 1 ulp (2 u relative) of its ROUNDED argument; an argument formed by k
                               roundings of relative size u moves the exponential by k u |arg| relative (|arg| reaches 100 in
                               the soft-argmax at beta = 0.02).  An exponential below the normal range may be flushed: 2^-126
                               absolute;
    an ONLINE softmax          (running max m, sum rescaled by expf(m_old - m_new) when the max moves) multiplies a term by at
                               most one factor per row its thread walks after it, and one more in the merge of the groups; all
                               the arguments have one sign and add up to the single argument (x - M), so the |arg| part is the
                               same as in the two-pass form and only the count of roundings grows: 3 per rescale;
    a float64 -> fp32 cast     of a statistic costs half an ulp, u relative.
Each reference returns its bound's terms separately (a dict name -> tensor) so a test can print which term an error uses;
the bound is their sum.
"""
import zlib

import torch
import torch.nn.functional as F

from tests.attend_ref import assert_within, ratio                      # noqa: F401  (re-exported: the comparison helpers)

U = 2.0 ** -24
FLOOR = 2.0 ** -126                 # smallest normal fp32: the absolute error of a flushed exponential or product
CR_COLS, CR_GROUPS, XB_PARTS, XC_GROUPS = 16, 64, 8, 16
BETA = float(torch.tensor(0.02, dtype=torch.float32))                  # the kernel is handed the fp32 value
EPS_NORM = float(torch.tensor(1e-5, dtype=torch.float32))
EPS_GN = float(torch.tensor(1e-5, dtype=torch.float32))
EPS_LA = float(torch.tensor(1e-6, dtype=torch.float32))


def gam(n):
    return n * U / (1.0 - n * U)


def cdiv(a, b):
    return -(-a // b)


def total(terms):
    return sum(terms.values())


def report(what, got, want, terms):
    """assert_within on the summed bound; before it, which terms make up the bound at the element with the worst err / bound."""
    bound = total(terms).expand_as(want)
    i = int(ratio(got, want, bound).reshape(-1).argmax())
    share = ", ".join(f"{name} {float(t.expand_as(want).reshape(-1)[i] / bound.reshape(-1)[i]):.0%}" for name, t in terms.items())
    print(f"    {what}: at the worst element the bound is {share}")
    return assert_within(what, got, want, bound)


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
# (h, B, regime)
ARGMAX_CASES = [(2, 1, "flat"), (2, 2, "tied"), (5, 2, "realistic"), (5, 1, "peaked"), (9, 1, "realistic"), (9, 2, "tied"),
                (16, 2, "realistic"), (16, 1, "peaked"), (16, 1, "flat"), (32, 1, "realistic"), (32, 1, "peaked")]
# (B, L, M, gain)
DUAL_CASES = [(1, 1, 7, 2), (2, 3, 40, 8), (2, 70, 130, 2), (2, 70, 130, 8), (1, 65, 17, 8), (1, 300, 530, 2), (1, 300, 530, 8)]
# (B, H, S, T, gain)
CROSS_CASES = [(1, 1, 1, 1, 3), (1, 2, 5, 3, 3), (1, 2, 5, 3, 12), (2, 3, 17, 33, 3), (2, 3, 17, 33, 12), (2, 3, 40, 56, 3),
               (1, 1, 512, 512, 12)]
CROSS_BIG = (1, 1, 512, 512, 12)
CROSS_VARIANTS = ["both", "g_src=0", "g_trg=0"]
# (B, L, H, Dv, channel_major, nsplit, gain)
LINEAR_CASES = [(1, 1, 1, 1, 0, 1, 0.7), (2, 33, 3, 32, 0, 1, 3.0), (2, 100, 3, 40, 0, 3, 0.7), (1, 100, 2, 33, 1, 64, 3.0),
                (2, 150, 3, 72, 1, 2, 0.7), (1, 130, 2, 65, 0, 2, 3.0), (1, 1024, 8, 256, 1, 16, 0.7)]
LINEAR_BIG = (1, 1024, 8, 256, 1, 16, 0.7)
LINEAR_NSPLIT_PAIRS = [((2, 100, 3, 40, 0, 3, 0.7), 1), ((1, 100, 2, 33, 1, 64, 3.0), 7)]      # (case, the other nsplit)
# (B, C, npos, offset): offset = the mean of y in units of its spread
GN_CASES = [(1, 1, 3, 0.0), (2, 5, 625, 0.0), (3, 8, 1296, 5.0), (1, 32, 65536, 0.0), (2, 3, 4100, 0.0)]
# (B, Cout, Cin, Hq, Wq, Hs, Ws)
DGRAD_CASES = [(2, 8, 8, 8, 8, 8, 8), (1, 32, 8, 16, 16, 16, 16), (1, 8, 32, 8, 8, 8, 8), (3, 12, 20, 4, 4, 4, 4),
               (1, 8, 4, 6, 6, 6, 6), (2, 5, 8, 6, 6, 6, 6), (1, 8, 8, 4, 8, 8, 16)]
# (rows, C, kind): kind "plain", "tiny" (|x| ~ 1e-4: eps is a tenth of the norm), "zero" (row 1 is exactly 0)
L2_CASES = [(1, 16, "plain"), (4, 64, "tiny"), (5, 100, "plain"), (5, 64, "zero"), (4, 1024, "plain"), (5, 1, "plain"),
            (1000, 64, "plain"), (1000, 16, "tiny")]
TRANSPOSE_CASES = [(1, 1, 1), (3, 31, 33), (2, 256, 16), (6, 100, 4096)]


def case_id(c):
    return "-".join(str(v) for v in c)


def _gen(*key):
    """A generator seeded by the case itself (stable across processes)."""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------------------------
# the expectation under a softmax: the form shared by the soft-argmax forward and the cross attention's forward
# ------------------------------------------------------------------------------------------------------------------
def softmax_parts(arg):
    """arg (..., n) float64, <= 0 with a 0 in every row -> (p, e, E): exp(arg), its row sum, the weights."""
    e = torch.exp(arg)
    E = e.sum(-1, keepdim=True)
    return e / E, e, E


def exp_rel(arg, k_arg, n_round):
    """Relative error of one weight's numerator: k_arg roundings of the argument, n_round roundings of exponentials and
    rescaling products (2 for a lone expf)."""
    return (k_arg * arg.abs() + n_round) * U


def expect_ref(arg, vals, k_arg, n_round, n_sum):
    """out[..., c] = sum_t p_t vals[..., t, c], p = softmax(arg) -> (want, terms).  The numerator and the denominator carry
    the SAME error of every exponential, so a relative error d_t of e_t moves the quotient by p_t d_t (v_t - out):
        expf       sum_t p_t |v_t - out| exp_rel_t
        sum        gam(n_sum) sum_t p_t (|v_t| + |out|)     (the additions round the two sums separately)
        underflow  2^-126 sum_t (|v_t| + |out|)             (E >= 1: the maximum's exponential is 1)"""
    p, e, E = softmax_parts(arg)
    out = torch.einsum("...t,...tc->...c", p, vals)
    dev = (vals - out.unsqueeze(-2)).abs()
    mag = vals.abs() + out.abs().unsqueeze(-2)
    terms = {"expf": torch.einsum("...t,...tc->...c", p * exp_rel(arg, k_arg, n_round), dev),
             "sum": gam(n_sum) * torch.einsum("...t,...tc->...c", p, mag),
             "underflow": FLOOR * mag.sum(-2)}
    return out, terms


def weight_rel(arg, p, k_arg, n_round, n_sum):
    """Relative error of a recomputed softmax weight e_t * (1 / E): its own exponential, the sum's share of every
    exponential's error, the additions of the sum, the reciprocal and the product."""
    return exp_rel(arg, k_arg, n_round) + (p * exp_rel(arg, k_arg, n_round)).sum(-1, keepdim=True) + gam(n_sum + 2)


# ------------------------------------------------------------------------------------------------------------------
# K8: soft-argmax pair
# ------------------------------------------------------------------------------------------------------------------
def lin11(h):
    return torch.linspace(-1.0, 1.0, h, dtype=torch.float64)


def coords(h):
    """(T, 2): (x, y) = (lin11(t % h), lin11(t / h)) of position t."""
    t = torch.arange(h * h)
    l = lin11(h)
    return torch.stack((l[t % h], l[t // h]), 1)


def coord_err(x):
    """Absolute error of lin11(i, n) = -1 + fl(2 / (n - 1)) i in fp32: the quotient and the product round relative to
    |x + 1| <= 2, the sum relative to |x| - an ABSOLUTE error of up to 4 u where the coordinate itself is near 0."""
    return U * (2 * (x + 1).abs() + x.abs())


def _argmax_counts(h):
    """Operation counts of the four soft-argmax kernels at T = h h.
    rows (two-pass, 256 threads): a weight is one expf of (c - m) / beta (2 roundings of the argument); a sum is
        ceil(T / 256) additions per thread, 6 wave steps, 2 across the waves; the coordinate lin11 costs 3 roundings, its
        product 1, the final division 1.
    cols forward (online, CR_GROUPS row groups): a thread walks ceil(T / 64) rows, each of which may rescale (3 roundings);
        the merge adds one expf, one product and CR_GROUPS additions.
    cols backward (online, 4 row groups): the same with ceil(T / 4) rows per thread and 4 groups."""
    T = h * h
    kf, kb = cdiv(T, CR_GROUPS), cdiv(T, 4)
    return {"rows": dict(n_round=2, n_sum=cdiv(T, 256) + 8 + 5),
            "cols": dict(n_round=2 + 3 * (kf + 1), n_sum=kf + CR_GROUPS + 6),
            "rows_bwd": dict(n_round=2, n_sum=cdiv(T, 256) + 8 + 2),
            "cols_bwd": dict(n_round=2 + 3 * (kb + 1), n_sum=kb + 4 + 2)}


def argmax_fwd_ref(c, h):
    """c (B, T, T) -> dict: t_to_s, s_to_t (B, 2, T) and their terms (see expect_ref; `coord`: sum_t p_t coord_err_t)."""
    B, T = c.shape[0], h * h
    c = c.double()
    n = _argmax_counts(h)
    xy = coords(h)
    res = {}
    for name, a, cnt in (("t_to_s", c, n["rows"]), ("s_to_t", c.transpose(1, 2), n["cols"])):
        arg = (a - a.max(-1, keepdim=True).values) / BETA
        want, terms = expect_ref(arg, xy.expand(B, T, T, 2), 2, cnt["n_round"], cnt["n_sum"])
        terms["coord"] = torch.einsum("bst,tc->bsc", softmax_parts(arg)[0], coord_err(xy))
        res[name] = want.transpose(1, 2).contiguous()                                   # (B, 2, T)
        res[name + "_terms"] = {k: v.transpose(1, 2).contiguous() for k, v in terms.items()}
    return res


def _argmax_bwd_dir(a, o, g, h, cnt):
    """One direction: a (B, n_keep, n_red) logits, o / g (B, 2, n_keep) forward output (as the kernel reads it) and its
    gradient -> d (B, n_keep, n_red) = p / beta (gx (x - ox) + gy (y - oy)) and the terms
        weight   |d| weight_rel   (the recomputed p / beta: one more product, by beta)
        bracket  p / beta (gam(4) (|gx| (|x| + |ox|) + |gy| (|y| + |oy|)) + |gx| coord_err(x) + |gy| coord_err(y))    (the
                 difference, the product, the sum of the two and the product with p / beta: 4; lin11's own error is absolute,
                 see coord_err) - the bracket is a difference of near-equal terms where p is large
        underflow 2^-126 (|bracket| / beta + 2)        (the weight, or the product, below the normal range)"""
    arg = (a - a.max(-1, keepdim=True).values) / BETA
    p, e, E = softmax_parts(arg)
    xy = coords(h)                                                                      # (n_red, 2)
    ox, oy, gx, gy = (t.unsqueeze(-1) for t in (o[:, 0], o[:, 1], g[:, 0], g[:, 1]))    # (B, n_keep, 1)
    x, y = xy[:, 0].view(1, 1, -1), xy[:, 1].view(1, 1, -1)
    br = gx * (x - ox) + gy * (y - oy)
    mag = gx.abs() * (x.abs() + ox.abs()) + gy.abs() * (y.abs() + oy.abs())
    d = p / BETA * br
    terms = {"weight": d.abs() * (weight_rel(arg, p, 2, cnt["n_round"], cnt["n_sum"]) + 2 * U),
             "bracket": p / BETA * (gam(4) * mag + gx.abs() * coord_err(x) + gy.abs() * coord_err(y)),
             "underflow": FLOOR * (br.abs() / BETA + 2)}
    return d, terms


def argmax_bwd_ref(c, h, t_to_s, s_to_t, g_t_to_s, g_s_to_t):
    """dc (B, T, T) = rows part + columns part, with the forward outputs as GIVEN; the last addition (the column kernel's
    `+=` on what the row kernel wrote) rounds once: u (|rows part| + |cols part|), in `bracket`."""
    c = c.double()
    n = _argmax_counts(h)
    dr, tr = _argmax_bwd_dir(c, t_to_s.double(), g_t_to_s.double(), h, n["rows_bwd"])
    dc_, tc = _argmax_bwd_dir(c.transpose(1, 2), s_to_t.double(), g_s_to_t.double(), h, n["cols_bwd"])
    dc_ = dc_.transpose(1, 2)
    terms = {k: tr[k] + tc[k].transpose(1, 2) for k in tr}
    terms["bracket"] = terms["bracket"] + U * (dr.abs() + dc_.abs())
    return dr + dc_, terms


def make_argmax_inputs(case):
    """c (B, T, T) fp32 of the regime, g_t_to_s / g_s_to_t (B, 2, T) fp32."""
    h, B, regime = case
    T = h * h
    gen = _gen("argmax", h, B, regime)
    if regime == "flat":
        c = torch.randn(B, T, T, generator=gen) * 0.05
    elif regime in ("realistic", "tied"):
        s, t = torch.randn(B, T, 64, generator=gen), torch.randn(B, T, 64, generator=gen)
        # neighbouring tokens share most of their direction, as image features do: correlations spread over [-1, 1]
        base = torch.randn(B, 1, 64, generator=gen)
        s, t = s + 0.7 * base + 0.8 * t, t + 0.7 * base
        c = torch.einsum("bsc,btc->bst", F.normalize(s, dim=-1), F.normalize(t, dim=-1))
        if regime == "tied":                                  # two exactly equal maxima in row 1 and in column 2
            c[:, 1, 0] = c[:, 1, 3] = c[:, 1].max(-1).values + 0.015625
            c[:, 0, 2] = c[:, 3, 2] = c[:, :, 2].max(-1).values + 0.015625
    else:                                                     # peaked: one entry per row and per column near 0.95
        c = torch.rand(B, T, T, generator=gen) * 0.6 - 0.3
        for b in range(B):
            perm = torch.randperm(T, generator=gen)
            c[b, torch.arange(T), perm] = 0.95 + 0.01 * torch.rand(T, generator=gen)
    return {"c": c.float().contiguous(), "g1": torch.randn(B, 2, T, generator=gen), "g2": torch.randn(B, 2, T, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# dual softmax
# ------------------------------------------------------------------------------------------------------------------
def dual_stats_ref(a):
    """a (B, L, M) -> dict: rmax, rsum (B, L), cmax, csum (B, M) and the terms of the two sums (the maxima are exact):
        expf      S sum_j p_j (|a_j - max| + n_round) u      (one rounding of the argument: the difference)
        sum       gam(n) S       rows: ceil(M / 64) additions per lane and 6 wave steps; columns: ceil(L / 64) per thread and
                                 CR_GROUPS in the merge, which also multiplies once
        underflow 2^-126 times the number of terms"""
    a = a.double()
    B, L, M = a.shape
    res = {}
    k = cdiv(L, CR_GROUPS)
    for name, x, n_round, n_sum in (("r", a, 2, cdiv(M, 64) + 6), ("c", a.transpose(1, 2), 2 + 3 * (k + 1), k + CR_GROUPS + 1)):
        mx = x.max(-1, keepdim=True).values
        arg = x - mx
        p, e, E = softmax_parts(arg)
        res[name + "max"], res[name + "sum"] = mx.squeeze(-1), E.squeeze(-1)
        res[name + "sum_terms"] = {"expf": (E * (p * exp_rel(arg, 1, n_round)).sum(-1, keepdim=True)).squeeze(-1),
                                   "sum": gam(n_sum) * E.squeeze(-1),
                                   "underflow": torch.full_like(E.squeeze(-1), FLOOR * x.shape[-1])}
    return res


def _dual_factors(a, rstat, cstat):
    """r, c (B, L, M) from the statistics as given, and the |argument| of each."""
    a = a.double()
    rm, rs = rstat.double()[..., 0].unsqueeze(2), rstat.double()[..., 1].unsqueeze(2)
    cm, cs = cstat.double()[..., 0].unsqueeze(1), cstat.double()[..., 1].unsqueeze(1)
    return torch.exp(a - rm) / rs, torch.exp(a - cm) / cs, (a - rm).abs(), (a - cm).abs()


def dual_f_ref(a, rstat, cstat):
    """f = (exp(a - rmax) / rsum) (exp(a - cmax) / csum) from the statistics the kernel RETURNED.  Terms:
        expf      f (|a - rmax| + |a - cmax| + 4) u     ops  3 u f  (two divisions, the product)
        underflow 3 x 2^-126   (either exponential or the product flushed; rsum, csum >= 1)"""
    r, c, ar, ac = _dual_factors(a, rstat, cstat)
    f = r * c
    return f, {"expf": f * (ar + ac + 4) * U, "ops": 3 * U * f, "underflow": torch.full_like(f, 3 * FLOOR)}


def dual_bwd_ref(a, rstat, cstat, f, df):
    """da = 2 r c df - r Srow - c Scol with r, c recomputed from the statistics as given and Srow_i = sum_j f df,
    Scol_j = sum_i f df over the f as GIVEN (csrc/ufc_match.hip states it so; r c is f up to f's own rounding).  Terms:
        expf      the three products' exponentials: |2 r c df| (ar + ac + 4) u + |r Srow| (ar + 2) u + |c Scol| (ac + 2) u
        sum       r gam(ceil(M/64) + 7) sum_j |f df| + c gam(ceil(L/64) + CR_GROUPS + 1) sum_i |f df|
        ops       gam(6) (|2 r c df| + |r Srow| + |c Scol|): divisions, products, the two subtractions - a difference of
                  near-equal terms wherever the softmaxes are peaked
        underflow 3 x 2^-126 (2 |df| + |Srow| + |Scol| + 1)"""
    r, c, ar, ac = _dual_factors(a, rstat, cstat)
    B, L, M = r.shape
    fd = f.double() * df.double()
    srow, scol = fd.sum(2, keepdim=True), fd.sum(1, keepdim=True)
    mrow, mcol = fd.abs().sum(2, keepdim=True), fd.abs().sum(1, keepdim=True)
    t1, t2, t3 = 2 * r * c * df.double(), r * srow, c * scol
    terms = {"expf": (t1.abs() * (ar + ac + 4) + t2.abs() * (ar + 2) + t3.abs() * (ac + 2)) * U,
             "sum": r * gam(cdiv(M, 64) + 7) * mrow + c * gam(cdiv(L, CR_GROUPS) + CR_GROUPS + 1) * mcol,
             "ops": gam(6) * (t1.abs() + t2.abs() + t3.abs()),
             "underflow": 3 * FLOOR * (2 * df.double().abs() + srow.abs() + scol.abs() + 1)}
    return t1 - t2 - t3, terms


def make_dual_inputs(case):
    B, L, M, gain = case
    gen = _gen("dual", B, L, M, gain)
    return {"a": (gain * torch.randn(B, L, M, generator=gen)).contiguous(), "df": torch.randn(B, L, M, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# K10: cross attention
# ------------------------------------------------------------------------------------------------------------------
def _cross_counts(S, T):
    """rows forward: one wave per row, the exponentials summed over ceil(T / 64) trips and 6 steps, the values over ceil(T / 2)
    trips per half wave and one step, a product and the division.  cols forward: online over XC_GROUPS groups.  Backward
    statistics: rows as the forward's sum; columns online over 8 groups."""
    kf, kb = cdiv(S, XC_GROUPS), cdiv(S, 8)
    return {"rows": dict(n_round=2, n_sum=cdiv(T, 2) + 4), "cols": dict(n_round=2 + 3 * (kf + 1), n_sum=kf + XC_GROUPS + 4),
            "rows_bwd": dict(n_round=2, n_sum=cdiv(T, 64) + 6), "cols_bwd": dict(n_round=2 + 3 * (kb + 1), n_sum=kb + 8 + 1)}


def cross_fwd_ref(corr, src_v, trg_v):
    """corr (B, H, S, T), src_v (B, S, H, 32), trg_v (B, T, H, 32) -> src_attn (B, S, H, 32), trg_attn (B, T, H, 32), terms."""
    c = corr.double()
    B, H, S, T = c.shape
    n = _cross_counts(S, T)
    sv, tv = src_v.double().permute(0, 2, 1, 3), trg_v.double().permute(0, 2, 1, 3)          # (B, H, S|T, C)
    res = {}
    for name, a, v, cnt in (("src_attn", c, tv, n["rows"]), ("trg_attn", c.transpose(2, 3), sv, n["cols"])):
        arg = a - a.max(-1, keepdim=True).values
        want, terms = expect_ref(arg, v.unsqueeze(2).expand(B, H, a.shape[2], a.shape[3], v.shape[-1]), 1, cnt["n_round"], cnt["n_sum"])
        res[name] = want.permute(0, 2, 1, 3).contiguous()
        res[name + "_terms"] = {k: t.permute(0, 2, 1, 3).contiguous() for k, t in terms.items()}
    return res


def cross_bwd_ref(corr, src_v, trg_v, src_attn, trg_attn, g_src, g_trg):
    """With P1 = softmax_t(c), P2 = softmax_s(c) and src_attn / trg_attn as GIVEN:
        dtv[t] = sum_s P1 g1[s],  dsv[s] = sum_t P2 g2[t],
        dc[s,t] = P1 (g1[s].tv[t] - g1[s].sa[s]) + P2 (sv[s].g2[t] - g2[t].ta[t])
    -> dict dcorr (B,H,S,T), dsrc_v (B,S,H,32), dtrg_v (B,T,H,32) and their terms:
        weight   |term| weight_rel of the recomputed P1 / P2 (see _cross_counts)
        dots     P gam(32 + 2) (sum_k |g||v| + sum_k |g||attn|)  (32 products in a chain, the subtracted dot's 5 steps are
                 fewer; the difference) - the bracket cancels where the softmax is peaked (attn ~ v)
        sum      dc: u (|first| + |second|); dsv: gam(ceil(T/16) + 5) sum_t P2 |g2|; dtv: gam(ceil(S/16) + 17) sum_s P1 |g1|
        underflow a weight below the normal range (gain 12: most of them) is exact to 2^-126 only, and so is a product that lands
                 there: dc 2^-126 (|first bracket| + |second bracket| + 2); dsv 2^-126 (sum_t |g2| + 1); dtv alike.  (The first
                 run on an MI355X met it: a dcorr of 3.17e-41 one subnormal ulp, 1.2e-45, from float64.)"""
    c = corr.double()
    B, H, S, T = c.shape
    n = _cross_counts(S, T)
    pm = lambda x: x.double().permute(0, 2, 1, 3)
    sv, tv, sa, ta, g1, g2 = pm(src_v), pm(trg_v), pm(src_attn), pm(trg_attn), pm(g_src), pm(g_trg)
    a1 = c - c.max(3, keepdim=True).values
    P1 = softmax_parts(a1)[0]
    rel1 = weight_rel(a1, P1, 1, n["rows_bwd"]["n_round"], n["rows_bwd"]["n_sum"])
    a2 = (c - c.max(2, keepdim=True).values).transpose(2, 3)
    P2t = softmax_parts(a2)[0]
    rel2 = weight_rel(a2, P2t, 1, n["cols_bwd"]["n_round"], n["cols_bwd"]["n_sum"]).transpose(2, 3)
    P2 = P2t.transpose(2, 3)
    d1 = torch.einsum("bhsk,bhtk->bhst", g1, tv) - (g1 * sa).sum(-1, keepdim=True)
    m1 = torch.einsum("bhsk,bhtk->bhst", g1.abs(), tv.abs()) + (g1 * sa).abs().sum(-1, keepdim=True)
    d2 = torch.einsum("bhsk,bhtk->bhst", sv, g2) - (g2 * ta).sum(-1).unsqueeze(2)
    m2 = torch.einsum("bhsk,bhtk->bhst", sv.abs(), g2.abs()) + (g2 * ta).abs().sum(-1).unsqueeze(2)
    A, Bt = P1 * d1, P2 * d2
    res = {"dcorr": A + Bt,
           "dcorr_terms": {"weight": A.abs() * (rel1 + U) + Bt.abs() * (rel2 + U), "dots": gam(34) * (P1 * m1 + P2 * m2),
                           "sum": U * (A.abs() + Bt.abs()), "underflow": FLOOR * (d1.abs() + d2.abs() + 2)}}
    back = lambda x: x.permute(0, 2, 1, 3).contiguous()
    res["dsrc_v"] = back(torch.einsum("bhst,bhtk->bhsk", P2, g2))
    res["dsrc_v_terms"] = {"weight": back(torch.einsum("bhst,bhtk->bhsk", P2 * (rel2 + U), g2.abs())),
                           "sum": back(gam(cdiv(T, 16) + 5) * torch.einsum("bhst,bhtk->bhsk", P2, g2.abs())),
                           "underflow": back(FLOOR * (g2.abs().sum(2, keepdim=True) + 1).expand(B, H, S, g2.shape[-1]))}
    res["dtrg_v"] = back(torch.einsum("bhst,bhsk->bhtk", P1, g1))
    res["dtrg_v_terms"] = {"weight": back(torch.einsum("bhst,bhsk->bhtk", P1 * (rel1 + U), g1.abs())),
                           "sum": back(gam(cdiv(S, 16) + 17) * torch.einsum("bhst,bhsk->bhtk", P1, g1.abs())),
                           "underflow": back(FLOOR * (g1.abs().sum(2, keepdim=True) + 1).expand(B, H, T, g1.shape[-1]))}
    return res


def make_cross_inputs(case):
    B, H, S, T, gain = case
    gen = _gen("cross", B, H, S, T, gain)
    r = lambda *s: torch.randn(*s, generator=gen)
    return {"corr": (gain * r(B, H, S, T)).contiguous(), "src_v": r(B, S, H, 32), "trg_v": r(B, T, H, 32),
            "g_src": r(B, S, H, 32), "g_trg": r(B, T, H, 32)}


# ------------------------------------------------------------------------------------------------------------------
# K9: linear attention
# ------------------------------------------------------------------------------------------------------------------
def _phi(x):
    return torch.where(x > 0, x + 1, torch.exp(torch.clamp(x, max=0.0)))


def _la_views(q, k, v, cm):
    """float64 q, k (B, L, H, 32) and v as (B, L, H, Dv) whatever its layout."""
    v = v.double()
    return q.double(), k.double(), (v.permute(0, 3, 1, 2) if cm else v)


def _la_layout(x, cm):
    return x.permute(0, 2, 3, 1).contiguous() if cm else x.contiguous()


def _la_counts(L, Dv, nsplit):
    """Chains of the linear attention.  A split's partial adds lper = ceil(L / nsplit) terms in token order and the combine
    adds nsplit partials; phi costs 2 roundings (x + 1, or an expf of an exact argument), v / L two (1 / L is itself rounded).
        kv   = lper + nsplit + 5      one entry of KV (phi, v / L, the product)
        ks   = lper + nsplit + 2      one entry of Ksum
        den  = ks + 32 + 5            phi(q) . Ksum + eps and the reciprocal: every term is positive, so this is RELATIVE"""
    lper = cdiv(L, nsplit)
    kv, ks = lper + nsplit + 5, lper + nsplit + 2
    return dict(lper=lper, kv=kv, ks=ks, den=ks + 37)


def linear_fwd_ref(q, k, v, cm, nsplit):
    """out = L Z_l phi(q)_l . KV, KV = sum_s phi(k)_s (x) v_s / L, Z_l = 1 / (phi(q)_l . sum_s phi(k)_s + eps) -> (want in
    out's layout, terms):  kv  L Z gam(kv + 35) sum_d P_d sum_s N_sd |v_s| / L   (32 more additions, the products)
                           den |out| (gam(den) + 2 u)                            (the two products with Z and L)"""
    q, k, v = _la_views(q, k, v, cm)
    B, L, H, Dv = v.shape
    n = _la_counts(L, Dv, nsplit)
    P, N = _phi(q), _phi(k)
    KV = torch.einsum("bshd,bshv->bhdv", N, v) / L
    KVm = torch.einsum("bshd,bshv->bhdv", N, v.abs()) / L
    Z = 1 / (torch.einsum("blhd,bhd->blh", P, N.sum(1)) + EPS_LA)
    out = torch.einsum("blhd,bhdv,blh->blhv", P, KV, Z) * L
    mag = torch.einsum("blhd,bhdv,blh->blhv", P, KVm, Z) * L
    return _la_layout(out, cm), {"kv": _la_layout(gam(n["kv"] + 35) * mag, cm), "den": _la_layout((gam(n["den"]) + 2 * U) * out.abs(), cm)}


def linear_bwd_ref(q, k, v, dout, cm, nsplit):
    """The VJP as include/coponerf_hip.h / csrc/ufc_attn.hip state it, with P = phi(q), N = phi(k):
        T_l = dout_l . KV^T,  a_l = P_l . T_l,  dden_l = -L a_l Z_l^2,  dq_l = (L Z_l T_l + dden_l Ks) phi'(q_l)
        dKV = sum_l P_l (x) (L Z_l dout_l),  dKs = sum_l dden_l P_l
        dk_s = (v_s . dKV^T / L + dKs) phi'(k_s),   dv_s = N_s . dKV / L
    -> dict dq, dk (B, L, H, 32), dv (v's layout) and terms.  Every chain below is the count of the additions along the way
    plus one per product, on the sum of absolute values at that point (m* = the same formula on absolute values):
        nT = Dv + 1 + kv;  nA = nT + 35;  ndd = nA + 2 den + 5 (dden = -L a Z^2)
        dq:  "T" gam(nT + den + 8) L Z mT phi' + "dden" gam(ndd + ks + 6) mdd Ks phi'
        ndKV = lper + nsplit + den + 6;  ndKs = ndd + 3 + lper + nsplit
        dk:  "dKV" gam(Dv + ndKV + 6) sum_dv |v| mdKV / L phi' + "dKs" gam(ndKs + 4) mdKs phi'
        dv:  "dKV" gam(32 + ndKV + 4) sum_d N mdKV / L"""
    q, k, v = _la_views(q, k, v, cm)
    g = dout.double().permute(0, 3, 1, 2) if cm else dout.double()
    B, L, H, Dv = v.shape
    n = _la_counts(L, Dv, nsplit)
    P, N = _phi(q), _phi(k)
    dP, dN = torch.where(q > 0, torch.ones_like(P), P), torch.where(k > 0, torch.ones_like(N), N)
    KV = torch.einsum("bshd,bshv->bhdv", N, v) / L
    KVm = torch.einsum("bshd,bshv->bhdv", N, v.abs()) / L
    Ks = N.sum(1)                                                                   # (B, H, 32)
    Z = (1 / (torch.einsum("blhd,bhd->blh", P, Ks) + EPS_LA)).unsqueeze(-1)          # (B, L, H, 1)
    T_ = torch.einsum("blhv,bhdv->blhd", g, KV)
    mT = torch.einsum("blhv,bhdv->blhd", g.abs(), KVm)
    a = (P * T_).sum(-1, keepdim=True)
    ma = (P * mT).sum(-1, keepdim=True)
    dden, mdd = -L * a * Z * Z, L * ma * Z * Z
    nT = Dv + 1 + n["kv"]
    ndd = nT + 35 + 2 * n["den"] + 5
    dq = (L * Z * T_ + dden * Ks.unsqueeze(1)) * dP
    dq_terms = {"T": gam(nT + n["den"] + 8) * L * Z * mT * dP, "dden": gam(ndd + n["ks"] + 6) * mdd * Ks.unsqueeze(1) * dP}
    dKV = torch.einsum("blhd,blhv->bhdv", P * L * Z, g)
    mdKV = torch.einsum("blhd,blhv->bhdv", P * L * Z, g.abs())
    dKs = (dden * P).sum(1)
    mdKs = (mdd * P).sum(1)
    ndKV, ndKs = n["lper"] + nsplit + n["den"] + 6, ndd + 3 + n["lper"] + nsplit
    dk = (torch.einsum("bshv,bhdv->bshd", v, dKV) / L + dKs.unsqueeze(1)) * dN
    dk_terms = {"dKV": gam(Dv + ndKV + 6) * torch.einsum("bshv,bhdv->bshd", v.abs(), mdKV) / L * dN,
                "dKs": gam(ndKs + 4) * mdKs.unsqueeze(1) * dN}
    dv = torch.einsum("bshd,bhdv->bshv", N, dKV) / L
    dv_terms = {"dKV": _la_layout(gam(32 + ndKV + 4) * torch.einsum("bshd,bhdv->bshv", N, mdKV) / L, cm)}
    return {"dq": dq, "dq_terms": dq_terms, "dk": dk, "dk_terms": dk_terms, "dv": _la_layout(dv, cm), "dv_terms": dv_terms}


def make_linear_inputs(case):
    """q, k with both signs and a few exact zeros (phi' at 0), v and dout in the layout of channel_major."""
    B, L, H, Dv, cm, nsplit, gain = case
    gen = _gen("linear", B, L, H, Dv, cm, gain)
    q, k = gain * torch.randn(B, L, H, 32, generator=gen), gain * torch.randn(B, L, H, 32, generator=gen)
    for t in (q, k):
        t.view(-1)[torch.randperm(t.numel(), generator=gen)[:max(1, t.numel() // 50)]] = 0.0
    shape = (B, H, Dv, L) if cm else (B, L, H, Dv)
    return {"q": q, "k": k, "v": torch.randn(*shape, generator=gen), "dout": torch.randn(*shape, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# GroupNorm (1 group) + ReLU
# ------------------------------------------------------------------------------------------------------------------
def gn_moments(y, eps=EPS_GN):
    """y (B, C, npos) -> (stats (B, 2) float64 = sum, sum of squares: what the test hands the kernels; mean, rstd (B, 1, 1)
    float64 from the two-pass variance)."""
    y = y.double()
    stats = torch.stack((y.sum((1, 2)), (y * y).sum((1, 2))), 1)
    mean = y.mean((1, 2), keepdim=True)
    var = ((y - mean) ** 2).mean((1, 2), keepdim=True)
    return stats, mean, 1 / torch.sqrt(var + eps)


def _gn_yhat(y, mean, rstd):
    """yh = (y - mean) rstd and its fp32 error: the casts of mean and rstd (u |mean| rstd + u |yh|), the difference and the
    product (u |y - mean| rstd + u |yh|)."""
    d = y.double() - mean
    yh = d * rstd
    return yh, {"cast": U * (mean.abs() * rstd + yh.abs()), "ops": U * (d.abs() * rstd + yh.abs())}


def gn_fwd_ref(y, gn_w, gn_b):
    """out = relu((y - mean) rstd w + b); |relu(a) - relu(b)| <= |a - b|, so the bound of the pre-activation holds.  Terms:
    cast / ops of yh times |w|; ops: + 2 u (|yh w| + |b|) (the product, the sum)."""
    stats, mean, rstd = gn_moments(y)
    yh, e = _gn_yhat(y, mean, rstd)
    w, b = gn_w.double().view(1, -1, 1), gn_b.double().view(1, -1, 1)
    v = yh * w + b
    return torch.relu(v), {"cast": e["cast"] * w.abs(), "ops": e["ops"] * w.abs() + 2 * U * ((yh * w).abs() + b.abs())}


def gn_bwd_ref(y, out, dout, gn_w):
    """dz = dout [out > 0] with `out` as GIVEN; n = C npos;  m1_b = sum dz w / n,  m2_b = sum dz w yh / n;
        dy = rstd (dz w - m1 - yh m2),  dgn_w_c = sum_{b,pos} dz yh,  dgn_b_c = sum dz
    The sums run in float64 over fp32 products (the 16-byte path first adds 4 of them in fp32): per term the error of yh, 6
    roundings at most, and the final cast.  Terms of dy:
        cast   rstd (|m2| yh_cast + sum |dz w| yh_cast / n |yh|) + u |dy|          (the rstd factor in front)
        ops    rstd (u |dz w| + dm1 + |yh| dm2 + |m2| yh_ops + gam(4) (|dz w| + |m1| + |yh m2|)) + u |dy|
               (gam(4): the casts of m1 / m2, the product yh m2, the two differences)
               dm1 = gam(5) sum |dz w| / n,  dm2 = (sum |dz w| yh_ops + gam(7) sum |dz w yh|) / n"""
    stats, mean, rstd = gn_moments(y)
    yh, e = _gn_yhat(y, mean, rstd)
    B, C, npos = y.shape
    n = C * npos
    w = gn_w.double().view(1, -1, 1)
    dz = torch.where(out > 0, dout, torch.zeros_like(dout)).double()
    s = lambda x: x.sum((1, 2), keepdim=True)
    dzw = dz * w
    m1, m2 = s(dzw) / n, s(dzw * yh) / n
    dy = rstd * (dzw - m1 - yh * m2)
    dm1 = gam(5) * s(dzw.abs()) / n
    dm2_ops = (s(dzw.abs() * e["ops"]) + gam(7) * s((dzw * yh).abs())) / n
    dm2_cast = s(dzw.abs() * e["cast"]) / n
    res = {"dy": dy,
           "dy_terms": {"cast": rstd * (m2.abs() * e["cast"] + yh.abs() * dm2_cast) + U * dy.abs(),
                        "ops": rstd * (U * dzw.abs() + dm1 + yh.abs() * dm2_ops + m2.abs() * e["ops"]
                                       + gam(4) * (dzw.abs() + m1.abs() + (yh * m2).abs())) + U * dy.abs()}}
    c = lambda x: x.sum((0, 2))
    res["dgn_w"] = c(dz * yh)
    res["dgn_w_terms"] = {"cast": c(dz.abs() * e["cast"]), "ops": c(dz.abs() * e["ops"]) + gam(7) * c((dz * yh).abs())}
    res["dgn_b"] = c(dz)
    res["dgn_b_terms"] = {"ops": gam(5) * c(dz.abs())}
    return res


def make_gn_inputs(case):
    B, C, npos, offset = case
    gen = _gen("gn", B, C, npos, offset)
    y = torch.randn(B, C, npos, generator=gen) * 1.5 + offset * 1.5
    w = torch.randn(C, generator=gen)
    if C > 1:
        w[0], w[1] = -abs(w[0]) - 0.1, abs(w[1]) + 0.1                               # both signs whatever the draw
    return {"y": y, "gn_w": w, "gn_b": torch.randn(C, generator=gen) * 0.5, "dout": torch.randn(B, C, npos, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# Conv4d data gradient (k3 s1 p1)
# ------------------------------------------------------------------------------------------------------------------
def conv4d_dgrad_ref(dy, wq, ws):
    """dy (B, Cout, Hq, Wq, Hs, Ws), wq / ws (Cout, Cin, 3, 3) -> (dx (B, Cin, ...), terms): the transpose of the layer's two
    separable branches - y = conv2d over (Hq, Wq) with wq + conv2d over (Hs, Ws) with ws, both padded by 1 - in float64.
    An output is 2 x 9 x Cout products in one chain: gam(18 Cout) on sum |w| |dy|."""
    def both(dy, wq, ws):
        B, Co, Hq, Wq, Hs, Ws = dy.shape
        Ci = wq.shape[1]
        a = F.conv_transpose2d(dy.permute(0, 4, 5, 1, 2, 3).reshape(B * Hs * Ws, Co, Hq, Wq), wq, padding=1)
        a = a.reshape(B, Hs, Ws, Ci, Hq, Wq).permute(0, 3, 4, 5, 1, 2)
        b = F.conv_transpose2d(dy.permute(0, 2, 3, 1, 4, 5).reshape(B * Hq * Wq, Co, Hs, Ws), ws, padding=1)
        b = b.reshape(B, Hq, Wq, Ci, Hs, Ws).permute(0, 3, 1, 2, 4, 5)
        return a + b
    dy, wq, ws = dy.double(), wq.double(), ws.double()
    return both(dy, wq, ws), {"chain": gam(18 * dy.shape[1]) * both(dy.abs(), wq.abs(), ws.abs())}


def make_dgrad_inputs(case):
    B, Co, Ci, Hq, Wq, Hs, Ws = case
    gen = _gen("dgrad", *case)
    return {"dy": torch.randn(B, Co, Hq, Wq, Hs, Ws, generator=gen), "wq": torch.randn(Co, Ci, 3, 3, generator=gen) * 0.3,
            "ws": torch.randn(Co, Ci, 3, 3, generator=gen) * 0.3}


# ------------------------------------------------------------------------------------------------------------------
# row normalisation y = x / (|x| + eps) and its VJP
# ------------------------------------------------------------------------------------------------------------------
def _l2_chain(C):
    return cdiv(C, 64) + 6 + 1                  # per-lane additions, 6 wave steps, the product


def l2norm_fwd_ref(x, eps=EPS_NORM):
    """y = x / (|x| + eps): the norm's sum (all terms positive: relative gam(chain), halved by the root, which rounds once),
    the sum with eps, the division."""
    x = x.double()
    r = x.norm(dim=1, keepdim=True)
    y = x / (r + eps)
    return y, {"norm": (gam(_l2_chain(x.shape[1])) + 3 * U) * y.abs()}


def l2norm_bwd_ref(x, y, dy, eps=EPS_NORM):
    """dx = dy / (|x| + eps) - y (y . dy) / max(|x|, tiny) with y as GIVEN; a row of zeros gives dy / eps (y = 0 there), which is
    the derivative of x / (|x| + eps) at 0.  Terms (r = |x|, inv = 1 / (r + eps), k = (y . dy) / r):
        norm  |dy inv| (gam(chain) + 4 u) + |y k| (gam(chain) + 2 u)      (r enters inv and k; the root, the sum, 1 /, the product)
        dot   |y| gam(chain) sum |y dy| / r
        ops   2 u (|dy inv| + |y k|)                                       (the product y k, the difference)"""
    x, y, dy = x.double(), y.double(), dy.double()
    C = x.shape[1]
    r = x.norm(dim=1, keepdim=True)
    rs = torch.clamp(r, min=1e-30)
    inv = 1 / (r + eps)
    dot, mdot = (y * dy).sum(1, keepdim=True), (y * dy).abs().sum(1, keepdim=True)
    t1, t2 = dy * inv, y * dot / rs
    g = gam(_l2_chain(C))
    return t1 - t2, {"norm": t1.abs() * (g + 4 * U) + t2.abs() * (g + 2 * U), "dot": y.abs() * g * mdot / rs,
                     "ops": 2 * U * (t1.abs() + t2.abs())}


def make_l2_inputs(case):
    rows, C, kind = case
    gen = _gen("l2", rows, C, kind)
    x = torch.randn(rows, C, generator=gen)
    if kind == "tiny":
        x = x / x.norm(dim=1, keepdim=True) * 1e-4 * (0.5 + torch.rand(rows, 1, generator=gen))
    if kind == "zero":
        x[1] = 0.0
    return {"x": x.contiguous(), "dy": torch.randn(rows, C, generator=gen)}
