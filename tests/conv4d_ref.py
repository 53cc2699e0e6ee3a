"""Float64 references, with element-wise error bounds, of the 4-D convolution of get_z and the depthwise convolution of its
feed-forward blocks - cpn_conv4d (every forward arm and the GroupNorm statistics it publishes), cpn_conv4d_strided_bwd,
cpn_conv_wgrad_planes, cpn_dwconv3x3_wgrad, cpn_dwconv3x3_tokens, cpn_dwconv3x3_tokens_wgrad (csrc/ufc_conv4d.hip,
csrc/ufc_strided_bwd.hip, csrc/ufc_wgrad.hip) - and the case lists, for tests/test_conv4d_ref.py (CPU) and
tests/test_gpu_conv4d_f64.py (GPU).  Helpers, not tests; the conventions are those of tests/ufc_bwd_ref.py, whose U, gam,
total, report, _gen, case_id, conv4d_dgrad_ref and gn_fwd_ref are imported, not copied.

Every reference takes the fp32 values the kernel reads, converted to float64, forms what include/coponerf_hip.h says the entry
computes and returns (want, terms): `terms` is a dict of named bound terms, first order in u = 2^-24, each gam(chain length)
times the float64 SUM OF ABSOLUTE VALUES of the element's products (never |want|).  A sum of n products costs every product
its own rounding and at most n - 1 additions WHATEVER the order of the additions (sequential, wave butterfly, MFMA k steps,
partial sums of workgroups), so gam(n) holds for every kernel that adds the same n products; the chain lengths below are n.

Every arm of cpn_conv4d and every strided-backward case has a case with four different extents (Hq, Wq, Hs, Ws): a kernel
that swapped the strides of two of them would read other elements and leave the bound.  (The MFMA arm needs Ws a power of two
and whole waves of positions; some of its shapes, and the 160 000-position one, repeat an extent and have a neighbour that
does not.)"""
import math

import torch
import torch.nn.functional as F

from tests.ufc_bwd_ref import U, gam, total, report, _gen, case_id, conv4d_dgrad_ref, gn_fwd_ref, cdiv, ratio  # noqa: F401

U64 = 2.0 ** -53
INF = float("inf")


def gam64(n):
    return n * U64 / (1.0 - n * U64)


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
# Forward: (arm, (B, Cin, Cout, Hq, Wq, Hs, Ws, k, s, p), wmul, variant).  `arm` is the kernel cpn_conv4d's dispatch must reach
# with the case as given (a strided case WITH scratch), W = cdiv(npos', 256) * wmul the workgroups per sample that arm
# launches (gn_publish counts gridDim.x * gridDim.y).  A strided case also runs with scratch = NULL, where it takes the generic
# kernel: cdiv * Cout workgroups.  variant: "" or which pointer starts 4 bytes into its buffer.
FWD_CASES = [
    ("generic", (2, 3, 5, 5, 6, 4, 7, 3, 1, 1), 5, ""),
    ("generic", (1, 2, 5, 5, 6, 4, 7, 5, 1, 2), 5, ""),
    ("pooled_c8", (2, 1, 8, 7, 9, 5, 10, 3, 2, 1), 1, ""),           # two workgroups per sample; NULL scratch: generic, 16
    ("pooled", (2, 2, 5, 9, 10, 6, 13, 5, 4, 2), 5, ""),
    ("pooled_c8", (2, 1, 8, 5, 6, 7, 8, 3, 2, 1), 1, ""),
    ("pooled_c8", (1, 2, 8, 9, 10, 6, 13, 5, 4, 2), 1, ""),
    ("pooled_c8", (1, 8, 8, 3, 6, 5, 8, 3, 2, 1), 1, ""),            # Hq = 3, not 4: a ragged window in either pair
    ("valu<4,true>", (2, 3, 8, 5, 6, 4, 7, 3, 1, 1), 2, ""),
    ("valu<8,true>", (1, 8, 32, 4, 5, 8, 6, 3, 1, 1), 4, ""),        # Ws = 6 keeps it off the MFMA arm
    ("valu<8,false>", (1, 1, 8, 16, 20, 25, 20, 3, 1, 1), 1, ""),    # B npos = 160 000 > 131 072
    ("valu<8,false>", (1, 1, 8, 16, 20, 25, 21, 3, 1, 1), 1, ""),    # 168 000 positions, no multiple of 256
    ("mfma1", (2, 4, 8, 2, 8, 4, 4, 3, 1, 1), 1, ""),
    ("mfma1", (1, 8, 12, 4, 2, 8, 8, 3, 1, 1), 1, ""),
    ("mfma1", (1, 4, 16, 2, 2, 4, 16, 3, 1, 1), 1, ""),
    ("mfma1", (1, 4, 8, 3, 2, 4, 8, 3, 1, 1), 1, ""),                # 192 positions: the fourth wave of the workgroup is idle
    ("mfma2", (1, 12, 20, 4, 2, 8, 8, 3, 1, 1), 1, ""),
    ("mfma2", (2, 8, 32, 2, 4, 2, 32, 3, 1, 1), 1, ""),
    ("mfma2", (1, 8, 20, 2, 3, 8, 4, 3, 1, 1), 1, ""),               # 192 positions, four different extents
    ("unaligned", (2, 4, 8, 2, 8, 4, 4, 3, 1, 1), 2, "x+4"),          # the first MFMA case off the MFMA arm: valu<4,true>
    ("unaligned", (2, 4, 8, 2, 8, 4, 4, 3, 1, 1), 2, "y+4"),
]
# one case per arm family for cpn_conv4d_gn_relu
GN_RELU_CASES = [next(fc for fc in FWD_CASES if fc[0] == arm) for arm in ("generic", "pooled_c8", "valu<4,true>", "mfma1")]
# Strided backward (entry limits: Cout = 8, Cin in {1, 2, 8}): (case, variant); "ties": x = round(2 relu(x)) / 2
SBWD_SHAPES = [(2, 1, 8, 5, 6, 7, 8, 3, 2, 1), (1, 2, 8, 9, 10, 6, 13, 5, 4, 2), (1, 8, 8, 3, 6, 5, 8, 3, 2, 1)]
SBWD_CASES = [(c, "") for c in SBWD_SHAPES] + [(SBWD_SHAPES[0], "ties")]
SBWD_TIES = (SBWD_SHAPES[0], "ties")
# cpn_conv_wgrad_planes (B, Cin, Cout, G, H, W, db given): every instantiation - <8,8>, <8,32>, <32,32>, <8,32,swap>
PLANES_CASES = [(1, 1, 1, 1, 1, 4, 1), (2, 7, 20, 3, 6, 10, 1), (1, 32, 32, 5, 64, 4, 1), (2, 8, 32, 9, 8, 32, 0),
                (2, 32, 8, 75, 16, 16, 1)]
# cpn_dwconv3x3_wgrad (N, C, H, W)
DW_WGRAD_CASES = [(1, 1, 1, 1), (2, 5, 3, 7), (3, 40, 16, 16)]
# cpn_dwconv3x3_tokens (B, H, W, C), each with flip 0, 1, 2; its weight gradient on the same shapes and one with C % 4 != 0
DW_TOKENS_CASES = [(1, 1, 1, 4), (2, 3, 5, 44), (3, 16, 16, 256)]
DW_FLIPS = [0, 1, 2]
DW_TOKENS_WGRAD_CASES = DW_TOKENS_CASES + [(2, 3, 5, 6)]


def fwd_id(c):
    return f"{c[0]}-{case_id(c[1])}" + (f"-{c[3]}" if c[3] else "")


def sbwd_id(c):
    return case_id(c[0]) + (f"-{c[1]}" if c[1] else "")


def out_dims(case):
    """(Oq, Pq, Os, Ps) of a Conv4d case: n' = (n + 2p - k) / s + 1, which make_geo requires to equal ceil(n / s)."""
    B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p = case
    o = tuple((n + 2 * p - k) // s + 1 for n in (Hq, Wq, Hs, Ws))
    assert o == tuple(cdiv(n, s) for n in (Hq, Wq, Hs, Ws)), case
    return o


def npos_of(case):
    return math.prod(out_dims(case))


def launched_w(fc, scratch=True):
    """Workgroups per sample of a forward case; scratch = False: a strided case handed scratch = NULL (the generic kernel)."""
    arm, case, wmul, _ = fc
    if case[8] > 1 and not scratch:
        wmul = case[2]
    return cdiv(npos_of(case), 256) * wmul


def make_conv4d_inputs(case, variant=""):
    """x, wq, bq, ws, bs, the GroupNorm affine, a residual and dy of a Conv4d case, fp32."""
    B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p = case
    gen = _gen("conv4d", *case)
    r = lambda *sh: torch.randn(*sh, generator=gen)
    x = r(B, Ci, Hq, Wq, Hs, Ws)
    if variant == "ties":
        x = torch.round(2 * torch.relu(x)) / 2                       # half of every window 0, the rest few distinct values
    o = out_dims(case)
    gw = r(Co)
    gw[0], gw[1] = -abs(gw[0]) - 0.1, abs(gw[1]) + 0.1
    return {"x": x.contiguous(), "wq": r(Co, Ci, k, k) * 0.3, "bq": r(Co) * 0.5, "ws": r(Co, Ci, k, k) * 0.3, "bs": r(Co) * 0.5,
            "gn_w": gw, "gn_b": r(Co) * 0.5, "res": r(B, Co, *o), "dy": r(B, Co, *o)}


# ------------------------------------------------------------------------------------------------------------------
# max-pool, kernel = stride = s, ceil mode, over the last two dims: values and the routing of the backward
# ------------------------------------------------------------------------------------------------------------------
def _windows(x, s, trunc=False):
    """(..., H, W) -> (..., O, P, s s): every window's elements in scan order (dy major), -inf where a ragged window of the
    ceil mode reaches past the input.  trunc (a seeded defect): a ragged window ends one element early."""
    H, W = x.shape[-2:]
    O, P = cdiv(H, s), cdiv(W, s)
    if trunc:
        x = x.clone()
        if H % s:
            x[..., H - 1, :] = -INF
        if W % s:
            x[..., :, W - 1] = -INF
    xp = F.pad(x, (0, P * s - W, 0, O * s - H), value=-INF)
    return xp.reshape(*x.shape[:-2], O, s, P, s).transpose(-3, -2).reshape(*x.shape[:-2], O, P, s * s)


def _unwindow(wv, H, W, s):
    """The inverse layout change of _windows: (..., O, P, s s) -> (..., H, W)."""
    O, P = wv.shape[-3:-1]
    return wv.reshape(*wv.shape[:-3], O, P, s, s).transpose(-3, -2).reshape(*wv.shape[:-3], O * s, P * s)[..., :H, :W]


def pool_last2(x, s, trunc=False, last=False):
    """-> (pooled (..., O, P), routed (..., H, W) bool): the maximum of every window and, written out, the element the backward
    routes to - the FIRST maximum of the window in scan order (last = True, a seeded defect: the last one)."""
    H, W = x.shape[-2:]
    win = _windows(x, s, trunc)
    m = win.max(-1).values
    eq = win == m.unsqueeze(-1)
    if last:
        first = eq & (eq.flip(-1).cumsum(-1).flip(-1) == 1)
    else:
        first = eq & (eq.cumsum(-1) == 1)
    return m, _unwindow(first, H, W, s)


def _swap_pairs(x):
    return x.permute(0, 1, 4, 5, 2, 3)


def pooled_pair(x, s, **kw):
    """x (B, C, Hq, Wq, Hs, Ws) float64 -> Ps (support dims pooled: the query branch's input), Pq (query dims pooled) and the
    two routing masks, both in x's layout."""
    if s == 1:
        one = torch.ones_like(x, dtype=torch.bool)
        return x, x, one, one
    ps, rs = pool_last2(x, s, **kw)
    pq, rq = pool_last2(_swap_pairs(x), s, **kw)
    return ps, _swap_pairs(pq), rs, _swap_pairs(rq)


# ------------------------------------------------------------------------------------------------------------------
# the two separable branches, tap by tap
# ------------------------------------------------------------------------------------------------------------------
def _branch(v, w, k, s, p, O, P, drop=None):
    """sum_{c,i,j} w[o,c,i,j] v[b,c, a s + i - p, b s + j - p, ...] over dims 2, 3 of v (B, C, H, W, M, N) -> (B, Co, O, P, M, N),
    zero padding.  drop = (i, j): a seeded defect - that tap adds nothing to output channel 0 in the last output row."""
    B, C, H, W = v.shape[:4]
    vp = F.pad(v, (0, 0, 0, 0, p, max(0, (P - 1) * s + k - p - W), p, max(0, (O - 1) * s + k - p - H)))
    out = torch.zeros(B, w.shape[0], O, P, *v.shape[4:], dtype=v.dtype)
    for i in range(k):
        for j in range(k):
            t = torch.einsum("oc,bcqrst->boqrst", w[:, :, i, j], vp[:, :, i:i + (O - 1) * s + 1:s, j:j + (P - 1) * s + 1:s])
            if drop == (i, j):
                t[:, 0, O - 1] = 0.0
            out += t
    return out


def _branch_t(g, w, k, s, p, H, W):
    """The transpose of _branch: g (B, Co, O, P, M, N) -> (B, C, H, W, M, N)."""
    B, Co, O, P = g.shape[:4]
    Hp, Wp = max(H + p, (O - 1) * s + k) + p, max(W + p, (P - 1) * s + k) + p
    out = torch.zeros(B, w.shape[1], Hp, Wp, *g.shape[4:], dtype=g.dtype)
    for i in range(k):
        for j in range(k):
            out[:, :, i:i + (O - 1) * s + 1:s, j:j + (P - 1) * s + 1:s] += torch.einsum("oc,boqrst->bcqrst", w[:, :, i, j], g)
    return out[:, :, p:p + H, p:p + W]


def _conv_both(ps, pq, wq, bq, ws, bs, k, s, p, o, drop=None):
    yq = _branch(ps, wq, k, s, p, o[0], o[1], drop)
    ys = _swap_pairs(_branch(_swap_pairs(pq), ws, k, s, p, o[2], o[3]))
    return yq + ys + (bq + bs).view(1, -1, 1, 1, 1, 1)


def conv4d_fwd_ref(x, wq, bq, ws, bs, k, s, p, drop=None, trunc=False, swap_q=False):
    """y[b,o,qy,qx,sy,sx] = bq[o] + bs[o] + sum_{c,i,j} wq[o,c,i,j] Ps[b,c,qy s+i-p,qx s+j-p,sy,sx]
                                          + sum_{c,i,j} ws[o,c,i,j] Pq[b,c,qy,qx,sy s+i-p,sx s+j-p]
    (the comment above conv4d_kernel in csrc/ufc_conv4d.hip), Ps / Pq = x max-pooled over the support / query pair (kernel =
    stride = s, ceil mode) when s > 1 -> (y, terms).  The max-pool is exact in fp32: pool first, then take absolute values.
    Chain: every arm starts an accumulator with fl(bq + bs) and adds the 2 k k Cin products to it (the generic, pooled and VALU
    kernels one fused or unfused multiply-add per tap, the MFMA kernel four input channels of a tap per v_mfma_f32_16x16x4_f32
    step): n = 2 k k Cin + 2, on |bq| + |bs| + sum |w| |P|.
    drop, trunc, swap_q: seeded defects (see _branch, _windows; swap_q reads x with the extents of Hq and Wq exchanged)."""
    x, wq, bq, ws, bs = (t.double() for t in (x, wq, bq, ws, bs))
    B, Ci, Hq, Wq, Hs, Ws = x.shape
    if swap_q:
        x = x.reshape(B, Ci, Wq, Hq, Hs, Ws).transpose(2, 3)
    o = tuple((n + 2 * p - k) // s + 1 for n in (Hq, Wq, Hs, Ws))
    ps, pq, _, _ = pooled_pair(x, s, trunc=trunc)
    y = _conv_both(ps, pq, wq, bq, ws, bs, k, s, p, o, drop)
    mag = _conv_both(ps.abs(), pq.abs(), wq.abs(), bq.abs(), ws.abs(), bs.abs(), k, s, p, o)
    return y, {"chain": gam(2 * k * k * Ci + 2) * mag}


def gn_stats_ref(y):
    """y (B, C, ...) the kernel's OWN fp32 output -> (want (B, 2) = float64 sum and sum of squares per sample, terms).  The
    kernels widen every element to double, square it there (exact: 48 bits) and add in double from the thread to the last
    workgroup: gam64(C npos) with u64 = 2^-53 on sum |y| and sum y^2."""
    y = y.double().flatten(1)
    n = y.shape[1]
    want = torch.stack((y.sum(1), (y * y).sum(1)), 1)
    return want, {"chain": gam64(n) * torch.stack((y.abs().sum(1), (y * y).sum(1)), 1)}


def stats_replay(stats, B, W):
    """The documented fixed order of gn_publish, replayed on the published partial pairs stats[3B + 2(bW + w) ..]: thread t
    of 256 adds the pairs w = t, t + 256, ... in ascending order starting from 0.0, then the halving LDS tree (n = 128 .. 1:
    tree[t] += tree[t + n]) -> (B, 2) float64, which must equal stats[2b], stats[2b + 1] bit for bit."""
    part = stats[3 * B:3 * B + 2 * B * W].reshape(B, W, 2)
    rows = cdiv(W, 256)
    part = torch.cat((part, torch.zeros(B, rows * 256 - W, 2, dtype=torch.float64)), 1).reshape(B, rows, 256, 2)
    acc = torch.zeros(B, 256, 2, dtype=torch.float64)
    for r in range(rows):
        acc = acc + part[:, r]
    n = 128
    while n > 0:
        acc = acc[:, :n] + acc[:, n:2 * n]
        n //= 2
    return acc[:, 0]


def written_partials(stats, B):
    """Partial slots per sample whose sum of squares is non-zero: the W of the launch (a workgroup has at least one live
    position, and a slot no workgroup wrote is still the zero the header requires on entry)."""
    n = int((stats[3 * B + 1::2] != 0).sum())
    assert n % B == 0, (n, B)
    return n // B


def emu_stats(y, B, W, nslots):
    """A stats buffer as a launch of W workgroups per sample leaves it, from y (B, C, npos) fp32: workgroup me = x + cdiv(npos, 256)
    g holds positions 256 x .. of channel group g (W / cdiv groups).  CPU stand-in for the tests of stats_replay."""
    B_, C, npos = y.shape
    nx = cdiv(npos, 256)
    G = W // nx
    yd = F.pad(y.double(), (0, nx * 256 - npos)).reshape(B, G, C // G, nx, 256)
    s1, s2 = yd.sum((2, 4)), (yd * yd).sum((2, 4))                              # (B, G, nx): me = x + nx g
    stats = torch.zeros(nslots, dtype=torch.float64)
    stats[3 * B:3 * B + 2 * B * W] = torch.stack((s1, s2), -1).reshape(-1)
    stats[2 * B:3 * B] = torch.full((B,), W, dtype=torch.int64).view(torch.float64)
    stats[:2 * B] = stats_replay(stats, B, W).reshape(-1)
    return stats


# ------------------------------------------------------------------------------------------------------------------
# VJP of the strided layer
# ------------------------------------------------------------------------------------------------------------------
def strided_bwd_ref(x, dy, wq, ws, k, s, p, trunc=False, last=False):
    """dict dx, gwq, gws, gb, their terms and `routed` (the elements of x that are the routed maximum of either window).
        gPs = transposed strided convolution of dy with wq, gPq with ws (_branch_t)
        dx  = [(U, V) is the FIRST maximum of its support window in scan order] gPs
            + [(Y, X) is the FIRST maximum of its query window] gPq                  ragged ceil-mode windows, see pool_last2
        gwq[o,c,i,j] = sum_{b,pos} dy[b,o,pos] Ps[b,c,qy s+i-p,qx s+j-p,sy,sx],  gws alike with Pq;  gb[o] = sum_{b,pos} dy
    Chains: dx - an input element belongs to ONE window per branch, whose gradient is at most Cout k k products, and the two
    are added: Cout k k + 1.  gwq / gws: B Oq Pq Os Ps products.  gb: B npos additions."""
    x, dy, wq, ws = (t.double() for t in (x, dy, wq, ws))
    B, Ci, Hq, Wq, Hs, Ws = x.shape
    Co = wq.shape[0]
    o = dy.shape[2:]
    ps, pq, rs, rq = pooled_pair(x, s, trunc=trunc, last=last)

    def grads(dy, wq, ws):
        gps = _branch_t(dy, wq, k, s, p, Hq, Wq)                                    # (B, Ci, Hq, Wq, Os, Ps)
        gpq = _swap_pairs(_branch_t(_swap_pairs(dy), ws, k, s, p, Hs, Ws))          # (B, Ci, Oq, Pq, Hs, Ws)
        up = lambda g: g.repeat_interleave(s, -2).repeat_interleave(s, -1)
        a = up(gps)[..., :Hs, :Ws] * rs
        b = _swap_pairs(up(_swap_pairs(gpq))[..., :Hq, :Wq]) * rq
        return a + b

    def wgrad(dy, v, O, P):
        """sum_{b, pos} dy[b,o,...] v[b,c, a s+i-p, b s+j-p, ...] -> (Co, Ci, k, k); the convolved pair is dims 2, 3 of v and dy"""
        H, W = v.shape[2:4]
        vp = F.pad(v, (0, 0, 0, 0, p, max(0, (P - 1) * s + k - p - W), p, max(0, (O - 1) * s + k - p - H)))
        g = torch.zeros(Co, Ci, k, k, dtype=torch.float64)
        for i in range(k):
            for j in range(k):
                g[:, :, i, j] = torch.einsum("boqrst,bcqrst->oc", dy, vp[:, :, i:i + (O - 1) * s + 1:s, j:j + (P - 1) * s + 1:s])
        return g

    n = B * math.prod(o)
    res = {"routed": rs | rq, "dx": grads(dy, wq, ws),
           "dx_terms": {"chain": gam(Co * k * k + 1) * grads(dy.abs(), wq.abs(), ws.abs())},
           "gwq": wgrad(dy, ps, o[0], o[1]), "gwq_terms": {"chain": gam(n) * wgrad(dy.abs(), ps.abs(), o[0], o[1])},
           "gws": wgrad(_swap_pairs(dy), _swap_pairs(pq), o[2], o[3]),
           "gws_terms": {"chain": gam(n) * wgrad(_swap_pairs(dy).abs(), _swap_pairs(pq).abs(), o[2], o[3])},
           "gb": dy.sum((0, 2, 3, 4, 5)), "gb_terms": {"chain": gam(n) * dy.abs().sum((0, 2, 3, 4, 5))}}
    return res


# ------------------------------------------------------------------------------------------------------------------
# weight gradients of the stride-1 branch and of the depthwise 3x3
# ------------------------------------------------------------------------------------------------------------------
def _shift9(x):
    """(..., H, W) -> (9, ..., H, W): x[y + i - 1, x + j - 1] with zero padding, tap = 3 i + j."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([xp[..., i:i + H, j:j + W] for i in range(3) for j in range(3)])


def wgrad_planes_ref(x, dy):
    """x (B, Cin, G, H, W), dy (B, Cout, G, H, W) -> dict dw (Cout, Cin, 3, 3) = sum_{b,g,y,x} dy[b,o,g,y,x] x[b,c,g,y+i-1,x+j-1],
    db (Cout) = sum dy, and terms.  Chain: B G H W products (db: additions) - the MFMA walks a plane four positions a step,
    a workgroup its planes in turn, and the workgroups' partial sums meet in the fixed order of partial_sum.h."""
    x, dy = x.double(), dy.double()
    n = x.shape[0] * x.shape[2] * x.shape[3] * x.shape[4]
    f = lambda x, dy: torch.einsum("bogyx,tbcgyx->oct", dy, _shift9(x)).reshape(dy.shape[1], x.shape[1], 3, 3)
    return {"dw": f(x, dy), "dw_terms": {"chain": gam(n) * f(x.abs(), dy.abs())},
            "db": dy.sum((0, 2, 3, 4)), "db_terms": {"chain": gam(n) * dy.abs().sum((0, 2, 3, 4))}}


def dwconv_wgrad_ref(x, dy):
    """x, dy (N, C, H, W) -> dw (C, 3, 3) = sum_{n,y,x} dy[n,c,y,x] x[n,c,y+i-1,x+j-1], db (C) = sum dy, terms.  Chain: N H W."""
    x, dy = x.double(), dy.double()
    n = x.shape[0] * x.shape[2] * x.shape[3]
    f = lambda x, dy: torch.einsum("ncyx,tncyx->ct", dy, _shift9(x)).reshape(-1, 3, 3)
    return {"dw": f(x, dy), "dw_terms": {"chain": gam(n) * f(x.abs(), dy.abs())},
            "db": dy.sum((0, 2, 3)), "db_terms": {"chain": gam(n) * dy.abs().sum((0, 2, 3))}}


ERF_ULPS = 4          # ASSUMED: no document of the ROCm installation states the device library's error of erff


def dwconv_tokens_ref(x, w, bias, H, W, flip):
    """x (B, H W, C) tokens, w (C, 9), bias (C) or None -> (y (B, H W, C), terms).
        flip & 1 == 0:  a = bias + sum_ij w[c][3i+j] x[p + (i-1, j-1)]         (forward)
        flip & 1 == 1:  a =        sum_ij w[c][8 - (3i+j)] x[p + (i-1, j-1)]   (data gradient: the flipped taps)
        flip & 2:       y = 0.5 a (1 + erf(a / sqrt 2)), the exact GELU; else y = a
    conv: gam(10) (|bias| + sum |w| |x|) - the accumulator starts as the bias and takes nine products.  With the GELU that
    error of a moves y by |g'(a)| = |Phi(a) + a phi(a)| times it, and the kernel's 0.5f a (1.0f + erff(a 0.70710678f)) adds
        erf  |a| / 2 (ERF_ULPS ulp of erf's value, <= 2 ERF_ULPS u |erf(t)|;  + 2 u |t| erf'(t): the constant and the product
             round the argument t = a / sqrt 2)
        ops  u |a| / 2 |1 + erf(t)| + u |y|      (the sum and the last product; the halving is exact)
    ERF_ULPS = 4 is an ASSUMPTION (see above).  Observed: err/bound 0.239 of the GELU arm on an MI355X at its worst element
    (3 x 16 x 16 x 256; erf 79 % of the bound there, ops 13 %, conv 8 %) - the device's erff stays inside a quarter of the
    assumed term; the CPU library's fp32 GELU reaches 0.794 on the same case."""
    x, w = x.double(), w.double()
    B, L, C = x.shape
    wt = w.flip(1) if flip & 1 else w
    xs = _shift9(x.reshape(B, H, W, C).permute(0, 3, 1, 2))                          # (9, B, C, H, W)
    b = torch.zeros(C, dtype=torch.float64) if bias is None else bias.double()
    back = lambda t: t.permute(0, 2, 3, 1).reshape(B, L, C)
    a = back(torch.einsum("ct,tbcyx->bcyx", wt, xs) + b.view(1, C, 1, 1))
    conv = gam(10) * back(torch.einsum("ct,tbcyx->bcyx", wt.abs(), xs.abs()) + b.abs().view(1, C, 1, 1))
    if not flip & 2:
        return a, {"conv": conv}
    t = a / math.sqrt(2.0)
    e = torch.erf(t)
    phi = torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
    y = 0.5 * a * (1 + e)
    return y, {"conv": conv * (0.5 * (1 + e) + a * phi).abs(),
               "erf": 0.5 * a.abs() * (2 * ERF_ULPS * U * e.abs() + 2 * U * t.abs() * 2 / math.sqrt(math.pi) * torch.exp(-t * t)),
               "ops": U * 0.5 * a.abs() * (1 + e).abs() + U * y.abs()}


def dwconv_tokens_wgrad_ref(x, dy, H, W):
    """x, dy (B, H W, C) -> dw (C, 9) = sum_{b,p} dy[b,p,c] x[b, p + (i-1, j-1), c], db (C) = sum dy, terms.  Chain: B H W."""
    B, L, C = x.shape
    nchw = lambda t: t.double().reshape(B, H, W, C).permute(0, 3, 1, 2)
    r = dwconv_wgrad_ref(nchw(x), nchw(dy))
    r["dw"], r["dw_terms"] = r["dw"].reshape(C, 9), {"chain": r["dw_terms"]["chain"].reshape(C, 9)}
    return r


def make_planes_inputs(case):
    B, Ci, Co, G, H, W, _ = case
    gen = _gen("planes", *case)
    return {"x": torch.randn(B, Ci, G, H, W, generator=gen), "dy": torch.randn(B, Co, G, H, W, generator=gen)}


def make_dw_wgrad_inputs(case):
    N, C, H, W = case
    gen = _gen("dw_wgrad", *case)
    return {"x": torch.randn(N, C, H, W, generator=gen), "dy": torch.randn(N, C, H, W, generator=gen)}


def make_dw_tokens_inputs(case):
    B, H, W, C = case
    gen = _gen("dw_tokens", *case)
    r = lambda *s: torch.randn(*s, generator=gen)
    return {"x": r(B, H * W, C) * 1.5, "w": r(C, 9) * 0.5, "bias": r(C) * 0.5, "dy": r(B, H * W, C)}
