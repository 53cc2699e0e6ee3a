"""Float64 references, with element-wise error bounds, of the fp32 kernels get_z runs only at inference - the correlation
(row normalisation + GEMM), the bilinear resize and its adjoint, the fused final correlation, the q / k assembly, the
low-resolution cost-volume attention and the pose head (csrc/ufc_corr.hip, csrc/ufc_attn.hip, csrc/pose.hip) - and the case
lists, for tests/test_getz_fwd_ref.py (CPU) and tests/test_gpu_getz_f64.py (GPU).  Helpers, not tests; nothing of the package
is touched.

Every resize in these kernels makes DISCONTINUOUS decisions in fp32: the taps i0 = (int)(scale I), i1 = i0 + (i0 < h - 1) and
the fraction l = scale I - i0 of csrc/ac_taps.h.  axis_taps() restates exactly that in numpy float32; the references take the
taps and the fraction as given numbers and do everything continuous in float64.  Every bound is first order in u = 2^-24 and
comes from the kernel's operation count, as in tests/ufc_bwd_ref.py:

    gam(n) = n u / (1 - n u)   times the float64 SUM OF ABSOLUTE VALUES of the element's terms, n = the longest chain of
                               additions plus the element-wise roundings (one per multiply, divide, 1 - l, ...);
    a blend  a (1 - l) + b l   rounds 1 - l, two products and the sum: gam(3) on |a| (1 - l) + |b| l; a 2-D bilinear value is
                               two levels of it, gam(6); interpolate4d is two such passes, gam(12);
    a chain of additions       is charged at its LENGTH (per-lane partial sums, the steps of a wave reduction, partials added
                               in order), whatever its order;
    phi = elu + 1              costs 2 roundings (x + 1, or an expf of an exact argument to 1 ulp);
    a division                 enters with the conditioning of its denominator: all denominators here are sums of positive
                               terms (norm + eps, phi(q) . sum phi(k) + eps), so their relative error is their chain's gam.
Each reference returns its bound's terms separately (a dict name -> tensor); the bound is their sum.
"""
import math

import numpy as np
import torch

from tests.ufc_bwd_ref import EPS_LA, EPS_NORM, U, _gen, _phi, case_id, cdiv, gam, l2norm_fwd_ref, report, total  # noqa: F401

F64 = torch.float64

# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
# (B, L, C); the arm each one takes is stated by correlation_arm and asserted in the tests
CORR_CASES = [(1, 1, 16), (2, 37, 16), (1, 100, 48), (2, 256, 64), (86, 130, 16), (4, 1024, 32), (512, 128, 16), (128, 256, 48),
              (512, 128, 32)]
CORR_ARMS = {(1, 1, 16): "nt2", (2, 37, 16): "nt2", (1, 100, 48): "nt2", (2, 256, 64): "nt2", (86, 130, 16): "nt8",
             (4, 1024, 32): "nt8", (512, 128, 16): "tile64", (128, 256, 48): "tile64", (512, 128, 32): "tile64"}
CORR_ZERO_ROW = (2, 37, 16)                       # this case has an all-zero row in src (row 3 of batch 1) and in trg (row 0)
# (planes, h, w, H, W)
RESIZE_CASES = [(1, 1, 1, 1, 1), (3, 1, 1, 5, 4), (2, 4, 7, 1, 1), (2, 3, 5, 8, 6), (2, 16, 16, 16, 16), (3, 9, 7, 4, 3),
                (5, 16, 16, 64, 64)]
RESIZE_IDENTITY = (2, 16, 16, 16, 16)
# (B, h0, h1, n)
MEAN3_CASES = [(1, 2, 3, 4), (2, 3, 5, 7), (1, 5, 7, 7), (1, 43, 45, 46)]
MEAN3_ARMS = {(1, 2, 3, 4): "planes", (2, 3, 5, 7): "planes", (1, 5, 7, 7): "planes", (1, 43, 45, 46): "thread"}
MEAN3_BOTH = (65536, 2, 3, 4)                     # B >= 65536 takes the per-thread arm at a shape whose planes fit in LDS
# (B, fs, h, w, nhead, dim)
QK_CASES = [(1, 1, 1, 1, 1, 1), (2, 5, 3, 4, 2, 3), (1, 3, 7, 7, 1, 4), (1, 16, 16, 16, 8, 32), (2, 32, 16, 16, 8, 32)]
# (B, fs, H, hs, Dv)
CVA_CASES = [(1, 1, 1, 1, 1), (1, 4, 1, 1, 3), (1, 9, 2, 1, 5), (1, 9, 2, 2, 5), (2, 5, 3, 5, 7), (1, 7, 2, 3, 300),
             (1, 32, 8, 16, 256)]
CVA_ONE_POINT = [(1, 4, 1, 1, 3), (1, 9, 2, 1, 5)]            # hs == 1, fs >= 4: the gather window must span the whole axis
# (B, V, n)
POSPOS_CASES = [(1, 1, 1), (2, 2, 5), (3, 2, 64)]
# (B, K, O, nsplit)
GEMV_CASES = [(1, 4, 1, 1), (2, 1028, 5, 8), (3, 160, 7, 64), (4, 4096, 512, 8), (1, 134144, 16, 8)]
# (B, nsplit, kind)
TAIL_CASES = [(1, 8, "plain"), (3, 8, "plain"), (6, 8, "plain"), (1, 0, "plain"), (3, 0, "plain"), (6, 0, "plain"),
              (3, 8, "degenerate"), (3, 0, "degenerate")]
TAIL_SHAPES = [(256, 512), (256,), (256, 256), (256,), (64, 128), (64,), (32, 64), (32,), (6, 32), (6,),
               (64, 128), (64,), (32, 64), (32,), (3, 32), (3,)]


# ------------------------------------------------------------------------------------------------------------------
# the tap of csrc/ac_taps.h, in fp32
# ------------------------------------------------------------------------------------------------------------------
def axis_taps(n_fine, h):
    """The n_fine taps of an axis resized from h points (align_corners) as axis_tap forms them:
    scale = fl(fl(h - 1) / fl(n_fine - 1)) (0 when n_fine == 1), f = fl(scale I), i0 = (int) f, i1 = i0 + (i0 < h - 1),
    l = f - i0 (exact) -> (i0, i1 int64, l float64 holding the fp32 value, f float64 likewise)."""
    scale = np.float32(h - 1) / np.float32(n_fine - 1) if n_fine > 1 else np.float32(0.0)
    f = (np.float32(scale) * np.arange(n_fine, dtype=np.float32)).astype(np.float32)
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < h - 1)
    l = (f - i0.astype(np.float32)).astype(np.float32)
    assert i0.min() >= 0 and i1.max() <= h - 1 and l.min() >= 0.0 and l.max() < 1.0
    as64 = lambda a: torch.from_numpy(a.astype(np.float64))
    return torch.from_numpy(i0.astype(np.int64)), torch.from_numpy(i1.astype(np.int64)), as64(l), as64(f)


def tap_matrix(n_fine, h, derivative=False):
    """(n_fine, h) float64: row I holds 1 - l at i0 and l at i1 (added where the two coincide); derivative: -1 and +1, the
    slope of the blend in l."""
    i0, i1, l, _ = axis_taps(n_fine, h)
    W = torch.zeros(n_fine, h, dtype=F64)
    rows = torch.arange(n_fine)
    W.index_put_((rows, i0), -torch.ones_like(l) if derivative else 1.0 - l, accumulate=True)
    W.index_put_((rows, i1), torch.ones_like(l) if derivative else l, accumulate=True)
    return W


def _nnz_cols(W):
    """The most fine points that touch one coarse point."""
    return int((W != 0).sum(0).max())


# ------------------------------------------------------------------------------------------------------------------
# correlation: row normalisation, then S_n . T_n^T
# ------------------------------------------------------------------------------------------------------------------
def correlation_arm(B, L):
    """cpn_correlation's dispatch, restated: the 64 x 64-per-wave kernel for L % 128 == 0 and at least 512 blocks of
    128 x 128; else 16 x 128 per wave (NT = 8) when that still gives 512 workgroups of 64 x 128; else 16 x 32 (NT = 2)."""
    if L % 128 == 0 and B * (L // 128) * (L // 128) >= 512:
        return "tile64"
    if B * cdiv(L, 128) * cdiv(L, 64) >= 512:
        return "nt8"
    return "nt2"


def correlation_ref(src, trg, eps=EPS_NORM):
    """src, trg (B, L, C) -> dict: src_n, trg_n (B, L, C) float64 = x / (|x| + eps) with their terms (l2norm_fwd_ref: the
    norm's chain, the root, the sum with eps, the division) and corr (B, L, L) = src_n . trg_n^T formed from THOSE."""
    B, L, C = src.shape
    res = {}
    for name, x in (("src_n", src), ("trg_n", trg)):
        y, terms = l2norm_fwd_ref(x.reshape(B * L, C), eps)
        res[name], res[name + "_terms"] = y.reshape(B, L, C), {k: v.reshape(B, L, C) for k, v in terms.items()}
    res["corr"] = torch.einsum("bsc,btc->bst", res["src_n"], res["trg_n"])
    return res


def correlation_gemm_ref(src_n, trg_n):
    """The GEMM on the normalised rows AS GIVEN (the kernel's own fp32 outputs): C products in one chain per output,
    gam(C) on sum |s| |t|.  A row of zeros gives exact zeros: its bound is 0."""
    s, t = src_n.double(), trg_n.double()
    return torch.einsum("bsc,btc->bst", s, t), {"chain": gam(s.shape[-1]) * torch.einsum("bsc,btc->bst", s.abs(), t.abs())}


def make_corr_inputs(case):
    B, L, C = case
    gen = _gen("corr", B, L, C)
    src, trg = torch.randn(B, L, C, generator=gen), torch.randn(B, L, C, generator=gen)
    if case == CORR_ZERO_ROW:
        src[1, 3] = 0.0
        trg[0, 0] = 0.0
    return {"src": src.contiguous(), "trg": trg.contiguous()}


# ------------------------------------------------------------------------------------------------------------------
# bilinear resize (align_corners) and its adjoint
# ------------------------------------------------------------------------------------------------------------------
def resize_ref(x, H, W, mats=None):
    """x (planes, h, w) -> (planes, H, W): gam(6) on the blend of |x| (two levels of a (1 - l) + b l).  mats: other (Wy, Wx)
    than tap_matrix's, for the CPU pin against a float64 resize; the same in every reference below."""
    x = x.double()
    Wy, Wx = mats or (tap_matrix(H, x.shape[1]), tap_matrix(W, x.shape[2]))
    f = lambda t: torch.einsum("Yy,pyx,Xx->pYX", Wy, t, Wx)
    return f(x), {"blend": gam(6) * f(x.abs())}


def resize_adjoint_ref(g, h, w, mats=None):
    """g (planes, H, W) -> (planes, h, w): out[y][x] = sum_Y wy(Y, y) sum_X wx(X, x) g[Y][X], the transpose of resize_ref's
    matrix.  A weight is (1 - l) [+ l]: 2 roundings; a product each with g and with the row; the row adds as many terms as
    fine columns touch x, the result as many as fine rows touch y: gam(ny + nx + 6) on the same sum of |g|."""
    g = g.double()
    Wy, Wx = mats or (tap_matrix(g.shape[1], h), tap_matrix(g.shape[2], w))
    f = lambda t: torch.einsum("Yy,pYX,Xx->pyx", Wy, t, Wx)
    return f(g), {"gather": gam(_nnz_cols(Wy) + _nnz_cols(Wx) + 6) * f(g.abs())}


def make_resize_inputs(case):
    planes, h, w, H, W = case
    gen = _gen("resize", *case)
    return {"x": torch.randn(planes, h, w, generator=gen), "g": torch.randn(planes, H, W, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# the final correlation: interpolate4d of the two coarse levels, ((u0 + u1) + c2) fl(1/3)
# ------------------------------------------------------------------------------------------------------------------
THIRD = float(np.float32(1.0) / np.float32(3.0))


def corr_mean3_arm(B, h0, h1):
    """cpn_corr_mean3's dispatch, restated: the LDS kernel while the eight tap planes (4 of each level) fit in 60 KiB."""
    return "planes" if 4 * (h0 * h0 + h1 * h1) * 4 <= 60 * 1024 and B < 65536 else "thread"


def interp4d(x, n, W=None):
    """x (B, h, h, h, h) float64 -> (B, n, n, n, n): both bilinear passes of interpolate4d, every axis through tap_matrix."""
    W = tap_matrix(n, x.shape[-1]) if W is None else W
    for _ in range(4):
        x = torch.tensordot(x, W, dims=([1], [1]))             # the contracted axis leaves the front, its image joins the back
    return x


def corr_mean3_ref(c0, c1, c2, mats=None):
    """c_k (B, h_k, h_k, h_k, h_k), c2 at n -> ((u0 + u1) + c2) fl(1/3) with fl(1/3) the fp32 constant.  Terms:
        blend  fl(1/3) gam(12) (blend of |c0| + blend of |c1|)      (two 2-D passes per level)
        sum    gam(3) fl(1/3) (blend |c0| + blend |c1| + |c2|)      (two additions, the product)"""
    n = c2.shape[-1]
    c0, c1, c2 = c0.double(), c1.double(), c2.double()
    W0, W1 = mats or (None, None)
    u0, u1 = interp4d(c0, n, W0), interp4d(c1, n, W1)
    m = interp4d(c0.abs(), n, W0) + interp4d(c1.abs(), n, W1)
    return ((u0 + u1) + c2) * THIRD, {"blend": THIRD * gam(12) * m, "sum": gam(3) * THIRD * (m + c2.abs())}


def make_mean3_inputs(case):
    B, h0, h1, n = case
    gen = _gen("mean3", *case)
    return {"c0": torch.randn(B, h0, h0, h0, h0, generator=gen), "c1": torch.randn(B, h1, h1, h1, h1, generator=gen),
            "c2": torch.randn(B, n, n, n, n, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# q / k assembly
# ------------------------------------------------------------------------------------------------------------------
def qk_assemble_ref(lin, low, pos, fs, h, w, nhead, dim, mats=None):
    """lin (B, L, 2d), low (B, 2d, h, w), pos (L, dim), d = nhead dim, L = fs fs -> (q, k (B, L, d), terms of each):
    [q | k][b, l, c] = (lin + up(low)[b, c, l]) + pos[l, c % dim], q the channels c < d and k the rest.  Terms:
        blend  gam(6) on the blend of |low|
        frac   the kernel keeps its own tap arithmetic and is compiled with contraction allowed, so l may be formed as
               fma(scale, I, -i0) from the UNROUNDED product: it then differs from the fp32 fraction by the product's rounding,
               u f, which moves the value by the blend's slope in l: u (fy |d up / d ly| + fx |d up / d lx|)
        sum    gam(2) (|lin| + blend |low| + |pos|)"""
    B, L, d2 = lin.shape
    d = nhead * dim
    assert d2 == 2 * d and L == fs * fs and tuple(low.shape) == (B, d2, h, w) and tuple(pos.shape) == (L, dim)
    lin, low, pos = lin.double(), low.double(), pos.double()
    Wy, Wx = mats or (tap_matrix(fs, h), tap_matrix(fs, w))
    Dy, Dx = tap_matrix(fs, h, True), tap_matrix(fs, w, True)
    fy, fx = axis_taps(fs, h)[3], axis_taps(fs, w)[3]
    f = lambda A, t, Bm: torch.einsum("Yy,bcyx,Xx->bYXc", A, t, Bm).reshape(B, L, d2)
    up, mag = f(Wy, low, Wx), f(Wy, low.abs(), Wx)
    fyl, fxl = fy.repeat_interleave(fs).view(1, L, 1), fx.repeat(fs).view(1, L, 1)
    pe = pos[:, torch.arange(d2) % dim].unsqueeze(0)                                    # (1, L, 2d)
    want = (lin + up) + pe
    terms = {"blend": gam(6) * mag, "frac": U * (fyl * f(Dy, low, Wx).abs() + fxl * f(Wy, low, Dx).abs()),
             "sum": gam(2) * (lin.abs() + mag + pe.abs())}
    half = lambda t, a, b: t.expand(B, L, d2)[..., a:b].contiguous()
    return (half(want, 0, d), half(want, d, d2),
            {k_: half(v, 0, d) for k_, v in terms.items()}, {k_: half(v, d, d2) for k_, v in terms.items()})


def make_qk_inputs(case):
    B, fs, h, w, nhead, dim = case
    gen = _gen("qk", *case)
    d2 = 2 * nhead * dim
    return {"lin": torch.randn(B, fs * fs, d2, generator=gen), "low": torch.randn(B, d2, h, w, generator=gen),
            "pos": torch.randn(fs * fs, dim, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# low-resolution cost-volume attention
# ------------------------------------------------------------------------------------------------------------------
def cva_ref(q, k, v_low, residual, fs, eps=EPS_LA, mats=None, stock=False):
    """q, k (B, L, H, 32), v_low / residual / result (B, H, P, Dv), P = hs hs, L = fs fs.  The REFERENCE's order in float64:
    v_low upsampled to fs x fs with the fp32-formed taps, LinearAttention over the L tokens (phi = elu + 1; KV over v / L,
    the message times L), the message sampled down to hs x hs, + residual.
    The bound follows the kernel, which forms the same thing as Qd (Kd^T v_low) with Kd = U^T phi(k) (P x 32),
    Qd = D (Z phi(q)) (P x 32), all of whose factors but v are positive; mag = sum_d Qd sum_p Kd |v|:
        kd   gam(2 nu + 8 + 16 + nblk + 1) mag      a Kd entry gathers nu x nu tokens (2 nu additions in its two chains;
                                                    phi 2, a weight 2, the products 2 ... 8), the partial of M adds 16
                                                    positions, the nblk = ceil(P / 16) partials add in order, one product
        qd   gam(nks + 18) mag                      Z's denominator holds sum phi(k) (nks = ceil(ceil(L / nblk) / 8) + 8 + nblk
                                                    + 2: per-thread chain, the tree of 8, the blocks, phi) in a 32-term dot
                                                    (1 + 5), + eps, phi(q) 2, the weight (1 - lx)(1 - ly) 3, its product, the
                                                    division, the 4 taps: 18
        dot  gam(34) mag [+ u (|residual| + |result|)]   the 32-term chain of Qd . M, its products, the residual's addition
    stock: the bound of the training form instead (cost_volume_attention_torch: the same association with library ops around
    the resize kernel and its adjoint).  Its chains are the library's: P terms in Kd^T v (for 16 + nblk), L in sum phi(k)
    (for the blocked sum).  And its phi is F.elu(x) + 1 = fl(fl(expm1(x)) + 1), whose error is ABSOLUTE, 2 u, where the kernel's
    expf is relative - the term
        elu  2 u carried through: d Kd_p = 2 u sum_l U_lp, d M = sum_p d Kd_p |v_p|; d den_l = 2 u (sum_d Ks_d + L sum_d Q_ld),
             d (Z Q)_ld = 2 u Z_l + Q_ld Z_l^2 d den_l, d Qd = D d (Z Q); d out = sum_d (d Qd_pd Mabs_d + Qd_pd d M)"""
    B, L, H, D = q.shape
    P, Dv = v_low.shape[2], v_low.shape[3]
    hs = math.isqrt(P)
    assert L == fs * fs and hs * hs == P and D == 32
    Wu, Wd = mats or (tap_matrix(fs, hs), tap_matrix(hs, fs))
    Uw, Dw = torch.kron(Wu, Wu), torch.kron(Wd, Wd)                                    # (L, P), (P, L)
    v = v_low.double()
    Q, K = _phi(q.double()), _phi(k.double())
    vc = torch.einsum("lp,bhpv->blhv", Uw, v)
    KV = torch.einsum("bshd,bshv->bhdv", K, vc / L)
    Z = 1 / (torch.einsum("blhd,bhd->blh", Q, K.sum(1)) + eps)
    msg = torch.einsum("blhd,bhdv,blh->blhv", Q, KV, Z) * L
    out = torch.einsum("pl,blhv->bhpv", Dw, msg)
    Kd = torch.einsum("lp,blhd->bhpd", Uw, K)
    Qd = torch.einsum("pl,blhd->bhpd", Dw, Q * Z.unsqueeze(-1))
    Mabs = torch.einsum("bhpd,bhpv->bhdv", Kd, v.abs())
    mag = torch.einsum("bhpd,bhdv->bhpv", Qd, Mabs)
    nu, nblk = _nnz_cols(Wu), cdiv(P, 16)
    nks = L + 2 if stock else cdiv(cdiv(L, nblk), 8) + 8 + nblk + 2
    terms = {"kd": gam(2 * nu + 8 + (P if stock else 16 + nblk) + 1) * mag, "qd": gam(nks + 18) * mag, "dot": gam(34) * mag}
    if stock:
        dM = 2 * U * torch.einsum("p,bhpv->bhv", Uw.sum(0), v.abs())
        dden = 2 * U * (K.sum(1).sum(-1).unsqueeze(1) + L * Q.sum(-1))                  # (B, L, H)
        dZQ = 2 * U * Z.unsqueeze(-1) + Q * (Z * Z * dden).unsqueeze(-1)
        dQd = torch.einsum("pl,blhd->bhpd", Dw, dZQ)
        terms["elu"] = torch.einsum("bhpd,bhdv->bhpv", dQd, Mabs) + Qd.sum(-1).unsqueeze(-1) * dM.unsqueeze(2)
    if residual is not None:
        out = residual.double() + out
        terms["dot"] = terms["dot"] + U * (residual.double().abs() + out.abs())
    return out, terms


def make_cva_inputs(case):
    B, fs, H, hs, Dv = case
    gen = _gen("cva", *case)
    r = lambda *s: torch.randn(*s, generator=gen)
    return {"q": 0.7 * r(B, fs * fs, H, 32), "k": 0.7 * r(B, fs * fs, H, 32), "v": r(B, H, hs * hs, Dv), "res": r(B, H, hs * hs, Dv)}


# ------------------------------------------------------------------------------------------------------------------
# pose head: the positional table
# ------------------------------------------------------------------------------------------------------------------
def pose_positional_ref(K, H, lin):
    """K (B, V, 4, 4) raw intrinsics (view 0 is used), H the image size, lin (n,) the fp32 grid -> (B, n n, 6):
    (p3^2, p4^2, p3 p4, p3, p4, 1) at index col n + row with p4 = (lin[col] - c) / a, p3 = (lin[row] - d) / b,
    a = 2 (fx / H) / (2 cx / H), c = 2 (cx / H) / (2 cx / H) - 1 (= 0), b and d alike from fy, cy.
    a is a quotient of two rounded quotients: 3 roundings; c: the quotient and the difference, 2 u absolute;
    p = (lin - c) / a: the difference, a's 3, the division - 5 u |p| + 2 u / |a|.  A square doubles it and rounds, the
    product adds both and rounds; the ones are exact."""
    B, n = K.shape[0], lin.shape[0]
    Kd, H, lin = K.double(), float(H), lin.double()
    fx, fy, cx, cy = (Kd[:, 0, 0, 0] / H).view(B, 1), (Kd[:, 0, 1, 1] / H).view(B, 1), (Kd[:, 0, 0, 2] / H).view(B, 1), (Kd[:, 0, 1, 2] / H).view(B, 1)
    hp, wp = cy * 2, cx * 2
    a, b = (fx / wp) * 2, (fy / hp) * 2
    c, d = (cx / wp) * 2 - 1, (cy / hp) * 2 - 1
    xs, ys = lin.repeat_interleave(n).view(1, -1), lin.repeat(n).view(1, -1)
    p4, p3 = (xs - c) / a, (ys - d) / b
    e4, e3 = gam(5) * p4.abs() + 2 * U / a.abs(), gam(5) * p3.abs() + 2 * U / b.abs()
    want = torch.stack((p3 * p3, p4 * p4, p3 * p4, p3, p4, torch.ones_like(p3)), 2)
    bound = torch.stack((2 * e3 * p3.abs() + U * p3 * p3, 2 * e4 * p4.abs() + U * p4 * p4,
                         e3 * p4.abs() + e4 * p3.abs() + U * (p3 * p4).abs(), e3, e4, torch.zeros_like(p3)), 2)
    return want, {"grid": bound}


def make_pospos_inputs(case):
    B, V, n = case
    gen = _gen("pospos", *case)
    K = torch.eye(4).repeat(B, V, 1, 1)
    H = 256.0
    K[:, :, 0, 0] = 180.0 + 60.0 * torch.rand(B, V, generator=gen)                      # fx != fy, cx != cy
    K[:, :, 1, 1] = 260.0 + 60.0 * torch.rand(B, V, generator=gen)
    K[:, :, 0, 2] = 110.0 + 20.0 * torch.rand(B, V, generator=gen)
    K[:, :, 1, 2] = 140.0 + 20.0 * torch.rand(B, V, generator=gen)
    return {"K": K.contiguous(), "H": H, "lin": torch.linspace(-1, 1, steps=n)}


# ------------------------------------------------------------------------------------------------------------------
# pose head: the chunked first layer
# ------------------------------------------------------------------------------------------------------------------
def gemv_chunks(K, nsplit):
    """[(lo, hi)] in units of one x / W element: chunk c covers 16-byte groups [c per, min((c + 1) per, K / 4)),
    per = ceil(K / 4 / nsplit); a chunk past the end is empty."""
    k4 = K // 4
    per = cdiv(k4, nsplit)
    return [(4 * min(c * per, k4), 4 * min(c * per + per, k4)) for c in range(nsplit)]


def pose_gemv_ref(x, W, nsplit):
    """x (B, K), W (O, K) -> partial (B, O, nsplit): chunk c's share of <W[o], x[b]>.  A thread adds a group of four products
    ((p0 + p1) + (p2 + p3): 1 + 2) per 256 groups of its chunk, the wave reduces in 6 steps and the four waves in 2:
    gam(ceil(per / 256) + 11) on the chunk's sum |w| |x|.  An empty chunk is an exact zero."""
    x, W = x.double(), W.double()
    K = x.shape[1]
    n = cdiv(cdiv(K // 4, nsplit), 256) + 11
    want, mag = [], []
    for lo, hi in gemv_chunks(K, nsplit):
        want.append(x[:, lo:hi] @ W[:, lo:hi].T)
        mag.append(x[:, lo:hi].abs() @ W[:, lo:hi].abs().T)
    return torch.stack(want, 2), {"chain": gam(n) * torch.stack(mag, 2)}


def make_gemv_inputs(case):
    B, K, O, nsplit = case
    gen = _gen("gemv", *case)
    return {"x": torch.randn(B, K, generator=gen), "W": torch.randn(O, K, generator=gen)}


# ------------------------------------------------------------------------------------------------------------------
# pose head: the dense tail, the 6-D rotation, the 4 x 4 assembly
# ------------------------------------------------------------------------------------------------------------------
def _dense(x, e, W, b):
    """y = W relu(x) + b with the error e of x carried through (|relu(a) - relu(b)| <= |a - b|): lanes stride over the inputs
    (ceil(n_in / 64) products in a chain), 6 wave steps, the product, the bias: gam(ceil(n_in / 64) + 8)."""
    W, b = W.double(), b.double()
    r = torch.relu(x)
    n = cdiv(W.shape[1], 64) + 8
    return r @ W.T + b, e @ W.abs().T + gam(n) * (r @ W.abs().T + b.abs())


def _unit(a, ea, rnd):
    """a / max(|a|, 1e-12) along the last dim with the error ea of a carried through the projection (I - b b^T) / |a| and, if
    rnd, its own roundings: the squares, two additions, the root (halved), the division - 4 u."""
    n = torch.clamp(a.norm(dim=-1, keepdim=True), min=1e-12)
    b = a / n
    return b, (ea + b.abs() * (b.abs() * ea).sum(-1, keepdim=True)) / n + rnd * 4 * U * b.abs()


def _cross(a, b):
    return torch.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def _rotation(a1, a2, e1, e2, rnd):
    """Rows b1, b2, b1 x b2 of Zhou et al.'s 6-D rotation and their first-order error from the errors e1, e2 of a1, a2 (rnd = 0)
    or from the rotation's own roundings (rnd = 1, e = 0): dt = b1 . a2 (gam(3)), u = a2 - dt b1 (the product, the
    difference), b2 = u / |u|, a cross product's component (two products, a difference: gam(2) on its two terms)."""
    b1, d1 = _unit(a1, e1, rnd)
    dt = (b1 * a2).sum(-1, keepdim=True)
    ddt = (d1 * a2.abs() + b1.abs() * e2).sum(-1, keepdim=True) + rnd * gam(3) * (b1 * a2).abs().sum(-1, keepdim=True)
    u = a2 - dt * b1
    du = e2 + ddt * b1.abs() + dt.abs() * d1 + rnd * U * ((dt * b1).abs() + u.abs())
    b2, d2 = _unit(u, du, rnd)
    return torch.stack((b1, b2, _cross(b1, b2)), -2), torch.stack((d1, d2, _cross_abs(b1.abs(), d1, b2.abs(), d2, rnd)), -2)


def _cross_abs(p, dp, q, dq, rnd):
    pair = lambda i, j: dp[..., i] * q[..., j] + p[..., i] * dq[..., j] + rnd * gam(2) * p[..., i] * q[..., j]
    return torch.stack((pair(1, 2) + pair(2, 1), pair(2, 0) + pair(0, 2), pair(0, 1) + pair(1, 0)), -1)


def pose_tail_ref(h, nsplit, bias0, weights):
    """h (B, 512, nsplit) chunk partials (summed in chunk order, + bias0: gam(nsplit)) or, nsplit == 0, (B, 512) a finished first
    layer (exact); weights: the 16 tensors of TAIL_SHAPES -> rel_pose (B, 4, 4).  Five dense layers (_dense), the latent is the
    first 128 of the second's ReLU, the rotation from six and the translation from three outputs, the bottom row 0 0 0 1.
        dense  the layers' accumulated error carried into the rotation / translation   rot  the rotation's own roundings"""
    w2, b2, w3, b3, r1, rb1, r2, rb2, r3, rb3, t1, tb1, t2, tb2, t3, tb3 = weights
    h = h.double()
    if nsplit > 0:
        s0 = h.sum(-1) + bias0.double()
        e0 = gam(nsplit) * (h.abs().sum(-1) + bias0.double().abs())
    else:
        s0, e0 = h, torch.zeros_like(h)
    s1, e1 = _dense(s0, e0, w2, b2)
    s2, e2 = _dense(s1, e1, w3, b3)
    lat, el = s2[:, :128], e2[:, :128]
    r, er = _dense(*_dense(*_dense(lat, el, r1, rb1), r2, rb2), r3, rb3)
    t, et = _dense(*_dense(*_dense(lat, el, t1, tb1), t2, tb2), t3, tb3)
    R, dR_in = _rotation(r[:, :3], r[:, 3:], er[:, :3], er[:, 3:], 0)
    _, dR_own = _rotation(r[:, :3], r[:, 3:], torch.zeros_like(er[:, :3]), torch.zeros_like(er[:, 3:]), 1)
    B = h.shape[0]
    want = torch.zeros(B, 4, 4, dtype=F64)
    want[:, :3, :3], want[:, :3, 3], want[:, 3, 3] = R, t, 1.0
    dense, rot = torch.zeros(B, 4, 4, dtype=F64), torch.zeros(B, 4, 4, dtype=F64)
    dense[:, :3, :3], dense[:, :3, 3], rot[:, :3, :3] = dR_in, et, dR_own
    return want, {"dense": dense, "rot": rot}


def make_tail_inputs(case):
    """The carried error of a dense chain grows by the row sums of |W| from layer to layer, so the weights are drawn with row
    sums near 1 - |N(0, 1)| 1.2 / fan_in, one sign in five flipped - and the biases (N(0, 0.5)) keep about a third of every
    layer's outputs below 0 for the ReLUs: the bound then stays at the roundings of a few O(1) sums and a defect in any layer is
    far outside it.  The six rotation outputs get an O(1) bias: |a1| and |a2 - (b1 . a2) b1| are O(1) (asserted by the CPU
    test).  degenerate: rows 0..2 of the last rotation layer and their biases are zero."""
    B, nsplit, kind = case
    gen = _gen("tail", B, kind)
    weights = []
    for shape in TAIL_SHAPES:
        if len(shape) == 2:
            sign = torch.where(torch.rand(*shape, generator=gen) < 0.2, -1.0, 1.0)
            weights.append(torch.randn(*shape, generator=gen).abs() * sign * (1.2 / shape[1]))
        else:
            weights.append(torch.randn(*shape, generator=gen) * (1.0 if shape[0] == 6 else 0.5))
    if kind == "degenerate":
        weights[8][:3] = 0.0
        weights[9][:3] = 0.0
    part = torch.randn(B, 512, 8, generator=gen) * 0.35 + 0.05                           # eight partials: a sum of spread ~ 1
    bias0 = torch.randn(512, generator=gen) * 0.1 + 0.1
    h = part if nsplit else (part.sum(-1) + bias0).contiguous()                           # nsplit == 0: a finished first layer
    return {"h": h.contiguous(), "bias0": bias0, "weights": weights}
