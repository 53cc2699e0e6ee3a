"""Float64 references, with element-wise error bounds, of the forward kernels of the reference-arithmetic render mode
(precision = "f32": render_f32.node_tables / render_f32.per_sample) - cpn_node_features_f32 and cpn_encode_hidden_f32(_rays)
(csrc/encode_f32.hip), the (hi, lo) key layer as two cpn_gemm_f16 calls (csrc/gemm_f16.hip, out_f32 = 1 then 2) and
cpn_linear_f32 (csrc/linear_f32.hip) - for tests/test_encode_f32_ref.py (CPU) and tests/test_gpu_encode_f32.py (GPU).
Helpers, not tests.

Nothing here looks at a kernel's output.  A reference takes the values a kernel READS (fp32 / fp16 bits converted to float64)
and forms the mathematical result in float64; the index-deciding arithmetic (which node, which texel) is that of
tests/encode_bwd_ref.py - fp32 coordinates, one rounding per operation - and the geometry helpers are reused from there.
The bounds are first order in u = 2^-24 (fp32) and U16 = 2^-11 (fp16), from operation counts; S_abs is the same formula on
absolute values.  ReLU is 1-Lipschitz, so a bound on the pre-activation holds behind it and no element near zero is left out.

    cpn_node_features_f32   |d| <= (4 + 3) u S_abs                                    NODE_C = 7
            four products added one by one; the fp32 weight (1 - fx)(1 - fy) against the reference's float64 one (3 roundings;
            for power-of-two image sizes the weights are exact and the 3 are margin).
    cpn_encode_hidden_f32   |hi + lo - r| <= (68 + 4 + 4 + 6) u S_abs + U16^2 |r| + 2^-25     ENC_C = 82
            r = ReLU(sum_t a_t tab[node_t] + sum_k w80t[k] x_k), x = [bilinear(map3) 64 | pe 3 | 1].  The kernel: the producer
            wave blends each x_k from 4 texels (4 roundings on a term's path, carried through |w80t|), the owner waves run the
            K = 68 contraction on the fp32 MFMA - a k-ordered fmaf chain from 0, 68 steps - then add the 4 table taps one by
            one (4); the tap weights and the texel weights are fp32 products of fp32 fractions, 3 roundings each (6; a term
            meets only one of the two, the count is generous).  The split hi = fp16(r), lo = fp16(r - hi): r - hi is exact in
            fp32 and at most U16 |r|, its rounding at most U16 of that - or 2^-25 where lo is an fp16 subnormal.
    the (hi, lo) key layer  computed expression (x_hi + x_lo) W_hi^T + x_hi W_lo^T + b: with key_exact_data bit for bit;
            intended layer ReLU(x W^T + b): residue + (K1 + K2 + 16) u S_abs, K1 = 3328, K2 = 1664 terms per element in the
            two calls, 8 of margin per call (logits_ref.C_L2's convention, not a derivation); residue = what the stored halves
            cannot hold, sum |x - x~||W| + |x~||W - W~| + |x_lo||W_lo|, from the data.  Loose by design.
    cpn_linear_f32          |d| <= (K + 3) u S_abs: a K-step fmaf chain from 0, then bias, res (2) and one of margin.

Calibration on the CPU (tests/test_encode_f32_ref.py, the kernels' rounding points in fp32 torch), worst err/bound over the
GPU test's own cases:
    cpn_node_features_f32 0.434      cpn_encode_hidden_f32 0.114      cpn_linear_f32 0.179
    key layer, intended 0.011 (exact data: bit-equal under torch's k order and three random ones)
    the split alone, 2 x 10^6 values from 7e-10 to 65 000: 1.0000 - attained, not exceeded: the term is tight
"""
import torch

from tests import encode_bwd_ref as bref
from tests.logits_ref import assert_within, outside, ratio  # noqa: F401  (the comparison helpers of the float64 tests)

V = 2
U32 = 2.0 ** -24             # u: unit roundoff of fp32
U16 = 2.0 ** -11
SUB16 = 2.0 ** -25           # half the spacing of the fp16 subnormals
NODE_C = 4 + 3
ENC_C = 68 + 4 + 4 + 6
K1, K2 = 3328, 1664          # terms per element of the key layer's two calls
KEY_C = K1 + K2 + 16
HS_LD = 3328                 # [hi_own | hi_other | lo_own | lo_other]
F16_LIMIT = 65520.0          # fp16(r) is inf from here on

# (H, W, nimg) of the node-feature test; (H, W, B, R, S, ray0, nrays) of the encode tests
NODE_CASES = [(16, 16, 3), (32, 32, 1), (64, 64, 2), (32, 64, 2)]
ENC_CASES = [(32, 32) + c for c in bref.RAGGED] + [(32, 64, 2, 7, 9, 3, 9), (64, 64, 2, 7, 9, 3, 9)]
ENC_IDS = ["%dx%d-B%d-R%d-S%d-ray%d+%d" % c for c in ENC_CASES]
# (M, N, K) of cpn_linear_f32: all three launch forms (N <= 16; M <= 16 384; above), odd K / 16, partial column tiles
LIN_CASES = [(1, 128, 16), (15, 128, 48), (17, 3, 128), (100, 64, 768), (260, 128, 1664), (16385, 128, 416), (16385, 20, 16),
             (64, 16, 32)]
KEY_M = [4, 60, 260, 1028]


# ------------------------------------------------------------------------------------------------------------------
# cpn_node_features_f32
# ------------------------------------------------------------------------------------------------------------------
def node_maps(H, W, nimg, gen, scale=10.0, exact=False):
    """The three coarse levels, NCHW fp32 with full mantissas.  exact: integers in -8..8 - for H, W powers of two the node
    fractions are multiples of 1/16 and the weights of 1/256, so the four products and their sums are exact in fp32."""
    shapes = [(nimg, 256, H >> (4 - l), W >> (4 - l)) for l in range(3)]
    if exact:
        return [torch.randint(-8, 9, s, generator=gen).float() for s in shapes]
    return [torch.randn(s, generator=gen) * scale for s in shapes]


def node_features_f32_ref(z, H, W):
    """-> (want, bound, s_abs), (nimg * table_nodes, 768) float64: node_features_ref on float64 copies of the fp32 maps;
    S_abs = sum_k |w_k v_k| from the operator's own matrix (node_features_matrix)."""
    nimg = z[0].shape[0]
    want = bref.node_features_ref(z[0], z[1], z[2], H, W)
    s_abs = []
    for l in range(3):
        A = bref.node_features_matrix(l, H, W).abs()                                    # (per, Hl Wl)
        s_abs.append(torch.einsum("pt,nct->npc", A, z[l].double().abs().flatten(2)))
    s_abs = torch.cat(s_abs, 2).reshape(nimg * bref.table_nodes(H, W), 768)
    return want, NODE_C * U32 * s_abs, s_abs


def rim_nodes(H, W, nimg):
    """(is_border, is_rim) of every table row: rim = the zeros-table nodes -4..-1 and M+1..M+4 of either axis."""
    (h0, w0), (h1, w1) = bref.table_dims(H, W, 0), bref.table_dims(H, W, 1)
    ny = torch.arange(h1).view(-1, 1) - bref.PAD
    nx = torch.arange(w1).view(1, -1) - bref.PAD
    rim = ((ny < 0) | (ny > H // 2) | (nx < 0) | (nx > W // 2)).reshape(-1)
    is_border = torch.cat((torch.ones(h0 * w0, dtype=torch.bool), torch.zeros(h1 * w1, dtype=torch.bool)))
    is_rim = torch.cat((torch.zeros(h0 * w0, dtype=torch.bool), rim))
    return is_border.repeat(nimg), is_rim.repeat(nimg)


# ------------------------------------------------------------------------------------------------------------------
# cpn_encode_hidden_f32
# ------------------------------------------------------------------------------------------------------------------
def encode_inputs(case, exact=False):
    """Everything one launch reads, on the CPU: tab (N nodes, 832), map3 (N, H, W, 64) NHWC, w80t (68, 832) (bias = row 67),
    pixel_val / sec_grid (N, R, S, 2), pe6 (N, R, S, 6) - random fp32 with full mantissas, coordinates random + the hostile
    set.  exact: coordinates on quarter-node fractions inside the image and small-integer values, so that every product and
    partial sum of a row is exact in fp32 (encode_exact_ok asserts it)."""
    H, W, B, R, S, ray0, nrays = case
    gen = torch.Generator().manual_seed(31 * H + W + 1000 * B + 10 * R + S)
    N = B * V
    nodes = N * bref.table_nodes(H, W)
    if exact:
        q = lambda *shape: torch.randint(-4, 5, shape, generator=gen).float()
        pos = lambda M: bref.node_coord(torch.randint(0, 4 * M + 1, (N, R, S), generator=gen).float() / 4, M)
        pv = torch.stack((pos(W // 2), pos(H // 2)), -1)
        sg = torch.stack((pos(W // 2), pos(H // 2)), -1)
        return {"tab": q(nodes, 832), "map3": q(N, H, W, 64), "w80t": q(68, 832), "pv": pv.contiguous(), "sg": sg.contiguous(),
                "pe6": q(N, R, S, 6) / 4}
    pv, sg = bref.random_coords(N, R, S, gen)
    bref.plant_hostile(pv, sg, H, W, gen)
    return {"tab": torch.randn(nodes, 832, generator=gen) * 2.0, "map3": torch.randn(N, H, W, 64, generator=gen) * 3.0,
            "w80t": torch.randn(68, 832, generator=gen) * 0.1, "pv": pv.contiguous(), "sg": sg.contiguous(),
            "pe6": (torch.rand(N, R, S, 6, generator=gen) * 2 - 1).contiguous()}


def encode_taps(d, B, R, S, H, W):
    """The taps of EVERY row of the (B, R, S) problem in the header's row order, row = ((ray V + v) S + s) 2 + j: table rows
    `node` (rows, 4) with float64 weights `a`, texels of map3 `tex` (rows, 4) with weights `b` (index into (N H W, 64)), and
    the row's point encoding `pe` (rows, 3) = pe6[sample of (b, v)][3 j : 3 j + 3]."""
    rt = bref.row_table(B, V, R, S, 0, B * R)
    g = bref.row_coords(rt, d["pv"], d["sg"])
    node, a = bref.node_taps_ref(g, rt["kind"], H, W)
    tex, b = bref.level_taps_ref(g, rt["kind"], H, W)
    pe = d["pe6"].reshape(-1, 2, 3)[rt["src"], rt["kind"]]
    return {"node": rt["img"].view(-1, 1) * bref.table_nodes(H, W) + node, "a": a, "tex": rt["img"].view(-1, 1) * (H * W) + tex,
            "b": b, "pe": pe, "img": rt["img"], "kind": rt["kind"], "g": g}


def encode_hidden_f32_ref(tab, map3, w80t, taps):
    """-> (r, bound, pre, s_abs) of every row of `taps`, (rows, 832) float64 (the counting: module docstring)."""
    tab64, m64, w64 = tab.double(), map3.double().reshape(-1, 64), w80t.double()
    t1 = torch.zeros(taps["node"].shape[0], 832, dtype=torch.float64)
    a1 = torch.zeros_like(t1)
    x3 = torch.zeros(taps["node"].shape[0], 64, dtype=torch.float64)
    x3a = torch.zeros_like(x3)
    for k in range(4):
        t1 += taps["a"][:, k:k + 1] * tab64[taps["node"][:, k]]
        a1 += taps["a"][:, k:k + 1].abs() * tab64[taps["node"][:, k]].abs()
        x3 += taps["b"][:, k:k + 1] * m64[taps["tex"][:, k]]
        x3a += taps["b"][:, k:k + 1].abs() * m64[taps["tex"][:, k]].abs()
    one = torch.ones(x3.shape[0], 1, dtype=torch.float64)
    pe = taps["pe"].double()
    pre = t1 + torch.cat((x3, pe, one), 1) @ w64
    s_abs = a1 + torch.cat((x3a, pe.abs(), one), 1) @ w64.abs()
    r = torch.relu(pre)
    assert float(r.max()) < F16_LIMIT, "a reference value leaves fp16's range"
    bound = ENC_C * U32 * s_abs + U16 * U16 * r + SUB16
    return r, bound, pre, s_abs


def near_zero(pre, bound):
    """The elements whose ReLU mask the kernel's rounding may flip: |pre-activation| <= bound.  They are compared like every
    other element, |got - max(pre, 0)| <= bound (max(., 0) of either side of a flip differs by less than the bound)."""
    return pre.abs() <= bound


def ray_rows(x, rays, S):
    """(B R V S 2, C) in row order -> the rows of the listed rays, in list order."""
    return x.reshape(-1, V * S * 2, x.shape[-1])[rays].reshape(len(rays) * V * S * 2, -1)


def split_hs(hs):
    """hs (rows, 3328) fp16 -> (hi, lo), each (rows 2, 832) fp16 in row order (row 2 + j)."""
    t = hs.reshape(-1, 2, 2, 832)                                                     # [row][hi / lo][j][channel]
    return t[:, 0].reshape(-1, 832), t[:, 1].reshape(-1, 832)


def make_hs(r):
    """(rows 2, 832) fp32 -> hs (rows, 3328) fp16, the split on the host: hi = fp16(r), lo = fp16(r - hi)."""
    hi = r.half()
    lo = (r - hi.float()).half()
    return torch.stack((hi.reshape(-1, 2, 832), lo.reshape(-1, 2, 832)), 1).reshape(-1, HS_LD).contiguous()


def encode_exact_ok(d, taps):
    """The exactness condition of the exact-data case: every weight a multiple of 2^-4 (quarter fractions), every value a
    multiple of 2^-2, so every term is a multiple of 2^-8, and sum |terms| < 2^16: every partial sum, in any order, has at
    most 24 significant bits.  The same for the four-term blend of every x_k."""
    for w in (taps["a"], taps["b"]):
        assert bool(((w * 16) == (w * 16).round()).all())
    for t in ("tab", "map3", "w80t", "pe6"):
        assert bool(((d[t] * 4) == (d[t] * 4).round()).all())
    _, _, _, s_abs = encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    assert float(s_abs.max()) < 2.0 ** 16
    return True


def split_ladder():
    """(72,) fp32 bias values of the split sweep: 2^-26 .. 2^15.5 geometrically (64), then the edges: the largest inputs below
    fp16's overflow, the smallest normal, the smallest subnormal, ties of the hi rounding, 0 and a negative."""
    lad = torch.pow(2.0, torch.linspace(-26.0, 15.5, 64, dtype=torch.float64)).float()
    edge = torch.tensor([65000.0, 65504.0, 2.0 ** -14, 2.0 ** -24, 1 + 2.0 ** -11, 1 + 2.0 ** -12, 0.0, -3.0])
    out = torch.cat((lad, edge))
    assert float(out.max()) < F16_LIMIT
    return out


# ------------------------------------------------------------------------------------------------------------------
# the (hi, lo) key layer
# ------------------------------------------------------------------------------------------------------------------
def key_split(W):
    """(N, 1664) fp32 -> (w1 (N, 3328) = [W_hi | W_hi], w2 (N, 1664) = W_lo) fp16, as render_f32.weights forms them."""
    hi = W.half()
    lo = (W - hi.float()).half()
    return torch.cat((hi, hi), 1).contiguous(), lo.contiguous()


def key_computed_ref(hs, w1, w2, b1, b2=None, relu2=True):
    """What the two calls compute, in float64 from the stored halves: call 1 (out_f32 = 1, no ReLU) C = [hi | lo] w1^T + b1,
    call 2 (out_f32 = 2) C += hi w2^T + b2, then the ReLU."""
    x = hs.double()
    c = x @ w1.double().t() + b1.double()
    c = c + x[:, :K2] @ w2.double().t()
    if b2 is not None:
        c = c + b2.double()
    return torch.relu(c) if relu2 else c


def key_intended_ref(x, W, b, hs, w1, w2):
    """The layer the two calls stand for, ReLU(x W^T + b) with x, W fp32 -> (want, bound): bound = residue + KEY_C u S_abs
    (module docstring), everything in float64 from the data."""
    x64, W64 = x.double(), W.double()
    xh, xl = hs[:, :K2].double(), hs[:, K2:].double()
    Wh, Wl = w1[:, :K2].double(), w2.double()
    want = torch.relu(x64 @ W64.t() + b.double())
    residue = (x64 - xh - xl).abs() @ W64.abs().t() + (xh + xl).abs() @ (W64 - Wh - Wl).abs().t() + xl.abs() @ Wl.abs().t()
    s_abs = (xh.abs() + xl.abs()) @ Wh.abs().t() + xh.abs() @ Wl.abs().t() + b.double().abs()
    return want, residue + KEY_C * U32 * s_abs


def key_exact_data(M, gen, N=128):
    """x (M, 1664), W (N, 1664), b (N) fp32 whose (hi, lo) products are all multiples of 2^-13 with sum |terms| < 2^11: every
    partial sum of the computed expression, in any order, is exact in fp32, so a kernel that forms it must match float64 bit
    for bit.  x: 40 non-zeros per row, m + n 2^-12 (m in 8..15, n in 0..15: hi = m, lo = n 2^-12); W = s (P + q 2^-13), s = +-1,
    P in {2, 3}, q in 0..7 (W_hi = s P, W_lo = s q 2^-13); b a multiple of 2^-6, |b| <= 1.  Both facts are asserted here."""
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).double()
    x = torch.zeros(M, K2, dtype=torch.float64)
    cols = torch.rand(M, K2, generator=gen).argsort(1)[:, :40]
    x.scatter_(1, cols, ri(8, 15, M, 40) + ri(0, 15, M, 40) * 2.0 ** -12)
    W = (ri(0, 1, N, K2) * 2 - 1) * (ri(2, 3, N, K2) + ri(0, 7, N, K2) * 2.0 ** -13)
    b = ri(-64, 64, N) * 2.0 ** -6
    x, W, b = x.float(), W.float(), b.float()
    hs = make_hs(x.reshape(-1, 832))                                  # a row of x is [own 832 | other 832]
    w1, w2 = key_split(W)
    xh, xl, Wh, Wl = hs[:, :K2].double(), hs[:, K2:].double(), w1[:, :K2].double(), w2.double()
    assert torch.equal(xh + xl, x.double()) and torch.equal(Wh + Wl, W.double()), "the halves do not hold the data exactly"
    whole = lambda t: bool((t == t.round()).all())                    # x_hi, W_hi integers, x_lo 2^12 and W_lo 2^13 integers:
    assert whole(xh) and whole(Wh) and whole(xl * 2.0 ** 12) and whole(Wl * 2.0 ** 13)     # every product a multiple of 2^-13
    s_abs = (xh + xl).abs() @ Wh.abs().t() + xh.abs() @ Wl.abs().t() + 2.0                # + the two biases, each <= 1
    assert float(s_abs.max()) < 2.0 ** 11, "partial sums may leave 24 bits"
    return x, W, b, hs, w1, w2


def key_realistic_data(M, sigma, gen):
    """x = ReLU(N(0, sigma)) with planted values 1e-6, 2^-14, 100, 3000; W = N(0, 0.05); b = N(0, 0.1)."""
    x = torch.relu(torch.randn(M, K2, generator=gen) * sigma)
    for i, val in enumerate((1e-6, 2.0 ** -14, 100.0, 3000.0)):
        x[i::7, 5 + 11 * i] = val
    W = torch.randn(128, K2, generator=gen) * 0.05
    b = torch.randn(128, generator=gen) * 0.1
    return x, W, b, make_hs(x.reshape(-1, 832))


# ------------------------------------------------------------------------------------------------------------------
# cpn_linear_f32
# ------------------------------------------------------------------------------------------------------------------
def linear_f32_ref(X, W, bias, res, relu_in, relu_out):
    """act_out(act_in(X) W^T + bias + res) in float64 -> (want, bound), bound = (K + 3) u S_abs."""
    x = torch.relu(X.double()) if relu_in else X.double()
    y = x @ W.double().t()
    s_abs = x.abs() @ W.double().abs().t()
    for t in (bias, res):
        if t is not None:
            y = y + t.double()
            s_abs = s_abs + t.double().abs()
    return (torch.relu(y) if relu_out else y), (X.shape[1] + 3) * U32 * s_abs


def linear_data(M, N, K, gen, exact=False):
    """X (M, K), W (N, K), bias (N), res (M, N) fp32.  exact: integers in -8..8, three entries in four of X zero; sum |terms|
    < 2^24 is asserted: every partial sum is an integer below 2^24, exact in fp32 in any order."""
    if not exact:
        return (torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen),
                torch.randn(M, N, generator=gen))
    q = lambda *shape: torch.randint(-8, 9, shape, generator=gen).float()
    X = q(M, K) * (torch.rand(M, K, generator=gen) < 0.25)
    W, bias, res = q(N, K), q(N), q(M, N)
    s_abs = X.double().abs() @ W.double().abs().t() + bias.double().abs() + res.double().abs()
    assert float(s_abs.max()) < 2.0 ** 24
    return X, W, bias, res
