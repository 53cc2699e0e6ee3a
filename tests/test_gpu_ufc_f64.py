"""The fp32 kernels behind the training backward of get_z - cpn_soft_argmax_pair(_bwd), cpn_dual_softmax(_bwd),
cpn_cross_attention(_bwd), cpn_linear_attention(_bwd), cpn_gn_relu(_bwd), cpn_conv4d_dgrad, cpn_l2norm_rows_bwd,
cpn_transpose_pairs - each called on its raw entry and held, element by element, to its float64 reference and derived bound
(tests/ufc_bwd_ref.py; pinned and calibrated on the CPU by tests/test_ufc_bwd_ref.py).  A backward is checked on the forward
kernel's OWN outputs, after those were checked themselves.  No element is left out of any comparison; every output and every
scratch buffer starts as NaN and has GUARD elements behind it, which must come back intact; two runs of every backward give
the same bits (cpn_gn_relu_bwd, whose partial sums meet in float64 atomics, the same values to within the bound).

max err/bound of the first run on an MI355X, the worst over the cases of each kernel, with the terms that make up the bound at
that element.  The bounds are not tuned to these figures; the CPU emulation of tests/test_ufc_bwd_ref.py shows the same ones to
three digits wherever a figure is above 0.1.
  cpn_soft_argmax_pair          t_to_s 0.317 (coord 54 %, sum 46 %), s_to_t 0.153 (sum 82 %)          both at h = 16 realistic
  cpn_soft_argmax_pair_bwd      dc 0.598 (weight 89 %: the rounded argument of expf, |arg| up to 100)   h = 16 realistic
  cpn_dual_softmax              rsum 0.263, csum 0.151 (sum 78 %), f 0.910 (expf 96 %)                  gain 8
  cpn_dual_softmax_bwd          da 0.674 (expf 71 %, sum 17 %, ops 12 %)                                (2, 3, 40) gain 8
  cpn_cross_attention           src_attn 0.224, trg_attn 0.184 (sum 96 %)
  cpn_cross_attention_bwd       dcorr 0.450, dsrc_v 0.214, dtrg_v 0.335 (weight 63 - 86 %)
  cpn_linear_attention          out 0.070          cpn_linear_attention_bwd   dq 0.007, dk 0.010, dv 0.016
  cpn_gn_relu                   out 0.510 (ops 86 %, cast 14 %)
  cpn_gn_relu_bwd               dy 0.450 (mean = 5 spreads), dgn_w 0.295, dgn_b 0.098
  cpn_conv4d_dgrad              0.049 (fallback arm, Cout = 5), 0.033 (MFMA arm)
  cpn_l2norm_rows_bwd           src_n 0.304, dx 0.272 (norm 79 %)                                       1000 rows, C = 64
f at 0.91: nearly all of its bound is u |a - max|, the rounding of the exponential's argument, which is attained (half an
ulp of an argument near 50) somewhere among 159 000 elements.  The linear attention and the Conv4d gradient sit far inside:
their bounds charge every addition of a chain of hundreds at full u, and fp32 sums of random signs lose about its square root.
That first run also found a term the cross attention backward's bound lacked - a dcorr of 3.17e-41, one subnormal ulp from
float64, at 512 x 512 with gain 12 and g_src = 0 (3 of 262 144 elements, err/bound 17.5 without the term) - now the `underflow`
term of cross_bwd_ref; the dcorr figure above is of the run with it.
"""
import functools

import pytest
import torch

from tests import ufc_bwd_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from coponerf_amd._hip import call
    call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _st())


def _lib():
    from coponerf_amd import _hip
    return _hip.lib()


def _out(n, dev, dtype=F32):
    """A flat buffer of n elements pre-filled with NaN, with GUARD elements of 7 behind it."""
    buf = torch.full((int(n) + GUARD,), NAN, dtype=dtype, device=dev)
    buf[int(n):] = 7.0
    return buf


def _guard_ok(buf, what):
    assert bool((buf[-GUARD:] == 7.0).all()), f"{what}: wrote behind the buffer"


def _take(buf, shape, what):
    """The output on the host in `shape`, after the guard was seen intact and every element finite."""
    torch.cuda.synchronize()
    out = buf.cpu()
    _guard_ok(out, what)
    out = out[:-GUARD].view(*shape)
    assert bool(torch.isfinite(out).all()), f"{what}: elements left unwritten or not finite"
    return out


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: two runs differ"


def _check(what, got, want, terms):
    return ref.report(what, got, want, terms)


# ------------------------------------------------------------------------------------------------------------------
# K8: soft-argmax pair
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _argmax_inputs(case):
    return ref.make_argmax_inputs(case)


@pytest.mark.parametrize("case", ref.ARGMAX_CASES, ids=ref.case_id)
def test_soft_argmax_pair_against_float64(case, dev):
    """Forward outputs against the float64 expectations; then dc against the float64 gradient formed with those outputs.  dc
    starts as NaN: the row kernel must write every element before the column kernel adds to it."""
    h, B, regime = case
    T = h * h
    x = _argmax_inputs(case)
    c = x["c"].to(dev)
    o1, o2 = _out(B * 2 * T, dev), _out(B * 2 * T, dev)
    _call("cpn_soft_argmax_pair", c, B, h, 0.02, o1, o2)
    what = "argmax " + ref.case_id(case)
    t_to_s, s_to_t = _take(o1, (B, 2, T), what + " t_to_s"), _take(o2, (B, 2, T), what + " s_to_t")
    f = ref.argmax_fwd_ref(x["c"], h)
    _check(what + " t_to_s", t_to_s, f["t_to_s"], f["t_to_s_terms"])
    _check(what + " s_to_t", s_to_t, f["s_to_t"], f["s_to_t_terms"])
    want, terms = ref.argmax_bwd_ref(x["c"], h, t_to_s, s_to_t, x["g1"], x["g2"])
    g1, g2 = x["g1"].to(dev), x["g2"].to(dev)
    runs = []
    for _ in range(2):
        dc = _out(B * T * T, dev)
        _call("cpn_soft_argmax_pair_bwd", c, B, h, 0.02, o1, o2, g1, g2, dc)
        runs.append(_take(dc, (B, T, T), what + " dc"))
    _check(what + " dc", runs[0], want, terms)
    _same_bits(runs[0], runs[1], what + " dc")


# ------------------------------------------------------------------------------------------------------------------
# dual softmax
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.DUAL_CASES, ids=ref.case_id)
def test_dual_softmax_against_float64(case, dev):
    """rstat / cstat against float64 (the maxima exactly), f against the float64 product formed from the statistics the kernel
    returned, da against the float64 gradient on the kernel's own rstat / cstat / f."""
    B, L, M, gain = case
    x = ref.make_dual_inputs(case)
    a, df = x["a"].to(dev), x["df"].to(dev)
    rs, cs, fb = _out(B * L * 2, dev), _out(B * M * 2, dev), _out(B * L * M, dev)
    _call("cpn_dual_softmax", a, B, L, M, rs, cs, fb)
    what = "dual " + ref.case_id(case)
    rstat, cstat, f = _take(rs, (B, L, 2), what + " rstat"), _take(cs, (B, M, 2), what + " cstat"), _take(fb, (B, L, M), what + " f")
    st = ref.dual_stats_ref(x["a"])
    assert torch.equal(rstat[..., 0].double(), st["rmax"]) and torch.equal(cstat[..., 0].double(), st["cmax"]), what + ": maxima"
    _check(what + " rsum", rstat[..., 1], st["rsum"], st["rsum_terms"])
    _check(what + " csum", cstat[..., 1], st["csum"], st["csum_terms"])
    _check(what + " f", f, *ref.dual_f_ref(x["a"], rstat, cstat))
    want, terms = ref.dual_bwd_ref(x["a"], rstat, cstat, f, x["df"])
    runs = []
    for _ in range(2):
        srow, scol, da = _out(B * L, dev), _out(B * M, dev), _out(B * L * M, dev)
        _call("cpn_dual_softmax_bwd", a, rs, cs, fb, df, B, L, M, srow, scol, da)
        runs.append(_take(da, (B, L, M), what + " da"))
        _take(srow, (B, L), what + " srow"), _take(scol, (B, M), what + " scol")
    _check(what + " da", runs[0], want, terms)
    _same_bits(runs[0], runs[1], what + " da")


# ------------------------------------------------------------------------------------------------------------------
# K10: cross attention
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cross_forward(case, dev):
    """The forward kernel's outputs, ASSERTED against float64: (inputs on the host, device buffers of src_attn / trg_attn,
    their host copies)."""
    B, H, S, T, gain = case
    x = ref.make_cross_inputs(case)
    sa, ta = _out(B * S * H * 32, dev), _out(B * T * H * 32, dev)
    _call("cpn_cross_attention", x["corr"].to(dev), x["src_v"].to(dev), x["trg_v"].to(dev), B, H, S, T, 32, sa, ta)
    what = "cross " + ref.case_id(case)
    src, trg = _take(sa, (B, S, H, 32), what + " src_attn"), _take(ta, (B, T, H, 32), what + " trg_attn")
    f = ref.cross_fwd_ref(x["corr"], x["src_v"], x["trg_v"])
    _check(what + " src_attn", src, f["src_attn"], f["src_attn_terms"])
    _check(what + " trg_attn", trg, f["trg_attn"], f["trg_attn_terms"])
    return x, sa, ta, src, trg


@pytest.mark.parametrize("variant", ref.CROSS_VARIANTS)
@pytest.mark.parametrize("case", ref.CROSS_CASES, ids=ref.case_id)
def test_cross_attention_against_float64(case, variant, dev):
    """src_attn / trg_attn against float64; dcorr, dsrc_v, dtrg_v against the float64 VJP formed with the kernel's own
    src_attn / trg_attn - with both gradients, and with either one all zeros (what _CrossAttentionFn passes for a missing one)."""
    B, H, S, T, gain = case
    x, sa, ta, src, trg = _cross_forward(case, dev)
    g1 = torch.zeros_like(x["g_src"]) if variant == "g_src=0" else x["g_src"]
    g2 = torch.zeros_like(x["g_trg"]) if variant == "g_trg=0" else x["g_trg"]
    want = ref.cross_bwd_ref(x["corr"], x["src_v"], x["trg_v"], src, trg, g1, g2)
    d = [t.to(dev) for t in (x["corr"], x["src_v"], x["trg_v"], g1, g2)]
    what = f"cross {variant} {ref.case_id(case)}"
    nscr = _lib().cpn_cross_attention_bwd_scratch(B, H, S, T)
    runs = []
    for _ in range(2):
        scr, dc, dsv, dtv = _out(nscr, dev), _out(B * H * S * T, dev), _out(B * S * H * 32, dev), _out(B * T * H * 32, dev)
        _call("cpn_cross_attention_bwd", d[0], d[1], d[2], sa, ta, d[3], d[4], B, H, S, T, 32, scr, dc, dsv, dtv)
        runs.append((_take(dc, (B, H, S, T), what + " dcorr"), _take(dsv, (B, S, H, 32), what + " dsrc_v"),
                     _take(dtv, (B, T, H, 32), what + " dtrg_v")))
        _take(scr, (nscr,), what + " scratch")
    for name, got, again in zip(("dcorr", "dsrc_v", "dtrg_v"), *runs):
        _check(f"{what} {name}", got, want[name], want[name + "_terms"])
        _same_bits(got, again, f"{what} {name}")


# ------------------------------------------------------------------------------------------------------------------
# K9: linear attention
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _linear_inputs(case):
    return ref.make_linear_inputs(case)


def _run_linear(case, nsplit, dev, what, backward=True):
    """-> out, (dq, dk, dv) of one forward and one backward call with `nsplit` splits."""
    B, L, H, Dv, cm, _, gain = case
    x = _linear_inputs(case)
    q, k, v, g = (x[n].to(dev) for n in ("q", "k", "v", "dout"))
    vshape = (B, H, Dv, L) if cm else (B, L, H, Dv)
    nf = _lib().cpn_linear_attention_scratch(B, H, Dv, nsplit)
    scr, out = _out(nf, dev), _out(B * L * H * Dv, dev)
    _call("cpn_linear_attention", q, k, v, B, L, H, Dv, cm, 1e-6, nsplit, scr, out)
    res = _take(out, vshape, what + " out")
    _guard_ok(scr.cpu(), what + " scratch")
    if not backward:
        return res, None
    nb = _lib().cpn_linear_attention_bwd_scratch(B, L, H, Dv, nsplit)
    scr, dq, dk, dv = _out(nb, dev), _out(B * L * H * 32, dev), _out(B * L * H * 32, dev), _out(B * L * H * Dv, dev)
    _call("cpn_linear_attention_bwd", q, k, v, g, B, L, H, Dv, cm, 1e-6, nsplit, scr, dq, dk, dv)
    grads = (_take(dq, (B, L, H, 32), what + " dq"), _take(dk, (B, L, H, 32), what + " dk"), _take(dv, vshape, what + " dv"))
    _guard_ok(scr.cpu(), what + " scratch")
    return res, grads


@pytest.mark.parametrize("case", ref.LINEAR_CASES, ids=ref.case_id)
def test_linear_attention_against_float64(case, dev):
    """out, then dq, dk, dv against the float64 statement of the VJP; q and k hold exact zeros (phi' at 0)."""
    B, L, H, Dv, cm, nsplit, gain = case
    x = _linear_inputs(case)
    what = "linear " + ref.case_id(case)
    out, grads = _run_linear(case, nsplit, dev, what)
    _check(what + " out", out, *ref.linear_fwd_ref(x["q"], x["k"], x["v"], cm, nsplit))
    want = ref.linear_bwd_ref(x["q"], x["k"], x["v"], x["dout"], cm, nsplit)
    _, again = _run_linear(case, nsplit, dev, what)
    for name, got, rerun in zip(("dq", "dk", "dv"), grads, again):
        _check(f"{what} {name}", got, want[name], want[name + "_terms"])
        _same_bits(got, rerun, f"{what} {name}")


@pytest.mark.parametrize("case,other", ref.LINEAR_NSPLIT_PAIRS, ids=lambda p: ref.case_id(p) if isinstance(p, tuple) else f"vs{p}")
def test_linear_attention_nsplit_changes_nothing_beyond_the_bound(case, other, dev):
    """The same arguments with another nsplit: each result inside its own bound, so the two differ by at most the two bounds."""
    B, L, H, Dv, cm, nsplit, gain = case
    x = _linear_inputs(case)
    res = {}
    for n in (nsplit, other):
        what = f"linear {ref.case_id(case)} nsplit={n}"
        out, grads = _run_linear(case, n, dev, what)
        fw, ft = ref.linear_fwd_ref(x["q"], x["k"], x["v"], cm, n)
        _check(what + " out", out, fw, ft)
        want = ref.linear_bwd_ref(x["q"], x["k"], x["v"], x["dout"], cm, n)
        res[n] = {"out": (out, ref.total(ft))}
        for name, got in zip(("dq", "dk", "dv"), grads):
            _check(f"{what} {name}", got, want[name], want[name + "_terms"])
            res[n][name] = (got, ref.total(want[name + "_terms"]))
    for name in ("out", "dq", "dk", "dv"):
        (a, ba), (b, bb) = res[nsplit][name], res[other][name]
        assert bool(((a.double() - b.double()).abs() <= ba + bb).all()), f"{name}: nsplit {nsplit} and {other} differ beyond the bounds"


# ------------------------------------------------------------------------------------------------------------------
# GroupNorm + ReLU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.GN_CASES, ids=ref.case_id)
def test_gn_relu_against_float64(case, dev):
    """out of cpn_gn_relu (no residual: what training does) against float64, then dy, dgn_w, dgn_b with that out as the mask.
    The statistics are float64 sums of the synthetic y.  Two runs of the backward are NOT compared bit for bit: its per-sample
    and per-channel sums meet in float64 atomicAdd, whose order varies; both runs must be inside the bound."""
    B, C, npos, offset = case
    x = ref.make_gn_inputs(case)
    sums = ref.gn_moments(x["y"])[0]
    nst = _lib().cpn_gn_stats_doubles(B, C, npos)
    stats = torch.zeros(nst + GUARD, dtype=torch.float64, device=dev)
    stats[nst:] = 7.0
    stats[:2 * B] = sums.reshape(-1).to(dev)
    y, w, b, dout = (x[n].to(dev) for n in ("y", "gn_w", "gn_b", "dout"))
    ob = _out(B * C * npos, dev)
    _call("cpn_gn_relu", y, stats, w, b, 0, 1e-5, B, C, npos, ob)
    what = "gn " + ref.case_id(case)
    out = _take(ob, (B, C, npos), what + " out")
    _check(what + " out", out, *ref.gn_fwd_ref(x["y"], x["gn_w"], x["gn_b"]))
    if offset:
        assert abs(float(x["y"].mean())) > 4 * float(x["y"].std())
    want = ref.gn_bwd_ref(x["y"], out, x["dout"], x["gn_w"])
    for run in range(2):
        red = torch.zeros(2 * B + 2 * C + GUARD, dtype=torch.float64, device=dev)
        red[2 * B + 2 * C:] = 7.0
        dy, dw, db = _out(B * C * npos, dev), _out(C, dev), _out(C, dev)
        _call("cpn_gn_relu_bwd", y, ob, dout, stats, w, 1e-5, B, C, npos, red, dy, dw, db)
        got = (_take(dy, (B, C, npos), what + " dy"), _take(dw, (C,), what + " dgn_w"), _take(db, (C,), what + " dgn_b"))
        _guard_ok(red.cpu(), what + " red")
        for name, t in zip(("dy", "dgn_w", "dgn_b"), got):
            _check(f"{what} run {run} {name}", t, want[name], want[name + "_terms"])
    _guard_ok(stats.cpu(), what + " stats")


# ------------------------------------------------------------------------------------------------------------------
# Conv4d data gradient
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.DGRAD_CASES, ids=ref.case_id)
def test_conv4d_dgrad_against_float64(case, dev):
    """Both dispatch arms (the fp32-MFMA form with one and two channel tiles; the VALU form with 4 and 8 channels per thread
    where Ws is no power of two and the positions no multiple of 64) against the float64 transpose of the layer's two
    separable branches: gam(18 Cout) on sum |w| |dy|."""
    B, Co, Ci, Hq, Wq, Hs, Ws = case
    x = ref.make_dgrad_inputs(case)
    want, terms = ref.conv4d_dgrad_ref(x["dy"], x["wq"], x["ws"])
    dy, wq, ws = (x[n].to(dev) for n in ("dy", "wq", "ws"))
    what = "dgrad " + ref.case_id(case)
    runs = []
    for _ in range(2):
        dx = _out(B * Ci * Hq * Wq * Hs * Ws, dev)
        _call("cpn_conv4d_dgrad", dy, wq, ws, B, Co, Ci, Hq, Wq, Hs, Ws, dx)
        runs.append(_take(dx, (B, Ci, Hq, Wq, Hs, Ws), what))
    _check(what, runs[0], want, terms)
    _same_bits(runs[0], runs[1], what)


# ------------------------------------------------------------------------------------------------------------------
# row normalisation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.L2_CASES, ids=ref.case_id)
def test_l2norm_rows_bwd_against_float64(case, dev):
    """y is what cpn_correlation wrote into src_n (C % 16 == 0; checked against float64 first) or the fp32 quotient formed on
    the host; dx against the float64 VJP on that y.  Rows with |x| ~ 1e-4 (eps is a tenth of the norm) and a row of zeros."""
    rows, C, kind = case
    x = ref.make_l2_inputs(case)
    xd, gd = x["x"].to(dev), x["dy"].to(dev)
    what = "l2norm " + ref.case_id(case)
    if C % 16 == 0:
        sn, tn, corr = _out(rows * C, dev), _out(rows * C, dev), _out(rows * rows, dev)
        _call("cpn_correlation", xd, xd, 1, rows, C, 1e-5, sn, tn, corr)
        y = _take(sn, (rows, C), what + " src_n")
        _take(tn, (rows, C), what + " trg_n"), _take(corr, (rows, rows), what + " corr")
        _check(what + " src_n", y, *ref.l2norm_fwd_ref(x["x"]))
        yd = sn
    else:
        y = x["x"] / (x["x"].norm(dim=1, keepdim=True) + torch.tensor(1e-5, dtype=F32))
        yd = y.to(dev)
    want, terms = ref.l2norm_bwd_ref(x["x"], y, x["dy"])
    runs = []
    for _ in range(2):
        dx = _out(rows * C, dev)
        _call("cpn_l2norm_rows_bwd", xd, yd, gd, rows, C, 1e-5, dx)
        runs.append(_take(dx, (rows, C), what + " dx"))
    _check(what + " dx", runs[0], want, terms)
    _same_bits(runs[0], runs[1], what + " dx")
    if kind == "zero":
        assert bool((x["x"][1] == 0).all()) and bool((y[1] == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# pair transpose
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.TRANSPOSE_CASES, ids=ref.case_id)
def test_transpose_pairs_is_a_copy(case, dev):
    """Bit-equal to permute(0, 2, 1).contiguous(), nothing written behind y."""
    N, P, Q = case
    x = torch.randn(N, P, Q, generator=torch.Generator().manual_seed(N * P + Q))
    x.view(-1)[::7] = -0.0
    y = _out(N * P * Q, dev)
    _call("cpn_transpose_pairs", x.to(dev), N, P, Q, y)
    got = _take(y, (N, Q, P), "transpose " + ref.case_id(case))
    _same_bits(got, x.permute(0, 2, 1).contiguous(), "transpose")
