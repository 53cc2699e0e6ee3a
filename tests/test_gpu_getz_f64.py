"""The fp32 kernels get_z runs only at inference - cpn_correlation, cpn_resize_bilinear_ac(_adjoint), cpn_corr_mean3,
cpn_qk_assemble, cpn_cost_volume_attention, cpn_pose_positional, cpn_pose_gemv, cpn_pose_tail - each called on its raw entry
and held, element by element, to its float64 reference and derived bound (tests/getz_fwd_ref.py; pinned and calibrated on the
CPU by tests/test_getz_fwd_ref.py).  The shapes are the smallest that reach every dispatch arm and every ragged path; which
arm a case takes is asserted from the dispatch rule.  No element is left out of any comparison; every output and every scratch
buffer starts as NaN and has GUARD elements behind it, which must come back intact; every call is made twice and gives the
same bits.  The correlation's GEMM is checked on the kernel's OWN normalised rows, after those were checked themselves.

max err/bound of the first run on an MI355X, the worst over the cases of each kernel, with the terms that make up the bound at
that element.  The bounds are not tuned to these figures; the CPU emulation of tests/test_getz_fwd_ref.py shows the same ones
(to two digits, or exactly where the emulation follows the kernel's summation order) wherever a figure is above 0.1.
  cpn_correlation               src_n / trg_n 0.344 (norm 100 %; C = 48), corr 0.336 (chain 100 %; tile-64, K = 16); by arm:
                                NT = 2 0.157, NT = 8 0.321, tile-64 0.336; adjacent and separate buffers gave equal bits
  cpn_resize_bilinear_ac        0.455 (blend 100 %; 16 -> 64)        its adjoint 0.112 (9 x 7 <- 4 x 3); the identity a bit copy
  cpn_corr_mean3                0.293 per-thread kernel (43, 45 -> 46), 0.222 LDS kernel; 0.375 on the 1024 pairs of the
                                both-arms test (sum 84 %, blend 16 %), where the two kernels gave equal bits on 65 535 pairs
  cpn_qk_assemble               q 0.687, k 0.649 (sum 87 %, blend 9 %, frac 5 %; fs = 32)
  cpn_cost_volume_attention     0.053 (kd 32 %, qd 32 %, dot 36 %; fs = 7, hs = 3, Dv = 300); hs == 1: 0.032
                                the stock-op training form 0.045
  cpn_pose_positional           0.181 (n = 64)
  cpn_pose_gemv                 0.151 (K / 4 = 40 in 64 chunks: chunks 40 .. 63 exact zeros); the product's K 0.002
  cpn_pose_tail                 0.023 (dense 100 %; the degenerate rotation, nsplit = 0), nsplit = 8 0.017; bottom row exact
The attention, the gemv at the product's K and the pose tail sit far inside: their bounds charge every addition of chains of
tens to hundreds at full u on sums of positive terms, and the tail carries each layer's worst case through the next ones.
Before the fix of this change, cva_kd_kernel's gather window for hs == 1 ended at token 2 whatever fs: run once on that kernel,
the hs == 1 cases gave err/bound 70 009 and 71 344 (fs = 4: one token of four dropped, got 2.6385 for 3.7227) and 124 552 and
125 944 (fs = 9), the figures the CPU emulation of that window predicts to the digit; every other case passed there too (for
hs >= 2 the fix leaves the window as it was: test_cva_reference asserts that the two windows give equal bits).
"""
import ctypes

import pytest
import torch

from tests import getz_fwd_ref as ref
from tests.test_gpu_ufc_f64 import GUARD, _lib, _out, _same_bits, _st, _take

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def call(name, *args):
    """An entry point with tensors passed as their device pointers; the stream is passed by the caller, so that every site
    shows the entry's full argument list (tests/test_binding.py counts it)."""
    from coponerf_amd import _hip
    _hip.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def _check(what, got, want, terms):
    return ref.report(what, got, want, terms)


# ------------------------------------------------------------------------------------------------------------------
# correlation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CORR_CASES, ids=ref.case_id)
def test_correlation_against_float64(case, dev):
    """cpn_correlation picks its GEMM by shape: the 64 x 64-per-wave kernel when L % 128 == 0 and B (L / 128)^2 >= 512; else
    gemm_nt_f32_kernel<8> when B ceil(L / 128) ceil(L / 64) >= 512; else gemm_nt_f32_kernel<2> - the arm of every case is
    asserted from that rule, so that a change of the thresholds cannot quietly move a case off its arm.  Within the two
    gemm_nt arms: (2, 37, 16) has a ragged M (rows clamped), N & 3 != 0 (scalar stores) and K = 16 (no loop iteration);
    (1, 100, 48) vector stores next to a dropped column tile and the odd K / 16 tail step; (86, 130, 16) the same ragged paths at
    NT = 8.  Each case runs with src_n / trg_n (and src / trg) as adjacent halves of one buffer - one normalise launch - and as
    separate allocations - two; all runs give the same bits."""
    B, L, C = case
    assert ref.correlation_arm(B, L) == ref.CORR_ARMS[case]
    x = ref.make_corr_inputs(case)
    n = B * L * C
    what = "correlation " + ref.case_id(case)
    runs = []
    for layout in ("adjacent", "adjacent", "separate", "separate"):
        if layout == "adjacent":
            both = torch.cat((x["src"].reshape(-1), x["trg"].reshape(-1))).to(dev)
            src, trg = both[:n], both[n:]
            nbuf = _out(2 * n, dev)
            sn, tn = nbuf[:n], nbuf[n:2 * n]
            assert trg.data_ptr() == src.data_ptr() + 4 * n and tn.data_ptr() == sn.data_ptr() + 4 * n
        else:
            src, trg = x["src"].to(dev), x["trg"].to(dev)
            nbuf, tbuf = _out(n, dev), _out(n, dev)
            sn, tn = nbuf, tbuf
            assert tn.data_ptr() != sn.data_ptr() + 4 * n
        out = _out(B * L * L, dev)
        call("cpn_correlation", src, trg, B, L, C, 1e-5, sn, tn, out, _st())
        corr = _take(out, (B, L, L), what + " corr")
        if layout == "adjacent":
            norm = _take(nbuf, (2, B, L, C), what + " normalised")
            runs.append((norm[0], norm[1], corr))
        else:
            runs.append((_take(nbuf, (B, L, C), what + " src_n"), _take(tbuf, (B, L, C), what + " trg_n"), corr))
    for other in runs[1:]:
        for name, a, b in zip(("src_n", "trg_n", "corr"), runs[0], other):
            _same_bits(a, b, f"{what} {name}")
    src_n, trg_n, corr = runs[0]
    r = ref.correlation_ref(x["src"], x["trg"])
    _check(what + " src_n", src_n, r["src_n"], r["src_n_terms"])
    _check(what + " trg_n", trg_n, r["trg_n"], r["trg_n_terms"])
    _check(what + " corr", corr, *ref.correlation_gemm_ref(src_n, trg_n))
    if case == ref.CORR_ZERO_ROW:
        assert bool((x["src"][1, 3] == 0).all()) and bool((src_n[1, 3] == 0).all()) and bool((trg_n[0, 0] == 0).all())
        assert bool((corr[1, 3] == 0).all()) and bool((corr[0, :, 0] == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# bilinear resize and its adjoint
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.RESIZE_CASES, ids=ref.case_id)
def test_resize_and_adjoint_against_float64(case, dev):
    """cpn_resize_bilinear_ac on x (planes, h, w) and cpn_resize_bilinear_ac_adjoint on g (planes, H, W): one point, scale 0,
    one output pixel, h != w, the identity (a bit copy), downsampling (fine rows skip coarse ones: their adjoint rows are 0)."""
    planes, h, w, H, W = case
    x = ref.make_resize_inputs(case)
    xd, gd = x["x"].to(dev), x["g"].to(dev)
    what = "resize " + ref.case_id(case)
    up, adj = [], []
    for _ in range(2):
        o1, o2 = _out(planes * H * W, dev), _out(planes * h * w, dev)
        call("cpn_resize_bilinear_ac", xd, o1, planes, h, w, H, W, _st())
        call("cpn_resize_bilinear_ac_adjoint", gd, o2, planes, h, w, H, W, _st())
        up.append(_take(o1, (planes, H, W), what))
        adj.append(_take(o2, (planes, h, w), what + " adjoint"))
    _same_bits(up[0], up[1], what)
    _same_bits(adj[0], adj[1], what + " adjoint")
    _check(what, up[0], *ref.resize_ref(x["x"], H, W))
    _check(what + " adjoint", adj[0], *ref.resize_adjoint_ref(x["g"], h, w))
    if case == ref.RESIZE_IDENTITY:
        _same_bits(up[0], x["x"], what + ": the identity is a copy")
        _same_bits(adj[0], x["g"], what + " adjoint: the identity is a copy")


# ------------------------------------------------------------------------------------------------------------------
# final correlation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.MEAN3_CASES, ids=ref.case_id)
def test_corr_mean3_against_float64(case, dev):
    """cpn_corr_mean3 stages the coarse levels' tap planes in LDS while 4 (h0^2 + h1^2) floats fit in 60 KiB and B < 65536, and
    reads them per thread otherwise: (1, 43, 45, 46) is the smallest shape past that limit.  (1, 5, 7, 7): a level already at n."""
    B, h0, h1, n = case
    assert ref.corr_mean3_arm(B, h0, h1) == ref.MEAN3_ARMS[case]
    x = ref.make_mean3_inputs(case)
    c0, c1, c2 = (x[k].to(dev) for k in ("c0", "c1", "c2"))
    what = "mean3 " + ref.case_id(case)
    runs = []
    for _ in range(2):
        out = _out(B * n ** 4, dev)
        call("cpn_corr_mean3", c0, h0, c1, h1, c2, n, B, out, _st())
        runs.append(_take(out, (B, n, n, n, n), what))
    _same_bits(runs[0], runs[1], what)
    _check(what, runs[0], *ref.corr_mean3_ref(x["c0"], x["c1"], x["c2"]))


def test_corr_mean3_arms_give_equal_bits(dev):
    """Both kernels on the same pairs: B = 65536 is past the LDS kernel's grid and takes the per-thread kernel whatever the
    shape; the first 65535 pairs of the same buffers take the LDS kernel."""
    B, h0, h1, n = ref.MEAN3_BOTH
    assert ref.corr_mean3_arm(B, h0, h1) == "thread" and ref.corr_mean3_arm(B - 1, h0, h1) == "planes"
    x = ref.make_mean3_inputs((1024, h0, h1, n))
    c0, c1, c2 = (x[k].to(dev).repeat(B // 1024, 1, 1, 1, 1).contiguous() for k in ("c0", "c1", "c2"))
    per = n ** 4
    thread, planes = _out(B * per, dev), _out((B - 1) * per, dev)
    call("cpn_corr_mean3", c0, h0, c1, h1, c2, n, B, thread, _st())
    call("cpn_corr_mean3", c0, h0, c1, h1, c2, n, B - 1, planes, _st())
    torch.cuda.synchronize()
    assert bool((thread[-GUARD:] == 7.0).all()) and bool((planes[-GUARD:] == 7.0).all())
    assert bool(torch.isfinite(thread[:-GUARD]).all())
    assert torch.equal(thread[:(B - 1) * per].view(torch.int32), planes[:-GUARD].view(torch.int32))
    first = thread[:1024 * per].cpu().view(1024, n, n, n, n)
    _check("mean3 both arms", first, *ref.corr_mean3_ref(x["c0"], x["c1"], x["c2"]))


# ------------------------------------------------------------------------------------------------------------------
# q / k assembly
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.QK_CASES, ids=ref.case_id)
def test_qk_assemble_against_float64(case, dev):
    """q and k each receive exactly their half of the 2 d channels (each buffer is NaN before and guarded behind), pos is indexed
    c % dim in both halves; h != w with a partly dead last workgroup, fs < h, the identity resize."""
    B, fs, h, w, nhead, dim = case
    x = ref.make_qk_inputs(case)
    lin, low, pos = (x[k].to(dev) for k in ("lin", "low", "pos"))
    L, d = fs * fs, nhead * dim
    what = "qk " + ref.case_id(case)
    runs = []
    for _ in range(2):
        q, k = _out(B * L * d, dev), _out(B * L * d, dev)
        call("cpn_qk_assemble", lin, low, pos, B, fs, h, w, nhead, dim, q, k, _st())
        runs.append((_take(q, (B, L, d), what + " q"), _take(k, (B, L, d), what + " k")))
    qw, kw, qt, kt = ref.qk_assemble_ref(x["lin"], x["low"], x["pos"], fs, h, w, nhead, dim)
    _same_bits(runs[0][0], runs[1][0], what + " q")
    _same_bits(runs[0][1], runs[1][1], what + " k")
    _check(what + " q", runs[0][0], qw, qt)
    _check(what + " k", runs[0][1], kw, kt)


# ------------------------------------------------------------------------------------------------------------------
# cost-volume attention
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_res", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("case", ref.CVA_CASES, ids=ref.case_id)
def test_cost_volume_attention_against_float64(case, with_res, dev):
    """cpn_cost_volume_attention against the reference's order in float64.  hs == 1 with fs >= 4: every token lands on the one
    low-resolution position and the Kd gather must span the whole axis (before the fix it ended at token 2); fs == hs with
    P = 25 (neither the 16- nor the 8-position blocks are full); a non-integer ratio with Dv = 300 (two passes of 256 threads)."""
    B, fs, H, hs, Dv = case
    x = ref.make_cva_inputs(case)
    q, k, v, res = (x[n].to(dev) for n in ("q", "k", "v", "res"))
    L, P = fs * fs, hs * hs
    what = f"cva {ref.case_id(case)} {'residual' if with_res else 'plain'}"
    nscr = _lib().cpn_cost_volume_attention_scratch(B, L, H, P, Dv)
    runs = []
    for _ in range(2):
        scr, out = _out(nscr, dev), _out(B * H * P * Dv, dev)
        call("cpn_cost_volume_attention", q, k, v, res if with_res else 0, B, fs, H, hs, Dv, 1e-6, scr, out, _st())
        runs.append(_take(out, (B, H, P, Dv), what))
        _take(scr, (nscr,), what + " scratch")
    _same_bits(runs[0], runs[1], what)
    _check(what, runs[0], *ref.cva_ref(x["q"], x["k"], x["v"], x["res"] if with_res else None, fs))


@pytest.mark.parametrize("case", ref.CVA_ONE_POINT + [(1, 7, 2, 3, 300)], ids=ref.case_id)
def test_cost_volume_attention_stock_form_against_float64(case, dev):
    """The training form (cost_volume_attention_torch: stock ops around the resize kernel and its adjoint) against the same
    reference, hs == 1 included: the adjoint always gathered over the whole axis there."""
    from coponerf_amd.ufc_ops import HipOps, cost_volume_attention_torch
    B, fs, H, hs, Dv = case
    x = ref.make_cva_inputs(case)
    vol = lambda t: t.reshape(B, H, hs, hs, Dv, 1).to(dev)
    with torch.no_grad():
        got = cost_volume_attention_torch(HipOps(), x["q"].to(dev), x["k"].to(dev), vol(x["v"]), fs, vol(x["res"]), 1e-6)
    torch.cuda.synchronize()
    _check("cva stock form " + ref.case_id(case), got.cpu().reshape(B, H, hs * hs, Dv),
           *ref.cva_ref(x["q"], x["k"], x["v"], x["res"], fs, stock=True))


# ------------------------------------------------------------------------------------------------------------------
# pose head
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.POSPOS_CASES, ids=ref.case_id)
def test_pose_positional_against_float64(case, dev):
    """fx != fy, cx != cy; view 1's intrinsics differ from view 0's and must not influence a bit."""
    B, V, n = case
    x = ref.make_pospos_inputs(case)
    lin = x["lin"].to(dev)
    other = x["K"].clone()
    other[:, 1:] = other[:, 1:] * 1.5
    what = "positional " + ref.case_id(case)
    runs = []
    for K in (x["K"], x["K"], other):
        out = _out(B * n * n * 6, dev)
        call("cpn_pose_positional", K.to(dev), B, V, x["H"], lin, n, out, _st())
        runs.append(_take(out, (B, n * n, 6), what))
    _same_bits(runs[0], runs[1], what)
    _same_bits(runs[0], runs[2], what + ": view 1 changed")
    _check(what, runs[0], *ref.pose_positional_ref(x["K"], x["H"], x["lin"]))


@pytest.mark.parametrize("case", ref.GEMV_CASES, ids=ref.case_id)
def test_pose_gemv_against_float64(case, dev):
    """The partials per (row, output, chunk) under the kernel's chunking rule, for 1, 2, 3 and 4 rows: a ragged last chunk
    (K / 4 = 257 in 8 chunks of 33), chunks past the end (K / 4 = 40 in 64 chunks: 40 .. 63 are exact zeros), the product's K."""
    B, K, O, nsplit = case
    x = ref.make_gemv_inputs(case)
    xd, wd = x["x"].to(dev), x["W"].to(dev)
    what = "gemv " + ref.case_id(case)
    runs = []
    for _ in range(2):
        part = _out(B * O * nsplit, dev)
        call("cpn_pose_gemv", xd, wd, B, K, O, nsplit, part, _st())
        runs.append(_take(part, (B, O, nsplit), what))
    _same_bits(runs[0], runs[1], what)
    _check(what, runs[0], *ref.pose_gemv_ref(x["x"], x["W"], nsplit))
    for c, (lo, hi) in enumerate(ref.gemv_chunks(K, nsplit)):
        if lo == hi:
            assert bool((runs[0][:, :, c] == 0).all()), f"{what}: empty chunk {c}"


@pytest.mark.parametrize("case", ref.TAIL_CASES, ids=ref.case_id)
def test_pose_tail_against_float64(case, dev):
    """Both arms of cpn_pose_tail - nsplit = 8 sums cpn_pose_gemv's chunk partials in chunk order and adds the bias, nsplit = 0
    takes a finished first layer, which is what every batch above 4 runs - at B = 1, 3, 6: five dense layers, the 6-D
    rotation, the 4 x 4 assembly.  degenerate: a1 = 0 exactly, so b1 = 0, b3 = 0 and b2 = a2 / |a2|."""
    B, nsplit, kind = case
    x = ref.make_tail_inputs(case)
    w = [t.to(dev).contiguous() for t in x["weights"]]
    assert [tuple(t.shape) for t in w] == ref.TAIL_SHAPES
    arr = (ctypes.c_void_p * len(w))(*[t.data_ptr() for t in w])
    h, bias0 = x["h"].to(dev), x["bias0"].to(dev)
    what = "tail " + ref.case_id(case)
    runs = []
    for _ in range(2):
        out = _out(B * 16, dev)
        call("cpn_pose_tail", h, nsplit, bias0 if nsplit else 0, arr, B, out, _st())
        runs.append(_take(out, (B, 4, 4), what))
    _same_bits(runs[0], runs[1], what)
    _check(what, runs[0], *ref.pose_tail_ref(x["h"], nsplit, x["bias0"], x["weights"]))
    _same_bits(runs[0][:, 3].contiguous(), torch.tensor([0., 0., 0., 1.]).expand(B, 4).contiguous(), what + ": bottom row")
    if kind == "degenerate":
        assert bool((runs[0][:, 0, :3] == 0).all()) and bool((runs[0][:, 2, :3] == 0).all()), what


# ------------------------------------------------------------------------------------------------------------------
# what the entries reject, before any launch
# ------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_are_status_codes():
    lib = _lib()
    p = 256                                                       # a non-null, 16-byte aligned "pointer" that is never read
    assert lib.cpn_correlation(None, p, 1, 4, 16, 1e-5, p, p, p, None) == -1
    assert lib.cpn_correlation(p, p, 1, 4, 24, 1e-5, p, p, p, None) == -2 and b"multiple of 16" in lib.cpn_last_error()
    assert lib.cpn_resize_bilinear_ac(None, p, 1, 2, 2, 4, 4, None) == -1
    assert lib.cpn_resize_bilinear_ac(p, p, 1, 0, 2, 4, 4, None) == -2
    assert lib.cpn_corr_mean3(p, 16, p, 32, p, 129, 1, p, None) == -2          # n > 128
    assert lib.cpn_corr_mean3(p, 16, p, 65, p, 64, 1, p, None) == -2           # h1 > n
    assert lib.cpn_corr_mean3(p, 16, p, 32, p, 64, 1, None, None) == -1
    assert lib.cpn_qk_assemble(p, p, None, 1, 4, 2, 2, 1, 4, p, p, None) == -1
    assert lib.cpn_qk_assemble(p, p, p, 1, 0, 2, 2, 1, 4, p, p, None) == -2
    assert lib.cpn_cost_volume_attention(p, p, p, None, 1, 3, 1, 4, 8, 1e-6, p, p, None) == -2      # fs < hs
    assert b"fs=3 hs=4" in lib.cpn_last_error()
    assert lib.cpn_cost_volume_attention(p, p, p, None, 1, 4, 1, 4, 8, 1e-6, None, p, None) == -1
    assert lib.cpn_pose_positional(None, 1, 2, 256.0, p, 4, p, None) == 1
    assert lib.cpn_pose_gemv(p, p, 1, 130, 4, 8, p, None) == 1 and b"K=130" in lib.cpn_last_error()  # K % 4 != 0
    assert lib.cpn_pose_gemv(p, p, 5, 128, 4, 8, p, None) == 1 and b"B=5" in lib.cpn_last_error()
    assert lib.cpn_pose_gemv(p, None, 1, 128, 4, 8, p, None) == 1
    arr = (ctypes.c_void_p * 16)(*([p] * 16))
    assert lib.cpn_pose_tail(None, 0, None, arr, 1, p, None) == 1
    assert lib.cpn_pose_tail(p, 8, None, arr, 1, p, None) == 1                 # chunk partials need the bias
    arr[7] = None
    assert lib.cpn_pose_tail(p, 0, None, arr, 1, p, None) == 1 and b"weight 7" in lib.cpn_last_error()
