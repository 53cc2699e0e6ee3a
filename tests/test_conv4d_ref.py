"""The float64 references of tests/conv4d_ref.py checked on the CPU, so that tests/test_gpu_conv4d_f64.py compares with
something that was itself checked:
  pin         every reference against an independent float64 evaluation - the Conv4d forward against oracle.ufc_ref.conv4d, the
              strided backward and all weight gradients against float64 autograd through that oracle and through F.conv2d, the
              token DWConv against the transpose / grouped conv2d / transpose form with torch's GELU - to 1e-12 of the
              element's sum of absolute values;
  routing     the written-out routing of the max-pool against the CPU library's, on the case with ties;
  calibrate   an fp32 CPU evaluation of every operation (the oracle in fp32, fp32 autograd) stays inside every bound on every
              case the GPU test uses; the ratios are printed;
  sensitivity seeded defects of the kinds the bounds exist for leave them, on every case of the class they concern;
  replay      stats_replay is the documented order of additions."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ufc_ref as oracle
from tests import conv4d_ref as ref

F32, F64 = torch.float32, torch.float64

FWD_SHAPES = list(dict.fromkeys(fc[1] for fc in ref.FWD_CASES))                 # the unaligned variants share a shape
PARAMS = ("wq", "bq", "ws", "bs")


def _mag(terms, n):
    """The element's sum of absolute values back out of its gam(n) term."""
    return terms["chain"] / ref.gam(n)


def _pinned(what, got, want, mag):
    err = (got - want).abs()
    worst = float((err / mag.expand_as(err).clamp_min(1e-300)).max())
    assert bool((err <= 1e-12 * mag).all()), (what, worst)


def _inside(what, got, want, terms):
    return ref.report(what, got, want, terms)


def _outside(what, got, want, terms):
    r = float(ref.ratio(got, want, ref.total(terms).expand_as(want)).max())
    print(f"{what}: worst err/bound {r:.3g}")
    assert r > 1.0, what


@functools.lru_cache(maxsize=None)
def _fwd(case, variant=""):
    x = ref.make_conv4d_inputs(case, variant)
    k, s, p = case[7:]
    return x, ref.conv4d_fwd_ref(*(x[n] for n in ("x",) + PARAMS), k, s, p)


@functools.lru_cache(maxsize=None)
def _sbwd(sc):
    case, variant = sc
    x = ref.make_conv4d_inputs(case, variant)
    k, s, p = case[7:]
    return x, ref.strided_bwd_ref(x["x"], x["dy"], x["wq"], x["ws"], k, s, p)


def _oracle_grads(x, case, dtype):
    """dx, gwq, gws, gb of the layer by autograd through the oracle in `dtype`."""
    k, s, p = case[7:]
    t = {n: x[n].to(dtype).clone().requires_grad_(True) for n in ("x",) + PARAMS}
    y = oracle.conv4d(t["x"], t["wq"], t["bq"], t["ws"], t["bs"], k, s, p)
    (y * x["dy"].to(dtype)).sum().backward()
    return {"dx": t["x"].grad, "gwq": t["wq"].grad, "gws": t["ws"].grad, "gb": t["bq"].grad}


def _planes_autograd(x, dtype):
    B, Ci, G, H, W = x["x"].shape
    fold = lambda t: t.to(dtype).permute(0, 2, 1, 3, 4).reshape(B * G, -1, H, W)
    w = torch.zeros(x["dy"].shape[1], Ci, 3, 3, dtype=dtype, requires_grad=True)
    b = torch.zeros(x["dy"].shape[1], dtype=dtype, requires_grad=True)
    (F.conv2d(fold(x["x"]), w, b, padding=1) * fold(x["dy"])).sum().backward()
    return {"dw": w.grad, "db": b.grad}


def _dw_autograd(xn, dyn, dtype):
    """xn, dyn (N, C, H, W) -> dw (C, 3, 3), db (C), dx by autograd through the grouped conv2d."""
    C = xn.shape[1]
    w = torch.zeros(C, 1, 3, 3, dtype=dtype, requires_grad=True)
    b = torch.zeros(C, dtype=dtype, requires_grad=True)
    (F.conv2d(xn.to(dtype), w, b, padding=1, groups=C) * dyn.to(dtype)).sum().backward()
    return {"dw": w.grad.reshape(C, 3, 3), "db": b.grad}


def _tokens_library(x, w, bias, H, W, flip, dtype):
    """The reference's form: transpose to (B, C, H, W), grouped conv2d, transpose back; flip = 1: autograd's data gradient."""
    B, L, C = x.shape
    xn = x.to(dtype).reshape(B, H, W, C).permute(0, 3, 1, 2)
    w4 = w.to(dtype).reshape(C, 1, 3, 3)
    back = lambda t: t.permute(0, 2, 3, 1).reshape(B, L, C)
    if flip & 1:
        z = torch.zeros_like(xn).requires_grad_(True)
        (F.conv2d(z, w4, None, padding=1, groups=C) * xn).sum().backward()
        return back(z.grad)
    y = F.conv2d(xn, w4, bias.to(dtype), padding=1, groups=C)
    return back(F.gelu(y) if flip & 2 else y)


def _nchw(t, case):
    B, H, W, C = case
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------
# the case lists reach what they name
# ------------------------------------------------------------------------------------------------------------------
def test_every_arm_has_a_case_with_four_different_extents_and_its_odd_sizes():
    for arm in {fc[0] for fc in ref.FWD_CASES} - {"unaligned"}:               # (the unaligned pair ends in valu<4,true>)
        assert any(fc[0] == arm and len(set(fc[1][3:7])) == 4 for fc in ref.FWD_CASES), arm
    for sc in ref.SBWD_CASES:
        assert len(set(sc[0][3:7])) == 4 and sc[0][2] == 8 and sc[0][1] in (1, 2, 8), sc
    for family in ("generic", "pooled", "valu"):
        assert any(fc[0].startswith(family) and ref.npos_of(fc[1]) % 256 for fc in ref.FWD_CASES), family
    assert any(ref.launched_w(fc) > 256 for fc in ref.FWD_CASES)              # more partials than threads in gn_publish
    x = ref.make_conv4d_inputs(*ref.SBWD_TIES)["x"]
    assert float((x == 0).double().mean()) > 0.4 and x.unique().numel() < 12


# ------------------------------------------------------------------------------------------------------------------
# 1. pin
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_SHAPES, ids=ref.case_id)
def test_conv4d_forward_reference_is_the_oracle_in_float64(case):
    x, (want, terms) = _fwd(case)
    k, s, p = case[7:]
    y = oracle.conv4d(*(x[n].double() for n in ("x",) + PARAMS), k, s, p)
    assert want.shape[2:] == ref.out_dims(case)
    _pinned("y", want, y, _mag(terms, 2 * k * k * case[1] + 2))


@pytest.mark.parametrize("sc", ref.SBWD_CASES, ids=ref.sbwd_id)
def test_strided_backward_reference_is_float64_autograd_of_the_oracle(sc):
    case, variant = sc
    B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p = case
    x, want = _sbwd(sc)
    g = _oracle_grads(x, case, F64)
    n = B * ref.npos_of(case)
    for name, chain in (("dx", Co * k * k + 1), ("gwq", n), ("gws", n), ("gb", n)):
        _pinned(name, want[name], g[name], _mag(want[name + "_terms"], chain))


@pytest.mark.parametrize("case", ref.PLANES_CASES, ids=ref.case_id)
def test_wgrad_planes_reference_is_float64_autograd_of_conv2d(case):
    x = ref.make_planes_inputs(case)
    want, g = ref.wgrad_planes_ref(x["x"], x["dy"]), _planes_autograd(x, F64)
    n = case[0] * case[3] * case[4] * case[5]
    for name in ("dw", "db"):
        _pinned(name, want[name], g[name], _mag(want[name + "_terms"], n))


@pytest.mark.parametrize("case", ref.DW_WGRAD_CASES, ids=ref.case_id)
def test_dwconv_wgrad_reference_is_float64_autograd_of_conv2d(case):
    x = ref.make_dw_wgrad_inputs(case)
    want, g = ref.dwconv_wgrad_ref(x["x"], x["dy"]), _dw_autograd(x["x"], x["dy"], F64)
    for name in ("dw", "db"):
        _pinned(name, want[name], g[name], _mag(want[name + "_terms"], case[0] * case[2] * case[3]))


@pytest.mark.parametrize("case", ref.DW_TOKENS_WGRAD_CASES, ids=ref.case_id)
def test_dwconv_tokens_references_are_the_transposed_grouped_conv2d_in_float64(case):
    B, H, W, C = case
    x = ref.make_dw_tokens_inputs(case)
    plain = None
    for flip in ref.DW_FLIPS:
        bias = None if flip == 1 else x["bias"]
        src = x["dy"] if flip == 1 else x["x"]
        want, terms = ref.dwconv_tokens_ref(src, x["w"], bias, H, W, flip)
        if flip == 0:
            plain = _mag({"chain": terms["conv"]}, 10)
        mag = _mag({"chain": ref.dwconv_tokens_ref(src, x["w"], bias, H, W, flip & 1)[1]["conv"]}, 10)
        _pinned(f"flip {flip}", want, _tokens_library(src, x["w"], x["bias"], H, W, flip, F64), mag)
    assert plain is not None
    want = ref.dwconv_tokens_wgrad_ref(x["x"], x["dy"], H, W)
    g = _dw_autograd(_nchw(x["x"], case), _nchw(x["dy"], case), F64)
    _pinned("dw", want["dw"], g["dw"].reshape(C, 9), _mag(want["dw_terms"], B * H * W))
    _pinned("db", want["db"], g["db"], _mag(want["db_terms"], B * H * W))


# ------------------------------------------------------------------------------------------------------------------
# 2. routing
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ref.SBWD_CASES, ids=ref.sbwd_id)
def test_written_out_routing_against_the_cpu_library(sc):
    """include/coponerf_hip.h: a window's gradient goes to its FIRST maximum in scan order.  pool_last2 writes that out; the CPU
    library's max_pool2d backward is compared with it.  Should a library version route a tie elsewhere, the header's rule is
    the specification: the reference is held to it here window by window, and the difference is only reported."""
    case, variant = sc
    s = case[8]
    x = ref.make_conv4d_inputs(case, variant)["x"].double()
    for name, v in (("support", x), ("query", x.permute(0, 1, 4, 5, 2, 3))):
        pooled, routed = ref.pool_last2(v, s)
        H, W = v.shape[-2:]
        flat = v.reshape(-1, 1, H, W).clone().requires_grad_(True)
        lib = F.max_pool2d(flat, s, s, 0, ceil_mode=True)
        assert torch.equal(lib.detach().reshape(pooled.shape), pooled)
        lib.sum().backward()
        # the rule itself: one element per window, a maximum, and no element before it in scan order equals it
        win, sel = ref._windows(v, s), ref._windows(routed.double(), s) == 1
        assert bool((sel.sum(-1) == 1).all())
        first = sel.double().argmax(-1, keepdim=True)
        assert torch.equal(win.gather(-1, first).squeeze(-1), pooled)
        before = torch.arange(s * s).view(*([1] * (win.dim() - 1)), -1) < first
        assert not bool(((win == pooled.unsqueeze(-1)) & before).any())
        same = torch.equal(flat.grad.reshape(routed.shape) != 0, routed)
        print(f"{ref.sbwd_id(sc)} {name} windows: the CPU library routes {'as' if same else 'NOT as'} the header's rule")
    if variant == "ties":
        win = ref._windows(x, s)
        assert float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).double().mean()) > 0.3      # ties in a third of the windows


# ------------------------------------------------------------------------------------------------------------------
# 3. calibrate: fp32 evaluations stay inside the bounds
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_SHAPES, ids=ref.case_id)
def test_fp32_oracle_forward_and_its_statistics_are_inside_the_bounds(case):
    x, (want, terms) = _fwd(case)
    k, s, p = case[7:]
    y = oracle.conv4d(*(x[n] for n in ("x",) + PARAMS), k, s, p)
    _inside("y " + ref.case_id(case), y, want, terms)
    B, Co = case[0], case[2]
    for fc in (f for f in ref.FWD_CASES if f[1] == case):
        for scratch in ((True, False) if s > 1 else (True,)):
            W = ref.launched_w(fc, scratch)
            stats = ref.emu_stats(y.reshape(B, Co, -1), B, W, 3 * B + 2 * B * W + 6)
            assert ref.written_partials(stats, B) == W
            assert torch.equal(ref.stats_replay(stats, B, W).reshape(-1), stats[:2 * B])
            _inside(f"stats W={W}", stats[:2 * B].reshape(B, 2), *ref.gn_stats_ref(y))


@pytest.mark.parametrize("sc", ref.SBWD_CASES, ids=ref.sbwd_id)
def test_fp32_autograd_of_the_strided_layer_is_inside_the_bounds(sc):
    case, variant = sc
    x, want = _sbwd(sc)
    g = _oracle_grads(x, case, F32)
    for name in ("dx", "gwq", "gws", "gb"):
        _inside(f"{name} {ref.sbwd_id(sc)}", g[name], want[name], want[name + "_terms"])
    assert torch.equal(g["dx"] != 0, want["routed"])


@pytest.mark.parametrize("case", ref.PLANES_CASES, ids=ref.case_id)
def test_fp32_autograd_of_the_plane_weight_gradient_is_inside_the_bounds(case):
    x = ref.make_planes_inputs(case)
    want, g = ref.wgrad_planes_ref(x["x"], x["dy"]), _planes_autograd(x, F32)
    for name in ("dw", "db"):
        _inside(f"{name} {ref.case_id(case)}", g[name], want[name], want[name + "_terms"])


@pytest.mark.parametrize("case", ref.DW_WGRAD_CASES, ids=ref.case_id)
def test_fp32_autograd_of_the_dwconv_weight_gradient_is_inside_the_bounds(case):
    x = ref.make_dw_wgrad_inputs(case)
    want, g = ref.dwconv_wgrad_ref(x["x"], x["dy"]), _dw_autograd(x["x"], x["dy"], F32)
    for name in ("dw", "db"):
        _inside(f"{name} {ref.case_id(case)}", g[name], want[name], want[name + "_terms"])


@pytest.mark.parametrize("case", ref.DW_TOKENS_WGRAD_CASES, ids=ref.case_id)
def test_fp32_token_dwconv_is_inside_the_bounds(case):
    B, H, W, C = case
    x = ref.make_dw_tokens_inputs(case)
    for flip in ref.DW_FLIPS:
        bias = None if flip == 1 else x["bias"]
        src = x["dy"] if flip == 1 else x["x"]
        _inside(f"tokens flip {flip} {ref.case_id(case)}", _tokens_library(src, x["w"], x["bias"], H, W, flip, F32),
                *ref.dwconv_tokens_ref(src, x["w"], bias, H, W, flip))
    want = ref.dwconv_tokens_wgrad_ref(x["x"], x["dy"], H, W)
    g = _dw_autograd(_nchw(x["x"], case), _nchw(x["dy"], case), F32)
    _inside("tokens dw " + ref.case_id(case), g["dw"].reshape(C, 9), want["dw"], want["dw_terms"])
    _inside("tokens db " + ref.case_id(case), g["db"], want["db"], want["db_terms"])


# ------------------------------------------------------------------------------------------------------------------
# 4. sensitivity: seeded defects leave the bounds on every case of their class
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_SHAPES, ids=ref.case_id)
def test_seeded_defects_leave_the_forward_bound(case):
    x, (want, terms) = _fwd(case)
    B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p = case
    args = [x[n] for n in ("x",) + PARAMS]
    what = ref.case_id(case)
    _outside(what + ": one border tap dropped", ref.conv4d_fwd_ref(*args, k, s, p, drop=(0, 0))[0], want, terms)
    _outside(what + ": Hq and Wq swapped in the indexing", ref.conv4d_fwd_ref(*args, k, s, p, swap_q=True)[0], want, terms)
    _outside(what + ": bs omitted", ref.conv4d_fwd_ref(*args[:4], torch.zeros(Co), k, s, p)[0], want, terms)
    o = min(Co, 16) - 1
    moved = want.clone()
    moved[:, o] = want[:, o - 1]
    _outside(what + f": channel {o}, the last of a 16-channel tile, taken from its neighbour", moved, want, terms)
    if s > 1:
        _outside(what + ": a ragged window truncated one element early", ref.conv4d_fwd_ref(*args, k, s, p, trunc=True)[0], want, terms)


@pytest.mark.parametrize("sc", ref.SBWD_CASES, ids=ref.sbwd_id)
def test_seeded_defects_leave_the_strided_backward_bounds(sc):
    case, variant = sc
    k, s, p = case[7:]
    x, want = _sbwd(sc)
    bad = ref.strided_bwd_ref(x["x"], x["dy"], x["wq"], x["ws"], k, s, p, trunc=True)
    for name in ("dx", "gwq", "gws"):
        _outside(f"{ref.sbwd_id(sc)} {name}: a ragged window truncated one element early", bad[name], want[name], want[name + "_terms"])
    if variant == "ties":
        bad = ref.strided_bwd_ref(x["x"], x["dy"], x["wq"], x["ws"], k, s, p, last=True)
        _outside("ties dx: routed to the last maximum", bad["dx"], want["dx"], want["dx_terms"])
        assert not torch.equal(bad["routed"], want["routed"])


@pytest.mark.parametrize("fc", ref.FWD_CASES, ids=ref.fwd_id)
def test_a_workgroup_partial_left_out_leaves_the_statistics_bound(fc):
    arm, case, wmul, _ = fc
    x, (want, terms) = _fwd(case)
    B, Co = case[0], case[2]
    y = want.float()
    for scratch in ((True, False) if case[8] > 1 else (True,)):
        W = ref.launched_w(fc, scratch)
        stats = ref.emu_stats(y.reshape(B, Co, -1), B, W, 3 * B + 2 * B * W)
        for w in {0, W - 1}:
            bad = stats.clone()
            bad[3 * B + 2 * ((B - 1) * W + w):3 * B + 2 * ((B - 1) * W + w) + 2] = 0.0
            _outside(f"{ref.fwd_id(fc)} W={W}: partial {w} of the last sample left out", ref.stats_replay(bad, B, W),
                     *ref.gn_stats_ref(y))


# ------------------------------------------------------------------------------------------------------------------
# 5. replay
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 5, 256, 257, 625])
def test_stats_replay_is_the_documented_order(W):
    B = 2
    gen = torch.Generator().manual_seed(W)
    stats = torch.zeros(3 * B + 2 * B * W, dtype=F64)
    stats[3 * B:] = torch.randn(2 * B * W, generator=gen, dtype=F64) * 10.0 ** torch.randint(-3, 4, (2 * B * W,), generator=gen).double()
    got = ref.stats_replay(stats, B, W)
    for b in range(B):
        for q in range(2):
            part = [float(v) for v in stats[3 * B + 2 * b * W + q:3 * B + 2 * (b + 1) * W:2]]
            tree = []
            for t in range(256):
                a = 0.0
                for w in range(t, W, 256):
                    a += part[w]
                tree.append(a)
            n = 128
            while n > 0:
                for t in range(n):
                    tree[t] += tree[t + n]
                n //= 2
            assert float(got[b, q]) == tree[0]
