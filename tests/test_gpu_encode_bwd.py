"""The kernels of the first encoder layer's table-form backward (EncodeFn._backward_tables: csrc/encode_bwd.hip and the
level-3 scatter of csrc/backward.hip), each against its float64 adjoint (tests/encode_bwd_ref.py), and the whole node
against float64 autograd under the GPU's own ReLU mask.  Every tolerance is derived beside its assertion or in the
helper that forms it; no element is left out of any comparison."""
import math

import pytest
import torch

from tests import encode_bwd_ref as ref

pytestmark = pytest.mark.gpu

V = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


# (H, W, B, R, S, ray0, nrays): the ragged ranges of the forward test at 32 x 32, one of them again at 64 x 64 and on a
# non-square image, and the pile-up shape
CASES = [(32, 32) + c for c in ref.RAGGED] + [(64, 64, 2, 7, 9, 3, 9), (32, 64, 2, 7, 9, 3, 9), (64, 64) + ref.PILEUP]
IDS = ["%dx%d-B%d-R%d-S%d-ray%d+%d" % c for c in CASES]


def make_case(H, W, B, R, S, ray0, nrays):
    """Coordinates of a case (random + the hostile set, or the pile-up construction), its row table and row coordinates."""
    gen = torch.Generator().manual_seed(H * 7 + W + 1000 * B + 10 * R + S)
    N = B * V
    if (B, R, S, ray0, nrays) == ref.PILEUP:
        pv, sg = ref.pileup_coords(H, W, gen)
    else:
        pv, sg = ref.random_coords(N, R, S, gen)
        ref.plant_hostile(pv, sg, H, W, gen)
    rt = ref.row_table(B, V, R, S, ray0, nrays)
    return gen, pv.contiguous(), sg.contiguous(), rt, ref.row_coords(rt, pv, sg)


def rows_per_tile(rt, nodes, wts, H, W):
    """Largest number of rows any (image, kind, 8 x 4-node tile) bucket of the table scatter receives."""
    base1 = ref.table_dims(H, W, 0)[0] * ref.table_dims(H, W, 0)[1]
    nw = (W // 2 + 1 + 2 * ref.PAD * rt["kind"]).view(-1, 1)
    local = nodes - (rt["kind"] * base1).view(-1, 1)
    key = ((rt["img"] * 2 + rt["kind"]).view(-1, 1) * 512 + (local // nw) // 4) * 512 + (local % nw) // 8
    key = torch.where(wts != 0, key, torch.full_like(key, -1)).sort(1).values
    first = torch.ones_like(key, dtype=torch.bool)
    first[:, 1:] = key[:, 1:] != key[:, :-1]
    return int(torch.bincount(key[first & (key >= 0)]).max())


# ------------------------------------------------------------------------------------------------------------------
# (a) cpn_scatter_rows_tables
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldx", [832, 896])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scatter_rows_tables_against_float64(case, ldx, dev):
    """dT[node_t] += a_t d[row] against index_add_ in float64: |got - want| <= gamma S_abs + 2^-20 max|d| on EVERY node and
    channel (gamma: ref.scatter_gamma, from the kernel's operation count), nodes that receive nothing exactly 0, the rows
    behind the table untouched, columns of d past 832 never read (they hold NaN)."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    H, W, B, R, S, ray0, nrays = case
    gen, pv, sg, rt, g = make_case(*case)
    N = B * V
    rows = nrays * V * S * 2
    d = ref.masked_grad(rows, 832, gen)
    dbuf = torch.full((rows, ldx), float("nan"), dtype=torch.float16)
    dbuf[:, :832] = d
    per = ref.table_nodes(H, W)
    assert per == int(_hip.lib().cpn_encode_table_nodes(H, W))
    nodes, wts = ref.node_taps_ref(g, rt["kind"], H, W)
    if case[2:] == ref.PILEUP:
        assert rows_per_tile(rt, nodes, wts, H, W) > ref.WMAX, "the pile-up case no longer splits a bucket"
    guard = 64
    dtab = torch.zeros(N * per + guard, 832, dtype=torch.float32, device=dev)
    dtab[N * per:] = 7.0
    nscr = int(_hip.lib().cpn_scatter_tables_scratch(H, W, B, V, R, S))
    assert nscr > 0
    scratch = torch.empty(nscr, dtype=torch.int32, device=dev)
    dd, pvd, sgd = dbuf.to(dev), pv.to(dev), sg.to(dev)
    call("cpn_scatter_rows_tables", dd.data_ptr(), ldx, H, W, pvd.data_ptr(), sgd.data_ptr(), B, V, R, S, ray0, nrays,
         dtab.data_ptr(), scratch.data_ptr(), _st())
    torch.cuda.synchronize()
    out = dtab.cpu()
    assert bool((out[N * per:] == 7.0).all()), "wrote behind the table"
    got = out[:N * per].double()
    want, s_abs, n = ref.scatter_tables_ref(d.float(), rt["img"], nodes, wts, N, H, W)
    dmax = float(d.float().abs().max())
    gamma = ref.scatter_gamma(n, min(R, nrays) * S).view(-1, 1)            # per node: its own term count (<= the largest)
    bound = ref.elementwise_bound(s_abs, gamma, dmax)
    err = (got - want).abs()
    worst = float((err / bound).max())
    print(f"scatter {case} ldx={ldx}: n_max={int(n.max())} gamma_max={float(gamma.max()):.2e} max err={float(err.max()):.3e} "
          f"max err/bound={worst:.3f} max|want|={float(want.abs().max()):.3e}")
    assert torch.isfinite(got).all()
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements off, first (node, channel) {bad[0].tolist()}: got " \
                             f"{float(got[tuple(bad[0])])} want {float(want[tuple(bad[0])])}, err/bound {worst:.2f}"
    assert bool((got[n == 0] == 0).all()), "a node that receives no tap is not exactly 0"


# ------------------------------------------------------------------------------------------------------------------
# (b) cpn_node_features_bwd
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nimg", [(32, 32, 1), (64, 64, 2), (32, 32, 6), (32, 64, 2)])
def test_node_features_bwd_against_float64_autograd(H, W, nimg, dev):
    """The adjoint of the node sampling against float64 autograd through node_features_ref, on four subsets with their own
    messages (edge ring and interior of each level; zeros-table nodes only; border-table nodes only).

    Bound |got - want| <= (n + 2) 2^-24 S_abs + 2^-20 max|dfeat|: for H, W powers of two the node coordinates and with them
    the texel fractions (multiples of 1/16) and weight products are exact in fp32, so a term w * dfeat is rounded once, the
    n terms of a texel (n: the nodes whose footprint holds it, from the float64 operator) are added one by one (n - 1), and
    one more covers a multiply and add that are not fused."""
    from coponerf_amd._hip import call
    gen = torch.Generator().manual_seed(H + W + nimg)
    per = ref.table_nodes(H, W)
    nb = ref.table_dims(H, W, 0)[0] * ref.table_dims(H, W, 0)[1]
    mats = [ref.node_features_matrix(l, H, W) for l in range(3)]
    shapes = [(H >> (4 - l), W >> (4 - l)) for l in range(3)]
    is_border = (torch.arange(per) < nb).repeat(nimg).view(-1, 1)
    for mode in ("all nodes", "zeros-table nodes only", "border-table nodes only"):
        dfeat = torch.randn(nimg * per, 768, generator=gen)
        if mode == "zeros-table nodes only":
            dfeat = dfeat * ~is_border
        elif mode == "border-table nodes only":
            dfeat = dfeat * is_border
        dfd = dfeat.to(dev).contiguous()
        dm = [torch.full((nimg, h, w, 256), float("nan"), dtype=torch.float32, device=dev) for h, w in shapes]
        call("cpn_node_features_bwd", dfd.data_ptr(), H, W, nimg, dm[0].data_ptr(), dm[1].data_ptr(), dm[2].data_ptr(), _st())
        torch.cuda.synchronize()
        z = [torch.zeros(nimg, 256, h, w, dtype=torch.float64, requires_grad=True) for h, w in shapes]
        (ref.node_features_ref(z[0], z[1], z[2], H, W) * dfeat.double()).sum().backward()
        dmax = float(dfeat.abs().max())
        for l, (h, w) in enumerate(shapes):
            got = dm[l].cpu().double()
            assert not torch.isnan(got).any(), f"level {l}: texels left unwritten ({mode})"
            want = z[l].grad.permute(0, 2, 3, 1)
            A = mats[l]
            dl = dfeat.double().view(nimg, per, 768)[:, :, l * 256:(l + 1) * 256]
            s_abs = torch.einsum("pt,npc->ntc", A.abs(), dl.abs()).view(nimg, h, w, 256)
            n = (A != 0).sum(0).view(1, h, w, 1).double()
            bound = ref.elementwise_bound(s_abs, (n + 2) * ref.U32, dmax)         # per texel: its own term count
            ok = (got - want).abs() <= bound
            ring = torch.zeros(h, w, dtype=torch.bool)
            ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
            print(f"node adjoint H={H} W={W} nimg={nimg} {mode} level {l}: n_max={int(n.max())} "
                  f"max err/bound={float(((got - want).abs() / bound).max()):.3f}")
            if mode == "all nodes":
                assert bool(ok[:, ring].all()), f"level {l}: edge ring off ({int((~ok[:, ring]).sum())} elements)"
                assert bool(ok[:, ~ring].all()), f"level {l}: interior off ({int((~ok[:, ~ring]).sum())} elements)"
            else:
                assert bool(ok.all()), f"level {l}: contributions of {mode} off ({int((~ok).sum())} elements, " \
                                       f"{int((~ok[:, ring]).sum())} of them on the edge ring)"


# ------------------------------------------------------------------------------------------------------------------
# (c) cpn_gather_rows_bwd_level3
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col0,ldx,start", [(0, 128, "zero"), (64, 192, "zero"), (0, 128, "nonzero")])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gather_rows_bwd_level3_against_float64_autograd(case, col0, ldx, start, dev):
    """grid_sample backward of the full-resolution level against float64 autograd through gather_levels at the lifted
    grids (ref.lift_grid: the fp32 pixel coordinate is the contract).  Same bound as the table scatter - cell, fractions,
    weights and additions are formed the same way (ref.scatter_gamma) - with the map's value on entry as one more term of
    the sum ("accumulated").  Columns of the gradient rows outside [col0, col0 + 64) hold NaN."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    H, W, B, R, S, ray0, nrays = case
    gen, pv, sg, rt, g = make_case(*case)
    N = B * V
    rows = nrays * V * S * 2
    d = ref.masked_grad(rows, 64, gen)
    dbuf = torch.full((rows, ldx), float("nan"), dtype=torch.float16)
    dbuf[:, col0:col0 + 64] = d
    init = torch.randn(N, H, W, 64, generator=gen) if start == "nonzero" else torch.zeros(N, H, W, 64)
    guard = 4096
    dm3 = torch.full((N * H * W * 64 + guard,), 7.0, dtype=torch.float32, device=dev)
    dm3[:N * H * W * 64] = init.reshape(-1).to(dev)
    boxes = torch.empty(B * V * int(_hip.lib().cpn_gather_bwd_chunks(R, S)) * 16, dtype=torch.int32, device=dev)
    dd, pvd, sgd = dbuf.to(dev), pv.to(dev), sg.to(dev)
    call("cpn_gather_rows_bwd_level3", dd.data_ptr(), ldx, col0, H, W, pvd.data_ptr(), sgd.data_ptr(), B, V, R, S, ray0,
         nrays, dm3.data_ptr(), boxes.data_ptr(), _st())
    torch.cuda.synchronize()
    out = dm3.cpu()
    assert bool((out[N * H * W * 64:] == 7.0).all()), "wrote behind the map"
    got = out[:N * H * W * 64].view(N, H, W, 64).double()
    want = ref.level3_bwd_ref(d.float(), H, W, pv, sg, B, V, R, S, ray0, nrays).permute(0, 2, 3, 1) + init.double()
    s_abs = ref.level3_bwd_ref(d.float().abs(), H, W, pv, sg, B, V, R, S, ray0, nrays).permute(0, 2, 3, 1) + init.abs().double()
    tex, wts = ref.level_taps_ref(g, rt["kind"], H, W)
    n = torch.zeros(N * H * W, dtype=torch.float64)
    for k in range(4):
        n.index_add_(0, rt["img"] * H * W + tex[:, k], (wts[:, k] != 0).double())
    dmax = max(float(d.float().abs().max()), float(init.abs().max()))
    gamma = ref.scatter_gamma(n + 1, 2 * min(R, nrays) * S).view(N, H, W, 1)  # per texel: its own term count
    bound = ref.elementwise_bound(s_abs, gamma, dmax)
    err = (got - want).abs()
    worst = float((err / bound).max())
    print(f"level3 {case} col0={col0} {start}: n_max={int(n.max())} max err={float(err.max()):.3e} max err/bound={worst:.3f}")
    assert torch.isfinite(got).all()
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements off, first (img, y, x, c) {bad[0].tolist()}, err/bound {worst:.2f}"
    untouched = (n == 0).view(N, H, W)
    assert torch.equal(got[untouched], init.double()[untouched]), "a texel that receives no tap changed"


# ------------------------------------------------------------------------------------------------------------------
# (d) cpn_gather_tail
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES[:-1], ids=IDS[:-1])
def test_gather_tail_against_float64(case, dev):
    """xt = [gather_3 | tanh(pt/5) | 1 | 0 x 60] against columns 768..834 of the layer's float64 input."""
    from coponerf_amd._hip import call
    H, W, B, R, S, ray0, nrays = case
    gen, pv, sg, rt, g = make_case(*case)
    N = B * V
    rows = nrays * V * S * 2
    z3 = torch.randn(N, 64, H, W, generator=gen).half().float()
    pe = (torch.rand(N, R, S, 6, generator=gen) * 2 - 1).contiguous()
    m3 = z3.permute(0, 2, 3, 1).contiguous().half().to(dev)
    guard = 64
    xt = torch.full((rows + guard, 128), float("nan"), dtype=torch.float16, device=dev)
    pvd, sgd, ped = pv.to(dev), sg.to(dev), pe.to(dev)
    call("cpn_gather_tail", m3.data_ptr(), H, W, pvd.data_ptr(), sgd.data_ptr(), ped.data_ptr(), B, V, R, S, ray0, nrays,
         xt.data_ptr(), _st())
    torch.cuda.synchronize()
    out = xt.cpu()
    assert torch.isnan(out[rows:].float()).all(), "wrote past the chunk"
    got = out[:rows]
    x3 = ref.chunk_rows(ref.gather_rows_ref([z3], pv, sg, B, V, R, S), B, V, R, S, ray0, nrays)          # (rows, 64) float64
    pe3 = ref.chunk_rows(pe.view(B, V, R, S, 2, 3).permute(0, 2, 1, 3, 4, 5).reshape(-1, 3), B, V, R, S, ray0, nrays)
    # one rounding to fp16 (half an ulp <= 2^-11 |want|) of a value blended in fp32 from fp16-exact texels (2^-24 max|z3|)
    err = (got[:, :64].double() - x3).abs()
    bound = ref.U16 * x3.abs() + ref.U32 * float(z3.abs().max())
    print(f"gather_tail {case}: max err/bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} gathered values off, worst err/bound {float((err / bound).max()):.2f}"
    assert torch.equal(got[:, 64:67].contiguous().view(torch.int16), pe3.half().view(torch.int16)), "point encoding columns"
    assert bool((got[:, 67] == 1).all()), "ones column"
    assert bool((got[:, 68:].contiguous().view(torch.int16) == 0).all()), "zero padding columns"


# ------------------------------------------------------------------------------------------------------------------
# (e) cpn_scale_to_f16
# ------------------------------------------------------------------------------------------------------------------
def _scale_call(x, target, dev, stale=0.0):
    """(s, 1/s, y on the host) of one call with a fresh scratch word (or one that holds the bits of `stale`)."""
    from coponerf_amd._hip import call
    xd = x.to(dev).contiguous()
    word = torch.tensor([stale], dtype=torch.float32, device=dev)
    y = torch.full((x.numel() + 8,), float("nan"), dtype=torch.float16, device=dev)
    sc = torch.zeros(2, dtype=torch.float32, device=dev)
    call("cpn_scale_to_f16", xd.data_ptr(), x.numel(), target, word.data_ptr(), y.data_ptr(), sc.data_ptr(), _st())
    torch.cuda.synchronize()
    yh = y.cpu()
    assert torch.isnan(yh[x.numel():].float()).all(), "wrote past y"
    return float(sc[0]), float(sc[1]), yh[:x.numel()]


def _check_scale(x, target, s, inv, y, amax=None):
    """The entry's contract: s a power of two in [2^-40, 2^40], 1/s exact, max|x| s in (target/2, target] when unclamped
    (the fp32 quotient target / max|x| and its logarithm are each rounded once: 1 +- 2^-22), y == fp16(x s) bit for bit (a
    power-of-two scale is exact in fp32 and both sides round to nearest even)."""
    assert s > 0 and math.frexp(s)[0] == 0.5 and 2.0 ** -40 <= s <= 2.0 ** 40, s
    assert inv == 1.0 / s
    finite = torch.isfinite(x)
    if amax is None:
        amax = float(x[finite].abs().max().double()) if bool(finite.any()) else 0.0
    if 2.0 ** -40 < s < 2.0 ** 40:
        assert target / 2 * (1 - 2.0 ** -22) < amax * s <= target * (1 + 2.0 ** -22), (amax, s, amax * s)
    elif s == 2.0 ** 40:
        assert max(amax, 1e-30) * s <= target * (1 + 2.0 ** -22)
    else:
        assert amax * s > target / 2 * (1 - 2.0 ** -22)
    want = (x * s).half()
    assert torch.equal(y.view(torch.int16)[finite], want.view(torch.int16)[finite]), "y is not fp16(x * s)"


def _scale_sizes():
    """n = 4; n whose absmax pass runs the tail loop only; n >= 4 * stride + tail for BOTH passes, from the entry's grids:
    absmax min(ceil(n4 / 1024), 512) workgroups, the scaling pass min(ceil(n4 / 256), 8192), 256 threads and one f32x4 each."""
    def grid(n4):
        return min(-(-n4 // 1024), 512) * 256, min(-(-n4 // 256), 8192) * 256
    tail_only = 4 * 100                                       # n4 = 100 < 256: i + 3 * stride < n4 never holds
    assert all(100 <= st for st in grid(100))
    n4 = 4 * 8192 * 256 + 12345
    assert all(n4 >= 4 * st + 12345 for st in grid(n4))
    return 4, tail_only, 4 * 1000, 4 * n4


def test_scale_to_f16_contract(dev):
    gen = torch.Generator().manual_seed(9)
    n_one, n_tail, n_mid, n_big = _scale_sizes()
    for n in (n_one, n_tail, n_mid):
        for target in (4096.0, 256.0):
            x = torch.randn(n, generator=gen) * 37.0
            _check_scale(x, target, *_scale_call(x, target, dev))
    # both loops of both passes; the largest entry once in the unrolled part, once in the tail, once first
    x = torch.randn(n_big, generator=gen)
    for where in (n_big // 3, n_big - 1, 0):
        xx = x.clone()
        xx[where] = -77.0
        s, inv, y = _scale_call(xx, 4096.0, dev)
        _check_scale(xx, 4096.0, s, inv, y)
        assert s == 32.0
    del x, xx, y
    # all zero: the scale is clamped, y is zero
    x = torch.zeros(n_mid)
    s, inv, y = _scale_call(x, 4096.0, dev)
    assert s == 2.0 ** 40 and inv == 2.0 ** -40 and bool((y.view(torch.int16) == 0).all())
    # one huge entry; all tiny (fp32 normals near the bottom, denormals)
    for big in (1e30, 3e38):
        x = torch.randn(n_mid, generator=gen)
        x[123] = big
        _check_scale(x, 4096.0, *_scale_call(x, 4096.0, dev))
    for tiny in (1e-38, 1e-40, 1e-44):
        x = torch.randn(n_mid, generator=gen).sign() * tiny
        s, inv, y = _scale_call(x, 4096.0, dev)
        assert s == 2.0 ** 40
        _check_scale(x, 4096.0, s, inv, y)
    # max|x| one ulp on either side of target / 2^k
    for target in (4096.0, 256.0):
        for k in (-5, 0, 1, 3, 10, 20):
            for eps in (-(2.0 ** -23), 0.0, 2.0 ** -23):
                top = torch.tensor(target / 2.0 ** k, dtype=torch.float64) * (1 + eps)
                x = (torch.rand(n_mid, generator=gen) - 0.5) * float(top)
                x[77] = -top.float()
                assert float(x.abs().max()) == float(top), "the planted value is not exact in fp32"
                s, inv, y = _scale_call(x, target, dev)
                _check_scale(x, target, s, inv, y)
    # inf / NaN planted: s stays a finite power of two, exactly the planted entries of y are not finite
    for plant in ((float("inf"),), (float("nan"),), (float("-inf"), float("nan"))):
        x = torch.randn(n_mid, generator=gen) * 3
        idx = [5 + 301 * i for i in range(len(plant))]
        for i, p in zip(idx, plant):
            x[i] = p
        s, inv, y = _scale_call(x, 4096.0, dev)
        amax = float("inf") if any(math.isinf(p) for p in plant) else None
        if amax is None:
            _check_scale(x, 4096.0, s, inv, y)
        else:
            assert s == 2.0 ** -40 and inv == 2.0 ** 40                            # target / inf = 0: clamped from below
            finite = torch.isfinite(x)
            assert torch.equal(y.view(torch.int16)[finite], (x * s).half().view(torch.int16)[finite])
        planted = torch.zeros(n_mid, dtype=torch.bool)
        planted[idx] = True
        assert torch.equal(~torch.isfinite(y.float()), planted)
    # a stale scratch word: the documented consequence of not zeroing it - s comes from the larger of the two values
    x = torch.randn(n_mid, generator=gen)
    amax = float(x.abs().max())
    s, inv, y = _scale_call(x, 4096.0, dev, stale=1000.0)
    _check_scale(x, 4096.0, s, inv, y, amax=1000.0)
    assert s == 4.0
    s, inv, y = _scale_call(x, 4096.0, dev, stale=amax / 8)
    _check_scale(x, 4096.0, s, inv, y)


# ------------------------------------------------------------------------------------------------------------------
# (f) argument checks: only what an entry rejects before any launch
# ------------------------------------------------------------------------------------------------------------------
def test_encode_backward_entry_points_reject_bad_arguments(dev):
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    st = _st()
    h = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    f = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    i = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    hp, fp, ip = h.data_ptr(), f.data_ptr(), i.data_ptr()

    def scatter(d=hp, H=32, W=32, ray0=0, nrays=1, scratch=ip, dtab=fp):
        call("cpn_scatter_rows_tables", d, 832, H, W, fp, fp, 1, 2, 1, 1, ray0, nrays, dtab, scratch, st)

    def level3(d=hp, H=32, W=32, ray0=0, nrays=1, boxes=ip):
        call("cpn_gather_rows_bwd_level3", d, 128, 0, H, W, fp, fp, 1, 2, 1, 1, ray0, nrays, fp, boxes, st)

    def tail(m3=hp, ray0=0, nrays=1, xt=hp):
        call("cpn_gather_tail", m3, 32, 32, fp, fp, fp, 1, 2, 1, 1, ray0, nrays, xt, st)

    def nodes_bwd(dfeat=fp, H=32, W=32, dm0=fp):
        call("cpn_node_features_bwd", dfeat, H, W, 1, dm0, fp, fp, st)

    def scale(x=fp, n=8, word=ip, y=hp):
        call("cpn_scale_to_f16", x, n, 4096.0, word, y, fp, st)

    null, shape, big, rng, algn = "null pointer", "bad shape", "1024", "ray range", "aligned"
    bad = [
        ("cpn_scatter_rows_tables", null, lambda: scatter(d=0)), ("cpn_scatter_rows_tables", null, lambda: scatter(scratch=0)),
        ("cpn_scatter_rows_tables", shape, lambda: scatter(H=24, W=24)), ("cpn_scatter_rows_tables", big, lambda: scatter(H=2048, W=2048)),
        ("cpn_scatter_rows_tables", rng, lambda: scatter(ray0=1, nrays=1)), ("cpn_scatter_rows_tables", rng, lambda: scatter(nrays=0)),
        ("cpn_scatter_rows_tables", algn, lambda: scatter(d=hp + 2)), ("cpn_scatter_rows_tables", algn, lambda: scatter(scratch=ip + 4)),
        ("cpn_gather_rows_bwd_level3", null, lambda: level3(d=0)), ("cpn_gather_rows_bwd_level3", null, lambda: level3(boxes=0)),
        ("cpn_gather_rows_bwd_level3", shape, lambda: level3(H=24, W=24)), ("cpn_gather_rows_bwd_level3", big, lambda: level3(H=2048, W=2048)),
        ("cpn_gather_rows_bwd_level3", rng, lambda: level3(ray0=1, nrays=1)),
        ("cpn_gather_tail", null, lambda: tail(m3=0)), ("cpn_gather_tail", rng, lambda: tail(ray0=0, nrays=2)),
        ("cpn_gather_tail", algn, lambda: tail(xt=hp + 2)),
        ("cpn_node_features_bwd", null, lambda: nodes_bwd(dfeat=0)), ("cpn_node_features_bwd", "multiples of 16", lambda: nodes_bwd(H=24, W=24)),
        ("cpn_node_features_bwd", algn, lambda: nodes_bwd(dm0=fp + 4)),
        ("cpn_scale_to_f16", null, lambda: scale(x=0)), ("cpn_scale_to_f16", null, lambda: scale(word=0)),
        ("cpn_scale_to_f16", "n % 4 == 0", lambda: scale(n=6)), ("cpn_scale_to_f16", algn, lambda: scale(x=fp + 4)),
        ("cpn_scale_to_f16", algn, lambda: scale(y=hp + 2)),
    ]
    for name, why, fn in bad:
        with pytest.raises(RuntimeError, match=name + ": .*" + why):
            fn()
    lib = _hip.lib()
    assert lib.cpn_scatter_tables_scratch(8, 32, 1, 2, 1, 1) == -1
    assert lib.cpn_scatter_tables_scratch(32, 32, 0, 2, 1, 1) == -1
    assert lib.cpn_scatter_tables_scratch(32, 32, 1, 2, 1, 0) == -1
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((h == 0).all()), "a rejected call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# the whole node: EncodeFn's backward under the GPU's own ReLU mask
# ------------------------------------------------------------------------------------------------------------------
# fp16 roundings on each gradient's path through EncodeFn._backward_tables (relative 2^-11 each):
#   dz0..2: d16 = fp16(s dC); dT16 = cpn_scale_to_f16(dT); wtab = fp16(W[:, :768])                          -> 3
#   dz3:    d16; W16 = fp16(W[:, 768:832]); dA = fp16(d16 . W16)                                            -> 3
#   dW:     columns 0..767: d16, dT16, the stored fp16 node features (3); columns 768..834: d16, xt (2)     -> 3
#   db:     d16 (the ones column of xt is exact)                                                            -> 1
K_ROUNDINGS = {"dz0": 3, "dz1": 3, "dz2": 3, "dz3": 3, "dW": 3, "db": 1}


@pytest.mark.parametrize("shape", [(2, 37, 24), ref.PILEUP[:3]], ids=["B2-R37-S24", "pileup"])
def test_encode_node_backward_against_float64_under_the_gpu_mask(shape, dev):
    """EncodeFn.apply(...).backward(dC) with nothing parked and nothing handed over (cpn_hid_grad_combine as a plain mask,
    then _backward_tables) against float64 autograd through grid_sample and the layer with d_pre = dC * (hid_gpu > 0): the
    mask is shared, so no ReLU flips are left and the error is the chain's fp16 roundings, K_ROUNDINGS[t] of them.
    Relative L2 per tensor <= k 2^-11; worst entry on the edge ring of every dz_l and on the pile-up texels
    <= 8 k 2^-11 max|want| (a lost edge or rim cannot hide in the L2 norm of the interior)."""
    from coponerf_amd.train_fns import EncodeFn, BackwardPass, KeyForward
    B, R, S = shape
    H = 64
    N = B * V
    pile = shape == ref.PILEUP[:3]
    gen = torch.Generator().manual_seed(77 + R)
    if pile:
        pv, sg = ref.pileup_coords(H, H, gen)
    else:
        pv, sg = ref.random_coords(N, R, S, gen)
        ref.plant_hostile(pv, sg, H, H, gen)
    pv, sg = pv.contiguous(), sg.contiguous()
    z = ref.make_maps(N, H, H, gen)
    pe = (torch.rand(N, R, S, 6, generator=gen) * 2 - 1).contiguous()
    W1 = (torch.rand(832, 835, generator=gen) * 2 - 1) / 835 ** 0.5
    b1 = (torch.rand(832, generator=gen) * 2 - 1) * 0.05
    Wk = (torch.rand(128, 1664, generator=gen) * 2 - 1) / 1664 ** 0.5
    bk = torch.zeros(128)
    rows = B * R * V * S * 2
    dC = torch.randn(rows, 832, generator=gen)
    zd = [t.to(dev).requires_grad_(True) for t in z]
    Wd, bd = W1.to(dev).requires_grad_(True), b1.to(dev).requires_grad_(True)
    bp = BackwardPass()
    hid = EncodeFn.apply(zd[0], zd[1], zd[2], zd[3], Wd, bd, pv.to(dev), sg.to(dev), pe.to(dev), (B, V, R, S), (H, H),
                         bp, KeyForward(Wk.to(dev), bk.to(dev)))
    # hid is fp16, so autograd hands its backward an fp16 gradient: by the pass's convention that is s * dC with s fixed by
    # the node that rounds first - here the test, with the pass's own rule (d16 = fp16(s dC), the first counted rounding)
    dCd = dC.to(dev)
    hid.backward((dCd * bp.ensure(dCd)).to(torch.float16))
    torch.cuda.synchronize()
    hid_gpu = hid.detach().float().cpu()
    # ---- float64 reference
    z64 = [t.double().requires_grad_(True) for t in z]
    W64, b64 = W1.double().requires_grad_(True), b1.double().requires_grad_(True)
    x = ref.encode_input_ref(z64, pv, sg, pe, B, V, R, S)
    pre = x @ W64.t() + b64
    want_hid = torch.relu(pre).detach()
    # the forward as test_encode_hidden_against_torch accepts it: the mask in use is a sane one
    scale = max(1.0, float(want_hid.abs().max()))
    assert torch.isfinite(hid_gpu).all()
    assert float((hid_gpu.double() - want_hid).abs().max()) <= 4e-3 * scale
    assert float((hid_gpu.double() - want_hid).pow(2).mean().sqrt()) <= 5e-4 * scale
    d_pre = dC.double() * (hid_gpu > 0)
    (pre * d_pre).sum().backward()
    got = {"dz%d" % l: zd[l].grad.cpu().double() for l in range(4)}
    got.update(dW=Wd.grad.cpu().double(), db=bd.grad.cpu().double())
    want = {"dz%d" % l: z64[l].grad for l in range(4)}
    want.update(dW=W64.grad, db=b64.grad)
    rt = ref.row_table(B, V, R, S, 0, B * R)
    g = ref.row_coords(rt, pv, sg)
    fails = []
    for name, k in K_ROUNDINGS.items():
        a, w = got[name], want[name]
        assert a.shape == w.shape and torch.isfinite(a).all(), name
        rel = float((a - w).norm() / w.norm())
        line = f"{name}: relative L2 {rel:.3e} (bar {k} * 2^-11 = {k * ref.U16:.3e})"
        if rel > k * ref.U16:
            fails.append(line)
        if name.startswith("dz"):
            l = int(name[2])
            Hl, Wl = w.shape[-2:]
            sel = torch.zeros(N, Hl, Wl, dtype=torch.bool)
            sel[:, 0], sel[:, -1], sel[:, :, 0], sel[:, :, -1] = True, True, True, True
            worst = {"edge ring": float((a - w).abs().permute(0, 2, 3, 1)[sel].max())}
            if pile:                                   # the texels of image 0 under the piled-up rows of pixel_val[0]
                own = (rt["img"] == 0) & (rt["kind"] == 0)
                tex, wts = ref.level_taps_ref(g[own], rt["kind"][own], Hl, Wl)
                sel = torch.zeros(N * Hl * Wl, dtype=torch.bool)
                sel[tex[wts != 0]] = True
                worst["pile-up texels"] = float((a - w).abs().permute(0, 2, 3, 1)[sel.view(N, Hl, Wl)].max())
            for what, e in worst.items():
                cap = 8 * k * ref.U16 * float(w.abs().max())
                line += f"; {what} worst {e:.3e} (cap {cap:.3e})"
                if e > cap:
                    fails.append(f"{name} {what}: worst entry {e:.3e} > {cap:.3e}")
        print(line)
    assert not fails, "\n".join(fails)
