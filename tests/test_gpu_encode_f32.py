"""The forward kernels of the reference-arithmetic render mode (precision = "f32": render_f32.node_tables, the per-sample stages
of render_f32.per_sample) each against its float64 reference (tests/encode_f32_ref.py): cpn_node_features_f32,
cpn_encode_hidden_f32 and its _rays form, the (hi, lo) key layer as per_sample issues it on cpn_gemm_f16 (out_f32 = 1, then 2),
cpn_linear_f32, and the chain of them against the original formulation.  Every element is compared; every bound is derived
beside its assertion or in the helper that forms it; outputs are NaN-filled with 7.0-filled guard rows behind them."""
import pytest
import torch

from tests import encode_bwd_ref as bref
from tests import encode_f32_ref as ref

pytestmark = pytest.mark.gpu

V = 2
GUARD = 64
FILL = 7.0
NAN = float("nan")
f16, f32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def stream64(dev):
    """A stream confined to 64 CUs (as test_cu_partition_streams makes one): the persistent grids shrink on it."""
    from coponerf_amd.streams import CUPartition, device_cus, stream_cus
    part = CUPartition(device_cus() - 64, 64, dev)
    assert stream_cus(part.getz) == 64
    yield part.getz
    part.close()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------------------------
# (a) cpn_node_features_f32
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,nimg", ref.NODE_CASES)
def test_node_features_f32_against_float64(H, W, nimg, dev):
    """|got - want| <= (4 + 3) u S_abs on every node and channel (ref.node_features_f32_ref), with separate messages for the
    border table, the zeros table inside the image and the zero rim; a value whose operator row is all zero (the outermost
    rim nodes of a level) is exactly 0.  On small-integer maps, whose products and sums are exact in fp32, bit-equal."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    gen = torch.Generator().manual_seed(H + W + nimg)
    rows = nimg * bref.table_nodes(H, W)
    assert rows == nimg * int(_hip.lib().cpn_encode_table_nodes(H, W))

    def run(z):
        maps = [t.permute(0, 2, 3, 1).contiguous().to(dev) for t in z]
        feat = torch.full((rows + GUARD, 768), NAN, dtype=f32, device=dev)
        feat[rows:] = FILL
        call("cpn_node_features_f32", maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), H, W, nimg, feat.data_ptr(), _st())
        torch.cuda.synchronize()
        out = feat.cpu()
        assert bool((out[rows:] == FILL).all()), "wrote behind the table"
        assert not torch.isnan(out[:rows]).any(), "nodes left unwritten"
        return out[:rows].double()

    z = ref.node_maps(H, W, nimg, gen)
    ze = ref.node_maps(H, W, nimg, gen, exact=True)
    assert torch.equal(run(ze), ref.node_features_f32_ref(ze, H, W)[0]), "exact data"
    want, bound, s_abs = ref.node_features_f32_ref(z, H, W)
    got = run(z)
    border, rim = ref.rim_nodes(H, W, nimg)
    r = ref.ratio(got, want, bound)
    sets = {"border-table nodes": border, "zeros-table nodes inside the image": ~border & ~rim, "zero rim (nodes -4..-1, M+1..M+4)": rim}
    print(f"node features {H}x{W}x{nimg}: max err/bound " + ", ".join(f"{k} {float(r[m].max()):.3f}" for k, m in sets.items()))
    for what, m in sets.items():
        assert bool((r[m] <= 1).all()), f"{what}: {int((~(r[m] <= 1)).sum())} elements off, worst err/bound {float(r[m].max()):.3f}"
    dead = s_abs == 0
    assert bool(dead[rim].any()) and not bool(dead[~rim].any())
    assert bool((got[dead] == 0).all()), "a rim value the float64 operator gives no weight is not exactly 0"


# ------------------------------------------------------------------------------------------------------------------
# (b) - (d) cpn_encode_hidden_f32 and its _rays form
# ------------------------------------------------------------------------------------------------------------------
def _to_dev(d, dev):
    return {k: v.contiguous().to(dev) for k, v in d.items()}


def _encode(dd, H, W, B, R, S, ray0, nrays, dev, stream=None, rays=None):
    """One launch -> hs on the host, (nrays V S + GUARD, 3328) fp16: NaN where the launch writes, FILL behind."""
    from coponerf_amd._hip import call
    rows = nrays * V * S
    hs = torch.full((rows + GUARD, ref.HS_LD), NAN, dtype=f16, device=dev)
    hs[rows:] = FILL
    torch.cuda.synchronize()
    s = _st() if stream is None else stream.cuda_stream
    if rays is None:
        call("cpn_encode_hidden_f32", dd["tab"].data_ptr(), dd["map3"].data_ptr(), H, W, dd["pv"].data_ptr(), dd["sg"].data_ptr(),
             dd["pe6"].data_ptr(), dd["w80t"].data_ptr(), B, V, R, S, ray0, nrays, hs.data_ptr(), s)
    else:
        call("cpn_encode_hidden_f32_rays", dd["tab"].data_ptr(), dd["map3"].data_ptr(), H, W, dd["pv"].data_ptr(), dd["sg"].data_ptr(),
             dd["pe6"].data_ptr(), dd["w80t"].data_ptr(), B, V, R, S, rays.data_ptr(), ray0, nrays, hs.data_ptr(), s)
    torch.cuda.synchronize()
    out = hs.cpu()
    assert bool((out[rows:] == FILL).all()), "wrote behind the chunk"
    return out[:rows]


def _check_encode(what, hs, want, bound, pre):
    """hs (rows, 3328) against r (rows 2, 832): hi + lo within the bound on the own and the other block; hi alone the fp16
    value of that sum (|hi - r| <= U16 (|r| + bound) + bound: a lo block stored where hi belongs cannot pass); the elements whose
    pre-activation is within the bound of 0 are part of both and are counted on their own."""
    assert not torch.isnan(hs.float()).any(), f"{what}: rows of the chunk left unwritten"
    hi, lo = ref.split_hs(hs)
    got = hi.double() + lo.double()
    worst = 0.0
    for j, blk in enumerate(("own", "other")):
        worst = max(worst, ref.assert_within(f"{what} hi + lo, {blk} image", got[j::2], want[j::2], bound[j::2]))
        ref.assert_within(f"{what} hi alone, {blk} image", hi.double()[j::2], want[j::2], bound[j::2] * (1 + ref.U16) + ref.U16 * want[j::2])
    near = ref.near_zero(pre, bound)
    n_off = ref.outside(got[near], want[near], bound[near])
    print(f"{what}: {int(near.sum())} elements within the bound of 0, {n_off} of them off")
    assert n_off == 0
    return worst


@pytest.mark.parametrize("case", ref.ENC_CASES, ids=ref.ENC_IDS)
def test_encode_hidden_f32_against_float64(case, dev, stream64):
    """The range form on full-mantissa tab / map3 / w80t and hostile coordinates against ref.encode_hidden_f32_ref, every
    channel of every live row; then the same launch on 64 CUs (a smaller grid, other batch ranges): the same bits."""
    H, W, B, R, S, ray0, nrays = case
    d = ref.encode_inputs(case)
    taps = ref.encode_taps(d, B, R, S, H, W)
    r, bound, pre, _ = ref.encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    rays = torch.arange(ray0, ray0 + nrays)
    dd = _to_dev(d, dev)
    hs = _encode(dd, H, W, B, R, S, ray0, nrays, dev)
    _check_encode(f"encode {case}", hs, ref.ray_rows(r, rays, S), ref.ray_rows(bound, rays, S), ref.ray_rows(pre, rays, S))
    hs64 = _encode(dd, H, W, B, R, S, ray0, nrays, dev, stream=stream64)
    assert torch.equal(_bits(hs64), _bits(hs)), "the result depends on the size of the grid"


def test_encode_hidden_f32_exact_data(dev):
    """Quarter-node coordinates and small-integer operands: every product and partial sum is exact in fp32
    (ref.encode_exact_ok), so hi + lo equals the float64 value exactly."""
    case = (32, 32, 2, 7, 9, 3, 9)
    H, W, B, R, S, ray0, nrays = case
    d = ref.encode_inputs(case, exact=True)
    taps = ref.encode_taps(d, B, R, S, H, W)
    assert ref.encode_exact_ok(d, taps)
    r, _, _, _ = ref.encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    hs = _encode(_to_dev(d, dev), H, W, B, R, S, ray0, nrays, dev)
    hi, lo = ref.split_hs(hs)
    want = ref.ray_rows(r, torch.arange(ray0, ray0 + nrays), S)
    diff = (hi.double() + lo.double() - want).abs()
    print(f"encode exact data: {int((diff != 0).sum())} of {diff.numel()} elements differ, max {float(diff.max()):.3e}")
    assert torch.equal(hi.double() + lo.double(), want)


def test_encode_hidden_f32_split_sweep(dev):
    """w80t = 0 except the bias row, tab = 0: r is the bias exactly, and hi, lo must be fp16(r), fp16(r - hi) of the host bit for
    bit over 2^-26 .. 65 504 - lo among the fp16 subnormals is not flushed, ties round to even.  (Nothing >= 65 520 is fed:
    hi would be inf; the kernel's header states the range.)"""
    case = (32, 32, 1, 3, 4, 0, 3)
    H, W, B, R, S, ray0, nrays = case
    d = ref.encode_inputs(case)
    lad = ref.split_ladder()
    bias = torch.rand(832, generator=torch.Generator().manual_seed(1)) * 100.0
    bias[:lad.numel()] = lad
    bias[416:416 + lad.numel()] = lad
    d["tab"] = torch.zeros_like(d["tab"])
    d["w80t"] = torch.zeros_like(d["w80t"])
    d["w80t"][67] = bias
    hs = _encode(_to_dev(d, dev), H, W, B, R, S, ray0, nrays, dev)
    hi, lo = ref.split_hs(hs)
    r = torch.relu(bias)
    want_hi = r.half()
    want_lo = (r - want_hi.float()).half()
    assert bool((want_lo.float() != 0).any()) and bool(((want_lo.float().abs() < 2.0 ** -14) & (want_lo != 0)).any()), "no subnormal lo in the sweep"
    bad_hi = (_bits(hi) != _bits(want_hi)[None]).sum(0)
    bad_lo = (_bits(lo) != _bits(want_lo)[None]).sum(0)
    print(f"split sweep: channels with a wrong hi {int((bad_hi > 0).sum())}, a wrong lo {int((bad_lo > 0).sum())}")
    assert int(bad_hi.sum()) == 0, f"hi != fp16(r) at channels {bad_hi.nonzero().reshape(-1).tolist()[:8]}: r = {r[bad_hi > 0][:8].tolist()}"
    assert int(bad_lo.sum()) == 0, f"lo != fp16(r - hi) at channels {bad_lo.nonzero().reshape(-1).tolist()[:8]}: r = {r[bad_lo > 0][:8].tolist()}"


def test_encode_hidden_f32_rays_against_float64(dev):
    """The list form against the float64 reference (not against the range form): a descending list with a ray listed twice,
    read from ray0 = 3 of a padded list, with one entry -1 and one entry B R - those resolve to dead rows, whose slots keep
    the fill pattern."""
    case = (32, 32, 2, 7, 9, 0, 14)
    H, W, B, R, S, _, _ = case
    d = ref.encode_inputs(case)
    taps = ref.encode_taps(d, B, R, S, H, W)
    r, bound, pre, _ = ref.encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    listed = [13, 9, 9, 8, -1, 5, B * R, 2, 0]
    ray0, nrays = 3, len(listed)
    rays = torch.tensor([1000, -1000, 6] + listed + [4, 1000], dtype=torch.int32)
    hs = _encode(_to_dev(d, dev), H, W, B, R, S, ray0, nrays, dev, rays=rays.to(dev))
    live = torch.tensor([0 <= t < B * R for t in listed])
    per_ray = hs.reshape(nrays, V * S * ref.HS_LD)
    assert torch.isnan(per_ray[~live].float()).all(), "the row slots of an out-of-range entry were written"
    sel = torch.tensor([t for t in listed if 0 <= t < B * R])
    _check_encode("encode, list form", per_ray[live].reshape(-1, ref.HS_LD), ref.ray_rows(r, sel, S), ref.ray_rows(bound, sel, S),
                  ref.ray_rows(pre, sel, S))


# ------------------------------------------------------------------------------------------------------------------
# (e) the (hi, lo) key layer on cpn_gemm_f16
# ------------------------------------------------------------------------------------------------------------------
def _key_layer(hs, w1, w2, b1, b2, dev, relu2=1, ldc=None):
    """The two calls exactly as render_f32.per_sample issues them -> kh on the host, (M, N) fp32."""
    from coponerf_amd._hip import call
    M, N = hs.shape[0], w1.shape[0]
    ldc = N if ldc is None else ldc
    hsd, w1d, w2d, b1d, b2d = [t.contiguous().to(dev) for t in (hs, w1, w2, b1, b2)]
    kh = torch.full((M + GUARD, ldc), NAN, dtype=f32, device=dev)
    kh[M:] = FILL
    kh[:, N:] = FILL
    call("cpn_gemm_f16", hsd.data_ptr(), ref.K1, w1d.data_ptr(), ref.K1, b1d.data_ptr(), kh.data_ptr(), ldc, M, N, ref.K1, 0, 1, _st())
    call("cpn_gemm_f16", hsd.data_ptr(), ref.K1, w2d.data_ptr(), ref.K2, b2d.data_ptr(), kh.data_ptr(), ldc, M, N, ref.K2, relu2, 2, _st())
    torch.cuda.synchronize()
    out = kh.cpu()
    assert bool((out[M:] == FILL).all()), "wrote behind the rows"
    assert bool((out[:, N:] == FILL).all()), "wrote columns past N"
    assert not torch.isnan(out[:M, :N]).any(), "elements left unwritten"
    return out[:M, :N]


@pytest.mark.parametrize("M", ref.KEY_M)
def test_key_layer_exact_data_is_bit_equal(M, dev):
    """On ref.key_exact_data every partial sum of (x_hi + x_lo) W_hi^T + x_hi W_lo^T + b is exact in fp32 in any order: the two
    calls must equal the float64 value of that expression bit for bit - with the ReLU in the second call and without, with a
    bias in the second call (out_f32 = 2 is "+= product + bias, then the ReLU"), with ldc = 136, and on the N = 208 tile."""
    gen = torch.Generator().manual_seed(M)
    x, W, b, hs, w1, w2 = ref.key_exact_data(M, gen)
    zero = torch.zeros(128)
    b2 = torch.randint(-64, 65, (128,), generator=gen).float() / 64
    pre = ref.key_computed_ref(hs, w1, w2, b, relu2=False)
    assert 0.3 < float((pre < 0).double().mean()) < 0.7
    variants = {"as per_sample issues them": (zero, 1, None), "relu = 0 in the second call": (zero, 0, None),
                "a bias in the second call": (b2, 1, None), "ldc = 136": (b2, 1, 136)}
    for what, (bias2, relu2, ldc) in variants.items():
        got = _key_layer(hs, w1, w2, b, bias2, dev, relu2=relu2, ldc=ldc)
        want = ref.key_computed_ref(hs, w1, w2, b, bias2, relu2=bool(relu2))
        diff = (got.double() - want).abs()
        print(f"key layer M={M} {what}: {int((diff != 0).sum())} of {diff.numel()} elements differ, max {float(diff.max()) * 2 ** 13:.1f} x 2^-13")
        assert torch.equal(got.double(), want), what
    x, W, b, hs, w1, w2 = ref.key_exact_data(M, gen, N=208)
    b2 = torch.randint(-64, 65, (208,), generator=gen).float() / 64
    got = _key_layer(hs, w1, w2, b, b2, dev)
    assert torch.equal(got.double(), ref.key_computed_ref(hs, w1, w2, b, b2)), "N = 208"


@pytest.mark.parametrize("sigma", [1.0, 10.0])
def test_key_layer_against_the_intended_layer(sigma, dev):
    """ReLU(x W^T + b) at M = 260 on x = ReLU(N(0, sigma)) with planted 1e-6, 2^-14, 100, 3000 and W = N(0, 0.05): within the
    representation residue + (K1 + K2 + 16) u S_abs of ref.key_intended_ref (loose by design; the exact-data test is sharp)."""
    gen = torch.Generator().manual_seed(int(sigma) + 5)
    x, W, b, hs = ref.key_realistic_data(260, sigma, gen)
    w1, w2 = ref.key_split(W)
    want, bound = ref.key_intended_ref(x, W, b, hs, w1, w2)
    got = _key_layer(hs, w1, w2, b, torch.zeros(128), dev)
    ref.assert_within(f"key layer, intended, sigma={sigma}", got.double(), want, bound)


# ------------------------------------------------------------------------------------------------------------------
# (f) cpn_linear_f32
# ------------------------------------------------------------------------------------------------------------------
def _padded(t, ld, dev, fill=NAN, guard=0):
    out = torch.full((t.shape[0] + guard, ld), fill, dtype=f32)
    out[:t.shape[0], :t.shape[1]] = t
    return out.to(dev)


def _linear(X, W, bias, res, relu_in, relu_out, dev, pad=False):
    """One call -> Y (M, N) on the host.  pad: every leading dimension larger than the width, ldr != ldy, the padding NaN (X, W,
    res: never read) or FILL (Y: never written); N = 3 runs the scalar epilogue at ldy = 3 and at ldy = 4."""
    from coponerf_amd._hip import call
    M, K = X.shape
    N = W.shape[0]
    ldx, ldw, ldy, ldr = (K + 8, K + 4, N + 4 - N % 4, N + 8) if pad else (K, K, N, N)
    Xd, Wd = _padded(X, ldx, dev), _padded(W, ldw, dev)
    bd = None if bias is None else bias.to(dev)
    rd = None if res is None else _padded(res, ldr, dev)
    Y = torch.full((M + GUARD, ldy), FILL, dtype=f32, device=dev)
    Y[:M, :N] = NAN
    call("cpn_linear_f32", Xd.data_ptr(), ldx, Wd.data_ptr(), ldw, 0 if bd is None else bd.data_ptr(), 0 if rd is None else rd.data_ptr(),
         0 if rd is None else ldr, Y.data_ptr(), ldy, M, N, K, relu_in, relu_out, _st())
    torch.cuda.synchronize()
    out = Y.cpu()
    assert bool((out[M:] == FILL).all()), "wrote rows >= M"
    assert bool((out[:, N:] == FILL).all()), "wrote columns >= N"
    assert not torch.isnan(out[:M, :N]).any(), "elements left unwritten (or a NaN of the padding read)"
    return out[:M, :N]


@pytest.mark.parametrize("M,N,K", ref.LIN_CASES, ids=["%dx%dx%d" % c for c in ref.LIN_CASES])
def test_linear_f32_against_float64(M, N, K, dev):
    """{bias, NULL} x {res, NULL} x {tight, padded leading dimensions}: |got - want| <= (K + 3) u S_abs on every element
    (ref.linear_f32_ref: a K-step fmaf chain, bias, res), and bit-equal to float64 on integer data whose partial sums are exact."""
    gen = torch.Generator().manual_seed(M + N + K)
    data = ref.linear_data(M, N, K, gen)
    exact = ref.linear_data(M, N, K, gen, exact=True)
    worst = 0.0
    for use_b in (True, False):
        for use_r in (True, False):
            X, W, bias, res = data
            want, bound = ref.linear_f32_ref(X, W, bias if use_b else None, res if use_r else None, 0, 0)
            Xe, We, be, re_ = exact
            want_e, _ = ref.linear_f32_ref(Xe, We, be if use_b else None, re_ if use_r else None, 0, 0)
            for pad in (False, True):
                got = _linear(X, W, bias if use_b else None, res if use_r else None, 0, 0, dev, pad=pad)
                worst = max(worst, float(ref.ratio(got.double(), want, bound).max()))
                n_off = ref.outside(got.double(), want, bound)
                assert n_off == 0, f"bias={use_b} res={use_r} pad={pad}: {n_off} elements off, worst err/bound {worst:.3f}"
                got = _linear(Xe, We, be if use_b else None, re_ if use_r else None, 0, 0, dev, pad=pad)
                assert torch.equal(got.double(), want_e), f"exact data, bias={use_b} res={use_r} pad={pad}"
    print(f"linear {M}x{N}x{K}: max err/bound = {worst:.3f}")


def test_linear_f32_relu_combinations(dev):
    M, N, K = 15, 128, 48
    gen = torch.Generator().manual_seed(4)
    X, W, bias, res = ref.linear_data(M, N, K, gen)
    for relu_in in (0, 1):
        for relu_out in (0, 1):
            want, bound = ref.linear_f32_ref(X, W, bias, res, relu_in, relu_out)
            got = _linear(X, W, bias, res, relu_in, relu_out, dev, pad=True)
            ref.assert_within(f"linear relu_in={relu_in} relu_out={relu_out}", got.double(), want, bound)
            assert bool((got >= 0).all()) == bool(relu_out)


def test_linear_f32_on_a_column_block_at_an_offset(dev):
    """As render_f32.linear_f32 calls it for the last 64 of 832 output columns (832 = 6 x 128 + 64): W rows 768.. of an
    (832, 768) matrix, bias + 768, Y and res columns 768.. of (M, 832) arrays.  The other columns of Y stay untouched."""
    from coponerf_amd._hip import call
    M, N, K, n0 = 100, 64, 768, 768
    gen = torch.Generator().manual_seed(8)
    X = torch.randn(M, K, generator=gen)
    Wfull, bfull, rfull = torch.randn(832, K, generator=gen) / K ** 0.5, torch.randn(832, generator=gen), torch.randn(M, 832, generator=gen)
    want, bound = ref.linear_f32_ref(X, Wfull[n0:], bfull[n0:], rfull[:, n0:], 0, 0)
    Xd, Wd, bd, rd = X.to(dev), Wfull.to(dev), bfull.to(dev), rfull.to(dev)
    Y = torch.full((M + GUARD, 832), FILL, dtype=f32, device=dev)
    Y[:M, n0:] = NAN
    call("cpn_linear_f32", Xd.data_ptr(), K, Wd.data_ptr() + n0 * K * 4, K, bd.data_ptr() + n0 * 4, rd.data_ptr() + n0 * 4, 832,
         Y.data_ptr() + n0 * 4, 832, M, N, K, 0, 0, _st())
    torch.cuda.synchronize()
    out = Y.cpu()
    assert bool((out[M:] == FILL).all()) and bool((out[:, :n0] == FILL).all()), "wrote outside the column block"
    ref.assert_within("linear, column block 768..831", out[:M, n0:].double(), want, bound)


def test_linear_f32_rejects_what_the_header_excludes(dev):
    """K a multiple of 16 and N <= 128: K = 20 and N = 129 are rejected with a message and write nothing."""
    from coponerf_amd._hip import call
    X = torch.ones(64, 64, device=dev)
    W = torch.ones(256, 64, device=dev)
    Y = torch.full((64, 256), FILL, dtype=f32, device=dev)
    for N, K in ((128, 20), (129, 32)):
        with pytest.raises(RuntimeError, match="cpn_linear_f32: need N<=128 and K%16==0"):
            call("cpn_linear_f32", X.data_ptr(), 64, W.data_ptr(), 64, 0, 0, 0, Y.data_ptr(), 256, 64, N, K, 0, 0, _st())
    torch.cuda.synchronize()
    assert bool((Y == FILL).all()), "a rejected call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# (g) the chain: weights + node_tables -> cpn_encode_hidden_f32 -> the key layer, against the original formulation
# ------------------------------------------------------------------------------------------------------------------
def test_chain_against_the_original_formulation(dev):
    """render_f32.weights + node_tables, cpn_encode_hidden_f32 and the key layer at H = W = 32, B = 1, R = 6, S = 5 on latents at
    get_z's statistics (not rounded to fp16), against float64 of the layers as the model states them: the 835-column input
    (grid_sample of all four levels | tanh(pt/5)), the 835 -> 832 layer, ReLU, the folded key matrix.  "A 1 x 1 convolution
    commutes with bilinear interpolation" is exact in real arithmetic; this is its check in fp32.

    hid:  |d| <= (7 + 771 + 82) u S_abs + COORD u (zmax |W1[:, :768]|^T) + U16^2 hid + 2^-25
          S_abs = (the same gather of |z|, |pe|) |W1|^T + |b1|.  A term passes the node sampling (ref.NODE_C = 7), the
          K = 768 projection on cpn_linear_f32 (K + 3) and the encode kernel (ref.ENC_C = 82); the bilinear weights are
          non-negative, so the tap blend of the nodes' S_abs is that gather.  COORD: the two formulations round a sample's
          coordinate differently - the tables use t = (g + 1) M / 2, grid_sample x = ((g + 1) Wl - 1) / 2 per level, each a
          few fp32 operations: at most 2 u (|g + 1| Wl + |x|) <= 10 u Wl texels apart for |g| <= 1.5, which moves a bilinear
          value by at most that times the difference of adjacent texels, <= 2 max|z_l|; Wl <= W / 4 on the table levels
          (beyond the clamps both are constant; level 3 uses grid_sample's own expression in both).
    kh:   |d| <= dhid |W'|^T + hid |W' - W~'|^T + (U16 hid) |W'_lo|^T + (K1 + K2 + 16) u (hid |W'|^T + |c'|)
          the first stage's bound through |W'| (ReLU is 1-Lipschitz), the residue of ref.key_intended_ref with |x_lo| <= U16 hid."""
    from coponerf_amd import render_f32, synthetic as syn
    from coponerf_amd._hip import call
    from coponerf_amd.render import RenderEngine
    H = W = 32
    B, R, S = 1, 6, 5
    N, rows = B * V, B * R * V * S
    params = syn.make_render_weights()
    z, _, _ = syn.make_latents(B, H, W, seed=21)
    z = syn.latents_at_getz_statistics(z)
    assert all(not torch.equal(t, t.half().float()) for t in z)
    gen = torch.Generator().manual_seed(17)
    pv, sg = bref.random_coords(N, R, S, gen)
    bref.plant_hostile(pv, sg, H, W, gen)
    assert bool(((pv.abs() <= 1.5) | (pv.abs() >= 1e9)).all()) and bool(((sg.abs() <= 1.5) | (sg.abs() >= 1e9)).all())
    pe6 = (torch.rand(N, R, S, 6, generator=gen) * 2 - 1).contiguous()
    pd = {k: v.to(dev) for k, v in params.items()}
    w = render_f32.weights(RenderEngine()._weights(pd), pd)
    tab, map3 = render_f32.node_tables([t.to(dev) for t in z], w, H, W, _st())
    dd = {"tab": tab, "map3": map3, "w80t": w["k80t"], "pv": pv.contiguous().to(dev), "sg": sg.contiguous().to(dev), "pe6": pe6.to(dev)}
    hs = _encode(dd, H, W, B, R, S, 0, B * R, dev)
    kh = _key_layer(hs, w["key_fold.w1"].cpu(), w["key_fold.w2"].cpu(), w["key_fold.b"].cpu(), torch.zeros(128), dev)
    # ---- float64, the original formulation
    W1 = params["query_encode_latent.weight"].reshape(832, 835).double()
    b1 = params["query_encode_latent.bias"].double()
    x = bref.encode_input_ref(z, pv, sg, pe6, B, V, R, S)
    xabs = bref.encode_input_ref([t.abs() for t in z], pv, sg, pe6.abs(), B, V, R, S)
    hid = torch.relu(x @ W1.t() + b1)
    zmax = torch.cat([torch.full((256,), float(t.abs().max()), dtype=torch.float64) for t in z[:3]])
    coord = 10 * (W // 4)
    dhid = (ref.NODE_C + 771 + ref.ENC_C) * ref.U32 * (xabs @ W1.abs().t() + b1.abs()) + coord * ref.U32 * (zmax @ W1[:, :768].abs().t()) \
        + ref.U16 * ref.U16 * hid + ref.SUB16
    hi, lo = ref.split_hs(hs)
    ref.assert_within("chain: hid", hi.double() + lo.double(), hid, dhid)
    Wf, cf = w["key_fold.w"].cpu().double(), w["key_fold.b"].cpu().double()
    Wh, Wl = w["key_fold.w1"].cpu()[:, :ref.K2].double(), w["key_fold.w2"].cpu().double()
    h2, dh2 = hid.reshape(rows, ref.K2), dhid.reshape(rows, ref.K2)
    want = torch.relu(h2 @ Wf.t() + cf)
    dkh = dh2 @ Wf.abs().t() + h2 @ (Wf - Wh - Wl).abs().t() + (ref.U16 * h2) @ Wl.abs().t() \
        + ref.KEY_C * ref.U32 * (h2 @ Wf.abs().t() + cf.abs())
    ref.assert_within("chain: kh", kh.double(), want, dkh)
    assert 0.1 < float((want > 0).double().mean()) < 0.9
