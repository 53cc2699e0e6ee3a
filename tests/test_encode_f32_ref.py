"""tests/encode_f32_ref.py checked without a device: for each reference, an fp32-torch emulation of the kernel's rounding
points stays inside the bound on the GPU test's own cases (the worst err/bound per kernel is recorded in that module's
docstring), and each seeded defect leaves it."""
import pytest
import torch

from tests import encode_bwd_ref as bref
from tests import encode_f32_ref as ref

f32 = torch.float32


def _worst(what, got, want, bound):
    w = ref.assert_within(what, got, want, bound)
    assert w < 1.0
    return w


# ------------------------------------------------------------------------------------------------------------------
# emulations: the kernels' rounding points in fp32 torch
# ------------------------------------------------------------------------------------------------------------------
def _weights32(fx, fy):
    """Tap weights as the kernels form them: fl(1 - f) and an fp32 product."""
    wx, wy = (1.0 - fx, fx), (1.0 - fy, fy)
    return torch.stack([wx[k & 1] * wy[k >> 1] for k in range(4)], 1)


def _taps32(taps, H, W):
    """fp32 tap and texel weights of every row of `taps`: the fractions are the reference's own (exact in fp32)."""
    a = taps["a"]
    a32 = _weights32((a[:, 1] + a[:, 3]).float(), (a[:, 2] + a[:, 3]).float())         # fx = a1 + a3: exact in float64
    frac = []
    for axis, size in ((0, W), (1, H)):                                                 # level_xy of csrc/taps.h
        x = ((taps["g"][:, axis] + 1.0) * float(size) - 1.0) / 2.0
        x = torch.where(taps["kind"] == 0, x.clamp(0.0, size - 1.0), x.clamp(-2.0, size + 1.0))
        frac.append(x - torch.floor(x))
    b32 = torch.where(taps["b"] != 0, _weights32(frac[0], frac[1]), torch.zeros(1))      # taps outside the map: 0
    assert float((a32.double() - a).abs().max()) <= 3 * ref.U32 and float((b32.double() - taps["b"]).abs().max()) <= 3 * ref.U32
    return a32, b32


def emu_encode(d, taps, H, W):
    """cpn_encode_hidden_f32 in fp32 torch: fp32 taps, the four-term blend of x_k, the k-ordered chain of 68 steps from 0, the
    four table taps, the ReLU and the split -> (hi, lo) fp16 (rows, 832)."""
    a32, b32 = _taps32(taps, H, W)
    m3 = d["map3"].reshape(-1, 64)
    x3 = torch.zeros(a32.shape[0], 64)
    for k in range(4):
        x3 = x3 + b32[:, k:k + 1] * m3[taps["tex"][:, k]]
    x = torch.cat((x3, taps["pe"], torch.ones(x3.shape[0], 1)), 1)
    acc = torch.zeros(a32.shape[0], 832)
    for k in range(68):
        acc = acc + x[:, k:k + 1] * d["w80t"][k]
    for k in range(4):
        acc = acc + a32[:, k:k + 1] * d["tab"][taps["node"][:, k]]
    r = torch.relu(acc)
    assert r.dtype == f32
    hi = r.half()
    return hi, (r - hi.float()).half()


def emu_key(hs, w1, w2, b1, b2=None, accumulate=True, second=True, perm=None):
    """The two cpn_gemm_f16 calls in fp32 torch (fp16 operands are exact in fp32); perm: a k order of both calls."""
    p1 = torch.arange(ref.K1) if perm is None else torch.cat((perm + ref.K2, perm))
    p2 = torch.arange(ref.K2) if perm is None else perm
    c = hs.float()[:, p1] @ w1.float()[:, p1].t() + b1
    if second:
        c2 = hs.float()[:, p2] @ w2.float()[:, p2].t() + (0 if b2 is None else b2)
        c = c + c2 if accumulate else c2
    return torch.relu(c)


def emu_linear(X, W, bias, res, relu_in, relu_out, skip_last_block=False):
    x = torch.relu(X) if relu_in else X
    K = X.shape[1] - (16 if skip_last_block else 0)
    y = x[:, :K] @ W[:, :K].t()
    if bias is not None:
        y = y + bias
    if res is not None:
        y = y + res
    return torch.relu(y) if relu_out else y


# ------------------------------------------------------------------------------------------------------------------
# the emulations stay inside the bounds
# ------------------------------------------------------------------------------------------------------------------
def test_node_features_emulation_within_bound():
    worst = 0.0
    for H, W, nimg in ref.NODE_CASES:
        gen = torch.Generator().manual_seed(H + W + nimg)
        z = ref.node_maps(H, W, nimg, gen)
        want, bound, s_abs = ref.node_features_f32_ref(z, H, W)
        got = torch.cat([torch.einsum("pt,nct->npc", bref.node_features_matrix(l, H, W).float(), z[l].flatten(2)) for l in range(3)], 2)
        worst = max(worst, _worst(f"node features {H}x{W}x{nimg}", got.reshape(want.shape), want, bound))
        ze = ref.node_maps(H, W, nimg, gen, exact=True)
        got = torch.cat([torch.einsum("pt,nct->npc", bref.node_features_matrix(l, H, W).float(), ze[l].flatten(2)) for l in range(3)], 2)
        assert torch.equal(got.reshape(want.shape).double(), ref.node_features_f32_ref(ze, H, W)[0])
        border, rim = ref.rim_nodes(H, W, nimg)
        assert int(border.sum()) == nimg * (H // 2 + 1) * (W // 2 + 1) and int(rim.sum()) == nimg * ((H // 2 + 9) * (W // 2 + 9) - (H // 2 + 1) * (W // 2 + 1))
        assert bool((s_abs[rim] == 0).any()) and bool((s_abs[rim] != 0).any())          # the rim holds both kinds of nodes
    print(f"CALIBRATION cpn_node_features_f32 {worst:.3f}")


@pytest.mark.parametrize("case", ref.ENC_CASES, ids=ref.ENC_IDS)
def test_encode_hidden_emulation_within_bound(case):
    H, W, B, R, S, ray0, nrays = case
    d = ref.encode_inputs(case)
    taps = ref.encode_taps(d, B, R, S, H, W)
    r, bound, pre, _ = ref.encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    hi, lo = emu_encode(d, taps, H, W)
    rows = torch.arange(ray0, ray0 + nrays)
    got = ref.ray_rows(hi.double() + lo.double(), rows, S)
    w = _worst(f"encode {case}", got, ref.ray_rows(r, rows, S), ref.ray_rows(bound, rows, S))
    near = ref.near_zero(pre, bound)
    print(f"CALIBRATION cpn_encode_hidden_f32 {w:.3f} ({int(near.sum())} of {near.numel()} elements within the bound of 0)")
    assert 0.3 < float((pre > 0).double().mean()) < 0.7


def test_encode_exact_data_emulation_is_exact():
    case = (32, 32, 2, 7, 9, 3, 9)
    d = ref.encode_inputs(case, exact=True)
    taps = ref.encode_taps(d, 2, 7, 9, 32, 32)
    assert ref.encode_exact_ok(d, taps)
    r, _, pre, _ = ref.encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    hi, lo = emu_encode(d, taps, 32, 32)
    assert torch.equal(hi.double() + lo.double(), r)
    assert 0.3 < float((pre > 0).double().mean()) < 0.7 and bool((lo != 0).any())


def test_split_bound_is_tight():
    """hi = fp16(r), lo = fp16(r - hi) on 2 x 10^6 values from 7e-10 to 65 000: |hi + lo - r| <= U16^2 |r| + 2^-25."""
    gen = torch.Generator().manual_seed(3)
    e = torch.rand(2_000_000, generator=gen, dtype=torch.float64)
    r = torch.cat((torch.exp(e * (torch.log(torch.tensor(65000.0 / 7e-10, dtype=torch.float64))) + torch.log(torch.tensor(7e-10, dtype=torch.float64))).float(),
                   ref.split_ladder().clamp_min(0)))
    hi = r.half()
    lo = (r - hi.float()).half()
    assert torch.isfinite(hi.float()).all()
    w = ref.ratio(hi.double() + lo.double(), r.double(), ref.U16 * ref.U16 * r.double() + ref.SUB16).max()
    print(f"CALIBRATION split {float(w):.4f}")
    assert 0.9 < float(w) <= 1.0


def test_key_layer_emulation():
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for sigma in (1.0, 10.0):
        x, W, b, hs = ref.key_realistic_data(260, sigma, gen)
        w1, w2 = ref.key_split(W)
        want, bound = ref.key_intended_ref(x, W, b, hs, w1, w2)
        worst = max(worst, _worst(f"key layer sigma={sigma}", emu_key(hs, w1, w2, b), want, bound))
        assert 0.3 < float((want > 0).double().mean()) < 0.7
    print(f"CALIBRATION key layer, intended {worst:.3f}")


@pytest.mark.parametrize("M", ref.KEY_M[:3])
def test_key_exact_data_is_order_independent(M):
    """Bit-equal to float64 under torch's own k order and three random ones; about half the outputs are cut by the ReLU."""
    gen = torch.Generator().manual_seed(M)
    x, W, b, hs, w1, w2 = ref.key_exact_data(M, gen)
    want = ref.key_computed_ref(hs, w1, w2, b)
    pre = ref.key_computed_ref(hs, w1, w2, b, relu2=False)
    assert 0.3 < float((pre < 0).double().mean()) < 0.7
    for perm in (None, torch.randperm(ref.K2, generator=gen), torch.randperm(ref.K2, generator=gen), torch.randperm(ref.K2, generator=gen)):
        assert torch.equal(emu_key(hs, w1, w2, b, perm=perm).double(), want)
    b2 = torch.randint(-64, 65, (128,), generator=gen).float() / 64
    assert torch.equal(emu_key(hs, w1, w2, b, b2=b2).double(), ref.key_computed_ref(hs, w1, w2, b, b2))


def test_linear_emulation_within_bound():
    worst = 0.0
    for M, N, K in ref.LIN_CASES:
        gen = torch.Generator().manual_seed(M + N + K)
        X, W, bias, res = ref.linear_data(M, N, K, gen)
        for b_, r_, ri, ro in ((bias, res, 0, 0), (None, None, 1, 1), (bias, None, 0, 1), (None, res, 1, 0)):
            want, bound = ref.linear_f32_ref(X, W, b_, r_, ri, ro)
            worst = max(worst, _worst(f"linear {M}x{N}x{K}", emu_linear(X, W, b_, r_, ri, ro), want, bound))
        X, W, bias, res = ref.linear_data(M, N, K, gen, exact=True)
        want, _ = ref.linear_f32_ref(X, W, bias, res, 0, 0)
        assert torch.equal(emu_linear(X, W, bias, res, 0, 0).double(), want)
    print(f"CALIBRATION cpn_linear_f32 {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------
# seeded defects leave the bounds
# ------------------------------------------------------------------------------------------------------------------
DEFECT_CASE = (32, 32, 2, 7, 9, 3, 9)


@pytest.fixture(scope="module")
def enc():
    H, W, B, R, S, _, _ = DEFECT_CASE
    d = ref.encode_inputs(DEFECT_CASE)
    taps = ref.encode_taps(d, B, R, S, H, W)
    r, bound, _, _ = ref.encode_hidden_f32_ref(d["tab"], d["map3"], d["w80t"], taps)
    return d, taps, r, bound


def _swap_image(taps, H, W):
    """Rows read the other image of their pair: own <-> other."""
    per, px = bref.table_nodes(H, W), H * W
    img2 = taps["img"] ^ 1
    t = dict(taps)
    t["node"] = taps["node"] + ((img2 - taps["img"]) * per).view(-1, 1)
    t["tex"] = taps["tex"] + ((img2 - taps["img"]) * px).view(-1, 1)
    return t


def _border_table_for_other(taps, d, H, W):
    """The rows of the other view (kind 1) tap the border table of their image."""
    rt_kind = torch.zeros_like(taps["kind"])
    node, a = bref.node_taps_ref(taps["g"], rt_kind, H, W)
    t = dict(taps)
    t["node"], t["a"] = taps["img"].view(-1, 1) * bref.table_nodes(H, W) + node, a
    return t


def _tap_off_by_one(taps):
    t = dict(taps)
    t["node"] = taps["node"].clone()
    t["node"][:, 1] -= 1                                   # (stays inside the table: tap 1 is the right-hand node of a cell)
    return t


def _pe_order(taps):
    t = dict(taps)
    t["pe"] = taps["pe"][:, [1, 0, 2]]
    return t


@pytest.mark.parametrize("name", ["own / other image swapped", "border table for the other view", "one tap's node off by one column",
                                  "tanh(pt/5) columns in the wrong order", "bias row ignored", "lo half dropped"])
def test_encode_defects_leave_the_bound(name, enc):
    d, taps, r, bound = enc
    H, W = DEFECT_CASE[:2]
    w80t = d["w80t"]
    if name == "lo half dropped":
        hi, _ = emu_encode(d, taps, H, W)
        got = hi.double()
    else:
        if name == "bias row ignored":
            w80t = w80t.clone()
            w80t[67] = 0
        t = {"own / other image swapped": lambda: _swap_image(taps, H, W), "border table for the other view": lambda: _border_table_for_other(taps, d, H, W),
             "one tap's node off by one column": lambda: _tap_off_by_one(taps), "tanh(pt/5) columns in the wrong order": lambda: _pe_order(taps),
             "bias row ignored": lambda: taps}[name]()
        got = ref.encode_hidden_f32_ref(d["tab"], d["map3"], w80t, t)[0]
    n = ref.outside(got, r, bound)
    print(f"{name}: {n} of {r.numel()} elements leave the bound")
    assert n > 0


@pytest.mark.parametrize("name", ["hi W_lo call dropped", "out_f32 = 2 overwrites", "second call's bias added twice"])
def test_key_defects_differ_on_exact_data(name):
    gen = torch.Generator().manual_seed(60)
    x, W, b, hs, w1, w2 = ref.key_exact_data(60, gen)
    b2 = torch.randint(-64, 65, (128,), generator=gen).float() / 64
    want = ref.key_computed_ref(hs, w1, w2, b, b2)
    got = {"hi W_lo call dropped": lambda: emu_key(hs, w1, w2, b + b2, second=False),
           "out_f32 = 2 overwrites": lambda: emu_key(hs, w1, w2, b, b2=b2, accumulate=False),
           "second call's bias added twice": lambda: emu_key(hs, w1, w2, b, b2=2 * b2)}[name]()
    assert ref.outside(got, want, torch.zeros_like(want)) > 0
    # ... and the dropped call is what an accumulation bound over K1 + K2 terms hides on realistic data
    if name == "hi W_lo call dropped":
        x, W, b, hs = ref.key_realistic_data(260, 1.0, gen)
        w1, w2 = ref.key_split(W)
        want, bound = ref.key_intended_ref(x, W, b, hs, w1, w2)
        hidden = ref.outside(emu_key(hs, w1, w2, b, second=False), want, bound)
        print(f"dropped hi W_lo call on realistic data: {hidden} of {want.numel()} elements leave the intended-layer bound")


def test_linear_defect_skipped_k_block():
    for M, N, K in [c for c in ref.LIN_CASES if (c[2] // 16) % 2 == 1]:
        gen = torch.Generator().manual_seed(M + N + K)
        X, W, bias, res = ref.linear_data(M, N, K, gen)
        want, bound = ref.linear_f32_ref(X, W, bias, res, 0, 0)
        assert ref.outside(emu_linear(X, W, bias, res, 0, 0, skip_last_block=True), want, bound) > 0
        X, W, bias, res = ref.linear_data(M, N, K, gen, exact=True)
        want, _ = ref.linear_f32_ref(X, W, bias, res, 0, 0)
        if bool((X[:, K - 16:] != 0).any()):
            assert not torch.equal(emu_linear(X, W, bias, res, 0, 0, skip_last_block=True).double(), want)
