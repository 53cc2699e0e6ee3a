"""coponerf_amd.lpips on the MI355X against the float64 restatement of tests/lpips_ref.py (`pytest -m gpu`).

Head kernel (csrc/lpips.hip, cpn_lpips_head), alone on synthetic maps, per image and layer, against float64 on the same fp32
inputs:  |d| <= K * 2^-24 * mean_pixels sum_c w_c (|a_c| + |b_c|)^2  with K = 96, counted from the code in units of one
rounding u = 2^-24:
    squared norm: at most 32 FMAs in a lane + 4 butterfly adds on non-negative terms      36 u, halved by the root -> 18
    sqrtf, + 1e-10 (and the fp32 value of 1e-10, 0.6 u of the sum), 1 / x, f * r          1 + 1.6 + 1 + 1         -> 22.6 on a, b
    a - b                                                                                  1                       -> 23.6 (|a| + |b|)
    d^2: twice that                                                                        47.2
    w * d, then per pixel 32 FMAs in a lane, + 4 pixels, + 4 butterfly adds, + a 4-level
    tree over the 16 groups (all on non-negative terms)                                    1 + 32 + 4 + 4 + 4 = 45
    float64 finish, rounded once to fp32                                                   1
  = 93.2, taken as 96.
Stem kernel (cpn_lpips_stem), per element against a float64 convolution of the fp32 round-tripped, float64-scaled input:
    |d| <= (27 + 4) * 2^-24 * (|bias| + sum |w| |x|)  +  2 * 2^-24 * sum |w| |x|      (28 FMA roundings with slack; the scaling
    layer's subtraction and division, one rounding each, relative to x, carried through |w|).
End to end: the bar is max(head bound, 4 x d_stock) with d_stock the distance from float64 of a stock-op fp32 composition of
the same network run on the device here (library convolutions in NCHW including conv1_1, the head as torch ops) - the library's
summation order is unknown, so this bar is measured - and, independently, |d| <= 5e-5: half a unit of the fourth decimal
test.py:300 prints.  tests/test_lpips_ref.py shows what mistakes cost on the same cases (at least 100 x 5e-5).
Every case prints its distances before it asserts; DESIGN.md §4.10 quotes them.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from coponerf_amd import _hip
from coponerf_amd import lpips as cl
from tests import lpips_ref as lr

pytestmark = pytest.mark.gpu

K_HEAD = 96
U = 2.0 ** -24
CAP = 5e-5
SEED = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ head
@functools.lru_cache(maxsize=None)
def head_case(N, C, h, w, kind="unit"):
    """(maps (2N, h, w, C) fp32, lin (C), float64 d (N), float64 bound term (N)) - computed once, shared, read-only."""
    scale = {"unit": 1.0, "large": 1e4, "tiny": 1e-12, "zeros": 1.0}[kind]
    feat, lin = lr.make_maps(N, C, h, w, seed=1000 * C + 10 * h + w + N, scale=scale)
    if kind == "zeros":
        f = feat.view(2 * N, h * w, C)
        f[0, 0] = 0.0                                       # pixel 0 of image 0: zero in both maps
        f[N, 0] = 0.0
        f[0, (h * w) // 2] = 0.0                            # zero in the prediction only
        f[2 * N - 1, h * w - 1] = 0.0                       # zero in the target only (last image, last pixel)
    d, term = lr.head64_nhwc(feat, lin, N)
    return feat, lin, d, term


def run_head(maps, lins, N, dev, per_layer=False):
    out = cl.lpips_head([m.to(dev) for m in maps], [l.to(dev) for l in lins], N, per_layer)
    return tuple(o.cpu() for o in out) if per_layer else out.cpu()


def check_head(tag, got, d, term):
    err = (got.double() - d).abs()
    bound = K_HEAD * U * term
    print(f"{tag}: d {[f'{v:.6g}' for v in d.tolist()]}  |kernel - f64| {[f'{v:.2e}' for v in err.tolist()]}  "
          f"bound {[f'{v:.2e}' for v in bound.tolist()]}")
    assert bool(torch.isfinite(got).all()), got
    assert bool((err <= bound).all()), (tag, err.tolist(), bound.tolist())


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (16, 16), (33, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_head_against_float64(C, hw, N, dev):
    feat, lin, d, term = head_case(N, C, hw[0], hw[1])
    got, layers = run_head([feat], [lin], N, dev, per_layer=True)
    check_head(f"C {C} {hw[0]} x {hw[1]} N {N}", got, d, term)
    assert torch.equal(layers[:, 0], got) and bool((layers[:, 1:] == 0).all())        # one layer: out is its term


@pytest.mark.parametrize("C", [192, 448])
def test_head_channel_counts_between_vggs(C, dev):
    """The entry takes every multiple of 64 up to 512; 3 and 7 loads per lane are the odd ones among those VGG does not use."""
    N, h, w = 3, 5, 7
    feat, lin, d, term = head_case(N, C, h, w)
    check_head(f"C {C}", run_head([feat], [lin], N, dev), d, term)
    assert run_head([torch.cat((feat[:N], feat[:N]))], [lin], N, dev).tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("kind", ["large", "tiny", "zeros"])
@pytest.mark.parametrize("C", [64, 512])
def test_head_magnitudes_and_zero_vectors(kind, C, dev):
    """1e4: the squared norms reach 5e10; 1e-12: the norms (1e-11) are below the 1e-10 that is added to them; zero vectors in both
    maps (0 / 1e-10 = 0: no NaN) and in one (the pixel contributes sum_c w_c b_c^2)."""
    N, h, w = 2, 5, 7
    feat, lin, d, term = head_case(N, C, h, w, kind)
    got = run_head([feat], [lin], N, dev)
    check_head(f"{kind} C {C}", got, d, term)
    assert bool((d > 0).all())
    if kind == "tiny":
        plain = lr.head64_nhwc(feat * 1e12, lin, N)[0]      # without the eps the scale would cancel
        assert bool(((d - plain).abs() > 0.5 * plain).all())


LAYER_SHAPES = ((64, 9, 11), (128, 5, 7), (256, 16, 16), (512, 3, 2), (512, 1, 1))


@pytest.mark.parametrize("layers", [5, 2])
def test_head_several_layers_in_one_call(layers, dev):
    N = 3
    cases = [head_case(N, C, h, w) for C, h, w in LAYER_SHAPES[:layers]]
    got, per = run_head([c[0] for c in cases], [c[1] for c in cases], N, dev, per_layer=True)
    for k, c in enumerate(cases):
        check_head(f"layer {k} of {layers} {LAYER_SHAPES[k]}", per[:, k], c[2], c[3])
        alone = run_head([c[0]], [c[1]], N, dev)
        assert torch.equal(per[:, k], alone)                # a layer's term does not depend on its neighbours
    assert bool((per[:, layers:] == 0).all())
    total = sum(c[2] for c in cases)
    check_head(f"sum of {layers}", got, total, sum(c[3] for c in cases) + total / K_HEAD)      # + the sum's one rounding


def test_head_properties(dev):
    N, C, h, w = 3, 256, 33, 20
    feat, lin, _, _ = head_case(N, C, h, w)
    clean = run_head([feat], [lin], N, dev)
    assert torch.equal(clean, run_head([feat], [lin], N, dev))                          # two runs, the same bits
    same = torch.cat((feat[:N], feat[:N]))
    assert run_head([same], [lin], N, dev).tolist() == [0.0, 0.0, 0.0]                  # identical maps: exactly 0
    for n in range(N):                                                                  # image values do not depend on N
        one = torch.stack((feat[n], feat[N + n]))
        assert torch.equal(run_head([one], [lin], 1, dev)[0], clean[n])
    for where in ((1, 0, 0, 0), (N + 1, h - 1, w - 1, C - 1)):                          # a NaN in image 1 of 3, either map
        bad = feat.clone()
        bad[where] = float("nan")
        got = run_head([bad], [lin], N, dev)
        assert bool(torch.isnan(got[1])) and torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_head_rejects_what_it_cannot_run(dev):
    lib = _hip.lib()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    assert lib.cpn_lpips_head_scratch(3, 2, ints(33, 5), ints(20, 7)) == 3 * (11 + 1)   # 660 and 35 pixels in 64s
    assert lib.cpn_lpips_head_scratch(0, 1, ints(4), ints(4)) == 0 and lib.cpn_lpips_head_scratch(1, 6, ints(4), ints(4)) == 0
    assert lib.cpn_lpips_head_scratch(1, 1, ints(0), ints(4)) == 0
    f = torch.zeros(2, 2, 2, 96, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        cl.lpips_head([f], [torch.zeros(96, device=dev)], 1)
    with pytest.raises(ValueError, match="contiguous"):
        cl.lpips_head([torch.zeros(2, 64, 2, 2, device=dev).permute(0, 2, 3, 1)], [torch.zeros(64, device=dev)], 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        cl.lpips_head([torch.zeros(2, 2, 2, 64)], [torch.zeros(64)], 1)


# ------------------------------------------------------------------------------------------------------------------ stem
def stem_weights():
    w, b, _ = cl.parse_state_dict(cl.synthetic_state_dict(SEED))
    return w[0].contiguous(), b[0].contiguous()


def run_stem(p, t, dev):
    """p, t (N, H, W, 3) fp32 -> (2N, H, W, 64) on the host; the raw status for a shape the kernel rejects."""
    w, b = (x.to(dev) for x in stem_weights())
    N, H, W, _ = p.shape
    pd, td = p.contiguous().to(dev), t.contiguous().to(dev)
    out = torch.full((2 * N, H, W, 64), float("nan"), device=dev)
    status = _hip.lib().cpn_lpips_stem(pd.data_ptr(), td.data_ptr(), w.data_ptr(), b.data_ptr(), N, H, W, out.data_ptr(),
                                       _hip.stream_handle())
    return out.cpu() if status == 0 else status


def stem_images(N, H, W):
    p, t = lr.make_images(N, H, W, seed=21, target_gain=1.5)
    return p.permute(0, 2, 3, 1).contiguous(), t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", [(16, 16), (20, 28), (17, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_against_float64(hw, N, dev):
    p, t = stem_images(N, *hw)
    assert float(p.abs().max()) > 1.0 and float(t.abs().max()) > 1.0
    w, b = stem_weights()
    want, full, mag = lr.stem64(p, t, w, b)
    got = run_stem(p, t, dev)
    assert got.shape == want.shape
    err = (got.double() - want).abs()
    bound = 31 * U * full + 2 * U * mag
    print(f"stem {hw[0]} x {hw[1]} N {N}: max |kernel - f64| {err.max():.2e}  max err / bound {(err / bound).max():.3f}  "
          f"values up to {want.max():.3f}, {(want > 0).double().mean():.2f} of them positive")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    assert torch.equal(got, run_stem(p, t, dev))                                        # bit-reproducible
    if N == 3:                                                                          # an image does not depend on N
        one = run_stem(p[1:2], t[1:2], dev)
        assert torch.equal(one[0], got[1]) and torch.equal(one[1], got[N + 1])


def test_stem_clamps_the_prediction_only(dev):
    p, t = stem_images(2, 20, 28)
    got = run_stem(p, t, dev)
    assert torch.equal(run_stem(p.clamp(-1, 1), t, dev), got)                           # bit for bit its clamped copy
    other = run_stem(p, t.clamp(-1, 1), dev)
    assert torch.equal(other[:2], got[:2]) and not torch.equal(other[2:], got[2:])     # the target is taken as it is
    assert torch.equal(run_stem(t.clamp(-1, 1), p, dev)[:2], other[2:])                 # both halves run the same arithmetic


def test_stem_shape_errors(dev):
    p, t = stem_images(1, 15, 16)
    assert run_stem(p, t, dev) == -2 and b"H, W >= 16" in _hip.lib().cpn_last_error()
    p, t = stem_images(1, 16, 15)
    assert run_stem(p, t, dev) == -2
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    with pytest.raises(ValueError, match="H, W >= 16"):
        lp(torch.zeros(1, 3, 15, 32, device=dev), torch.zeros(1, 3, 15, 32, device=dev))
    with pytest.raises(RuntimeError, match="HIP device only"):
        lp(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


# ------------------------------------------------------------------------------------------------------------ end to end
def stock_lpips(p, t, weights, biases, lins):
    """The same network as stock fp32 device ops, NOT the module under test: library convolutions in NCHW including conv1_1,
    the head as torch ops.  p, t (N, 3, H, W) on the device."""
    shift = lr.SHIFT32.to(p.device).view(1, 3, 1, 1)
    scale = lr.SCALE32.to(p.device).view(1, 3, 1, 1)
    x = torch.cat((lr.round_trip32(p.clamp(-1.0, 1.0)), lr.round_trip32(t)))
    x = (x - shift) / scale
    N, total, n = p.shape[0], 0, 0
    for j, block in enumerate(cl.BLOCKS):
        if j:
            x = F.max_pool2d(x, 2, 2)
        for _ in block:
            x = F.relu(F.conv2d(x, weights[n], biases[n], padding=1))
            n += 1
        a = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = (a[:N] - a[N:]).pow(2)
        total = total + (d * lins[j].view(1, -1, 1, 1)).sum(1, keepdim=True).mean(dim=(2, 3)).view(N)
    return total


@pytest.mark.parametrize("case", list(lr.CASES))
def test_end_to_end_against_float64(case, dev):
    H, W, kw = lr.CASES[case]
    N = 3
    p, t = lr.make_images(N, H, W, seed=11, identical=1, **kw)
    want, want_layers, terms = lr.lpips64(p, t, SEED)
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    with torch.no_grad():
        got, layers = lp(p.to(dev), t.to(dev), per_layer=True)
        weights, biases, lins = ([x.to(dev) for x in part] for part in cl.parse_state_dict(cl.synthetic_state_dict(SEED)))
        stock = stock_lpips(p.to(dev), t.to(dev), weights, biases, lins)
    got, layers, stock = got.cpu().double(), layers.cpu().double(), stock.cpu().double()
    d, d_stock = (got - want).abs(), (stock - want).abs()
    head_bound = K_HEAD * U * terms.sum(1)
    bar = torch.maximum(head_bound, 4 * d_stock)
    print(f"{case}: lpips64 {[f'{v:.6f}' for v in want.tolist()]}  |module - f64| {[f'{v:.2e}' for v in d.tolist()]}  "
          f"|stock - f64| {[f'{v:.2e}' for v in d_stock.tolist()]}  head bound {[f'{v:.2e}' for v in head_bound.tolist()]}  "
          f"per layer |d| {[f'{v:.2e}' for v in (layers - want_layers).abs().max(0).values.tolist()]}")
    # the identical pair: exactly 0 in float64 and out of the head kernel (test_head_properties); through the library's
    # convolutions only within the bar, like the other images - they need not give images 1 and N + 1 of one batch the same
    # bits (the stock composition, which holds no kernel of this package, is 7.5e-14 from 0 on the 16 x 16 case, the module
    # 1.7e-13)
    assert want[1].item() == 0.0 and d_stock[1].item() <= CAP
    assert bool((want[[0, 2]] > 0.05).all())
    assert bool((d <= bar).all()), (d.tolist(), bar.tolist())
    assert bool((d <= CAP).all()), d.tolist()
    assert bool(((layers.sum(1) - got).abs() <= 6 * U * got.max()).all())                # per_layer: the terms of the sum, each rounded


def test_layouts_and_batch_independence(dev):
    """The hook's channels-last views are taken without a copy; an NCHW-contiguous batch goes through one and reaches the stem
    kernel as the same bytes.  Past the stem the library's convolutions decide the last bits - they are not the same from call
    to call on every machine, so whole results are compared within the end-to-end cap, not bit for bit (the two kernels
    themselves are bit-reproducible and batch-independent: tested above)."""
    H, W = 20, 28
    p, t = lr.make_images(3, H, W, seed=5)
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    pv = p.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)                 # as Evaluator.add hands it over
    tv = t.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
    pc, tc = p.to(dev), t.to(dev)                                                       # NCHW-contiguous
    assert lp._channels_last(pv).data_ptr() == pv.data_ptr() and lp._channels_last(pc).data_ptr() != pc.data_ptr()
    assert torch.equal(lp.stem(lp._channels_last(pv), lp._channels_last(tv)), lp.stem(lp._channels_last(pc), lp._channels_last(tc)))
    a, b, one = lp(pv, tv), lp(pc, tc), lp(pv[1:2], tv[1:2])
    assert a.shape == (3,) and a.dtype == torch.float32
    print("hook views", a.tolist(), "NCHW", b.tolist(), "image 1 alone", one.tolist())
    assert bool(((a - b).abs() <= CAP).all()) and bool(((one - a[1:2]).abs() <= CAP).all())


def test_trunk_takes_an_nchw_stem_output(dev):
    """Whatever layout relu1_1 arrives in, the taps are the contiguous NHWC the head reads: an NCHW-contiguous relu1_1 goes
    through the same trunk as the stem's channels_last view and gives its result within the bar."""
    p, t = lr.make_images(2, 20, 28, seed=5)
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    x = lp.stem(p.permute(0, 2, 3, 1).contiguous().to(dev), t.permute(0, 2, 3, 1).contiguous().to(dev))
    x_nchw = x.contiguous()
    assert x_nchw.is_contiguous() and not x.is_contiguous() and torch.equal(x, x_nchw)
    with torch.no_grad():
        taps, taps_nchw = lp.trunk(x), lp.trunk(x_nchw)
        a, b = lp.head(taps, 2), lp.head(taps_nchw, 2)
    for k, (u, v) in enumerate(zip(taps, taps_nchw)):
        assert u.is_contiguous() and v.is_contiguous() and u.shape == v.shape == (4, 20 >> k, 28 >> k, cl.TAP_CHANNELS[k])
    print("lpips from a channels_last / an NCHW relu1_1:", a.tolist(), b.tolist())
    assert bool(((a - b).abs() <= CAP).all())


# ------------------------------------------------------------------------------------------------------------- Evaluator
def test_evaluator_column(dev):
    from coponerf_amd.evaluate import Evaluator
    from tests.test_gpu_evaluate import _fake_output
    H = W = 32
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    ev = Evaluator(extra={"lpips": lp})
    outs = [_fake_output(2, H, W, 3 + i, dev) for i in range(2)]
    for out, _ in outs:
        out["rgb"] = out["rgb"] * 1.3                                                   # leaves [-1, 1] in places
    # an evaluation loop adds its batches behind get_z, which keeps the convolution library on its deterministic algorithms
    # for inference (getz._conv_determinism); this test has no model, so it puts the process into that state itself.  Left
    # free, the library's fp32 convolutions are not bit-equal from call to call at this size on every machine.
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    ev.add(outs[0][0], outs[0][1], [0.3, 0.8], image_shape=(H, W))                      # first call: allocations, library set-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add(outs[1][0], outs[1][1], [0.6, 0.7], image_shape=(H, W))
        direct = []
        for out, gt in outs:
            pv = out["rgb"].view(2, H, W, 3).clamp(-1, 1).permute(0, 3, 1, 2)
            direct.append(lp(pv, gt.view(2, H, W, 3).permute(0, 3, 1, 2)))
        rows = ev.rows()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.backends.cudnn.deterministic = was
    assert ev.host_reads == 0
    want = torch.cat(direct).double()
    assert ev.columns[-1] == "lpips" and torch.equal(rows[:, 8], want)                  # bit-equal to the direct call
    vals = want.tolist()
    print("evaluator lpips", vals)
    assert all(0.0 < v < 2.0 for v in vals)
    s = ev.summary()
    assert ev.host_reads == 1
    assert s["all"]["lpips"] == pytest.approx(((vals[0] + vals[1]) / 2 + (vals[2] + vals[3]) / 2) / 2, rel=1e-12)     # per call
    assert "LPIPS: " in ev.format_summary(s)
