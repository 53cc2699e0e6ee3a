"""The adjoint kernels of csrc/lpips.hip and LPIPS.differentiable on the MI355X against float64 (`pytest -m gpu`).

Every comparison is to tests/lpips_grad_ref.py in float64 on the same fp32 inputs, per element:
    |d| <= K * 2^-24 * (sum of the absolute values of the element's terms).

Head (cpn_lpips_head_bwd), df_j = r u_j - (sum_c u_c f_c) r r / s f_j; the terms are r |u_j| and (sum_c |u_c| |f_c|) r^2 |f_j| / s
with |u_c| = lin_c (|a_c| + |b_c|) 2 |g| / P.  K_HEAD_BWD = 132, counted from the code in units of one rounding u = 2^-24:
    squared norm: at most 32 FMAs in a lane + 4 butterfly adds on non-negative terms        36 u, halved by the root -> 18
    s = sqrtf                                                                                1                       -> 19 on s
    + 1e-10 (and the fp32 value of 1e-10, 0.6 u of the sum), 1 / x                           1.6 + 1                 -> 21.6 on r
    a = f r, b likewise; a - b                                                               1; 1          -> 23.6 on (|a| + |b|)
    lin * d; coef = 2 g / P (P to float, the division); * coef                               1; 1.5; 1               -> 27.1 on |u|
    first term: r (21.6), u (27.1), the product                                              1                       -> 49.7
    dot = sum u f: 32 FMAs in a lane + 4 butterfly adds, on sum |u| |f|; u's own             36 + 27.1               -> 63.1
    k2 = dot r r / s: r twice, s, three operations                                           43.2 + 19 + 3           -> 128.3
    the final FMA rounds the element once, at most 1 u of the sum of both terms              1 on each
  = 50.7 on the first term, 129.3 on the second; 129.3 on their sum, taken as 132.
Stem (cpn_lpips_stem_bwd), terms |w| |dy'| / scale.  K_STEM_BWD = 20:
    per (ci, ky, kx): a product and 3 FMAs in a lane, 4 butterfly adds                       8
    the nine taps: 8 additions                                                               8
    / scale                                                                                  1
  = 17, taken as 20.
Where the terms are 0 (a zero prediction vector; a pred outside [-1, 1] or NaN) the result must be exactly 0.

End to end (LPIPS.differentiable, the gradient of its sum to p): per image, max over the elements, the bar is
max(own bound, 4 x d_stock), d_stock the same distance from float64 of a stock-op fp32 composition under autograd on the device
(tests/test_gpu_lpips.py's stock_lpips).  The own bound is K_STEM_BWD * 2^-24 * max of the stem's terms on the float64
gradient of relu1_1: it counts the LAST kernel alone, as if its input were exact, and takes no account of the head's adjoint
or of the twelve convolutions' backward, whose summation order is the library's and unknown.  In practice the bar is therefore
4 x d_stock, a measured bar as the forward's is; the counted part only keeps it from collapsing where the stock composition
happens to land on float64.  The value meets the forward test's bounds.
Every case prints before it asserts; DESIGN.md §4.12 quotes the figures.
"""
import pytest
import torch

from coponerf_amd import _hip
from coponerf_amd import lpips as cl
from tests import lpips_grad_ref as gr
from tests import lpips_ref as lr
from tests.test_gpu_lpips import CAP, K_HEAD, stock_lpips

pytestmark = pytest.mark.gpu

U = gr.U
SEED = gr.SEED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------ head
def run_head_bwd(feat, lin, g, dev):
    return cl.lpips_head_bwd([feat.to(dev)], [lin.to(dev)], g.to(dev))[0].cpu()


def check(tag, got, want, terms, K):
    err = (got.double() - want).abs()
    bound = K * U * terms
    live = terms > 0
    worst = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"{tag}: max |g| {float(want.abs().max()):.3e}  max |kernel - f64| {float(err.max()):.3e}  max err / bound {worst:.3f}  "
          f"({int((~live).sum())} of {live.numel()} elements exactly 0)")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), tag
    assert bool((got[~live] == 0).all())


@pytest.mark.parametrize("kind", gr.HEAD_KINDS)
@pytest.mark.parametrize("N", gr.HEAD_N)
@pytest.mark.parametrize("hw", gr.HEAD_HW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", gr.HEAD_C)
def test_head_bwd_against_float64(C, hw, N, kind, dev):
    h, w = hw
    feat, lin, g = gr.head_case(N, C, h, w, kind)
    want, terms = gr.head_grad_closed(feat, lin, N, g)
    got = run_head_bwd(feat, lin, g, dev)
    assert got.shape == (N, h, w, C)
    check(f"head bwd C {C} {h} x {w} N {N} {kind}", got, want, terms, gr.K_HEAD_BWD)
    if kind == "zeros":
        flat = got.view(N, h * w, C)
        for n, pix in gr.zero_pixels(N, h, w):                          # a zero prediction vector: exactly 0, finite
            assert bool((flat[n, pix] == 0).all())
        # the neighbours: what the same maps give without the zeroed vectors, wherever the vectors are the same
        plain, _, _ = gr.head_case(N, C, h, w, "unit")
        same = (plain.view(2 * N, h * w, C) == feat.view(2 * N, h * w, C)).all(-1)
        same = same[:N] & same[N:]
        assert int((~same).sum()) == len({(0, 0), (0, (h * w) // 2), (N - 1, h * w - 1)})
        other = run_head_bwd(plain, lin, g, dev).view(N, h * w, C)
        assert torch.equal(flat[same], other[same])


def test_head_bwd_properties(dev):
    N, C, h, w = 3, 512, 5, 7
    feat, lin, g = gr.head_case(N, C, h, w)
    clean = run_head_bwd(feat, lin, g, dev)
    assert torch.equal(clean, run_head_bwd(feat, lin, g, dev))                          # two runs, the same bits
    for n in range(N):                                                                  # image n does not depend on N
        one = torch.stack((feat[n], feat[N + n]))
        assert torch.equal(run_head_bwd(one, lin, g[n:n + 1], dev)[0], clean[n])
    assert bool((run_head_bwd(feat, lin, torch.zeros(N), dev) == 0).all())
    same = torch.cat((feat[:N], feat[:N]))                                              # identical maps: u = 0 exactly
    assert bool((run_head_bwd(same, lin, g, dev) == 0).all())


def test_head_bwd_several_layers_in_one_call(dev):
    N = 3
    shapes = ((64, 16, 16), (512, 5, 7), (512, 2, 2), (64, 1, 1), (512, 1, 1))
    cases = [gr.head_case(N, C, h, w) for C, h, w in shapes]
    g = cases[0][2]
    got = cl.lpips_head_bwd([c[0].to(dev) for c in cases], [c[1].to(dev) for c in cases], g.to(dev))
    for c, d in zip(cases, got):
        assert torch.equal(d.cpu(), run_head_bwd(c[0], c[1], g, dev))                   # a layer does not depend on its neighbours


def test_head_bwd_rejects_what_it_cannot_run(dev):
    f = torch.zeros(2, 2, 2, 96, device=dev)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        cl.lpips_head_bwd([f], [torch.zeros(96, device=dev)], torch.zeros(1, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        cl.lpips_head_bwd([torch.zeros(2, 64, 2, 2, device=dev).permute(0, 2, 3, 1)], [torch.zeros(64, device=dev)],
                          torch.zeros(1, device=dev))
    with pytest.raises(ValueError, match="2N"):
        cl.lpips_head_bwd([torch.zeros(2, 2, 2, 64, device=dev)], [torch.zeros(64, device=dev)], torch.zeros(2, device=dev))


# ------------------------------------------------------------------------------------------------------------------ stem
def run_stem_bwd(p, y, dy, dev):
    """(N, H, W, 3) on the host; the raw status for a shape the kernel rejects."""
    w = gr.stem_weights()[0].to(dev)
    N, H, W, _ = p.shape
    pd, yd, dyd = p.to(dev), y.to(dev), dy.to(dev)
    out = torch.full((N, H, W, 3), float("nan"), device=dev)
    status = _hip.lib().cpn_lpips_stem_bwd(dyd.data_ptr(), yd.data_ptr(), pd.data_ptr(), w.data_ptr(), N, H, W, out.data_ptr(),
                                           _hip.stream_handle())
    return out.cpu() if status == 0 else status


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("hw", gr.STEM_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_bwd_against_float64(hw, N, dev):
    p, y, dy = gr.stem_case(N, *hw)
    w = gr.stem_weights()[0]
    want, terms = gr.stem_grad_closed(p, y, dy, w)
    got = run_stem_bwd(p, y, dy, dev)
    check(f"stem bwd {hw[0]} x {hw[1]} N {N}", got, want, terms, gr.K_STEM_BWD)
    out = (p.abs() > 1) | torch.isnan(p)
    assert bool((got[out] == 0).all()) and bool((got[p.abs() == 1] != 0).all())       # torch's clamp mask, inclusive
    # borders against absent taps: the same gradient with the image embedded in a larger one whose extra ring has dy = 0
    ring = lambda t, v: torch.nn.functional.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1), value=v).permute(0, 2, 3, 1).contiguous()
    big = run_stem_bwd(ring(p, 0.0), ring(y, 1.0), ring(dy, 0.0), dev)
    assert torch.equal(big[:, 1:-1, 1:-1], got)
    assert torch.equal(got, run_stem_bwd(p, y, dy, dev))                                # bit-reproducible
    if N == 2:                                                                          # an image does not depend on N
        assert torch.equal(run_stem_bwd(p[1:2], y[1:2], dy[1:2], dev)[0], got[1])


def test_stem_bwd_takes_the_relu_mask_from_y(dev):
    N, H, W = 1, 16, 40
    p, y, dy = gr.stem_case(N, H, W)
    got = run_stem_bwd(p, y, dy, dev)
    assert torch.equal(run_stem_bwd(p, y, torch.where(y > 0, dy, torch.full_like(dy, 1e30)), dev), got)      # dy is not read there
    assert bool((run_stem_bwd(p, torch.zeros_like(y), dy, dev) == 0).all())


def test_stem_bwd_shape_errors(dev):
    z = lambda *s: torch.zeros(*s)
    assert run_stem_bwd(z(1, 15, 16, 3), z(1, 15, 16, 64), z(1, 15, 16, 64), dev) == -2
    assert b"H, W >= 16" in _hip.lib().cpn_last_error()
    assert run_stem_bwd(z(1, 16, 15, 3), z(1, 16, 15, 64), z(1, 16, 15, 64), dev) == -2


# ------------------------------------------------------------------------------------------------------------ end to end
def img_max(x):
    return x.abs().reshape(x.shape[0], -1).max(1).values


def reference_and_bars(p, t, dev, tag):
    """p, t (N, 3, H, W) fp32 on the host -> (lpips64 (N), its gradient to p, the bar of the value (N), the bar of the gradient
    (N): per image, on the max over its elements), float64.  Shared with tests/test_gpu_lpips_loss.py."""
    want, gwant, mag = gr.lpips_grad64(p, t, SEED)
    terms = lr.lpips64(p, t, SEED)[2]
    weights, biases, lins = ([x.to(dev) for x in part] for part in cl.parse_state_dict(cl.synthetic_state_dict(SEED)))
    ps = p.to(dev).requires_grad_(True)
    stock = stock_lpips(ps, t.to(dev), weights, biases, lins)
    stock.sum().backward()
    d_stock = (stock.detach().cpu().double() - want).abs()
    e_stock = img_max(ps.grad.cpu().double() - gwant)
    own = gr.K_STEM_BWD * U * img_max(mag)
    print(f"{tag}: lpips64 {[f'{v:.6f}' for v in want.tolist()]}  |stock - f64| {[f'{v:.2e}' for v in d_stock.tolist()]}  "
          f"max |grad64| {[f'{v:.3e}' for v in img_max(gwant).tolist()]}  max |stock grad - f64| "
          f"{[f'{v:.2e}' for v in e_stock.tolist()]}  own bound {[f'{v:.2e}' for v in own.tolist()]}")
    return want, gwant, torch.maximum(K_HEAD * U * terms.sum(1), 4 * d_stock), torch.maximum(own, 4 * e_stock)


@pytest.mark.parametrize("side", [16, 32])
def test_differentiable_against_float64(side, dev):
    N = 2
    p, t = lr.make_images(N, side, side, seed=11, low_contrast=side == 16)
    want, gwant, bar, gbar = reference_and_bars(p, t, dev, f"{side} x {side}")
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    pd, td = p.to(dev).requires_grad_(True), t.to(dev).requires_grad_(True)
    val = lp.differentiable(pd, td)
    assert val.shape == (N,) and val.requires_grad
    val.sum().backward()
    assert td.grad is None and pd.grad is not None and pd.grad.shape == p.shape
    d = (val.detach().cpu().double() - want).abs()                                      # the value: the forward test's bounds
    g = pd.grad.cpu().double()
    e = img_max(g - gwant)                                                              # the gradient, per image
    print(f"{side} x {side}: |module - f64| {[f'{v:.2e}' for v in d.tolist()]}  max |module grad - f64| {[f'{v:.2e}' for v in e.tolist()]}")
    assert bool((d <= bar).all()) and bool((d <= CAP).all())
    assert bool(torch.isfinite(g).all()) and bool((img_max(gwant) > 0).all())
    assert bool((e <= gbar).all()), (e.tolist(), gbar.tolist())
    assert bool((g[p.abs() > 1] == 0).all())                                            # the clamp passes nothing outside [-1, 1]


def test_differentiable_checks_its_inputs_like_forward(dev):
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    with pytest.raises(ValueError, match="H, W >= 16"):
        lp.differentiable(torch.zeros(1, 3, 15, 32, device=dev), torch.zeros(1, 3, 15, 32, device=dev))
    with pytest.raises(RuntimeError, match="HIP device only"):
        lp.differentiable(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    p, t = lr.make_images(2, 16, 16, seed=11, low_contrast=True)
    pd, td = p.to(dev).requires_grad_(True), t.to(dev)
    lp.differentiable(pd, td).sum().backward()                                          # first call: allocations, library set-up
    pd.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                             # it reads nothing on the host
    try:
        lp.differentiable(pd, td).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(pd.grad).all())
