"""tests/lpips_grad_ref.py pinned on the CPU: its closed-form adjoints equal float64 autograd through tests/lpips_ref.py, its
one own rule (gradient 0 at an all-zero prediction vector, where autograd gives NaN) is what it says, and every seeded
defect exceeds the bounds of tests/test_gpu_lpips_grad.py at least 100 times on that test's own cases - the bounds catch
something."""
import pytest
import torch

from tests import lpips_grad_ref as gr
from tests import lpips_ref as lr

REL = 1e-12


def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("kind", ["unit", "large", "tiny"])
@pytest.mark.parametrize("hw", gr.HEAD_HW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", gr.HEAD_C)
def test_head_closed_form_is_autograd(C, hw, kind):
    N = 3
    feat, lin, g = gr.head_case(N, C, hw[0], hw[1], kind)
    want = gr.head_grad_autograd(feat, lin, N, g)
    got, terms = gr.head_grad_closed(feat, lin, N, g)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    # the projection cancels the radial part of r u: relative to the terms it is made of
    assert float(((got - want).abs() / terms).max()) <= REL and rel_err(got, want) <= REL
    assert bool((got.abs() <= terms * (1 + 1e-12)).all())


def test_head_zero_vector_rule():
    N, C, h, w = 3, 64, 5, 7
    feat, lin, g = gr.head_case(N, C, h, w, "zeros")
    auto = gr.head_grad_autograd(feat, lin, N, g).view(N, h * w, C)
    got, terms = (x.view(N, h * w, C) for x in gr.head_grad_closed(feat, lin, N, g))
    zero = torch.zeros(N, h * w, dtype=torch.bool)
    for n, pix in gr.zero_pixels(N, h, w):
        zero[n, pix] = True
        assert bool(torch.isnan(auto[n, pix]).all())                    # autograd: NaN over the whole pixel
        assert bool((got[n, pix] == 0).all()) and bool((terms[n, pix] == 0).all())
    assert int(zero.sum()) == 2
    rest = ~zero
    assert bool(torch.isfinite(auto[rest]).all())                       # a zero vector in the TARGET alone is no special case
    assert float(((got[rest] - auto[rest]).abs() / terms[rest]).max()) <= REL


@pytest.mark.parametrize("hw", gr.STEM_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stem_closed_form_is_autograd(hw):
    N = 2
    p, y, dy = gr.stem_case(N, *hw)
    w, _ = gr.stem_weights()
    want = gr.stem_grad_autograd(p, y, dy, w)
    got, terms = gr.stem_grad_closed(p, y, dy, w)
    assert float(((got - want).abs() / terms.clamp_min(1e-300)).max()) <= REL
    out = (p.abs() > 1) | torch.isnan(p)
    assert int(out.sum()) > 10 and bool((got[out] == 0).all())          # outside the clamp and at a NaN: exactly 0
    assert bool((got[p.abs() == 1] != 0).all()) and int((p.abs() == 1).sum()) >= 3      # the bounds are inclusive
    assert 0.2 < float((y > 0).float().mean()) < 0.8


def test_end_to_end_reference_is_lpips_ref():
    """lpips_grad64 writes the trunk out to reach the gradient of relu1_1; its VALUE is lpips_ref.lpips64's."""
    p, t = lr.make_images(2, 16, 16, seed=11, low_contrast=True)
    want = lr.lpips64(p, t, gr.SEED)[0]
    got, grad, mag = gr.lpips_grad64(p, t, gr.SEED)
    assert float(((got - want).abs() / want).max()) <= REL
    assert grad.shape == p.shape and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    assert bool((grad.abs() <= mag * (1 + 1e-9)).all())


def head_cases():
    return [(N, C, h, w, kind) for kind in gr.HEAD_KINDS for C in gr.HEAD_C for (h, w) in gr.HEAD_HW for N in gr.HEAD_N]


@pytest.mark.parametrize("defect", gr.HEAD_DEFECTS)
def test_head_defects_exceed_the_gpu_bound(defect):
    worst = float("inf")
    for N, C, h, w, kind in head_cases():
        if defect == "no_pixel_mean" and h * w == 1:
            continue                                                    # the mean over one pixel is the pixel
        feat, lin, g = gr.head_case(N, C, h, w, kind)
        good, terms = gr.head_grad_closed(feat, lin, N, g)
        bad, _ = gr.head_grad_closed(feat, lin, N, g, defect)
        live = terms > 0                                                # `zeros`: the pixels whose gradient is not 0 by rule
        if not bool(live.any()):
            continue                                                    # 1 x 1 with N = 1: the one prediction vector is zero
        ratio = float(((bad - good).abs()[live] / (gr.K_HEAD_BWD * gr.U * terms[live])).max())
        worst = min(worst, ratio)
    print(f"{defect}: at least {worst:.3g} x the bound")
    assert worst >= 100


@pytest.mark.parametrize("defect", gr.STEM_DEFECTS)
def test_stem_defects_exceed_the_gpu_bound(defect):
    w, _ = gr.stem_weights()
    worst = float("inf")
    for hw in gr.STEM_HW:
        p, y, dy = gr.stem_case(2, *hw)
        good, terms = gr.stem_grad_closed(p, y, dy, w)
        bad, bad_terms = gr.stem_grad_closed(p, y, dy, w, defect)
        bound = gr.K_STEM_BWD * gr.U * torch.maximum(terms, bad_terms).clamp_min(1e-300)
        ratio = float(((bad - good).abs() / bound).max())
        worst = min(worst, ratio)
    print(f"{defect}: at least {worst:.3g} x the bound")
    assert worst >= 100
