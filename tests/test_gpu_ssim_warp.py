"""The flow-warp SSIM term on the MI355X (csrc/ssim_warp.hip through coponerf_amd.losses) against float64, the stock fp32
composition and upstream's own numbers (tests/golden/ssim.npz, made by tests/golden/make_golden_ssim.py).

Bars.  The float64 yardstick (tests/ssim_ref.ref64_loss) runs at the KERNEL's fp32 sampling coordinates lifted to float64, so
a tap pair can never differ between the two.  The kernel may then be as far from it as 4 x the stock fp32 composition is on
the same inputs (the separable window rounds differently from upstream's rounded 11 x 11 outer product, and the sums run in
another order: at most a factor 2 each), with floors of 2^-22 for the loss and 2^-18 relative L2 for dflow (64 fp32
roundings on one pixel's path: two 11-term window sums per moment, the quotient, the adjoint sums, the taps); a worst dflow
entry may be 4 x its relative-L2 bar of max |want|.  Against upstream's fixture, which ran ATen-CPU's coordinates, the bars
are twice those.  The yardstick is the stock composition, never the kernel.

Shapes: 8 x 12 at s = 1 (the window overhangs the image on both sides), 48 x 48 at s = 2, 40 x 72 at s = 4 (not square, ragged
tiles), the fixture's 2 x 256 x 256 at s = 4.
"""
import functools
import os

import numpy as np
import pytest
import torch

from coponerf_amd import dist as cdist
from coponerf_amd import losses
from tests import ssim_ref as R
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

FLOOR_LOSS, FLOOR_L2 = 2.0 ** -22, 2.0 ** -18
COORD_BAR = 2.0 ** -13          # px: at most 8 roundings of quantities below 512, each <= 2^-16

SHAPES = {"8x12s1": (1, 8, 12, 1), "48x48s2": (1, 48, 48, 2), "40x72s4": (1, 40, 72, 4), "fixture": (2, 256, 256, 4)}
CASES = [
    ("8x12s1", "recipe", "all"), ("8x12s1", "far", "all"), ("8x12s1", "rim", "checker"), ("8x12s1", "zero", "all"),
    ("48x48s2", "recipe", "checker"), ("48x48s2", "rim", "all"),
    ("40x72s4", "recipe", "own"), ("40x72s4", "far", "checker"), ("40x72s4", "zero", "checker"), ("40x72s4", "rim", "all"),
    ("fixture", "recipe", "fixture"),
]


def dev():
    return torch.device("cuda:0")


def fixture():
    return np.load(os.path.join(GOLDEN, "ssim.npz"))


def flows(kind, B, H, W, s, f0, f1):
    h, w = H // s, W // s
    if kind == "recipe":
        return f0, f1
    if kind == "zero":
        return torch.zeros_like(f0), torch.zeros_like(f1)
    if kind == "far":                                  # every tap outside the image: zero value, zero gradient
        return torch.full_like(f0, 1e4), torch.full_like(f1, -1e4)
    # rim: targets between -1 and 0 and between W - 1 and W (rows alternate; the same in y by columns): partial taps
    xc = (torch.arange(w, dtype=torch.float32) + 0.5) * s - 0.5
    yc = (torch.arange(h, dtype=torch.float32) + 0.5) * s - 0.5
    rows, cols = torch.arange(h) % 2 == 0, torch.arange(w) % 2 == 0
    tx = torch.where(rows, torch.tensor(-0.5), torch.tensor(W - 0.5))[:, None].expand(h, w)
    ty = torch.where(cols, torch.tensor(-0.4), torch.tensor(H - 0.6))[None, :].expand(h, w)
    f = torch.stack(((tx - xc[None, :]) / s, (ty - yc[:, None]) / s))[None].expand(B, -1, -1, -1).contiguous()
    return f, (f * 0.5 + f1 * 0.1).contiguous()


def make_masks(kind, B, H, W, s, f0, f1):
    if kind == "all":
        return torch.ones(B, 2, H, W, dtype=torch.bool)
    if kind == "none":
        return torch.zeros(B, 2, H, W, dtype=torch.bool)
    if kind == "checker":
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        return (((ys + xs) % 2) == 0)[None, None].expand(B, 2, H, W).contiguous()
    if kind == "fixture":
        fx = fixture()
        return torch.stack([R.unpack_mask(fx[f"mask{d}"], (B, H, W)) for d in (0, 1)], 1)
    return torch.stack(R.masks_of(f0, f1, H, W), 1)


def run_kernel(rgb, f0, f1, masks):
    """(loss (2,), coords, sums, d loss_d / d f_d) of the HIP path."""
    a = f0.to(dev()).requires_grad_(True)
    b = f1.to(dev()).requires_grad_(True)
    loss, coords, sums = losses.ssim_warp_terms(rgb.to(dev()), a, b, masks.to(dev()))
    (loss[0] + loss[1]).backward()
    return loss.detach(), coords, sums, (a.grad, b.grad)


@functools.lru_cache(maxsize=None)
def measured(shape, fkind, mkind):
    """One case: the kernel, the float64 yardstick at the kernel's lifted coordinates, the stock composition's gap to it."""
    B, H, W, s = SHAPES[shape]
    rgb, f0, f1 = R.case(B, H, W, s)
    f0, f1 = flows(fkind, B, H, W, s, f0, f1)
    masks = make_masks(mkind, B, H, W, s, f0, f1)
    loss, coords, sums, grads = run_kernel(rgb, f0, f1, masks)
    coords = coords.view(B, 2, 2, H, W)
    rows = []
    for d, f in enumerate((f0, f1)):
        want_loss, want_g = R.ref64_loss(rgb, f, masks[:, d], d, coords[:, d])
        leaf = f.to(dev()).requires_grad_(True)
        sl = R.stock_loss(rgb.to(dev()), leaf, masks[:, d].to(dev()), d)
        sg, = torch.autograd.grad(sl, leaf)
        rows.append(dict(want_loss=float(want_loss), want_g=want_g, loss=float(loss[d]), g=grads[d].cpu(),
                         gap_loss=abs(float(sl.detach()) - float(want_loss)),
                         gap_l2=R.rel_l2(sg, want_g) if float(want_g.norm()) > 0 else 0.0))
    return dict(rgb=rgb, f=(f0, f1), masks=masks, coords=coords, sums=sums.cpu(), rows=rows)


def check_direction(tag, row, relax=1.0, want_loss=None, want_g=None):
    want_loss = row["want_loss"] if want_loss is None else want_loss
    want_g = row["want_g"] if want_g is None else want_g
    bar_loss = relax * max(4 * row["gap_loss"], FLOOR_LOSS)
    bar_l2 = relax * max(4 * row["gap_l2"], FLOOR_L2)
    e_loss = abs(row["loss"] - want_loss)
    if float(want_g.norm()) == 0:
        e_l2 = e_max = float(row["g"].abs().max())                 # nothing to be relative to: the gradient must be zero too
        bar_l2 = 0.0
    else:
        e_l2, e_max = R.rel_l2(row["g"], want_g), R.rel_max(row["g"], want_g)
    print(f"[{tag}] loss {row['loss']:.9f} err {e_loss:.2e} (stock gap {row['gap_loss']:.2e}, bar {bar_loss:.2e}); "
          f"dflow relL2 {e_l2:.2e} worst {e_max:.2e} (stock gap {row['gap_l2']:.2e}, bar {bar_l2:.2e})")
    assert e_loss <= bar_loss, (tag, e_loss, bar_loss)
    assert e_l2 <= bar_l2 and e_max <= 4 * bar_l2, (tag, e_l2, e_max, bar_l2)


@pytest.mark.parametrize("shape,fkind,mkind", CASES)
def test_coordinates_follow_atens_fp32_expression(shape, fkind, mkind):
    m = measured(shape, fkind, mkind)
    B, H, W, s = SHAPES[shape]
    for d in (0, 1):
        want = R.unnormalised_coords(R.upsample(m["f"][d], H, W))          # ATen on the CPU, fp32
        err = float((m["coords"][:, d].cpu() - want).abs().max())
        scale = max(1.0, float(want.abs().max()) / 512)                    # the +-1e4 flows: the same roundings of larger numbers
        print(f"[{shape} {fkind} d{d}] coords max |diff| {err:.2e} px (bar {COORD_BAR * scale:.2e})")
        assert err <= COORD_BAR * scale


@pytest.mark.parametrize("shape,fkind,mkind", CASES)
def test_forward_and_backward_against_float64(shape, fkind, mkind):
    m = measured(shape, fkind, mkind)
    B = SHAPES[shape][0]
    for d in (0, 1):
        check_direction(f"{shape} {fkind} {mkind} d{d}", m["rows"][d])
        if fkind == "far":
            assert float(m["rows"][d]["g"].abs().max()) == 0.0
    # the per-item sums add up to the direction's loss (upstream normalises a direction over the whole batch)
    sums = m["sums"].view(B, 2, 2).double()
    for d in (0, 1):
        tot = sums[:, d].sum(0)
        assert abs(float(tot[0] / tot[1] / 3) - m["rows"][d]["loss"]) <= 2.0 ** -22


def test_fixture_of_upstream():
    """Upstream's own loss and gradients (ATen-CPU coordinates, not the kernel's) at twice the bars of the float64 test.  A
    tap pair that flips between the two coordinate sets would show here as one cell: it is printed, the bar is not widened."""
    fx = fixture()
    m = measured("fixture", "recipe", "fixture")
    got = (m["rows"][0]["loss"] + m["rows"][1]["loss"]) / 2
    bar = 2 * max(4 * max(r["gap_loss"] for r in m["rows"]), FLOOR_LOSS)
    print(f"ssim_loss {got:.9f} vs upstream {float(fx['ssim_loss']):.9f} (bar {bar:.2e})")
    assert abs(got - float(fx["ssim_loss"])) <= bar
    for d in (0, 1):
        want = 2 * torch.from_numpy(fx[f"dflow{d}"]).double()              # the fixture differentiates (L0 + L1) / 2
        diff = (m["rows"][d]["g"].double() - want).abs()
        cell = np.unravel_index(int(diff.argmax()), tuple(diff.shape))
        print(f"d{d}: worst cell {cell}: {float(diff.max()):.2e} of max |want| {float(want.abs().max()):.2e}")
        check_direction(f"fixture vs upstream d{d}", m["rows"][d], relax=2.0, want_loss=m["rows"][d]["loss"], want_g=want)


def test_two_runs_give_equal_bits():
    B, H, W, s = SHAPES["40x72s4"]
    rgb, f0, f1 = R.case(B, H, W, s)
    masks = make_masks("own", B, H, W, s, f0, f1)
    a, b = run_kernel(rgb, f0, f1, masks), run_kernel(rgb, f0, f1, masks)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[3][0], b[3][0]) and torch.equal(a[3][1], b[3][1])
    m = measured("fixture", "recipe", "fixture")
    again = run_kernel(m["rgb"], m["f"][0], m["f"][1], m["masks"])
    assert [float(x) for x in again[0]] == [r["loss"] for r in m["rows"]]
    assert torch.equal(again[3][0].cpu(), m["rows"][0]["g"]) and torch.equal(again[3][1].cpu(), m["rows"][1]["g"])


def test_empty_mask_is_nan_and_the_guard_skips():
    B, H, W, s = SHAPES["40x72s4"]
    rgb, f0, f1 = R.case(B, H, W, s)
    loss, _, _, grads = run_kernel(rgb, f0, f1, make_masks("none", B, H, W, s, f0, f1))
    assert bool(torch.isnan(loss).all())
    for g in grads:
        assert not bool(torch.isfinite(g).any())
    p = torch.nn.Parameter(torch.zeros_like(grads[0]))
    p.grad = grads[0]
    ok, _, _ = cdist.guard_on_device([p], 1.0)
    assert float(ok) == 0.0


def test_autograd_with_the_flows_own_masks():
    """ssim_warp_loss(masks=None) on the fixture's flows as leaves: the masks the product derives are the fixture's, bit for
    bit, and the gradients are upstream's at the fixture test's bars."""
    from coponerf_amd.aux_outputs import cycle_masks
    fx = fixture()
    m = measured("fixture", "recipe", "fixture")
    B, H, W, s = SHAPES["fixture"]
    f0 = m["f"][0].to(dev()).requires_grad_(True)
    f1 = m["f"][1].to(dev()).requires_grad_(True)
    with torch.no_grad():
        m0, m1 = cycle_masks((f0, f1), f0.shape[2])
    assert torch.equal(m0.cpu(), m["masks"][:, 0]) and torch.equal(m1.cpu(), m["masks"][:, 1])
    loss = losses.ssim_warp_loss(m["rgb"].to(dev()), f0, f1)
    loss.backward()
    bar = 2 * max(4 * max(r["gap_loss"] for r in m["rows"]), FLOOR_LOSS)
    assert abs(float(loss) - float(fx["ssim_loss"])) <= bar
    for d, f in enumerate((f0, f1)):
        want = torch.from_numpy(fx[f"dflow{d}"])
        bar_l2 = 2 * max(4 * m["rows"][d]["gap_l2"], FLOOR_L2)
        e_l2, e_max = R.rel_l2(f.grad, want), R.rel_max(f.grad, want)
        print(f"d{d}: relL2 {e_l2:.2e} worst {e_max:.2e} (bar {bar_l2:.2e})")
        assert e_l2 <= bar_l2 and e_max <= 4 * bar_l2


def test_unsupported_shapes_are_status_codes():
    rgb, f0, f1 = R.case(1, 48, 48, 2)
    masks = torch.ones(1, 2, 48, 48, dtype=torch.bool)
    bad = torch.zeros(1, 2, 16, 16)                                       # scale 3
    with pytest.raises(RuntimeError, match="cpn_ssim_warp"):
        losses.ssim_warp_terms(rgb.to(dev()), bad.to(dev()), bad.to(dev()), masks.to(dev()))
