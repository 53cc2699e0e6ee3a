"""The yardsticks of tests/summaries_ref.py against the reference's own output (tests/golden/summaries.npz), the rules of
coponerf_amd.summaries.make_grid on CPU tensors, and the caps the GPU tests of the flow panels rely on, asserted for the
reference's own fp32 arithmetic.  No GPU."""
import os

import numpy as np
import pytest
import torch

from coponerf_amd import summaries as sm
from tests import ssim_ref
from tests import summaries_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "summaries.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def stock():
    model_input, model_output = sr.inputs()
    S = sr.FIXTURE["S"]
    return sr.stock_summaries(model_input, model_output, (S, S))


def test_stock_restatement_reproduces_the_reference(golden, stock):
    """Scalars to 1e-6 relative; the sampled image values to 1 ulp (they come out equal: the restatement calls the same
    library functions in the same order)."""
    images, scalars = stock
    assert set(images) == set(sr.IMAGE_TAGS) == {k[:-6] for k in golden if k.endswith("_shape")}
    assert {"scalar_" + k for k in scalars} == {k for k in golden if k.startswith("scalar_")}
    for tag, value in scalars.items():
        want = float(golden["scalar_" + tag])
        print(tag, float(value), want)
        assert abs(float(value) - want) <= 1e-6 * abs(want), tag
    for tag, (img, normalize, scale_each) in images.items():
        assert tuple(img.shape) == tuple(golden[tag + "_shape"]), tag
        assert [normalize, scale_each] == golden[tag + "_flags"].tolist(), tag
        got = img.reshape(-1)[torch.from_numpy(sr.positions(tag, img.numel()))].numpy()
        want = golden[tag + "_values"]
        ulp = np.spacing(np.abs(want).astype(np.float32))
        worst = float(np.max(np.abs(got.astype(np.float64) - want) / ulp))
        print(tag, "largest difference in ulp", worst)
        assert worst <= 1.0, tag
        assert np.array_equal(golden[tag + "_range"], [float(img.min()), float(img.max())]), tag


def test_jet_table_is_the_fixtures_colour_map(golden):
    """Every colour the reference's matplotlib call produced on the fixture's depths is an entry of the closed-form table (or
    the `bad` colour), at the index of matplotlib's float32 arithmetic."""
    _, model_output = sr.inputs()
    S = sr.FIXTURE["S"]
    want = golden["depth_images_values"]
    got = sr.jet_lookup(model_output["depth_ray"].reshape(-1, S, S).numpy()).transpose(0, 3, 1, 2).astype(np.float32)
    assert np.array_equal(got.reshape(-1)[sr.positions("depth_images", got.size)], want)
    table = sm.jet_table()
    assert table.shape == (256, 3) and table[0].tolist() == [0.0, 0.0, 0.5] and table[255].tolist() == [0.5, 0.0, 0.0]
    edges = np.array([0.0, 10.0, np.nextafter(np.float32(10), np.float32(np.inf)), -0.5, 12.0, np.nan], dtype=np.float32)
    assert np.array_equal(sr.jet_lookup(edges), np.stack([table[0], table[255], table[255], table[0], table[255], np.zeros(3)]))


def test_coords32_is_the_upsample_to_rounding():
    """The explicit fp32 sequence against F.interpolate on the CPU, whose vector kernels contract some of the operations: the
    same values to a few ulp of the largest flow, and the same tap indices and weights inside (checked through the values)."""
    for B, S, s in sr.PANEL_CASES:
        _, f0, _, _ = sr.panel_case(B, S, s)
        up, coords = sr.coords32(f0, S)
        stock_up = ssim_ref.upsample(f0, S, S)
        assert float((up - stock_up).abs().max()) <= 4 * sr.U * float(stock_up.abs().max())
        assert float((coords - ssim_ref.unnormalised_coords(stock_up)).abs().max()) <= sr.coord_bound((f0,), S)


@pytest.mark.parametrize("N", [1, 2, 8, 9])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("scale_each", [False, True])
def test_make_grid_rules(N, C, scale_each):
    H, W = 5, 7
    g = torch.Generator().manual_seed(10 * N + C)
    x = torch.randn(N, C, H, W, generator=g) * 3 + 1
    if N > 1:
        x[1] = 2.5                                          # a constant image: max == min when scaled on its own
    grid = sm.make_grid(x, normalize=True, scale_each=scale_each)
    x3 = x.expand(N, 3, H, W)
    if scale_each:
        lo, hi = x3.amin(dim=(1, 2, 3), keepdim=True), x3.amax(dim=(1, 2, 3), keepdim=True)
    else:
        lo, hi = x3.min(), x3.max()
    want = (x3 - lo) / (hi - lo + 1e-5)
    if N == 1:
        assert grid.shape == (3, H, W)                      # a single image comes back as it is, without padding
        assert torch.allclose(grid, want[0], rtol=0, atol=1e-6)
        return
    xmaps = min(8, N)
    ymaps = -(-N // xmaps)
    assert grid.shape == (3, ymaps * (H + 2) + 2, xmaps * (W + 2) + 2)
    covered = torch.zeros_like(grid, dtype=torch.bool)
    for k in range(N):
        y0, x0 = (k // xmaps) * (H + 2) + 2, (k % xmaps) * (W + 2) + 2
        assert torch.allclose(grid[:, y0:y0 + H, x0:x0 + W], want[k], rtol=0, atol=1e-6), k
        covered[:, y0:y0 + H, x0:x0 + W] = True
    assert bool((grid[~covered] == 0).all())                # padding and the empty cells of the last row: pad_value 0
    assert float(grid.min()) >= 0.0 and float(grid.max()) <= 1.0
    if scale_each:
        assert bool((grid[:, 2:2 + H, (W + 2) + 2:(W + 2) + 2 + W] == 0).all())        # the constant image: 0 / 1e-5
    plain = sm.make_grid(x, normalize=False)
    assert torch.equal(plain[:, 2:2 + H, 2:2 + W], x3[0])
    with pytest.raises(ValueError):
        sm.make_grid(torch.zeros(2, 2, H, W))


@pytest.mark.parametrize("B,S,s", sr.PANEL_CASES)
def test_reference_arithmetic_keeps_the_caps_of_the_gpu_tests(B, S, s):
    """For the reference's own fp32 stock ops against the float64 form at THEIR sampling coordinates: at most 0.5 % of the
    pixels lie within 1e-3 px of a mask threshold (measured: 0 - 0.03 %), the masks agree everywhere else, both outcomes
    occur (24 - 71 % true), and outside that band the overlay differs from the float64 chain by at most one grey level on at
    most 1 % of its elements (measured: 0 - 0.0004 %).  The warped values are printed, not held to WARP_BOUND: the CPU
    library contracts parts of its coordinate arithmetic, so its coordinates are not the ones given here to the last bit."""
    rgb, f0, f1, _ = sr.panel_case(B, S, s)
    coords = tuple(ssim_ref.unnormalised_coords(ssim_ref.upsample(f, S, S)) for f in (f0, f1))
    ref = sr.panels64(rgb, f0, f1, coords)
    warped, mask, overlay, _ = sr.stock_panels(rgb, f0, f1)
    fig = sr.compare_panels(warped, mask, overlay, ref)
    print(fig, "WARP_BOUND", sr.WARP_BOUND, "with coordinates", sr.fixture_warp_bound((f0, f1), S))
    assert fig["band"] <= 0.005
    assert fig["mask_mismatch"] == 0
    assert 0.2 <= fig["true"] <= 0.75
    assert fig["overlay_max"] <= 1 and fig["overlay_share"] <= 0.01
    assert fig["warped_err"] <= sr.fixture_warp_bound((f0, f1), S)
    assert torch.equal(overlay, sr.overlay_rule(warped, mask))


def test_overlay_rule_is_the_reference_function():
    """overlay_rule against a literal transcription of the numpy arithmetic (float64 blend, assignment into uint8)."""
    g = torch.Generator().manual_seed(3)
    warped = torch.rand(6, 9, 3, generator=g) * 255.0
    warped[0, 0] = torch.tensor([0.0, 254.99998, 255.0])
    mask = torch.rand(6, 9, generator=g) > 0.5
    im = np.asarray(warped.numpy(), dtype=np.uint8)
    ann = np.asarray(255 - mask.numpy() * 255, dtype=np.uint8)
    fg = im * 0.5 + 0.5 * np.asarray(sr.COLOR, dtype=np.uint8)
    want = im.copy()
    want[ann > 0] = fg[ann > 0]
    assert np.array_equal(sr.overlay_rule(warped, mask).numpy(), want)


@pytest.mark.parametrize("rows,S", sr.ENTROPY_SHAPES)
def test_fp32_entropy_lies_within_the_bound_of_float64(rows, S):
    for name, w in sr.entropy_cases(rows, S).items():
        for flag in (False, True):
            got, want = float(sr.entropy(w, flag)), float(sr.entropy64(w, flag))
            if name == "nanrow" and not flag:
                assert got != got and want != want
                continue
            print(name, flag, got, want, abs(got - want), sr.entropy_bound(w))
            assert abs(got - want) <= sr.entropy_bound(w), (name, flag)


def test_wrappers_refuse_host_tensors():
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.attention_entropy(torch.rand(3, 4))
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.depth_colors(torch.rand(5))
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.flow_panels(torch.rand(1, 2, 8, 8, 3), (torch.rand(1, 2, 4, 4), torch.rand(1, 2, 4, 4)))
    with pytest.raises(TypeError):
        sm.depth_colors([1.0, 2.0])


def test_entry_points_check_arguments_before_any_launch():
    from coponerf_amd import _hip
    lib = _hip.lib()
    assert lib.cpn_flow_panels(None, None, None, 1, 8, 4, None, None, None, None) == -1 and b"null" in lib.cpn_last_error()
    assert lib.cpn_flow_panels(16, 16, 16, 1, 4, 8, 16, 16, 16, None) == -2 and b"S >= h" in lib.cpn_last_error()
    assert lib.cpn_flow_panels(16, 16, 16, 40000, 8, 4, 16, 16, 16, None) == -2
    assert lib.cpn_depth_jet(None, 4, None, None, None) == -1
    assert lib.cpn_depth_jet(16, 0, 16, 16, None) == -2
    assert lib.cpn_attention_entropy(None, 4, 4, 0, None, None, None) == -1
    assert lib.cpn_attention_entropy(16, 0, 4, 0, 16, 16, None) == -2 and lib.cpn_attention_entropy(16, 4, 0, 0, 16, 16, None) == -2
    assert [lib.cpn_attention_entropy_blocks(r) for r in (0, 1, 32, 33, 65536)] == [0, 1, 1, 2, 2048]
