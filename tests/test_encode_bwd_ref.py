"""The float64 references of tests/encode_bwd_ref.py pinned against ATen's grid_sample and against the row order of the
forward tests - on the CPU, so the GPU tests of the table-form backward compare with something that was itself checked."""
import pytest
import torch

from oracle.render_ref import gather_levels
from tests import encode_bwd_ref as ref


def _table_form(z, g, kind, img, H, W):
    """sum_t a_t node_features_ref[node_t] of every sample: the layer's coarse input in its table form, float64."""
    feat = ref.node_features_ref(z[0], z[1], z[2], H, W)
    nodes, wts = ref.node_taps_ref(g, kind, H, W)
    per = ref.table_nodes(H, W)
    out = torch.zeros(g.shape[0], 768, dtype=torch.float64)
    for k in range(4):
        out += wts[:, k:k + 1] * feat[img * per + nodes[:, k]]
    return out


def _coordinate_rounding_bound(z, H, W):
    """dt_x Sx + dt_y Sy: the node position's fp32 rounding (2^-23 * M / 2: g + 1 < 4) times the steepest slope of any
    level's interpolant per node, adjacent texel difference (zero padded: the rim) over the level's pitch."""
    sx = sy = 0.0
    for l, t in enumerate(z):
        p = 8 >> l
        tp = torch.nn.functional.pad(t, (1, 1, 1, 1))
        sx = max(sx, float((tp[..., :, 1:] - tp[..., :, :-1]).abs().max()) / p)
        sy = max(sy, float((tp[..., 1:, :] - tp[..., :-1, :]).abs().max()) / p)
    return 2.0 ** -23 * (W // 4) * sx + 2.0 ** -23 * (H // 4) * sy


@pytest.mark.parametrize("H,W", [(32, 32), (64, 64), (32, 64)])
@pytest.mark.parametrize("coords", ["random", "hostile"])
def test_table_form_equals_grid_sample(H, W, coords):
    """Four taps of the node tables reproduce grid_sample on the three coarse levels, for both paddings.

    Tolerance 1e-6 max|z| (the issue's figure).  Both sides hold float64 VALUES; they differ in the coordinate: node_taps_ref
    forms the node position t = (g + 1) * (M / 2) in fp32, grid_sample (float64 here) in float64.  g + 1 is rounded once, by
    at most 2^-24 where |g + 1| < 2 (inside the map and on its rim up to node M; 2^-23 beyond, where only the fading zero
    rim is left), and M / 2 <= 16 is a power of two: dt <= 2^-24 * 16 = 9.5e-7 nodes per axis.  The interpolant of level l is
    piecewise bilinear with a texel pitch of p = 8, 4, 2 nodes, so |dv/dt| <= max|dz| / p <= max|dz| / 2 per axis, dz the
    difference of adjacent texels (map border: z against 0).  The bound that follows, for ANY coordinates, is
    dt * (Sx + Sy) with Sx, Sy the largest adjacent differences over the pitch: the test computes it from its maps and asserts
    it as well (it is 1.2e-6 to 1.4e-6 max|z| for standard normal maps at M = 32).  1e-6 max|z| is below that worst case: it
    holds for the seeded samples of this test (they reach 0.4e-6 to 0.8e-6 max|z|), not for every coordinate one could draw;
    a wrong tap or weight shows at 1e-2 max|z|.  The sample coordinates are drawn in float64 and rounded to fp32 so that
    g + 1 really rounds: fp32 draws of torch.rand are multiples of 2^-24, for which both sides agree to 1e-15.  Coordinates
    that fp32 represents with g + 1 exact (every hostile one: nodes, texel centres, +-1, the rim) agree to float64 rounding,
    asserted below at 1e-12."""
    gen = torch.Generator().manual_seed(H * 100 + W)
    N = 2
    z = ref.make_maps(N, H, W, gen)[:3]
    z = [t.double() for t in z]
    zmax = max(float(t.abs().max()) for t in z)
    if coords == "random":
        n = 4000
        # drawn in float64 and rounded: fp32 draws are multiples of 2^-24, for which g + 1 is exact and nothing is tested
        g = (torch.rand(n, 2, generator=gen, dtype=torch.float64) * 3 - 1.5).float()
    else:
        g = ref.hostile_coords(H, W)
        n = g.shape[0]
    for kind, padding in ((0, "border"), (1, "zeros")):
        img = torch.arange(n) % N
        got = _table_form(z, g, torch.full((n,), kind), img, H, W)
        want = torch.empty_like(got)
        for i in range(N):
            sel = img == i
            grid = g[sel].double().view(1, -1, 1, 2)
            want[sel] = gather_levels([t[i:i + 1] for t in z], grid, padding).reshape(-1, 768)
        err = float((got - want).abs().max())
        print(f"H={H} W={W} {coords} {padding}: max|table form - grid_sample| = {err:.3e} (max|z| = {zmax:.2f})")
        assert err <= 1e-6 * zmax, (padding, err)
        assert err <= _coordinate_rounding_bound(z, H, W), (padding, err)
        if coords == "hostile":
            exact = (g.abs() <= 2).all(1)                        # (1e10 + 1 is rounded; every other hostile g + 1 is exact)
            assert float((got - want)[exact].abs().max()) <= 1e-12 * zmax, padding
            assert int(exact.sum()) >= n - 5


def test_node_taps_weights_and_dummy_taps():
    """Weights are non-negative and sum to 1; a zero fraction leaves exactly the taps the kernel keeps; every node index
    is inside its table; 1e10 lands on the last cell with its whole weight on the far node."""
    H, W = 32, 64
    g = ref.hostile_coords(H, W)
    for kind in (0, 1):
        nodes, wts = ref.node_taps_ref(g, torch.full((len(g),), kind), H, W)
        nh, nw = ref.table_dims(H, W, kind)
        base = kind * ref.table_dims(H, W, 0)[0] * ref.table_dims(H, W, 0)[1]
        assert (wts >= 0).all() and torch.allclose(wts.sum(1), torch.ones(len(g), dtype=torch.float64), atol=1e-15)
        assert (nodes >= base).all() and (nodes < base + nh * nw).all()
        assert nodes[2, 3] == base + nh * nw - 1 and wts[2, 3] == 1.0             # (1e10, 1e10): the far corner node
        assert nodes[1, 2] == base + (nh - 1) * nw and wts[1, 2] == 1.0           # (-1e10, 1e10)


@pytest.mark.parametrize("B,R,S,ray0,nrays", ref.RAGGED + [(2, 7, 9, 0, 14)])
def test_row_table_is_the_forward_tests_row_order(B, R, S, ray0, nrays):
    """row_table reproduces the rows of x.permute(0, 2, 1, 3, 4, 5) in test_encode_hidden_against_torch (chunked as in
    test_encode_hidden_ragged_ranges): every entry of that tensor is tagged with (image read, kind, coordinate index)."""
    V = 2
    N = B * V
    tag = torch.arange(N * R * S).view(N, R, S, 1)
    imgs = torch.arange(N).view(N, 1, 1, 1).expand(N, R, S, 1)
    # what the forward tests do: 'prim' samples image n at pixel_val[n], 'sec' samples the swapped views at sec_grid[n]
    prim = torch.cat((imgs, torch.zeros_like(imgs), tag), -1).view(B, V, R, S, 3)
    swapped = imgs.view(B, V, R, S, 1).flip(1)
    sec = torch.cat((swapped, torch.ones_like(swapped), tag.view(B, V, R, S, 1)), -1)
    x = torch.stack((prim, sec), dim=4)                                                   # (B, V, R, S, 2, 3)
    x = x.permute(0, 2, 1, 3, 4, 5).reshape(B * R, V * S * 2, 3)[ray0:ray0 + nrays].reshape(-1, 3)
    rt = ref.row_table(B, V, R, S, ray0, nrays)
    assert rt["img"].shape[0] == nrays * V * S * 2
    assert torch.equal(rt["img"], x[:, 0]) and torch.equal(rt["kind"], x[:, 1]) and torch.equal(rt["src"], x[:, 2])
    # and the header's formula, row by row
    row = (((rt["b"] * R + rt["r"] - ray0) * V + rt["v"]) * S + rt["s"]) * 2 + rt["kind"]
    assert torch.equal(row, torch.arange(row.shape[0]))


def test_gather_rows_ref_f32_is_the_forward_tests_input():
    """encode_input_ref(float32), which test_encode_hidden_against_torch and test_encode_hidden_ragged_ranges now call, is
    the construction those tests spelled out before (restated here: grid_sample on the own view with 'border', on the
    swapped views with 'zeros', concatenated with the point encoding, rows permuted); its float64 form (lifted grids) differs
    from it by fp32 blending only."""
    gen = torch.Generator().manual_seed(3)
    B, V, R, S, H = 2, 2, 5, 7, 32
    N = B * V
    z = ref.make_maps(N, H, H, gen)
    pv, sg = ref.random_coords(N, R, S, gen)
    ref.plant_hostile(pv, sg, H, H, gen)
    pe = torch.rand(N, R, S, 6, generator=gen) * 2 - 1
    prim = gather_levels(z, pv, "border").view(B, V, R, S, 832)
    z_swapped = [t.view(B, V, *t.shape[1:]).flip(1).reshape(t.shape) for t in z]
    sec = gather_levels(z_swapped, sg, "zeros").view(B, V, R, S, 832)
    pe5 = pe.view(B, V, R, S, 6)
    x = torch.stack((torch.cat((prim, pe5[..., 0:3]), -1), torch.cat((sec, pe5[..., 3:6]), -1)), dim=4)
    x = x.permute(0, 2, 1, 3, 4, 5).reshape(-1, 835)
    x32 = ref.encode_input_ref(z, pv, sg, pe, B, V, R, S, torch.float32)
    assert torch.equal(x32, x)
    x64 = ref.encode_input_ref(z, pv, sg, pe, B, V, R, S)
    zmax = max(float(t.abs().max()) for t in z)
    # fp32 blend of four fp16-exact texels: (1 - f) twice, a product and four multiply-adds, each 2^-24 relative
    assert float((x64 - x.double()).abs().max()) <= 8 * ref.U32 * zmax


def test_level_taps_and_level3_adjoint_agree():
    """The explicit level taps (used for term counts) and autograd through grid_sample (the reference gradient) are the
    same operator on the full-resolution level."""
    gen = torch.Generator().manual_seed(11)
    B, V, R, S, H, W = 2, 2, 7, 9, 32, 64
    ray0, nrays = 3, 9
    pv, sg = ref.random_coords(B * V, R, S, gen)
    ref.plant_hostile(pv, sg, H, W, gen)
    rt = ref.row_table(B, V, R, S, ray0, nrays)
    d = torch.randn(nrays * V * S * 2, 64, generator=gen, dtype=torch.float64)
    want = ref.level3_bwd_ref(d, H, W, pv, sg, B, V, R, S, ray0, nrays)
    tex, wts = ref.level_taps_ref(ref.row_coords(rt, pv, sg), rt["kind"], H, W)
    got = torch.zeros(B * V * H * W, 64, dtype=torch.float64)
    for k in range(4):
        got.index_add_(0, rt["img"] * H * W + tex[:, k], wts[:, k:k + 1] * d)
    got = got.view(B * V, H, W, 64).permute(0, 3, 1, 2)
    assert float((got - want).abs().max()) <= 1e-12 * float(d.abs().max()) * 16


def test_node_features_matrix_is_node_features_ref():
    gen = torch.Generator().manual_seed(2)
    H, W = 32, 64
    z = ref.make_maps(1, H, W, gen)
    feat = ref.node_features_ref(z[0], z[1], z[2], H, W)
    for lvl in range(3):
        A = ref.node_features_matrix(lvl, H, W)
        want = A @ z[lvl][0].double().reshape(256, -1).t()
        assert float((feat[:, lvl * 256:(lvl + 1) * 256] - want).abs().max()) <= 1e-12
