"""Parity of the HIP render path with the CPU oracle — runs on a real MI355X (`pytest -m gpu`).

Every compute call goes through the C ABI of coponerf_amd/libcoponerf_hip.so; the oracle
(oracle/render_ref.py) is only the checker.  Bars (BASELINE.json north_star):
  * sample coordinates / tap indices: bit-exact
  * rendered RGB: within 1e-3 abs
"""
import numpy as np
import pytest
import torch

from coponerf_amd import synthetic as syn
from tests.helpers import load_case, case_inputs, to_device, tap_indices

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-3          # north_star: "within 1e-3 abs on rendered RGB"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return syn.make_render_weights()


@pytest.fixture(scope="module")
def model(dev, weights):
    from coponerf_amd import CoPoNeRF
    m = CoPoNeRF.CoPoNeRF(n_view=2)
    missing, unexpected = m.load_state_dict(weights, strict=False)
    assert not unexpected
    return m.to(dev).eval()


def run_pair(model, dev, weights, cfg):
    from oracle import render_ref as orc
    inp, z, rel, flow = case_inputs(cfg)
    with torch.no_grad():
        ref = orc.forward(inp, z, rel, flow, cfg["val"], weights, npoints=cfg["S"], keep=True)
        model.npoints = cfg["S"]
        out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=cfg["val"],
                    flow=to_device(flow, dev), debug=True)
    return ref, out


@pytest.mark.parametrize("name", ["c1_val", "train_b2", "wide_val", "hd_val"])
def test_forward_parity(name, model, dev, weights):
    cfg, gold = load_case(name)
    ref, out = run_pair(model, dev, weights, cfg)
    core = out["_core"]
    B, R, S, H = cfg["B"], cfg["R"], cfg["S"], cfg["H"]
    # ---- indices: bit-exact against the oracle
    assert out["pixel_val"].device.type == "cpu"
    assert torch.equal(out["pixel_val"], ref["pixel_val"]), "pixel_val not bit-identical"
    assert torch.equal(core["coords"].cpu(), ref["coords"]), "Pluecker coords not bit-identical"
    sec = core["sec_grid"].cpu().view(B, 2, R, S, 2)                 # [b,v] = view-v samples seen from image 1-v
    assert torch.equal(sec[:, 1], ref["sec_grid"].view(B, 2, R, S, 2)[:, 0])
    assert torch.equal(sec[:, 0], ref["sec_grid"].view(B, 2, R, S, 2)[:, 1])
    assert torch.equal(core["pt"].cpu(), ref["pt"]), "closest points (float64 island) not bit-identical"
    assert torch.equal(out["valid_mask"].cpu(), ref["valid_mask"])
    for a, b in zip(tap_indices(out["pixel_val"], H), tap_indices(torch.from_numpy(gold["pixel_val"]), H)):
        assert int((a != b).sum()) == 0                               # vs the upstream reference itself: every tap index
    # ---- values
    assert (out["rgb"].cpu() - ref["rgb"]).abs().max() <= RGB_TOL
    assert (out["rgb"].cpu() - torch.from_numpy(gold["rgb"])).abs().max() <= RGB_TOL
    assert (out["at_wt"].cpu() - ref["at_wt"]).abs().max() <= 2e-3
    assert (core["z_local"].cpu() - ref["z_local"].reshape(-1, 416)).abs().max() <= 5e-3
    assert abs(float(out["at_wt"].view(B, 2, R, S).sum(dim=(1, 3)).mean()) - 1.0) < 1e-5
    assert (out["depth_ray"].cpu() - ref["depth_ray"]).abs().max() <= 2e-2
    assert out["at_wt_max"].dtype == torch.int64 and out["at_wt_max"].shape == (2 * B, R, 1)
    for k in ("rel_pose_flip", "gt_rel_pose", "gt_rel_pose_flip"):
        assert (out[k].cpu() - ref[k]).abs().max() <= 1e-5
    for k in ("mask_c2", "matchability_cycle_mask"):
        assert (out[k].cpu() != ref[k]).float().mean() <= 2e-2
    assert set(ref_keys()) <= set(out.keys())


def ref_keys():
    return ["flow", "coords", "uv", "pixel_val", "at_wts", "at_wt", "at_wt_max", "matchability_cycle_mask", "mask_c2",
            "T_to_C1_pts", "T_to_C2_pts", "C2_pts_to_C1", "depth_ray", "valid_mask", "rgb", "z", "rel_pose",
            "rel_pose_flip", "gt_rel_pose", "gt_rel_pose_flip"]


def test_stage_intermediates(model, dev, weights):
    """inter fixture: gathers / encoder / attention stages against the oracle AND the upstream intermediates."""
    cfg, gold = load_case("inter")
    ref, out = run_pair(model, dev, weights, cfg)
    core = out["_core"]
    assert torch.equal(out["pixel_val"], ref["pixel_val"])
    assert (core["rgb_raw"].cpu() - torch.from_numpy(gold["rgb_raw"]).reshape(-1, 3)).abs().max() <= RGB_TOL
    gpt = torch.from_numpy(gold["pt"])      # near-parallel lines: |pt| up to ~1e3, error grows with magnitude
    assert ((core["pt"].cpu() - gpt).abs() / (1 + gpt.abs())).max() <= 2e-4


def test_gemm_f16_against_torch(dev):
    """cpn_gemm_f16 vs an fp32 torch matmul on the same fp16-rounded operands; ragged M, K tail of 32, both tiles."""
    from coponerf_amd._hip import call
    torch.manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    for (M, N, K, ld) in [(1000, 832, 864, 896), (513, 416, 832, 832), (256, 128, 128, 128), (77, 128, 832, 832),
                          (4096, 832, 864, 896)]:
        A = torch.zeros(M, ld, device=dev, dtype=torch.float16)
        A[:, :K] = torch.randn(M, K, device=dev) * 0.5
        Wt = torch.zeros(N, ld, device=dev, dtype=torch.float16)
        Wt[:, :K] = torch.randn(N, K, device=dev) * 0.05
        bias = torch.randn(N, device=dev)
        ref = A[:, :K].float() @ Wt[:, :K].float().t() + bias
        for relu in (0, 1):
            for f32 in (0, 1):
                C = torch.full((M, N), float("nan"), device=dev, dtype=torch.float32 if f32 else torch.float16)
                call("cpn_gemm_f16", A.data_ptr(), ld, Wt.data_ptr(), ld, bias.data_ptr(), C.data_ptr(), N, M, N, K,
                     relu, f32, s)
                want = ref.clamp_min(0) if relu else ref
                err = (C.float() - want).abs().max().item()
                assert err <= (2e-4 if f32 else 4e-3) * max(1.0, want.abs().max().item()), (M, N, K, relu, f32, err)


def test_small_call_forms_are_bit_identical(dev):
    """A ray's value must not depend on the size of the call it is rendered in (the callers render an image as 18 calls of
    3 641 rays): at M <= 16 384 cpn_linear_f32 runs as 4 x as many waves of 2 column tiles each (228 waves of 8 tiles leave
    most SIMDs empty and walk K as a chain of L2 round trips: 35 -> 13-19 us at K = 416), at M <= 8 192 the value projection
    takes cpn_gemm_f16_fewrows; both must reproduce the large-M forms bit for bit on the same rows."""
    from coponerf_amd._hip import call
    torch.manual_seed(5)
    s = torch.cuda.current_stream().cuda_stream
    # cpn_gemm_f16_fewrows (weights pre-packed in MFMA fragment order) against the tiled cpn_gemm_f16 with fp32 output
    for (N, K, ld, M) in [(416, 1664, 1664, 3641), (416, 1664, 1664, 8192), (128, 832, 896, 77), (832, 864, 896, 1000), (48, 32, 32, 5)]:
        A = torch.zeros(M, ld, device=dev, dtype=torch.float16)
        A[:, :K] = torch.randn(M, K, device=dev) * 0.5
        Wt = torch.zeros(N, ld, device=dev, dtype=torch.float16)
        Wt[:, :K] = torch.randn(N, K, device=dev) * 0.05
        bias = torch.randn(N, device=dev)
        Wp = torch.full((N * K,), float("nan"), device=dev, dtype=torch.float16)
        call("cpn_pack_gemm_frags", Wt.data_ptr(), ld, N, K, Wp.data_ptr(), s)
        assert not torch.isnan(Wp).any()
        for relu in (0, 1):
            few = torch.full((M, N), float("nan"), device=dev)
            call("cpn_gemm_f16_fewrows", A.data_ptr(), ld, Wp.data_ptr(), bias.data_ptr(), few.data_ptr(), N, M, N, K, relu, s)
            ref = A[:, :K].float() @ Wt[:, :K].float().t() + bias
            ref = ref.clamp_min(0) if relu else ref
            assert (few - ref).abs().max() <= 2e-4 * max(1.0, float(ref.abs().max())), (N, K, M, relu)
            if N % 208 == 0 or N % 128 == 0:
                tiled = torch.full((M, N), float("nan"), device=dev)
                call("cpn_gemm_f16", A.data_ptr(), ld, Wt.data_ptr(), ld, bias.data_ptr(), tiled.data_ptr(), N, M, N, K, relu, 1, s)
                assert torch.equal(few, tiled), (N, K, M, relu, int((few != tiled).sum()))
    for (N, K) in [(128, 416), (128, 128), (48, 32)]:
        Mbig, Msmall = 16384 + 64, 3641
        X = torch.randn(Mbig, K, device=dev)
        Wt = torch.randn(N, K, device=dev) * 0.1
        b = torch.randn(N, device=dev)
        big, small = torch.empty(Mbig, N, device=dev), torch.empty(Msmall, N, device=dev)
        call("cpn_linear_f32", X.data_ptr(), K, Wt.data_ptr(), K, b.data_ptr(), 0, 0, big.data_ptr(), N, Mbig, N, K, 1, 0, s)
        call("cpn_linear_f32", X.data_ptr(), K, Wt.data_ptr(), K, b.data_ptr(), 0, 0, small.data_ptr(), N, Msmall, N, K, 1, 0, s)
        assert torch.equal(small, big[:Msmall]), (N, K)


def test_linear_f32_against_torch(dev):
    from coponerf_amd._hip import call
    torch.manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    for (M, N, K) in [(100, 128, 416), (64, 3, 128), (1000, 128, 32), (17, 128, 128)]:
        X = torch.randn(M, K, device=dev)
        Wt = torch.randn(N, K, device=dev) * 0.1
        b = torch.randn(N, device=dev)
        res = torch.randn(M, N, device=dev)
        Y = torch.empty(M, N, device=dev)
        call("cpn_linear_f32", X.data_ptr(), K, Wt.data_ptr(), K, b.data_ptr(), res.data_ptr(), N, Y.data_ptr(), N,
             M, N, K, 1, 1, s)
        want = torch.relu(torch.relu(X).double() @ Wt.double().t() + b.double() + res.double()).float()
        assert (Y - want).abs().max() <= 1e-4


def test_full_size_properties(model, dev, weights):
    """BASELINE config-2 sizes (256x256, S=64): size-independent properties instead of an oracle run."""
    H, S, R = 256, 64, 8192
    inp = to_device(syn.make_inputs(1, H, H, R, seed=21), dev)
    z, rel, flow = syn.make_latents(1, H, H, seed=22)
    z, rel, flow = to_device(z, dev), rel.to(dev), to_device(flow, dev)
    model.npoints = S
    with torch.no_grad():
        full = model(inp, z=z, rel_pose=rel, val=True, flow=flow)
        # rays are independent work units: rendering two halves reproduces the whole bit for bit
        halves = []
        for sl in (slice(0, R // 2), slice(R // 2, R)):
            part = {"context": inp["context"], "query": dict(inp["query"], uv=inp["query"]["uv"][:, :, sl].contiguous(),
                                                             rgb=inp["query"]["rgb"][:, :, sl])}
            halves.append(model(part, z=z, rel_pose=rel, val=True, flow=flow))
    assert torch.equal(torch.cat([h["rgb"] for h in halves], dim=2), full["rgb"])
    assert torch.equal(torch.cat([h["pixel_val"] for h in halves], dim=1), full["pixel_val"])
    w = full["at_wt"].view(1, 2, R, S)
    assert (w.sum(dim=(1, 3)) - 1).abs().max() < 1e-5 and float(w.min()) >= 0
    assert torch.isfinite(full["rgb"]).all()
    invalid = full["valid_mask"][..., 0] == 0
    assert (full["rgb"][:, 0][invalid] == 1).all()


@pytest.mark.parametrize("H,S,R,rig", [(256, 64, 192, "wide"), (512, 128, 96, "narrow")])
def test_other_baseline_configs_against_oracle(H, S, R, rig, model, dev, weights):
    """BASELINE configs 4 (ACID-like wide baseline, 256x256x64) and 5 (512x512, 128 samples per ray), render path:
    same bars as the fixture cases — indices bit-identical to the oracle, rgb within 1e-3."""
    from oracle import render_ref as orc
    inp = syn.make_inputs(1, H, H, R, seed=33, rig=rig)
    z, rel, flow = syn.make_latents(1, H, H, seed=34)
    with torch.no_grad():
        ref = orc.forward(inp, z, rel, flow, True, weights, npoints=S, keep=True)
        model.npoints = S
        out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=True, flow=to_device(flow, dev),
                    debug=True)
    assert torch.equal(out["pixel_val"], ref["pixel_val"])
    assert torch.equal(out["_core"]["pt"].cpu(), ref["pt"])
    assert (out["rgb"].cpu() - ref["rgb"]).abs().max() <= RGB_TOL
    assert (out["at_wt"].cpu() - ref["at_wt"]).abs().max() <= 2e-3
    assert torch.equal(out["valid_mask"].cpu(), ref["valid_mask"])


@pytest.mark.parametrize("B,H,S,R,val", [(3, 96, 24, 77, True), (2, 48, 40, 33, False), (1, 64, 7, 129, True)])
def test_ragged_shapes_against_oracle(B, H, S, R, val, model, dev, weights):
    """Sizes that are multiples of nothing convenient: odd ray counts, sample counts that are not powers of two (7, 24,
    40), batch 3, ray chunks that end in the middle of a batch element (chunk_rays = 50)."""
    from oracle import render_ref as orc
    inp = syn.make_inputs(B, H, H, R, seed=91)
    z, rel, flow = syn.make_latents(B, H, H, seed=92)
    old_chunk, old_s = model._engine.chunk_rays, model.npoints
    try:
        with torch.no_grad():
            ref = orc.forward(inp, z, rel, flow, val, weights, npoints=S, keep=True)
            model.npoints, model._engine.chunk_rays = S, 50
            out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=val,
                        flow=to_device(flow, dev), debug=True)
    finally:
        model._engine.chunk_rays, model.npoints = old_chunk, old_s
    assert torch.equal(out["pixel_val"], ref["pixel_val"])
    assert torch.equal(out["_core"]["pt"].cpu(), ref["pt"])
    assert (out["rgb"].cpu() - ref["rgb"]).abs().max() <= RGB_TOL
    assert (out["at_wt"].cpu() - ref["at_wt"]).abs().max() <= 2e-3
    assert torch.equal(out["valid_mask"].cpu(), ref["valid_mask"])


def test_missing_library_is_loud(monkeypatch):
    from coponerf_amd import _hip
    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "LIB_PATH", "/nonexistent/libcoponerf_hip.so")
    with pytest.raises(_hip.HipLibraryError):
        _hip.lib()


# ------------------------------------------------------------------------------------------------------------------
# round 2: the projected-table form of the first encoder layer (csrc/encode.hip) and the parity holes of round 1
# ------------------------------------------------------------------------------------------------------------------
def _encode_first_layer(dev, geo_args, frag, b1d, B, V, R, S, ray0, nrays, hid):
    """hid of the first encoder layer through cpn_encode_key (the library's only form of the layer since round 6) with a ZERO key
    layer behind it; returns kh (= ReLU(0) = 0 everywhere it was written)."""
    from coponerf_amd._hip import call
    ring = torch.zeros(2 * 13 * 8 * 2 * 64 * 8, dtype=torch.float16, device=dev)
    kb = torch.zeros(128, device=dev)
    kh = torch.full((nrays * V * S + 16, 128), -1.0, dtype=torch.float16, device=dev)
    call("cpn_encode_key", *geo_args, frag.data_ptr(), b1d.data_ptr(), ring.data_ptr(), kb.data_ptr(), B, V, R, S, ray0, nrays,
         hid.data_ptr(), kh.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert bool((kh[:nrays * V * S] == 0).all()) and bool((kh[nrays * V * S:] == -1).all())
    return kh


def test_encode_hidden_against_torch(dev):
    """The first encoder layer on the node tables (cpn_encode_key: tables + K = 80 MFMA) vs grid_sample + the layer in float64 on
    the same fp16-rounded maps; border + zeros padding, huge / on-texel / rim coordinates, ray and sample counts that do not
    fill the 4-ray x 4-sample units."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    from tests.encode_bwd_ref import encode_input_ref
    torch.manual_seed(5)
    B, V, R, S, H = 1, 2, 9, 20, 64                       # 9*2*20*2 = 720 rows = 5.6 tiles
    N = B * V
    z = [torch.randn(N, 256, H // 16, H // 16), torch.randn(N, 256, H // 8, H // 8),
         torch.randn(N, 256, H // 4, H // 4), torch.randn(N, 64, H, H)]
    z = [t.half().float() for t in z]
    pv = torch.rand(N, R, S, 2) * 2.4 - 1.2
    sg = torch.rand(N, R, S, 2) * 3 - 1.5
    sg[0, 0, 0] = torch.tensor([1e10, -1e10])
    sg[1, 0, 1] = torch.tensor([-1.0, 1.0])
    pv[0, 1, 2] = torch.tensor([-1.0 + 1.0 / H, 1.0 - 1.0 / H])      # exactly on texel centres of the finest level
    pv[0, 1, 3] = torch.tensor([-1.0, 1.0])                          # image corners: inside the per-level border clamps
    pv[1, 2, 0] = torch.tensor([1.0 - 4.0 / H, -1.0 + 2.0 / H])      # on the clamp nodes of levels 1 / 2
    for k, t in enumerate((-4, -3.5, -2, -1, -0.25, 0, 0.5)):        # the zero rim of the secondary gather, node by node
        sg[0, 3, k] = torch.tensor([2.0 * t / (H // 2) - 1.0, 2.0 * (H // 2 - t) / (H // 2) - 1.0])
    pe = torch.rand(N, R, S, 6) * 2 - 1
    W1 = ((torch.rand(832, 835) * 2 - 1) / 835 ** 0.5)
    b1 = (torch.rand(832) * 2 - 1) * 0.05
    s = torch.cuda.current_stream().cuda_stream
    maps = []
    for t in z:
        n, c, h, w = t.shape
        d = torch.empty(n, h, w, c, dtype=torch.float16, device=dev)
        src = t.to(dev).contiguous()
        call("cpn_nchw_to_nhwc_f16", src.data_ptr(), d.data_ptr(), n, c, h, w, s)
        maps.append(d)
    W1d, b1d = W1.to(dev).contiguous(), b1.to(dev).contiguous()
    frag = torch.empty(_hip.ENC_FRAG_HALVES, dtype=torch.float16, device=dev)
    wtab = torch.empty(_hip.TAB_LD, 768, dtype=torch.float16, device=dev)
    call("cpn_pack_encode_weights", W1d.data_ptr(), 835, frag.data_ptr(), wtab.data_ptr(), s)
    zero_bias = torch.zeros(_hip.TAB_LD, device=dev)
    nodes = N * int(_hip.lib().cpn_encode_table_nodes(H, H))
    assert nodes == N * ((H // 2 + 1) ** 2 + (H // 2 + 9) ** 2)
    feat = torch.empty(nodes, 768, dtype=torch.float16, device=dev)
    call("cpn_node_features", maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), H, H, N, feat.data_ptr(), s)
    tab = torch.empty(nodes, _hip.TAB_LD, dtype=torch.float16, device=dev)
    call("cpn_gemm_f16", feat.data_ptr(), 768, wtab.data_ptr(), 768, zero_bias.data_ptr(), tab.data_ptr(), _hip.TAB_LD,
         nodes, _hip.TAB_LD, 768, 0, 0, s)
    pvd, sgd, ped = pv.to(dev), sg.to(dev), pe.to(dev)
    rows = B * R * V * S * 2
    hid = torch.full((rows, 832), float("nan"), dtype=torch.float16, device=dev)
    _encode_first_layer(dev, (tab.data_ptr(), maps[3].data_ptr(), H, H, pvd.data_ptr(), sgd.data_ptr(), ped.data_ptr()), frag, b1d,
                        B, V, R, S, 0, B * R, hid)
    # ---- fp32 reference: grid_sample on the fp16-rounded maps, then the layer in float64
    x = encode_input_ref(z, pv, sg, pe, B, V, R, S, torch.float32)                                         # (rows, 835), row order
    assert x.shape == (rows, 835)
    want = torch.relu(x.double() @ W1.double().t() + b1.double()).float()
    got = hid.float().cpu()
    assert torch.isfinite(got).all()
    scale = float(want.abs().max())
    assert (got - want).abs().max() <= 4e-3 * max(1.0, scale), float((got - want).abs().max())
    # fp16 node features, fp16 table entries, fp16 K = 80 operands, fp16 output: rms 3e-4 of the largest value (the gather + GEMM
    # form of rounds 1-5 - one rounding per channel instead of one per table tap - measured the same)
    assert float((got - want).pow(2).mean().sqrt()) <= 5e-4 * max(1.0, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("B,R,S,ray0,nrays", [
    (1, 1, 1, 0, 1),            # one row pair
    (1, 5, 3, 0, 5),            # neither a multiple of the 4-ray x 4-sample wave tile
    (2, 7, 9, 3, 9),            # a ray range that starts mid-group and crosses the batch boundary
    (3, 6, 33, 6, 12),          # all of batch element 1 and 2, none of 0
    (2, 17, 64, 30, 4),         # the tail of the last element
    (1, 130, 8, 1, 127),        # more than 8 workgroups' worth of wave tiles, odd ends
])
def test_encode_hidden_ragged_ranges(B, R, S, ray0, nrays, dev):
    """The first layer (cpn_encode_key) on ray sub-ranges / shapes that leave units partly dead: rows inside the range equal
    grid_sample + the layer in float64 on the same fp16-rounded maps, rows outside it are not written at all."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    from tests.encode_bwd_ref import encode_input_ref, chunk_rows
    g = torch.Generator().manual_seed(1000 * B + 10 * R + S)
    V, H = 2, 32
    N = B * V
    z = [torch.randn(N, 256, H // 16, H // 16, generator=g), torch.randn(N, 256, H // 8, H // 8, generator=g),
         torch.randn(N, 256, H // 4, H // 4, generator=g), torch.randn(N, 64, H, H, generator=g)]
    z = [t.half().float() for t in z]
    pv = torch.rand(N, R, S, 2, generator=g) * 2.4 - 1.2
    sg = torch.rand(N, R, S, 2, generator=g) * 3 - 1.5
    pe = torch.rand(N, R, S, 6, generator=g) * 2 - 1
    W1 = (torch.rand(832, 835, generator=g) * 2 - 1) / 835 ** 0.5
    b1 = (torch.rand(832, generator=g) * 2 - 1) * 0.05
    s = torch.cuda.current_stream().cuda_stream
    maps = []
    for t in z:
        n, c, h, w = t.shape
        d = torch.empty(n, h, w, c, dtype=torch.float16, device=dev)
        src = t.to(dev).contiguous()
        call("cpn_nchw_to_nhwc_f16", src.data_ptr(), d.data_ptr(), n, c, h, w, s)
        maps.append(d)
    W1d, b1d = W1.to(dev).contiguous(), b1.to(dev).contiguous()
    frag = torch.empty(_hip.ENC_FRAG_HALVES, dtype=torch.float16, device=dev)
    wtab = torch.empty(_hip.TAB_LD, 768, dtype=torch.float16, device=dev)
    call("cpn_pack_encode_weights", W1d.data_ptr(), 835, frag.data_ptr(), wtab.data_ptr(), s)
    zero_bias = torch.zeros(_hip.TAB_LD, device=dev)
    nodes = N * int(_hip.lib().cpn_encode_table_nodes(H, H))
    feat = torch.empty(nodes, 768, dtype=torch.float16, device=dev)
    call("cpn_node_features", maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), H, H, N, feat.data_ptr(), s)
    tab = torch.empty(nodes, _hip.TAB_LD, dtype=torch.float16, device=dev)
    call("cpn_gemm_f16", feat.data_ptr(), 768, wtab.data_ptr(), 768, zero_bias.data_ptr(), tab.data_ptr(), _hip.TAB_LD,
         nodes, _hip.TAB_LD, 768, 0, 0, s)
    pvd, sgd, ped = pv.to(dev), sg.to(dev), pe.to(dev)
    rows = nrays * V * S * 2                                   # the chunk's rows only (row 0 = ray0)
    guard = 64                                                 # canary rows behind the chunk
    hid = torch.full((rows + guard, 832), float("nan"), dtype=torch.float16, device=dev)
    _encode_first_layer(dev, (tab.data_ptr(), maps[3].data_ptr(), H, H, pvd.data_ptr(), sgd.data_ptr(), ped.data_ptr()), frag, b1d,
                        B, V, R, S, ray0, nrays, hid)
    torch.cuda.synchronize()
    x = chunk_rows(encode_input_ref(z, pv, sg, pe, B, V, R, S, torch.float32), B, V, R, S, ray0, nrays)    # the chunk's rows
    assert x.shape == (rows, 835)
    ref = torch.relu(x.double() @ W1.double().t() + b1.double()).float()
    got = hid[:rows].float().cpu()
    assert torch.isfinite(got).all(), "rows of the chunk left unwritten"
    assert torch.isnan(hid[rows:].float()).all(), "wrote past the chunk"
    scale = max(1.0, float(ref.abs().max()))
    assert float((got - ref).abs().max()) <= 6e-3 * scale, float((got - ref).abs().max())
    assert float((got - ref).pow(2).mean().sqrt()) <= 5e-4 * scale


def _encode_entry_setup(model, dev, cfg):
    inp, z, rel, flow = case_inputs(cfg)
    H, S = cfg["H"], cfg["S"]
    eng = model._engine
    model.npoints = S
    w = eng._weights(model._render_params())
    maps, tabs = eng._feature_maps(to_device(z, dev), w)
    ctx, qry = to_device(inp["context"], dev), to_device(inp["query"], dev)
    g = eng._geometry(ctx["cam2world"], ctx["intrinsics"], qry["cam2world"], qry["intrinsics"], qry["uv"], rel.to(dev), cfg["val"], S, H, H)
    geo = (tabs[0].data_ptr(), maps[3].data_ptr(), H, H, g["pixel_val"].data_ptr(), g["sec_grid"].data_ptr(), g["pe6"].data_ptr())
    return w, geo, (maps, tabs, g)


def test_encode_key_entry_is_bit_identical(model, dev, weights):
    """The C entry itself: cpn_encode_key (csrc/encode_fused.hip: several units per wave, the taps of slice n + 1 issued before
    the key MFMAs of slice n) writes the same kh as cpn_gemm_f16 on the hid it wrote, bit for bit, in row order and in unit
    order — on a ragged chunk (ray0 > 0, a ray count that is no multiple of 4, dead units at the end of most workgroups'
    ranges) and on a whole fixture case; nothing is written past the chunk."""
    from coponerf_amd._hip import call
    cfg, _ = load_case("wide_val")
    B, R, S, V = cfg["B"], cfg["R"], cfg["S"], 2
    w, geo, keep = _encode_entry_setup(model, dev, cfg)
    s = torch.cuda.current_stream().cuda_stream
    for ray0, n in ((7, R - 18), (0, B * R), (R - 3, 5 if B > 1 else 3)):
        rows2 = n * V * S * 2
        hid = torch.full((rows2 + 64, 832), -1.0, dtype=torch.float16, device=dev)        # + a guard band behind the chunk
        kh = torch.full((rows2 // 2 + 64, 128), -1.0, dtype=torch.float16, device=dev)
        call("cpn_encode_key", *geo, w["enc.frag"].data_ptr(), w["query_encode_latent.b"].data_ptr(), w["key_fold.wpk"].data_ptr(),
             w["key_fold.b"].data_ptr(), B, V, R, S, ray0, n, hid.data_ptr(), kh.data_ptr(), 0, s)
        hid_ref = hid[:rows2].clone()
        assert int((hid_ref == -1).sum()) == 0
        kh_ref = torch.empty(rows2 // 2, 128, dtype=torch.float16, device=dev)
        call("cpn_gemm_f16", hid_ref.data_ptr(), 1664, w["key_fold.w16"].data_ptr(), 1664, w["key_fold.b"].data_ptr(), kh_ref.data_ptr(), 128,
             rows2 // 2, 128, 1664, 1, 0, s)
        assert torch.equal(kh[:rows2 // 2], kh_ref), (ray0, n, int((kh[:rows2 // 2] != kh_ref).sum()))
        assert bool((hid[rows2:] == -1).all()) and bool((kh[rows2 // 2:] == -1).all()), "wrote past the chunk"
        # kh_units = 1: the same numbers in UNIT order (what cpn_local_units reads as MFMA B fragments); units * 16 row slots
        from coponerf_amd import _hip
        from coponerf_amd.render import rows_from_unit_order, unit_rows
        units = int(_hip.lib().cpn_encode_units(B, R, S, ray0, n))
        idx = unit_rows(B, R, S, ray0, n)
        assert idx.numel() == units * 16 and sorted(idx[idx >= 0].tolist()) == list(range(rows2 // 2))
        khu = torch.full((units * 16 + 64, 128), -1.0, dtype=torch.float16, device=dev)
        hid.fill_(-1.0)
        call("cpn_encode_key", *geo, w["enc.frag"].data_ptr(), w["query_encode_latent.b"].data_ptr(), w["key_fold.wpk"].data_ptr(),
             w["key_fold.b"].data_ptr(), B, V, R, S, ray0, n, hid.data_ptr(), khu.data_ptr(), 1, s)
        assert torch.equal(hid[:rows2], hid_ref)
        assert torch.equal(rows_from_unit_order(khu, B, R, S, ray0, n), kh_ref)
        assert bool((khu[units * 16:] == -1).all()), "wrote past the unit-order buffer"


def test_psnr_against_ground_truth_within_a_tenth_of_a_db(model, dev, weights):
    """north_star: "PSNR within 0.1 dB of reference".  PSNR of the rendered rays against the query image's own pixels (the
    quantity test.py:218-224 reports, images in [-1, 1]: peak-to-peak 2) for the HIP path, the fp32 CPU oracle and the upstream
    fixture on every fixture case: the three agree to 0.01 dB, and the HIP render against the oracle's is above 70 dB."""
    def psnr(a, b):
        return float(10 * torch.log10(4.0 / ((a - b) ** 2).mean().clamp_min(1e-20)))
    for name in ("c1_val", "train_b2", "wide_val", "hd_val"):
        cfg, gold = load_case(name)
        ref, out = run_pair(model, dev, weights, cfg)
        inp = case_inputs(cfg)[0]
        gt = inp["query"]["rgb"].float()
        ours, want, up = out["rgb"].cpu(), ref["rgb"], torch.from_numpy(gold["rgb"])
        p_ours, p_ref, p_up = psnr(ours, gt), psnr(want, gt), psnr(up, gt)
        print(name, "PSNR vs ground truth: HIP %.4f  oracle %.4f  upstream %.4f dB;  HIP vs oracle %.1f dB" %
              (p_ours, p_ref, p_up, psnr(ours, want)))
        assert abs(p_ours - p_ref) <= 0.01 and abs(p_ours - p_up) <= 0.01, (name, p_ours, p_ref, p_up)
        assert psnr(ours, want) >= 70.0


def test_announced_pair_is_bit_identical(model, dev):
    """CoPoNeRF.prepare_next(): the per-pair preparation (camera copy to the host, NHWC maps, node tables, flow products)
    started on its own stream while the previous pair renders.  Every output of the following forward() equals the
    unannounced call's bit for bit, the prepared pieces were the ones used (consumed, no rebuild), an unannounced pair
    still works in between, and a pair announced but changed in place before its call is rebuilt, not served stale."""
    eng = model._engine
    pairs = []
    for name in ("c1_val", "wide_val", "c1_val"):
        cfg, _ = load_case(name)
        inp, z, rel, flow = case_inputs(cfg)
        pairs.append((cfg, to_device(inp, dev), to_device(z, dev), rel.to(dev), to_device(flow, dev)))
    keys = ("rgb", "at_wt", "valid_mask", "depth_ray", "mask_c2", "matchability_cycle_mask", "gt_rel_pose", "rel_pose_flip")

    def fwd(p):
        model.npoints = p[0]["S"]
        with torch.no_grad():
            o = model(p[1], z=p[2], rel_pose=p[3], val=p[0]["val"], flow=p[4])
        return {k: o[k].clone() for k in keys} | {"pixel_val": o["pixel_val"].clone()}

    plain = [fwd(p) for p in pairs]
    for lanes in (1, 2):
        eng.call_lanes = lanes
        eng.invalidate()
        model.prepare_next(*pairs[0][1:])
        got = []
        for i, p in enumerate(pairs):
            if i + 1 < len(pairs):
                nxt = pairs[i + 1]
                model.prepare_next(nxt[1], nxt[2], nxt[3], nxt[4])
                assert eng._next[0]["stage"] is not None and eng._next[0]["mkey"] is not None
            mine = next(e for e in eng._next if e["z"][0] is p[2][0])
            got.append(fwd(p))
            assert mine["stage"] is None and mine["mkey"] is None, "the prepared pieces were not the ones used"
            if i + 1 < len(pairs):
                assert eng._next[0]["z"][0] is pairs[i + 1][2][0] and eng._next[0]["mkey"] is not None   # parked for the next call
        for a, b in zip(plain, got):
            for k in a:
                assert torch.equal(a[k], b[k]), (lanes, k)
    # announced, then its latent maps change in place before the call: the version check must drop the prepared tables
    p = pairs[1]
    model.prepare_next(*p[1:])
    p[2][0].mul_(0.5)
    changed = fwd(p)
    assert eng._next[0]["mkey"] is not None, "stale tables were adopted"
    eng.invalidate()
    again = fwd(p)
    assert torch.equal(changed["rgb"], again["rgb"]) and not torch.equal(changed["rgb"], plain[1]["rgb"])
    p[2][0].mul_(2.0)
    eng.call_lanes = 2
    eng._ws.clear()


def test_f32_mode_is_the_reference_arithmetic(model, dev, weights):
    """RenderEngine.precision = "f32" (VERDICT r4 missing #4): the reference's arithmetic on this device, in the default's
    formulation - fp32 node tables, exact-fp32 MFMA layers, hid as fp16 (hi, lo) pairs with exact products (csrc/encode_f32.hip).
    (1) It reproduces the fp32 CPU oracle / the upstream fixture to fp32 rounding (1e-5, two orders below the fp16-operand
    default); (2) the default's distance from it is bounded: |rgb_f16 - rgb_f32| <= 4e-4 and |at_wt_f16 - at_wt_f32| <= 2e-3 on
    every fixture case incl. the ragged one - the same-precision statement beside the headline.  (Round 5's layer-by-layer
    form of the mode, exact fp32 operands in the reference's own order, agreed with this one to <= 1e-6 before it left.)"""
    eng = model._engine
    for name in ("c1_val", "train_b2", "wide_val", "hd_val"):
        cfg, gold = load_case(name)
        ref, out16 = run_pair(model, dev, weights, cfg)
        eng.precision, eng.f32_chunk_rays = "f32", 96                   # several chunks, the last one ragged
        try:
            _, out32 = run_pair(model, dev, weights, cfg)
        finally:
            eng.precision, eng.f32_chunk_rays = "f16", 16384
        assert torch.equal(out16["pixel_val"], out32["pixel_val"])
        e_ref = float((out32["rgb"].cpu() - ref["rgb"]).abs().max())
        e_gold = float((out32["rgb"].cpu() - torch.from_numpy(gold["rgb"])).abs().max())
        e_wt = float((out32["at_wt"].cpu() - ref["at_wt"]).abs().max())
        e_zl = float((out32["_core"]["z_local"].cpu() - ref["z_local"].reshape(-1, 416)).abs().max())
        d_rgb = float((out16["rgb"] - out32["rgb"]).abs().max())
        d_wt = float((out16["at_wt"] - out32["at_wt"]).abs().max())
        print(f"{name}: f32 mode vs oracle rgb {e_ref:.1e} (upstream fixture {e_gold:.1e}), at_wt {e_wt:.1e}, z_local {e_zl:.1e};"
              f"  f16 default vs f32 mode rgb {d_rgb:.1e}, at_wt {d_wt:.1e}")
        assert e_ref <= 1e-5 and e_gold <= 2e-5 and e_wt <= 1e-5, (name, e_ref, e_gold, e_wt)
        assert d_rgb <= 4e-4 and d_wt <= 2e-3, (name, d_rgb, d_wt)
    eng._ws.clear()


def test_feature_cache_is_keyed_on_identity(model, dev, weights):
    """a new pair's latents allocated at the freed addresses of the previous pair must not hit the NHWC / table
    cache.  Render pair A, free its latents, render pair B (same shapes, likely the same addresses): B's image must be
    B's, i.e. equal to a render of B through a fresh engine."""
    from coponerf_amd.render import RenderEngine
    cfg, _ = load_case("c1_val")
    inp, zA, rel, flow = case_inputs(cfg)
    _, zB, _, _ = case_inputs(dict(cfg, seed=cfg["seed"] + 100))
    model.npoints = cfg["S"]
    d_inp, d_flow = to_device(inp, dev), to_device(flow, dev)
    with torch.no_grad():
        z = to_device(zA, dev)
        rgbA = model(d_inp, z=z, rel_pose=rel.to(dev), val=True, flow=d_flow)["rgb"].clone()
        del z
        z = to_device(zB, dev)                                    # the allocator hands back the freed blocks
        rgbB = model(d_inp, z=z, rel_pose=rel.to(dev), val=True, flow=d_flow)["rgb"].clone()
        old = model._engine
        model._engine = RenderEngine()
        try:
            rgbB_fresh = model(d_inp, z=z, rel_pose=rel.to(dev), val=True, flow=d_flow)["rgb"].clone()
        finally:
            model._engine = old
    assert torch.equal(rgbB, rgbB_fresh)
    assert (rgbA - rgbB).abs().max() > 1e-3                       # the two pairs really differ


def test_segment_clipper_edge_cases_on_device(dev):
    """The 10 degenerate rays of tests/golden/edges.npz (camera at the origin, origin behind the image plane, ray
    parallel to the image plane, miss, both ends inside, ...; models/epipolar.py:175-253) through cpn_project_rays:
    bit-equal to the oracle on the same rays, equal to the upstream outputs within 1e-6 (NaN-aware)."""
    from coponerf_amd import _hip
    from coponerf_amd._hip import call
    from oracle import render_ref as orc
    import os
    from tests.helpers import GOLDEN
    g = dict(np.load(os.path.join(GOLDEN, "edges.npz")))
    o, d, K = (torch.from_numpy(g[k]) for k in ("o", "d", "K"))
    n = len(o)
    # one camera per ray: T = [0 0 d | o], uv = (0,0), unit intrinsics -> direction normalize((d + o) - o)
    T = torch.zeros(n, 4, 4)
    T[:, :3, 2], T[:, :3, 3], T[:, 3, 3] = d, o, 1.0
    Kq = torch.eye(4)[None].repeat(n, 1, 1)
    uv = torch.zeros(n, 1, 2)
    dir_o, mom_o, org_o = orc.plucker_rays(T, uv, Kq)
    Kn = K[None].expand(n, -1, -1).contiguous()
    xy0, xy1, ok, _, _ = orc.project_rays(org_o, dir_o, Kn)
    cam = torch.zeros(n, 2, _hip.CAM_STRIDE)
    cam[:, :, _hip.CAM_TQ:_hip.CAM_TQ + 16] = T.reshape(n, 1, 16)
    cam[:, :, _hip.CAM_KQ:_hip.CAM_KQ + 4] = torch.tensor([1.0, 1.0, 0.0, 0.0])
    cam[:, :, _hip.CAM_KN:_hip.CAM_KN + 9] = K.reshape(1, 1, 9)
    camd, uvd = cam.reshape(2 * n, -1).to(dev).contiguous(), uv.reshape(n, 1, 2).to(dev).contiguous()
    c9 = torch.empty(2 * n, 1, 9, device=dev)
    seg = torch.empty(2 * n, 1, 4, device=dev)
    ov = torch.empty(2 * n, 1, dtype=torch.uint8, device=dev)
    call("cpn_project_rays", camd.data_ptr(), uvd.data_ptr(), 2, n, 2, 1, c9.data_ptr(), seg.data_ptr(), ov.data_ptr(),
         torch.cuda.current_stream().cuda_stream)
    c9, seg, ov = c9.cpu().view(n, 2, 9), seg.cpu().view(n, 2, 4), ov.cpu().view(n, 2)
    scrub = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    want_seg = torch.cat((scrub((xy0[:, 0] - 0.5) * 2.0), scrub((xy1[:, 0] - 0.5) * 2.0)), -1)
    for v in range(2):
        assert torch.equal(c9[:, v, 0:3], dir_o[:, 0]) and torch.equal(c9[:, v, 3:6], mom_o[:, 0])
        assert torch.equal(seg[:, v], want_seg), (seg[:, v], want_seg)
        assert torch.equal(ov[:, v].bool(), ok[:, 0])
    # ... and against the upstream reference's own outputs
    assert torch.equal(ov[:, 0].bool(), torch.from_numpy(g["overlaps_image"]))
    up = torch.cat((scrub((torch.from_numpy(g["xy_min"]) - 0.5) * 2.0), scrub((torch.from_numpy(g["xy_max"]) - 0.5) * 2.0)), -1)
    assert (seg[:, 0] - up).abs().max() <= 2e-6


@pytest.mark.parametrize("name", ["c1_val", "train_b2", "wide_val"])
def test_aux_outputs_values_on_device(name, model, dev, weights):
    """Row a20: the auxiliary outputs that feed the cycle loss / summaries, by VALUE on the GPU against the oracle and
    the upstream fixture (round 1 only compared depth_ray, the two masks and the shape of at_wt_max)."""
    cfg, gold = load_case(name)
    ref, out = run_pair(model, dev, weights, cfg)
    # at_wt_max: argmax over samples; a different index is only acceptable where the two largest weights tie to 1e-4
    got, want = out["at_wt_max"].cpu()[..., 0], ref["at_wt_max"][..., 0]
    diff = got != want
    if diff.any():
        w = ref["at_wt"]
        gap = (w.gather(-1, want[..., None]) - w.gather(-1, got[..., None]))[..., 0][diff]
        assert float(gap.abs().max()) <= 1e-4
    assert diff.float().mean() <= 1e-2
    for k in ("T_to_C1_pts", "T_to_C2_pts"):            # pixels (unbounded: points far outside the frame reach 1e4 px)
        want_k = ref[k]
        e = (out[k].cpu() - want_k).abs() / (1.0 + want_k.abs())
        # the depth enters through fp16-weighted sums, and single rays whose expected point projects with w ~ 0 amplify whatever
        # rounding noise they get: 1.2e-3 / 3.8e-3 on the worst ray of wide_val with two roundings of the first layer that leave
        # rgb, at_wt and z_local where they were (tools/_build A/B, round 6)
        assert float(e.max()) <= 6e-3, (k, float(e.max()))
        if k in gold:
            gk = torch.from_numpy(gold[k])
            assert float(((out[k].cpu() - gk).abs() / (1.0 + gk.abs())).max()) <= 6e-3
    # C2_pts_to_C1 = integer pixel + flow looked up there: equal unless the reprojected pixel moved across a pixel edge
    c = (out["C2_pts_to_C1"].cpu() - ref["C2_pts_to_C1"]).abs().amax(-1)
    assert (c > 1e-3).float().mean() <= 2e-2
    assert (out["depth_ray"].cpu() - ref["depth_ray"]).abs().max() <= 2e-2


def test_full_image_four_chunks_against_oracle(model, dev, weights):
    """BASELINE configs[1] at its real size: 256x256, all 65 536 rays (4 chunks of 16 384), 64 samples.  The oracle
    takes seconds per thousand rays, so a strided subset of 2 048 rays (every 32nd: touches all four chunks) is
    rendered by the oracle on its own and compared with the same rays of the full-image HIP render."""
    from oracle import render_ref as orc
    H, S = 256, 64
    inp = syn.make_inputs(1, H, H, 0, seed=41, full_image=True)
    z, rel, flow = syn.make_latents(1, H, H, seed=42)
    R = inp["query"]["uv"].shape[2]
    assert R == 65536
    sel = torch.arange(0, R, 32)
    sub = {"context": inp["context"], "query": {k: (v[:, :, sel].contiguous() if k in ("uv", "rgb") else v)
                                                for k, v in inp["query"].items()}}
    model.npoints = S
    old = model._engine.chunk_rays
    model._engine.chunk_rays = 16384
    try:
        with torch.no_grad():
            dinp, dz, dflow = to_device(inp, dev), to_device(z, dev), to_device(flow, dev)
            out = model(dinp, z=dz, rel_pose=rel.to(dev), val=True, flow=dflow)
            ref = orc.forward(sub, z, rel, flow, True, weights, npoints=S)
            # the engine's automatic chunk size renders the image as ONE chunk on a 288 GB device: a ray's arithmetic does
            # not depend on the chunk it is in
            model._engine.chunk_rays = 0
            assert model._engine._auto_chunk(S, dev) == 65536
            one = model(dinp, z=dz, rel_pose=rel.to(dev), val=True, flow=dflow)
            for k in ("rgb", "at_wt", "pixel_val", "valid_mask", "depth_ray"):
                assert torch.equal(one[k], out[k]), k
            del one
    finally:
        model._engine.chunk_rays = old
        model._engine._ws.clear()                                  # 30 GB of one-chunk workspace: not needed by later tests
    assert torch.equal(out["pixel_val"][:, sel], ref["pixel_val"])
    assert (out["rgb"][:, :, sel].cpu() - ref["rgb"]).abs().max() <= RGB_TOL
    assert (out["at_wt"][:, sel].cpu() - ref["at_wt"]).abs().max() <= 2e-3
    assert torch.equal(out["valid_mask"][:, sel].cpu(), ref["valid_mask"])


def test_config5_batch2_full_image_against_oracle(model, dev, weights):
    """BASELINE configs[4] at its real per-pair size and B = 2: 512x512, all 262 144 rays of BOTH pairs in one call (32
    chunks of 16 384), 128 samples — the node tables of the two pairs are 2 x 254 MB.  The oracle renders a strided
    subset (every 509th ray, prime stride: all image rows and columns, all chunks) of each pair."""
    from oracle import render_ref as orc
    H, S, B = 512, 128, 2
    inp = syn.make_inputs(B, H, H, 0, seed=51, full_image=True)
    z, rel, flow = syn.make_latents(B, H, H, seed=52)
    R = inp["query"]["uv"].shape[2]
    assert R == 262144
    sel = torch.arange(0, R, 509)
    sub = {"context": inp["context"], "query": {k: (v[:, :, sel].contiguous() if k in ("uv", "rgb") else v)
                                                for k, v in inp["query"].items()}}
    old_n, old_c = model.npoints, model._engine.chunk_rays
    model.npoints, model._engine.chunk_rays = S, 16384
    try:
        with torch.no_grad():
            out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=True, flow=to_device(flow, dev))
            ref = orc.forward(sub, z, rel, flow, True, weights, npoints=S)
        got = {k: out[k] for k in ("pixel_val", "rgb", "at_wt", "valid_mask")}
        del out
    finally:
        model.npoints, model._engine.chunk_rays = old_n, old_c
        model._engine._ws.clear()                                  # 14 GB of chunk workspace: not needed by later tests
    assert torch.equal(got["pixel_val"][:, sel], ref["pixel_val"])
    err = (got["rgb"][:, :, sel].cpu() - ref["rgb"]).abs()
    print(f"configs[4] B=2: rgb max-abs vs oracle {float(err.max()):.2e} over {B * len(sel)} rays")
    assert err.max() <= RGB_TOL
    assert (got["at_wt"][:, sel].cpu() - ref["at_wt"]).abs().max() <= 2e-3
    assert torch.equal(got["valid_mask"][:, sel].cpu(), ref["valid_mask"])


def _strided_query(inp, sel):
    return {"context": inp["context"], "query": {k: (v[:, :, sel].contiguous() if k in ("uv", "rgb") else v)
                                                 for k, v in inp["query"].items()}}


def test_config4_full_image_wide_rig_against_oracle(model, dev, weights):
    """BASELINE configs[3] at its real size: the ACID-like WIDE-baseline rig, 256x256, all 65 536 rays in one
    call (one chunk), 64 samples - the case whose reprojected secondary samples leave the other image over large parts of
    the frame (zero-padded table rim, clipped segments).  Oracle on every 251st ray (prime stride: all rows, all columns)."""
    from oracle import render_ref as orc
    H, S = 256, 64
    inp = syn.make_inputs(1, H, H, 0, seed=33, rig="wide", full_image=True)
    z, rel, flow = syn.make_latents(1, H, H, seed=34)
    R = inp["query"]["uv"].shape[2]
    sel = torch.arange(0, R, 251)
    old_n = model.npoints
    model.npoints = S
    try:
        with torch.no_grad():
            out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=True, flow=to_device(flow, dev))
            ref = orc.forward(_strided_query(inp, sel), z, rel, flow, True, weights, npoints=S)
        got = {k: out[k] for k in ("pixel_val", "rgb", "at_wt", "valid_mask")}
        del out
    finally:
        model.npoints = old_n
    assert torch.equal(got["pixel_val"][:, sel], ref["pixel_val"])
    err = (got["rgb"][:, :, sel].cpu() - ref["rgb"]).abs()
    invalid = int((ref["valid_mask"] == 0).sum())
    print(f"configs[3] full image, wide rig: rgb max-abs vs oracle {float(err.max()):.2e} over {len(sel)} rays ({invalid} without overlap)")
    assert err.max() <= RGB_TOL
    assert (got["at_wt"][:, sel].cpu() - ref["at_wt"]).abs().max() <= 2e-3
    assert torch.equal(got["valid_mask"][:, sel].cpu(), ref["valid_mask"])
    assert torch.isfinite(got["rgb"]).all()


def test_config5_batch8_against_oracle_pair_by_pair(model, dev, weights):
    """BASELINE configs[4] at its real batch: 8 pairs of 512x512, 128 samples, all 8 x 262 144 rays in ONE
    call (128 chunks of 16 384 rays; 16 node tables = 2 GB).  The oracle renders every 4 093rd ray (prime) of every pair,
    pair by pair (its own memory stays that of one pair)."""
    from oracle import render_ref as orc
    H, S, B = 512, 128, 8
    inp = syn.make_inputs(B, H, H, 0, seed=57, full_image=True)
    z, rel, flow = syn.make_latents(B, H, H, seed=58)
    R = inp["query"]["uv"].shape[2]
    sel = torch.arange(0, R, 4093)
    old_n, old_c = model.npoints, model._engine.chunk_rays
    model.npoints, model._engine.chunk_rays = S, 16384
    try:
        with torch.no_grad():
            out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=True, flow=to_device(flow, dev))
            got = {"pixel_val": out["pixel_val"][:, sel].cpu(), "rgb": out["rgb"][:, :, sel].cpu(),
                   "at_wt": out["at_wt"][:, sel].cpu(), "valid_mask": out["valid_mask"][:, sel].cpu()}
            finite = bool(torch.isfinite(out["rgb"]).all())
            del out
    finally:
        model.npoints, model._engine.chunk_rays = old_n, old_c
        model._engine._ws.clear()
        model._engine.invalidate()                                    # 2 GB of tables, 1 GB of NHWC maps
        torch.cuda.empty_cache()
    assert finite
    worst = 0.0
    for b in range(B):
        one = lambda o: ({k: one(v) for k, v in o.items()} if isinstance(o, dict) else
                         (type(o)(one(v) for v in o) if isinstance(o, (list, tuple)) else o[b:b + 1]))
        sub = _strided_query(one(inp), sel)
        zb = [t[2 * b:2 * b + 2] for t in z]
        fb = tuple(t[b:b + 1] for t in flow) if isinstance(flow, (list, tuple)) else flow[b:b + 1]
        with torch.no_grad():
            ref = orc.forward(sub, zb, rel[b:b + 1], fb, True, weights, npoints=S)
        assert torch.equal(got["pixel_val"][2 * b:2 * b + 2], ref["pixel_val"]), b
        err = float((got["rgb"][b:b + 1] - ref["rgb"]).abs().max())
        worst = max(worst, err)
        assert err <= RGB_TOL, (b, err)
        assert (got["at_wt"][2 * b:2 * b + 2] - ref["at_wt"]).abs().max() <= 2e-3, b
        assert torch.equal(got["valid_mask"][b:b + 1], ref["valid_mask"]), b
    print(f"configs[4] B=8: rgb max-abs vs oracle {worst:.2e} over {B * len(sel)} rays")


def test_per_ray_intermediates_against_upstream(dev, weights):
    """What the folded formulation still forms of the reference's tensors - per RAY: encode_latent(z_local round 1)
    (CoPoNeRF.py:468) - compared ON THE GPU with the upstream model's own intermediates (tests/golden/inter.npz).  (The per-sample
    tensors of the reference's ordering - query_encode_latent_2, latent_value, key_map_2, query_embed_2, query_repeat_embed_2 -
    are never formed: the layer-by-layer mode that did, rounds 1-5, matched them to 3e-4 .. 6e-4 of each tensor's scale and left
    the library in round 6; the CPU oracle is pinned on them, tests/test_oracle_golden.py.)"""
    from coponerf_amd import CoPoNeRF
    cfg, gold = load_case("inter")
    inp, z, rel, flow = case_inputs(cfg)
    R, S = cfg["R"], cfg["S"]
    m = CoPoNeRF.CoPoNeRF(n_view=2, npoints=S)
    m.load_state_dict(weights, strict=False)
    m = m.to(dev).eval()
    eng = m._engine
    eng.call_lanes = 1                                              # workspace of the caller's stream, un-prefixed names
    with torch.no_grad():
        out = m(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=cfg["val"], flow=to_device(flow, dev))
    torch.cuda.synchronize()
    ze = eng._ws["ze.0"][:R * 128].view(R, 128).cpu()
    gze = torch.from_numpy(gold["ze"])
    err = float((ze[None] - gze).abs().max() / gze.abs().max())
    print(f"encode_latent output, max-abs error / tensor max: {err:.1e}")
    assert err <= 1e-3
    assert (out["rgb"].cpu() - torch.from_numpy(gold["rgb"])).abs().max() <= RGB_TOL


def test_peaked_attention_case(dev, weights):
    """HIP path on the peaked-attention case (peaked_val.npz: largest softmax weight of a ray > 0.5 on most rays, latents at
    get_z's output statistics) against the upstream reference's outputs and the oracle: north_star's 1e-3 on rgb where no
    averaging over 2 S near-equal weights hides the fp16 operands."""
    from coponerf_amd import CoPoNeRF
    from oracle import render_ref as orc
    from tests.helpers import case_weights
    cfg, gold = load_case("peaked_val")
    w = case_weights(cfg, weights)
    inp, z, rel, flow = case_inputs(cfg)
    m = CoPoNeRF.CoPoNeRF(n_view=2, npoints=cfg["S"])
    m.load_state_dict(w, strict=False)
    m = m.to(dev).eval()
    with torch.no_grad():
        ref = orc.forward(inp, z, rel, flow, cfg["val"], w, npoints=cfg["S"], keep=True)
        out = m(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=cfg["val"], flow=to_device(flow, dev), debug=True)
    B, R, S = cfg["B"], cfg["R"], cfg["S"]
    at = out["at_wt"].cpu()
    peak = at.view(B, 2, R, S).permute(0, 2, 1, 3).reshape(B * R, 2 * S).max(dim=1).values
    assert float((peak > 0.5).float().mean()) >= 0.8
    assert torch.equal(out["pixel_val"], ref["pixel_val"])
    e_ref = float((out["rgb"].cpu() - ref["rgb"]).abs().max())
    e_up = float((out["rgb"].cpu() - torch.from_numpy(gold["rgb"])).abs().max())
    e_wt = float((at - torch.from_numpy(gold["at_wt"])).abs().max())
    e_zl = float((out["_core"]["z_local"].cpu() - ref["z_local"].reshape(-1, 416)).abs().max())
    print(f"peaked attention: rgb vs oracle {e_ref:.2e}, vs upstream {e_up:.2e}; at_wt vs upstream {e_wt:.2e}; z_local {e_zl:.2e} "
          f"(|z_local| max {float(ref['z_local'].abs().max()):.2f}); median peak weight {float(peak.median()):.2f}")
    # MEASURED, and outside north_star's 1e-3: 3.0e-3 on rgb, 1.5e-2 on a weight.  The logits (|l| up to ~50 here) are formed from
    # fp16 operands end to end and carry ~3e-4 relative error; a flat softmax averaged that away on every other fixture.  The
    # envelope inside which 1e-3 holds is charted in tests/test_gpu_range.py::test_rgb_error_over_attention_sharpness (median
    # peak weight <= 0.2); this case sits beyond it and is held to what the fp16 path delivers there ...
    assert e_ref <= 5e-3 and e_up <= 5e-3
    assert e_wt <= 2.5e-2
    assert (out["at_wt_max"].cpu() != torch.from_numpy(gold["at_wt_max"])).float().mean() <= 1e-2
    # ... and the reference-arithmetic mode to the 1e-3 bar with two orders to spare:
    # the same case with exact fp32 operands (precision = "f32"): the reference's arithmetic
    m._engine.precision = "f32"
    with torch.no_grad():
        out32 = m(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=cfg["val"], flow=to_device(flow, dev))
    assert float((out32["rgb"].cpu() - ref["rgb"]).abs().max()) <= 5e-5
    assert float((out32["at_wt"].cpu() - ref["at_wt"]).abs().max()) <= 2e-4
