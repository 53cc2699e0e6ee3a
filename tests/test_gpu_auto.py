"""precision = "auto" (RenderEngine): the fp16 default with a per-ray logit guard; the rays it flags are rendered again in the
reference's arithmetic and merged in before the decoder — runs on a real MI355X (`pytest -m gpu`).

Kernels (csrc/guard.hip, the _rays entries of csrc/encode_f32.hip) against torch and against their range forms; the two limits
of the threshold; the per-ray mix; peaked_val at north_star's bar; a held-out sharpness sweep (seeds used neither by
tools/auto_calibrate.py nor by peaked_val); the callers' 18-call loop; and the f16 / f32 modes' launches left alone."""
import math

import pytest
import torch

from coponerf_amd import _hip
from coponerf_amd import synthetic as syn
from tests.helpers import case_inputs, case_weights, load_case, to_device

pytestmark = pytest.mark.gpu

NEW_ENTRIES = ("cpn_logit_guard", "cpn_select_rays", "cpn_encode_hidden_f32_rays", "cpn_attend_hidden_f32_rays")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _s():
    return _hip.stream_handle()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- 1. guard and selection against torch -------------------------------------------------------------------------------
def _guard_ref(lg, nray, T):
    """(score, scale): the score in float64 and the size of its terms, sum_i w_i |l_i| (1 - w_i cancels in fp32 on a sharp ray:
    the kernel's error is relative to that scale)"""
    l = (lg.float() / 11.31).double().view(nray, T)
    w = torch.softmax(l, dim=1)
    return (w * (1 - w) * l.abs()).sum(dim=1), (w * l.abs()).sum(dim=1)


def _select(score, tau, dev):
    n = score.numel()
    lst = torch.full((n,), -5, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), -5, dtype=torch.int32, device=dev)
    _hip.call("cpn_select_rays", score.data_ptr(), n, float(tau), lst.data_ptr(), cnt.data_ptr(), _s())
    torch.cuda.synchronize()
    k = int(cnt.item())
    want = torch.nonzero(score > tau).reshape(-1).to(torch.int32)
    assert k == want.numel(), (tau, k, want.numel())
    assert torch.equal(lst[:k], want), tau
    assert bool((lst[k:] == -5).all())                     # nothing past the count is written


def test_guard_and_select_against_torch(dev):
    g = torch.Generator().manual_seed(5)
    B, V, R, S = 2, 2, 37, 16
    T, nray = V * S, B * R
    # per-ray logit scales from flat to very sharp
    scale = torch.logspace(-2, 2.2, nray)[torch.randperm(nray, generator=g)]
    lg1 = (torch.randn(nray, T, generator=g) * scale[:, None]).reshape(-1).to(dev)
    lg2 = (torch.randn(nray, T, generator=g) * scale.flip(0)[:, None]).reshape(-1).to(dev)
    score = torch.full((nray,), float("nan"), device=dev)
    for ray0, n in ((0, 33), (33, nray - 33)):               # two chunks, the second at an odd ray0
        for lg, acc in ((lg1, 0), (lg2, 1)):
            _hip.call("cpn_logit_guard", lg[ray0 * T:].data_ptr(), B, V, R, S, ray0, n, score.data_ptr(), acc, _s())
    torch.cuda.synchronize()
    (s1, m1), (s2, m2) = _guard_ref(lg1.cpu(), nray, T), _guard_ref(lg2.cpu(), nray, T)
    want, scale = torch.maximum(s1, s2), torch.maximum(m1, m2)
    got = score.cpu().double()
    assert bool(torch.isfinite(got).all())
    assert float(((got - want).abs() / scale.clamp_min(1e-30)).max()) <= 1e-5
    for tau in (-1.0, math.inf) + tuple(float(score.quantile(q)) for q in (0.1, 0.5, 0.9)):
        _select(score, tau, dev)
    big = torch.rand(200000, generator=g).to(dev)            # 49 tiles of the scan
    for tau in (-1.0, math.inf) + tuple(float(big.quantile(q)) for q in (0.01, 0.5, 0.999)):
        _select(big, tau, dev)


# ---- 2. the _rays entries equal the range entries ----------------------------------------------------------------------------
def test_list_entries_equal_range_entries(dev):
    g = torch.Generator().manual_seed(9)
    B, V, R, S, H, W = 2, 2, 37, 16, 32, 32
    T, nray, N = V * S, B * R, B * V
    f32 = torch.float32
    nodes = N * int(_hip.lib().cpn_encode_table_nodes(H, W))
    tab = torch.randn(nodes, _hip.TAB_LD, generator=g).to(dev)
    map3 = torch.randn(N, H, W, 64, generator=g).to(dev)
    pixel_val = (torch.rand(N, R, S, 2, generator=g) * 2.2 - 1.1).to(dev)
    sec_grid = (torch.rand(N, R, S, 2, generator=g) * 2.2 - 1.1).to(dev)
    pe6 = torch.randn(N, R, S, 6, generator=g).to(dev)
    w80t = (torch.randn(68, 832, generator=g) * 0.1).to(dev)
    s = _s()

    def enc(rays, ray0, n):
        hs = torch.empty(n * T, 3328, dtype=torch.float16, device=dev)
        args = (tab.data_ptr(), map3.data_ptr(), H, W, pixel_val.data_ptr(), sec_grid.data_ptr(), pe6.data_ptr(), w80t.data_ptr(),
                B, V, R, S)
        if rays is None:
            _hip.call("cpn_encode_hidden_f32", *args, ray0, n, hs.data_ptr(), s)
        else:
            _hip.call("cpn_encode_hidden_f32_rays", *args, rays.data_ptr(), ray0, n, hs.data_ptr(), s)
        return hs

    qa = torch.randn(nray * T, 128, generator=g).to(dev)
    qb = torch.randn(nray * T, 128, generator=g).to(dev) * 0.3

    def att(rays, ray0, n, hs, a, b):
        hbar = torch.empty(n, 1664, dtype=f32, device=dev)
        at = torch.full((N, R, S), -7.0, device=dev)
        if rays is None:
            _hip.call("cpn_attend_hidden_f32", a.data_ptr(), b.data_ptr(), hs.data_ptr(), B, V, R, S, ray0, n, hbar.data_ptr(),
                      at.data_ptr(), s)
        else:
            _hip.call("cpn_attend_hidden_f32_rays", a.data_ptr(), b.data_ptr(), hs.data_ptr(), B, V, R, S, rays.data_ptr(), ray0, n,
                      hbar.data_ptr(), at.data_ptr(), s)
        return hbar, at

    full = enc(None, 0, nray)
    hb_full, at_full = att(None, 0, nray, full, qa, qb)
    ar = torch.arange(nray, dtype=torch.int32, device=dev)
    assert _same(enc(ar, 0, nray), full)
    hb, at = att(ar, 0, nray, full, qa, qb)
    assert _same(hb, hb_full) and _same(at, at_full)
    # an inner range of the arange list == the same range of the range entries
    part = enc(None, 5, 20)
    assert _same(enc(ar, 5, 20), part)
    assert _same(att(ar, 5, 20, part, qa[5 * T:], qb[5 * T:])[0], att(None, 5, 20, part, qa[5 * T:], qb[5 * T:])[0])
    # a random ascending subset: every listed ray's rows are that ray's rows of the full run
    sub = torch.sort(torch.randperm(nray, generator=g)[:23]).values
    rows = (sub[:, None] * T + torch.arange(T)[None]).reshape(-1).to(dev)
    subd = sub.to(torch.int32).to(dev)
    pad = torch.cat((torch.zeros(3, dtype=torch.int32, device=dev), subd))      # list offset 3
    hs_sub = enc(pad, 3, sub.numel())
    torch.cuda.synchronize()
    assert _same(hs_sub, full[rows])
    hb, at = att(pad, 3, sub.numel(), hs_sub, qa[rows].contiguous(), qb[rows].contiguous())
    torch.cuda.synchronize()
    assert _same(hb, hb_full[sub.to(dev)])
    b_, r_ = sub // R, sub % R
    listed = torch.zeros(N, R, dtype=torch.bool)
    listed[b_ * V, r_] = True
    listed[b_ * V + 1, r_] = True
    at_c, full_c = at.cpu(), at_full.cpu()
    assert _same(at_c[listed], full_c[listed])
    assert bool((at_c[~listed] == -7.0).all())


# ---- model-level helpers ----------------------------------------------------------------------------------------------------
def _model(dev, weights, S, **engine):
    from coponerf_amd import CoPoNeRF
    m = CoPoNeRF.CoPoNeRF(n_view=2, npoints=S)
    m.load_state_dict(weights, strict=False)
    m = m.to(dev).eval()
    for k, v in engine.items():
        setattr(m._engine, k, v)
    return m


def _sweep_case(seed_inp, seed_lat, B=1, H=64, R=256):
    inp = syn.make_inputs(B, H, H, R, seed=seed_inp)
    z, rel, flow = syn.make_latents(B, H, H, seed=seed_lat)
    return inp, syn.latents_at_getz_statistics(z), rel, flow


def _run(m, dev, case, precision, **kw):
    inp, z, rel, flow = case
    m._engine.precision = precision
    for k, v in kw.items():
        setattr(m._engine, k, v)
    with torch.no_grad():
        return m(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=True, flow=to_device(flow, dev), debug=True)


# ---- 3. the limits of the threshold -------------------------------------------------------------------------------------------
def test_threshold_limits(dev):
    case = _sweep_case(61, 62)
    m = _model(dev, syn.peaked_weights(syn.make_render_weights(seed=19), 48.0), 32)
    o16 = _run(m, dev, case, "f16")
    oa = _run(m, dev, case, "auto", auto_threshold=math.inf)
    assert m._engine.last_exact_rays == (0, 256)
    assert m._engine._t32 is None                              # the fp32 tables were never built
    for k in ("rgb", "at_wt", "at_wt_max"):
        assert _same(oa[k], o16[k]), k
    assert _same(oa["_core"]["z_local"], o16["_core"]["z_local"])
    assert torch.equal(oa["pixel_val"], o16["pixel_val"])
    assert "guard_score" in oa["_core"] and oa["_core"]["guard_score"].shape == (1, 256)
    assert "guard_score" not in o16["_core"]
    assert set(oa["_core"]) - {"guard_score"} == set(o16["_core"])
    o32 = _run(m, dev, case, "f32")
    assert "guard_score" not in o32["_core"]
    oa = _run(m, dev, case, "auto", auto_threshold=-1.0)
    assert m._engine.last_exact_rays == (256, 256)
    for k in ("rgb", "at_wt"):
        assert _same(oa[k], o32[k]), k
    assert _same(oa["_core"]["z_local"], o32["_core"]["z_local"])
    assert m._engine._t32 is not None
    _run(m, dev, _sweep_case(63, 64), "auto", auto_threshold=math.inf)      # a new pair that flags nothing
    assert m._engine._t32 is None                              # the old pair's fp32 tables are not kept
    with pytest.raises(ValueError, match="auto"):
        _run(m, dev, case, "fp8")


# ---- 4. auto is a per-ray mix -------------------------------------------------------------------------------------------------
def test_auto_is_a_per_ray_mix(dev):
    B, H, S = 2, 64, 32
    inp = syn.make_inputs(B, H, H, 0, seed=71, full_image=True)       # 8192 rays: at gain 48 a few stay below the threshold
    z, rel, flow = syn.make_latents(B, H, H, seed=72)
    case = (inp, syn.latents_at_getz_statistics(z), rel, flow)
    m = _model(dev, syn.peaked_weights(syn.make_render_weights(seed=19), 48.0), S)
    from coponerf_amd.render import RenderEngine
    eng = RenderEngine(chunk_rays=1300, lanes=2)              # ragged fp16 chunks over two lanes
    eng.f32_chunk_rays = 1000                                 # ragged fp32 chunks
    m._engine = eng
    o16 = _run(m, dev, case, "f16")
    o32 = _run(m, dev, case, "f32")
    oa = _run(m, dev, case, "auto")
    assert eng.auto_threshold == RenderEngine.AUTO_THRESHOLD
    k, n = eng.last_exact_rays
    R = H * H
    assert n == B * R and 0 < k < n, (k, n)
    flag = (oa["_core"]["guard_score"].reshape(-1) > eng.auto_threshold).cpu()
    assert int(flag.sum()) == k

    def per_ray(o, key):
        t = o[key] if key != "z_local" else o["_core"]["z_local"]
        if key == "rgb":
            return t.reshape(B * R, 3).cpu()
        if key == "at_wt":
            return t.view(B, 2, R, S).permute(0, 2, 1, 3).reshape(B * R, 2 * S).cpu()
        return t.reshape(B * R, 416).cpu()

    for key in ("rgb", "at_wt", "z_local"):
        a, x16, x32 = per_ray(oa, key), per_ray(o16, key), per_ray(o32, key)
        assert _same(a[flag], x32[flag]), key
        assert _same(a[~flag], x16[~flag]), key


# ---- 5. peaked_val at the contract ---------------------------------------------------------------------------------------------
def test_peaked_val_auto_meets_north_star(dev):
    from oracle import render_ref as orc
    cfg, gold = load_case("peaked_val")
    w = case_weights(cfg, syn.make_render_weights())
    inp, z, rel, flow = case_inputs(cfg)
    m = _model(dev, w, cfg["S"])
    with torch.no_grad():
        ref = orc.forward(inp, z, rel, flow, cfg["val"], w, npoints=cfg["S"], keep=True)
    oa = _run(m, dev, (inp, z, rel, flow), "auto")
    k, n = m._engine.last_exact_rays
    o32 = _run(m, dev, (inp, z, rel, flow), "f32")
    e_ref = float((oa["rgb"].cpu() - ref["rgb"]).abs().max())
    e_up = float((oa["rgb"].cpu() - torch.from_numpy(gold["rgb"])).abs().max())
    e_wt = float((oa["at_wt"].cpu() - torch.from_numpy(gold["at_wt"])).abs().max())
    gmax = torch.from_numpy(gold["at_wt_max"])
    mis_a = float((oa["at_wt_max"].cpu() != gmax).float().mean())
    mis_32 = float((o32["at_wt_max"].cpu() != gmax).float().mean())
    print(f"peaked_val, auto: {k}/{n} rays exact; rgb vs oracle {e_ref:.2e}, vs upstream {e_up:.2e}; at_wt vs upstream {e_wt:.2e}; "
          f"at_wt_max mismatches {mis_a:.4f} (f32 mode {mis_32:.4f})")
    assert e_ref <= 1e-3 and e_up <= 1e-3
    assert e_wt <= 2e-3
    assert mis_a <= mis_32


# ---- 6. held-out sharpness sweep -----------------------------------------------------------------------------------------------
def test_held_out_sharpness_sweep(dev):
    from oracle import render_ref as orc
    case = _sweep_case(51, 52)
    inp, z, rel, flow = case
    rows, bad = [], []
    for g in (1.0, 16.0, 24.0, 32.0, 48.0, 64.0):
        w = syn.peaked_weights(syn.make_render_weights(seed=17), g)
        m = _model(dev, w, 32)
        with torch.no_grad():
            ref = orc.forward(inp, z, rel, flow, True, w, npoints=32, keep=True)
        oa = _run(m, dev, case, "auto")
        k, n = m._engine.last_exact_rays
        err = float((oa["rgb"].cpu() - ref["rgb"]).abs().max())
        e_wt = float((oa["at_wt"].cpu() - ref["at_wt"]).abs().max())
        rows.append((g, k / n, err, e_wt))
        if err > 1e-3 or e_wt > 2e-3 or (g == 1.0 and k != 0):
            bad.append(rows[-1])
    print("gain  flagged   rgb max-abs   at_wt err")
    for r in rows:
        print("%4.0f  %7.3f  %12.3e  %10.3e" % r)
    assert not bad, bad


# ---- 7. the callers' loop ------------------------------------------------------------------------------------------------------
def _callers_loop_equals_one_call(dev, precision):
    from coponerf_amd.evalloop import render_in_chunks
    B, H = 2, 64
    m = _model(dev, syn.peaked_weights(syn.make_render_weights(seed=19), 48.0), 32)
    m._engine.precision = precision
    m._engine.call_lanes = 2
    inp = to_device(syn.make_inputs(B, H, H, 0, seed=71, full_image=True), dev)
    z, rel, flow = syn.make_latents(B, H, H, seed=72)
    z = to_device(syn.latents_at_getz_statistics(z), dev)
    rel, flow = rel.to(dev), to_device(flow, dev)
    with torch.no_grad():
        full = m(inp, z=z, rel_pose=rel, val=True, flow=flow)
    if precision == "auto":
        k, n = m._engine.last_exact_rays
        assert 0 < k < n
    joined = render_in_chunks(m, inp, 18, latents=(z, rel, flow))
    assert torch.equal(joined["pixel_val"], full["pixel_val"])
    assert torch.equal(joined["at_wt_max"], full["at_wt_max"])
    for key in ("rgb", "at_wt", "depth_ray", "valid_mask"):
        assert joined[key].shape == full[key].shape, key
        assert _same(joined[key], full[key]), key


def test_callers_loop_equals_one_call(dev):
    _callers_loop_equals_one_call(dev, "auto")


def test_callers_loop_equals_one_call_in_f32_mode(dev):
    """the f32 mode's tables are built by the loop's first call on one call lane and read by the next call on the other"""
    _callers_loop_equals_one_call(dev, "f32")


# ---- 8. the default and the f32 mode run none of the new entries ---------------------------------------------------------------
def test_f16_and_f32_modes_do_not_launch_the_guard(dev, monkeypatch):
    import coponerf_amd.render as render_mod
    import coponerf_amd.render_f32 as render_f32_mod
    seen = []
    inner = render_mod.call

    def counting(name, *args):
        seen.append(name)
        return inner(name, *args)

    for mod in (render_mod, render_f32_mod):
        monkeypatch.setattr(mod, "call", counting)
    case = _sweep_case(61, 62)
    m = _model(dev, syn.peaked_weights(syn.make_render_weights(seed=19), 48.0), 32)
    for precision in ("f16", "f32"):
        seen.clear()
        _run(m, dev, case, precision)
        assert seen and not set(seen) & set(NEW_ENTRIES), precision
        assert m._engine.last_exact_rays is None
    seen.clear()
    _run(m, dev, case, "auto")
    assert {"cpn_logit_guard", "cpn_select_rays"} <= set(seen)
