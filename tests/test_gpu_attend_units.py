"""cpn_attend_units (one launch per attention round) against the two kernels it is made of, cpn_local_units followed by
cpn_attend_hidden: the SAME BITS — hbar, at_wt and the optional raw logits with torch.equal, no tolerance (the logits come from
the same device functions, the softmax reproduces attend_hidden_ray's association, the weighted sum keeps the row order).
Runs on a real MI355X (`pytest -m gpu`); the binding test at the end needs no GPU."""
import pytest
import torch

from coponerf_amd import _hip, synthetic as syn
from tests.helpers import load_case, case_inputs, to_device

V = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _groups(R, ray0, nrays):
    """first ray group of a call and how many it touches (csrc/local_units_body.h, unit_geo)"""
    gpb = (R + 3) // 4
    b_lo, b_hi = ray0 // R, (ray0 + nrays - 1) // R
    g0 = b_lo * gpb + (ray0 - b_lo * R) // 4
    g1 = b_hi * gpb + (ray0 + nrays - 1 - b_hi * R) // 4
    return g0, g1 - g0 + 1


def _inputs(dev, mode, B, R, S, ray0, nrays, gain=1.0, seed=3):
    """operands of one attention round from the counter-hash generators; `gain` scales the operand the logits are linear in"""
    N, T = B * V, V * S
    nsblk = (S + 3) // 4
    _, ngroups = _groups(R, ray0, nrays)
    f16 = torch.float16
    d = {
        "loc8": syn.uniform((N, R, S, 8), seed, -1.0, 1.0, stream=1),
        "coords9": syn.uniform((N, R, 9), seed, -1.0, 1.0, stream=2),
        "w1": syn.normal((128, 16), seed, 0.5, stream=3), "b1": syn.normal((128,), seed, 0.1, stream=4),
        "w2": syn.normal((128, 128), seed, 0.1, stream=5).to(f16), "b2": syn.normal((128,), seed, 0.1, stream=6),
        "wk2": syn.normal((128, 128), seed, 0.1, stream=7).to(f16), "bk2": syn.normal((128,), seed, 0.1, stream=8),
        "w1b": syn.normal((128, 16), seed, 0.5, stream=9), "b1b": syn.normal((128,), seed, 0.1, stream=10),
        "add": syn.normal((nrays, 128), seed, 0.3, stream=11),
        "kh": syn.normal((ngroups * V * nsblk * 16, 128), seed, 1.0, stream=12).to(f16),
        "lvu": syn.uniform((B * ((R + 3) // 4) * V * nsblk * 64, 4), seed, -1.0, 1.0, stream=13),
        "hid": syn.uniform((nrays * T * 2, 832), seed, 0.0, 2.0, stream=14).to(f16),
    }
    if mode == 0:
        d["kh"] = (d["kh"].float() * gain).to(f16)                 # key_map_2 is linear in kh
    else:
        d["w2"] = (d["w2"].float() * gain).to(f16)                 # the second query is linear in query_repeat_embed_2
    return {k: v.to(dev).contiguous() for k, v in d.items()}


def _body_args(mode, d, use_lvu):
    p = lambda k: d[k].data_ptr()
    if mode == 0:
        return (0, p("loc8"), p("coords9"), p("w1"), 16, p("b1"), 0, p("w2"), 128, p("b2"), p("wk2"), 128, p("bk2"), 0, 0, 0, p("kh"))
    return (2, p("loc8"), p("coords9"), p("w1"), 16, p("b1"), p("add"), p("w2"), 128, p("b2"), p("wk2"), 128, p("bk2"),
            p("w1b"), 16, p("b1b"), 0)


def _run_both(dev, mode, B, R, S, ray0, nrays, gain=1.0, use_lvu=True, want_logits=True):
    d = _inputs(dev, mode, B, R, S, ray0, nrays, gain)
    T = V * S
    s = torch.cuda.current_stream().cuda_stream
    body = _body_args(mode, d, use_lvu)
    lvu = d["lvu"].data_ptr() if use_lvu else 0
    new = lambda: (torch.zeros(nrays, 1664, dtype=torch.float16, device=dev), torch.zeros(B * V, R, S, device=dev),
                   torch.zeros(nrays * T, device=dev))
    hbar_p, wt_p, lg_p = new()
    _hip.call("cpn_local_units", *body, B, V, R, S, ray0, nrays, 0, lvu, lg_p.data_ptr(), s)
    _hip.call("cpn_attend_hidden", 0, 0, lg_p.data_ptr(), d["hid"].data_ptr(), B, V, R, S, ray0, nrays, hbar_p.data_ptr(),
              wt_p.data_ptr(), s)
    hbar_u, wt_u, lg_u = new()
    _hip.call("cpn_attend_units", *body, d["hid"].data_ptr(), B, V, R, S, ray0, nrays, lvu, hbar_u.data_ptr(), wt_u.data_ptr(),
              lg_u.data_ptr() if want_logits else 0, s)
    torch.cuda.synchronize()
    return (hbar_p, wt_p, lg_p), (hbar_u, wt_u, lg_u)


# (B, R, S, ray0, nrays): the bench shape scaled down; R and S no multiples of 4; a window that starts and ends inside a ray group
# and crosses the batch boundary (R = 38: rays 17 .. 46 = b 0 from r = 17 (group 4 is 16 .. 19) to b 1 r = 8 (group 2 is 8 .. 11));
# one ray; S = 128
SHAPES = [(1, 256, 64, 0, 256), (1, 37, 30, 0, 37), (2, 38, 16, 17, 30), (1, 37, 30, 22, 1), (1, 24, 128, 0, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_entry_equals_the_pair(dev, mode, shape):
    pair, unit = _run_both(dev, mode, *shape)
    assert torch.isfinite(pair[0].float()).all() and torch.isfinite(pair[1]).all()
    assert float(pair[1].sum()) > 0.0
    for name, a, b in zip(("hbar", "at_wt", "logits"), pair, unit):
        print(f"mode {mode} shape {shape} {name}: differing elements {int((a != b).sum())} of {a.numel()}")
    for name, a, b in zip(("hbar", "at_wt", "logits"), pair, unit):
        assert torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
def test_entry_equals_the_pair_without_unit_order_inputs_and_logits(dev, mode):
    """lv_u = NULL (the body gathers loc8 / coords9 itself) and logits = NULL (nothing stored)"""
    pair, unit = _run_both(dev, mode, 1, 37, 30, 5, 30, use_lvu=False, want_logits=False)
    assert torch.equal(pair[0], unit[0]) and torch.equal(pair[1], unit[1])
    assert int((unit[2] != 0).sum()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
def test_entry_equals_the_pair_on_a_peaked_softmax(dev, mode):
    """logits scaled away from the flat regime: the largest weight of the call exceeds 0.5"""
    pair, unit = _run_both(dev, mode, 1, 64, 64, 0, 64, gain=16.0)
    assert torch.isfinite(pair[0].float()).all() and torch.isfinite(pair[1]).all()
    print(f"mode {mode}: largest softmax weight {float(pair[1].max()):.4f}")
    assert float(pair[1].max()) > 0.5
    for name, a, b in zip(("hbar", "at_wt", "logits"), pair, unit):
        assert torch.equal(a, b), name


def test_rejects_what_lds_cannot_hold():
    """V*S = 2048: three 4-ray arrays of it do not fit beside the weights - a status code before any launch (no GPU needed)"""
    with pytest.raises(RuntimeError, match="cpn_attend_units"):
        _hip.call("cpn_attend_units", 0, 16, 16, 16, 16, 16, 0, 16, 128, 16, 16, 128, 16, 0, 0, 0, 16, 16, 1, 2, 4, 1024, 0, 4, 0,
                  16, 0, 0, None)


@pytest.mark.gpu
def test_render_equals_render_with_the_pair(dev, monkeypatch):
    """render() of the c1_val inputs: rgb, at_wt, z_local equal to what the same engine returns when each cpn_attend_units call is
    replaced, from here, by the two kernels it stands for."""
    from coponerf_amd import CoPoNeRF, render
    cfg, _ = load_case("c1_val")
    weights = syn.make_render_weights()
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    model.load_state_dict(weights, strict=False)
    model = model.to(dev).eval()
    model.npoints = cfg["S"]
    inp, z, rel, flow = case_inputs(cfg)

    def run():
        with torch.no_grad():
            out = model(to_device(inp, dev), z=to_device(z, dev), rel_pose=rel.to(dev), val=cfg["val"], flow=to_device(flow, dev),
                        debug=True)
        torch.cuda.synchronize()
        return out["rgb"].clone(), out["at_wt"].clone(), out["_core"]["z_local"].clone()

    got = run()
    calls = []

    def with_the_pair(name, *a):
        if name != "cpn_attend_units":
            return _hip.call(name, *a)
        body, hid, dims, lvu, hbar, at_wt, logits, stream = a[:17], a[17], a[18:24], a[24], a[25], a[26], a[27], a[28]
        Bq, Vq, Rq, Sq, ray0, n = dims
        lg = torch.empty(n * Vq * Sq, device=dev)
        calls.append(lg)                                            # alive until the stream has run
        _hip.call("cpn_local_units", *body, *dims, 0, lvu, lg.data_ptr(), stream)
        _hip.call("cpn_attend_hidden", 0, 0, lg.data_ptr(), hid, *dims, hbar, at_wt, stream)

    monkeypatch.setattr(render, "call", with_the_pair)
    want = run()
    assert len(calls) >= 2
    for name, a, b in zip(("rgb", "at_wt", "z_local"), want, got):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), name


def test_attend_units_is_bound():
    """the SIGNATURES row has the header declaration's argument count (tests/test_cabi.py: the library exports the symbol)"""
    import re
    assert "cpn_attend_units" in _hip.SIGNATURES and "cpn_attend_units" in _hip.declared_symbols()
    with open(_hip.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"\bint\s+cpn_attend_units\s*\(([^)]*)\)", text).group(1)
    assert len(decl.split(",")) == len(_hip.SIGNATURES["cpn_attend_units"]) == 29
    # the pair's operands, minus ce_u (nothing of coords_embed is stored), plus hid / hbar / at_wt
    assert len(_hip.SIGNATURES["cpn_attend_units"]) == len(_hip.SIGNATURES["cpn_local_units"]) - 1 + 3
    assert _hip.ABI_VERSION == 12
