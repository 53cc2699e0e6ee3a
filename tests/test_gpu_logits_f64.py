"""The kernels that form the attention logits - cpn_local_units, the logit half of cpn_attend_units (one body,
csrc/local_units_body.h), cpn_local_hidden - each against its float64 reference with an element-wise bound (tests/logits_ref.py;
pinned and calibrated on the CPU by tests/test_logits_ref.py), and the unit-order input copy lv_u of cpn_sample_geometry against
the header's layout built on the host.  No element is left out of any comparison; every output starts as NaN and has guard rows
of a constant behind it; loc8 / coords9 hold 1e4 on every ray outside the window and kh_u 100 on every dead row of a unit.

Observations: the full logit against dlogit (an L1 bound, loose by about sqrt(128)), and every branch element by element - ce
through the stored ce_u of mode 0, key / q2 / the recomputed ce through probe weights under which the other operand is exactly
one-hot, all 128 channels (logits_ref.PROBES).

max err/bound of the first run on an MI355X, the worst over the cases of each kernel and observation:
  cpn_local_units   logit 0.060 (mode 0), 0.032 (mode 2), both at the 4224-unit case; stored ce 0.412, under a leading bias 0.897
                    probes: key 0.922, q2 0.387, the recomputed ce 0.411 (and the bits of mode 0's ce_u)
  cpn_attend_units  logit 0.051 (mode 0), 0.029 (mode 2) at 515 groups on 256 CUs, 0.049 / 0.028 at the LDS limit; at_wt 0.277
                    (gain 16), 0.170 (515 groups); hbar 0.998
  cpn_local_hidden  0.985 (add NULL and given, ldw 16 and 144: the same figures)
The logit bound is L1 over 128 channels: 0.03 - 0.06 is what sqrt(128) of looseness leaves.  Where a ratio sits just under 1 the
fp16 rounding of the output fills the bound (key has no hidden layer in front of it; ce and q2 carry |W2| dh, some 2.5 half-ulps).
The CPU emulation of tests/test_logits_ref.py shows the same figures to three digits.  No defect was found in any kernel.
"""
import functools

import pytest
import torch

from tests import attend_ref
from tests import logits_ref as ref

pytestmark = pytest.mark.gpu

V = ref.V
HC = 1664
GUARD = 64
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _out(rows, cols, dtype, dev):
    """An output of `rows` rows pre-filled with NaN, with GUARD rows of 7 behind it."""
    buf = torch.full((rows + GUARD, cols), NAN, dtype=dtype, device=dev)
    buf[rows:] = 7.0
    return buf


def _take(buf, rows, what, host=True, finite=True):
    """The output rows, after the guard rows were seen intact and every output element finite."""
    torch.cuda.synchronize()
    out = buf.cpu() if host else buf
    assert bool((out[rows:] == 7.0).all()), f"{what}: wrote behind the output"
    if finite:
        assert bool(torch.isfinite(out[:rows].float()).all()), f"{what}: elements left unwritten or not finite"
    return out[:rows]


def _take_ce(ce_u, case, what):
    """The live rows of a stored unit-order coords_embed in row order.  (The dead rows of a unit are written too, from whatever
    their clamped inputs hold - here the 1e4 of a ray outside the window: nothing is asked of them.)"""
    from coponerf_amd.render import rows_from_unit_order
    B, R, S, ray0, nrays, _ = case
    ce = rows_from_unit_order(_take(ce_u, ref.unit_count(B, R, S, ray0, nrays) * 16, what, finite=False), B, R, S, ray0, nrays)
    assert bool(torch.isfinite(ce.float()).all()), f"{what}: live rows left unwritten or not finite"
    return ce


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                     b.view(torch.int16 if b.element_size() == 2 else torch.int32))


# ------------------------------------------------------------------------------------------------------------------
# inputs and launches
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _state(case, dev, hid=False):
    """(the host operands of a case, the same on the device with kh_u and the header-layout lv_u beside them)"""
    B, R, S, ray0, nrays, _ = case
    d = ref.make_inputs(case, hid=hid)
    d["kh_u"] = ref.to_unit_order(d["kh"], B, R, S, ray0, nrays)
    d["lvu"] = ref.lvu_from_loc(d["loc8"], d["coords9"], B, R, S)
    assert d["kh_u"].shape[0] == ref.unit_count(B, R, S, ray0, nrays) * 16 and d["lvu"].shape[0] == ref.total_units(B, R, S) * 64
    g = {k: v.to(dev).contiguous() for k, v in d.items()}
    g["eye"] = torch.eye(128, device=dev)
    g["zero16"] = torch.zeros(128, 128, dtype=torch.float16, device=dev)
    return d, g


def _body(mode, g, wide1=False, wide2=False, over=None):
    """The 17 operand arguments both entry points begin with.  wide1: the first layers inside (128, 144) matrices at column 128,
    as the render path passes query_repeat_embed.weight[:, 128:144]; wide2: the second layers with a leading dimension of 136;
    over: name -> pointer, for the probes."""
    first = lambda k: (g[k + "_144"].data_ptr() + 128 * 4, 144) if wide1 else (g[k].data_ptr(), 16)
    second = lambda k: (g[k + "_136"].data_ptr(), 136) if wide2 else (g[k].data_ptr(), 128)
    p = {"b1": g["b1"].data_ptr(), "b2": g["b2"].data_ptr(), "bk2": g["bk2"].data_ptr(), "b1b": g["b1b"].data_ptr(),
         "w1": first("w1"), "w1b": first("w1b"), "w2": second("w2" if mode == 0 else "w2g"), "wk2": second("wk2")}
    p.update(over or {})
    if mode == 0:
        return (0, g["loc8"].data_ptr(), g["coords9"].data_ptr(), *p["w1"], p["b1"], 0, *p["w2"], p["b2"], *p["wk2"], p["bk2"],
                0, 0, 0, g["kh_u"].data_ptr())
    return (2, g["loc8"].data_ptr(), g["coords9"].data_ptr(), *p["w1"], p["b1"], g["add"].data_ptr(), *p["w2"], p["b2"], *p["wk2"],
            p["bk2"], *p["w1b"], p["b1b"], 0)


def _local_units(case, mode, g, dev, lvu=True, ce_u=None, logits=None, **kw):
    """One cpn_local_units launch -> the logit buffer on the device (not yet read)."""
    from coponerf_amd._hip import call
    B, R, S, ray0, nrays, _ = case
    lg = _out(nrays * V * S, 1, torch.float32, dev) if logits is None else logits
    call("cpn_local_units", *_body(mode, g, **kw), B, V, R, S, ray0, nrays, _ptr(ce_u), g["lvu"].data_ptr() if lvu else 0,
         lg.data_ptr(), _st())
    return lg


@functools.lru_cache(maxsize=None)
def _want(case, mode, dev, on_device=False, led=False):
    """logits_ref of a case: L16 read back out of the lv_u the launch is given (its slot 3 must hold the 1.0), which must be what
    loc8 / coords9 give."""
    B, R, S, ray0, nrays, _ = case
    d, g = _state(case, dev)
    src = g if on_device else d
    L16 = ref.L16_of_lvu(src["lvu"], B, R, S, ray0, nrays)
    assert torch.equal(L16, ref.rows_L16(src["loc8"], src["coords9"], B, R, S, ray0, nrays))
    ops = ref.operands(src, mode)
    return ref.logits_ref(mode, L16, ref.bias_led(ops) if led else ops, S, kh=src["kh"])


@functools.lru_cache(maxsize=None)
def _checked_local_units(case, mode, dev):
    """The logits of cpn_local_units on the host, ASSERTED: lv_u given and NULL, ldw1 = 16 and 144 give the same bits, every
    element is inside dlogit, and (mode 0) the stored ce_u is inside dce element by element."""
    B, R, S, ray0, nrays, _ = case
    _, g = _state(case, dev)
    rows, units = nrays * V * S, ref.unit_count(B, R, S, ray0, nrays)
    what = f"cpn_local_units mode {mode} {ref.case_id(case)}"
    ce_u = _out(units * 16, 128, torch.float16, dev) if mode == 0 else None
    a = _take(_local_units(case, mode, g, dev, lvu=True, ce_u=ce_u), rows, what).view(-1)
    b = _take(_local_units(case, mode, g, dev, lvu=False, wide1=True), rows, what + " lv_u NULL ld 144").view(-1)
    assert _same_bits(a, b), "lv_u = NULL / ldw1 = 144 changes the logits"
    want = _want(case, mode, dev)
    ref.assert_within(what + " logit", a, *want["logit"])
    if mode == 0:
        ref.assert_within(what + " ce", _take_ce(ce_u, case, what + " ce_u"), *want["ce"])
    return a


# ------------------------------------------------------------------------------------------------------------------
# (a) cpn_local_units
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", ref.SMALL_CASES, ids=ref.case_id)
def test_local_units_against_float64(case, mode, dev):
    lg = _checked_local_units(case, mode, dev)
    if case == ref.GAIN16:
        print(f"largest |logit| {float(lg.abs().max()):.1f}")
        assert float(lg.abs().max()) > 200.0
    if case == ref.PLAIN:                                                  # ldw2, ldwk2 > 128 once
        _, g = _state(case, dev)
        wide = _take(_local_units(case, mode, g, dev, wide2=True), lg.numel(), "ld 136").view(-1)
        assert _same_bits(wide, lg), "ldw2 = ldwk2 = 136 changes the logits"


def test_local_units_stored_ce_under_a_leading_bias(dev):
    """ce_u element by element where |W2| dh is small beside ce's own rounding (logits_ref.bias_led): the bound is then within
    1.3 half-ulps, which a conversion rounding the wrong way leaves (tests/test_logits_ref.py, the truncation defect)."""
    case = ref.PLAIN
    B, R, S, ray0, nrays, _ = case
    d, g = _state(case, dev)
    led = {k: v.to(dev) for k, v in ref.bias_led(ref.operands(d, 0)).items()}
    units = ref.unit_count(B, R, S, ray0, nrays)
    ce_u = _out(units * 16, 128, torch.float16, dev)
    lg = _local_units(case, 0, g, dev, ce_u=ce_u, over={"w2": (led["w2"].data_ptr(), 128), "b2": led["b2"].data_ptr()})
    want = _want(case, 0, dev, led=True)
    ref.assert_within("cpn_local_units mode 0 logit, bias-led", _take(lg, nrays * V * S, "bias-led").view(-1), *want["logit"])
    ref.assert_within("cpn_local_units mode 0 ce, bias-led", _take_ce(ce_u, case, "bias-led ce_u"), *want["ce"])


@pytest.mark.parametrize("mode", [0, 2])
def test_local_units_beyond_4096_units(mode, dev):
    """4224 units: the second unit of a wave is live and blocks 0 .. 15 take a second trip (the look-ahead fetch, cur = nxt,
    min(x, nunits - 1)); the float64 products run on the device."""
    case = ref.BIG
    B, R, S, ray0, nrays, _ = case
    assert ref.unit_count(B, R, S, ray0, nrays) == 4224
    _, g = _state(case, dev)
    rows = nrays * V * S
    what = f"cpn_local_units mode {mode} {ref.case_id(case)}"
    a = _take(_local_units(case, mode, g, dev, lvu=True), rows, what, host=False).view(-1)
    b = _take(_local_units(case, mode, g, dev, lvu=False, wide1=True), rows, what + " lv_u NULL", host=False).view(-1)
    assert _same_bits(a, b), "lv_u = NULL changes the logits"
    ref.assert_within(what + " logit", a, *_want(case, mode, dev, on_device=True)["logit"])


@pytest.mark.parametrize("probe", sorted(ref.PROBES))
@pytest.mark.parametrize("case", ref.PROBE_CASES, ids=ref.case_id)
def test_local_units_branches_through_probes(case, probe, dev):
    """One launch per channel c with the other operand exactly e_c: the logit is the fp16 value of channel c of the branch, held
    to the branch's element-wise bound.  The recomputed ce of mode 2 must also be, bit for bit, the ce_u mode 0 stores for the
    same query_embed weights (include/coponerf_hip.h)."""
    B, R, S, ray0, nrays, _ = case
    mode, wkey, bkey, branch = ref.PROBES[probe]
    _, g = _state(case, dev)
    rows = nrays * V * S
    out = [_out(rows, 1, torch.float32, dev) for _ in range(128)]
    for c in range(128):
        _local_units(case, mode, g, dev, lvu=bool(c & 1), logits=out[c],
                     over={wkey: (g["zero16"].data_ptr(), 128), bkey: g["eye"][c].data_ptr()})
    what = f"probe {probe} {ref.case_id(case)}"
    got = torch.stack([_take(o, rows, what).view(-1) for o in out], 1)
    ref.assert_within(what, got, *_want(case, mode, dev)[branch])
    if probe == "ce2":
        units = ref.unit_count(B, R, S, ray0, nrays)
        ce_u = _out(units * 16, 128, torch.float16, dev)
        emb = {"w1": (g["w1b"].data_ptr(), 16), "b1": g["b1b"].data_ptr(), "w2": (g["wk2"].data_ptr(), 128), "b2": g["bk2"].data_ptr()}
        _local_units(case, 0, g, dev, ce_u=ce_u, over=emb)
        assert torch.equal(got, _take_ce(ce_u, case, what + " ce_u").float()), "mode 2 recomputes other bits than mode 0 stores"


# ------------------------------------------------------------------------------------------------------------------
# (b) cpn_attend_units
# ------------------------------------------------------------------------------------------------------------------
def _window_of(buf, B, R, S, ray0, nrays, what):
    """The (nrays, T) window of a (B V R + GUARD, S) weight buffer that started as NaN, on the buffer's device: every entry
    outside the window still holds the sentinel's bits, the guard rows their constant."""
    torch.cuda.synchronize()
    n = B * V * R
    assert bool((buf[n:] == 7.0).all()), f"{what}: wrote behind the output"
    idx = attend_ref.weight_index(B, R, S, ray0, nrays).to(buf.device)
    untouched = torch.ones(n * S, dtype=torch.bool, device=buf.device)
    untouched[idx.reshape(-1)] = False
    sentinel = torch.tensor(NAN).view(torch.int32).to(buf.device)
    assert bool((buf[:n].reshape(-1).view(torch.int32)[untouched] == sentinel).all()), f"{what}: wrote outside the ray window"
    w = buf[:n].reshape(-1)[idx]
    assert bool(torch.isfinite(w).all()), f"{what}: weights left unwritten or not finite"
    return w


def _attend_units(case, mode, g, dev, lvu=True):
    """One cpn_attend_units launch -> (logits, at_wt window, hbar), each checked for guards and sentinels, on the device."""
    from coponerf_amd._hip import call
    B, R, S, ray0, nrays, _ = case
    rows = nrays * V * S
    lg, hbar, wbuf = _out(rows, 1, torch.float32, dev), _out(nrays, HC, torch.float16, dev), _out(B * V * R, S, torch.float32, dev)
    call("cpn_attend_units", *_body(mode, g), g["hid"].data_ptr(), B, V, R, S, ray0, nrays, g["lvu"].data_ptr() if lvu else 0,
         hbar.data_ptr(), wbuf.data_ptr(), lg.data_ptr(), _st())
    what = f"cpn_attend_units mode {mode} {ref.case_id(case)}"
    return (_take(lg, rows, what + " logits", host=False).view(-1), _window_of(wbuf, B, R, S, ray0, nrays, what + " at_wt"),
            _take(hbar, nrays, what + " hbar", host=False))


def _check_softmax_and_sum(what, lg, w, hbar, hid, case):
    """at_wt and hbar against tests/attend_ref.py under the logits the launch stored, with that module's bounds."""
    B, R, S, ray0, nrays, _ = case
    fwd = attend_ref.attend_fwd_ref(None, None, lg, hid, B, R, S, ray0, nrays)
    ref.assert_within(what + " at_wt", w, fwd["w"], fwd["w_bound"])
    ref.assert_within(what + " hbar", hbar, *attend_ref.hbar_ref(w, hid, nrays, S))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", ref.SMALL_CASES, ids=ref.case_id)
def test_attend_units_against_float64(case, mode, dev):
    """The stored logits: the bits of cpn_local_units and inside dlogit; at_wt and hbar under them; lv_u = NULL the same bits."""
    _, g = _state(case, dev, True)
    want = _checked_local_units(case, mode, dev)
    lg, w, hbar = (t.cpu() for t in _attend_units(case, mode, g, dev))
    what = f"cpn_attend_units mode {mode} {ref.case_id(case)}"
    assert _same_bits(lg, want), "the stored logits are not cpn_local_units'"
    ref.assert_within(what + " logit", lg, *_want(case, mode, dev)["logit"])
    _check_softmax_and_sum(what, lg, w, hbar, _state(case, dev, True)[0]["hid"], case)
    lg2, w2, hbar2 = (t.cpu() for t in _attend_units(case, mode, g, dev, lvu=False))
    assert _same_bits(lg2, lg) and _same_bits(w2, w) and _same_bits(hbar2, hbar), "lv_u = NULL changes the result"


@pytest.mark.parametrize("mode", [0, 2])
def test_attend_units_with_several_groups_per_workgroup(mode, dev):
    """2 ncu + 3 ray groups: every workgroup owns two or three, both ring slots are used again and the barrier hand-over between
    the logit waves and the streaming waves takes effect; the first and the last group are partial."""
    from coponerf_amd import streams
    ncu = streams.stream_cus(torch.cuda.current_stream())
    R = 4 * (2 * ncu + 2) + 2
    case = (1, R, 6, 1, R - 2, 1)
    B, R, S, ray0, nrays, _ = case
    groups = ref.unit_count(B, R, S, ray0, nrays) // (V * 2)                 # rays 1 .. R - 2 touch groups 0 .. (R - 2) // 4
    assert groups == 2 * ncu + 3 and 2 * ncu < groups <= 3 * ncu
    _, g = _state(case, dev, True)
    lg, w, hbar = _attend_units(case, mode, g, dev)
    what = f"cpn_attend_units mode {mode} {groups} groups on {ncu} CUs"
    ref.assert_within(what + " logit", lg, *_want(case, mode, dev, on_device=True)["logit"])
    pair = _take(_local_units(case, mode, g, dev), nrays * V * S, what + " cpn_local_units", host=False).view(-1)
    assert _same_bits(lg, pair), "the stored logits are not cpn_local_units'"
    _check_softmax_and_sum(what, lg, w, hbar, g["hid"], case)


@pytest.mark.parametrize("mode", [0, 2])
def test_attend_units_at_the_lds_limit(mode, dev):
    """V S = 1856 (mode 0) / 1684 (mode 2): unit_lds_bytes<MODE>() + 48 V S <= 160 KiB to the last ray-group array; one sample
    more is CPN_E_SHAPE before any launch."""
    from coponerf_amd._hip import call
    case = ref.LIMIT_CASES[mode]
    B, R, S, ray0, nrays, _ = case
    d, g = _state(case, dev, True)
    lg, w, hbar = (t.cpu() for t in _attend_units(case, mode, g, dev))
    what = f"cpn_attend_units mode {mode} {ref.case_id(case)}"
    ref.assert_within(what + " logit", lg, *_want(case, mode, dev)["logit"])
    pair = _take(_local_units(case, mode, g, dev), nrays * V * S, what + " cpn_local_units").view(-1)
    assert _same_bits(lg, pair), "the stored logits are not cpn_local_units'"
    _check_softmax_and_sum(what, lg, w, hbar, d["hid"], case)
    out = _out(64, 64, torch.float32, dev)
    with pytest.raises(RuntimeError, match=r"cpn_attend_units failed \(status -2\)"):
        call("cpn_attend_units", *_body(mode, g), g["hid"].data_ptr(), B, V, R, S + 1, ray0, nrays, 0, out.data_ptr(), out.data_ptr(),
             out.data_ptr(), _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:64]).all()) and bool((out[64:] == 7.0).all()), "a rejected call wrote something"


# ------------------------------------------------------------------------------------------------------------------
# (c) cpn_local_hidden
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.HIDDEN_CASES, ids=ref.case_id)
def test_local_hidden_against_float64(case, dev):
    """fp16(relu(W[:, :16] L16 + bias + add[ray - ray0])) in row order, every element: add NULL and given, ldw = 16 and 144."""
    from coponerf_amd._hip import call
    B, R, S, ray0, nrays, _ = case
    d, g = _state(case, dev)
    rows = nrays * V * S
    L16 = ref.rows_L16(d["loc8"], d["coords9"], B, R, S, ray0, nrays)
    for with_add in (False, True):
        want, bound = ref.local_hidden_ref(L16, d["w1"], d["b1"], ref.add_rows_of(d["add"], S) if with_add else None)
        got = []
        for wptr, ldw in ((g["w1"].data_ptr(), 16), (g["w1_144"].data_ptr() + 128 * 4, 144)):
            out = _out(rows, 128, torch.float16, dev)
            call("cpn_local_hidden", g["loc8"].data_ptr(), g["coords9"].data_ptr(), wptr, ldw, g["b1"].data_ptr(),
                 g["add"].data_ptr() if with_add else 0, B, V, R, S, ray0, nrays, out.data_ptr(), _st())
            what = f"cpn_local_hidden {ref.case_id(case)} add {with_add} ldw {ldw}"
            got.append(_take(out, rows, what))
            ref.assert_within(what, got[-1], want, bound)
        assert _same_bits(got[0], got[1]), "ldw = 144 changes the result"


# ------------------------------------------------------------------------------------------------------------------
# (d) the unit-order copy lv_u of cpn_sample_geometry
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.GEOMETRY_SHAPES, ids=lambda s: "B%d-R%d-S%d" % s)
def test_sample_geometry_unit_order_copy(shape, dev):
    """A layout check: with lv_u the other five outputs keep their bits; lv_u is the header's layout of the loc8 / coords9 the
    same call wrote; every slot is written (NaN fill), the slots of rays >= R / samples >= S are zero, the lanes behind intact."""
    from coponerf_amd import render, synthetic as syn
    from coponerf_amd._hip import call
    B, R, S = shape
    H = W = 64
    N = B * V
    inp = syn.make_inputs(B, H, W, R, seed=4)
    cam, _ = render.build_camera_block(inp["context"]["cam2world"], inp["context"]["intrinsics"], inp["query"]["cam2world"],
                                       inp["query"]["intrinsics"], None, False, H)
    cam = cam.to(dev).contiguous()
    uv = inp["query"]["uv"].reshape(B, R, 2).contiguous().to(dev)
    interval = torch.linspace(0, 1, S).to(dev)
    coords9, seg = torch.zeros(N, R, 9, device=dev), torch.zeros(N, R, 4, device=dev)
    overlaps = torch.zeros(N, R, dtype=torch.uint8, device=dev)
    call("cpn_project_rays", cam.data_ptr(), uv.data_ptr(), 2 * R, B, V, R, coords9.data_ptr(), seg.data_ptr(), overlaps.data_ptr(), _st())
    widths = {"pixel_val": 2, "pt": 3, "sec_grid": 2, "pe6": 6, "loc8": 8}

    def run(lvu):
        o = {k: _out(N * R * S, c, torch.float32, dev) for k, c in widths.items()}
        call("cpn_sample_geometry", cam.data_ptr(), coords9.data_ptr(), seg.data_ptr(), interval.data_ptr(), B, V, R, S, H, W,
             *(o[k].data_ptr() for k in widths), _ptr(lvu), _st())
        torch.cuda.synchronize()
        for k, t in o.items():
            assert bool((t[N * R * S:] == 7.0).all()), f"{k}: wrote behind the output"
            assert not bool(torch.isnan(t[:N * R * S]).any()), f"{k}: elements left unwritten"
        return {k: t[:N * R * S].cpu() for k, t in o.items()}

    lanes = ref.total_units(B, R, S) * 64
    lvu = _out(lanes, 4, torch.float32, dev)
    with_copy, plain = run(lvu), run(None)
    for k in widths:
        assert _same_bits(with_copy[k], plain[k]), f"{k} differs when lv_u is asked for"
    got = lvu.cpu()
    assert bool((got[lanes:] == 7.0).all()), "lv_u: wrote behind the buffer"
    assert not bool(torch.isnan(got[:lanes]).any()), "lv_u: slots left unwritten"
    want = ref.lvu_from_loc(with_copy["loc8"].view(N, R, S, 8), coords9.cpu(), B, R, S)
    dead = (render.unit_rows(B, R, S, 0, B * R) < 0).view(-1, 16)                      # [unit][c]
    slots = got[:lanes].view(-1, 4, 16, 4).permute(0, 2, 1, 3)                         # [unit][c][fg][4]
    assert int(dead.sum()) == lanes // 4 - N * R * S
    assert bool((slots[dead].view(torch.int32) == 0).all()), "a slot of a ray >= R / sample >= S is not +0.0"
    assert bool((slots[~dead][:, 0, 3] == 1.0).all())
    assert _same_bits(got[:lanes], want), "lv_u is not the header's layout of loc8 / coords9"
