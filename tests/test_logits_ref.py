"""The float64 references of tests/logits_ref.py pinned on the CPU - against a dense formula written with plain loops and
torch.nn.functional.linear, the row maps against coponerf_amd.render.unit_rows and the header's lv_u formula - and their bounds
calibrated from both sides with the kernels' rounding points written in fp32 torch: the plain emulation stays inside every bound
on every case the GPU tests use (a scaled-down copy of the 4224-unit one), and each seeded defect of the kind the bounds exist
for leaves the bound of the observation named beside it.  So the GPU tests compare with something that was itself checked.
The emulation decides nothing about the kernels; tests/test_gpu_logits_f64.py does."""
import functools

import pytest
import torch
import torch.nn.functional as F

from coponerf_amd.render import rows_from_unit_order, unit_rows
from tests import logits_ref as ref

V = ref.V


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return ref.make_inputs(case)


# ------------------------------------------------------------------------------------------------------------------
# the kernels' rounding points in fp32 torch, in row order; `defect` seeds one of the mistakes the bounds must catch
# ------------------------------------------------------------------------------------------------------------------
def _split(x):
    hi = x.half()
    return hi.float(), (x - hi.float()).half().float()


def _trunc_half(x):
    """fp32 -> fp16 rounded toward zero."""
    h = x.half()
    over = h.float().abs() > x.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)


def emu_first(x, W1, b1, add_rows, defect=None, which=""):
    """fp16(relu(.)) of the K = 16 layer as three hi / lo products on an fp32 accumulator that starts at the add row; x (rows, 16)
    fp32 with 1.0 on slot 3, which the bias rides on."""
    w = W1[:, :16].clone()
    w[:, 3] = 0.0 if defect == "first-layer bias dropped" + which else b1
    if defect == "input slot 12 dropped":
        x = x.clone()
        x[:, 12] = 0.0
    wh, wl = _split(w)
    xh, xl = _split(x)
    acc = torch.zeros(x.shape[0], 128) if add_rows is None else add_rows.clone()
    acc = acc + xh @ wl.t()
    acc = acc + xl @ wh.t()
    acc = acc + xh @ wh.t()
    h = acc.half()
    return h if defect == "no ReLU" + which else torch.relu(h)


def emu_layer128(h16, W2, b2, defect=None, which=""):
    out = b2 + h16.float() @ W2[:, :128].float().t()
    if defect == "second-layer bias dropped" + which:
        out = out - b2
    o16 = _trunc_half(out) if defect == "truncation" + which else out.half()
    if defect == "4-channel blocks swapped" + which:
        o16 = o16.clone()
        o16[:, 0:8] = torch.cat((o16[:, 4:8], o16[:, 0:4]), 1)
    return o16


def emu_add_rows(add, case, defect):
    B, R, S, ray0, nrays, _ = case
    t = torch.arange(nrays)
    if defect == "add row from ray":
        t = torch.clamp(t + ray0, max=nrays - 1)                        # (the kernel clamps the row it reads)
    if defect == "neighbour's add row for the last ray":
        t[-1] = nrays - 2
    return add[t].repeat_interleave(V * S, 0)


def emu_logits(mode, x, d, case, kh=None, defect=None):
    """cpn_local_units in row order -> dict of the fp16 branches and the fp32 logit."""
    B, R, S, ray0, nrays, _ = case
    dot = lambda a, b: (a.float() * b.float()).sum(1)
    if mode == 0:
        ce = emu_layer128(emu_first(x, d["w1"], d["b1"], None, defect, " (ce)"), d["w2"], d["b2"], defect, " (ce)")
        key = emu_layer128(kh, d["wk2"], d["bk2"], defect, " (key)")
        out = {"ce": ce, "key": key, "logit": dot(key, ce)}
    else:
        q2 = emu_layer128(emu_first(x, d["w1"], d["b1"], emu_add_rows(d["add"], case, defect), defect, " (q2)"), d["w2"], d["b2"],
                          defect, " (q2)")
        ce = emu_layer128(emu_first(x, d["w1b"], d["b1b"], None, defect, " (ce)"), d["wk2"], d["bk2"], defect, " (ce)")
        out = {"q2": q2, "ce": ce, "logit": dot(q2, ce)}
    if defect == "unit row map transposed":
        # slot c of a unit is taken for sample c & 3, ray c >> 2: the logit of slot c lands on the row of slot (c & 3) 4 + (c >> 2)
        idx = unit_rows(B, R, S, ray0, nrays).view(-1, 16)
        c = torch.arange(16)
        to = idx[:, (c & 3) * 4 + (c >> 2)]
        ok = (idx >= 0) & (to >= 0)
        lg = out["logit"].clone()
        lg[to[ok]] = out["logit"][idx[ok]]
        out["logit"] = lg
    return out


def emu_local_hidden(L16, W, bias, add_rows):
    acc = bias.expand(L16.shape[0], 128) if add_rows is None else bias + add_rows
    return torch.relu(acc + L16.float() @ W[:, :16].t()).half()


def _rows32(d, case):
    """The rows' 16 K slots in fp32 as the kernel multiplies them: through lv_u in the header's layout."""
    B, R, S, ray0, nrays, _ = case
    return ref.rows_from_lvu(ref.lvu_from_loc(d["loc8"], d["coords9"], B, R, S), B, R, S, ray0, nrays)


@functools.lru_cache(maxsize=None)
def _ref(case, mode):
    B, R, S, ray0, nrays, _ = case
    d = _inputs(case)
    return ref.logits_ref(mode, ref.rows_L16(d["loc8"], d["coords9"], B, R, S, ray0, nrays), ref.operands(d, mode), S, kh=d["kh"])


# ------------------------------------------------------------------------------------------------------------------
# the references and the row maps
# ------------------------------------------------------------------------------------------------------------------
def test_references_equal_a_dense_formula():
    """Every row of a tiny case, one at a time: L16 gathered by explicit index, the layers with torch.nn.functional.linear."""
    case = ref.SHORT
    B, R, S, ray0, nrays, _ = case
    d = _inputs(case)
    r0, r2 = _ref(case, 0), _ref(case, 2)
    hid_want, _ = ref.local_hidden_ref(ref.rows_L16(d["loc8"], d["coords9"], B, R, S, ray0, nrays), d["w1"], d["b1"],
                                       ref.add_rows_of(d["add"], S))
    f64 = lambda k: d[k].double()
    row = 0
    for ray in range(ray0, ray0 + nrays):
        b, r = divmod(ray, R)
        for v in range(V):
            for s in range(S):
                l8, c9 = f64("loc8")[b * V + v, r, s], f64("coords9")[b * V + v, r]
                x = torch.tensor([l8[0], l8[1], l8[2], 0, 0, 0, c9[0], c9[1], c9[2], l8[3], l8[4], l8[5], l8[6], c9[6], c9[7], c9[8]],
                                 dtype=torch.float64)
                ce = F.linear(torch.relu(F.linear(x, f64("w1"), f64("b1"))), f64("w2"), f64("b2"))
                key = F.linear(f64("kh")[row], f64("wk2"), f64("bk2"))
                pre = F.linear(x, f64("w1"), f64("b1")) + f64("add")[ray - ray0]
                q2 = F.linear(torch.relu(pre), f64("w2g"), f64("b2"))
                ce2 = F.linear(torch.relu(F.linear(x, f64("w1b"), f64("b1b"))), f64("wk2"), f64("bk2"))
                for want, got in ((ce, r0["ce"][0][row]), (key, r0["key"][0][row]), (ce @ key, r0["logit"][0][row]),
                                  (q2, r2["q2"][0][row]), (ce2, r2["ce"][0][row]), (q2 @ ce2, r2["logit"][0][row]),
                                  (torch.relu(pre), hid_want[row])):
                    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)
                row += 1
    assert row == nrays * V * S


@pytest.mark.parametrize("case", [ref.PLAIN, ref.WINDOW, ref.SHORT], ids=ref.case_id)
def test_unit_order_helpers_follow_the_header(case):
    """lv_u built on the host holds, in lane c + 16 fg of unit ((b ceil(R/4) + r/4) V + v) ceil(S/4) + s/4, the four K entries the
    header names, zeros in the slots of no row; the window's rows come back out of it; to_unit_order inverts rows_from_unit_order."""
    B, R, S, ray0, nrays, _ = case
    d = _inputs(case)
    lvu = ref.lvu_from_loc(d["loc8"], d["coords9"], B, R, S).view(-1, 64, 4)
    gpb, nsblk = (R + 3) // 4, (S + 3) // 4
    assert lvu.shape[0] == ref.total_units(B, R, S)
    seen = torch.zeros(lvu.shape[0], 64, dtype=torch.bool)
    for b in range(B):
        for r in range(R):
            for v in range(V):
                for s in range(S):
                    l8, c9 = d["loc8"][b * V + v, r, s], d["coords9"][b * V + v, r]
                    k16 = [l8[0], l8[1], l8[2], 1.0, 0.0, 0.0, c9[0], c9[1], c9[2], l8[3], l8[4], l8[5], l8[6], c9[6], c9[7], c9[8]]
                    u, c = ((b * gpb + r // 4) * V + v) * nsblk + s // 4, (s & 3) * 4 + (r & 3)
                    for fg in range(4):
                        assert lvu[u, c + 16 * fg].tolist() == [float(k) for k in k16[4 * fg:4 * fg + 4]]
                        seen[u, c + 16 * fg] = True
    assert bool((lvu[~seen] == 0).all())
    x = ref.rows_from_lvu(lvu, B, R, S, ray0, nrays)
    want = ref.rows_L16(d["loc8"], d["coords9"], B, R, S, ray0, nrays).float()
    want[:, 3] = 1.0
    assert torch.equal(x, want)
    assert torch.equal(ref.L16_of_lvu(lvu, B, R, S, ray0, nrays), ref.rows_L16(d["loc8"], d["coords9"], B, R, S, ray0, nrays))
    kh_u = ref.to_unit_order(d["kh"], B, R, S, ray0, nrays)
    assert kh_u.shape == (ref.unit_count(B, R, S, ray0, nrays) * 16, 128)
    assert torch.equal(rows_from_unit_order(kh_u, B, R, S, ray0, nrays), d["kh"])
    assert int((kh_u == ref.DEAD).sum()) == 128 * int((unit_rows(B, R, S, ray0, nrays) < 0).sum())


def test_the_cases_reach_what_they_are_for():
    B, R, S, ray0, nrays, _ = ref.BIG
    assert ref.unit_count(B, R, S, ray0, nrays) == 4224 > 2 * 8 * 256
    assert ref.unit_count(*ref.BIG_SMALL[:5]) == 6 * 2 * 3
    for mode, (B, R, S, ray0, nrays, _) in ref.LIMIT_CASES.items():
        lds = (65536 + 1024 + 8192 if mode == 0 else 65536 + 1024 + 16384) + 48 * V * S
        assert lds <= 160 * 1024 < lds + 48 * V
    for case in (ref.PLAIN, ref.WINDOW, ref.ONE_RAY, ref.SHORT):             # each has dead rows inside live units
        assert bool((unit_rows(*case[:5]) < 0).any())


# ------------------------------------------------------------------------------------------------------------------
# the bounds from both sides
# ------------------------------------------------------------------------------------------------------------------
_worst = {}


def _note(key, r):
    _worst[key] = max(_worst.get(key, 0.0), r)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", ref.EMU_CASES, ids=ref.case_id)
def test_emulation_is_inside_every_bound(case, mode):
    d = _inputs(case)
    got = emu_logits(mode, _rows32(d, case), ref.operands(d, mode), case, kh=d["kh"])
    want = _ref(case, mode)
    for name, (w, b) in want.items():
        _note((mode, name), ref.assert_within(f"emulation mode {mode} {name} {ref.case_id(case)}", got[name], w, b))
    print("worst so far:", {k: round(v, 3) for k, v in sorted(_worst.items())})


def test_emulation_is_inside_the_bias_led_ce_bound():
    d = _inputs(ref.PLAIN)
    ops = ref.bias_led(ref.operands(d, 0))
    want, bound = ref.logits_ref(0, ref.rows_L16(d["loc8"], d["coords9"], *ref.PLAIN[:5]), ops, ref.PLAIN[2], kh=d["kh"])["ce"]
    ref.assert_within("emulation mode 0 ce, bias-led", emu_logits(0, _rows32(d, ref.PLAIN), ops, ref.PLAIN, kh=d["kh"])["ce"], want, bound)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("case", ref.HIDDEN_CASES, ids=ref.case_id)
def test_local_hidden_emulation_is_inside_its_bound(case, with_add):
    B, R, S, ray0, nrays, _ = case
    d = _inputs(case)
    L16 = ref.rows_L16(d["loc8"], d["coords9"], B, R, S, ray0, nrays)
    add_rows = ref.add_rows_of(d["add"], S) if with_add else None
    want, bound = ref.local_hidden_ref(L16, d["w1"], d["b1"], add_rows)
    ref.assert_within(f"emulation local_hidden {ref.case_id(case)}", emu_local_hidden(L16, d["w1"], d["b1"], add_rows), want, bound)
    defect = emu_local_hidden(L16.roll(1, 1), d["w1"], d["b1"], add_rows)             # the 16 inputs one slot off
    assert ref.outside(defect, want, bound) > 0


def test_a_probe_shows_one_channel_of_one_branch():
    """Under the probe weights the emulated logit IS the fp16 value of that channel: exactly, for every probe and a few channels."""
    case = ref.WINDOW
    d = _inputs(case)
    x = _rows32(d, case)
    eye = torch.eye(128)
    for name, (mode, _, bkey, branch) in ref.PROBES.items():
        ops = ref.operands(d, mode)
        plain = emu_logits(mode, x, ops, case, kh=d["kh"])
        for c in (0, 5, 64, 127):
            p = ref.probe_operands(ops, name, eye)
            p[bkey] = eye[c]
            got = emu_logits(mode, x, p, case, kh=d["kh"])
            assert torch.equal(got["logit"], plain[branch][:, c].float()), (name, c)


# defect -> (case, mode, the observation whose bound it must leave: the full logits or a probe / the stored ce)
DEFECTS = {
    "4-channel blocks swapped (ce)": (ref.PLAIN, 0, "logit"),
    "4-channel blocks swapped (q2)": (ref.PLAIN, 2, "q2"),
    "input slot 12 dropped": (ref.PLAIN, 0, "logit"),                      # tanh(depth / 1000)
    "second-layer bias dropped (key)": (ref.PLAIN, 0, "key"),
    "first-layer bias dropped (q2)": (ref.PLAIN, 2, "q2"),
    "add row from ray": (ref.WINDOW, 2, "q2"),
    "neighbour's add row for the last ray": (ref.WINDOW, 2, "q2"),
    "truncation (ce)": (ref.PLAIN, 0, "ce, bias-led"),                     # (hidden behind |W2| dh at the plain scales: ref.bias_led)
    "no ReLU (ce)": (ref.PLAIN, 0, "logit"),
    "unit row map transposed": (ref.PLAIN, 0, "logit"),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_seeded_defect_leaves_the_bound(defect):
    case, mode, seen_by = DEFECTS[defect]
    d = _inputs(case)
    ops, want = ref.operands(d, mode), _ref(case, mode)
    if seen_by.endswith(", bias-led"):
        seen_by = seen_by[:-len(", bias-led")]
        ops = ref.bias_led(ops)
        want = ref.logits_ref(mode, ref.rows_L16(d["loc8"], d["coords9"], *case[:5]), ops, case[2], kh=d["kh"])
    got = emu_logits(mode, _rows32(d, case), ops, case, kh=d["kh"], defect=defect)
    want, bound = want[seen_by]
    n = ref.outside(got[seen_by], want, bound)
    print(f"{defect}: {n} of {want.numel()} elements of `{seen_by}` (mode {mode}, {ref.case_id(case)}) leave the bound")
    assert n > 0
    if defect == "neighbour's add row for the last ray":                   # only the last ray's rows may be off
        T = V * case[2]
        assert ref.outside(got[seen_by][:-T], want[:-T], bound[:-T]) == 0
