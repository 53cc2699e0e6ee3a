"""The float64 references of tests/attend_ref.py pinned on the CPU - the adjoint against float64 autograd of the forward, the
combine against a dense formula - and their bounds calibrated from both sides with the kernels' arithmetic written in fp32
torch: the plain emulation stays inside every bound on every case the GPU tests use, and each of four seeded defects of the
kind the bounds exist for leaves them.  So the GPU tests compare with something that was itself checked."""
import functools

import pytest
import torch

from tests import attend_ref as ref

V, HC = ref.V, ref.HC
F_SCALE = torch.tensor(11.31, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return ref.make_inputs(case)


# ------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32 torch (fp16 outputs); `defect` seeds one of the mistakes the bounds must catch
# ------------------------------------------------------------------------------------------------------------------
def emu_fwd(qa, qb, logits, hid, B, R, S, ray0, nrays):
    """cpn_attend_hidden: -> (at_wt (B V, R, S) fp32 with NaN outside the window, hbar (nrays, 1664) fp16)."""
    T = V * S
    l = ((qa.float() * qb.float()).sum(1) if logits is None else logits) / F_SCALE
    l = l.view(nrays, T)
    e = torch.exp(l - l.max(1, keepdim=True).values)
    w = e * (1.0 / e.sum(1, keepdim=True))
    hbar = (w.unsqueeze(-1) * hid.float().view(nrays, T, HC)).sum(1).half()
    return ref.to_global(w, B, R, S, ray0, nrays), hbar


def emu_bwd(qa, qb, hid, at_wt, dhbar, dw_ext, acc, B, R, S, ray0, nrays, defect=None):
    """cpn_attend_hidden_bwd: at_wt / dw_ext global, everything else launch-local -> (dqa, dqb, dhid) fp16."""
    T = V * S
    idx = ref.weight_index(B, R, S, 0 if defect == "ray0 dropped" else ray0, nrays)
    w = at_wt.reshape(-1)[idx]
    h = hid.float().view(nrays, T, HC)
    g = dhbar.view(nrays, HC, 1)
    if defect == "last chunk dropped":
        dw = torch.bmm(h[:, :, :HC - 8], g[:, :HC - 8]).squeeze(-1)
    else:
        dw = torch.bmm(h, g).squeeze(-1)
    if dw_ext is not None:
        dw = dw + dw_ext.reshape(-1)[idx]
    n = T - T % 4 if defect == "dot over T - T % 4 rows" else T
    dot = (w[:, :n] * dw[:, :n]).sum(1, keepdim=True)
    dl = (w * (dw - dot) / F_SCALE).unsqueeze(-1)
    a, b = qa.float().view(nrays, T, 128), qb.float().view(nrays, T, 128)
    dqa = (dl * b).half()
    if acc is None:
        dqb = (dl * a).half()
    else:
        p = acc.float().view(nrays, T, 128)
        dqb = ((p + p if defect == "dqb_acc twice" else p) + dl * a).half()
    dhid = (w.unsqueeze(-1) * dhbar.view(nrays, 1, HC)).half()
    return dqa.view(-1, 128), dqb.view(-1, 128), dhid.view(-1, HC)


def emu_combine(dkey, hid, w1, dh1, w2, dh2, B, R, S, ray0, nrays):
    """cpn_hid_grad_combine on the (nrays T, 1664) view: w1 / w2 global."""
    T = V * S
    idx = ref.weight_index(B, R, S, ray0, nrays)
    acc = dkey.float().view(nrays, T, HC).clone() if dkey is not None else torch.zeros(nrays, T, HC)
    for w, dh in ((w1, dh1), (w2, dh2)):
        if w is not None:
            acc += w.reshape(-1)[idx].unsqueeze(-1) * dh.view(nrays, 1, HC)
    return torch.where(hid.float().view(nrays, T, HC) > 0, acc.half(), torch.zeros((), dtype=torch.float16)).view(-1, HC)


def _emulated_backward(case, defect=None, with_ext=True):
    """(emulated dqa, dqb, dhid; the reference dict) of a case, the weights coming from the emulated forward."""
    B, R, S, gain, ray0, nrays = case
    x = _inputs(case)
    at_wt, _ = emu_fwd(x["qa"], x["qb"], None, x["hid"], B, R, S, ray0, nrays)
    ext, acc = (x["dw_ext"], x["acc"]) if with_ext else (None, None)
    got = emu_bwd(x["qa"], x["qb"], x["hid"], at_wt, x["dhbar"], ext, acc, B, R, S, ray0, nrays, defect)
    w = ref.from_global(at_wt, B, R, S, ray0, nrays)
    ext_l = ref.from_global(ext, B, R, S, ray0, nrays) if with_ext else None
    want = ref.attend_bwd_ref(x["qa"], x["qb"], x["hid"], w, x["dhbar"], ext_l, acc, S, nrays, want_dhid=True)
    return got, want


# ------------------------------------------------------------------------------------------------------------------
# 1. the references are pinned
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ref.PLAIN, ref.WINDOW, ref.RAGGED, ref.SHORT], ids=ref.case_id)
def test_backward_reference_is_the_float64_autograd_of_the_forward_reference(case):
    """attend_bwd_ref against autograd through attend_fwd_ref with the loss sum hbar dhbar + sum w dw_ext, the weights laid out
    (B V, R, S) through weight_index and dw_ext given in that layout: 1e-12 relative to the largest entry."""
    B, R, S, gain, ray0, nrays = case
    T = V * S
    x = _inputs(case)
    qa = x["qa"].double().requires_grad_(True)
    qb = x["qb"].double().requires_grad_(True)
    hid = x["hid"].double().requires_grad_(True)
    fwd = ref.attend_fwd_ref(qa, qb, None, hid, B, R, S, ray0, nrays)
    ext = torch.nan_to_num(x["dw_ext"].double(), nan=0.0)
    w_glob = torch.zeros(B * V * R * S, dtype=torch.float64).index_put((fwd["idx"].reshape(-1),), fwd["w"].reshape(-1))
    ((fwd["hbar"] * x["dhbar"].double()).sum() + (w_glob.view(B * V, R, S) * ext).sum()).backward()
    got = ref.attend_bwd_ref(x["qa"], x["qb"], x["hid"], fwd["w"].detach(), x["dhbar"],
                             ref.from_global(x["dw_ext"], B, R, S, ray0, nrays), x["acc"], S, nrays, want_dhid=True)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(got["dqa"], qa.grad) <= 1e-12
    assert rel(got["dqb"] - x["acc"].double(), qb.grad) <= 1e-12
    assert rel(got["dhid"], hid.grad) <= 1e-12
    # logits mode of the forward: the same weights from the row dots themselves
    dots = (x["qa"].double() * x["qb"].double()).sum(1)
    assert rel(ref.attend_fwd_ref(None, None, dots, x["hid"], B, R, S, ray0, nrays)["w"], fwd["w"].detach()) <= 1e-12


def test_weight_index_is_the_layout_of_the_header():
    """(b V + v, r, s) of ray b R + r, written out with loops."""
    B, R, S, ray0, nrays = 3, 3, 4, 2, 6
    idx = ref.weight_index(B, R, S, ray0, nrays)
    for t in range(nrays):
        b, r = (ray0 + t) // R, (ray0 + t) % R
        for v in range(V):
            for s in range(S):
                assert int(idx[t, v * S + s]) == ((b * V + v) * R + r) * S + s
    out = ref.outside_window(B, R, S, ray0, nrays)
    assert int((~out).sum()) == nrays * V * S and bool(out[0, :2].all()) and bool(out[5, 2].all()) and not bool(out[4, 1].any())


@pytest.mark.parametrize("case", ref.COMBINE_CASES, ids=ref.case_id)
def test_combine_reference_against_the_dense_formula(case):
    B, R, S, gain, ray0, nrays = case
    x = ref.make_combine_inputs(case)
    w1, w2 = (ref.from_global(x[k], B, R, S, ray0, nrays) for k in ("w1", "w2"))
    want, bound, live = ref.combine_ref(x["dkey"], x["hid"], w1, x["dh1"], w2, x["dh2"], S, nrays)
    rep = lambda dh: dh.double().repeat_interleave(V * S, 0)
    dense = x["dkey"].double() + w1.double().reshape(-1, 1) * rep(x["dh1"]) + w2.double().reshape(-1, 1) * rep(x["dh2"])
    dense = dense * (x["hid"].double() > 0)
    assert float((want - dense).abs().max()) <= 1e-12 * float(dense.abs().max())
    neg_zero = x["hid"].view(torch.int16) == -32768
    assert bool(neg_zero.any()) and not bool(live[neg_zero].any()) and bool((bound[~live] == 0).all())
    # the (rows 2, 832) view of the kernel is the same memory: row = ((t V + v) S + s) 2 + j, column 832 j + c
    assert torch.equal(want.view(-1, 832)[5], want[2, 832:])


# ------------------------------------------------------------------------------------------------------------------
# 2. the bounds admit a correct kernel
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["qa.qb", "logits"])
@pytest.mark.parametrize("case", ref.EMU_CASES, ids=ref.case_id)
def test_bounds_admit_the_fp32_forward(case, mode):
    B, R, S, gain, ray0, nrays = case
    x = _inputs(case)
    lg = x["logits"] if mode == "logits" else None
    at_wt, hbar = emu_fwd(x["qa"], x["qb"], lg, x["hid"], B, R, S, ray0, nrays)
    fwd = ref.attend_fwd_ref(x["qa"], x["qb"], lg, x["hid"], B, R, S, ray0, nrays)
    w = ref.from_global(at_wt, B, R, S, ray0, nrays)
    ref.assert_within(f"emulated weights {mode}", w, fwd["w"], fwd["w_bound"])
    for name, t in fwd["terms"].items():
        print(f"    err / (w * {name} term) = {float(ref.ratio(w, fwd['w'], fwd['w'] * t).max()):.3f}")
    want, bound = ref.hbar_ref(w, x["hid"], nrays, S)
    ref.assert_within(f"emulated hbar {mode}", hbar, want, bound)
    if case == ref.PEAKED:
        assert float(fwd["w"].max()) > 0.3
    if case == ref.RAGGED:
        assert float(fwd["w"].max()) > 0.25


@pytest.mark.parametrize("with_ext", [True, False], ids=["ext+acc", "plain"])
@pytest.mark.parametrize("case", [c for c in ref.EMU_CASES if c != ref.LIMIT_FWD], ids=ref.case_id)
def test_bounds_admit_the_fp32_backward(case, with_ext):
    (dqa, dqb, dhid), want = _emulated_backward(case, with_ext=with_ext)
    assert float(want["dqa"].abs().max()) < 6e4 and float(want["dqb"].abs().max()) < 6e4, "a gradient leaves fp16's range"
    ref.assert_within("emulated dqa", dqa, want["dqa"], want["dqa_bound"])
    ref.assert_within("emulated dqb", dqb, want["dqb"], want["dqb_bound"])
    ref.assert_within("emulated dhid", dhid, want["dhid"], want["dhid_bound"])


@pytest.mark.parametrize("case", ref.FWD_CASES, ids=ref.case_id)
def test_bounds_without_the_fp16_terms_admit_the_fp32_arithmetic(case):
    """What tests/test_gpu_attend_f64.py asks of the f32 kernels on every case: fp32 torch on make_inputs_f32 (hid = hi + lo
    rounded to fp32, fp32 outputs) stays inside the bounds with f16_out=False, forward and - up to T = 2048 - backward."""
    B, R, S, gain, ray0, nrays = case
    T = V * S
    x = ref.make_inputs_f32(case)
    hid32 = x["hs"][:, :HC].float() + x["hs"][:, HC:].float()
    hid = x["hs"][:, :HC].double() + x["hs"][:, HC:].double()
    l = ((x["qa"] * x["qb"]).sum(1) / F_SCALE).view(nrays, T)
    e = torch.exp(l - l.max(1, keepdim=True).values)
    w = e * (1.0 / e.sum(1, keepdim=True))
    hbar = (w.unsqueeze(-1) * hid32.view(nrays, T, HC)).sum(1)
    fwd = ref.attend_fwd_ref(x["qa"], x["qb"], None, hid, B, R, S, ray0, nrays)
    ref.assert_within("fp32 weights", w, fwd["w"], fwd["w_bound"])
    want, bound = ref.hbar_ref(w, hid, nrays, S, f16_out=False)
    ref.assert_within("fp32 hbar", hbar, want, bound)
    if case not in ref.BWD_CASES:
        return
    ext = ref.from_global(x["dw_ext"], B, R, S, ray0, nrays)
    dw = torch.bmm(hid32.view(nrays, T, HC), x["dhbar"].view(nrays, HC, 1)).squeeze(-1) + ext
    dl = (w * (dw - (w * dw).sum(1, keepdim=True)) / F_SCALE).unsqueeze(-1)
    dqa = (dl * x["qb"].view(nrays, T, 128)).view(-1, 128)
    dqb = (x["acc"].view(nrays, T, 128) + dl * x["qa"].view(nrays, T, 128)).view(-1, 128)
    want = ref.attend_bwd_ref(x["qa"], x["qb"], hid, w, x["dhbar"], ext, x["acc"], S, nrays, f16_out=False)
    ref.assert_within("fp32 dqa", dqa, want["dqa"], want["dqa_bound"])
    ref.assert_within("fp32 dqb", dqb, want["dqb"], want["dqb_bound"])


@pytest.mark.parametrize("case", ref.COMBINE_CASES + ref.GEMM_CASES, ids=ref.case_id)
def test_bounds_admit_the_fp32_combine(case):
    B, R, S, gain, ray0, nrays = case[:6]
    x = ref.make_combine_inputs(case)
    w1, w2 = (ref.from_global(x[k], B, R, S, ray0, nrays) for k in ("w1", "w2"))
    if len(case) > 6:                                  # the GEMM form: the product is rounded to fp16 first
        hid = x["hs"][:, :HC]
        dkey = (x["dkh"].float() @ x["Wt"].float().t()).half()
        want, bound, _ = ref.gemm_combine_ref(x["dkh"], x["Wt"], hid, w1, x["dh1"], w2, x["dh2"], S, nrays)
    else:
        hid, dkey = x["hid"], x["dkey"]
        want, bound, _ = ref.combine_ref(dkey, hid, w1, x["dh1"], w2, x["dh2"], S, nrays)
    got = emu_combine(dkey, hid, x["w1"], x["dh1"], x["w2"], x["dh2"], B, R, S, ray0, nrays)
    ref.assert_within("emulated combine", got, want, bound)
    if len(case) == 6:
        got = emu_combine(None, hid, x["w1"], x["dh1"], None, None, B, R, S, ray0, nrays)
        ref.assert_within("emulated combine, one part, no dkey", got, *ref.combine_ref(None, hid, w1, x["dh1"], None, None, S, nrays)[:2])


# ------------------------------------------------------------------------------------------------------------------
# 3. the bounds reject wrong kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,case,output", [
    ("last chunk dropped", ref.PLAIN, "dqa"),
    ("ray0 dropped", ref.WINDOW, "dqa"),
    ("dqb_acc twice", ref.PLAIN, "dqb"),
    ("dot over T - T % 4 rows", ref.SHORT, "dqa"),
])
def test_bounds_reject_a_seeded_defect(defect, case, output):
    """Each defect moves a gradient by a fraction of a percent or less of its scale: it must leave the bound on at least one
    element of its case - and the same emulation without it stays inside (test_bounds_admit_the_fp32_backward)."""
    (dqa, dqb, _), want = _emulated_backward(case, defect=defect)
    got = {"dqa": dqa, "dqb": dqb}[output]
    r = ref.ratio(got, want[output], want[output + "_bound"])
    print(f"{defect} on {ref.case_id(case)}: {int((~(r <= 1)).sum())} of {r.numel()} elements of {output} off, worst err/bound "
          f"{float(r.max()):.1f}")
    assert not bool((r <= 1).all())
    with pytest.raises(AssertionError, match="elements off"):
        ref.assert_within(defect, got, want[output], want[output + "_bound"])
