"""The four kernels every sample of the default training path goes through - cpn_attend_hidden, cpn_attend_hidden_bwd,
cpn_hid_grad_combine, cpn_gemm_f16_combine(_hs) - and their fp32 siblings on the same cases, each against its float64
reference with an element-wise bound (tests/attend_ref.py; pinned and calibrated on the CPU by tests/test_attend_ref.py).
No element is left out of any comparison; every global tensor holds NaN outside the ray window, every output starts as NaN
and has 64 guard rows behind it.

max err/bound of the first run on an MI355X, the worst over the cases of each kernel:
  cpn_attend_hidden            at_wt 0.009 (qa.qb mode), 0.095 (logits mode; the __expf term alone: 0.41); hbar 0.990
  cpn_attend_hidden_bwd        dqa 0.997, dqb 0.994, dhid 0.999 (all four ways; the fp16 rounding term dominates)
  cpn_attend_hidden_f32        at_wt 0.018, hbar 0.241        cpn_attend_hidden_bwd_f32   dqa 0.015, dqb 0.473
                               (every forward / backward case since round 14; on WINDOW and RAGGED alone 0.136 and 0.323)
  cpn_hid_grad_combine         0.999 (both parts, one part, no dkey)
  cpn_gemm_f16_combine(_hs)    0.974 (K = 64), 0.943 (K = 128); the two entries give the same figures
Where a ratio sits just under 1 the fp16 rounding of the output (half an ulp against u16 |want|) is what fills the bound; the
CPU emulation of tests/test_attend_ref.py shows the same figures to three digits.
"""
import functools

import pytest
import torch

from tests import attend_ref as ref

pytestmark = pytest.mark.gpu

V, HC = ref.V, ref.HC
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


def _take(buf, rows, what):
    """The output rows on the host, after the guard rows were seen intact and every output element finite."""
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[rows:] == 7.0).all()), f"{what}: wrote behind the output"
    assert bool(torch.isfinite(out[:rows].float()).all()), f"{what}: elements left unwritten or not finite"
    return out[:rows]


def _take_global(buf, B, R, S, ray0, nrays, what):
    """The (nrays, T) window of a (B V R + GUARD, S) weight buffer that started as NaN: every entry outside the window still
    holds the bits of the sentinel, the guard rows their constant."""
    torch.cuda.synchronize()
    out = buf.cpu()
    n = B * V * R
    assert bool((out[n:] == 7.0).all()), f"{what}: wrote behind the output"
    outside = ref.outside_window(B, R, S, ray0, nrays)
    sentinel = torch.tensor(NAN).view(torch.int32)
    assert bool((out[:n].view(B * V, R, S).view(torch.int32)[outside] == sentinel).all()), f"{what}: wrote outside the ray window"
    w = ref.from_global(out[:n], B, R, S, ray0, nrays)
    assert bool(torch.isfinite(w).all()), f"{what}: weights left unwritten or not finite"
    return w


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return ref.make_inputs(case)


@functools.lru_cache(maxsize=None)
def _fwd_ref(case, mode):
    x = _inputs(case)
    B, R, S, gain, ray0, nrays = case
    return ref.attend_fwd_ref(x["qa"], x["qb"], x["logits"] if mode == "logits" else None, x["hid"], B, R, S, ray0, nrays)


# ------------------------------------------------------------------------------------------------------------------
# (a) cpn_attend_hidden
# ------------------------------------------------------------------------------------------------------------------
def _run_forward(case, mode, dev, with_weights=True):
    """One launch -> (hbar on the host, the weight buffer on the device or None)."""
    from coponerf_amd._hip import call
    B, R, S, gain, ray0, nrays = case
    x = _inputs(case)
    qa, qb, hid = x["qa"].to(dev), x["qb"].to(dev), x["hid"].to(dev)
    lg = x["logits"].to(dev) if mode == "logits" else None
    hbar = _out(nrays, HC, torch.float16, dev)
    wbuf = _out(B * V * R, S, torch.float32, dev) if with_weights else None
    if mode == "logits":
        qa = qb = None                                                   # the mode must not need them
    call("cpn_attend_hidden", _ptr(qa), _ptr(qb), _ptr(lg), hid.data_ptr(), B, V, R, S, ray0, nrays, hbar.data_ptr(), _ptr(wbuf), _st())
    return _take(hbar, nrays, f"hbar {mode}"), wbuf


@functools.lru_cache(maxsize=None)
def _checked_forward(case, mode, dev):
    """The forward kernel's weights, ASSERTED against the reference: (weight buffer on the device, its (nrays, T) window on
    the host, hbar on the host).  The backward tests take their at_wt from here."""
    B, R, S, gain, ray0, nrays = case
    hbar, wbuf = _run_forward(case, mode, dev)
    w = _take_global(wbuf, B, R, S, ray0, nrays, f"at_wt {mode}")
    fwd = _fwd_ref(case, mode)
    if case == ref.PEAKED:
        assert float(fwd["w"].max()) > 0.3
    if case == ref.RAGGED:
        assert float(fwd["w"].max()) > 0.25
    for name, t in fwd["terms"].items():                                  # which term of the bound the error uses
        print(f"    at_wt {mode} {ref.case_id(case)}: err / (w * {name} term) = {float(ref.ratio(w, fwd['w'], fwd['w'] * t).max()):.3f}")
    ref.assert_within(f"at_wt {mode} {ref.case_id(case)}", w, fwd["w"], fwd["w_bound"])
    return wbuf, w, hbar


@pytest.mark.parametrize("mode", ["qa.qb", "logits"])
@pytest.mark.parametrize("case", ref.FWD_CASES, ids=ref.case_id)
def test_attend_hidden_against_float64(case, mode, dev):
    """Weights against softmax in float64 (bound: attend_fwd_ref), hbar against the float64 sum under the weights the kernel
    returned (bound: hbar_ref), the window of at_wt and nothing else written, hbar the same bits without at_wt."""
    B, R, S, gain, ray0, nrays = case
    _, w, hbar = _checked_forward(case, mode, dev)
    want, bound = ref.hbar_ref(w, _inputs(case)["hid"], nrays, S)
    ref.assert_within(f"hbar {mode} {ref.case_id(case)}", hbar, want, bound)
    hbar_alone, _ = _run_forward(case, mode, dev, with_weights=False)
    assert torch.equal(hbar_alone.view(torch.int16), hbar.view(torch.int16)), "hbar differs when at_wt is not asked for"


# ------------------------------------------------------------------------------------------------------------------
# (b) cpn_attend_hidden_bwd
# ------------------------------------------------------------------------------------------------------------------
def _run_backward(case, dev, wbuf, dhbar, dw_ext, acc, want_dhid, what):
    from coponerf_amd._hip import call
    B, R, S, gain, ray0, nrays = case
    x = _inputs(case)
    rows = nrays * V * S
    qa, qb, hid = x["qa"].to(dev), x["qb"].to(dev), x["hid"].to(dev)
    dh = dhbar.to(dev)
    ext = dw_ext.to(dev) if dw_ext is not None else None
    accd = acc.to(dev) if acc is not None else None
    dqa, dqb = _out(rows, 128, torch.float16, dev), _out(rows, 128, torch.float16, dev)
    dhid = _out(rows, HC, torch.float16, dev) if want_dhid else None
    call("cpn_attend_hidden_bwd", qa.data_ptr(), qb.data_ptr(), hid.data_ptr(), wbuf.data_ptr(), dh.data_ptr(), _ptr(ext),
         B, V, R, S, ray0, nrays, dqa.data_ptr(), dqb.data_ptr(), _ptr(dhid), _ptr(accd), _st())
    return (_take(dqa, rows, what + " dqa"), _take(dqb, rows, what + " dqb"),
            _take(dhid, rows, what + " dhid") if want_dhid else None)


def _check_backward(case, got, w, dhbar, dw_ext, acc, what):
    B, R, S, gain, ray0, nrays = case
    x = _inputs(case)
    ext = ref.from_global(dw_ext, B, R, S, ray0, nrays) if dw_ext is not None else None
    want = ref.attend_bwd_ref(x["qa"], x["qb"], x["hid"], w, dhbar, ext, acc, S, nrays, want_dhid=got[2] is not None)
    assert float(want["dqa"].abs().max()) < 6e4 and float(want["dqb"].abs().max()) < 6e4
    ref.assert_within(f"{what} dqa", got[0], want["dqa"], want["dqa_bound"])
    ref.assert_within(f"{what} dqb", got[1], want["dqb"], want["dqb_bound"])
    if got[2] is not None:
        ref.assert_within(f"{what} dhid", got[2], want["dhid"], want["dhid_bound"])


@pytest.mark.parametrize("variant", ["ext+acc", "plain", "dhid", "chain"])
@pytest.mark.parametrize("case", ref.BWD_CASES, ids=ref.case_id)
def test_attend_hidden_bwd_against_float64(case, variant, dev):
    """dqa, dqb (and dhid) against the float64 adjoint under the forward kernel's own weights (bounds: attend_bwd_ref):
    with dw_ext and dqb_acc; with neither; with dhid asked for; and as the product chains its two rounds - dqb_acc of the
    second call is the fp16 dqb the first one wrote, and the second dqb is checked against dqb_1 (as read) + dl_2 qa."""
    x = _inputs(case)
    wbuf, w, _ = _checked_forward(case, "qa.qb", dev)
    what = f"bwd {variant} {ref.case_id(case)}"
    if variant == "chain":
        first = _run_backward(case, dev, wbuf, x["dhbar"], x["dw_ext"], None, False, what + " call 1")
        _check_backward(case, first, w, x["dhbar"], x["dw_ext"], None, what + " call 1")
        second = _run_backward(case, dev, wbuf, x["dhbar2"], None, first[1], False, what + " call 2")
        _check_backward(case, second, w, x["dhbar2"], None, first[1], what + " call 2")
        return
    ext, acc = (x["dw_ext"], x["acc"]) if variant != "plain" else (None, None)
    got = _run_backward(case, dev, wbuf, x["dhbar"], ext, acc, variant == "dhid", what)
    _check_backward(case, got, w, x["dhbar"], ext, acc, what)


# ------------------------------------------------------------------------------------------------------------------
# (c) the fp32 siblings under a ray window
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.FWD_CASES, ids=ref.case_id)
def test_f32_attention_kernels_under_a_ray_window(case, dev):
    """cpn_attend_hidden_f32 on every forward case and cpn_attend_hidden_bwd_f32 on every backward case - the f32 kernels are
    the fp16 kernels' body under another trait, so they run at the edges of the same control flow (T = 6 < 8, a peaked ray, the
    limits T = 2048 and, forward only, 4096) - against the derived bounds: the references of the fp16 kernels with
    hid = hi + lo and without the fp16 rounding terms.  With ray0 != 0 (test_attend_hidden_bwd_f32_against_float64_autograd
    runs whole batches only), on WINDOW and RAGGED, per element the tighter of the bound and that test's 1e-5 max|want|."""
    from coponerf_amd._hip import call
    B, R, S, gain, ray0, nrays = case
    rows = nrays * V * S
    x = ref.make_inputs_f32(case)
    hid = x["hs"][:, :HC].double() + x["hs"][:, HC:].double()
    qa, qb, hs, dhbar, ext, acc = (x[k].to(dev) for k in ("qa", "qb", "hs", "dhbar", "dw_ext", "acc"))
    hbar = _out(nrays, HC, torch.float32, dev)
    wbuf = _out(B * V * R, S, torch.float32, dev)
    call("cpn_attend_hidden_f32", qa.data_ptr(), qb.data_ptr(), hs.data_ptr(), B, V, R, S, ray0, nrays, hbar.data_ptr(), wbuf.data_ptr(), _st())
    w = _take_global(wbuf, B, R, S, ray0, nrays, "f32 at_wt")
    if case in (ref.WINDOW, ref.RAGGED):
        tighter = lambda bound, want: torch.minimum(bound, 1e-5 * want.abs().max().expand_as(bound))
    else:
        tighter = lambda bound, want: bound
    what = "f32 " + ref.case_id(case)
    fwd = ref.attend_fwd_ref(x["qa"], x["qb"], None, hid, B, R, S, ray0, nrays)
    if case == ref.PEAKED:
        assert float(fwd["w"].max()) > 0.3
    ref.assert_within(what + " at_wt", w, fwd["w"], tighter(fwd["w_bound"], fwd["w"]))
    want, bound = ref.hbar_ref(w, hid, nrays, S, f16_out=False)
    ref.assert_within(what + " hbar", _take(hbar, nrays, "f32 hbar"), want, tighter(bound, want))
    if case not in ref.BWD_CASES:
        return
    for with_ext in (True, False):
        dqa, dqb = _out(rows, 128, torch.float32, dev), _out(rows, 128, torch.float32, dev)
        call("cpn_attend_hidden_bwd_f32", qa.data_ptr(), qb.data_ptr(), hs.data_ptr(), wbuf.data_ptr(), dhbar.data_ptr(),
             ext.data_ptr() if with_ext else 0, B, V, R, S, ray0, nrays, dqa.data_ptr(), dqb.data_ptr(),
             acc.data_ptr() if with_ext else 0, _st())
        want = ref.attend_bwd_ref(x["qa"], x["qb"], hid, w, x["dhbar"], ref.from_global(x["dw_ext"], B, R, S, ray0, nrays) if with_ext else None,
                                  x["acc"] if with_ext else None, S, nrays, f16_out=False)
        tag = what + (" ext+acc" if with_ext else " plain")
        ref.assert_within(tag + " dqa", _take(dqa, rows, tag + " dqa"), want["dqa"], tighter(want["dqa_bound"], want["dqa"]))
        ref.assert_within(tag + " dqb", _take(dqb, rows, tag + " dqb"), want["dqb"], tighter(want["dqb_bound"], want["dqb"]))


# ------------------------------------------------------------------------------------------------------------------
# (d) cpn_hid_grad_combine
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["both parts", "one part", "no dkey"])
@pytest.mark.parametrize("case", ref.COMBINE_CASES, ids=ref.case_id)
def test_hid_grad_combine_against_float64(case, variant, dev):
    """Every row and channel against combine_ref; hid <= 0 (-0.0 and what surrounds the planted subnormals included) gives
    exactly 0; w1 / w2 hold NaN outside the window."""
    from coponerf_amd._hip import call
    B, R, S, gain, ray0, nrays = case
    x = ref.make_combine_inputs(case)
    rows2 = nrays * V * S * 2
    dkey = None if variant == "no dkey" else x["dkey"]
    second = variant != "one part"
    d = {k: x[k].to(dev) for k in ("hid", "w1", "dh1", "w2", "dh2")}
    dk = dkey.to(dev) if dkey is not None else None
    out = _out(rows2, 832, torch.float16, dev)
    call("cpn_hid_grad_combine", _ptr(dk), d["hid"].data_ptr(), d["w1"].data_ptr(), d["dh1"].data_ptr(),
         d["w2"].data_ptr() if second else 0, d["dh2"].data_ptr() if second else 0, B, V, R, S, ray0, nrays, out.data_ptr(), _st())
    w1, w2 = (ref.from_global(x[k], B, R, S, ray0, nrays) for k in ("w1", "w2"))
    want, bound, live = ref.combine_ref(dkey, x["hid"], w1, x["dh1"], w2 if second else None, x["dh2"] if second else None, S, nrays)
    what = f"combine {variant} {ref.case_id(case)}"
    got = _take(out, rows2, what).view(-1, HC)
    assert bool((x["hid"].view(torch.int16) == -32768).any()) and bool(((x["hid"] > 0) & (x["hid"] < 2.0 ** -14)).any())
    assert bool((got[~live] == 0).all()), "an element with hid <= 0 is not exactly 0"
    ref.assert_within(what, got, want, bound)


# ------------------------------------------------------------------------------------------------------------------
# (e) cpn_gemm_f16_combine, cpn_gemm_f16_combine_hs
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["cpn_gemm_f16_combine", "cpn_gemm_f16_combine_hs"])
@pytest.mark.parametrize("case", ref.GEMM_CASES, ids=ref.case_id)
def test_gemm_combine_against_float64(case, entry, dev):
    """Every row and channel of the fused form against dkh Wt^T + parts in float64 (test_combine_gemm_equals_gemm_then_combine
    samples 64 rows at a global 2e-2): 192 and 480 rows, K = 128 and 64; the _hs entry reads its mask from the hi half of hs."""
    from coponerf_amd._hip import call
    B, R, S, gain, ray0, nrays, K = case
    x = ref.make_combine_inputs(case)
    rows = nrays * V * S
    hi = x["hs"][:, :HC].contiguous()
    mask = (x["hs"] if entry.endswith("_hs") else hi).to(dev)
    d = {k: x[k].to(dev) for k in ("dkh", "Wt", "w1", "dh1", "w2", "dh2")}
    out = _out(rows, HC, torch.float16, dev)
    call(entry, d["dkh"].data_ptr(), K, d["Wt"].data_ptr(), K, mask.data_ptr(), d["w1"].data_ptr(), d["dh1"].data_ptr(),
         d["w2"].data_ptr(), d["dh2"].data_ptr(), B, V, R, S, ray0, nrays, K, out.data_ptr(), _st())
    w1, w2 = (ref.from_global(x[k], B, R, S, ray0, nrays) for k in ("w1", "w2"))
    want, bound, live = ref.gemm_combine_ref(x["dkh"], x["Wt"], hi, w1, x["dh1"], w2, x["dh2"], S, nrays)
    what = f"{entry} {ref.case_id(case)}"
    got = _take(out, rows, what)
    assert bool((got[~live] == 0).all()), "an element with hid <= 0 is not exactly 0"
    ref.assert_within(what, got, want, bound)


# ------------------------------------------------------------------------------------------------------------------
# (f) argument checks: only what an entry rejects before any launch
# ------------------------------------------------------------------------------------------------------------------
def test_attention_entry_points_reject_bad_arguments(dev):
    from coponerf_amd._hip import call
    st = _st()
    h = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    f = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    hp, fp = h.data_ptr(), f.data_ptr()

    def fwd(ray0=0, nrays=1):
        call("cpn_attend_hidden", hp, hp, 0, hp, 1, 2, 1, 4, ray0, nrays, hp, fp, st)

    def bwd(dhbar=fp, S=4, ray0=0, nrays=1):
        call("cpn_attend_hidden_bwd", hp, hp, hp, fp, dhbar, 0, 1, 2, 1, S, ray0, nrays, hp, hp, 0, 0, st)

    def bwd_f32(ray0=0, nrays=1):
        call("cpn_attend_hidden_bwd_f32", fp, fp, hp, fp, fp, 0, 1, 2, 1, 4, ray0, nrays, fp, fp, 0, st)

    def combine(ray0=0, nrays=1):
        call("cpn_hid_grad_combine", hp, hp, fp, fp, 0, 0, 1, 2, 1, 4, ray0, nrays, hp, st)

    def gemm(entry, S=16, ray0=0, nrays=1):
        call(entry, hp, 128, hp, 128, hp, fp, fp, 0, 0, 1, 2, 1, S, ray0, nrays, 128, hp, st)

    bad = [
        ("cpn_attend_hidden_bwd", "null pointer", lambda: bwd(dhbar=0)),
        ("cpn_attend_hidden_bwd", "bad shape", lambda: bwd(S=1025)),                        # V S = 2050
        ("cpn_attend_hidden_bwd", "ray range", lambda: bwd(ray0=1, nrays=1)),
        ("cpn_attend_hidden_bwd_f32", "ray range", lambda: bwd_f32(ray0=0, nrays=2)),
        ("cpn_attend_hidden", "ray range", lambda: fwd(ray0=1, nrays=1)),
        ("cpn_hid_grad_combine", "ray range", lambda: combine(ray0=0, nrays=2)),
        ("cpn_gemm_f16_combine", "ray range", lambda: gemm("cpn_gemm_f16_combine", ray0=1)),
        ("cpn_gemm_f16_combine", "S % 16", lambda: gemm("cpn_gemm_f16_combine", S=24)),
        ("cpn_gemm_f16_combine_hs", "S % 16", lambda: gemm("cpn_gemm_f16_combine_hs", S=24)),
    ]
    for name, why, fn in bad:
        with pytest.raises(RuntimeError, match=name + ": .*" + why):
            fn()
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((h == 0).all()), "a rejected call wrote something"
