"""Float64 references, with element-wise error bounds, of the attention block's fp16 kernels - cpn_attend_hidden
(csrc/attend.hip), cpn_attend_hidden_bwd and cpn_hid_grad_combine (csrc/backward.hip), the combine epilogue of
cpn_gemm_f16_combine (csrc/gemm_f16.hip) - and of their fp32 siblings, for tests/test_attend_ref.py (CPU) and
tests/test_gpu_attend_f64.py (GPU).  Helpers, not tests.

Nothing here looks at a kernel's arithmetic: every reference takes the values a kernel READS (its fp16 / fp32 bits converted to
float64) and forms the mathematical result in float64.  The bounds are first order in the unit roundoffs u16 = 2^-11 (fp16)
and u32 = 2^-24 (fp32), each from the kernel's operation count; a `mag` is the same formula evaluated on absolute values.

Layouts.  T = V S rows per ray, V = 2.  qa / qb / dqa / dqb / dqb_acc are (nrays T, 128), hid (nrays T, 1664), hbar / dhbar
(nrays, 1664), all indexed by the LAUNCH-LOCAL ray; the softmax weights and what travels with them (at_wt, dw_ext, w1, w2) are
GLOBAL, (B V, R, S), entry (b V + v, r, s) of ray b R + r = ray0 + local ray, row = v S + s: weight_index() is the one place that
says so, for the references, the CPU emulation and the GPU tests alike.
"""
import torch

V = 2
HC = 1664
U32 = 2.0 ** -24                # unit roundoff of fp32, round to nearest
U16 = 2.0 ** -11                # unit roundoff of fp16
SUB16 = 2.0 ** -25              # half the spacing of the fp16 subnormals: the rounding error of a value below 2^-14
SCALE = float(torch.tensor(11.31, dtype=torch.float32))        # the kernels divide by the fp32 constant 11.31f

# (B, R, S, gain, ray0, nrays); one reason each
PLAIN = (2, 5, 32, 1, 0, 10)
WINDOW = (3, 3, 16, 1, 2, 6)            # the window starts inside b = 0 and ends inside b = 2
RAGGED = (2, 6, 30, 16, 4, 5)           # S % 4 != 0, T % 8 != 0, crosses the batch boundary, largest weight > 0.25
SHORT = (1, 4, 3, 1, 1, 2)              # T = 6 < 8: two waves own no row, the clamped second row in flight is the last one
PEAKED = (1, 3, 128, 32, 0, 3)          # largest weight of the call > 0.3
LIMIT_BWD = (1, 1, 1024, 1, 0, 1)       # T = 2048, the backward's limit: every `row += 256` loop takes 8 trips
LIMIT_FWD = (1, 1, 2048, 1, 0, 1)       # T = 4096, the forward's limit
FWD_CASES = [PLAIN, WINDOW, RAGGED, SHORT, PEAKED, LIMIT_BWD, LIMIT_FWD]
BWD_CASES = FWD_CASES[:-1]
COMBINE_CASES = [PLAIN, WINDOW, RAGGED]
# (B, R, S, gain, ray0, nrays, K): 192 and 480 rows (ragged 256-row tiles), T = 32 and 96 (the epilogue's "32 | T")
GEMM_CASES = [WINDOW + (128,), WINDOW + (64,), (1, 9, 48, 1, 2, 5, 128), (1, 9, 48, 1, 2, 5, 64)]
# the cases the CPU emulation is held inside the bounds on: every GPU case and the second shape of the existing f32 test
EMU_CASES = [PLAIN, (1, 7, 64, 8, 0, 7), WINDOW, RAGGED, PEAKED, SHORT, LIMIT_BWD, LIMIT_FWD]


def case_id(c):
    return "B%d-R%d-S%d-gain%d-ray%d+%d" % tuple(c[:6]) + ("-K%d" % c[6] if len(c) > 6 else "")


# ------------------------------------------------------------------------------------------------------------------
# the global weight layout
# ------------------------------------------------------------------------------------------------------------------
def weight_index(B, R, S, ray0, nrays):
    """(nrays, T) flat index into a (B V, R, S) tensor of row `row` = v S + s of local ray t: ray = ray0 + t = b R + r."""
    assert 0 <= ray0 and nrays > 0 and ray0 + nrays <= B * R
    ray = torch.arange(ray0, ray0 + nrays).view(-1, 1)
    row = torch.arange(V * S).view(1, -1)
    b, r = ray // R, ray % R
    v, s = row // S, row % S
    return ((b * V + v) * R + r) * S + s


def to_global(x, B, R, S, ray0, nrays, fill=float("nan")):
    """(nrays, T) values of the window -> (B V, R, S) with `fill` everywhere outside it."""
    out = torch.full((B * V * R * S,), fill, dtype=x.dtype)
    out[weight_index(B, R, S, ray0, nrays).reshape(-1)] = x.reshape(-1)
    return out.view(B * V, R, S)


def from_global(x, B, R, S, ray0, nrays):
    """(B V, R, S) -> the (nrays, T) values of the window."""
    return x.reshape(-1)[weight_index(B, R, S, ray0, nrays)]


def outside_window(B, R, S, ray0, nrays):
    """(B V, R, S) bool: the entries no ray of the window owns."""
    m = torch.ones(B * V * R * S, dtype=torch.bool)
    m[weight_index(B, R, S, ray0, nrays).reshape(-1)] = False
    return m.view(B * V, R, S)


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def attend_fwd_ref(qa, qb, logits, hid, B, R, S, ray0, nrays):
    """w = softmax_T(l), hbar = sum_T w hid with l = <qa, qb> / 11.31 (logits None) or logits / 11.31, in float64 and
    differentiable.  -> dict: l, w (nrays, T), hbar (nrays, 1664), idx (weight_index of the window), terms (the three
    relative terms of the weight bound, each (nrays, T)) and w_bound = w * sum(terms):

        |dw| <= w (2 max_row dl + (|l - l_max| + 4) 2^-22 + (T + 4) u32)

      * "logit": an absolute error dl on every logit of a row moves a softmax weight by at most 2 max dl relative (numerator
        and denominator).  qa.qb mode: dl = 130 u32 mag_l (128 exact products of fp16 values summed in fp32 in any order, the
        division); logits mode: dl = 2 u32 |l| (the division and its constant).
      * "expf": __expf(x) taken as exp2(x log2 e): one rounding of the product, |x| u32 relative, plus one ulp of the hardware
        exponential, times a margin of 4.  On the MI355X the error reaches 0.41 of this term alone (logits mode, the peaked
        case; tests/test_gpu_attend_f64.py prints the ratio per term).
      * "sum": T exponentials added in fp32, the reciprocal, the product with it.
    Holds while no exponential underflows fp32 (|l - l_max| < 87): the cases stay far inside."""
    T = V * S
    if logits is None:
        a, b = qa.double(), qb.double()
        l = (a * b).sum(1) / SCALE
        dl = 130 * U32 * (a.abs() * b.abs()).sum(1).detach() / SCALE
    else:
        l = logits.double() / SCALE
        dl = 2 * U32 * l.abs().detach()
    l, dl = l.view(nrays, T), dl.view(nrays, T)
    w = torch.softmax(l, 1)
    hbar = (w.unsqueeze(-1) * hid.double().view(nrays, T, HC)).sum(1)
    with torch.no_grad():
        x = (l - l.max(1, keepdim=True).values).abs()
        assert float(x.max()) < 87.0, "an exponential underflows fp32: the weight bound does not cover this input"
        terms = {"logit": (2 * dl.max(1, keepdim=True).values).expand(nrays, T), "expf": (x + 4) * 2.0 ** -22,
                 "sum": torch.full((nrays, T), (T + 4) * U32, dtype=torch.float64, device=l.device)}
        w_bound = w * sum(terms.values())
    return {"l": l, "w": w, "hbar": hbar, "idx": weight_index(B, R, S, ray0, nrays), "terms": terms, "w_bound": w_bound}


def hbar_ref(w_used, hid, nrays, S, f16_out=True):
    """(want, bound) of hbar = sum_T w hid formed from the weights the kernel RETURNED (they are what its sum used, and they are
    checked on their own): |d| <= u16 |want| + (T + 2) u32 mag + 2^-25.  A term passes at most T additions and 2 roundings of
    its own (channels 6 and 7 of hid_sum.h add a rounded product; the f32 kernel rounds hi + lo and the product), the result is
    rounded to fp16 once (f16_out; 2^-25 where it lands among the subnormals)."""
    T = V * S
    h = hid.double().view(nrays, T, HC)
    w = w_used.double().view(nrays, T, 1)
    want = (w * h).sum(1)
    mag = (w.abs() * h.abs()).sum(1)
    bound = (T + 2) * U32 * mag
    if f16_out:
        bound = bound + U16 * want.abs() + SUB16
    return want, bound


def attend_bwd_ref(qa, qb, hid, w, dhbar, dw_ext, dqb_acc, S, nrays, want_dhid=False, f16_out=True):
    """The adjoint of attend_fwd_ref with the weights as an INPUT (w (nrays, T): what the forward kernel stored), float64:
        dw = <hid, dhbar> + dw_ext,  dl = w (dw - sum_T w dw) / 11.31,  dqa = dl qb,  dqb = dqb_acc + dl qa,  dhid = w dhbar
    dw_ext (nrays, T) and dqb_acc (nrays T, 128) may be None.  -> dict of dqa, dqb, dhid (if asked) and their bounds:
        ddl    = (w / 11.31) ((1664 + 8) u32 mag_dw + (1664 + T + 8) u32 mag_dot + 4 u32 (|dw| + |dot|))
        |ddqa| <= u16 |want| + ddl |qb| + 2 u32 |want| + 2^-25
        |ddqb| <= u16 |want| + ddl |qa| + 2 u32 (|dqb_acc| + |dl qa|) + 2^-25
        |ddhid| <= u16 |want| + 2 u32 |want| + 2^-25
    (a row's dot product is 1664 products added in fp32 in some order, then dw_ext; `dot` adds T products of those; the
    difference, the product with w and the division are the 4 u32; a product dl qb and the sum with dqb_acc are rounded in fp32
    and once to fp16).  f16_out False (the f32 kernel, hid = hi + lo): without the u16 and 2^-25 terms."""
    T = V * S
    a, b = qa.double().view(nrays, T, 128), qb.double().view(nrays, T, 128)
    h = hid.double().view(nrays, T, HC)
    w = w.double().view(nrays, T)
    g = dhbar.double().view(nrays, HC, 1)
    dw = torch.bmm(h, g).squeeze(-1)
    mag_dw = torch.bmm(h.abs(), g.abs()).squeeze(-1)
    if dw_ext is not None:
        dw = dw + dw_ext.double().view(nrays, T)
        mag_dw = mag_dw + dw_ext.double().abs().view(nrays, T)
    dot = (w * dw).sum(1, keepdim=True)
    mag_dot = (w.abs() * mag_dw).sum(1, keepdim=True)
    dl = w * (dw - dot) / SCALE
    ddl = (w.abs() / SCALE) * ((HC + 8) * U32 * mag_dw + (HC + T + 8) * U32 * mag_dot + 4 * U32 * (dw.abs() + dot.abs()))
    dl3, ddl3 = dl.unsqueeze(-1), ddl.unsqueeze(-1)
    out16 = (lambda want: U16 * want.abs() + SUB16) if f16_out else (lambda want: 0.0)
    dqa = dl3 * b
    prod = dl3 * a
    acc = dqb_acc.double().view(nrays, T, 128) if dqb_acc is not None else torch.zeros_like(prod)
    dqb = acc + prod
    res = {"dl": dl, "dqa": dqa.view(nrays * T, 128), "dqb": dqb.view(nrays * T, 128),
           "dqa_bound": (out16(dqa) + ddl3 * b.abs() + 2 * U32 * dqa.abs()).view(nrays * T, 128),
           "dqb_bound": (out16(dqb) + ddl3 * a.abs() + 2 * U32 * (acc.abs() + prod.abs())).view(nrays * T, 128)}
    if want_dhid:
        dhid = w.unsqueeze(-1) * g.view(nrays, 1, HC)
        res["dhid"] = dhid.view(nrays * T, HC)
        res["dhid_bound"] = (out16(dhid) + 2 * U32 * dhid.abs()).view(nrays * T, HC)
    return res


def combine_ref(dkey, hid, w1, dh1, w2, dh2, S, nrays, dkey_mag=None, K=0):
    """out = hid > 0 ? dkey + w1 dh1 + w2 dh2 : 0 in float64 -> (want, bound, live), each (nrays T, 1664) - the same memory as
    the (nrays T 2, 832) rows of cpn_hid_grad_combine, row = ((t V + v) S + s) 2 + j, part_i[row, c] = w_i[t, v S + s]
    dh_i[t, 832 j + c].  dkey, (w1, dh1), (w2, dh2) may each be None; w_i (nrays, T), dh_i (nrays, 1664).
        |d| <= u16 |want| + 4 u32 mag + 2^-25          (two products, two additions in fp32; one rounding to fp16)
    and elements with hid <= 0 (`live` False; -0.0 among them) must be EXACTLY 0: their bound is 0.
    The GEMM form (dkey = dkh Wt^T formed by the caller in float64, dkey_mag the same on absolute values, K its length) rounds
    the product to fp16 before the parts are added: the bound gains u16 |dkey| + (K + 4) u32 dkey_mag."""
    T = V * S
    h = hid.double().reshape(nrays, T, HC)
    want = torch.zeros_like(h)
    mag = torch.zeros_like(h)
    if dkey is not None:
        want = want + dkey.double().reshape(nrays, T, HC)
        mag = mag + dkey.double().abs().reshape(nrays, T, HC)
    for w, dh in ((w1, dh1), (w2, dh2)):
        if w is not None:
            part = w.double().view(nrays, T, 1) * dh.double().view(nrays, 1, HC)
            want = want + part
            mag = mag + part.abs()
    bound = U16 * want.abs() + 4 * U32 * mag + SUB16
    if dkey_mag is not None:
        bound = bound + U16 * dkey.double().abs().reshape(nrays, T, HC) + (K + 4) * U32 * dkey_mag.reshape(nrays, T, HC)
    live = h > 0
    zero = torch.zeros_like(want)
    return (torch.where(live, want, zero).view(nrays * T, HC), torch.where(live, bound, zero).view(nrays * T, HC),
            live.view(nrays * T, HC))


def gemm_combine_ref(dkh, Wt, hid, w1, dh1, w2, dh2, S, nrays):
    """combine_ref with dkey = dkh Wt^T (dkh (nrays T, K), Wt (1664, K)) in float64."""
    a, b = dkh.double(), Wt.double()
    return combine_ref(a @ b.t(), hid, w1, dh1, w2, dh2, S, nrays, dkey_mag=a.abs() @ b.abs().t(), K=dkh.shape[1])


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def ratio(got, want, bound):
    """err / bound per element; 0 where both are 0; inf where the error is not finite (a NaN must never pass)."""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return torch.where(torch.isfinite(err), r, torch.full_like(r, float("inf")))


def assert_within(what, got, want, bound):
    """Every element of `got` within `bound` of `want`; prints and returns max err/bound."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    r = ratio(got, want, bound)
    worst = float(r.max())
    print(f"{what}: max err/bound = {worst:.3f}  (max|want| = {float(want.abs().max()):.3e})")
    bad = (~(r <= 1)).nonzero()
    if bad.numel():
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {r.numel()} elements off, first {list(i)}: got {float(got[i])!r} want "
                             f"{float(want[i])!r}, err/bound {float(r[i]):.3f} (worst {worst:.3f})")
    return worst


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def plant_hid(hid16, gen):
    """A few -0.0 and positive fp16 subnormals at random places of an fp16 tensor (in place)."""
    flat = hid16.view(-1)
    k = max(1, min(64, flat.numel() // 16))
    where = torch.randperm(flat.numel(), generator=gen)[:2 * k]
    flat[where[:k]] = -0.0
    flat[where[k:]] = torch.randint(1, 1024, (k,), generator=gen).to(torch.int16).view(torch.float16)
    return hid16


def make_hid(rows, cols, gen):
    return plant_hid((2.0 * torch.relu(torch.randn(rows, cols, generator=gen))).half(), gen)


def make_hs(rows, gen):
    """(rows, 3328) = [hi | lo] fp16 pairs of 2 relu(randn), as test_gpu_train_f32._hs builds them."""
    x = torch.relu(torch.randn(rows, HC, generator=gen)) * 2.0
    hi = x.half()
    return torch.cat((hi, (x - hi.float()).half()), 1).contiguous()


def global_randn(B, R, S, ray0, nrays, gen, uniform=False):
    """(B V, R, S) fp32 random values with NaN on every entry outside the ray window."""
    x = torch.rand(B * V, R, S, generator=gen) if uniform else torch.randn(B * V, R, S, generator=gen)
    x[outside_window(B, R, S, ray0, nrays)] = float("nan")
    return x


def make_inputs(case):
    """Everything the attention kernels read for a case, on the CPU: fp16 qa / qb / hid / dqb_acc, fp32 dhbar (two of them,
    for the two-round chain), the poisoned global dw_ext and the fp32 logits of the `logits` mode (the float64 row dots,
    rounded)."""
    B, R, S, gain, ray0, nrays = case[:6]
    T = V * S
    # (the ragged case's draw is the first of its seeds whose largest weight passes the 0.25 its reason names: asserted by users)
    gen = torch.Generator().manual_seed(100000 * B + 1000 * R + 10 * S + ray0 + int(gain) + (7919 if case == RAGGED else 0))
    rows = nrays * T
    qa = (0.3 * gain * torch.randn(rows, 128, generator=gen)).half()
    qb = (0.3 * torch.randn(rows, 128, generator=gen)).half()
    return {"qa": qa, "qb": qb, "hid": make_hid(rows, HC, gen),
            "dhbar": torch.randn(nrays, HC, generator=gen), "dhbar2": torch.randn(nrays, HC, generator=gen),
            "dw_ext": global_randn(B, R, S, ray0, nrays, gen), "acc": torch.randn(rows, 128, generator=gen).half(),
            "logits": (qa.double() * qb.double()).sum(1).float()}


def make_inputs_f32(case):
    """The same for the f32 kernels: fp32 qa / qb / dqb_acc and hs = [hi | lo]."""
    B, R, S, gain, ray0, nrays = case[:6]
    gen = torch.Generator().manual_seed(200000 * B + 1000 * R + 10 * S + ray0 + int(gain))
    rows = nrays * V * S
    return {"qa": 0.3 * gain * torch.randn(rows, 128, generator=gen), "qb": 0.3 * torch.randn(rows, 128, generator=gen),
            "hs": make_hs(rows, gen), "dhbar": torch.randn(nrays, HC, generator=gen),
            "dw_ext": global_randn(B, R, S, ray0, nrays, gen), "acc": torch.randn(rows, 128, generator=gen)}


def make_combine_inputs(case):
    """dkey / hid as (nrays T, 1664) fp16, the poisoned global w1 / w2 in [0, 1), fp32 dh1 / dh2; for a GEMM case also dkh,
    Wt and hs (its hi half is the mask)."""
    B, R, S, gain, ray0, nrays = case[:6]
    gen = torch.Generator().manual_seed(300000 * B + 1000 * R + 10 * S + ray0 + (case[6] if len(case) > 6 else 0))
    rows = nrays * V * S
    d = {"dkey": torch.randn(rows, HC, generator=gen).half(), "hid": make_hid(rows, HC, gen),
         "w1": global_randn(B, R, S, ray0, nrays, gen, uniform=True), "w2": global_randn(B, R, S, ray0, nrays, gen, uniform=True),
         "dh1": torch.randn(nrays, HC, generator=gen), "dh2": torch.randn(nrays, HC, generator=gen)}
    if len(case) > 6:
        K = case[6]
        d["dkh"] = (torch.randn(rows, K, generator=gen) * 0.5).half()
        d["Wt"] = (torch.randn(HC, K, generator=gen) * 0.1).half()
        d["hs"] = make_hs(rows, gen)
        d["hs"][:, :HC] = plant_hid(d["hs"][:, :HC].contiguous(), gen)
    return d
