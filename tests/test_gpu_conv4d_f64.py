"""The 4-D convolution of get_z and the depthwise convolution of its feed-forward blocks - cpn_conv4d on every arm of its
dispatch with the GroupNorm statistics it publishes, cpn_conv4d_gn_relu, cpn_conv4d_strided_bwd, cpn_conv_wgrad_planes,
cpn_dwconv3x3_wgrad, cpn_dwconv3x3_tokens, cpn_dwconv3x3_tokens_wgrad - each called on its raw entry and held, element by
element, to its float64 reference and derived bound (tests/conv4d_ref.py; pinned, calibrated and shown to see seeded defects on
the CPU by tests/test_conv4d_ref.py).  No element is left out of any comparison; every output and every scratch buffer starts
as NaN and has GUARD elements behind it, which must come back intact; `stats` is zero on entry as the header requires; every
result must be finite; two runs of every entry give the same bits.  A forward case names the arm it must reach: the number of
partial pairs the launch published must be that arm's workgroups per sample.

max err/bound of the first run on an MI355X, the worst over the cases of each entry, with the terms that make up the bound at
that element (one term, the chain, unless named).  The bounds are not tuned to these figures; in brackets the fp32 CPU
evaluation of tests/test_conv4d_ref.py wherever either figure is above 0.1.
  cpn_conv4d y, by arm          generic 0.075   pooled 0.026   pooled c8 0.166 [0.086]   VALU <4,true> 0.069   <8,true> 0.029
                                <8,false> 0.264 [0.166]: 18 products, 160 000 x 8 elements   MFMA one tile 0.055, two tiles 0.033
                                misaligned x or y (off the MFMA arm, VALU <4,true>) 0.038
  cpn_conv4d stats              0.003 at most, of gam64(C npos) on sum |y| and sum y^2; bit-equal to the replay on every case
  cpn_conv4d_gn_relu            out 0.525 plain, 0.845 with a residual (VALU <4,true>; MFMA 0.423 / 0.804, residual 86 % of the
                                bound there: the one rounding of the last addition, nearly attained somewhere in the volume),
                                bit-equal to the two calls
  cpn_conv4d_strided_bwd        dx 0.032, gwq 0.020, gws 0.014, gb 0.006; the routed set exact, ties included
  cpn_conv_wgrad_planes         dw 0.275 [0.275] (one plane of four positions: a single product's rounding), db 0.001
  cpn_dwconv3x3_wgrad           dw 0.358 [0.358] (one position), db 0.006
  cpn_dwconv3x3_tokens          flip 0 0.273 [0.341], flip 1 0.280 [0.353], flip 2 0.239 [0.794] (erf 79 %, ops 13 %, conv 8 %:
                                the device's erff uses a quarter of the 4 ulp the bound ASSUMES)
  cpn_dwconv3x3_tokens_wgrad    dw 0.688 [0.688] (one position), db 0.024
The long chains sit far inside: their bounds charge every addition at full u, and fp32 sums of random signs lose about its
square root.  Nothing left a bound on that run and no kernel was changed.
"""
import functools

import pytest
import torch

from tests import conv4d_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")
F32 = torch.float32
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from coponerf_amd._hip import call
    call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _st())


def _lib():
    from coponerf_amd import _hip
    return _hip.lib()


def _out(n, dev, dtype=F32, fill=NAN):
    """A flat buffer of n elements pre-filled with NaN (`stats`: zero), with GUARD elements of 7 behind it."""
    buf = torch.full((int(n) + GUARD,), fill, dtype=dtype, device=dev)
    buf[int(n):] = 7.0
    return buf


def _guard_ok(buf, what):
    assert bool((buf[-GUARD:] == 7.0).all()), f"{what}: wrote behind the buffer"


def _take(buf, shape, what, lead=0):
    """The output on the host in `shape`, after the guard was seen intact and every element finite.  lead: elements in front
    of the output (a pointer handed over 4 bytes into its buffer), which must still be NaN."""
    torch.cuda.synchronize()
    out = buf.cpu()
    _guard_ok(out, what)
    assert bool(torch.isnan(out[:lead]).all()), f"{what}: wrote in front of the buffer"
    out = out[lead:-GUARD].view(*shape)
    assert bool(torch.isfinite(out).all()), f"{what}: elements left unwritten or not finite"
    return out


def _untouched(buf, what):
    torch.cuda.synchronize()
    out = buf.cpu()
    _guard_ok(out, what)
    assert bool(torch.isnan(out[:-GUARD]).all()), f"{what}: a rejected call wrote something"


def _same_bits(a, b, what):
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    assert torch.equal(a.view(view), b.view(view)), f"{what}: not the same bits"


def _check(what, got, want, terms):
    return ref.report(what, got, want, terms)


# ------------------------------------------------------------------------------------------------------------------
# cpn_conv4d: every arm, the published statistics
# ------------------------------------------------------------------------------------------------------------------
PARAMS = ("wq", "bq", "ws", "bs")


@functools.lru_cache(maxsize=None)
def _fwd_want(case):
    x = ref.make_conv4d_inputs(case)
    return x, ref.conv4d_fwd_ref(*(x[n] for n in ("x",) + PARAMS), *case[7:])


def _shifted(t, lead, dev):
    """t on the device, starting `lead` elements into its allocation."""
    buf = torch.empty(t.numel() + lead, dtype=t.dtype, device=dev)
    buf[lead:] = t.reshape(-1).to(dev)
    return buf[lead:]


def _conv4d(fc, dev, scratch, what, entry="cpn_conv4d", extra=()):
    """One call of cpn_conv4d (or, with `extra` = gn_w, gn_b, residual, eps, of cpn_conv4d_gn_relu) on fresh buffers ->
    (y on the host, stats on the host without its guard, the device buffers of y and stats)."""
    arm, case, wmul, variant = fc
    B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p = case
    x = _fwd_want(case)[0]
    npos = ref.npos_of(case)
    lx, ly = int(variant == "x+4"), int(variant == "y+4")
    xd = _shifted(x["x"], lx, dev)
    assert xd.data_ptr() % 16 == 4 * lx
    w = [x[n].to(dev) for n in PARAMS]
    yb = _out(B * Co * npos + ly, dev)
    nst = _lib().cpn_gn_stats_doubles(B, Co, npos)
    stats = _out(nst, dev, torch.float64, 0.0)
    nscr = _lib().cpn_conv4d_scratch(B, Ci, Hq, Wq, Hs, Ws, s)
    assert (nscr > 0) == (s > 1)
    scr = _out(nscr, dev) if scratch and s > 1 else 0
    _call(entry, xd, *w, *extra, B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p, yb[ly:], stats, scr)
    y = _take(yb, (B, Co, *ref.out_dims(case)), what + " y", lead=ly)
    if isinstance(scr, torch.Tensor):
        _take(scr, (nscr,), what + " scratch")
    st = stats.cpu()
    _guard_ok(st, what + " stats")
    return y, st[:-GUARD], yb, stats


def _check_stats(what, st, y, B, W):
    assert ref.written_partials(st, B) == W, f"{what}: {ref.written_partials(st, B)} partial pairs per sample, the arm launches {W}"
    assert st[2 * B:3 * B].view(torch.int64).tolist() == [W] * B, f"{what}: arrival counters"
    final = st[:2 * B].reshape(B, 2)
    _same_bits(final, ref.stats_replay(st, B, W), what + " stats against the replay of the fixed order")
    _check(what + " stats", final, *ref.gn_stats_ref(y))


@pytest.mark.parametrize("fc", ref.FWD_CASES, ids=ref.fwd_id)
def test_conv4d_forward_against_float64(fc, dev):
    """y against float64 on the arm the case names (the launch published that arm's number of partial pairs), the final
    statistics bit-equal to the replay of gn_publish's fixed order over those pairs and within float64 rounding of the sums of
    the kernel's own y, a second run with the same bits.  A strided case with scratch and with scratch = NULL: either y within
    the one reference's bound."""
    arm, case, wmul, variant = fc
    B = case[0]
    want, terms = _fwd_want(case)[1]
    for scratch in ((True, False) if case[8] > 1 else (True,)):
        what = f"conv4d {ref.fwd_id(fc)}" + ("" if scratch else " scratch=NULL")
        W = ref.launched_w(fc, scratch)
        y, st, _, _ = _conv4d(fc, dev, scratch, what)
        _check(what + " y", y, want, terms)
        _check_stats(what, st, y, B, W)
        y2, st2, _, _ = _conv4d(fc, dev, scratch, what + " again")
        _same_bits(y, y2, what + " y, two runs")
        _same_bits(st, st2, what + " stats, two runs")


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("fc", ref.GN_RELU_CASES, ids=ref.fwd_id)
def test_conv4d_gn_relu_is_conv4d_then_gn_relu(fc, residual, dev):
    """One case per arm family: out bit-identical to cpn_conv4d followed by cpn_gn_relu in place (what the fused entry says it
    is), and within gn_fwd_ref's bound formed from the kernel's own y; the residual's addition rounds once more: u |out|."""
    arm, case, wmul, variant = fc
    B, Co = case[0], case[2]
    npos = ref.npos_of(case)
    x = _fwd_want(case)[0]
    gw, gb = x["gn_w"].to(dev), x["gn_b"].to(dev)
    res = x["res"].to(dev) if residual else 0
    what = f"conv4d_gn_relu {ref.fwd_id(fc)}" + (" +residual" if residual else "")
    y, st, yb, stats = _conv4d(fc, dev, True, what + " (two calls)")
    _call("cpn_gn_relu", yb, stats, gw, gb, res, EPS, B, Co, npos, yb)
    two = _take(yb, y.shape, what + " out of the two calls")
    out, st1, _, _ = _conv4d(fc, dev, True, what, entry="cpn_conv4d_gn_relu", extra=(gw, gb, res, EPS))
    _same_bits(out, two, what + " against cpn_conv4d + cpn_gn_relu")
    _same_bits(st, st1, what + " stats")
    want, terms = ref.gn_fwd_ref(y.reshape(B, Co, npos), x["gn_w"], x["gn_b"])
    if residual:
        want = want + x["res"].double().reshape(B, Co, npos)
        terms = dict(terms, residual=ref.U * want.abs())
    _check(what + " out", out.reshape(B, Co, npos), want, terms)


# ------------------------------------------------------------------------------------------------------------------
# cpn_conv4d_strided_bwd
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ref.SBWD_CASES, ids=ref.sbwd_id)
def test_conv4d_strided_bwd_against_float64(sc, dev):
    """dx, gwq, gws, gb against the float64 VJP with the routing written out (ragged ceil-mode windows; on the ties case half of
    every window is 0 and the rest repeats); the non-zero elements of dx are exactly the routed ones; dx = NULL and
    gwq = gws = gb = NULL change no bit of the other outputs; two runs give the same bits."""
    case, variant = sc
    B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p = case
    x = ref.make_conv4d_inputs(case, variant)
    want = ref.strided_bwd_ref(x["x"], x["dy"], x["wq"], x["ws"], k, s, p)
    xd, dyd, wq, ws = (x[n].to(dev) for n in ("x", "dy", "wq", "ws"))
    nscr = _lib().cpn_conv4d_strided_bwd_scratch(B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p)
    assert nscr > 0
    what = "strided_bwd " + ref.sbwd_id(sc)
    shapes = {"dx": x["x"].shape, "gwq": x["wq"].shape, "gws": x["ws"].shape, "gb": (Co,)}

    def run(tag, names):
        scr = _out(nscr, dev)
        bufs = {n: (_out(torch.Size(shapes[n]).numel(), dev) if n in names else 0) for n in shapes}
        _call("cpn_conv4d_strided_bwd", xd, dyd, wq, ws, B, Ci, Co, Hq, Wq, Hs, Ws, k, s, p, scr, bufs["dx"], bufs["gwq"], bufs["gws"],
              bufs["gb"])
        got = {n: _take(bufs[n], shapes[n], f"{what} {tag} {n}") for n in names}
        _guard_ok(scr.cpu(), f"{what} {tag} scratch")
        return got

    full = run("full", ("dx", "gwq", "gws", "gb"))
    for n in shapes:
        _check(f"{what} {n}", full[n], want[n], want[n + "_terms"])
    assert torch.equal(full["dx"] != 0, want["routed"]), f"{what}: dx is non-zero at other elements than the routed maxima"
    again = run("again", ("dx", "gwq", "gws", "gb"))
    only_w = run("dx=NULL", ("gwq", "gws", "gb"))
    only_x = run("weights=NULL", ("dx",))
    for n in shapes:
        _same_bits(full[n], again[n], f"{what} {n}, two runs")
        _same_bits(full[n], (only_x if n == "dx" else only_w)[n], f"{what} {n}, with the other outputs NULL")


# ------------------------------------------------------------------------------------------------------------------
# weight gradients and the token DWConv
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.PLANES_CASES, ids=ref.case_id)
def test_conv_wgrad_planes_against_float64(case, dev):
    """Every instantiation (<8,8>, <8,32>, <32,32> and the swapped <8,32>), one plane and more planes than workgroups' turns,
    H W = 256 and odd sizes; db = NULL changes no bit of dw."""
    B, Ci, Co, G, H, W, with_db = case
    x = ref.make_planes_inputs(case)
    want = ref.wgrad_planes_ref(x["x"], x["dy"])
    xd, dyd = x["x"].to(dev), x["dy"].to(dev)
    npart = _lib().cpn_conv_wgrad_scratch(Ci, Co)
    what = "wgrad_planes " + ref.case_id(case)

    def run(tag, db_given):
        part, dw, db = _out(npart, dev), _out(Co * Ci * 9, dev), (_out(Co, dev) if db_given else 0)
        _call("cpn_conv_wgrad_planes", xd, dyd, B, Ci, Co, G, H, W, part, dw, db)
        got = _take(dw, (Co, Ci, 3, 3), f"{what} {tag} dw"), (_take(db, (Co,), f"{what} {tag} db") if db_given else None)
        _guard_ok(part.cpu(), f"{what} {tag} partial")
        return got

    dw, db = run("first", True)
    _check(what + " dw", dw, want["dw"], want["dw_terms"])
    _check(what + " db", db, want["db"], want["db_terms"])
    dw2, db2 = run("again", True)
    _same_bits(dw, dw2, what + " dw, two runs")
    _same_bits(db, db2, what + " db, two runs")
    if not with_db:
        _same_bits(dw, run("db=NULL", False)[0], what + " dw with db = NULL")


@pytest.mark.parametrize("case", ref.DW_WGRAD_CASES, ids=ref.case_id)
def test_dwconv3x3_wgrad_against_float64(case, dev):
    N, C, H, W = case
    x = ref.make_dw_wgrad_inputs(case)
    want = ref.dwconv_wgrad_ref(x["x"], x["dy"])
    xd, dyd = x["x"].to(dev), x["dy"].to(dev)
    what = "dwconv_wgrad " + ref.case_id(case)
    runs = []
    for db_given in (True, True, False):
        dw, db = _out(C * 9, dev), (_out(C, dev) if db_given else 0)
        _call("cpn_dwconv3x3_wgrad", xd, dyd, N, C, H, W, dw, db)
        runs.append((_take(dw, (C, 3, 3), what + " dw"), _take(db, (C,), what + " db") if db_given else None))
    _check(what + " dw", runs[0][0], want["dw"], want["dw_terms"])
    _check(what + " db", runs[0][1], want["db"], want["db_terms"])
    _same_bits(runs[0][0], runs[1][0], what + " dw, two runs")
    _same_bits(runs[0][1], runs[1][1], what + " db, two runs")
    _same_bits(runs[0][0], runs[2][0], what + " dw with db = NULL")


@pytest.mark.parametrize("flip", ref.DW_FLIPS)
@pytest.mark.parametrize("case", ref.DW_TOKENS_CASES, ids=ref.case_id)
def test_dwconv3x3_tokens_against_float64(case, flip, dev):
    """flip 0: the forward with its bias; 1: the data gradient (flipped taps, bias NULL) of dy; 2: the forward with the exact
    GELU, whose bound carries the ASSUMED 4 ulp of erff (tests/conv4d_ref.py).  H != W but on the 16 x 16 case."""
    B, H, W, C = case
    x = ref.make_dw_tokens_inputs(case)
    src, bias = (x["dy"], None) if flip == 1 else (x["x"], x["bias"])
    want, terms = ref.dwconv_tokens_ref(src, x["w"], bias, H, W, flip)
    sd, wd, bd = src.to(dev), x["w"].to(dev), (0 if bias is None else bias.to(dev))
    what = f"dwconv_tokens flip {flip} {ref.case_id(case)}"
    runs = []
    for _ in range(2):
        y = _out(B * H * W * C, dev)
        _call("cpn_dwconv3x3_tokens", sd, wd, bd, B, H, W, C, flip, y)
        runs.append(_take(y, (B, H * W, C), what))
    _check(what, runs[0], want, terms)
    _same_bits(runs[0], runs[1], what + ", two runs")


@pytest.mark.parametrize("case", ref.DW_TOKENS_WGRAD_CASES, ids=ref.case_id)
def test_dwconv3x3_tokens_wgrad_against_float64(case, dev):
    B, H, W, C = case
    x = ref.make_dw_tokens_inputs(case)
    want = ref.dwconv_tokens_wgrad_ref(x["x"], x["dy"], H, W)
    xd, dyd = x["x"].to(dev), x["dy"].to(dev)
    npart = _lib().cpn_dwconv3x3_tokens_wgrad_scratch(B, H, C)
    what = "dwconv_tokens_wgrad " + ref.case_id(case)
    runs = []
    for db_given in (True, True, False):
        part, dw, db = _out(npart, dev), _out(C * 9, dev), (_out(C, dev) if db_given else 0)
        _call("cpn_dwconv3x3_tokens_wgrad", xd, dyd, B, H, W, C, part, dw, db)
        runs.append((_take(dw, (C, 9), what + " dw"), _take(db, (C,), what + " db") if db_given else None))
        _take(part, (npart,), what + " partial")
    _check(what + " dw", runs[0][0], want["dw"], want["dw_terms"])
    _check(what + " db", runs[0][1], want["db"], want["db_terms"])
    _same_bits(runs[0][0], runs[1][0], what + " dw, two runs")
    _same_bits(runs[0][1], runs[1][1], what + " db, two runs")
    _same_bits(runs[0][0], runs[2][0], what + " dw with db = NULL")


# ------------------------------------------------------------------------------------------------------------------
# rejections
# ------------------------------------------------------------------------------------------------------------------
def test_rejected_shapes_return_the_error_code_and_write_nothing(dev):
    """CPN_E_SHAPE (-2) before any launch: a NaN output stays NaN, zeroed statistics stay zero.  The buffers are large enough
    for the launch that must not happen."""
    big = 1 << 16
    src = torch.zeros(big, device=dev)

    def rejected(name, *args):
        with pytest.raises(RuntimeError, match=rf"{name} failed \(status -2\)"):
            _call(name, *args)

    y, stats = _out(big, dev), _out(big, dev, torch.float64, 0.0)
    rejected("cpn_conv4d", src, src, src, src, src, 1, 1, 8, 6, 6, 6, 6, 3, 2, 0, y, stats, 0)       # conv output 2, pooled size 3
    _untouched(y, "cpn_conv4d y")
    torch.cuda.synchronize()
    st = stats.cpu()
    _guard_ok(st, "cpn_conv4d stats")
    assert bool((st[:-GUARD] == 0).all()), "cpn_conv4d: a rejected call wrote statistics"

    part, dw, db = _out(_lib().cpn_conv_wgrad_scratch(1, 1), dev), _out(big, dev), _out(big, dev)
    rejected("cpn_conv_wgrad_planes", src, src, 1, 1, 1, 2, 5, 3, part, dw, db)                      # W = 3
    rejected("cpn_conv_wgrad_planes", src, src, 1, 1, 1, 2, 1, 257, part, dw, db)                    # H W = 257
    for buf, name in ((part, "partial"), (dw, "dw"), (db, "db")):
        _untouched(buf, "cpn_conv_wgrad_planes " + name)

    y = _out(big, dev)
    rejected("cpn_dwconv3x3_tokens", src, src, src, 1, 3, 5, 6, 0, y)                                # C = 6
    _untouched(y, "cpn_dwconv3x3_tokens y")

    scr, dx, gwq, gws, gb = (_out(big, dev) for _ in range(5))
    rejected("cpn_conv4d_strided_bwd", src, src, src, src, 1, 1, 4, 5, 6, 7, 8, 3, 2, 1, scr, dx, gwq, gws, gb)   # Cout = 4
    for buf, name in ((scr, "scratch"), (dx, "dx"), (gwq, "gwq"), (gws, "gws"), (gb, "gb")):
        _untouched(buf, "cpn_conv4d_strided_bwd " + name)
