"""Float64 references, with element-wise error bounds, of the kernels that form the attention logits - cpn_local_units and the
logit half of cpn_attend_units (csrc/local_units_body.h: the three-layer per-sample MLP tails of both attention rounds on MFMA
fragments in unit order), cpn_local_hidden (csrc/gather.hip: the same first layer in row order, for training) - and the host
form of the unit-order input copy lv_u that cpn_sample_geometry writes, for tests/test_logits_ref.py (CPU) and
tests/test_gpu_logits_f64.py (GPU).  Helpers, not tests.

Nothing here looks at a kernel's arithmetic: every reference takes the values a kernel READS (fp16 / fp32 bits converted to
float64) and forms the mathematical result in float64, on whatever device its inputs live on.  The bounds are first order in
u16 = 2^-11 and u32 = 2^-24, from operation counts; a `mag` is the same formula on absolute values.

The operation
    L16(row)  = ctx dir 3 (loc8[0:3]) | 0 0 0 | query dir 3 (coords9[0:3]) | tanh depth x4 (loc8[3:7]) | origin 3 (coords9[6:9])
    h         = relu(W1 L16 + b1 (+ add[ray - ray0]))              (columns 3 .. 5 of W1 meet zeros: they cannot matter)
    out       = W2 h + b2
    mode 0:   ce = out(query_embed, query_embed_2),  key = Wk2 kh + bk2,                      logit = <key, ce>
    mode 2:   q2 = out(query_repeat_embed[:, 128:144] with add, query_repeat_embed_2),  ce as in mode 0 from (w1b, b1b, wk2, bk2),
              logit = <q2, ce>
Rows are in row order, row = ((ray - ray0) V + v) S + s; the unit-order operands (kh_u, ce_u, lv_u) are indexed through
coponerf_amd.render.unit_rows only (tests/test_pack_layouts.py pins it).

The bounds, and where their counts come from (csrc/local_units_body.h)
    dh    = u16 h + 52 u32 mag1 + 2^-25 (sum_k |x_k| + |w_k|) + 2^-25
            first layer as three K = 16 fp16 MFMAs on a hi / lo split (w = wh + wl, x = xh + xl): the products are exact in
            fp32; the dropped wl xl is 2^-22 |w x| = 4 u32; three MFMAs of 16 terms onto one accumulator that starts at the add row
            are at most 48 fp32 additions per term; a lo half that lands among the fp16 subnormals is off by 2^-25 absolute, times
            the other operand; the hidden value is rounded to fp16 once (packed conversion, ReLU behind it: the same value).
            mag1 = |W1| |x| + |b1| + |add|.
    dout  = u16 |out| + |W2| dh + 136 u32 mag2 + 2^-25
            ReLU is 1-Lipschitz: dh passes it unchanged and no hidden unit near zero needs an exclusion.  Four K = 32 MFMAs on an
            accumulator that starts at the bias: 129 terms, 128 additions in an order the hardware chooses, 8 of margin; one
            rounding to fp16.  mag2 = |W2| h + |b2|.  dkey is the same with kh exact (dh = 0).
    dlogit = sum_c (da |b| + db |a| + da db) + 136 u32 sum_c |a| |b|
            128 products of fp16 values (exact in fp32) added in fp32: 32 per lane, two __shfl_xor steps.
The logit bound is an L1 bound over 128 channels and loose by about sqrt(128), so each branch is ALSO seen element by element
through probe weights that make the other operand exactly one-hot in fp16 (PROBES): the logit is then the fp16 value of one
channel of one branch.  A defect at the 2^-22 level of the hi / lo split (a dropped wh xl term is 2^-11, and is seen; a dropped
wl xl or a wrongly rounded lo half is not) is below what fp16 outputs can show: no test here claims it.

cpn_local_hidden: out = fp16(relu(W L16 + bias + add)) with fp32 operands on the fp32 MFMA:
    |d| <= u16 |want| + 19 u32 mag + 2^-25       (16 terms added, bias + add, one rounding of a product)

Calibration on the CPU (tests/test_logits_ref.py, the kernels' rounding points in fp32 torch), worst err/bound over its cases:
    mode 0: ce 0.412, key 0.935, logit 0.035      mode 2: q2 0.448, ce 0.425, logit 0.023
    ce under a leading bias (bias_led) 0.897      cpn_local_hidden 0.985
"""
import torch

from coponerf_amd import synthetic as syn
from coponerf_amd.render import unit_rows

V = 2
U32 = 2.0 ** -24
U16 = 2.0 ** -11
SUB16 = 2.0 ** -25
F16_MAX = 65504.0
C_L1 = 52               # first layer: 48 additions + 4 u32 for the dropped lo x lo products
C_L2 = 136              # a 128 -> 128 layer / the 128-term dot product
C_HID = 19              # cpn_local_hidden
DEAD = 100.0            # what the dead rows of kh_u hold: finite, and far outside anything a live row produces
POISON = 1.0e4          # loc8 / coords9 of rays outside the window

# (B, R, S, ray0, nrays, gain); one reason each
PLAIN = (2, 5, 6, 0, 10, 1)             # R, S no multiples of 4: partial units in both directions
WINDOW = (3, 3, 16, 2, 6, 1)            # starts inside b = 0, ends inside b = 2: dead rows that belong to rays outside the window
ONE_RAY = (1, 37, 30, 22, 1, 1)         # one ray in the middle of a group
SHORT = (1, 4, 3, 1, 2, 1)              # S < 4: one sample block, T = 6
GAIN16 = (3, 3, 16, 2, 6, 16)           # large logits
BIG = (1, 262, 126, 1, 260, 1)          # 66 groups x 2 x 32 = 4224 units > 4096: live second units, a second trip of some waves
BIG_SMALL = (1, 22, 10, 1, 20, 1)       # the same window (first and last group partial) for the CPU emulation
SMALL_CASES = [PLAIN, WINDOW, ONE_RAY, SHORT, GAIN16]
PROBE_CASES = [PLAIN, WINDOW]
HIDDEN_CASES = [PLAIN, WINDOW, ONE_RAY]
LIMIT_CASES = {0: (1, 3, 928, 0, 3, 1), 2: (1, 3, 842, 0, 3, 1)}     # unit_lds_bytes<MODE>() + 48 V S <= 160 KiB, to the byte
GEOMETRY_SHAPES = [(2, 5, 70), (1, 4, 64), (1, 3, 7), (1, 9, 128)]   # (B, R, S)
EMU_CASES = SMALL_CASES + [BIG_SMALL]


def case_id(c):
    return "B%d-R%d-S%d-ray%d+%d-gain%d" % tuple(c)


# ------------------------------------------------------------------------------------------------------------------
# row maps
# ------------------------------------------------------------------------------------------------------------------
def first_group(R, ray0):
    gpb = (R + 3) // 4
    b = ray0 // R
    return b * gpb + (ray0 - b * R) // 4


def unit_count(B, R, S, ray0, nrays):
    return unit_rows(B, R, S, ray0, nrays).numel() // 16


def total_units(B, R, S):
    return B * ((R + 3) // 4) * V * ((S + 3) // 4)


def sample_index(B, R, S, ray0, nrays, device=None):
    """(nrays V S,) flat index into (B V, R, S) of every row of the window, in row order."""
    ray = torch.arange(ray0, ray0 + nrays, device=device).view(-1, 1, 1)
    v = torch.arange(V, device=device).view(1, -1, 1)
    s = torch.arange(S, device=device).view(1, 1, -1)
    return ((((ray // R) * V + v) * R + ray % R) * S + s).reshape(-1)


def rows_L16(loc8, coords9, B, R, S, ray0, nrays):
    """(nrays V S, 16) float64: local_coords of every row of the window from loc8 (B V, R, S, 8) / coords9 (B V, R, 9)."""
    idx = sample_index(B, R, S, ray0, nrays, loc8.device)
    l8 = loc8.reshape(-1, 8)[idx].double()
    c9 = coords9.reshape(-1, 9)[idx // S].double()
    z = torch.zeros_like(l8[:, :3])
    return torch.cat((l8[:, 0:3], z, c9[:, 0:3], l8[:, 3:7], c9[:, 6:9]), 1)


def lvu_from_loc(loc8, coords9, B, R, S):
    """The header's lv_u of the WHOLE (B, R, S) problem, built on the host: (units 64, 4) fp32, lane c + 16 fg of unit
    ((b ceil(R/4) + r/4) V + v) ceil(S/4) + s/4, c = (s & 3) 4 + (r & 3), holds K entries 4 fg .. 4 fg + 3 of the row's 16
    inputs with 1.0 (the bias's multiplier) on K slot 3; slots of rays >= R / samples >= S are zero."""
    idx = unit_rows(B, R, S, 0, B * R, loc8.device)                  # the whole problem: group0 = 0, global unit numbers
    x = rows_L16(loc8, coords9, B, R, S, 0, B * R).float()
    x[:, 3] = 1.0
    units = idx.numel() // 16
    out = torch.zeros(units * 16, 16, dtype=torch.float32, device=loc8.device)
    out[idx >= 0] = x[idx[idx >= 0]]
    return out.view(units, 16, 4, 4).permute(0, 2, 1, 3).reshape(units * 64, 4).contiguous()    # [unit][c][fg][4] -> [unit][fg][c][4]


def rows_from_lvu(lvu, B, R, S, ray0, nrays):
    """(nrays V S, 16) fp32: the 16 K slots of every row of the window as a given lv_u holds them (slot 3 is the bias's 1.0)."""
    idx = unit_rows(B, R, S, ray0, nrays, lvu.device)
    units = idx.numel() // 16
    u0 = first_group(R, ray0) * V * ((S + 3) // 4)
    t = lvu.reshape(-1, 64, 4)[u0:u0 + units].reshape(units, 4, 16, 4).permute(0, 2, 1, 3).reshape(units * 16, 16)
    out = torch.zeros(nrays * V * S, 16, dtype=lvu.dtype, device=lvu.device)
    out[idx[idx >= 0]] = t[idx >= 0]
    return out


def L16_of_lvu(lvu, B, R, S, ray0, nrays):
    """rows_from_lvu as float64 local_coords: slot 3 must hold the 1.0 and is the zero channel of L16."""
    x = rows_from_lvu(lvu, B, R, S, ray0, nrays).double()
    assert bool((x[:, 3] == 1.0).all()), "K slot 3 of lv_u is not 1.0"
    x[:, 3] = 0.0
    return x


def to_unit_order(x, B, R, S, ray0, nrays, dead=DEAD):
    """(nrays V S, 128) row-major -> the launch's unit order (units 16, 128) [unit][p][lane = c + 16 fg][8]; dead rows = `dead`.
    The inverse of coponerf_amd.render.rows_from_unit_order."""
    idx = unit_rows(B, R, S, ray0, nrays, x.device)
    units = idx.numel() // 16
    t = torch.full((units * 16, 128), dead, dtype=x.dtype, device=x.device)
    t[idx >= 0] = x[idx[idx >= 0]]
    return t.view(units, 16, 4, 4, 8).permute(0, 2, 3, 1, 4).reshape(units * 16, 128).contiguous()     # [unit][c][p][fg][8] ->


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def first_layer_ref(L16, W1, b1, add_rows, c_u32=C_L1, split=True):
    """h = relu(W1 L16 + b1 (+ add)) in float64 -> (h, dh).  add_rows: (rows, 128) or None."""
    x, w = L16.double(), W1.double()[:, :16]
    pre = x @ w.t() + b1.double()
    mag = x.abs() @ w.abs().t() + b1.double().abs()
    if add_rows is not None:
        pre = pre + add_rows.double()
        mag = mag + add_rows.double().abs()
    h = torch.relu(pre)
    dh = U16 * h + c_u32 * U32 * mag + SUB16
    if split:
        live = (x != 0).double()
        dh = dh + SUB16 * (x.abs().sum(1, keepdim=True) + live @ w.abs().t() + 1.0)        # (+ 1: the bias's lo half times 1.0)
    return h, dh


def layer128_ref(h, dh, W2, b2):
    """out = W2 h + b2 -> (out, dout); h exact when dh is None."""
    w, b = W2.double()[:, :128], b2.double()
    out = h @ w.t() + b
    mag = h.abs() @ w.abs().t() + b.abs()
    dout = U16 * out.abs() + C_L2 * U32 * mag + SUB16
    if dh is not None:
        dout = dout + dh @ w.abs().t()
    assert float(out.abs().max()) < F16_MAX, "a reference value leaves fp16's range"
    return out, dout


def mlp_ref(L16, W1, b1, add_rows, W2, b2):
    h, dh = first_layer_ref(L16, W1, b1, add_rows)
    return layer128_ref(h, dh, W2, b2)


def dot_ref(a, da, b, db):
    """logit = <a, b> -> (logit, dlogit)."""
    want = (a * b).sum(1)
    bound = (da * b.abs() + db * a.abs() + da * db).sum(1) + C_L2 * U32 * (a.abs() * b.abs()).sum(1)
    return want, bound


def add_rows_of(add, S):
    """(nrays, 128) -> (nrays V S, 128): the row of `add` every row of the window reads, ray - ray0."""
    return add.repeat_interleave(V * S, 0)


def logits_ref(mode, L16, d, S, kh=None):
    """The reference of one launch -> dict of the branches (value, bound) and the logit.  d: the operand dict of make_inputs (or
    one with probe weights); L16 from rows_L16 / L16_of_lvu; kh (rows, 128) fp16 in row order (mode 0)."""
    if mode == 0:
        ce, dce = mlp_ref(L16, d["w1"], d["b1"], None, d["w2"], d["b2"])
        key, dkey = layer128_ref(kh.double(), None, d["wk2"], d["bk2"])
        lg, dlg = dot_ref(key, dkey, ce, dce)
        return {"ce": (ce, dce), "key": (key, dkey), "logit": (lg, dlg)}
    q2, dq2 = mlp_ref(L16, d["w1"], d["b1"], add_rows_of(d["add"], S), d["w2"], d["b2"])
    ce, dce = mlp_ref(L16, d["w1b"], d["b1b"], None, d["wk2"], d["bk2"])
    lg, dlg = dot_ref(q2, dq2, ce, dce)
    return {"q2": (q2, dq2), "ce": (ce, dce), "logit": (lg, dlg)}


def local_hidden_ref(L16, W, bias, add_rows):
    """cpn_local_hidden -> (want, bound), (rows, 128)."""
    return first_layer_ref(L16, W, bias, add_rows, c_u32=C_HID, split=False)


# ------------------------------------------------------------------------------------------------------------------
# probes: weights under which the logit is one channel of one branch
# ------------------------------------------------------------------------------------------------------------------
# name -> (mode, the layer made one-hot: weight key zeroed, bias key = e_c, the branch of logits_ref the logit then equals)
PROBES = {
    "key": (0, "w2", "b2", "key"),               # ce is exactly e_c: logit = fp16(key_c)
    "q2": (2, "wk2", "bk2", "q2"),               # the recomputed ce is e_c: logit = fp16(q2_c)
    "ce2": (2, "w2", "b2", "ce"),                # q2 is e_c: logit = the recomputed ce_c
}


def probe_operands(d, name, eye):
    """The operand dict of a probe: the one-hot layer's weight zeroed; its bias is row c of `eye` (128, 128), per launch."""
    _, wkey, bkey, _ = PROBES[name]
    p = dict(d)
    p[wkey] = torch.zeros_like(d[wkey])
    p[bkey] = eye
    return p


# ------------------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------------------
def ratio(got, want, bound):
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


def outside(got, want, bound):
    """How many elements leave the bound (a seeded defect must make this > 0)."""
    return int((~(ratio(got, want, bound) <= 1)).sum())


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def make_inputs(case, hid=False):
    """Everything one attention round reads for a case, on the CPU, from the counter-hash generators at the operand scales of
    tests/test_gpu_attend_units.py (`add` at 1.0: it differs strongly from ray to ray).  loc8 / coords9 of rays outside the
    window hold POISON; kh is (rows, 128) fp16 in ROW order (kh_u = to_unit_order(kh)); the first layers are also given inside a
    (128, 144) matrix at column 128 (w1_144, w1b_144) and the second layers inside (128, 136) (w2_136, wk2_136), the rest of
    which is POISON.  gain scales kh (what mode 0's logit is linear in) and w2g = gain w2 (mode 2's)."""
    B, R, S, ray0, nrays, gain = case
    N, T = B * V, V * S
    rows = nrays * T
    seed = 7 + 1000 * B + 100 * R + 10 * S + ray0
    f16 = torch.float16
    d = {
        "loc8": syn.uniform((N, R, S, 8), seed, -1.0, 1.0, stream=1), "coords9": syn.uniform((N, R, 9), seed, -1.0, 1.0, stream=2),
        "w1": syn.normal((128, 16), seed, 0.5, stream=3), "b1": syn.normal((128,), seed, 0.1, stream=4),
        "w2": syn.normal((128, 128), seed, 0.1, stream=5).to(f16), "b2": syn.normal((128,), seed, 0.1, stream=6),
        "wk2": syn.normal((128, 128), seed, 0.1, stream=7).to(f16), "bk2": syn.normal((128,), seed, 0.1, stream=8),
        "w1b": syn.normal((128, 16), seed, 0.5, stream=9), "b1b": syn.normal((128,), seed, 0.1, stream=10),
        "add": syn.normal((nrays, 128), seed, 1.0, stream=11),
        "kh": (syn.normal((rows, 128), seed, 1.0, stream=12) * gain).to(f16),
    }
    d["loc8"][..., 7] = 0.0
    out = torch.ones(B * R, dtype=torch.bool)
    out[ray0:ray0 + nrays] = False
    out = out.view(B, 1, R).expand(B, V, R).reshape(N, R)
    d["loc8"][out] = POISON
    d["coords9"][out] = POISON
    d["w2g"] = (d["w2"].float() * gain).to(f16)
    for k in ("w1", "w1b"):
        wide = torch.full((128, 144), POISON)
        wide[:, 128:] = d[k]
        d[k + "_144"] = wide
    for k in ("w2", "wk2", "w2g"):
        wide = torch.full((128, 136), POISON, dtype=f16)
        wide[:, :128] = d[k]
        d[k + "_136"] = wide
    if hid:
        d["hid"] = syn.uniform((rows * 2, 832), seed, 0.0, 2.0, stream=14).to(f16)
    return d


def bias_led(ops):
    """The operands with query_embed_2 scaled so that its bias leads (mode 0: w2 / 16, exact in fp16, and 10 b2): what the hidden
    layer's own rounding adds to ce is then well below ce's final rounding, and the element-wise ce bound is within a factor
    1.3 of half an ulp - tight enough for a conversion that rounds the wrong way to leave it.  At the plain operand scales
    |W2| dh is some 2.5 half-ulps of ce and hides it."""
    p = dict(ops)
    p["w2"] = (ops["w2"].float() / 16).to(torch.float16)
    p["b2"] = ops["b2"] * 10
    return p


def operands(d, mode):
    """The operand dict logits_ref takes for a mode of make_inputs' dict (mode 2's second layer carries the gain)."""
    if mode == 0:
        return {k: d[k] for k in ("w1", "b1", "w2", "b2", "wk2", "bk2")}
    return {"w1": d["w1"], "b1": d["b1"], "add": d["add"], "w2": d["w2g"], "b2": d["b2"], "wk2": d["wk2"], "bk2": d["bk2"],
            "w1b": d["w1b"], "b1b": d["b1b"]}
