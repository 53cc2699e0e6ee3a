"""Yardstick of coponerf_amd.matches.refine_homography, model_gric and select_pose (csrc/model_select.hip, csrc/sampson_h.h): a numpy
restatement, for ONE pair and vectorised over its matches, of the two rules of include/coponerf_hip.h (round 23) in the header's
operation sequence.  tests/test_model_select_ref.py holds it to independent forms on the CPU; tests/test_gpu_model_select.py compares
the kernels with it.  The summation order is tests/matches_ref.py's block_sum, the Jacobi method, the frames and the decomposition
tests/homography_ref.py's, the residual under E and the whole of RANSAC tests/ransac_ref.py's.

numpy float64 arithmetic is IEEE with one rounding per operation, which is what -ffp-contract=off gives the kernels, and every
expression below is written in the kernels' order.

Bounds (E = 2^-53), from operation counts, none from a run:
  gric          gric_bound: (RHO_OPS + the depth of the sum + 4) E (sum |rho| + ln 4 d n_u + ln(4 n_u) k).  A rho is at most
                RHO_OPS = 64 operations deep (2 into a normalised coordinate, 4 into m, 2 into C, 4 into a J, 5 into S, 8 through
                the Cholesky factor and y, 3 into e^2, 1 the quotient by sigma^2; under E round 16's 13 + 16 + 3), each relative
                to a value that is itself non-negative: nothing cancels between the terms.  The sum is rounds + 6 + 2 additions
                deep, the two penalties and their sums 4.  The bound assumes that no row changes sides at its cap: cap_margin.
  one step      refine_step_bound: tests/matches_ref.py's refine_step_bound at NP parameters - |delta - delta_ref|_2 <=
                |A^-1|_2 (|dA|_F |delta|_2 + |dg|_2) + CHOL_OPS(NP) E cond_2(A) |delta|_2 with dA and dg (TERM_OPS_H + the depth of
                the sum + 4) E times the sums of the absolute forms of the terms.  A term (w J0_j) J0_k + (w J1_j) J1_k is at most
                TERM_OPS_H = 160 operations deep: 30 into y (above), about 60 more into dy (dm 4, dC 2, dJ 4, dA / dBq / dCq 7, the
                four quotients of the factor's derivative 8, dy 9, on top of y's own), 6 for the weight, 5 for the term; 160 leaves
                room for the second order.  The absolute forms replace every difference by the sum of the magnitudes and keep the
                true l00, l10, l11 in the denominators.  Mode 0 then normalises h + delta: an entry moves by at most 2 |d delta| +
                STATE_OPS E; mode 1 is tests/matches_ref.py's POSE_OPS E.
  recovery      rounding_tolerance: exact matches whose coordinates are rounded to fp32 move by at most eps = half an fp32 ulp of
                256 per coordinate, 2 eps per match in the norm e measures; to first order the least-squares state moves by at
                most 2 eps sqrt(n) / sqrt(lambda) with lambda the smallest eigenvalue of the (unweighted: w = 1 at e = 0) normal
                matrix on the directions the gauge leaves free.
"""
import functools

import numpy as np

from tests import homography_ref as hr
from tests import matches_ref as mr
from tests import ransac_ref as rr

E = mr.E
NT = mr.NT
RHO_OPS = 64
TERM_OPS_H = 160
STATE_OPS = 32
LN4 = 1.3862943611198906
DIM = (3.0, 2.0, 2.0)
PAR = (5.0, 8.0, 3.0)
CAP_MARGIN = 1e-9


def chol_ops(NP):
    return NP * NP * 4


# ------------------------------------------------------------------------------------------------------------ the residual
def sampson_h(H, k0, k1, a0, a1, b0, b1, true=None):
    """THE HOMOGRAPHY'S SAMPSON RESIDUAL of the normalised points under H (9) -> dict of the header's values and `ok`.
    true: the dict of the same call on the true values - this call then forms the ABSOLUTE form (H, a, b must be magnitudes):
    every difference is the sum of the magnitudes, the denominators l00, l10, l11 are the true ones."""
    mag = true is not None
    sub = (lambda p, c: p + c) if mag else (lambda p, c: p - c)
    with np.errstate(all="ignore"):
        m0 = (H[0] * b0 + H[1] * b1) + H[2]
        m1 = (H[3] * b0 + H[4] * b1) + H[5]
        m2 = (H[6] * b0 + H[7] * b1) + H[8]
        C0, C1 = sub(m0, a0 * m2), sub(m1, a1 * m2)
        neg = m2 if mag else -m2
        J00, J11 = neg / k0[0], neg / k0[1]
        J02, J03 = sub(H[0], a0 * H[6]) / k1[0], sub(H[1], a0 * H[7]) / k1[1]
        J12, J13 = sub(H[3], a1 * H[6]) / k1[0], sub(H[4], a1 * H[7]) / k1[1]
        if mag:
            l00, l10, l11 = true["l00"], np.abs(true["l10"]), true["l11"]
            y0 = C0 / l00
            y1 = (C1 + l10 * y0) / l11
            return dict(a0=a0, a1=a1, b0=b0, b1=b1, C0=C0, C1=C1, J00=J00, J02=J02, J03=J03, J11=J11, J12=J12, J13=J13, l00=l00,
                        l10=l10, l11=l11, y0=y0, y1=y1, e2=true["e2"], ok=true["ok"])
        A = (J00 * J00 + J02 * J02) + J03 * J03
        Bq = J02 * J12 + J03 * J13
        Cq = (J11 * J11 + J12 * J12) + J13 * J13
        l00 = np.sqrt(A)
        l10 = Bq / l00
        d = Cq - l10 * l10
        l11 = np.sqrt(d)
        y0 = C0 / l00
        y1 = (C1 - l10 * y0) / l11
        e2 = y0 * y0 + y1 * y1
        ok = (A > 0.0) & (d > 0.0)
        for v in (m0, m1, m2, C0, C1, A, Bq, Cq, l00, l10, l11, y0, y1, e2):
            ok = ok & np.isfinite(v)
    return dict(a0=a0, a1=a1, b0=b0, b1=b1, C0=C0, C1=C1, J00=J00, J02=J02, J03=J03, J11=J11, J12=J12, J13=J13, l00=l00, l10=l10,
                l11=l11, y0=y0, y1=y1, e2=e2, ok=ok, A=A, Bq=Bq, Cq=Cq)


def along(s, dH, k0, k1, defect=None, mag=False):
    """(dy0, dy1) ALONG the direction dH (9): the full derivative of y.  defect="dropped dl11": dy1 without its y1 dl11 term;
    "frozen whitening": L is not differentiated.  mag=True: the absolute form on sampson_h's absolute dict (dH magnitudes)."""
    sub = (lambda p, c: p + c) if mag else (lambda p, c: p - c)
    with np.errstate(all="ignore"):
        dm0 = (dH[0] * s["b0"] + dH[1] * s["b1"]) + dH[2]
        dm1 = (dH[3] * s["b0"] + dH[4] * s["b1"]) + dH[5]
        dm2 = (dH[6] * s["b0"] + dH[7] * s["b1"]) + dH[8]
        dC0, dC1 = sub(dm0, s["a0"] * dm2), sub(dm1, s["a1"] * dm2)
        neg = dm2 if mag else -dm2
        dJ00, dJ11 = neg / k0[0], neg / k0[1]
        dJ02, dJ03 = sub(dH[0], s["a0"] * dH[6]) / k1[0], sub(dH[1], s["a0"] * dH[7]) / k1[1]
        dJ12, dJ13 = sub(dH[3], s["a1"] * dH[6]) / k1[0], sub(dH[4], s["a1"] * dH[7]) / k1[1]
        dA = 2.0 * ((s["J00"] * dJ00 + s["J02"] * dJ02) + s["J03"] * dJ03)
        dBq = ((dJ02 * s["J12"] + s["J02"] * dJ12) + dJ03 * s["J13"]) + s["J03"] * dJ13
        dCq = 2.0 * ((s["J11"] * dJ11 + s["J12"] * dJ12) + s["J13"] * dJ13)
        if defect == "frozen whitening":
            dA, dBq, dCq = 0.0 * dA, 0.0 * dBq, 0.0 * dCq
        dl00 = dA / (2.0 * s["l00"])
        dl10 = sub(dBq, s["l10"] * dl00) / s["l00"]
        dl11 = sub(dCq, (2.0 * s["l10"]) * dl10) / (2.0 * s["l11"])
        dy0 = sub(dC0, s["y0"] * dl00) / s["l00"]
        if defect == "dropped dl11":
            dy1 = sub(sub(dC1, dl10 * s["y0"]), s["l10"] * dy0) / s["l11"]
        else:
            dy1 = sub(sub(sub(dC1, dl10 * s["y0"]), s["l10"] * dy0), s["y1"] * dl11) / s["l11"]
    return dy0, dy1


def unit_directions():
    return [np.eye(9)[k] for k in range(9)]


def rotation_directions(R9):
    return [mr.cross_rows(R9.reshape(3, 3), k).reshape(9) for k in range(3)]


def n_sums(NP):
    return NP * (NP + 1) // 2 + NP + 3


def pass_sums(rows, k0, k1, H, dirs, scale_px, defect=None, magnitude=False):
    """The sums of one pass over the matches rows (n, 4) float64 pixels at the state H (9) with the directions dirs: the upper
    triangle of the normal matrix by rows, the gradient, the cost, the sum of weights, the rows that count.  magnitude=True: the
    sums of the absolute forms of the terms of the matrix and the gradient (the last three as they are).
    defect="wave order": the four waves are added ((0 + 1) + 2) + 3 .. in the order 3, 2, 1, 0."""
    NP = len(dirs)
    a0, a1, b0, b1 = rr.normalised(rows, k0, k1)
    with np.errstate(all="ignore"):
        s = sampson_h(H, k0, k1, a0, a1, b0, b1)
        if magnitude:
            true = s
            r = np.abs(rows)
            s = sampson_h(np.abs(H), k0, k1, (r[:, 0] + abs(k0[2])) / k0[0], (r[:, 1] + abs(k0[3])) / k0[1],
                          (r[:, 2] + abs(k1[2])) / k1[0], (r[:, 3] + abs(k1[3])) / k1[1], true=true)
            J = [along(s, np.abs(d), k0, k1, mag=True) for d in dirs]
        else:
            J = [along(s, d, k0, k1, defect=defect) for d in dirs]
        u = 1.0 + s["e2"] / (scale_px * scale_px)
        w = 1.0 / (u * u)
        cols, grad = [], []
        for j in range(NP):
            w0, w1 = w * J[j][0], w * J[j][1]
            cols += [w0 * J[k][0] + w1 * J[k][1] for k in range(j, NP)]
            grad.append(w0 * s["y0"] + w1 * s["y1"])
        cols += grad + [(s["e2"] / 2.0) / u, w, np.ones_like(w)]
        terms = np.where(s["ok"][:, None], np.stack(cols, 1), 0.0)
    if defect == "wave order":
        return block_sum_reversed(terms)
    return mr.block_sum(terms)


def block_sum_reversed(terms):
    """block_sum with the waves added in another order: ((3 + 2) + 1) + 0."""
    n, V = terms.shape
    rounds = -(-n // NT)
    padded = np.zeros((rounds * NT, V))
    padded[:n] = terms
    acc = np.zeros((NT, V))
    for r in range(rounds):
        acc = acc + padded[r * NT:(r + 1) * NT]
    v = acc.reshape(4, 64, V)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    w = v[:, 0]
    return ((w[3] + w[2]) + w[1]) + w[0]


def damped(sums, NP, h=None, defect=None):
    """(A, g, M) of a pass: M the symmetric matrix of the sums, A = M with A_jj = M_jj + 1e-3 M_jj and, with h (mode 0), the
    gauge A += (tr M / 9) h h^T.  defect="no gauge"."""
    M = np.zeros((NP, NP))
    at = 0
    for j in range(NP):
        for k in range(j, NP):
            M[j, k] = M[k, j] = sums[at]
            at += 1
    g = sums[at:at + NP].copy()
    A = M.copy()
    trace = 0.0
    for j in range(NP):
        trace += M[j, j]
    for j in range(NP):
        A[j, j] = M[j, j] + 1e-3 * M[j, j]
    if h is not None and defect != "no gauge":
        pin = trace / 9.0
        for i in range(NP):
            for j in range(NP):
                A[i, j] = A[i, j] + pin * (h[i] * h[j])
    return A, g, M


def solve(A, g):
    """delta = -A^-1 g by the kernel's Cholesky (tests/matches_ref.py's solve6 at a size), or None."""
    NP = len(g)
    L = A.copy()
    with np.errstate(all="ignore"):
        for j in range(NP):
            s = L[j, j]
            for k in range(j):
                s -= L[j, k] * L[j, k]
            if not (s > 0.0) or not np.isfinite(s):
                return None
            l = np.sqrt(s)
            L[j, j] = l
            for i in range(j + 1, NP):
                v = L[i, j]
                for k in range(j):
                    v -= L[i, k] * L[j, k]
                L[i, j] = v / l
        y, x = np.zeros(NP), np.zeros(NP)
        for i in range(NP):
            v = -g[i]
            for k in range(i):
                v -= L[i, k] * y[k]
            y[i] = v / L[i, i]
        for i in range(NP - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, NP):
                v -= L[k, i] * x[k]
            x[i] = v / L[i, i]
    return x if np.isfinite(x).all() else None


def sum_squares9(h):
    ss = h[0] * h[0]
    for c in range(1, 9):
        ss = ss + h[c] * h[c]
    return ss


def nearest_rotation(h):
    """R_n = (u_1 v_1^T + u_2 v_2^T) + u_3 v_3^T (9) from round 20's Jacobi method and frames, as homography_ref.decompose forms it."""
    G, V, _ = hr.jacobi(h)
    with np.errstate(all="ignore"):
        U, W = rr._frame(G), rr._frame(V)
        Rn = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                Rn[i, j] = (U[0, i] * W[0, j] + U[1, i] * W[1, j]) + U[2, i] * W[2, j]
    return Rn.reshape(9)


def start_state(H0, mode):
    """The state the passes begin at, or None (status 2)."""
    h = np.asarray(H0, dtype=np.float64).reshape(9)
    if not np.isfinite(h).all():
        return None
    with np.errstate(all="ignore"):
        if mode == 0:
            nrm = np.sqrt(sum_squares9(h))
            if not (nrm > 0.0) or not np.isfinite(nrm):
                return None
            u = h / nrm
            if hr.determinant(u, hr.adjugate(u)) < 0.0:
                u = -u
            return u if np.isfinite(u).all() else None
        Rn = nearest_rotation(h)
    return Rn if np.isfinite(Rn).all() else None


def apply_step(H, x, mode):
    with np.errstate(all="ignore"):
        if mode == 0:
            nh = H + x
            ln = np.sqrt(sum_squares9(nh))
            if not (ln > 0.0) or not np.isfinite(ln):
                return None
            nh = nh / ln
        else:
            new = mr.apply_step(H.reshape(3, 3), np.array([1.0, 0.0, 0.0]), np.concatenate((x, np.zeros(3))))
            if new is None:
                return None
            nh = new[0].reshape(9)
    return nh if np.isfinite(nh).all() else None


def refine_homography(xy, count, intrinsics, H0, mode, iters=10, scale_px=2.0, defect=None):
    """The rule of cpn_refine_homography for ONE pair: xy (N, 4) fp32, H0 (9) -> (H (9), pose (4, 4) float64 before the fp32
    store, stats (8), trace): trace holds per solved pass the dict of A, g, M, delta, sums and the state, and last the sums and the
    state of the pass that only measured."""
    xy = np.asarray(xy, dtype=np.float32).astype(np.float64)
    H0 = np.asarray(H0, dtype=np.float64).reshape(9)
    n = min(max(int(count), 0), len(xy))
    H = start_state(H0, mode) if (n > 0 and iters > 0) else None
    if H is None:
        return H0.copy(), np.eye(4), np.array([0.0] * 7 + [2.0]), []
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    rows, start = xy[:n], H.copy()
    NP = 9 if mode == 0 else 3
    at = NP * (NP + 1) // 2 + NP
    trace, done, status, cost0 = [], 0, 0, 0.0
    for it in range(iters + 1):
        dirs = unit_directions() if mode == 0 else rotation_directions(H)
        sums = pass_sums(rows, k0, k1, H, dirs, scale_px, defect=defect)
        if it == 0:
            cost0 = sums[at]
        if it == iters:
            break
        A, g, M = damped(sums, NP, H if mode == 0 else None, defect)
        x = solve(A, g)
        new = apply_step(H, x, mode) if x is not None else None
        if new is None:
            status = 1
            break
        trace.append({"A": A, "g": g, "M": M, "delta": x, "sums": sums, "H": H, "rows": rows, "cams": (k0, k1), "dirs": dirs})
        H = new
        done += 1
    trace.append({"final": True, "sums": sums, "H": H, "rows": rows, "cams": (k0, k1)})
    pose = np.eye(4)
    moved = 0.0
    for c in range(9):
        e = H[c] - start[c]
        moved += e * e
    if mode == 0:
        moved = np.sqrt(moved)
        with np.errstate(all="ignore"):
            sg = hr.jacobi(H)[2]
            spread = sg[0] / sg[1] - sg[2] / sg[1]
    else:
        moved = 2.0 * np.arcsin(min(np.sqrt(moved) / 2.8284271247461903, 1.0)) * rr.DEG
        spread = 0.0
        pose[:3, :3] = H.reshape(3, 3)
    stats = np.array([cost0, sums[at], sums[at + 1], sums[at + 2], moved, spread, float(done), float(status)])
    return H, pose, stats, trace


def refine_step_bound(step, scale_px, mode):
    """What the state after ONE step may differ by between two float64 evaluations of the rule (the module's docstring) ->
    (bound on |delta - delta_ref|_2, bound on an entry of the state, cond_2(A))."""
    k0, k1 = step["cams"]
    NP = len(step["delta"])
    mags = pass_sums(step["rows"], k0, k1, step["H"], step["dirs"], scale_px, magnitude=True)
    rounds = -(-len(step["rows"]) // NT)
    rel = (TERM_OPS_H + rounds + 8 + 4) * E
    absM = damped(mags, NP)[2]
    absg = mags[NP * (NP + 1) // 2:NP * (NP + 1) // 2 + NP]
    dA = rel * np.sqrt((absM * absM).sum()) * (1.0 + 1e-3 + 1.0)          # the damping and the gauge scale M by less than 2
    dg = rel * np.sqrt((absg * absg).sum())
    sv = np.linalg.svd(step["A"], compute_uv=False)
    cond, inv = sv[0] / sv[-1], 1.0 / sv[-1]
    nd = np.sqrt((step["delta"] ** 2).sum())
    d_delta = inv * (dA * nd + dg) + chol_ops(NP) * E * cond * nd
    entry = 2.0 * d_delta + STATE_OPS * E if mode == 0 else d_delta + mr.POSE_OPS * E
    return d_delta, entry, cond


def rounding_tolerance(final, mode, coordinate=256.0):
    """The first-order bound of the module's docstring on the distance of the state from the truth that the fp32 rounding of exact
    matches allows; final: the trace's last entry at the truth (or near it), its sums taken with weights 1 at e = 0."""
    NP = 9 if mode == 0 else 3
    M = damped(final["sums"], NP)[2]
    lam = np.linalg.eigvalsh(M)
    smallest = lam[1] if mode == 0 else lam[0]                    # mode 0: the direction h itself carries no information
    n = final["sums"][NP * (NP + 1) // 2 + NP + 2]
    eps = 0.5 * float(np.spacing(np.float32(np.nextafter(np.float32(coordinate), np.float32(0.0)))))
    return 2.0 * eps * np.sqrt(n) / np.sqrt(smallest)


# --------------------------------------------------------------------------------------------------------------- the choice
def ln4n_table(N):
    """(N + 1): entry u = ln(4 u) as numpy computes it on the host, entry 0 is 0: the table the caller hands to cpn_model_gric."""
    t = np.zeros(N + 1)
    t[1:] = np.log(4.0 * np.arange(1, N + 1, dtype=np.float64))
    return t


def pick(gric, defect=None):
    """THE PICK among three gric values (+inf: out) -> (the smallest, the runner-up), -1 where there is none; a tie goes to the model
    with fewer parameters: the rotation, then the plane, then E.  defect="ties reversed"."""
    order = (2, 1, 0) if defect != "ties reversed" else (0, 1, 2)
    best = second = -1
    for m in order:
        if gric[m] < np.inf and (best < 0 or gric[m] < gric[best]):
            best = m
    for m in order:
        if m != best and gric[m] < np.inf and (second < 0 or gric[m] < gric[second]):
            second = m
    return best, second


def model_gric(xy, count, intrinsics, pose_e, H_plane, H_rot, avail, sigma_px=0.5, defect=None):
    """The rule of cpn_model_gric for ONE pair -> (gric (3), label (N) uint8, stats (7), info): info holds `x` (3, n_rows) the
    e^2 / sigma^2 of the usable rows (NaN where the residual does not count), `bound` (3) gric_bound, `cap_margin` the smallest
    |x - cap| of a model that is in.  defect: "caps swapped" (2 (4 - d) with the two values of d exchanged), "k swapped" (the
    plane's and the rotation's parameter counts), "cap inclusive" (x <= cap), "wave order", "ties reversed"."""
    xy32 = np.asarray(xy, dtype=np.float32)
    N = len(xy32)
    n = min(max(int(count), 0), N)
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    P = np.asarray(pose_e, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        models = [mr.essential(P[:3, :3], P[:3, 3]).reshape(9), np.asarray(H_plane, dtype=np.float64).reshape(9),
                  np.asarray(H_rot, dtype=np.float64).reshape(9)]
    inn = [bool(avail[m]) and bool(np.isfinite(models[m]).all()) for m in range(3)]
    usable = np.isfinite(xy32[:n]).all(axis=1)
    rows = xy32[:n].astype(np.float64)
    a0, a1, b0, b1 = rr.normalised(rows, k0, k1)
    s2 = sigma_px * sigma_px
    caps = [2.0, 4.0, 4.0] if defect != "caps swapped" else [4.0, 2.0, 2.0]
    par = PAR if defect != "k swapped" else (5.0, 3.0, 8.0)
    with np.errstate(all="ignore"):
        se = mr.sampson(models[0].reshape(3, 3), k0, k1, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
        r, ok_e = mr.residual(se)
        sp = sampson_h(models[1], k0, k1, a0, a1, b0, b1)
        sr = sampson_h(models[2], k0, k1, a0, a1, b0, b1)
        e2 = [r * r, sp["e2"], sr["e2"]]
        counts = [ok_e, sp["ok"], sr["ok"]]
        cols, xs, label = [], [], np.zeros(N, dtype=np.uint8)
        below_all = []
        for m in range(3):
            x = e2[m] / s2
            below = usable & inn[m] & counts[m] & ((x <= caps[m]) if defect == "cap inclusive" else (x < caps[m]))
            cols.append(np.where(usable, np.where(below, x, caps[m]), 0.0))
            below_all.append(below)
            xs.append(np.where(usable & counts[m], x, np.nan))
            label[:n] |= (below.astype(np.uint8) << m).astype(np.uint8)
        cols += [b.astype(np.float64) for b in below_all] + [usable.astype(np.float64)]
        terms = np.stack(cols, 1) if n else np.zeros((0, 7))
    acc = block_sum_reversed(terms) if defect == "wave order" else mr.block_sum(terms)
    nu = acc[6]
    table = ln4n_table(N)
    gric, bound = np.full(3, np.inf), np.zeros(3)
    rounds = -(-n // NT)
    for m in range(3):
        if inn[m] and nu > 0.0:
            gric[m] = (acc[m] + (LN4 * DIM[m]) * nu) + table[int(nu)] * par[m]
            bound[m] = (RHO_OPS + rounds + 8 + 4) * E * gric[m]
    best, second = pick(gric, defect)
    stats = np.zeros(7)
    stats[0], stats[1] = float(best), nu
    for m in range(3):
        stats[2 + m] = acc[3 + m] if (nu > 0.0 and inn[m]) else 0.0
    stats[5] = gric[second] - gric[best] if (best >= 0 and second >= 0) else np.inf
    stats[6] = (0.0 if any(inn) else 1.0) if nu > 0.0 else 2.0
    margins = [np.abs(xs[m][np.isfinite(xs[m])] - caps[m]) for m in range(3) if inn[m]]
    margins = np.concatenate(margins) if margins else np.zeros(0)
    info = {"x": xs, "bound": bound, "cap_margin": float(margins.min()) if len(margins) else np.inf, "in": inn, "sums": acc}
    return gric, label, stats, info


# ------------------------------------------------------------------------------------------------------------ the whole call
def one_slot_finish(H, xy, count, intrinsics, inlier_px, rel_pose):
    """cpn_ransac_score_h and cpn_ransac_finish_h on ONE slot, H (9), with a valid byte of 1 -> homography_ref.finish's tuple."""
    Hm, valid = np.asarray(H, dtype=np.float64).reshape(1, 9), np.ones(1, dtype=np.uint8)
    partial = hr.score(Hm, valid, xy, count, intrinsics, inlier_px)
    return hr.finish(Hm, valid, partial, xy, count, intrinsics, inlier_px, rel_pose, 0.0)


def select_pose(xy, count, intrinsics, rel_pose=None, hypotheses_n=1024, inlier_px=1.0, seed=0, sigma_px=0.5, iters=10,
                scale_px=2.0, producers=None):
    """The rule of coponerf_amd.matches.select_pose for ONE pair with the 8-point solver -> dict: pose (4, 4) float64 before the
    fp32 store, model, gric, label, stats, avail, info (model_gric's) and `producers`, everything before model_gric (hand it back
    in to score the same producers at another sigma_px)."""
    if producers is None:
        e_pose, _, e_stats, _ = rr.ransac_pose(xy, count, intrinsics, rel_pose, hypotheses_n, inlier_px, seed)
        r_pose, r_stats, _ = mr.refine_pose(xy, count, intrinsics, e_pose.astype(np.float32), iters, scale_px)
        h_pose, _, h_H, _, h_stats, _ = hr.homography_pose(xy, count, intrinsics, rel_pose, hypotheses_n, inlier_px, seed, 0.0)
        p_H, _, p_stats, _ = refine_homography(xy, count, intrinsics, h_H, 0, iters, scale_px)
        t_H, t_pose, t_stats, _ = refine_homography(xy, count, intrinsics, h_H, 1, iters, scale_px)
        f_pose, f_twin, f_H, f_inl, f_stats, _ = one_slot_finish(p_H, xy, count, intrinsics, inlier_px, rel_pose)
        h_ok = h_stats[11] in (0.0, 3.0)
        avail = np.array([e_stats[7] == 0 and r_stats[7] <= 1, h_ok and p_stats[7] <= 1 and f_stats[11] == 0,
                          h_ok and t_stats[7] <= 1], dtype=np.uint8)
        producers = dict(ransac_pose=e_pose, ransac_stats=e_stats, refined_pose=r_pose, refined_stats=r_stats, homography_pose=h_pose,
                         homography_H=h_H, homography_stats=h_stats, plane_H=p_H, plane_stats=p_stats, rotation_H=t_H,
                         rotation_pose=t_pose, rotation_stats=t_stats, finish_pose=f_pose, finish_twin=f_twin, finish_H=f_H,
                         finish_inlier=f_inl, finish_stats=f_stats, avail=avail)
    pr = producers
    gric, label, stats, info = model_gric(xy, count, intrinsics, pr["refined_pose"].astype(np.float32), pr["plane_H"], pr["rotation_H"],
                                          pr["avail"], sigma_px)
    model = int(stats[0])
    none = np.eye(4) if rel_pose is None else np.asarray(rel_pose, dtype=np.float32).astype(np.float64)
    pose = (pr["refined_pose"], pr["finish_pose"], pr["rotation_pose"], none)[model]
    return dict(pose=pose, model=model, gric=gric, label=label, stats=stats, avail=pr["avail"], info=info, producers=pr)


@functools.lru_cache(maxsize=None)
def scene_selection(name, hypotheses_n=256, seed=0):
    """select_pose's producers on one of homography_ref.scenes(), with the scene's truth as rel_pose (the rotation scene has none).
    Computed once per process, shared, never written to."""
    sc = dict(hr.scenes())[name]
    rel = rr.true_pose(sc) if name != "rotation" else None
    return sc, rel, select_pose(sc["xy"], 1000, sc["intrinsics"], rel, hypotheses_n, 1.0, seed)


EXPECTED = {"wall": 1, "curved": 0, "rotation": 2}


def unrefined_pick(sc, rel, pr, sigma_px):
    """What GRIC picks on the RANSAC winners as they are: ransac_pose's pose, homography_pose's H and the rotation nearest to it."""
    with np.errstate(all="ignore"):
        Rn = nearest_rotation(pr["homography_H"])
    avail = np.array([pr["ransac_stats"][7] == 0, pr["homography_stats"][11] in (0.0, 3.0), pr["homography_stats"][11] in (0.0, 3.0)],
                     dtype=np.uint8)
    gric, _, stats, _ = model_gric(sc["xy"], 1000, sc["intrinsics"], pr["ransac_pose"].astype(np.float32), pr["homography_H"], Rn, avail,
                                   sigma_px)
    return int(stats[0]), gric


def wall_truth():
    """The wall's true homography as a unit h with det > 0: H = R + t n1^T / d1 for the plane n . X0 = 3 seen from view 1."""
    from tests import ransac5_ref as r5
    sc = r5.wall_scene(**r5.WALL)
    nrm = np.array([0.25, -0.1, 1.0])
    R, t = sc["R_true"], sc["t_true"]
    H = R + np.outer(t, R.T @ nrm) / (3.0 - nrm @ t)
    h = H.reshape(9) / np.linalg.norm(H)
    return h if np.linalg.det(H) > 0 else -h
