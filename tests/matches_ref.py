"""Yardsticks of coponerf_amd/matches.py (csrc/matches.hip) and the inputs of its tests: numpy restatements of the three rules of
include/coponerf_hip.h (round 16) and the synthetic scenes.  tests/test_matches_ref.py holds them to independent forms on the CPU.

The match fields have two layers, as tests/summaries_ref.py's panels have.  Everything that SELECTS - the source index and the
weights of F.interpolate, the sampling coordinate of `warp`, its floor - is restated in single fp32 operations in the kernel's
order (numpy float32 arithmetic is IEEE, one rounding per operation, which is what -ffp-contract=off gives the kernel).  Every
VALUE is then formed in float64 from those fp32 weights, in the kernel's order.

Bounds (U = 2^-24, E = 2^-53), from operation counts, none from a run:
  q             |kernel - float64| <= UP_OPS U M_u + U |q|.  u = ((ly0 (lx0 a + lx1 b)) + (ly1 (lx0 c + lx1 d))) s carries a
                product and a sum along x, a product and a sum along y and the scale: 5 roundings relative to M_u, the same
                expression on the absolute taps; UP_OPS = 6 leaves room for the second order.  p + u rounds once more.
  cycle         the error e = u + sum_k o_k wt_k per axis: the bound of u, the bounds of the four tap values weighted by wt_k,
                TAP_OPS U sum_k |o_k wt_k| (two differences and a product in wt_k, the product with o_k, the sums: 8, TAP_OPS
                = 9) and U |e|; cycle = sqrt(e_x^2 + e_y^2) moves by at most the sum of the two and carries two products, a
                sum and a root of its own: 3 U cycle.
  epi           float64 on both sides and one rounding to fp32: ulp32(|ref|) / 2 + E (N_OPS M_n / sqrt(D) + D_OPS |ref|).  The
                longest path into n is 2 (a normalised coordinate) + 3 (an entry of E) + 4 (E b) + 4 (a . E b) = 13
                operations, N_OPS = 14, relative to M_n, the same expression on absolute values; D is a sum of squares of
                such values, divided and rooted: D_OPS = 16.  Compared on the q the kernel itself wrote: epi is defined on the
                fp32 match.
  inside, mask  equal wherever no decision lies within BAND = 1e-3 px of its threshold (tests/summaries_ref.py's band); the
                tests count the pixels in the band and hold their share to BAND_SHARE = 0.5 %.
  compaction    bytes.
  one step      refine_step_bound: |delta - delta_ref|_2 <= |A^-1|_2 (|dA|_F |delta|_2 + |dg|_2) + CHOL_OPS E cond_2(A)
                |delta|_2, the first-order perturbation bound of a linear system and the backward error of a 6 x 6 Cholesky
                solve (CHOL_OPS = 6 . 6 . 4).  dA and dg are (TERM_OPS + the depth of the sum + 4) E times the sums of the
                absolute terms of H and g: a term w J_j J_k is at most TERM_OPS = 96 operations deep (13 into n, 16 into D,
                as many again into dn and dD, the quotient forms of J, the weight), each relative to the absolute form of the
                term; the sum is rounds + 6 + 2 additions deep.  An entry of the pose then differs by at most that (a rotation
                by delta moves an entry of R by at most |delta|, and |t0| times it for the translation), POSE_OPS = 64 E for
                Rodrigues, its sine and cosine and the two products, and half an fp32 ulp of the store.
"""
import functools

import numpy as np

U = 2.0 ** -24
E = 2.0 ** -53
BAND = 1e-3
BAND_SHARE = 0.005
UP_OPS = 6
TAP_OPS = 9
N_OPS = 14
D_OPS = 16
TERM_OPS = 96
CHOL_OPS = 6 * 6 * 4
POSE_OPS = 64
NT = 256
F32 = np.float32


def half_ulp32(x):
    return 0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ match fields
def up_index(S, h):
    """ATen's area_pixel_compute_source_index(align_corners=False) in fp32 -> (i0, i1, l0, l1) of the S output positions."""
    rs = F32(h) / F32(S)
    src = rs * (np.arange(S, dtype=F32) + F32(0.5)) - F32(0.5)
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int64), h - 1)
    i1 = i0 + (i0 < h - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def upsample(flow, S, dtype):
    """(S / h) . F.interpolate(flow (B, 2, h, h), S, mode="bilinear") with the fp32 weights of up_index, the values in `dtype`
    (np.float32: the kernel's own sequence bit for bit; np.float64: the yardstick)."""
    h = flow.shape[2]
    i0, i1, l0, l1 = up_index(S, h)
    f = flow.astype(dtype)
    ya, yb, xa, xb = i0[:, None], i1[:, None], i0[None, :], i1[None, :]
    ly0, ly1, lx0, lx1 = (w.astype(dtype) for w in (l0[:, None], l1[:, None], l0[None, :], l1[None, :]))
    up = ly0 * (lx0 * f[:, :, ya, xa] + lx1 * f[:, :, ya, xb]) + ly1 * (lx0 * f[:, :, yb, xa] + lx1 * f[:, :, yb, xb])
    return (up * dtype(F32(S / h))).astype(dtype)


def warp_coord32(up32):
    """utils.warp's normalisation of p + u and grid_sample's unnormalisation, in fp32 -> (ix, iy) (B, S, S)."""
    S = up32.shape[-1]
    gx = np.arange(S, dtype=F32)[None, None, :]
    gy = np.arange(S, dtype=F32)[None, :, None]
    den = F32(max(S - 1, 1))
    out = []
    for g, u in ((gx, up32[:, 0]), (gy, up32[:, 1])):
        v = (g + u).astype(F32)
        n = (F32(2) * v / den - F32(1)).astype(F32)
        out.append((((n + F32(1)) * F32(S) - F32(1)) / F32(2)).astype(F32))
    return out


def cam_of(K44):
    K44 = np.asarray(K44, dtype=np.float32).astype(np.float64)
    return K44[0, 0], K44[1, 1], K44[0, 2], K44[1, 2]


def essential(R, t):
    """E = [t]x R, every entry one difference of two products."""
    Em = np.empty((3, 3))
    for j in range(3):
        Em[0, j] = t[1] * R[2, j] - t[2] * R[1, j]
        Em[1, j] = t[2] * R[0, j] - t[0] * R[2, j]
        Em[2, j] = t[0] * R[1, j] - t[1] * R[0, j]
    return Em


def essential_abs(R, t):
    R, t = np.abs(R), np.abs(t)
    Em = np.empty((3, 3))
    for j in range(3):
        Em[0, j] = t[1] * R[2, j] + t[2] * R[1, j]
        Em[1, j] = t[2] * R[0, j] + t[0] * R[2, j]
        Em[2, j] = t[0] * R[1, j] + t[1] * R[0, j]
    return Em


def sampson(Em, k0, k1, x0, y0, x1, y1, magnitude=False):
    """The pieces of the Sampson residual of the pixel pairs, in the header's operation order -> dict of a0, a1, b0, b1, g (4
    arrays), n, D.  magnitude=True: the same expression on absolute values (Em must be essential_abs's), for the bounds."""
    sub = (lambda p, c: np.abs(p) + np.abs(c)) if magnitude else (lambda p, c: p - c)
    a0, a1 = sub(x0, k0[2]) / k0[0], sub(y0, k0[3]) / k0[1]
    b0, b1 = sub(x1, k1[2]) / k1[0], sub(y1, k1[3]) / k1[1]
    eb = [(Em[i, 0] * b0 + Em[i, 1] * b1) + Em[i, 2] for i in range(3)]
    ea = [(Em[0, j] * a0 + Em[1, j] * a1) + Em[2, j] for j in range(2)]
    n = (a0 * eb[0] + a1 * eb[1]) + eb[2]
    g = [eb[0] / k0[0], eb[1] / k0[1], ea[0] / k1[0], ea[1] / k1[1]]
    D = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) + g[3] * g[3]
    return {"a0": a0, "a1": a1, "b0": b0, "b1": b1, "g": g, "n": n, "D": D}


def residual(s):
    """(r = n / sqrt(D), whether it counts) of sampson()'s pieces."""
    with np.errstate(all="ignore"):
        r = s["n"] / np.sqrt(s["D"])
        ok = (s["D"] > 0) & np.isfinite(s["D"]) & np.isfinite(s["n"]) & np.isfinite(r)
    return r, ok


def epi_field(q, intrinsics, rel_pose, defect=None):
    """q (2, B, S, S, 2) fp32: the matches a kernel or match_fields() wrote -> (epi (2, B, S, S) float64 with NaN where the
    residual does not count, bound (2, B, S, S)).  defect="swapped direction": direction 1 pairs (p, q) instead of (q, p)."""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    _, B, S, _, _ = q.shape
    P = np.asarray(rel_pose, dtype=np.float32).astype(np.float64)
    px = np.broadcast_to(np.arange(S, dtype=np.float64)[None, :], (S, S))
    py = np.broadcast_to(np.arange(S, dtype=np.float64)[:, None], (S, S))
    epi, bound = np.full((2, B, S, S), np.nan), np.zeros((2, B, S, S))
    for b in range(B):
        k0, k1 = cam_of(intrinsics[b][0]), cam_of(intrinsics[b][1])
        Em, Ea = essential(P[b, :3, :3], P[b, :3, 3]), essential_abs(P[b, :3, :3], P[b, :3, 3])
        for d in range(2):
            pair = (px, py, q[d, b, ..., 0], q[d, b, ..., 1])
            if d == 1 and defect != "swapped direction":
                pair = pair[2:] + pair[:2]
            with np.errstate(all="ignore"):
                s, m = sampson(Em, k0, k1, *pair), sampson(Ea, k0, k1, *pair, magnitude=True)
                r, ok = residual(s)
                epi[d, b] = np.where(ok, r, np.nan)
                bound[d, b] = np.where(ok, half_ulp32(np.where(ok, r, 0.0)) + E * (N_OPS * m["n"] / np.sqrt(s["D"]) + D_OPS * np.abs(r)), 0.0)
    return epi, bound


def match_fields(f0, f1, intrinsics, rel_pose, S, defect=None):
    """The rule of cpn_match_fields.  f0, f1 (B, 2, h, h) fp32 -> a dict of (2, B, ...) arrays:
      q (.., S, S, 2) float64 and q_bound; q32 (.., S, S, 2) fp32: the kernel's own sequence, bit for bit;
      cycle (.., S, S) float64 (NaN or inf where the kernel's is not finite) and cycle_bound;
      epi, epi_bound: epi_field of q32;  inside (.., S, S) bool, decided on q;
      margin (.., S, S): the smallest distance in pixels of the decisions `inside` and `cycle <= 10` from their thresholds.
    defect="tap outside": a tap outside the image reads the nearest pixel inside instead of contributing 0."""
    fl = (np.asarray(f0, dtype=np.float32), np.asarray(f1, dtype=np.float32))
    B = fl[0].shape[0]
    with np.errstate(all="ignore"):
        up32 = [upsample(f, S, np.float32) for f in fl]
        up64 = [upsample(f, S, np.float64) for f in fl]
        mag = [upsample(np.abs(f), S, np.float64) for f in fl]
    grid = np.stack(np.broadcast_arrays(np.arange(S, dtype=np.float64)[None, :], np.arange(S, dtype=np.float64)[:, None]))     # (2, S, S): x, y
    out = {k: [] for k in ("q", "q_bound", "q32", "cycle", "cycle_bound", "inside", "margin")}
    bidx = np.arange(B)[:, None, None]
    for d in range(2):
        own, oth = up64[d], up64[1 - d]
        with np.errstate(all="ignore"):
            b_own = UP_OPS * U * mag[d]                                              # (B, 2, S, S)
            b_oth = UP_OPS * U * mag[1 - d]
            q = own + grid[None]
            q32 = (up32[d] + grid[None].astype(F32)).astype(F32)
            out["q"].append(np.moveaxis(q, 1, -1))
            out["q_bound"].append(np.moveaxis(b_own + U * np.abs(q), 1, -1))
            out["q32"].append(np.moveaxis(q32, 1, -1))
            ix, iy = warp_coord32(up32[d])
            fx0, fy0 = np.floor(ix), np.floor(iy)
            fx1, fy1 = fx0 + F32(1), fy0 + F32(1)
            hi = F32(S - 1)
            wx = ((fx1.astype(np.float64) - ix, ix - fx0.astype(np.float64)))
            wy = ((fy1.astype(np.float64) - iy, iy - fy0.astype(np.float64)))
            tapx, tapy = (fx0, fx1), (fy0, fy1)
            c = np.zeros((B, 2, S, S))
            c_abs, c_bound = np.zeros((B, 2, S, S)), np.zeros((B, 2, S, S))
            for ky, kx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                okx, oky = (tapx[kx] >= 0) & (tapx[kx] <= hi), (tapy[ky] >= 0) & (tapy[ky] <= hi)
                ok = okx & oky
                tx = np.where(okx, tapx[kx], 0).astype(np.int64)
                ty = np.where(oky, tapy[ky], 0).astype(np.int64)
                if defect == "tap outside":
                    near = np.isfinite(ix) & np.isfinite(iy)
                    tx = np.where(near, np.clip(np.where(near, tapx[kx], 0), 0, S - 1), 0).astype(np.int64)
                    ty = np.where(near, np.clip(np.where(near, tapy[ky], 0), 0, S - 1), 0).astype(np.int64)
                    ok = near
                wt = wx[kx] * wy[ky]
                for a in range(2):
                    o = oth[bidx, a, ty, tx]
                    term = np.where(ok, o * wt, 0.0)
                    c[:, a] = c[:, a] + term
                    c_abs[:, a] += np.where(ok, np.abs(o * wt), 0.0)
                    c_bound[:, a] += np.where(ok, b_oth[bidx, a, ty, tx] * np.abs(wt), 0.0)
            e = own + c
            cycle = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
            be = b_own + c_bound + TAP_OPS * U * c_abs + U * np.abs(e)
            out["cycle"].append(cycle)
            out["cycle_bound"].append(be[:, 0] + be[:, 1] + 3 * U * cycle)
            inside = (q[:, 0] >= 0) & (q[:, 0] <= S - 1) & (q[:, 1] >= 0) & (q[:, 1] <= S - 1)
            out["inside"].append(inside)
            edge = np.minimum(np.abs(q), np.abs(q - (S - 1))).min(axis=1)
            margin = np.minimum(np.abs(cycle - 10.0), edge)
            out["margin"].append(np.where(np.isfinite(margin), margin, np.inf))       # a NaN decides nothing near a threshold
    out = {k: np.stack(v) for k, v in out.items()}
    out["epi"], out["epi_bound"] = epi_field(out["q32"], intrinsics, rel_pose)
    return out


def mask_of(ref):
    """(cycle <= 10) & inside of match_fields' dict, and the pixels whose decisions are at least BAND from their thresholds."""
    with np.errstate(invalid="ignore"):
        return (ref["cycle"] <= 10.0) & ref["inside"], ref["margin"] >= BAND


# -------------------------------------------------------------------------------------------------------------- compaction
def compact(keep, q, cycle, epi, defect=None):
    """keep (2, B, S, S) bytes, q (2, B, S, S, 2), cycle, epi (2, B, S, S) fp32 -> (xy: list of (n_b, 4) fp32, err: list of
    (n_b, 2) fp32, counts (B) int32): the kept matches in (direction, row, column) order, view 0's point first.
    defect="order": the first kept match of every pair goes last."""
    keep = np.asarray(keep)
    _, B, S, _ = keep.shape
    py, px = np.divmod(np.arange(S * S), S)
    xys, errs, counts = [], [], []
    for b in range(B):
        rows_xy, rows_err = [], []
        for d in range(2):
            on = keep[d, b].reshape(-1) != 0
            p = np.stack((px[on], py[on]), 1).astype(np.float32)
            m = np.asarray(q[d, b], dtype=np.float32).reshape(-1, 2)[on]
            rows_xy.append(np.concatenate((p, m) if d == 0 else (m, p), 1))
            rows_err.append(np.stack((np.asarray(cycle[d, b], dtype=np.float32).reshape(-1)[on],
                                      np.asarray(epi[d, b], dtype=np.float32).reshape(-1)[on]), 1))
        xy, err = np.concatenate(rows_xy), np.concatenate(rows_err)
        if defect == "order" and len(xy) > 1:
            xy, err = np.roll(xy, -1, axis=0), np.roll(err, -1, axis=0)
        xys.append(np.ascontiguousarray(xy, dtype=np.float32))
        errs.append(np.ascontiguousarray(err, dtype=np.float32))
        counts.append(len(xy))
    return xys, errs, np.asarray(counts, dtype=np.int32)


def stride_keep(ref_mask, stride):
    """select()'s mask: ref_mask (2, B, S, S) bool and the pixels with x % stride == y % stride == stride // 2."""
    S = ref_mask.shape[-1]
    on = np.arange(S) % stride == stride // 2
    return ref_mask & (on[:, None] & on[None, :])


# -------------------------------------------------------------------------------------------------------------- refinement
def cross_rows(R, k):
    """[e_k]x R."""
    M = np.zeros((3, 3))
    k1, k2 = (k + 1) % 3, (k + 2) % 3
    M[k1], M[k2] = -R[k2], R[k1]
    return M


def block_sum(terms):
    """terms (n, V): the kernel's sum of V values over n matches by 256 threads: thread t adds t, t + 256, .. in ascending order
    from 0, the 64 lanes of a wave by the xor butterfly 32 .. 1, the four waves as (0 + 1) + (2 + 3)."""
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
    return (w[0] + w[1]) + (w[2] + w[3])


def pass_sums(xy, k0, k1, R, t, scale_px, defect=None, magnitude=False):
    """The 30 sums of one pass over the matches xy (n, 4) float64 at the state (R, t): H (21, upper triangle by rows), g (6),
    the cost, the sum of weights, the matches that count.  defect="dropped term": the Jacobian without its dD part.
    magnitude=True: the sums of the absolute forms of the terms of H and g (the other three as they are)."""
    x0, y0, x1, y1 = (xy[:, i] for i in range(4))
    with np.errstate(all="ignore"):
        s = sampson(essential(R, t), k0, k1, x0, y0, x1, y1)
        r, ok = residual(s)
        sd = np.sqrt(s["D"])
        m = sampson(essential_abs(R, t), k0, k1, x0, y0, x1, y1, magnitude=True) if magnitude else None
        J = []
        for k in range(6):
            Mk = cross_rows(R, k % 3)
            dE = essential(Mk, t) if k < 3 else Mk
            db = [(dE[i, 0] * s["b0"] + dE[i, 1] * s["b1"]) + dE[i, 2] for i in range(3)]
            da = [(dE[0, j] * s["a0"] + dE[1, j] * s["a1"]) + dE[2, j] for j in range(2)]
            dn = (s["a0"] * db[0] + s["a1"] * db[1]) + db[2]
            g = s["g"]
            dD = 2.0 * (((g[0] * (db[0] / k0[0]) + g[1] * (db[1] / k0[1])) + g[2] * (da[0] / k1[0])) + g[3] * (da[1] / k1[1]))
            if magnitude:
                dA = np.abs(essential_abs(Mk, t) if k < 3 else Mk)
                dbm = [(dA[i, 0] * m["b0"] + dA[i, 1] * m["b1"]) + dA[i, 2] for i in range(3)]
                dam = [(dA[0, j] * m["a0"] + dA[1, j] * m["a1"]) + dA[2, j] for j in range(2)]
                dnm = (m["a0"] * dbm[0] + m["a1"] * dbm[1]) + dbm[2]
                gm = m["g"]
                dDm = 2.0 * (((gm[0] * (dbm[0] / k0[0]) + gm[1] * (dbm[1] / k0[1])) + gm[2] * (dam[0] / k1[0])) + gm[3] * (dam[1] / k1[1]))
                J.append(dnm / sd + (m["n"] * dDm) / ((2.0 * s["D"]) * sd))
            elif defect == "dropped term":
                J.append(dn / sd)
            else:
                J.append(dn / sd - (s["n"] * dD) / ((2.0 * s["D"]) * sd))
        z = r / scale_px
        u = 1.0 + z * z
        w = 1.0 / (u * u)
        rr = m["n"] / sd if magnitude else r
        cols = []
        for j in range(6):
            wj = w * J[j]
            cols += [wj * J[k] for k in range(j, 6)]
        cols += [(w * J[j]) * rr for j in range(6)]
        cols += [((r * r) / 2.0) / u, w, np.ones_like(r)]
        terms = np.stack(cols, 1)                                   # (n, 30)
        terms = np.where(ok[:, None], terms, 0.0)
    return block_sum(terms)


def damped(sums, t):
    """(A, g, H) of a pass: H the symmetric matrix of the sums, A = H with A_jj = H_jj + 1e-3 H_jj and the translation block
    += (tr H / 6) t t^T."""
    H = np.zeros((6, 6))
    at = 0
    for j in range(6):
        for k in range(j, 6):
            H[j, k] = H[k, j] = sums[at]
            at += 1
    g = sums[21:27].copy()
    A = H.copy()
    trace = 0.0
    for j in range(6):
        trace += H[j, j]
    for j in range(6):
        A[j, j] = H[j, j] + 1e-3 * H[j, j]
    pin = trace / 6.0
    for i in range(3):
        for j in range(3):
            A[3 + i, 3 + j] = A[3 + i, 3 + j] + pin * (t[i] * t[j])
    return A, g, H


def solve6(A, g):
    """delta = -A^-1 g by the kernel's Cholesky, or None where a pivot is not positive or a value not finite."""
    L = A.copy()
    with np.errstate(all="ignore"):
        for j in range(6):
            s = L[j, j]
            for k in range(j):
                s -= L[j, k] * L[j, k]
            if not (s > 0.0) or not np.isfinite(s):
                return None
            l = np.sqrt(s)
            L[j, j] = l
            for i in range(j + 1, 6):
                v = L[i, j]
                for k in range(j):
                    v -= L[i, k] * L[j, k]
                L[i, j] = v / l
        y, x = np.zeros(6), np.zeros(6)
        for i in range(6):
            v = -g[i]
            for k in range(i):
                v -= L[i, k] * y[k]
            y[i] = v / L[i, i]
        for i in range(5, -1, -1):
            v = y[i]
            for k in range(i + 1, 6):
                v -= L[k, i] * x[k]
            x[i] = v / L[i, i]
    return x if np.isfinite(x).all() else None


def apply_step(R, t, x):
    """R <- exp([w]x) R by Rodrigues (the identity below 1e-12), t <- (t + dt) / |t + dt|; None where the result is not finite."""
    th = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    Q = np.eye(3)
    if th >= 1e-12:
        k = x[:3] / th
        s, c = np.sin(th), 1.0 - np.cos(th)
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        for i in range(3):
            for j in range(3):
                kk = (K[i, 0] * K[0, j] + K[i, 1] * K[1, j]) + K[i, 2] * K[2, j]
                Q[i, j] = (Q[i, j] + s * K[i, j]) + c * kk
    Rn = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (Q[i, 0] * R[0, j] + Q[i, 1] * R[1, j]) + Q[i, 2] * R[2, j]
    tn = t + x[3:]
    ln = np.sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2])
    if not (ln > 0.0) or not np.isfinite(ln) or not np.isfinite(Rn).all():
        return None
    return Rn, tn / ln


def refine_pose(xy, count, intrinsics, rel_pose, iters, scale_px, defect=None):
    """The rule of cpn_refine_pose for ONE pair: xy (N, 4) fp32, count, intrinsics (2, 4, 4), rel_pose (4, 4) fp32 ->
    (pose (4, 4) float64 before the fp32 store, stats (8), trace): trace is a list with, per solved pass, the dict of A, g, H,
    delta, sums and the state (R, t) it was formed at - what refine_step_bound reads - and last the sums and the state of the
    pass that only measured."""
    P32 = np.asarray(rel_pose, dtype=np.float32)
    P = P32.astype(np.float64)
    xy = np.asarray(xy, dtype=np.float32).astype(np.float64)
    n = min(max(int(count), 0), len(xy))
    R, t0 = P[:3, :3].copy(), P[:3, 3].copy()
    with np.errstate(all="ignore"):
        len0 = np.sqrt((t0[0] * t0[0] + t0[1] * t0[1]) + t0[2] * t0[2])
    if not (np.isfinite(R).all() and np.isfinite(t0).all() and len0 > 0.0 and np.isfinite(len0) and n > 0 and iters > 0):
        return P.copy(), np.array([0.0] * 7 + [2.0]), []
    k0, k1 = cam_of(intrinsics[0]), cam_of(intrinsics[1])
    t = t0 / len0
    trace, done, status, cost0 = [], 0, 0, 0.0
    rows = xy[:n]
    for it in range(iters + 1):
        sums = pass_sums(rows, k0, k1, R, t, scale_px, defect=defect)
        if it == 0:
            cost0 = sums[27]
        if it == iters:
            break
        A, g, H = damped(sums, t)
        x = solve6(A, g)
        new = apply_step(R, t, x) if x is not None else None
        if new is None:
            status = 1
            break
        trace.append({"A": A, "g": g, "H": H, "delta": x, "sums": sums, "R": R, "t": t, "rows": rows, "cams": (k0, k1)})
        R, t = new
        done += 1
    trace.append({"final": True, "sums": sums, "R": R, "t": t, "rows": rows, "cams": (k0, k1)})
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, len0 * t
    dR = np.sqrt(((R - P[:3, :3]) ** 2).sum())
    dt = np.sqrt(((t - P[:3, 3] / len0) ** 2).sum())
    stats = np.array([cost0, sums[27], sums[28], sums[29], np.degrees(2.0 * np.arcsin(min(dR / (2.0 * np.sqrt(2.0)), 1.0))),
                      np.degrees(2.0 * np.arcsin(min(dt / 2.0, 1.0))), float(done), float(status)])
    return pose, stats, trace


def refine_step_bound(step, scale_px, len0):
    """What an entry of the pose after ONE step may differ by between two float64 evaluations of the rule (the module's
    docstring): -> (bound on |delta - delta_ref|_2, bound on a rotation entry, bound on a translation entry, cond_2(A)), the
    fp32 store's half ulp not included."""
    k0, k1 = step["cams"]
    mags = pass_sums(step["rows"], k0, k1, step["R"], step["t"], scale_px, magnitude=True)
    rounds = -(-len(step["rows"]) // NT)
    rel = (TERM_OPS + rounds + 8 + 4) * E
    absH, absg = damped(mags, np.zeros(3))[2], mags[21:27]
    dA = rel * np.sqrt((absH * absH).sum()) * (1.0 + 1e-3 + 0.5)          # the damping and the gauge scale H by less than 1.5
    dg = rel * np.sqrt((absg * absg).sum())
    sv = np.linalg.svd(step["A"], compute_uv=False)
    cond, inv = sv[0] / sv[-1], 1.0 / sv[-1]
    nd = np.sqrt((step["delta"] ** 2).sum())
    d_delta = inv * (dA * nd + dg) + CHOL_OPS * E * cond * nd
    return d_delta, d_delta + POSE_OPS * E, (d_delta + POSE_OPS * E) * len0, cond


# ------------------------------------------------------------------------------------------------------------- the scenes
def rodrigues(axis, deg):
    axis = np.asarray(axis, dtype=np.float64)
    k = axis / np.linalg.norm(axis)
    th = np.radians(deg)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def rotation_angle_deg(Ra, Rb):
    """The geodesic angle between two rotations, exact down to the smallest angles: |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2)."""
    return float(np.degrees(2.0 * np.arcsin(min(np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0)), 1.0))))


def direction_angle_deg(ta, tb):
    ta, tb = ta / np.linalg.norm(ta), tb / np.linalg.norm(tb)
    return float(np.degrees(2.0 * np.arcsin(min(np.linalg.norm(ta - tb) / 2.0, 1.0))))


def pinhole(f, S):
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = f
    K[0, 2] = K[1, 2] = S / 2.0
    return K


@functools.lru_cache(maxsize=None)
def refine_scene(n=1000, seed=16, noise_px=0.0, outliers=0.0):
    """Random points at depths 1 - 6 seen by two cameras of f = 200 px in 256 x 256 images, the coordinates rounded to fp32, and
    a start 5 degrees off in rotation and 17 degrees off in the translation's direction.  noise_px: gaussian noise on view 1's
    points; outliers: that share of view 1's points replaced by uniformly random ones.  Returns a dict: xy (n, 4) fp32,
    intrinsics (2, 4, 4) fp32, rel_pose (4, 4) fp32 (the start), R_true, t_true.  Computed once, shared, never written to."""
    rng = np.random.default_rng(seed)
    S, f = 256, 200.0
    R_true = rodrigues((0.3, 1.0, -0.2), 12.0)
    t_true = np.array([0.55, 0.08, 0.21])
    p0 = rng.uniform(0.0, S, size=(n, 2))
    depth = rng.uniform(1.0, 6.0, size=n)
    X0 = np.concatenate(((p0 - S / 2.0) / f, np.ones((n, 1))), 1) * depth[:, None]
    X1 = (X0 - t_true) @ R_true                                     # X0 = R X1 + t  ->  X1 = R^T (X0 - t)
    p1 = f * X1[:, :2] / X1[:, 2:] + S / 2.0
    if noise_px:
        p1 = p1 + rng.normal(scale=noise_px, size=p1.shape)
    if outliers:
        bad = rng.random(n) < outliers
        p1[bad] = rng.uniform(0.0, S, size=(int(bad.sum()), 2))
    R_start = rodrigues((1.0, -0.5, 0.7), 5.0) @ R_true
    perp = np.cross(t_true, (0.0, 0.0, 1.0))
    t_start = rodrigues(perp, 17.0) @ t_true
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R_start, t_start
    K = pinhole(f, S)
    return {"xy": np.concatenate((p0, p1), 1).astype(np.float32), "intrinsics": np.stack((K, K)), "rel_pose": pose.astype(np.float32),
            "R_true": R_true, "t_true": t_true}


def pose_errors(pose, scene):
    """(rotation error, translation-direction error) in degrees of a (4, 4) pose against the scene's truth."""
    pose = np.asarray(pose, dtype=np.float64)
    return rotation_angle_deg(pose[:3, :3], scene["R_true"]), direction_angle_deg(pose[:3, 3], scene["t_true"])


@functools.lru_cache(maxsize=None)
def fields_case(B, S, h, nan=True):
    """Two flows of a smooth warp and its approximate inverse on an S x S grid with h x h flows: view 1 is view 0 turned,
    stretched and shifted so that part of the matches leave the image, the inverse is off by a ramp that crosses the 10 pixel
    threshold inside the image, and (nan=True) one flow entry is NaN.  Returns (f0, f1 (B, 2, h, h) fp32, intrinsics
    (B, 2, 4, 4) fp32, rel_pose (B, 4, 4) fp32).  Computed once, shared, never written to."""
    s = S / h
    c = (np.arange(h) + 0.5) * s - 0.5                              # the cells' centres on the S grid
    x, y = np.meshgrid(c, c)
    f0, f1, Ks, Ps = [], [], [], []
    for b in range(B):
        ang = np.radians(4.0 + 3.0 * b)
        A = (1.05 + 0.03 * b) * np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        shift = np.array([0.17 * S + 0.02 * S * b, -0.11 * S])
        mid = (S - 1) / 2.0
        wob = 0.02 * S
        fx = A[0, 0] * (x - mid) + A[0, 1] * (y - mid) + mid + shift[0] + wob * np.sin(2 * np.pi * y / S) - x
        fy = A[1, 0] * (x - mid) + A[1, 1] * (y - mid) + mid + shift[1] + wob * np.cos(2 * np.pi * x / S) - y
        Ai = np.linalg.inv(A)
        ramp = 22.0 * (x / S) ** 2 + 1.3                            # pixels of forward-backward disagreement, 1.3 .. 23
        gx = Ai[0, 0] * (x - mid - shift[0]) + Ai[0, 1] * (y - mid - shift[1]) + mid - x + ramp
        gy = Ai[1, 0] * (x - mid - shift[0]) + Ai[1, 1] * (y - mid - shift[1]) + mid - y - 0.4 * ramp
        f0.append(np.stack((fx, fy)) / s)
        f1.append(np.stack((gx, gy)) / s)
        K0, K1 = pinhole(0.8 * S + 3 * b, S), pinhole(0.9 * S, S)
        K1[0, 2] += 1.5
        K1[1, 1] *= 1.02
        Ks.append(np.stack((K0, K1)))
        P = np.eye(4)
        P[:3, :3] = rodrigues((0.2, 1.0, 0.1), 9.0 + 2 * b)
        P[:3, 3] = (0.4, -0.05 * (b + 1), 0.12)
        Ps.append(P)
    f0, f1 = np.asarray(f0, dtype=np.float32), np.asarray(f1, dtype=np.float32)
    if nan:
        f0[B - 1, 1, h // 3, h // 2] = np.nan
    return f0, f1, np.asarray(Ks, dtype=np.float32), np.asarray(Ps, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def fields_ref(B, S, h, nan=True):
    """match_fields of fields_case(B, S, h): computed once per process, shared, never written to."""
    f0, f1, K, P = fields_case(B, S, h, nan)
    return match_fields(f0, f1, K, P, S)
