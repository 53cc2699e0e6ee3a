"""Yardstick of coponerf_amd.matches.ransac_pose(solver="5pt") (csrc/ransac5.hip): a numpy restatement, for ONE pair and vectorised
over the samples, of the rule of cpn_ransac_hypotheses5 in include/coponerf_hip.h (round 21), in the header's operation sequence;
an INDEPENDENT 5-point solver (library SVD, dictionary polynomials, the eigenvectors of the 10 x 10 action matrix) to pin it
against; and the planar scene that the 8-point solver cannot do.  tests/test_ransac5_ref.py holds the restatement to its
definition and to the independent solver on the CPU; tests/test_gpu_ransac5.py compares the kernel with it.  The score and the
finish are tests/ransac_ref.py's, fed with 10 slots per sample.

numpy float64 arithmetic is IEEE with one rounding per operation, which is what -ffp-contract=off gives the kernel, and every
expression below is written in the kernel's order: only + - * / sqrt and comparisons, fixed trip counts.

Bounds (E = 2^-53), from operation counts, none from a run:
  the samples   |a_j^T E b_j| <= SAMPLE_OPS E kappa_5 |a_j| |b_j| with SAMPLE_OPS = 2000: E is a combination of four null
                vectors of the 5 x 9 system, each from 5 elimination steps of at most 5 x 9 updates of two operations and a back
                substitution of 5 rows of at most 8 terms (under 600 operations), combined with 7 more and normalised with 28;
                kappa_5 = sigma_1 / sigma_5 of the system is the conditioning of its null space.  It does not depend on the
                roots: any x, y, z give a vector of the null space.
  the cubics    |det E| and |2 E E^T E - tr(E E^T) E|_max of a unit E <= CUBIC_OPS E kappa_10 kappa_root: the 10 x 20
                coefficients cost under 400 operations each, the Gauss-Jordan elimination 10 steps of 20 columns, the 3 x 3
                determinant in z under 700, the Sturm chain and the Newton steps under 600 - CUBIC_OPS = 4000 -, kappa_10 is
                the condition number of the 10 x 10 block that is eliminated, and kappa_root = max(1, max |f| / (|z f'|)) at
                the root - the conditioning of a root of the degree-10 polynomial f - is measured per root.
"""
import functools
import itertools

import numpy as np

from tests import matches_ref as mr
from tests import ransac_ref as rr

E = mr.E
RANK_TOL10 = 1e-10         # the 10 x 20 elimination; the 5 x 9 one keeps round 20's (rr.RANK_TOL)
BISECT = 40
NEWTON = 4
SAMPLE_OPS = 2000
CUBIC_OPS = 4000

# the monomials: variables 0 = x, 1 = y, 2 = z, 3 = 1; a quadratic's 10 and a cubic's 20 coefficients in lexicographic order
PAIRS = list(itertools.combinations_with_replacement(range(4), 2))
TRIPLES = list(itertools.combinations_with_replacement(range(4), 3))
# the 20 columns of the constraint matrix: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
COLUMNS = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
           (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3)]


# ------------------------------------------------------------------------------------------------------------- the sampler
def draw_samples5(seed, Hn, n, defect=None):
    """Round 20's draw stopped at 5 distinct rows -> (sample (Hn, 5) int32, -1 where none was; got (Hn))."""
    return rr.draw_samples(seed, Hn, n, defect=defect, k=5)


# ----------------------------------------------------------------------------------------------------------- the null space
def null_basis(A, defect=None):
    """A (H, 5, 9) -> (basis (H, 4, 9): the null vectors with the permuted unknowns 5, 6, 7, 8 set to 1 one at a time; valid):
    round 20's elimination stopped after 5 steps, and four of its back substitutions."""
    A, perm, valid = rr.eliminate(A, 5, defect)
    return np.stack([rr.back_substitute(A, perm, 5, free=5 + j) for j in range(4)], axis=1), valid


# ---------------------------------------------------------------------------------------------------------- the constraints
def mul11(a, b):
    """Two linear forms (H, 4) -> the quadratic (H, 10): out[PAIR(i, j)] += a_i b_j, i outer, j inner, from 0."""
    out = np.zeros((len(a), 10))
    for i in range(4):
        for j in range(4):
            q = PAIRS.index((min(i, j), max(i, j)))
            out[:, q] = out[:, q] + a[:, i] * b[:, j]
    return out


def mul21(a, b):
    """A quadratic (H, 10) times a linear form (H, 4) -> the cubic (H, 20): out[TRIPLE] += a_m b_k, m outer, k inner, from 0."""
    out = np.zeros((len(a), 20))
    for m, (i, j) in enumerate(PAIRS):
        for k in range(4):
            c = TRIPLES.index(tuple(sorted((i, j, k))))
            out[:, c] = out[:, c] + a[:, m] * b[:, k]
    return out


def constraints(basis, defect=None):
    """basis (H, 4, 9) -> M (H, 10, 20): row 0 det E, row 1 + 3 i + j entry (i, j) of E E^T E - tr(E E^T) E / 2, for
    E = x basis_0 + y basis_1 + z basis_2 + basis_3, the columns in COLUMNS' order."""
    e = [np.ascontiguousarray(basis[:, :, c]) for c in range(9)]                     # entry c of E: a linear form (H, 4)
    rows = []
    with np.errstate(all="ignore"):
        q0 = mul11(e[4], e[8]) - mul11(e[5], e[7])
        q1 = mul11(e[3], e[8]) - mul11(e[5], e[6])
        q2 = mul11(e[3], e[7]) - mul11(e[4], e[6])
        rows.append((mul21(q0, e[0]) - mul21(q1, e[1])) + mul21(q2, e[2]))
        G = {}
        for i in range(3):
            for j in range(i, 3):
                G[i, j] = G[j, i] = (mul11(e[3 * i], e[3 * j]) + mul11(e[3 * i + 1], e[3 * j + 1])) + mul11(e[3 * i + 2], e[3 * j + 2])
        half = 0.5 * ((G[0, 0] + G[1, 1]) + G[2, 2])
        for i in range(3):
            G[i, i] = G[i, i] - half
        for i in range(3):
            for j in range(3):
                rows.append((mul21(G[i, 0], e[j]) + mul21(G[i, 1], e[3 + j])) + mul21(G[i, 2], e[6 + j]))
    order = [TRIPLES.index(c) for c in COLUMNS]
    if defect == "swapped monomial":
        order[10], order[11] = order[11], order[10]
    M = np.stack(rows, axis=1)[:, :, order]
    if defect == "dropped row":
        M[:, 9] = M[:, 8]
    return M


def gauss_jordan(M, defect=None):
    """M (H, 10, 20) -> (M reduced, valid).  Step k: the pivot is the first largest |M_rk| of rows k .. 9; rows exchanged on
    columns k .. 19; RANK TEST finite and |p_k| > 1e-10 |p_0|; row k divided by p_k beyond column k; rows r > k, and rows
    4 <= r < k, become row_r - M_rk row_k beyond column k.  Rows 0 .. 3 are not reduced upwards: nothing reads them."""
    M = np.array(M, dtype=np.float64)
    H = len(M)
    ar = np.arange(H)
    valid = np.ones(H, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(10):
            col = np.abs(M[:, k:, k])
            col = np.where(np.isnan(col), -1.0, col)
            pr = k + col.argmax(axis=1)
            rk, rp = M[ar, k, k:].copy(), M[ar, pr, k:].copy()
            M[ar, pr, k:], M[ar, k, k:] = rk, rp
            p = M[:, k, k].copy()
            if k == 0:
                p0 = np.abs(p)
            if defect != "no rank test":
                valid &= np.isfinite(p) & (np.abs(p) > RANK_TOL10 * p0)
            M[:, k, k + 1:] = M[:, k, k + 1:] / p[:, None]
            for r in range(10):
                if r > k or 4 <= r < k:
                    m = M[:, r, k].copy()
                    M[:, r, k + 1:] = M[:, r, k + 1:] - m[:, None] * M[:, k, k + 1:]
    return M, valid


# --------------------------------------------------------------------------------------------------------------- the roots
def conv(a, b):
    """Polynomials in z, ascending: out[i + j] += a_i b_j, i outer, j inner, from 0."""
    out = np.zeros((len(a), a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            out[:, i + j] = out[:, i + j] + a[:, i] * b[:, j]
    return out


def z_matrix(M):
    """The reduced M -> B[i][j], i, j = 0 .. 2: row_(4 + 2 i) - z row_(5 + 2 i) collected as x B_i0(z) + y B_i1(z) + B_i2(z)."""
    B = []
    for i in range(3):
        a, b = M[:, 4 + 2 * i], M[:, 5 + 2 * i]
        B.append([np.stack((a[:, 12], a[:, 11] - b[:, 12], a[:, 10] - b[:, 11], -b[:, 10]), 1),
                  np.stack((a[:, 15], a[:, 14] - b[:, 15], a[:, 13] - b[:, 14], -b[:, 13]), 1),
                  np.stack((a[:, 19], a[:, 18] - b[:, 19], a[:, 17] - b[:, 18], a[:, 16] - b[:, 17], -b[:, 16]), 1)])
    return B


def determinant(B):
    """-> (p1 (H, 8), p2 (H, 8), p3 (H, 7), det (H, 11)): the cross product of rows 0 and 1 and its product with row 2."""
    p1 = conv(B[0][1], B[1][2]) - conv(B[1][1], B[0][2])
    p2 = conv(B[1][0], B[0][2]) - conv(B[0][0], B[1][2])
    p3 = conv(B[0][0], B[1][1]) - conv(B[1][0], B[0][1])
    return p1, p2, p3, (conv(p1, B[2][0]) + conv(p2, B[2][1])) + conv(p3, B[2][2])


def sturm_chain(det):
    """det (H, 11) -> (chain: f_0 (H, 11) .. f_10 (H, 1), valid).  f_0 = det / |det_10|; f_1[k - 1] = k f_0[k]; f_(i + 1) =
    -(rem(f_(i - 1), f_i)) / |its leading coefficient| by two steps of long division."""
    s = np.abs(det[:, 10])
    valid = np.isfinite(s) & (s > 0.0)
    f0 = det / s[:, None]
    f1 = np.stack([float(k) * f0[:, k] for k in range(1, 11)], 1)
    chain = [f0, f1]
    for i in range(1, 10):
        prev, cur = chain[i - 1], chain[i]
        n = prev.shape[1] - 1                                       # the degree of prev; cur's is n - 1
        r = prev.copy()
        g = cur[:, n - 1]
        q = r[:, n] / g
        for k in range(n - 1):
            r[:, k + 1] = r[:, k + 1] - q * cur[:, k]
        q = r[:, n - 1] / g
        for k in range(n - 1):
            r[:, k] = r[:, k] - q * cur[:, k]
        s = np.abs(r[:, n - 2])
        valid &= np.isfinite(s) & (s > 0.0)
        chain.append(-(r[:, :n - 1] / s[:, None]))
    return chain, valid


def horner(f, z):
    """f (H, d + 1), z (H) or (H, K) -> f(z)."""
    ex = (slice(None),) + (None,) * (z.ndim - 1)
    v = np.broadcast_to(f[:, -1][ex], z.shape)
    for k in range(f.shape[1] - 2, -1, -1):
        v = v * z + f[:, k][ex]
    return v


def sign_changes(chain, z):
    changes = np.zeros(z.shape, dtype=np.int64)
    last = np.zeros(z.shape, dtype=np.int64)
    for f in chain:
        v = horner(f, z)
        s = (v > 0.0).astype(np.int64) - (v < 0.0).astype(np.int64)
        changes += (s != 0) & (last != 0) & (s != last)
        last = np.where(s != 0, s, last)
    return changes


def real_roots(chain, defect=None):
    """-> (z (H, 10) ascending in the root's index, count (H)).  The real line is z = t / (1 - |t|), t in (-1, 1).  The sign
    changes at -inf and +inf are those of the leading coefficients (times (-1)^degree at -inf); count is their difference.  Root
    r is the smallest z with at least r + 1 roots in (-inf, z], by BISECT halvings of t from (-1, 1) with the chain's sign
    changes at z(t), then NEWTON steps z - f_0 / f_1, each taken only where the new z stays in the last interval."""
    f0, f1 = chain[0], chain[1]
    H = len(f0)
    lead = np.stack([f[:, -1] for f in chain], 1)                    # (H, 11): degree 10 - i
    alt = np.where(np.arange(11) % 2 == 0, 1.0, -1.0)               # (-1)^(10 - i)

    def changes_of(v):
        s = (v > 0.0).astype(np.int64) - (v < 0.0).astype(np.int64)
        return ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] != 0) & (s[:, :-1] != 0)).sum(axis=1)     # no leading coefficient is 0

    VL = changes_of(lead * alt)
    count = np.clip(VL - changes_of(lead), 0, 10)
    k = np.arange(10)[None, :]
    if defect == "roots descending":
        k = (count[:, None] - 1 - k) % 10
    lo, hi = np.full((H, 10), -1.0), np.full((H, 10), 1.0)
    for _ in range(8 if defect == "few bisections" else BISECT):
        mid = (lo + hi) * 0.5
        left = (VL[:, None] - sign_changes(chain, mid / (1.0 - np.abs(mid)))) >= k + 1
        hi = np.where(left, mid, hi)
        lo = np.where(left, lo, mid)
    mid = (lo + hi) * 0.5
    z, zlo, zhi = mid / (1.0 - np.abs(mid)), lo / (1.0 - np.abs(lo)), hi / (1.0 - np.abs(hi))
    for _ in range(0 if defect == "few bisections" else NEWTON):
        zn = z - horner(f0, z) / horner(f1, z)
        z = np.where((zn >= zlo) & (zn <= zhi), zn, z)
    return z, count


def solutions(basis, defect=None):
    """basis (H, 4, 9), all samples taken as valid so far -> (E (H, 10, 9), valid (H, 10) bool, info)."""
    H = len(basis)
    with np.errstate(all="ignore"):
        M0 = constraints(basis, defect)
        M, ok = gauss_jordan(M0, defect)
        B = z_matrix(M)
        p1, p2, p3, det = determinant(B)
        chain, ok2 = sturm_chain(det)
        z, count = real_roots(chain, defect)
        ok = ok & ok2
        d = horner(p3, z)
        x, y = horner(p1, z) / d, horner(p2, z) / d
        e = ((x[..., None] * basis[:, None, 0] + y[..., None] * basis[:, None, 1]) + z[..., None] * basis[:, None, 2]) + basis[:, None, 3]
        ss = e[..., 0] * e[..., 0]
        for c in range(1, 9):
            ss = ss + e[..., c] * e[..., c]
        e = e / np.sqrt(ss)[..., None]
        mag = np.where(np.isnan(e), -1.0, np.abs(e))
        lead = np.take_along_axis(e, mag.argmax(axis=2)[..., None], 2)
        e = np.where(lead < 0.0, -e, e)
        valid = ok[:, None] & (np.arange(10)[None] < count[:, None]) & np.isfinite(e).all(axis=2)
    e = np.where(valid[..., None], e, 0.0)
    return e, valid, {"M0": M0, "M": M, "det": det, "chain": chain, "z": z, "x": x, "y": y, "count": count, "ok": ok}


def hypotheses5(xy, count, intrinsics, Hn, seed, defect=None):
    """The rule of cpn_ransac_hypotheses5 for one pair: xy (N, 4) fp32 -> (E (Hn, 10, 9) float64, sample (Hn, 5) int32, valid
    (Hn, 10) uint8, info)."""
    xy = np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy))
    sample, got = draw_samples5(seed, Hn, n, defect)
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    rows = xy[np.maximum(sample, 0)]
    ok = (got == 5) & np.isfinite(rows).all(axis=(1, 2))
    A = rr.system(*rr.normalised(rows, k0, k1))
    A[~ok] = 0.0
    basis, okb = null_basis(A, defect)
    ok &= okb
    basis[~ok] = 0.0
    e, valid, info = solutions(basis, defect)
    valid &= ok[:, None]
    e[~valid] = 0.0
    info.update(A=A, basis=basis, sample_ok=ok)
    return e, sample, valid.astype(np.uint8), info


def ransac_pose5(xy, count, intrinsics, rel_pose=None, hypotheses_n=1024, inlier_px=1.0, seed=0, defect=None):
    """hypotheses5, then round 20's score and finish over the 10 hypotheses_n slots -> (pose, inlier, stats, info)."""
    Em, sample, valid, _ = hypotheses5(xy, count, intrinsics, hypotheses_n, seed, defect)
    Em, valid = Em.reshape(-1, 9), valid.reshape(-1)
    partial = rr.score(Em, valid, xy, count, intrinsics, inlier_px, rel_pose)
    pose, inlier, stats, info = rr.finish(Em, valid, partial, xy, count, intrinsics, inlier_px, rel_pose)
    info.update(E=Em, sample=sample, valid=valid, partial=partial)
    return pose, inlier, stats, info


# ------------------------------------------------------------------------------------------------- the independent solver
class _Poly(dict):
    """A polynomial in x, y, z as {exponents: coefficient}."""

    def __add__(self, o):
        out = _Poly(self)
        for m, c in o.items():
            out[m] = out.get(m, 0.0) + c
        return out

    def __mul__(self, o):
        if not isinstance(o, dict):
            return _Poly({m: c * o for m, c in self.items()})
        out = _Poly()
        for (m, c), (n, d) in itertools.product(self.items(), o.items()):
            key = (m[0] + n[0], m[1] + n[1], m[2] + n[2])
            out[key] = out.get(key, 0.0) + c * d
        return out

    def __sub__(self, o):
        return self + o * -1.0


_CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def independent(A):
    """One 5 x 9 system -> (E (r, 9) of the real roots, unit norm, largest entry positive; the 10 eigenvalues; cond of the
    10 x 10 block): SVD null space, the ten cubics by dictionary polynomials, the action matrix of x on the quotient basis."""
    N = np.linalg.svd(A)[2][5:]
    Em = [[_Poly({(1, 0, 0): N[0, 3 * i + j], (0, 1, 0): N[1, 3 * i + j], (0, 0, 1): N[2, 3 * i + j], (0, 0, 0): N[3, 3 * i + j]})
           for j in range(3)] for i in range(3)]
    mat = lambda X, Y: [[X[i][0] * Y[0][j] + X[i][1] * Y[1][j] + X[i][2] * Y[2][j] for j in range(3)] for i in range(3)]
    Et = [[Em[j][i] for j in range(3)] for i in range(3)]
    G = mat(Em, Et)
    tr = G[0][0] + G[1][1] + G[2][2]
    GE = mat(G, Em)
    eqs = [GE[i][j] * 2.0 - tr * Em[i][j] for i in range(3) for j in range(3)]
    eqs.append(Em[0][0] * (Em[1][1] * Em[2][2] - Em[1][2] * Em[2][1]) - Em[0][1] * (Em[1][0] * Em[2][2] - Em[1][2] * Em[2][0])
               + Em[0][2] * (Em[1][0] * Em[2][1] - Em[1][1] * Em[2][0]))
    C = np.array([[q.get(m, 0.0) for m in _CUBIC + _BASIS] for q in eqs])
    red = np.linalg.solve(C[:, :10], C[:, 10:])                     # cubic monomial = -red . basis
    act = np.zeros((10, 10))
    for r, m in enumerate(_BASIS):                                  # x times the basis monomial m
        t = (m[0] + 1, m[1], m[2])
        if t in _CUBIC:
            act[r] = -red[_CUBIC.index(t)]
        else:
            act[r, _BASIS.index(t)] = 1.0
    w, V = np.linalg.eig(act)
    out = []
    for k in np.flatnonzero(np.abs(w.imag) <= 1e-9 * np.maximum(1.0, np.abs(w.real))):
        v = V[:, k].real
        e = (v[6] * N[0] + v[7] * N[1] + v[8] * N[2] + v[9] * N[3])
        e = e / np.linalg.norm(e)
        out.append(e if e[np.abs(e).argmax()] > 0 else -e)
    return np.array(out).reshape(-1, 9), w, np.linalg.cond(C[:, :10])


def cubic_residual(e):
    """e (.., 9) -> the largest of |det E| and |2 E E^T E - tr(E E^T) E| per E."""
    M = np.asarray(e).reshape(e.shape[:-1] + (3, 3))
    G = M @ np.swapaxes(M, -1, -2)
    tr = np.trace(G, axis1=-2, axis2=-1)
    return np.maximum(np.abs(np.linalg.det(M)), np.abs(2.0 * G @ M - tr[..., None, None] * M).max(axis=(-1, -2)))


# ------------------------------------------------------------------------------------------------------------- the scenes
WALL = dict(n=1000, seed=16, noise_px=0.5, outliers=0.3, off_plane=0.0)


@functools.lru_cache(maxsize=None)
def wall_scene(n=1000, seed=16, noise_px=0.0, outliers=0.0, off_plane=0.0):
    """refine_scene with its points on the plane (0.25, -0.1, 1) . X = 3: the same cameras, pose and random stream (the depths
    are drawn and, but for a share off_plane of the points chosen by a draw after all others, replaced by 3 / (ray . normal)).
    Returns refine_scene's dict.  Computed once, shared, never written to."""
    rng = np.random.default_rng(seed)
    S, f = 256, 200.0
    R_true, t_true = mr.rodrigues((0.3, 1.0, -0.2), 12.0), np.array([0.55, 0.08, 0.21])
    p0 = rng.uniform(0.0, S, size=(n, 2))
    free = rng.uniform(1.0, 6.0, size=n)
    noise = rng.normal(scale=noise_px, size=(n, 2)) if noise_px else 0.0
    ray = np.concatenate(((p0 - S / 2.0) / f, np.ones((n, 1))), 1)
    depth = 3.0 / (ray @ np.array([0.25, -0.1, 1.0]))
    bad = rng.random(n) < outliers if outliers else np.zeros(n, dtype=bool)
    wild = rng.uniform(0.0, S, size=(int(bad.sum()), 2))
    if off_plane:
        off = rng.random(n) < off_plane
        depth[off] = free[off]
    X1 = (ray * depth[:, None] - t_true) @ R_true
    p1 = f * X1[:, :2] / X1[:, 2:] + S / 2.0 + noise
    p1[bad] = wild
    K = mr.pinhole(f, S)
    return {"xy": np.concatenate((p0, p1), 1).astype(np.float32), "intrinsics": np.stack((K, K)),
            "rel_pose": mr.refine_scene()["rel_pose"], "R_true": R_true, "t_true": t_true}


NAN_ROW = 17


@functools.lru_cache(maxsize=None)
def hypotheses5_case():
    """B = 6 pairs of N = 64 rows of the noisy scene: counts 64, 6 (redraws), 4 (below 5), 100 (beyond N), -3, and 64 with a NaN
    row inside the count -> (xy (6, 64, 4) fp32, counts (6) int32, intrinsics (6, 2, 4, 4) fp32).  Shared, never written to."""
    sc = mr.refine_scene(**rr.NOISY)
    xy = np.stack([sc["xy"][64 * b:64 * b + 64] for b in (0, 1, 2, 0, 3, 0)]).copy()
    xy[5, NAN_ROW, 2] = np.nan
    return xy, np.asarray((64, 6, 4, 100, -3, 64), dtype=np.int32), np.stack([sc["intrinsics"]] * 6)


@functools.lru_cache(maxsize=None)
def pose_case(Hn=64):
    """The batch of the whole-call test: the wall and the noisy scene, N = 1000, Hn samples, 1 px, seed 0, rel_pose the truth
    -> per pair (scene, the restatement's (pose, inlier, stats, info)).  Shared, never written to."""
    out = []
    for sc in (wall_scene(**WALL), mr.refine_scene(**rr.NOISY)):
        out.append((sc, ransac_pose5(sc["xy"], 1000, sc["intrinsics"], rr.true_pose(sc), Hn, 1.0, 0)))
    return out


@functools.lru_cache(maxsize=None)
def systems(scene, Hn=1024, seed=0):
    """-> (scene dict, the restatement's (E, sample, valid, info) of Hn samples of a scene ("noisy", "wall" or "exact"))."""
    sc = {"noisy": lambda: mr.refine_scene(**rr.NOISY), "exact": lambda: mr.refine_scene(**rr.EXACT),
          "wall": lambda: wall_scene(**WALL)}[scene]()
    return sc, hypotheses5(sc["xy"], len(sc["xy"]), sc["intrinsics"], Hn, seed)
