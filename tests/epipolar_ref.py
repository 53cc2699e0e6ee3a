"""Yardsticks of the log's drawings (coponerf_amd/summaries.py: epipolar_lines, epipolar_panels, mask_contour;
csrc/epipolar.hip) and the inputs of their tests.

  two_view_geometry(...)   summary/inspect_epipolar_geometry.py:13-43 in numpy float64 from the fp32 inputs, np.linalg.inv and
                           np.dot as there; pinned against the reference's own function by tests/golden/epipolar_F.npz
                           (tests/golden/make_golden_epipolar.py)
  epilines(...)            l = F (x, y, 1) per point, and line_ends(...): the end points of drawpointslines (:54-55), int()
                           truncating toward zero, with the validity rule of include/coponerf_hip.h
  in_disc / on_line        the coverage rules of include/coponerf_hip.h evaluated with PYTHON INTEGERS: exact at any magnitude
  fringe(...)              the pixels of a line whose decision is numerically delicate: |4 (w x d)^2 - T^2 L^2| <= 1e-9 T^2 L^2
                           and the two cap analogues
  panels(...)              the (2, B, S, 2 S, 3) panels from given end points: the blend of :105-106 in float32
  contour_rule(...)        the contour of summaries.py:65-71 as the border-point rule, and masks(S): the masks of its tests

The bound of the float64 geometry, EPS64 = 64 x 2^-53 relative to the absolute-value products:
  |F_dev - F_ref| <= EPS64 x G,  G = |inv(K0)|^T |[t]x| |R| |inv(K1)|  (entrywise),   |l_dev - l_ref| <= EPS64 x G (x, y, 1).
What numpy does there: skew() builds a float64 array (Python ints beside float32 scalars), so E and both products are
float64; but np.linalg.inv of an fp32 matrix works in float64 and returns the inverse ROUNDED TO fp32.  The kernel does the
same, so the two sides multiply the SAME fp32 inverses, provided no entry of the float64 inverse lies so close to the midpoint
of two fp32 numbers that the two float64 forms round apart: an entry of an inverse of a pinhole matrix (upper triangular:
every cofactor is ONE product, the other being a product with an exact 0) costs the cofactor (1), the determinant (3 products,
2 sums: 5) and the division (1): 7 roundings in the kernel's cofactor form, and no more in LAPACK's for a triangular matrix;
inverse_margin(...) returns how much further than 16 x 2^-53 (relative) every entry lies from such a midpoint, and
tests/test_epipolar_ref.py asserts it positive for every case.  What remains, each rounding relative to the entry's own terms
of G: an entry of E = [t]x R two products and a sum (the third term is an exact 0): 3; each of the two 3-term products
sum_j a_j b_j 3 in the standard gamma_3 form: 9 for either side, 18 for the two, and 3 more each for the line's own 3-term
product: 24 < 64.  The bound is relative to G and not to |F|: where the terms of an entry cancel, neither side is accurate
relative to the entry itself.  For intrinsics that are not triangular a cofactor is a difference of two products and the
two inverses may round apart (by one fp32 ulp of an entry: cond(K) 2^-53 decides).

An end point y = -c / b (or -(c + a W) / b) then moves by at most
  |y| (dc / |c'| + db / |b|) + 2^-52 |y|,   dc = EPS64 (G x)_2 (+ W EPS64 (G x)_0 + 2^-52 (|c| + |a| W) for the second),
and int(y) is the same on both sides when y is further than that from an integer: end_margin(...) returns distance minus
movement, and the cases below are chosen so that it is positive for every line (tests/test_epipolar_ref.py asserts it).
"""
import functools
import math

import numpy as np
import torch

from coponerf_amd import synthetic as syn
from coponerf_amd.summaries import EPIPOLAR_COLORS, default_points

EPS64 = 64 * 2.0 ** -53
FRINGE = 1e-9
CONTOUR_COLOR = (255, 102, 51)
GOLDEN_SEED, GOLDEN_SIDE = 131, 64


# ------------------------------------------------------------------------------------------------------- the geometry
def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def two_view_geometry(intrinsics, rel_pose, gt_rel_pose):
    """(E, F), each (2, B, 3, 3) float64, entry 0 under rel_pose and entry 1 under gt_rel_pose, as inspect() calls
    two_view_geometry(K1 = intrinsics[:, 1], K2 = intrinsics[:, 0], ...): F = inv(K2).T . E . inv(K1), E = [t]x R.  The arrays
    keep the dtypes they have there: skew() of fp32 scalars is float64, inv() of an fp32 matrix is fp32."""
    K = intrinsics.numpy()
    E, F = [], []
    for pose in (rel_pose.numpy(), gt_rel_pose.numpy()):
        tx = np.stack([skew(pose[i, :3, 3]) for i in range(len(pose))])
        e = np.matmul(tx, pose[:, :3, :3])
        E.append(e)
        F.append(np.stack([np.linalg.inv(K[i, 0, :3, :3]).T.dot(e[i]).dot(np.linalg.inv(K[i, 1, :3, :3])) for i in range(len(e))]))
    return np.stack(E).astype(np.float64), np.stack(F).astype(np.float64)


def geometry_scale(intrinsics, rel_pose, gt_rel_pose):
    """G (2, B, 3, 3): |inv(K0)|^T |[t]x| |R| |inv(K1)|, what the bound of F is relative to."""
    K = intrinsics.numpy().astype(np.float64)
    out = []
    for pose in (rel_pose.numpy().astype(np.float64), gt_rel_pose.numpy().astype(np.float64)):
        out.append(np.stack([np.abs(np.linalg.inv(K[i, 0, :3, :3])).T @ np.abs(skew(pose[i, :3, 3])) @ np.abs(pose[i, :3, :3])
                             @ np.abs(np.linalg.inv(K[i, 1, :3, :3])) for i in range(len(K))]))
    return np.stack(out)


def inverse_margin(intrinsics):
    """Smallest over the entries of both float64 inverses of: relative distance from the nearest midpoint of two neighbouring
    fp32 numbers, minus 16 x 2^-53.  Positive: any two float64 forms of the inverse round to the same fp32 matrix.  Entries
    that are exactly 0 round alike and are left out."""
    inv = np.linalg.inv(intrinsics.numpy().astype(np.float64)[..., :3, :3])
    v = np.abs(inv[inv != 0])
    r = v.astype(np.float32)                                                          # v lies between the midpoints beside r
    mids = np.stack([(r.astype(np.float64) + np.nextafter(r, np.float32(side)).astype(np.float64)) / 2 for side in (0, np.inf)])
    return float((np.abs(mids - v).min(axis=0) / v).min() - 16 * 2.0 ** -53)


def homogeneous(points):
    p = np.asarray(points, dtype=np.float64)
    return np.concatenate([p, np.ones((len(p), 1))], axis=1)


def epilines(F, points):
    """(2, B, P, 3) float64: l = F (x, y, 1) of every point."""
    return np.einsum("kbij,pj->kbpi", F, homogeneous(points))


def line_scale(G, points):
    return np.einsum("kbij,pj->kbpi", G, np.abs(homogeneous(points)))


def line_ends(lines, W):
    """(ends (..., 4) int64, valid (...) bool) of lines (..., 3): drawpointslines' end points and the validity rule."""
    a, b, c = lines[..., 0], lines[..., 1], lines[..., 2]
    with np.errstate(all="ignore"):
        y0, y1 = -c / b, -(c + a * W) / b
    ok = (b != 0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(y0) & np.isfinite(y1)
    ok &= (np.abs(np.where(ok, y0, 0)) < 2.0 ** 31) & (np.abs(np.where(ok, y1, 0)) < 2.0 ** 31)
    ends = np.zeros(lines.shape[:-1] + (4,), dtype=np.int64)
    ends[..., 1] = np.trunc(np.where(ok, y0, 0)).astype(np.int64)
    ends[..., 2] = np.where(ok, W, 0)
    ends[..., 3] = np.trunc(np.where(ok, y1, 0)).astype(np.int64)
    return ends, ok


def end_margin(lines, scale, W):
    """(..., 2): how much further from an integer each end point's y lies than the two sides' roundings can move it (module
    docstring); NaN for an invalid line.  Positive: int(y) is decided."""
    a, b, c = lines[..., 0], lines[..., 1], lines[..., 2]
    da, db, dc = (EPS64 * scale[..., i] for i in range(3))
    out = []
    with np.errstate(all="ignore"):
        for num, dnum in ((c, dc), (c + a * W, dc + W * da + 2.0 ** -52 * (np.abs(c) + np.abs(a) * W))):
            y = -num / b
            move = np.abs(y) * (dnum / np.abs(num) + db / np.abs(b) + 2.0 ** -52)
            out.append(np.abs(y - np.rint(y)) - move)
    return np.stack(out, axis=-1)


# ------------------------------------------------------------------------------------------------------ coverage rules
def in_disc(x, y, cx, cy, r):
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def disc_half_widths(r):
    """Half-width of every row 0 .. r of the disc of radius r (0 for a row that holds the centre column only)."""
    return [max(dx for dx in range(r + 1) if in_disc(dx, dy, 0, 0, r)) for dy in range(r + 1)]


def _grid(S):
    ys, xs = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    return xs.astype(object), ys.astype(object)               # Python integers: exact at any magnitude


def _terms(S, p0, p1):
    x, y = _grid(S)
    x0, y0, x1, y1 = (int(v) for v in (*p0, *p1))
    dx, dy, wx, wy = x1 - x0, y1 - y0, x - x0, y - y0
    return dx * dx + dy * dy, wx * dx + wy * dy, wx * wx + wy * wy, (x - x1) ** 2 + (y - y1) ** 2, wx * dy - wy * dx


_NEAR = np.frompyfunc(lambda lhs, rhs: abs(lhs - rhs) * 10 ** 9 <= rhs, 2, 1)      # FRINGE = 1e-9, in integers


def line_cover(S, p0, p1, T):
    """(on, fringe), each (S, S) bool [y, x], in Python integers.  on: the capsule of thickness T around the segment p0 p1.
    fringe: pixels whose own test lies within FRINGE (relative) of equality - where a float64 evaluation of the rule may decide
    the other way."""
    LL, s, ww, ee, cr = _terms(S, p0, p1)
    TT = int(T) * int(T)
    start, end = (s <= 0).astype(bool), (s >= LL).astype(bool)
    lhs = np.where(start, 4 * ww, np.where(end, 4 * ee, 4 * cr * cr))
    rhs = np.where(start | end, np.full(s.shape, TT, dtype=object), np.full(s.shape, TT * LL, dtype=object))
    return (lhs <= rhs).astype(bool), _NEAR(lhs, rhs).astype(bool)


def on_line(S, p0, p1, T):
    return line_cover(S, p0, p1, T)[0]


def fringe(S, p0, p1, T):
    return line_cover(S, p0, p1, T)[1]


def brute_force_distance(S, p0, p1):
    """(S, S) float64: distance of every pixel to the segment, the textbook way (clamped projection, a square root)."""
    ys, xs = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    d = p1 - p0
    LL = float(d @ d)
    t = np.zeros_like(xs) if LL == 0 else np.clip(((xs - p0[0]) * d[0] + (ys - p0[1]) * d[1]) / LL, 0.0, 1.0)
    return np.hypot(xs - (p0[0] + t * d[0]), ys - (p0[1] + t * d[1]))


def panels(rgb, points, colors, ends, valid, radius, thickness):
    """(out (2, B, S, 2 S, 3) float32, hit (2, B, S, 2 S) int: index of the point / line that colours the pixel or -1,
    delicate (2, B, S, 2 S) bool: the union of the lines' fringes) from ends (2, B, P, 4) and valid (2, B, P)."""
    rgb = rgb.numpy()
    B, S = rgb.shape[0], rgb.shape[2]
    colors = np.asarray(colors, dtype=np.float32)
    view = (rgb + np.float32(1.0)) * np.float32(127.5)
    out = np.empty((2, B, S, 2 * S, 3), dtype=np.float32)
    hit = np.full((2, B, S, 2 * S), -1, dtype=np.int64)
    delicate = np.zeros((2, B, S, 2 * S), dtype=bool)
    x, y = _grid(S)
    discs = [in_disc(x, y, int(px), int(py), int(radius)).astype(bool) for px, py in points]
    for k in range(2):
        for b in range(B):
            for p in range(len(points)):
                hit[k, b, :, :S][discs[p]] = p
                if valid[k, b, p]:
                    e = ends[k, b, p]
                    on, near = line_cover(S, e[:2], e[2:], thickness)
                    hit[k, b, :, S:][on] = p
                    delicate[k, b, :, S:] |= near
            out[k, b, :, :S], out[k, b, :, S:] = view[b, 1], view[b, 0]
    on = hit >= 0
    col = colors[np.maximum(hit, 0)]
    right = np.zeros_like(on)
    right[..., S:] = True
    blend = np.float32(0.4) * col + np.float32(0.6) * out
    out = np.where((on & right)[..., None], blend, np.where((on & ~right)[..., None], col, out)).astype(np.float32)
    return out, hit, delicate


def covered(got, rgb):
    """(2, B, S, 2 S) bool: where a panel differs from the plain views - the pixels the kernel drew on."""
    view = (rgb.numpy() + np.float32(1.0)) * np.float32(127.5)
    plain = np.concatenate([view[:, 1], view[:, 0]], axis=2)
    return (got != plain[None]).any(axis=-1)


# ------------------------------------------------------------------------------------------------------------ contour
def contour_rule(mask):
    """(..., S, S) bool: invalid pixels (mask == 0) with a valid or outside-the-image 4-neighbour."""
    valid = np.asarray(mask) != 0
    pad = np.pad(valid, [(0, 0)] * (valid.ndim - 2) + [(1, 1), (1, 1)], constant_values=True)
    near = pad[..., :-2, 1:-1] | pad[..., 2:, 1:-1] | pad[..., 1:-1, :-2] | pad[..., 1:-1, 2:]
    return ~valid & near


def draw_contour(overlay, mask):
    out = np.array(overlay, copy=True)
    out[contour_rule(mask)] = CONTOUR_COLOR
    return out


def masks(S):
    """{name: (S, S) uint8, 1 = valid}: the invalid REGION is empty, full, a single pixel (inside, in a corner), a ring with a
    hole, two squares touching diagonally, seeded noise at three densities, and a smooth blob that touches the border."""
    out = {"empty": np.ones((S, S), np.uint8), "full": np.zeros((S, S), np.uint8)}
    m = np.ones((S, S), np.uint8)
    m[S // 2, S // 3] = 0
    out["pixel"] = m
    m = np.ones((S, S), np.uint8)
    m[0, S - 1] = 0
    out["corner"] = m
    m = np.ones((S, S), np.uint8)
    m[1:S - 1, 1:S - 1] = 0
    m[3:S - 3, 3:S - 3] = 1
    out["ring"] = m
    m = np.ones((S, S), np.uint8)
    h = S // 2
    m[h - 3:h, h - 3:h] = 0
    m[h:h + 3, h:h + 3] = 0
    out["diagonal"] = m
    for i, density in enumerate((0.1, 0.5, 0.9)):
        out[f"noise{i}"] = (syn.uniform((S, S), 7 + S, 0.0, 1.0, stream=40 + i).numpy() < density).astype(np.uint8)
    ys, xs = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    out["blob"] = (np.hypot(xs - 0.2 * S, ys - 0.6 * S) > 0.35 * S).astype(np.uint8)
    return out


# -------------------------------------------------------------------------------------------------------------- cases
def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def _K(S, f, cx, cy):
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f * S
    K[0, 2], K[1, 2] = cx * S, cy * S
    return K


def _pose(rot, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, t
    return m


CASES = ("generic", "same", "miss", "vertical", "nan", "shared", "steep")


@functools.lru_cache(maxsize=None)
def case(name, B, S):
    """(rgb (B, 2, S, S, 3), intrinsics (B, 2, 4, 4), rel_pose, gt_rel_pose (B, 4, 4), points (P, 2) int) fp32 tensors, pure
    functions of the arguments; shared, never written to.
      generic   unequal intrinsics, poses 0.2 - 0.4 rad off one another, slanted lines through the image; the nine points
                plus (0, 0) and (S - 1, S / 2), whose discs the border clips
      same      rel_pose == gt_rel_pose
      miss      sideways translation with view 0's principal point five image sides down: every line lies far below the image
      vertical  pure y translation, equal intrinsics, no rotation: b == 0 for every line
      nan       generic with a NaN in rel_pose of item 1 (B >= 2) or item 0
      shared    pure x translation, focal lengths 0.8 S and 0.7 S: points (S/4, S/2 + 4) and (3S/4, S/2 + 4) share a line
      steep     translation (1 / 15000.7, 1, 0) x 0.3: |y| of the end points between 2^16 and 2^20, lines 3 - 4 px apart in x"""
    from tests import ssim_ref
    rgb = ssim_ref.case(B, S, S, 4, seed=300 + S)[0]
    K = np.stack([np.stack([_K(S, 0.8, 0.5, 0.5), _K(S, 0.7, 0.53, 0.48)])] * B)
    extra = [(0, 0), (S - 1, S // 2)]
    points = list(default_points(S)) + extra
    rel, gt = [], []
    for b in range(B):
        rel.append(_pose(syn._rot_y(-0.2 - 0.1 * b) @ _rot_x(0.07 * (b + 1)), [0.3, 0.06 * (b + 1), 0.05 - 0.03 * b]))
        gt.append(_pose(syn._rot_y(-0.1), [0.3, 0.013, 0.0]))
    if name == "same":
        rel = gt
    elif name == "miss":
        K = np.stack([np.stack([_K(S, 0.8, 0.5, 5.0), _K(S, 0.7, 0.53, 0.48)])] * B)
        rel = [_pose(np.eye(3), [0.3, 0.0, 0.0])] * B
        gt = [_pose(np.eye(3), [0.3, 0.02, 0.0])] * B
    elif name == "vertical":
        K = np.stack([np.stack([_K(S, 0.8, 0.5, 0.5)] * 2)] * B)
        rel = [_pose(np.eye(3), [0.0, 0.3, 0.0])] * B
        gt = [_pose(np.eye(3), [0.0, -0.25, 0.0])] * B
    elif name == "nan":
        rel[min(1, B - 1)] = rel[min(1, B - 1)].copy()
        rel[min(1, B - 1)][1, 2] = float("nan")
    elif name == "shared":
        K = np.stack([np.stack([_K(S, 0.8, 0.5, 0.5), _K(S, 0.7, 0.5, 0.5)])] * B)
        rel = [_pose(np.eye(3), [0.3, 0.0, 0.0])] * B
        gt = [_pose(np.eye(3), [-0.2, 0.0, 0.0])] * B
        points = [(S // 4, S // 2 + 4), (S // 2, S // 4), (3 * S // 4, S // 2 + 4)]
    elif name == "steep":
        K = np.stack([np.stack([_K(S, 0.8, 0.5, 0.5)] * 2)] * B)
        rel = [_pose(np.eye(3), [0.3 / 15000.7, 0.3, 0.0])] * B
        gt = [_pose(np.eye(3), [-0.3 / 9000.3, 0.3, 0.0])] * B
        points = list(default_points(S))
    elif name != "generic":
        raise KeyError(name)
    f32 = lambda a: torch.from_numpy(np.stack(a).astype(np.float32)).contiguous()
    return rgb, f32(K), f32(rel), f32(gt), torch.tensor(points, dtype=torch.int32)


def colors_for(P):
    """(P, 3) float32: the reference's nine colours, continued by seeded ones."""
    more = syn.uniform((max(P - 9, 1), 3), 55, 0.0, 256.0, stream=3).numpy().astype(np.int64)
    return np.concatenate([np.asarray(EPIPOLAR_COLORS, dtype=np.int64), more])[:P].astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_lines(name, B, S):
    """The float64 side of case(name, B, S): dict of F, G, lines, scale, ends, valid, margin."""
    _, K, rel, gt, points = case(name, B, S)
    _, F = two_view_geometry(K, rel, gt)
    G = geometry_scale(K, rel, gt)
    lines = epilines(F, points.numpy())
    scale = line_scale(G, points.numpy())
    ends, valid = line_ends(lines, S)
    return {"F": F, "G": G, "lines": lines, "scale": scale, "ends": ends, "valid": valid, "margin": end_margin(lines, scale, S)}


def golden_inputs():
    """(intrinsics (4, 2, 4, 4), rel_pose, gt_rel_pose (4, 4, 4)) fp32 of tests/golden/epipolar_F.npz: four pairs of
    coponerf_amd.synthetic's wide rig; the true relative pose from the pairs' cameras, the estimate a seeded turn and shift off."""
    inp = syn.make_inputs(4, GOLDEN_SIDE, GOLDEN_SIDE, 16, seed=GOLDEN_SEED, rig="wide", jitter=0.05)
    c2w = inp["context"]["cam2world"].double().numpy()
    gt = np.stack([np.linalg.inv(c2w[b, 1]) @ c2w[b, 0] for b in range(4)])
    jit = syn.uniform((4, 4), GOLDEN_SEED, -0.1, 0.1, stream=9).numpy().astype(np.float64)
    rel = np.stack([_pose(syn._rot_y(jit[b, 3]) @ gt[b, :3, :3], gt[b, :3, 3] + jit[b, :3]) for b in range(4)])
    K = inp["context"]["intrinsics"].clone()
    K[:, 1, 0, 0] *= 0.9                                     # unequal views: the order of the two inverses matters
    K[:, 1, 1, 1] *= 0.9
    K[:, 1, 0, 2] += 1.5
    return K.contiguous(), torch.from_numpy(rel.astype(np.float32)), torch.from_numpy(gt.astype(np.float32))
