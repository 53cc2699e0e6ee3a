"""numpy restatements of csrc/splat.hip's three entry points, in the operation order include/coponerf_hip.h fixes, and the cases
of tests/test_gpu_splat.py.  Pinned on the CPU by tests/test_splat_ref.py against a painter's implementation.

Every result is an integer or a bit pattern: the keys are (bits of the fp32 depth) << 32 | index, the outputs follow from
them.  numpy's float64 element-wise operations round once each, as the kernel's do with contraction off, so the comparison on
the GPU is exact; `band` marks the points with a decision within BAND of a threshold (u + 0.5 or v + 0.5 of an integer, Y_z of
near), and tests/test_splat_ref.py holds every case to none.
"""
import numpy as np

BAND = 1e-9
EMPTY = np.uint64(2 ** 64 - 1)
LIM = 2.0 ** 30
NEAR = 1e-3


# ------------------------------------------------------------------------------------------------------------ restatements
def project(X32, pose32, intr32, near):
    """One camera, n points: (counts (n) bool, c (n) int64, r (n) int64, z32 (n) float32, band (n) bool) of xyz (n, 3) fp32,
    pose (4, 4) fp32 and intrinsics (4, 4) fp32, every operation in float64 and in the header's order."""
    X, P, Km = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (X32, pose32, intr32))
    R, t = P[:3, :3], P[:3, 3]
    fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
    with np.errstate(all="ignore"):
        d = X - t
        Y = [(R[0, j] * d[:, 0] + R[1, j] * d[:, 1]) + R[2, j] * d[:, 2] for j in range(3)]
        u = (fx * Y[0]) / Y[2] + cx
        v = (fy * Y[1]) / Y[2] + cy
        z32 = Y[2].astype(np.float32)
        finite_in = np.isfinite(X).all(axis=1) & np.isfinite(P[:3]).all() & np.isfinite([fx, fy, cx, cy]).all()
        in_front = finite_in & (Y[2] >= near)
        counts = in_front & (np.abs(u) < LIM) & (np.abs(v) < LIM) & np.isfinite(z32)       # NaN compares false
        pu, pv = np.floor(u + 0.5), np.floor(v + 0.5)
        band = finite_in & (np.abs(Y[2] - near) < BAND)
        band |= counts & ((np.abs(u + 0.5 - np.rint(u + 0.5)) < BAND) | (np.abs(v + 0.5 - np.rint(v + 0.5)) < BAND))
    c = np.where(counts, pu, 0).astype(np.int64)
    r = np.where(counts, pv, 0).astype(np.int64)
    return counts, c, r, z32, band


def splat_points(xyz, count, poses, intrinsics, H, W, radius, near=NEAR):
    """cpn_splat_points -> (zbuf (K, B, H, W) uint64, band (K, B, cap) bool)."""
    K, B, cap = poses.shape[0], poses.shape[1], xyz.shape[1]
    zbuf = np.full((K, B, H * W), EMPTY, dtype=np.uint64)
    band = np.zeros((K, B, cap), dtype=bool)
    for k in range(K):
        for b in range(B):
            n = min(max(int(count[b]), 0), cap)
            counts, c, r, z32, band[k, b, :n] = project(xyz[b, :n], poses[k, b], intrinsics[b], near)
            key = (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    rr, cc = r + dy, c + dx
                    ok = counts & (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
                    np.minimum.at(zbuf[k, b], (rr * W + cc)[ok], key[ok])
    return zbuf.reshape(K, B, H, W), band


def resolve(zbuf, rgb, fill, background=(0, 0, 0)):
    """cpn_splat_resolve -> (frames (K, B, H, W, 3) uint8, depth bits (K, B, H, W) uint32 - 0x7FC00000 where empty, compare
    with isnan there -, index (K, B, H, W) int32)."""
    K, B, H, W = zbuf.shape
    cap = rgb.shape[1]
    key = zbuf.copy()
    if fill > 0:
        pad = np.full((K, B, H + 2 * fill, W + 2 * fill), EMPTY, dtype=np.uint64)
        pad[:, :, fill:fill + H, fill:fill + W] = zbuf
        around = zbuf.copy()
        for dy in range(2 * fill + 1):
            for dx in range(2 * fill + 1):
                around = np.minimum(around, pad[:, :, dy:dy + H, dx:dx + W])
        key = np.where(zbuf == EMPTY, around, zbuf)                     # from the unfilled buffer only: no cascading
    low = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hit = (key != EMPTY) & (low < cap)
    index = np.where(hit, low, -1).astype(np.int32)
    bits = np.where(hit, key >> np.uint64(32), 0x7FC00000).astype(np.uint32)
    frames = np.empty((K, B, H, W, 3), dtype=np.uint8)
    frames[...] = np.asarray(background, dtype=np.uint8)
    for b in range(B):
        frames[:, b][hit[:, b]] = rgb[b][low[:, b][hit[:, b]]]
    return frames, bits, index


def score(frames, index, target):
    """cpn_splat_score -> stats (K, B, 2) int64."""
    e = frames.astype(np.int64) - target.astype(np.int64)
    hit = index >= 0
    return np.stack((hit.sum(axis=(2, 3)), ((e * e).sum(axis=4) * hit).sum(axis=(2, 3))), axis=-1).astype(np.int64)


def coverage_psnr(stats, H, W):
    """splat.score's two figures of stats, in float64."""
    n, sse = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)
    with np.errstate(all="ignore"):
        return n / float(H * W), 10.0 * np.log10(((255.0 ** 2 * 3.0) * n) / sse)


def draw(case, radius, fill, background=(0, 0, 0)):
    """The whole of a case at (radius, fill): dict of zbuf, frames, bits, index, band."""
    key = (id(case), radius, fill, tuple(background))
    if key not in _CACHE:
        zkey = (id(case), radius)
        if zkey not in _CACHE:
            _CACHE[zkey] = splat_points(case["xyz"], case["count"], case["poses"], case["intrinsics"], case["H"], case["W"], radius)
        zbuf, band = _CACHE[zkey]
        frames, bits, index = resolve(zbuf, case["rgb"], fill, background)
        _CACHE[key] = dict(zbuf=zbuf, frames=frames, bits=bits, index=index, band=band)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------------- cases
_CACHE = {}


def rigid(deg_xyz, t):
    """(4, 4) fp32: rotations about x, y and z (degrees, in that order), then the translation: camera to reference."""
    ax, ay, az = np.radians(deg_xyz)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Rz @ Ry @ Rx, t
    return P.astype(np.float32)


def intrinsics_of(fx, fy, cx, cy):
    return np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)


def place(pose, intr, u, v, d):
    """fp32 points of depth d on the rays of the pixels (u, v) of a camera, in the reference frame."""
    P, Km = pose.astype(np.float64), intr.astype(np.float64)
    p = np.stack(((u - Km[0, 2]) / Km[0, 0] * d, (v - Km[1, 2]) / Km[1, 1] * d, d * np.ones_like(u)), axis=-1)
    return (p @ P[:3, :3].T + P[:3, 3]).astype(np.float32)


def _frozen(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _off(rng, n):
    return rng.uniform(-0.35, 0.35, size=n)                             # a pixel centre plus this stays clear of the half


def main_case():
    """H x W = 24 x 40, B = 2, K = 3, cap = 600, counts (517, 0).  Camera 0 of each pair is the identity, so a point's Y_z there
    is its own fp32 z and equal depths are equal bit patterns; cameras 1 and 2 turn and move.  Pair 0's rows, in order:
      0 .. 405    406 points over the image and up to 3 pixels beyond it (outside, and footprints clipped), depths 1 .. 5
      406 .. 413  the four corners and the four edge middles, depth 0.8
      414 .. 419  just outside each border and two corners, depth 0.75: their footprints reach in at radius 1 or 2
      420 .. 439  behind camera 0
      440 .. 449  in front of camera 0 but nearer than near
      450 .. 461  a NaN, +inf or -inf in one coordinate
      462 .. 481  / 482 .. 501  twenty pairs of one pixel and ONE fp32 depth, 0.9: the first of a pair must win
      502 .. 516  exact duplicates of the rows 0, 20, 40, ..
      517 .. 599  beyond the count: points at depth 0.5 all over the image that would win every pixel, and NaN
    Pair 1's count is 0 and its 600 rows are such points too."""
    if "main" in _CACHE:
        return _CACHE["main"]
    rng = np.random.default_rng(17)
    H, W, B, K, cap = 24, 40, 2, 3, 600
    intr = np.stack((intrinsics_of(34.0, 31.0, 19.3, 11.6), intrinsics_of(29.0, 33.0, 20.4, 12.2)))
    moves = (((0, 0, 0), (0, 0, 0)), ((2.0, -5.0, 1.0), (0.20, -0.05, 0.10)), ((-3.0, 6.0, -2.0), (-0.15, 0.10, -0.20)))
    poses = np.stack([np.stack([rigid(deg, np.array(t) * (1.0 - 0.2 * b)) for b in range(B)]) for deg, t in moves])
    eye = poses[0, 0]
    assert np.array_equal(eye, np.eye(4, dtype=np.float32))

    def at(c, r, d):
        c, r = np.asarray(c, dtype=np.float64), np.asarray(r, dtype=np.float64)
        return place(eye, intr[0], c + _off(rng, c.shape), r + _off(rng, r.shape), np.asarray(d, dtype=np.float64))

    rows = [at(rng.integers(-3, W + 3, 406), rng.integers(-3, H + 3, 406), rng.uniform(1.0, 5.0, 406))]
    rows.append(at([0, W - 1, 0, W - 1, W // 2, W // 2, 0, W - 1], [0, 0, H - 1, H - 1, 0, H - 1, H // 2, H // 2], 0.8 * np.ones(8)))
    rows.append(at([-1, W, -2, W + 1, 7, 30], [-1, H, 5, 17, -2, H + 1], 0.75 * np.ones(6)))
    rows.append(at(rng.integers(0, W, 20), rng.integers(0, H, 20), -rng.uniform(0.5, 4.0, 20)))
    rows.append(at(rng.integers(0, W, 10), rng.integers(0, H, 10), rng.uniform(1e-4, 5e-4, 10)))
    bad = at(rng.integers(0, W, 12), rng.integers(0, H, 12), 0.7 * np.ones(12))
    for i, value in enumerate([np.nan, np.inf, -np.inf] * 4):
        bad[i, i % 3] = value
    rows.append(bad)
    pc, pr_ = 3 + 4 * (np.arange(20) % 9), 4 + 6 * (np.arange(20) // 9)   # pixels of the pairs, apart from each other
    first, second = at(pc, pr_, 0.9 * np.ones(20)), at(pc, pr_, 0.9 * np.ones(20))
    assert np.array_equal(first[:, 2], second[:, 2]) and not np.array_equal(first[:, :2], second[:, :2])
    rows += [first, second]
    rows.append(rows[0][0:300:20].copy())
    xyz0 = np.concatenate(rows)
    assert xyz0.shape == (517, 3)
    garbage = at(np.arange(cap) % W, (np.arange(cap) // W) % H, 0.5 * np.ones(cap))
    garbage[::7] = np.nan
    xyz = np.stack((np.concatenate((xyz0, garbage[517:])), garbage))
    rgb = rng.integers(0, 256, size=(B, cap, 3), dtype=np.uint8)
    case = dict(xyz=xyz, rgb=rgb, count=np.array([517, 0], dtype=np.int32), poses=poses, intrinsics=intr, H=H, W=W, K=K, B=B, cap=cap)
    _CACHE["main"] = _frozen(case)
    return case


PILE_N = 4096
PILE_A, PILE_B = (3, 2), (5, 6)                                        # (column, row) of the two pixels


def pile_case():
    """An 8 x 8 image, one camera (the identity), radius 0: rows 0 .. 4095 fall on pixel PILE_A with the distinct depths
    1 + j / 4096 in shuffled order, rows 4096 .. 8191 on pixel PILE_B with ONE depth: row 4096 must win it."""
    if "pile" in _CACHE:
        return _CACHE["pile"]
    rng = np.random.default_rng(18)
    intr = intrinsics_of(9.0, 8.0, 3.6, 3.3)[None]
    eye = np.eye(4, dtype=np.float32)
    n = PILE_N
    depth = 1.0 + rng.permutation(n) / float(n)
    a = place(eye, intr[0], PILE_A[0] + _off(rng, n), PILE_A[1] + _off(rng, n), depth)
    b = place(eye, intr[0], PILE_B[0] + _off(rng, n), PILE_B[1] + _off(rng, n), 2.5 * np.ones(n))
    case = dict(xyz=np.concatenate((a, b))[None], rgb=rng.integers(0, 256, size=(1, 2 * n, 3), dtype=np.uint8),
                count=np.array([2 * n], dtype=np.int32), poses=eye[None, None], intrinsics=intr, H=8, W=8, K=1, B=1, cap=2 * n,
                nearest=int(np.argmin(depth)))
    _CACHE["pile"] = _frozen(case)
    return case


def wide_case():
    """cap = 70 000 points over a 64 x 64 image in one turned camera, for radius 2: 274 workgroups of points for the pair, and
    indices above 65 535 that win pixels."""
    if "wide" in _CACHE:
        return _CACHE["wide"]
    rng = np.random.default_rng(19)
    n, H, W = 70000, 64, 64
    intr = intrinsics_of(70.0, 66.0, 31.2, 32.7)[None]
    pose = rigid((4.0, -7.0, 3.0), (0.3, -0.2, 0.1))
    xyz = place(pose, intr[0], rng.integers(-2, W + 2, n) + _off(rng, n), rng.integers(-2, H + 2, n) + _off(rng, n),
                rng.uniform(1.0, 6.0, n))
    case = dict(xyz=xyz[None], rgb=rng.integers(0, 256, size=(1, n, 3), dtype=np.uint8), count=np.array([n], dtype=np.int32),
                poses=pose[None, None], intrinsics=intr, H=H, W=W, K=1, B=1, cap=n)
    _CACHE["wide"] = _frozen(case)
    return case


def all_cases():
    return dict(main=main_case(), pile=pile_case(), wide=wide_case())
