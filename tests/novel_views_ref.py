"""Yardsticks of coponerf_amd/novel_views.py (csrc/novel_views.hip) and the inputs of its tests: float64 or integer restatements
of the three rules, and the fp32 bounds, derived here from operation counts - none from a run.

  axis_weights(...)   the resample rule of one axis as a dense (n_out, n_in) float64 matrix, and its largest tap count
  fit64(...)          crop, resample, `v / 127.5 - 1` of uint8 photos in float64
  fit_bound(...)      what cpn_fit_images_u8 may differ from fit64 by
  path64(...)         the camera path in float64 (numpy)
  path_bound(...)     U max(1, |entry|): the fp32 store
  pack_rule(...)      the byte pack in numpy float32, operation by operation
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from coponerf_amd import synthetic as syn
from coponerf_amd.shards import crop_window
from coponerf_amd.summaries import jet_table

U = 2.0 ** -24                                              # unit roundoff of fp32
SEED = 131

# ((Hi, Wi), size) of the GPU tests: identity | odd sizes, crop side 36, scale 2.25 | upsampling, crop 8 | upstream's own
# frames | scale 21.9, over 40 taps per axis
FIT_CASES = (((16, 16), 16), ((37, 53), 16), ((9, 12), 16), ((360, 640), 256), ((1000, 700), 32))


# ----------------------------------------------------------------------------------------------------------- the resample
def axis_weights(n_in, n_out, antialias):
    """((n_out, n_in) float64 W, T): row i holds the normalised weights of output i - taps
    j in [max(trunc(c - sup + 0.5), 0), min(trunc(c + sup + 0.5), n_in)), weight max(0, 1 - |j + 0.5 - c| / sup),
    c = (i + 0.5) n_in / n_out, sup = max(n_in / n_out, 1) (1 without antialias) - and T the largest number of taps of a row."""
    scale = n_in / n_out
    sup = max(scale, 1.0) if antialias else 1.0
    W = np.zeros((n_out, n_in))
    T = 0
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
        j = np.arange(lo, hi)
        w = np.maximum(0.0, 1.0 - np.abs(j + 0.5 - c) / sup)
        W[i, lo:hi] = w / w.sum()
        T = max(T, hi - lo)
    return W, T


def crop(img):
    """utils_training/data_util.py:116-121 on (..., Hi, Wi, 3)."""
    y0, x0, side = crop_window(img.shape[-3], img.shape[-2])
    return img[..., y0:y0 + side, x0:x0 + side, :]


def resample64(img_u8, size, antialias):
    """(B, size, size, 3) float64 grey levels of (B, Hi, Wi, 3) uint8 photos: the crop, then both axes of the rule."""
    x = crop(np.asarray(img_u8)).astype(np.float64)
    W, _ = axis_weights(x.shape[1], size, antialias)
    rows = np.tensordot(W, x, axes=(1, 1))                  # (o, b, x, c)
    return np.tensordot(rows, W, axes=(2, 1)).transpose(1, 0, 3, 2)       # (o, b, c, p) -> (b, o, p, c)


def fit64(img_u8, size, antialias):
    return resample64(img_u8, size, antialias) / 127.5 - 1.0


def interpolate64(img_u8, size, antialias):
    """The yardstick of the rule: F.interpolate in float64 on the cropped photo, grey levels."""
    x = torch.from_numpy(crop(np.asarray(img_u8)).astype(np.float64)).permute(0, 3, 1, 2)
    y = F.interpolate(x, size=(size, size), mode="bilinear", antialias=antialias, align_corners=False)
    return y.permute(0, 2, 3, 1).numpy()


def _gamma(n):
    return n * U / (1.0 - n * U)


def fit_bound(Hi, Wi, size, antialias):
    """|cpn_fit_images_u8 - fit64| per element, in the output's units.

    One pass forms, for T taps of values in [0, 255], acc = sum w_j v_j and ws = sum w_j in fp32 and divides.  Each weight is
    a float64 value rounded to fp32 once (1 rounding; the float64 formation itself errs by a few 2^-53 n_in, the FLOAT64 term
    below).  A term of acc carries that rounding, its product and at most T - 1 additions: T + 1 roundings; a term of ws the
    weight's rounding and T - 1 additions: T.  The quotient of two sums of non-negative terms whose terms are off by relative
    (T + 1) U and T U lies within (2 T + 1) U of the exact weighted mean, relative to a mean <= 255; the division rounds once
    more: 2 T + 2.  The second pass is a weighted mean too - it passes the first pass's error on with a factor <= 1 and adds
    its own: 2 (T_y + T_x) + 4 roundings relative to 255 grey levels, taken as gamma(n) = n U / (1 - n U) for the higher-order
    terms.  v / 127.5 - 1 turns a grey level into 1 / 127.5, and rounds a quotient <= 2 and a difference <= 1: 3 U."""
    side = crop_window(Hi, Wi)[2]
    _, T = axis_weights(side, size, antialias)
    float64_term = 2 * T * 8 * side * 2.0 ** -53 * 255.0
    grey = 255.0 * _gamma(4 * T + 4) + float64_term
    return grey / 127.5 * (1 + U) + 3 * U


@functools.lru_cache(maxsize=None)
def fit_case(Hi, Wi, size, B=3):
    """(noise (B, Hi, Wi, 3) uint8, constant (B, Hi, Wi, 3) uint8 - grey level 201, 7, 128 per image -, and the float64 results
    {(kind, antialias): (B, size, size, 3)}): computed once, shared, never written to."""
    n = B * Hi * Wi * 3
    noise = (syn._bits(n, SEED, Hi * 4096 + Wi) >> np.uint64(56)).astype(np.uint8).reshape(B, Hi, Wi, 3)
    const = np.empty_like(noise)
    for b in range(B):
        const[b] = (201, 7, 128)[b % 3]
    ref = {(kind, aa): fit64(img, size, aa) for kind, img in (("noise", noise), ("const", const)) for aa in (True, False)}
    for a in (noise, const, *ref.values()):
        a.setflags(write=False)
    return noise, const, ref


# --------------------------------------------------------------------------------------------------------------- the path
def rotation_about(axis, angle):
    """(3, 3) float64 rotation by `angle` about `axis` (Rodrigues)."""
    n = np.asarray(axis, dtype=np.float64)
    n = n / np.linalg.norm(n)
    N = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
    return np.eye(3) + np.sin(angle) * N + (1 - np.cos(angle)) * (N @ N)


def power_of_rotation(R, t):
    """exp(t log R) of one (3, 3) float64 matrix: the identity below an angle of 1e-12 and at t == 0, R itself at t == 1; up to
    a quarter turn the axis is the antisymmetric part's, beyond it that of the symmetric part (R + R^T) / 2 = cos I +
    (1 - cos) n n^T, with the sign of what is left of the antisymmetric one."""
    if t == 1.0:
        return R.copy()
    if t == 0.0:
        return np.eye(3)
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.sqrt(a @ a)
    cs = min(max(0.5 * (np.trace(R) - 1.0), -1.0), 1.0)
    theta = np.arctan2(s, cs)
    if theta < 1e-12:
        return np.eye(3)
    if cs >= 0.0:
        n = a / (2.0 * s)
    else:
        M = (0.5 * (R + R.T) - cs * np.eye(3)) / (1.0 - cs)
        m = int(np.argmax(np.diag(M)))
        n = M[:, m] / np.sqrt(M[m, m])
        n = n / np.linalg.norm(n) * (-1.0 if n @ a < 0.0 else 1.0)
    return rotation_about(n, t * theta)


def path64(rel_pose, t, sway=0.0, turns=2.0):
    """(K, B, 4, 4) float64: pose k of pair b is [exp(t_k log R) | t_k p] of rel_pose[b] = [R | p], plus, with sway > 0,
    R_k sway (cos(2 pi turns t_k), sin(2 pi turns t_k), 0)."""
    rel = np.asarray(rel_pose, dtype=np.float64)
    ts = np.asarray(t, dtype=np.float64).reshape(-1)
    out = np.zeros((len(ts), rel.shape[0], 4, 4))
    out[:, :, 3, 3] = 1.0
    for k, tk in enumerate(ts):
        for b in range(rel.shape[0]):
            Q = power_of_rotation(rel[b, :3, :3], float(tk))
            p = tk * rel[b, :3, 3]
            if sway > 0.0:
                ph = 2.0 * np.pi * turns * tk
                p = p + Q @ np.array([sway * np.cos(ph), sway * np.sin(ph), 0.0])
            out[k, b, :3, :3], out[k, b, :3, 3] = Q, p
    return out


def path_bound(ref):
    """The kernel computes in float64 and rounds each entry to fp32 once: U max(1, |entry|) per entry (the store itself is
    half of that; the rest covers float64 libraries that differ in the last places)."""
    return U * np.maximum(1.0, np.abs(ref))


def path_poses():
    """(3, 4, 4) fp32 rel_pose of the GPU test: angles 0, 0.3 and pi - 1e-4 about three different axes."""
    rel = np.tile(np.eye(4), (3, 1, 1))
    rel[1, :3, :3] = rotation_about((0.2, 1.0, -0.3), 0.3)
    rel[2, :3, :3] = rotation_about((1.0, -0.4, 0.7), np.pi - 1e-4)
    rel[:, :3, 3] = ((0.3, -0.05, 0.02), (-0.25, 0.06, 0.4), (1.5, 0.2, -0.7))
    return rel.astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- the pack
def to_byte(v):
    """rint(min(max(v, 0), 255)) of float32 grey levels, NaN -> 0 (np.fmax / np.fmin return the operand that is a number)."""
    v = np.asarray(v, dtype=np.float32)
    return np.rint(np.fmin(np.fmax(v, np.float32(0)), np.float32(255))).astype(np.uint8)


def pack_rule(rgb, h, w, depth=None):
    """(B, h, w, 3) uint8 of rgb (B, h * w, 3) float32, or (B, h, 2 w, 3) with depth (B, h * w): every operation one float32
    rounding.  The depth panel is matplotlib's lookup (tests/summaries_ref.jet_lookup) in the fp32 table, times 255."""
    rgb = np.asarray(rgb, dtype=np.float32)
    B = rgb.shape[0]
    left = to_byte((rgb.reshape(B, h, w, 3) + np.float32(1)) * np.float32(127.5))
    if depth is None:
        return left
    xa = (np.asarray(depth, dtype=np.float32).reshape(B, h, w) / np.float32(10)) * np.float32(256)
    with np.errstate(invalid="ignore"):
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, xa.astype(np.int64)))
    colours = jet_table().astype(np.float32)[np.where(np.isnan(xa), 0, idx)]
    colours[np.isnan(xa)] = 0.0
    return np.concatenate((left, to_byte(colours * np.float32(255))), axis=2)


def pack_values():
    """float32 inputs of the pack test: out of range both ways, NaN, both zeros, infinities, and every x of a fine scan whose
    (x + 1) * 127.5 is EXACTLY k + 0.5 in float32 (x = 0 -> 127.5 is one; rint takes such ties to the even byte)."""
    special = np.array([-1.5, 1.5, np.nan, 0.0, -0.0, np.inf, -np.inf, -1.0, 1.0, 1.0 / 127.5 - 1.0], dtype=np.float32)
    k = np.arange(0, 255, dtype=np.float64) + 0.5
    cand = (k / 127.5 - 1.0).astype(np.float32)
    cand = np.concatenate([np.nextafter(cand, np.float32(-2)), cand, np.nextafter(cand, np.float32(2))])
    g = (cand + np.float32(1)) * np.float32(127.5)
    ties = cand[g - np.floor(g) == np.float32(0.5)]
    return special, ties
