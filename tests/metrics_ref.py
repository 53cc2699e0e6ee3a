"""Float64 yardstick for coponerf_amd.evaluate (helper, no tests of its own: tests/test_metrics_ref.py pins it).

skimage is not a dependency, so the SSIM of `structural_similarity(win_size=11, gaussian_weights=True, channel_axis=-1,
data_range=1)` is restated here in plain numpy from its definition: `gaussian_filter(sigma=1.5, truncate=3.5,
mode="reflect")` of x, y, x x, y y, x y (an 11-tap separable window with scipy's reflect indexing, written out below and
compared with scipy's own filter in the CPU test), variances without the sample-covariance factor, C1 = 1e-4, C2 = 9e-4, the
map cropped by 5 pixels on every side, mean over the channels.

  ssim64 / mse64 / psnr64   float64 on the fp32 inputs: what the kernel is measured against
  ssim32_straight           the same in straight fp32 with uncentred moments: the reference's arithmetic on fp32 images, whose
                            distance from float64 says what fp32 alone costs on a case
  ssim32_centred            fp32 with both images shifted by -1/2 first (the kernel's form), for the comparison in DESIGN.md §4.8
  pose64                    rotation geodesic, translation distance, translation angle of (B, 4, 4) poses
  summary_ref               the list bookkeeping of the reference's evaluation script, in plain Python
  cases / make_case         the inputs of tests/test_gpu_metrics.py: pure functions of their seeds (coponerf_amd.synthetic)
"""
import math

import numpy as np

from coponerf_amd import synthetic as syn

RAD, WIN, SIGMA = 5, 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window64():
    x = np.arange(-RAD, RAD + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def reflect_index(i, n):
    """scipy.ndimage mode="reflect": d c b a | a b c d | d c b a, for any integer offset."""
    i = np.mod(i, 2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def filter2d(img, dtype=np.float64):
    """The separable window over a (H, W) image, axis 0 then axis 1, accumulated tap by tap in `dtype`."""
    g = window64().astype(dtype)
    out = np.asarray(img, dtype=dtype)
    for axis in (0, 1):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for k in range(WIN):
            acc = acc + g[k] * np.take(out, reflect_index(np.arange(n) + k - RAD, n), axis=axis)
        out = acc.astype(dtype)
    return out


def to_unit(pred, target, dtype=np.float64):
    """p = (clamp(pred, -1, 1) + 1) / 2, t = (target + 1) / 2: only the prediction is clamped, NaNs stay."""
    p = (np.clip(np.asarray(pred, dtype=dtype), -1, 1) + dtype(1)) * dtype(0.5)
    t = (np.asarray(target, dtype=dtype) + dtype(1)) * dtype(0.5)
    return p, t


def _ssim_image(p, t, dtype, shift):
    """p, t (H, W, 3) in [0, 1]."""
    c1, c2 = dtype(C1), dtype(C2)
    vals = []
    for c in range(3):
        x, y = p[..., c] - dtype(shift), t[..., c] - dtype(shift)
        ux, uy = filter2d(x, dtype), filter2d(y, dtype)
        uxx, uyy, uxy = filter2d(x * x, dtype), filter2d(y * y, dtype), filter2d(x * y, dtype)
        vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
        ux, uy = ux + dtype(shift), uy + dtype(shift)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        vals.append(s[RAD:s.shape[0] - RAD, RAD:s.shape[1] - RAD].mean(dtype=np.float64))
    return float(np.mean(vals))


def _per_image(pred, target, dtype, shift):
    pred, target = np.asarray(pred), np.asarray(target)
    assert pred.ndim == 4 and pred.shape[-1] == 3 and pred.shape == target.shape
    p, t = to_unit(pred, target, dtype)
    return np.array([_ssim_image(p[n], t[n], dtype, shift) for n in range(pred.shape[0])], dtype=np.float64)


def ssim64(pred, target):
    """(N,) float64 SSIM of (N, H, W, 3) fp32 images in the model's range."""
    return _per_image(pred, target, np.float64, 0.0)


def ssim32_straight(pred, target):
    return _per_image(pred, target, np.float32, 0.0)


def ssim32_centred(pred, target):
    return _per_image(pred, target, np.float32, 0.5)


def mse64(pred, target):
    p, t = to_unit(pred, target)
    return ((p - t) ** 2).reshape(p.shape[0], -1).mean(axis=1)


def psnr64(mse):
    with np.errstate(divide="ignore"):
        return -10.0 * np.log(np.asarray(mse, dtype=np.float64)) / math.log(10.0)


def pose64(rel_pose, gt_rel_pose):
    """(B, 3) float64: geodesic rotation distance (radians), |t - t_gt|, angle between t and t_gt (radians)."""
    a, b = np.asarray(rel_pose, dtype=np.float64), np.asarray(gt_rel_pose, dtype=np.float64)
    m = a[:, :3, :3] @ np.swapaxes(b[:, :3, :3], 1, 2)
    cos = np.clip((np.trace(m, axis1=1, axis2=2) - 1) / 2, -1, 1)
    ta, tb = a[:, :3, 3], b[:, :3, 3]
    na, nb = ta / np.linalg.norm(ta, axis=-1, keepdims=True), tb / np.linalg.norm(tb, axis=-1, keepdims=True)
    ang = np.arccos(np.clip((na * nb).sum(-1), -1, 1))
    return np.stack([np.arccos(cos), np.linalg.norm(ta - tb, axis=-1), ang], axis=-1)


# ---------------------------------------------------------------------------------------------------- bookkeeping
METRICS = ("mse", "psnr", "ssim", "rot", "trans", "angle_trans")


def bucket(overlap):
    return "large" if overlap > 0.75 else ("medium" if overlap >= 0.5 else "small")


def mean(v):
    return math.fsum(v) / len(v)


def median_index(v):
    """torch.median: the LOWER middle of the sorted values (index into v)."""
    order = sorted(range(len(v)), key=lambda i: v[i])
    return order[(len(v) - 1) // 2]


def std(v):
    """torch.std: unbiased; NaN for a single value."""
    if len(v) < 2:
        return float("nan")
    m = mean(v)
    return math.sqrt(math.fsum((x - m) ** 2 for x in v) / (len(v) - 1))


def summary_ref(rows, calls, extras=()):
    """rows: one dict per image with METRICS, "overlap" and the extras, in the order they were added; calls: the number of
    images of every add call.  Lists are kept per key the way the evaluation script keeps them - a bucket gets per-image
    values; "all" gets, per call, the pooled MSE, its PSNR, the mean SSIM / translation angle / extras, and rot and trans of
    every image - and the printed statistics are taken from them.  `<name>_median_at` is the position of the median in that
    key's list (for rot and trans of "all": among all images in order)."""
    names = METRICS + tuple(extras)
    lists = {k: {n: [] for n in names} for k in ("all", "small", "medium", "large")}
    at = 0
    for count in calls:
        rs = rows[at:at + count]
        at += count
        mse = mean([r["mse"] for r in rs])
        a = lists["all"]
        a["mse"].append(mse)
        a["psnr"].append(float(psnr64(mse)))
        a["ssim"].append(mean([r["ssim"] for r in rs]))
        a["rot"].extend(r["rot"] for r in rs)
        a["trans"].extend(r["trans"] for r in rs)
        a["angle_trans"].append(mean([r["angle_trans"] for r in rs]))
        for e in extras:
            a[e].append(mean([r[e] for r in rs]))
        for r in rs:
            if r["overlap"] is None:
                continue
            for n in names:
                lists[bucket(r["overlap"])][n].append(r[n])
    out = {}
    for key, g in lists.items():
        if not g["mse"]:
            continue
        s = {"n": len(g["mse"])}
        for n in ("psnr", "ssim", "mse") + tuple(extras):
            s[n] = mean(g[n])
        for n in ("rot", "trans", "angle_trans"):
            i = median_index(g[n])
            s[n + "_mean"], s[n + "_median"], s[n + "_median_at"], s[n + "_std"] = mean(g[n]), g[n][i], i, std(g[n])
        out[key] = s
    return out


# ---------------------------------------------------------------------------------------------------------- inputs
CASE_NAMES = ("textured", "smooth_vs_noisy", "flat", "bright", "out_of_range", "identical", "negative_covariance")
# 11 x 11: one cropped pixel.  12 x 37: odd, narrower than a 16 x 32 tile.  64 x 48: whole tiles down, ragged across.
# 41 x 75: 3 x 3 tiles, ragged in both axes.  256 x 256: the evaluation's own size (one case only).
SHAPES = ((3, 11, 11), (2, 12, 37), (1, 64, 48), (3, 41, 75))
FULL = ("textured", 2, 256, 256)


def _smooth(N, H, W, seed):
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ph = syn.uniform((N, 3, 2), seed, 0.0, 2 * math.pi, stream=9).numpy().astype(np.float64)
    out = np.empty((N, H, W, 3))
    for n in range(N):
        for c in range(3):
            out[n, ..., c] = 0.55 * np.sin(0.31 * x + 0.17 * y + ph[n, c, 0]) * np.cos(0.23 * y - 0.11 * x + ph[n, c, 1]) \
                + 0.1 * (c - 1)
    return out


def make_case(name, N, H, W, seed=0):
    """(pred, target): fp32 (N, H, W, 3) numpy arrays in the model's range [-1, 1] (some cases leave it on purpose)."""
    shape = (N, H, W, 3)
    seed = seed * 131 + CASE_NAMES.index(name) * 17 + H * 7 + W
    noise = lambda std, stream: syn.normal(shape, seed, std, stream=stream).numpy().astype(np.float64)
    textured = _smooth(N, H, W, seed) + noise(0.08, 1)
    if name == "textured":
        target, pred = textured, textured + noise(0.05, 2)
    elif name == "smooth_vs_noisy":
        target, pred = _smooth(N, H, W, seed), syn.uniform(shape, seed, -1.0, 1.0, stream=3).numpy()
    elif name == "flat":                                    # the cancellation case: variances of 1e-6 under means of 0.7
        pred = np.full(shape, 0.4)
        target = pred + noise(2e-3, 2)
    elif name == "bright":
        target = np.ones(shape)
        pred = 1.0 - syn.uniform(shape, seed, 0.0, 0.03, stream=3).numpy()
    elif name == "out_of_range":
        target, pred = textured.copy(), textured + noise(0.05, 2)
        u = syn.uniform(shape, seed, 0.0, 1.0, stream=4).numpy()
        far = syn.uniform(shape, seed, 1.0, 1.6, stream=5).numpy()
        pred = np.where(u < 0.05, far, np.where(u < 0.10, -far, pred))             # 10 % outside, both sides
        target = np.where((u > 0.5) & (u < 0.53), 1.25 * np.sign(target + 1e-9), target)   # 3 % outside: NOT clamped
    elif name == "identical":
        target = np.clip(textured, -0.95, 0.95)
        pred = target
    elif name == "negative_covariance":                     # p = 1 - t in image range is pred = -target in the model's
        target = textured
        pred = -np.asarray(textured, dtype=np.float32).astype(np.float64)
    else:
        raise KeyError(name)
    target = np.ascontiguousarray(target, dtype=np.float32)
    pred = target.copy() if name == "identical" else np.ascontiguousarray(pred, dtype=np.float32)
    return pred, target


def cases():
    """[(id, name, N, H, W)]: every case at every small shape, and the one full-size case."""
    out = [(f"{name}-{N}x{H}x{W}", name, N, H, W) for (N, H, W) in SHAPES for name in CASE_NAMES]
    name, N, H, W = FULL
    out.append((f"{name}-{N}x{H}x{W}", name, N, H, W))
    return out
