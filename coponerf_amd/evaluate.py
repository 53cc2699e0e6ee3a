"""The reference's evaluation metrics (test.py:222-300), kept on the device.

test.py turns every rendered validation pair into numbers on the host: five `.item()` reads, two images copied to numpy,
`skimage.metrics.structural_similarity` twice on the CPU, and Python lists that `np.mean` / `torch.median` walk after every
pair.  Here

  image_metrics   MSE, PSNR and the 11-tap gaussian SSIM of N images: csrc/image_metrics.hip, 2 launches      test.py:227-229, 246-253, 267
  pose_metrics    rotation geodesic, translation distance, translation angle: stock ops on (B, 4, 4)         test.py:34-48, 232-243
  Evaluator       one row per image in a device-resident table; `summary()` makes the ONE host read and      test.py:160, 271-300
                  returns the statistics of the reference's printed line for "all" / "small" / "medium" / "large"

`Evaluator.add` reads no device value on the host and copies no pageable host memory, so it can follow
`pipeline.render_images` without stalling it.  LPIPS (test.py:149, 258-263) is `coponerf_amd.lpips.LPIPS`, on
the user's own weight files (none are part of this package): `Evaluator(extra={"lpips": LPIPS.from_files(...).to(dev)})` adds
its column, and `extra` takes any other callable `fn(pred, target) -> (N,)` the same way.

`Evaluator(geometry={...})` (round 25) also scores every pose `matches.from_flows` returns - the refined, RANSAC's,
the homography's, the selected one - against the ground truth in float64 (csrc/pose_eval.hip: cpn_pose_errors), measures the matches'
residuals under the true pose (cpn_residual_stats) and summarises each source by `pose_auc`.  Without the keyword nothing changes.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import _hip

COLUMNS = ("mse", "psnr", "ssim", "rot", "trans", "angle_trans", "overlap", "call")
BUCKETS = ("small", "medium", "large")
# Evaluator(geometry=...): the poses from_flows can return, in the order of their columns; what is measured of the matches; the
# labels of select_pose's `model` (0, 1, 2; -1 is "none"); the thresholds of the AUC in degrees
SOURCES = ("network", "refined", "ransac", "homography", "select", "adjusted")
QUALITY = ("matches", "usable_gt", "med_gt", "in_gt", "sigma_gt", "med_network", "in_network")
MODELS = ("E", "plane", "rotation")
AUC_AT = (5, 10, 20)
_GEOMETRY_KEYS = ("S", "refine", "max_cycle_px", "max_epi_px", "stride", "iters", "scale_px", "ransac", "homography", "select",
                  "triangulate", "inlier_px")
WIN = 11                                                  # structural_similarity(win_size=11): the smallest image side


def _check(pred: torch.Tensor, target: torch.Tensor, image_shape: Optional[Sequence[int]]) -> Tuple[int, int, int]:
    if not (torch.is_tensor(pred) and torch.is_tensor(target)):
        raise TypeError("image_metrics: pred and target must be tensors")
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("image_metrics runs on the HIP device only (coponerf_amd has no non-HIP compute path)")
    if pred.device != target.device:
        raise ValueError(f"image_metrics: pred is on {pred.device}, target on {target.device}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"image_metrics: fp32 tensors only, got {pred.dtype} and {target.dtype}")
    if not (pred.is_contiguous() and target.is_contiguous()):
        raise ValueError("image_metrics: pred and target must be contiguous (N, H, W, 3) images, or views of them")
    if pred.dim() < 1 or pred.shape[-1] != 3 or target.dim() < 1 or target.shape[-1] != 3:
        raise ValueError(f"image_metrics: channels last, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if image_shape is None:
        if pred.dim() != 4:
            raise ValueError(f"image_metrics: pass image_shape=(H, W) for a tensor of shape {tuple(pred.shape)}")
        image_shape = pred.shape[1:3]
    H, W = int(image_shape[0]), int(image_shape[1])
    if H < WIN or W < WIN:
        raise ValueError(f"image_metrics: the {WIN}-tap SSIM window needs H, W >= {WIN}, got {H} x {W}")
    per = H * W * 3
    if pred.numel() == 0 or pred.numel() % per or pred.numel() != target.numel():
        raise ValueError(f"image_metrics: {tuple(pred.shape)} and {tuple(target.shape)} are not the same number of "
                         f"{H} x {W} x 3 images")
    return pred.numel() // per, H, W


def image_metrics(pred: torch.Tensor, target: torch.Tensor, image_shape: Optional[Sequence[int]] = None) -> torch.Tensor:
    """(N, 3) fp32 on the device: mse, psnr (dB), ssim of every image, as test.py:227-229, 246-253, 267 compute them.

    pred, target: contiguous fp32 (N, H, W, 3) in the model's range [-1, 1], or any contiguous view of that memory such as
    the (B, 1, H*W, 3) of `forward(val=True)['rgb']` and `gt['rgb']` with image_shape=(H, W).  Only the prediction is clamped;
    a NaN sample makes its image's three values NaN.  Bit-reproducible, and an image's values do not depend on N."""
    N, H, W = _check(pred, target, image_shape)
    n = _hip.lib().cpn_image_metrics_scratch(N, H, W)
    if n <= 0:
        raise ValueError(f"image_metrics: {N} images of {H} x {W} are too many for one launch")
    partial = torch.empty(n, dtype=torch.float32, device=pred.device)
    out = torch.empty(N, 3, dtype=torch.float32, device=pred.device)
    with torch.cuda.device(pred.device):
        _hip.call("cpn_image_metrics", pred.data_ptr(), target.data_ptr(), N, H, W, partial.data_ptr(), out.data_ptr(),
                  _hip.stream_handle())
    return out


def pose_metrics(rel_pose: torch.Tensor, gt_rel_pose: torch.Tensor) -> torch.Tensor:
    """(B, 3): rotation geodesic in RADIANS (the reference calls it `rot_distance_degrees`; acos returns radians and nothing
    converts them - test.py:34-48, 232), translation distance (test.py:235) and the angle between the two translation
    directions in radians (test.py:238-243).  rel_pose, gt_rel_pose: (B, 4, 4) on the device."""
    if rel_pose.dim() != 3 or tuple(rel_pose.shape[1:]) != (4, 4) or rel_pose.shape != gt_rel_pose.shape:
        raise ValueError(f"pose_metrics: two (B, 4, 4) poses, got {tuple(rel_pose.shape)} and {tuple(gt_rel_pose.shape)}")
    if not (rel_pose.is_cuda and gt_rel_pose.is_cuda):
        raise RuntimeError("pose_metrics runs on the HIP device only (coponerf_amd has no non-HIP compute path)")
    m = torch.bmm(rel_pose[:, :3, :3], gt_rel_pose[:, :3, :3].transpose(1, 2))
    cos = (m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2
    rot = torch.acos(cos.clamp(-1.0, 1.0))
    tp, tg = rel_pose[:, :3, 3], gt_rel_pose[:, :3, 3]
    trans = torch.linalg.norm(tp - tg, dim=-1)
    npred = tp / torch.linalg.norm(tp, dim=-1, keepdim=True)
    ngt = tg / torch.linalg.norm(tg, dim=-1, keepdim=True)
    angle = torch.acos((npred * ngt).sum(-1).clamp(-1.0, 1.0))
    return torch.stack((rot, trans, angle), dim=-1)


def bucket_of(overlap: float) -> Optional[str]:
    """test.py:271-272; None for an image that came without an overlap."""
    if overlap != overlap:
        return None
    return "large" if overlap > 0.75 else ("medium" if overlap >= 0.5 else "small")


def _stats(values: Sequence[float]) -> Dict[str, float]:
    """torch.mean / torch.median (the lower middle) / torch.std (unbiased; NaN for one value) of fp32 values, as the reference
    takes them of its fp32 lists.  `rot` and `trans` are fp32 already; the "all" group's `angle_trans` entries are per-call
    means formed in float64 and rounded to fp32 here, half an ulp from the reference's own fp32 mean."""
    t = torch.tensor(list(values), dtype=torch.float32)
    return {"mean": float(t.mean()), "median": float(t.median()), "std": float(t.std()) if t.numel() > 1 else float("nan")}


def _mean(values: Sequence[float]) -> float:
    return math.fsum(values) / len(values)                 # np.mean of Python floats, without its rounding


def _stats64(values: Sequence[float]) -> Dict[str, float]:
    """_stats of float64 values, kept in float64: the rot64 / angle64 columns resolve what fp32 would round away."""
    t = torch.tensor(list(values), dtype=torch.float64)
    return {"mean": float(t.mean()), "median": float(t.median()), "std": float(t.std()) if t.numel() > 1 else float("nan")}


def _nanmean(values: Sequence[float]) -> float:
    """The mean of the values that are numbers; NaN where none is."""
    kept = [v for v in values if v == v]
    return _mean(kept) if kept else float("nan")


def pose_auc(errors: Sequence[float], thresholds: Sequence[float] = AUC_AT) -> List[float]:
    """The area under the recall curve of `errors` up to each threshold, normalised by the threshold: the pose literature's
    exact trapezoid over the sorted errors - the curve runs through (0, 0) and (e_i, i / n) for the i-th smallest error and is
    cut at the threshold with the recall of the last error below it.  A NaN error is a miss: it counts in n and is never
    recalled.  Host, float64."""
    errs = sorted(float("inf") if e != e else float(e) for e in errors)
    n = len(errs)
    out = []
    for t in thresholds:
        xs, ys = [0.0], [0.0]
        for i, e in enumerate(errs):
            if not e < t:
                break
            xs.append(e)
            ys.append((i + 1) / n)
        xs.append(float(t))
        ys.append(ys[-1])
        out.append(math.fsum((xs[i + 1] - xs[i]) * (ys[i + 1] + ys[i]) / 2.0 for i in range(len(xs) - 1)) / t if n else float("nan"))
    return out


def _to_device(obj, dev):
    if torch.is_tensor(obj):
        return obj if obj.device == dev else obj.to(dev, non_blocking=True)
    if isinstance(obj, dict):
        return {k: _to_device(v, dev) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_device(v, dev) for v in obj)
    return obj


class Evaluator:
    """The bookkeeping of test.py:160, 222-300 as one device-resident table.

        ev = Evaluator()
        ev.run(model, val_loader, nchunks=18)        # or ev.add(model_output, gt, overlap) per rendered batch
        print(ev.format_summary())

    A row per image: COLUMNS, then one column per entry of `extra`.  The table is float64 (fp32 metrics, overlaps and call
    indices are all exact in it), preallocated at `capacity` rows and doubled when it fills.  `host_reads` counts the device
    -> host reads made here: `add` and `run` make none, `summary`, `format_summary` and `rows(host=True)` one each.

    geometry: None, or a dict of matches.from_flows' own keywords (S, refine, max_cycle_px, max_epi_px, stride, iters, scale_px,
    ransac, homography, select, triangulate) and `inlier_px` (1.0).  `add` then needs `intrinsics`, runs from_flows on the batch's flows and
    pose and scores EVERY pose it returns against the ground truth - `self.sources`, of SOURCES: network, refined (unless
    refine=False), ransac, homography, select, and adjusted: with `triangulate` = a dict of `pose` and `adjust` (from_flows' own),
    bundle adjustment's pose from that pose (round 27) - in float64: per source s the columns `rot64_s`, `trans64_s`, `angle64_s`
    (matches.pose_errors: radians and scene units, as the built-in ones), then QUALITY: `matches` (the pair's count), and of the
    matches' Sampson residuals under the GROUND-TRUTH pose `usable_gt`, `med_gt` (the median |r| in pixels), `in_gt` (the share
    within inlier_px), `sigma_gt` (matches.residual_stats' sigma[1]), under the network's pose `med_network`, `in_network`; with
    select `model`, select_pose's label.  Two more launches beside from_flows' own and still no host read.  Without the keyword
    nothing changes: no launch, no column, no key."""

    def __init__(self, extra: Optional[Dict[str, Callable]] = None, capacity: int = 256, device=None,
                 geometry: Optional[Dict] = None):
        self.extra: Dict[str, Callable] = dict(extra or {})
        for name in self.extra:
            if name in COLUMNS:
                raise ValueError(f"Evaluator: extra metric {name!r} collides with a built-in column")
        self.columns: Tuple[str, ...] = COLUMNS + tuple(self.extra)
        self.geometry: Optional[Dict] = None
        self.sources: Tuple[str, ...] = ()
        if geometry is not None:
            if not isinstance(geometry, dict):
                raise ValueError(f"Evaluator: geometry must be None or a dict of from_flows' keywords and inlier_px, got "
                                 f"{type(geometry).__name__}")
            unknown = set(geometry) - set(_GEOMETRY_KEYS)
            if unknown:
                raise ValueError(f"Evaluator: geometry holds unknown keywords {sorted(unknown)}; it takes {_GEOMETRY_KEYS}")
            self.geometry = dict(geometry)
            self._inlier_px = float(self.geometry.pop("inlier_px", 1.0))
            if not 0.0 <= self._inlier_px < float("inf"):
                raise ValueError(f"Evaluator: geometry['inlier_px'] must be finite and >= 0, got {geometry['inlier_px']}")
            on = {"network": True, "refined": bool(self.geometry.get("refine", True))}
            on.update({k: self.geometry.get(k) is not None for k in ("ransac", "homography", "select")})
            tri = self.geometry.get("triangulate")
            if tri is not None and not (isinstance(tri, dict) and tri.get("adjust") is not None):
                raise ValueError("Evaluator: geometry['triangulate'] is taken for its `adjust` alone: a dict of `pose` and `adjust`")
            on["adjusted"] = tri is not None
            self.sources = tuple(s for s in SOURCES if on[s])
            names = tuple(f"{c}_{s}" for s in self.sources for c in ("rot64", "trans64", "angle64")) + QUALITY
            names += ("model",) if on["select"] else ()
            clash = set(names) & set(self.columns)
            if clash:
                raise ValueError(f"Evaluator: extra metrics {sorted(clash)} collide with the geometry columns")
            self.columns += names
        self._capacity = max(1, int(capacity))
        self._device = torch.device(device) if device is not None else None
        self._table: Optional[torch.Tensor] = None
        self._n = 0
        self._calls = 0
        self.host_reads = 0

    def __len__(self) -> int:
        return self._n

    # ------------------------------------------------------------------------------------------------------ the table
    def _reserve(self, rows: int, dev) -> None:
        if self._table is None:
            self._device = self._device or dev
            while self._capacity < rows:
                self._capacity *= 2
            self._table = torch.empty(self._capacity, len(self.columns), dtype=torch.float64, device=self._device)
        elif self._n + rows > self._capacity:
            while self._capacity < self._n + rows:
                self._capacity *= 2
            grown = torch.empty(self._capacity, len(self.columns), dtype=torch.float64, device=self._device)
            grown[:self._n] = self._table[:self._n]
            self._table = grown

    @staticmethod
    def _overlap_column(overlap, B: int, dev) -> Optional[torch.Tensor]:
        if overlap is None:
            return None
        if torch.is_tensor(overlap):
            ov = overlap.detach().reshape(-1)
            if not ov.is_cuda:                              # a loader's CPU tensor: pinned, so the copy does not wait
                ov = ov.to(torch.float64).pin_memory().to(dev, non_blocking=True)
        else:
            overlap = list(overlap)
            if any(torch.is_tensor(v) and v.is_cuda for v in overlap):     # float() of each would be a host read per image
                raise TypeError("Evaluator.add: overlap holds device tensors; pass one tensor of length B, or host numbers")
            ov = torch.tensor([float(v) for v in overlap], dtype=torch.float64).pin_memory().to(dev, non_blocking=True)
        if ov.numel() != B:
            raise ValueError(f"Evaluator.add: {ov.numel()} overlaps for {B} images")
        return ov

    @torch.no_grad()
    def add(self, model_output: Dict, gt_rgb, overlap=None, image_shape: Optional[Sequence[int]] = None,
            intrinsics: Optional[torch.Tensor] = None) -> None:
        """One rendered batch (test.py:222-296): `model_output` is the joined dict of `forward(val=True)` / `render_images`
        ('rgb', 'rel_pose', 'gt_rel_pose'), `gt_rgb` the ground truth (gt['rgb'], or the gt dict itself), `overlap` one value
        per image (host sequence, tensor, or None: then the images join no bucket).  image_shape=(H, W); None takes a 4-D
        (B, H, W, 3) shape as it is and a (B, 1, R, 3) one as square.  With `geometry`, model_output['flow'] and intrinsics
        (B, 2, 4, 4), `context.intrinsics`, are needed as well.  Enqueues device work only."""
        if self.geometry is not None and intrinsics is None:
            raise ValueError("Evaluator.add: geometry needs intrinsics=model_input['context']['intrinsics']")
        rgb = model_output["rgb"].contiguous()              # as forward() and the chunk join return it: no copy
        gt = (gt_rgb["rgb"] if isinstance(gt_rgb, dict) else gt_rgb).contiguous()
        rel, gt_rel = model_output["rel_pose"], model_output["gt_rel_pose"]
        B = int(rel.shape[0])
        if image_shape is None and not (rgb.dim() == 4 and rgb.shape[1] > 1):
            side = math.isqrt(rgb.numel() // (3 * B)) if B else 0
            if side * side * 3 * B != rgb.numel():
                raise ValueError(f"Evaluator.add: pass image_shape=(H, W) for rgb of shape {tuple(rgb.shape)}")
            image_shape = (side, side)
        N, H, W = _check(rgb, gt, image_shape)
        if N != B:
            raise ValueError(f"Evaluator.add: {N} images of {H} x {W} but {B} poses")
        dev = rgb.device
        ov = self._overlap_column(overlap, B, dev)
        self._reserve(B, dev)
        rows = self._table[self._n:self._n + B]
        rows[:, 0:3] = image_metrics(rgb, gt, (H, W))
        rows[:, 3:6] = pose_metrics(rel, gt_rel)
        if ov is None:
            rows[:, 6].fill_(float("nan"))
        else:
            rows[:, 6] = ov
        rows[:, 7].fill_(float(self._calls))
        if self.extra:
            # test.py:258-259: both images back in [-1, 1], channels first; the prediction is the clamped one
            p = rgb.view(B, H, W, 3).clamp(-1, 1).permute(0, 3, 1, 2)
            t = gt.view(B, H, W, 3).permute(0, 3, 1, 2)
            for j, fn in enumerate(self.extra.values()):
                rows[:, len(COLUMNS) + j] = torch.as_tensor(fn(p, t), device=dev).reshape(B)
        if self.geometry is not None:
            self._add_geometry(rows, model_output["flow"], rel, gt_rel, intrinsics)
        self._n += B
        self._calls += 1

    def _add_geometry(self, rows: torch.Tensor, flow, rel: torch.Tensor, gt_rel: torch.Tensor, intrinsics: torch.Tensor) -> None:
        """The geometry columns of a batch: from_flows, ONE cpn_pose_errors on the stack of its poses, ONE cpn_residual_stats on
        (ground truth, network)."""
        from . import matches as mt
        flows = (flow[0].float().contiguous(), flow[1].float().contiguous())
        K, rel, gt_rel = intrinsics.float().contiguous(), rel.float().contiguous(), gt_rel.float().contiguous()
        found = mt.from_flows(flows, K, rel, **self.geometry)
        pose = {"network": rel, "refined": found["pose"]}
        pose.update({k: found[k]["pose"] for k in ("ransac", "homography", "select") if k in found})
        if "adjust" in found:
            pose["adjusted"] = found["adjust"]["pose"]
        errs = mt.pose_errors(torch.stack([pose[s] for s in self.sources], dim=1).contiguous(), gt_rel)
        at = len(COLUMNS) + len(self.extra)
        rows[:, at:at + 3 * len(self.sources)] = errs.reshape(errs.shape[0], -1)
        at += 3 * len(self.sources)
        st = mt.residual_stats(found["matches"], K, torch.stack((gt_rel, rel), dim=1).contiguous(), q=(0.5,),
                               thresholds=(self._inlier_px,))
        share = st["within"][:, :, 0].to(torch.float64) / st["usable"].to(torch.float64)          # 0 / 0: NaN
        for j, col in enumerate((found["matches"].count, st["usable"][:, 0], st["quant"][:, 0, 0], share[:, 0], st["sigma"][:, 0, 1],
                                 st["quant"][:, 1, 0], share[:, 1])):
            rows[:, at + j] = col
        if "select" in found:
            rows[:, at + len(QUALITY)] = found["select"]["model"]

    @torch.no_grad()
    def run(self, model, loader: Iterable, nchunks: Optional[int] = None, image_shape: Optional[Sequence[int]] = None,
            summary_log=None, **render_images_kwargs) -> "Evaluator":
        """test.py:161-296 over a validation loader that yields (model_input, gt, overlap) triples
        (data/realestate10k_dataio.py:683): every batch rendered through `pipeline.render_images` (nchunks=18 is test.py's own
        chunking) and added.  Tensors still on the host are moved to the model's device first, as utils.dict_to_gpu does.
        summary_log: a `summaries.SummaryLog`; every batch is also logged through it (test.py:270), under the index of its
        `add` call as the step.  The caller flushes it."""
        from .pipeline import render_images
        dev = next(model.parameters()).device
        pending: deque = deque()

        def inputs():
            for model_input, gt, overlap in loader:
                pending.append((_to_device(gt, dev), overlap))
                yield _to_device(model_input, dev)

        for model_input, out in render_images(model, inputs(), nchunks=nchunks, **render_images_kwargs):
            gt, overlap = pending.popleft()
            if summary_log is not None:
                summary_log.add(model_input, out, self._calls, image_shape=image_shape)
            self.add(out, gt, overlap, image_shape=image_shape,
                     intrinsics=model_input["context"]["intrinsics"] if self.geometry is not None else None)
        return self

    # ------------------------------------------------------------------------------------------------- reading it back
    def rows(self, host: bool = False) -> torch.Tensor:
        """The (images, len(columns)) float64 table: on the device (a copy; no host read), or with host=True on the CPU.
        Before the first `add` it is empty, on the device the Evaluator was given (on the CPU if it was given none)."""
        if self._table is None:                             # nothing added yet: no device is known unless one was given
            return torch.empty(0, len(self.columns), dtype=torch.float64, device=None if host else self._device)
        t = self._table[:self._n]
        if host:
            self.host_reads += 1
            return t.cpu()
        return t.clone()

    def summary(self) -> Dict[str, Dict[str, float]]:
        """{"all" | "small" | "medium" | "large": statistics}: what test.py:298-300 prints, from one host read.

        Every group has `n`, mean `psnr` / `ssim` / `mse`, `{rot,trans,angle_trans}_{mean,median,std}` and a mean per extra.
        A bucket (test.py:271-272 by the image's overlap) holds per-image values.  "all" follows test.py:246-280 per `add`
        call: the MSE pooled over the call's images, the PSNR of that pooled MSE, the call's mean SSIM, translation angle and
        extras, and `rot` / `trans` per image.  Groups without entries are omitted.
        With `geometry` every group gains, from its images one by one (in "all" too), per source s
        `{rot64,angle64}_s_{mean,median,std}` in float64 and `auc5_s`, `auc10_s`, `auc20_s` - pose_auc of max(rot64_s, angle64_s)
        in degrees -, the mean of every QUALITY column over the images where it is a number, and with select `model_E`,
        `model_plane`, `model_rotation`, `model_none`: the share of each label."""
        table = self.rows(host=True).tolist()
        c = {name: i for i, name in enumerate(self.columns)}
        groups: Dict[str, Dict[str, List[float]]] = {}

        def push(key: str, **values) -> None:
            g = groups.setdefault(key, {})
            for k, v in values.items():
                g.setdefault(k, []).extend(v if isinstance(v, list) else [v])

        calls: Dict[int, List[List[float]]] = {}
        for r in table:
            calls.setdefault(int(r[c["call"]]), []).append(r)
            key = bucket_of(r[c["overlap"]])
            if key is not None:
                push(key, **{name: r[c[name]] for name in self.columns if name not in ("overlap", "call")})
        for idx in sorted(calls):
            rs = calls[idx]
            mse = _mean([r[c["mse"]] for r in rs])          # equal-sized images: the mean over all their samples
            psnr = -10.0 * math.log10(mse) if mse > 0 else (float("inf") if mse == 0 else float("nan"))
            push("all", mse=mse, psnr=psnr, ssim=_mean([r[c["ssim"]] for r in rs]),
                 rot=[r[c["rot"]] for r in rs], trans=[r[c["trans"]] for r in rs],
                 angle_trans=_mean([r[c["angle_trans"]] for r in rs]),
                 **{name: _mean([r[c[name]] for r in rs]) for name in self.extra},
                 **{name: [r[c[name]] for r in rs] for name in self.columns[len(COLUMNS) + len(self.extra):]})
        out: Dict[str, Dict[str, float]] = {}
        for key in ("all",) + BUCKETS:
            g = groups.get(key)
            if not g:
                continue
            s: Dict[str, float] = {"n": len(g["mse"])}
            for name in ("psnr", "ssim", "mse"):
                s[name] = _mean(g[name])
            for name in ("rot", "trans", "angle_trans"):
                for stat, v in _stats(g[name]).items():
                    s[f"{name}_{stat}"] = v
            for name in self.extra:
                s[name] = _mean(g[name])
            for src in self.sources:
                for name in ("rot64", "angle64"):
                    for stat, v in _stats64(g[f"{name}_{src}"]).items():
                        s[f"{name}_{src}_{stat}"] = v
                worst = [math.degrees(max(a, b)) if a == a and b == b else float("nan")
                         for a, b in zip(g[f"rot64_{src}"], g[f"angle64_{src}"])]
                for t, v in zip(AUC_AT, pose_auc(worst, AUC_AT)):
                    s[f"auc{t}_{src}"] = v
            if self.geometry is not None:
                for name in QUALITY:
                    s[name] = _nanmean(g[name])
                if "select" in self.sources:
                    for label, name in enumerate(MODELS + ("none",)):
                        s[f"model_{name}"] = sum(1 for v in g["model"] if int(v) == (label if label < len(MODELS) else -1)) / len(g["model"])
            out[key] = s
        return out

    def format_summary(self, summary: Optional[Dict[str, Dict[str, float]]] = None) -> str:
        """The line test.py:300 prints after every pair, one per group; extras are printed by their upper-cased names."""
        summary = self.summary() if summary is None else summary
        lines = []
        for key, s in summary.items():
            parts = [f"PSNR: {s['psnr']:.4f}", f"SSIM: {s['ssim']:.4f}"]
            parts += [f"{name.upper()}: {s[name]:.4f}" for name in self.extra if name in s]
            parts.append(f"MSE: {s['mse']:.4f}")
            for label, name in (("Rot", "rot"), ("Trans", "trans")):
                parts += [f"{label}_avg: {s[name + '_mean']:.4f}", f"{label}_median: {s[name + '_median']:.4f}",
                          f"{label}_std: {s[name + '_std']:.4f}"]
            parts += [f"Avg_Trans_angle: {s['angle_trans_mean']:.4f}", f"Med_Trans_angle: {s['angle_trans_median']:.4f}",
                      f"std_Trans_angle: {s['angle_trans_std']:.4f}"]
            lines.append(f"{key}: " + ", ".join(parts))
            for src in self.sources:                        # one more line per group and scored pose, in degrees
                if f"rot64_{src}_mean" not in s:
                    continue
                lines.append(f"{key}/{src}: " + ", ".join(
                    [f"{label}_{stat}: {math.degrees(s[f'{name}_{src}_{stat}']):.6f}" for label, name in (("Rot64_deg", "rot64"), ("Angle64_deg", "angle64"))
                     for stat in ("mean", "median", "std")] + [f"AUC@{t}: {s[f'auc{t}_{src}']:.4f}" for t in AUC_AT]))
        return "\n".join(lines)
