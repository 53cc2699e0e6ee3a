"""Two photos in, their dense correspondences out, and the estimated pose polished against them - on the device until the
user asks for the matches.

`get_z` returns two flows beside the pose: flow[0] lives on view 0's grid and points into view 1, flow[1] the other way
round.  The reference uses them for the cycle loss and a warped panel only.  Here

  match_fields  per pixel of both directions: the match, the cycle error cycle_masks thresholds, the in-image test and the
                signed Sampson residual under rel_pose, in pixels: cpn_match_fields, one launch
  select        the keep mask with stock ops, cpn_compact_matches -> a Matches
  Matches       xy (x0, y0, x1, y1) / err (cycle, epi) / count on the device; numpy(b) is the one host read
  refine_pose   robust Gauss-Newton of the relative pose on the Sampson residuals of the matches: cpn_refine_pose, one launch
  ransac_pose   the relative pose from the matches ALONE: 8-point RANSAC, cpn_ransac_hypotheses / _score / _finish, three
                launches; with it the inlier count of rel_pose under the same rule and an inlier mask; solver="5pt" takes
                minimal samples instead (cpn_ransac_hypotheses5, up to 10 solutions each); score="msac" and lo=K (round 24,
                opt-in) grade the inliers and polish the K best hypotheses inside the loop (cpn_ransac_score_slots /
                _polish / _finish_lo)
  homography_pose  the same RANSAC with a homography as its model, for walls, floors and pure rotations, where the essential
                matrix is under-determined: cpn_ransac_homographies / _score_h / _finish_h, three launches; with it the twin
                pose, the singular values of H and the statistics that say which regime a pair is in
  refine_homography  refine_pose's Gauss-Newton on the homography's own Sampson residual, for the plane (nine entries) or for the
                rotation alone (three parameters): cpn_refine_homography, one launch
  model_gric    Torr's GRIC of E, the plane and the rotation alone on the same matches: cpn_model_gric, one launch
  select_pose   all of the above in a row and the picked model's pose: which estimator to believe, decided on the device
  pose_errors   up to 8 poses per pair against a ground truth in float64, both angles by atan2: cpn_pose_errors, one launch
  residual_stats  exact quantiles, inlier counts and a robust sigma of the matches' residuals under given poses - under the true
                pose the evidence the thresholds above should be set by: cpn_residual_stats, one launch
  from_pair     get_z once, then the above (ransac_pose with ransac={...}, homography_pose with homography={...}, select_pose
                with select={...}; triangulate={...} adds the matches' 3-D points, coponerf_amd.triangulate.points)
  photo_coords  host: matches of a prepare_pair dict in the coordinates of the original photos

The conventions and the arithmetic are in include/coponerf_hip.h (round 16).  The selection defaults (cycle error up to 10
pixels - the reference's own mask -, one match per native flow cell) and scale_px are this package's choices and have not been
tried on a trained checkpoint, because none is available offline; whether the refined pose is closer to the truth than the
network's on real data is unknown.  The epipolar residual cannot see the translation's length: the refined pose keeps the
network's (coponerf_amd.triangulate.depth_scale, round 26, measures it against the model's own rendered depth).

refine_pose is a local method: from a rel_pose 30 degrees off it does not move.  ransac_pose (round 20 of the header) does not
look at rel_pose to find its pose, so the pose head cannot spoil it; `ransac={..., "start": "ransac" | "best"}` lets from_flows
and from_pair refine from it.  Its sampler, solver, threshold and hypothesis count are this package's definitions as well and
are as untried on a trained checkpoint; the linear 8-point solver is degenerate for a planar scene and for a pure rotation.
solver="5pt" (round 21 of the header) is not degenerate on a plane - a wall, a floor -, where the 8-point solver returns a wrong
pose with as many inliers as the true one; a purely planar scene keeps a two-fold ambiguity that only the vote on the depths
breaks, and a pure rotation gives E = 0 for either solver.

homography_pose (round 22 of the header) is the model of exactly those cases: one plane, or no baseline.  It returns a pose where
the essential-matrix solvers cannot - on the wall with 64 samples, where the 5-point solver's winner is 10.3, 50.7 degrees off, its
pose is 1.0, 3.2 degrees off and the wrong one is returned beside it as `twin` -, few inliers where the scene is not planar (39
against the 8-point solver's 684 on the curved scene: the planarity verdict), and sigma_1 - sigma_3 of H, the baseline over the
plane's distance, which says "no baseline".  Its transfer-error inlier rule, its visibility vote, its pick order and min_baseline
with its default are this package's definitions and untried on a trained checkpoint; a fronto-parallel plane in a narrow field of
view can leave the vote tied, and stats[4..7] then says so.

select_pose (round 23 of the header) is the verdict between them.  GRIC on the RANSAC winners as they are misreads the pure rotation;
after refine_homography - ten robust Gauss-Newton passes on the homography's Sampson residual, from homography_pose's H and from the
rotation nearest to it - the wall picks the plane, the curved scene E and the pure rotation the rotation alone.  The rotation-only
model inside the criterion is what min_baseline was a stand-in for.  The residual, the weights, the gauge, sigma_px = 0.5 (half the
default inlier_px), the tie rule and the (d, k) table are this package's definitions and untried on a trained checkpoint.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._args import device_tensors, one_device
from .shards import crop_window


def _cameras(who: str, intrinsics: torch.Tensor, rel_pose: Optional[torch.Tensor], B: int) -> None:
    if tuple(intrinsics.shape) != (B, 2, 4, 4):
        raise ValueError(f"{who}: intrinsics must be (B, 2, 4, 4) with B = {B} (`context.intrinsics`), got {tuple(intrinsics.shape)}")
    if rel_pose is not None and tuple(rel_pose.shape) != (B, 4, 4):
        raise ValueError(f"{who}: rel_pose must be (B, 4, 4) with B = {B}, got {tuple(rel_pose.shape)}")


@torch.no_grad()
def match_fields(flow: Sequence[torch.Tensor], intrinsics: torch.Tensor, rel_pose: torch.Tensor, S: int = 256) -> Dict[str, torch.Tensor]:
    """cpn_match_fields: flow = (flow[0], flow[1]), each (B, 2, h, h) fp32 as get_z returns them, intrinsics (B, 2, 4, 4) fp32
    (`context.intrinsics`), rel_pose (B, 4, 4) fp32, S a multiple of h -> a dict, index 0 of every tensor the direction:
    `q` (2, B, S, S, 2) fp32 the match of every pixel, `cycle` (2, B, S, S) fp32 the forward-backward error in pixels, `epi`
    (2, B, S, S) fp32 the signed Sampson residual in pixels (NaN where it is not defined), `inside` (2, B, S, S) uint8."""
    if len(flow) < 2:
        raise ValueError("match_fields: flow must hold the two directions")
    f0, f1 = flow[0], flow[1]
    device_tensors("match_fields", (("flow[0]", f0, torch.float32, None), ("flow[1]", f1, torch.float32, None),
                                    ("intrinsics", intrinsics, torch.float32, None), ("rel_pose", rel_pose, torch.float32, None)))
    if f0.dim() != 4 or f0.shape[1] != 2 or f0.shape[2] != f0.shape[3] or f1.shape != f0.shape:
        raise ValueError(f"match_fields: flows must both be (B, 2, h, h), got {tuple(f0.shape)} and {tuple(f1.shape)}")
    B, h, S = int(f0.shape[0]), int(f0.shape[2]), int(S)
    _cameras("match_fields", intrinsics, rel_pose, B)
    if h < 1 or S < h or S % h or not 1 <= B <= 32767 or S > 16384 or 2 * B * S * S >= 2 ** 31:
        raise ValueError(f"match_fields: need S a multiple of h, 1 <= B <= 32767, S <= 16384 and 2 B S S < 2^31, got B = {B}, S = {S}, "
                         f"h = {h}")
    dev = f0.device
    q = torch.empty(2, B, S, S, 2, dtype=torch.float32, device=dev)
    cycle = torch.empty(2, B, S, S, dtype=torch.float32, device=dev)
    epi = torch.empty(2, B, S, S, dtype=torch.float32, device=dev)
    inside = torch.empty(2, B, S, S, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_match_fields", f0.data_ptr(), f1.data_ptr(), intrinsics.data_ptr(), rel_pose.data_ptr(), B, S, h, q.data_ptr(),
                  cycle.data_ptr(), epi.data_ptr(), inside.data_ptr(), _hip.stream_handle())
    return {"q": q, "cycle": cycle, "epi": epi, "inside": inside}


def pack_matches(count: torch.Tensor, xy: torch.Tensor, err: torch.Tensor) -> torch.Tensor:
    """One pair's count (1) int32, xy (cap, 4) fp32 and err (cap, 2) fp32 as one uint8 buffer: what Matches.numpy reads."""
    return torch.cat((count.view(torch.uint8), xy.view(torch.uint8).reshape(-1), err.view(torch.uint8).reshape(-1)))


def unpack_matches(packed: np.ndarray, cap: int) -> Tuple[np.ndarray, np.ndarray]:
    """pack_matches' buffer on the host -> ((n, 4) float32, (n, 2) float32): the rows beyond the count are dropped here."""
    n = int(packed[:4].view(np.int32)[0])
    xy = packed[4:4 + 16 * cap].view(np.float32).reshape(cap, 4)[:n].copy()
    err = packed[4 + 16 * cap:4 + 24 * cap].view(np.float32).reshape(cap, 2)[:n].copy()
    return xy, err


class Matches:
    """The kept matches of B pairs on the device: xy (B, cap, 4) fp32 = (x0, y0, x1, y1) in the pixels of the S x S grid, view
    0's point first whatever the direction it was found in; err (B, cap, 2) fp32 = (cycle error, epipolar residual) in pixels;
    count (B) int32.  Pair b's matches are the rows [0, count[b]) in (direction, row, column) order; the rows beyond are not
    written."""

    def __init__(self, xy: torch.Tensor, err: torch.Tensor, count: torch.Tensor):
        self.xy, self.err, self.count = xy, err, count

    @torch.no_grad()
    def numpy(self, b: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Pair b's matches on the host: ((n, 4) float32, (n, 2) float32).  ONE read: the count, xy and err of the pair travel in
        one buffer."""
        return unpack_matches(pack_matches(self.count[b:b + 1], self.xy[b], self.err[b]).cpu().numpy(), int(self.xy.shape[1]))


_STRIDE_MASKS: Dict = {}


def _stride_mask(S: int, stride: int, dev) -> torch.Tensor:
    """(S, S) bool: the pixels with x % stride == stride // 2 and y % stride == stride // 2; a constant, built once."""
    key = (S, stride, str(dev))
    m = _STRIDE_MASKS.get(key)
    if m is None:
        on = torch.arange(S, device=dev) % stride == stride // 2
        m = _STRIDE_MASKS[key] = on[:, None] & on[None, :]
    return m


@torch.no_grad()
def compact(keep: torch.Tensor, q: torch.Tensor, cycle: torch.Tensor, epi: torch.Tensor) -> Matches:
    """cpn_compact_matches: keep (2, B, S, S) uint8 (non-zero = kept) and match_fields' q, cycle and epi -> the Matches of every
    pair in (direction, row, column) order, cap = 2 S S rows per pair."""
    one_device("compact", keep, q, cycle, epi)
    if keep.dtype != torch.uint8 or keep.dim() != 4 or keep.shape[0] != 2 or keep.shape[2] != keep.shape[3]:
        raise ValueError(f"compact: keep must be (2, B, S, S) uint8, got {tuple(keep.shape)} {keep.dtype}")
    B, S = int(keep.shape[1]), int(keep.shape[2])
    for what, x, shape in (("q", q, (2, B, S, S, 2)), ("cycle", cycle, (2, B, S, S)), ("epi", epi, (2, B, S, S))):
        if x.dtype != torch.float32 or tuple(x.shape) != shape:
            raise ValueError(f"compact: {what} must be {shape} fp32, got {tuple(x.shape)} {x.dtype}")
    n_scratch = _hip.lib().cpn_compact_matches_scratch(B, S)
    if n_scratch <= 0:
        raise ValueError(f"compact: need 1 <= B <= 32767, S <= 16384 and 2 B S S < 2^31, got B = {B}, S = {S}")
    dev, cap = keep.device, 2 * S * S
    xy = torch.empty(B, cap, 4, dtype=torch.float32, device=dev)
    err = torch.empty(B, cap, 2, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(n_scratch, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_compact_matches", keep.data_ptr(), q.data_ptr(), cycle.data_ptr(), epi.data_ptr(), B, S, scratch.data_ptr(),
                  xy.data_ptr(), err.data_ptr(), count.data_ptr(), _hip.stream_handle())
    return Matches(xy, err, count)


@torch.no_grad()
def select(fields: Dict[str, torch.Tensor], max_cycle_px: float = 10.0, max_epi_px: Optional[float] = None, stride: int = 4) -> Matches:
    """The Matches of match_fields' dict: a pixel is kept iff its match lies inside the image, its cycle error is at most
    max_cycle_px (10: the reference's own mask), with max_epi_px its |epi| is at most that (a NaN epi is dropped), and
    x % stride == y % stride == stride // 2.  stride=4 keeps one match per native flow cell of a 64 x 64 flow at 256 x 256,
    where neighbouring pixels are 16-fold redundant; stride=1 keeps every pixel.  Stock ops form the mask, the kernel
    compacts it; nothing is read on the host."""
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"select: stride must be >= 1, got {stride}")
    cycle, epi, inside = fields["cycle"], fields["epi"], fields["inside"]
    keep = (inside != 0) & (cycle <= float(max_cycle_px))
    if max_epi_px is not None:
        keep &= epi.abs() <= float(max_epi_px)
    if stride > 1:
        keep &= _stride_mask(int(cycle.shape[-1]), stride, cycle.device)
    return compact(keep.to(torch.uint8), fields["q"], cycle, epi)


_select_matches = select                  # from_flows has a keyword of this name


def _matches_args(who: str, matches: Matches) -> Tuple[int, int]:
    xy, count = matches.xy, matches.count
    if xy.dim() != 3 or xy.shape[2] != 4 or xy.shape[1] < 1:
        raise ValueError(f"{who}: matches.xy must be (B, N, 4) with N >= 1, got {tuple(xy.shape)}")
    B, N = int(xy.shape[0]), int(xy.shape[1])
    if not torch.is_tensor(count) or count.device != xy.device or count.dtype != torch.int32 or tuple(count.shape) != (B,) or \
            not count.is_contiguous():
        raise ValueError(f"{who}: matches.count must be a contiguous ({B},) int32 tensor on xy's device")
    return B, N


@torch.no_grad()
def refine_pose(matches: Matches, intrinsics: torch.Tensor, rel_pose: torch.Tensor, iters: int = 10,
                scale_px: float = 2.0) -> Dict[str, torch.Tensor]:
    """cpn_refine_pose: `iters` damped Gauss-Newton steps of the relative pose on the Sampson residuals of the matches, each
    weighted 1 / (1 + (r / scale_px)^2)^2, float64 inside, one launch for all pairs -> `pose` (B, 4, 4) fp32 = [R | |t0| t]
    (the translation keeps rel_pose's length, which the residual cannot see) and `stats` (B, 8) float64: the cost at the
    start, the cost / sum of weights / number of usable matches at the end, the angles in degrees the rotation and the
    translation direction moved by, the updates made, and the status (0 ok, 1 a failed solve: the state before it is
    returned, 2 nothing to do: no matches, a zero or non-finite pose, or iters == 0 - pose is rel_pose, the rest 0)."""
    xy, count = matches.xy, matches.count
    device_tensors("refine_pose", (("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None),
                                   ("rel_pose", rel_pose, torch.float32, None)))
    B, N = _matches_args("refine_pose", matches)
    _cameras("refine_pose", intrinsics, rel_pose, B)
    if int(iters) < 0 or not 0.0 < float(scale_px) < float("inf"):
        raise ValueError(f"refine_pose: need iters >= 0 and a finite scale_px > 0, got {iters} and {scale_px}")
    pose = torch.empty(B, 4, 4, dtype=torch.float32, device=xy.device)
    stats = torch.empty(B, 8, dtype=torch.float64, device=xy.device)
    with torch.cuda.device(xy.device):
        _hip.call("cpn_refine_pose", xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), rel_pose.data_ptr(), B, N, int(iters),
                  float(scale_px), pose.data_ptr(), stats.data_ptr(), _hip.stream_handle())
    return {"pose": pose, "stats": stats}


@torch.no_grad()
def ransac_pose(matches: Matches, intrinsics: torch.Tensor, rel_pose: Optional[torch.Tensor] = None, hypotheses: int = 1024,
                inlier_px: float = 1.0, seed: int = 0, solver: str = "8pt", score: str = "inliers", lo: int = 0, lo_iters: int = 4,
                lo_scale_px: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """cpn_ransac_hypotheses, cpn_ransac_score, cpn_ransac_finish: `hypotheses` linear 8-point solutions from samples drawn by
    a counter hash of (seed, hypothesis, draw) - the same for every pair -, each scored by its matches within inlier_px of
    Sampson residual, the best split into the pose that puts its inliers in front of both cameras.  float64 inside, three
    launches for all pairs, nothing read on the host -> `pose` (B, 4, 4) fp32 = [R | s t] with |t| = 1 and s the length of
    rel_pose's translation (1 without a usable one: the residual cannot see it), `inlier` (B, N) uint8 and `stats` (B, 8)
    float64: the winner's inliers, the usable matches, the winner's index, the valid hypotheses, the inliers of rel_pose under
    the same rule (-1 without one), the angles in degrees between the pose and rel_pose (rotation, translation direction), the
    status (0 ok, 1 no valid hypothesis, 2 nothing to do: fewer than 8 usable matches or hypotheses == 0 - pose is rel_pose,
    or the identity without one).  rel_pose is only measured against, never searched from.
    solver="5pt" (cpn_ransac_hypotheses5, round 21 of the header) draws `hypotheses` samples of 5 matches - the first 5 of the
    8-point sample of the same index - and solves each for up to 10 essential matrices, the real roots of a degree-10
    polynomial: the hypothesis buffers hold 10 slots per sample, slot 10 h + r is root r of sample h, stats[2] is the winning
    SLOT (its sample is stats[2] // 10) and stats[3] the number of valid slots.  Unlike the 8-point solver it is not degenerate
    where the matches lie on one plane (a wall, a floor); a purely planar scene keeps a two-fold ambiguity that only the vote
    on the depths breaks, and a pure rotation gives E = 0 for either solver.  Status 2 stays "fewer than 8 usable matches".
    Three launches as well, with 10 times the slots to score.
    LO-MSAC (round 24 of the header), opt-in: score="msac" grades an inlier by floor(2^20 (1 - r^2 / inlier_px^2)) instead of
    counting it, an integer still; lo=K (0 .. 16) polishes the K best-scoring slots by lo_iters passes of refine_pose's
    Gauss-Newton on all matches (weights of scale lo_scale_px, None: inlier_px) inside the loop, scores them as slots
    `slots` .. `slots` + K - 1 and lets the finish choose among all: a polished slot wins only where it scores strictly higher.
    With score="inliers" and lo=0 the call is the three launches above; otherwise hypotheses, cpn_ransac_score_slots,
    cpn_ransac_finish_lo are three launches too, and lo > 0 adds cpn_ransac_polish and a second cpn_ransac_score_slots on the K
    new slots alone: five.  Nothing is read on the host.  stats keep their meaning: [0] is the winner's inlier COUNT under either
    score, [2] the winning slot - at or beyond `slots` a polished one - and [3] counts the valid slots among all slots + K.  With
    either keyword off its default the result gains `score` (B,) int64, the winner's score (in units of 2^-20 inlier for "msac", the count otherwise), and `lo`
    (B, 4) float64: whether a polished slot won, the slot it was polished from and that slot's rank (-1 where none won), and the
    passes made."""
    if solver not in _SOLVERS:
        raise ValueError(f"ransac_pose: solver must be one of {_SOLVERS}, got {solver!r}")
    if score not in _SCORES:
        raise ValueError(f"ransac_pose: score must be one of {_SCORES}, got {score!r}")
    if isinstance(lo, bool) or not isinstance(lo, int) or not 0 <= lo <= _hip.CONSTANTS["RANSAC_LO_MAX"]:
        raise ValueError(f"ransac_pose: lo must be an integer in 0 .. {_hip.CONSTANTS['RANSAC_LO_MAX']}, got {lo!r}")
    if isinstance(lo_iters, bool) or not isinstance(lo_iters, int) or lo_iters < 0:
        raise ValueError(f"ransac_pose: lo_iters must be an integer >= 0, got {lo_iters!r}")
    if lo_scale_px is not None and not 0.0 < float(lo_scale_px) < float("inf"):
        raise ValueError(f"ransac_pose: lo_scale_px must be None or finite and > 0, got {lo_scale_px!r}")
    if lo and lo_scale_px is None and not float(inlier_px) > 0.0:
        raise ValueError(f"ransac_pose: lo > 0 with lo_scale_px None takes inlier_px as the scale, which must be > 0; got lo = {lo}, "
                         f"inlier_px = {inlier_px}")
    per = 10 if solver == "5pt" else 1                              # hypothesis slots per sample
    xy, count = matches.xy, matches.count
    named = [("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None)]
    if rel_pose is not None:
        named.append(("rel_pose", rel_pose, torch.float32, None))
    device_tensors("ransac_pose", tuple(named))
    B, N = _matches_args("ransac_pose", matches)
    _cameras("ransac_pose", intrinsics, rel_pose, B)
    Hn, px, seed = int(hypotheses), float(inlier_px), int(seed)
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    slots = per * Hn
    if not 0 <= slots <= 2 ** 20 - lo or not 1 <= B <= 32767 or N > 2 ** 24 or B * chunks * (slots + lo + 1) >= 2 ** 31:
        what = "hypotheses" if per == 1 else f"{per} hypotheses"
        what = what if lo == 0 else f"{what} + lo"
        raise ValueError(f"ransac_pose: need 0 <= {what} <= 2^20, 1 <= B <= 32767, N <= 2^24 and B ceil(N / "
                         f"{_hip.CONSTANTS['RANSAC_CHUNK']}) ({what} + 1) < 2^31, got hypotheses = {hypotheses}, lo = {lo}, B = {B}, "
                         f"N = {N}")
    if not 0.0 <= px < float("inf"):
        raise ValueError(f"ransac_pose: need a finite inlier_px >= 0, got {inlier_px}")
    if not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError(f"ransac_pose: seed must fit 64 bits, got {seed}")
    dev = xy.device
    E = torch.empty(B, max(slots, 1), 9, dtype=torch.float64, device=dev)
    sample = torch.empty(B, max(Hn, 1), 5 if per == 10 else 8, dtype=torch.int32, device=dev)
    valid = torch.empty(B, max(slots, 1), dtype=torch.uint8, device=dev)
    partial = torch.empty(B, chunks, slots + lo + 1, dtype=torch.int32, device=dev)
    pose = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    inlier = torch.empty(B, N, dtype=torch.uint8, device=dev)
    stats = torch.empty(B, 8, dtype=torch.float64, device=dev)
    rel = 0 if rel_pose is None else rel_pose.data_ptr()
    graded = 1 if score == "msac" else 0
    with torch.cuda.device(dev):
        s = _hip.stream_handle()
        if Hn:
            _hip.call("cpn_ransac_hypotheses5" if per == 10 else "cpn_ransac_hypotheses", xy.data_ptr(), count.data_ptr(),
                      intrinsics.data_ptr(), B, N, Hn, seed, E.data_ptr(), sample.data_ptr(), valid.data_ptr(), s)
        if not graded and lo == 0:                                  # round 20's path, as it was
            _hip.call("cpn_ransac_score", E.data_ptr(), valid.data_ptr(), xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), rel, B,
                      N, slots, px, partial.data_ptr(), s)
            _hip.call("cpn_ransac_finish", E.data_ptr(), valid.data_ptr(), partial.data_ptr(), xy.data_ptr(), count.data_ptr(),
                      intrinsics.data_ptr(), rel, B, N, slots, px, pose.data_ptr(), inlier.data_ptr(), stats.data_ptr(), s)
            return {"pose": pose, "inlier": inlier, "stats": stats}
        E_lo = torch.empty(B, max(lo, 1), 9, dtype=torch.float64, device=dev)
        valid_lo = torch.empty(B, max(lo, 1), dtype=torch.uint8, device=dev)
        info = torch.empty(B, max(lo, 1), 8, dtype=torch.float64, device=dev)
        won = torch.empty(B, dtype=torch.int64, device=dev)
        lo_out = torch.empty(B, 4, dtype=torch.float64, device=dev)
        _hip.call("cpn_ransac_score_slots", E.data_ptr(), valid.data_ptr(), xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), rel, B,
                  N, slots, 0, slots + lo, graded, px, partial.data_ptr(), s)
        if lo:
            _hip.call("cpn_ransac_polish", E.data_ptr(), valid.data_ptr(), partial.data_ptr(), xy.data_ptr(), count.data_ptr(),
                      intrinsics.data_ptr(), B, N, slots, lo, lo_iters, px, float(px if lo_scale_px is None else lo_scale_px),
                      E_lo.data_ptr(), valid_lo.data_ptr(), info.data_ptr(), s)
            _hip.call("cpn_ransac_score_slots", E_lo.data_ptr(), valid_lo.data_ptr(), xy.data_ptr(), count.data_ptr(),
                      intrinsics.data_ptr(), rel, B, N, lo, slots, slots + lo, graded, px, partial.data_ptr(), s)
        _hip.call("cpn_ransac_finish_lo", E.data_ptr(), valid.data_ptr(), E_lo.data_ptr(), valid_lo.data_ptr(), info.data_ptr(),
                  partial.data_ptr(), xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), rel, B, N, slots, lo, graded, px,
                  pose.data_ptr(), inlier.data_ptr(), stats.data_ptr(), won.data_ptr(), lo_out.data_ptr(), s)
    return {"pose": pose, "inlier": inlier, "stats": stats, "score": won, "lo": lo_out}


@torch.no_grad()
def homography_pose(matches: Matches, intrinsics: torch.Tensor, rel_pose: Optional[torch.Tensor] = None, hypotheses: int = 1024,
                    inlier_px: float = 1.0, seed: int = 0, min_baseline: float = 0.0) -> Dict[str, torch.Tensor]:
    """cpn_ransac_homographies, cpn_ransac_score_h, cpn_ransac_finish_h (round 22 of the header): the RANSAC of ransac_pose with
    a homography a ~ H b as its model, for the pairs that one plane (a wall, a floor) or a pure rotation explains, where the
    essential matrix is under-determined.  `hypotheses` samples of 4 matches - the first 4 of ransac_pose's sample of the same
    index -, each H scored by the matches whose transfer error is within inlier_px in BOTH views, the best decomposed into its
    four (R, T, N); the winner's inliers vote on the side of the plane (it must lie in front of the camera), and the Sampson
    inliers of E = [T]x R under ransac_pose's own rule break a tie.  float64 inside, three launches for all pairs, nothing read on
    the host -> `pose` (B, 4, 4) fp32 = [R | s T / |T|] with s as in ransac_pose; `twin` (B, 4, 4) fp32, the better-voted pose of
    the other solution family - on a wall the pose the 8-point and the few-sample 5-point solver fall into -; `H` (B, 9)
    float64, the winner with sigma_2 = 1 and det > 0; `inlier` (B, N) uint8; `stats` (B, 12) float64: [0] the winner's inliers,
    [1] usable matches, [2] the winner's index, [3] valid hypotheses, [4], [5] the votes of the pose and of the twin, [6], [7]
    the Sampson inliers of their essential matrices, [8] sigma_1 / sigma_2, [9] sigma_3 / sigma_2, [10] sigma_1 - sigma_3 = the
    baseline over the plane's distance, [11] the status: 0 ok, 1 no valid hypothesis, 2 nothing to do (fewer than 4 usable matches
    or hypotheses == 0; pose is rel_pose, or the identity without one), 3 rotation only ([10] <= min_baseline: pose = twin =
    [R | 0] with R the rotation nearest to H).  [4] = [5] and [6] = [7] say that the ambiguity was not resolved - a fronto-parallel
    plane in a narrow field of view can do that -; [0] against ransac_pose's stats[0] is the planarity verdict.
    rel_pose is only measured against, never searched from.  The transfer-error rule, the vote, the pick order and min_baseline
    are this package's definitions and untried on a trained checkpoint; min_baseline = 0.0 means "only an exactly rotation-only H
    gets status 3", and where to set it for real data is unknown."""
    xy, count = matches.xy, matches.count
    named = [("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None)]
    if rel_pose is not None:
        named.append(("rel_pose", rel_pose, torch.float32, None))
    device_tensors("homography_pose", tuple(named))
    B, N = _matches_args("homography_pose", matches)
    _cameras("homography_pose", intrinsics, rel_pose, B)
    Hn, px, seed, base = int(hypotheses), float(inlier_px), int(seed), float(min_baseline)
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    if not 0 <= Hn <= 2 ** 20 or not 1 <= B <= 32767 or N > 2 ** 24 or B * chunks * (Hn + 1) >= 2 ** 31:
        raise ValueError(f"homography_pose: need 0 <= hypotheses <= 2^20, 1 <= B <= 32767, N <= 2^24 and B ceil(N / "
                         f"{_hip.CONSTANTS['RANSAC_CHUNK']}) (hypotheses + 1) < 2^31, got hypotheses = {hypotheses}, B = {B}, N = {N}")
    if not 0.0 <= px < float("inf"):
        raise ValueError(f"homography_pose: need a finite inlier_px >= 0, got {inlier_px}")
    if not 0.0 <= base < float("inf"):
        raise ValueError(f"homography_pose: need a finite min_baseline >= 0, got {min_baseline}")
    if not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError(f"homography_pose: seed must fit 64 bits, got {seed}")
    dev = xy.device
    Hm = torch.empty(B, max(Hn, 1), 9, dtype=torch.float64, device=dev)
    sample = torch.empty(B, max(Hn, 1), 4, dtype=torch.int32, device=dev)
    valid = torch.empty(B, max(Hn, 1), dtype=torch.uint8, device=dev)
    partial = torch.empty(B, chunks, max(Hn, 1), dtype=torch.int32, device=dev)
    pose = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    twin = torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
    Hout = torch.empty(B, 9, dtype=torch.float64, device=dev)
    inlier = torch.empty(B, N, dtype=torch.uint8, device=dev)
    stats = torch.empty(B, 12, dtype=torch.float64, device=dev)
    rel = 0 if rel_pose is None else rel_pose.data_ptr()
    with torch.cuda.device(dev):
        s = _hip.stream_handle()
        if Hn:
            _hip.call("cpn_ransac_homographies", xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), B, N, Hn, seed, Hm.data_ptr(),
                      sample.data_ptr(), valid.data_ptr(), s)
            _hip.call("cpn_ransac_score_h", Hm.data_ptr(), valid.data_ptr(), xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), B, N,
                      Hn, px, partial.data_ptr(), s)
        _hip.call("cpn_ransac_finish_h", Hm.data_ptr(), valid.data_ptr(), partial.data_ptr(), xy.data_ptr(), count.data_ptr(),
                  intrinsics.data_ptr(), rel, B, N, Hn, px, base, pose.data_ptr(), twin.data_ptr(), Hout.data_ptr(), inlier.data_ptr(),
                  stats.data_ptr(), s)
    return {"pose": pose, "twin": twin, "H": Hout, "inlier": inlier, "stats": stats}


_H_MODELS = ("plane", "rotation")


@torch.no_grad()
def refine_homography(matches: Matches, intrinsics: torch.Tensor, H: torch.Tensor, model: str = "plane", iters: int = 10,
                      scale_px: float = 2.0) -> Dict[str, torch.Tensor]:
    """cpn_refine_homography (round 23 of the header): refine_pose's robust Gauss-Newton on the homography's Sampson residual
    e^2 - to first order the squared distance in pixels from a match to the matches that satisfy H, weighted
    1 / (1 + e^2 / scale_px^2)^2 -, float64 inside, one launch for all pairs.  H (B, 9) float64 is the start (homography_pose's
    `H`).  model="plane" refines the nine entries with |h| = 1 (the gauge pins the length); model="rotation" refines the rotation
    nearest to H, three parameters -> `H` (B, 9) float64 (the unit h with det > 0, or the rotation), `pose` (B, 4, 4) fp32
    ([R | 0] for "rotation", the identity for "plane": a plane's pose takes the decomposition of cpn_ransac_finish_h) and
    `stats` (B, 8) float64: the cost at the start, the cost / sum of weights / rows that count at the end, how far the state
    moved (Frobenius distance of the unit h, or degrees), sigma_1 - sigma_3 of the refined plane (0 for "rotation"), the updates
    made, the status (0 ok, 1 a failed solve: the state before it is returned, 2 nothing to do: no matches, iters == 0, a zero
    or non-finite H - H as it came, the identity, the rest 0)."""
    if model not in _H_MODELS:
        raise ValueError(f"refine_homography: model must be one of {_H_MODELS}, got {model!r}")
    xy, count = matches.xy, matches.count
    device_tensors("refine_homography", (("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None),
                                         ("H", H, torch.float64, None)))
    B, N = _matches_args("refine_homography", matches)
    _cameras("refine_homography", intrinsics, None, B)
    if tuple(H.shape) != (B, 9):
        raise ValueError(f"refine_homography: H must be (B, 9) with B = {B}, got {tuple(H.shape)}")
    if not 1 <= B <= 32767 or N > 2 ** 24:
        raise ValueError(f"refine_homography: need 1 <= B <= 32767 and N <= 2^24, got B = {B}, N = {N}")
    if int(iters) < 0 or not 0.0 < float(scale_px) < float("inf"):
        raise ValueError(f"refine_homography: need iters >= 0 and a finite scale_px > 0, got {iters} and {scale_px}")
    Hout = torch.empty(B, 9, dtype=torch.float64, device=xy.device)
    pose = torch.empty(B, 4, 4, dtype=torch.float32, device=xy.device)
    stats = torch.empty(B, 8, dtype=torch.float64, device=xy.device)
    with torch.cuda.device(xy.device):
        _hip.call("cpn_refine_homography", xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), H.data_ptr(), B, N,
                  _H_MODELS.index(model), int(iters), float(scale_px), Hout.data_ptr(), pose.data_ptr(), stats.data_ptr(),
                  _hip.stream_handle())
    return {"H": Hout, "pose": pose, "stats": stats}


_LN4N: Dict = {}


def ln4n_table(N: int) -> np.ndarray:
    """(N + 1) float64: entry u is ln(4 u) as numpy computes it on the host, entry 0 is 0 - cpn_model_gric's table."""
    t = np.zeros(N + 1)
    t[1:] = np.log(4.0 * np.arange(1, N + 1, dtype=np.float64))
    return t


def _ln4n(N: int, dev) -> torch.Tensor:
    """ln4n_table on the device; a constant, built and copied once per (N, device)."""
    key = (N, str(dev))
    t = _LN4N.get(key)
    if t is None:
        t = _LN4N[key] = torch.from_numpy(ln4n_table(N)).to(dev)
    return t


@torch.no_grad()
def model_gric(matches: Matches, intrinsics: torch.Tensor, pose_e: torch.Tensor, H_plane: torch.Tensor, H_rot: torch.Tensor,
               avail: torch.Tensor, sigma_px: float = 0.5) -> Dict[str, torch.Tensor]:
    """cpn_model_gric (round 23 of the header): Torr's GRIC of three models of the same matches - E = [t]x R of pose_e (B, 4, 4)
    fp32, the plane H_plane and the rotation H_rot (B, 9) float64 -, one launch, nothing read on the host.  Every usable match
    pays min(e^2 / sigma_px^2, 2 (4 - d)) with e^2 the squared Sampson residual in pixels under the model; the model pays
    ln 4 . d per match for its dimension d (3 for E, 2 for the other two) and ln(4 n) per parameter (5, 8, 3).  avail (B, 3) uint8
    says which models take part; a model with a non-finite value is out as well -> `gric` (B, 3) float64 (+inf where out),
    `label` (B, N) uint8 (bit m: the match lies below model m's cap) and `stats` (B, 7) float64: the pick (0 E, 1 plane, 2 rotation;
    the smallest gric, a tie to the model with fewer parameters; -1 where none is in), the usable matches, the matches below the cap
    per model, the runner-up's gric minus the winner's, the status (0 ok, 1 no model in, 2 no usable match).  sigma_px = 0.5 is
    half the default inlier_px, this package's choice and untried on a trained checkpoint."""
    xy, count = matches.xy, matches.count
    device_tensors("model_gric", (("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None),
                                  ("pose_e", pose_e, torch.float32, None), ("H_plane", H_plane, torch.float64, None),
                                  ("H_rot", H_rot, torch.float64, None), ("avail", avail, torch.uint8, None)))
    B, N = _matches_args("model_gric", matches)
    _cameras("model_gric", intrinsics, pose_e, B)
    for what, x, shape in (("H_plane", H_plane, (B, 9)), ("H_rot", H_rot, (B, 9)), ("avail", avail, (B, 3))):
        if tuple(x.shape) != shape:
            raise ValueError(f"model_gric: {what} must be {shape}, got {tuple(x.shape)}")
    if not 1 <= B <= 32767 or N > 2 ** 24:
        raise ValueError(f"model_gric: need 1 <= B <= 32767 and N <= 2^24, got B = {B}, N = {N}")
    if not 0.0 < float(sigma_px) < float("inf"):
        raise ValueError(f"model_gric: need a finite sigma_px > 0, got {sigma_px}")
    dev = xy.device
    table = _ln4n(N, dev)
    gric = torch.empty(B, 3, dtype=torch.float64, device=dev)
    label = torch.empty(B, N, dtype=torch.uint8, device=dev)
    stats = torch.empty(B, 7, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_model_gric", xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), pose_e.data_ptr(), H_plane.data_ptr(),
                  H_rot.data_ptr(), avail.data_ptr(), table.data_ptr(), B, N, float(sigma_px), gric.data_ptr(), label.data_ptr(),
                  stats.data_ptr(), _hip.stream_handle())
    return {"gric": gric, "label": label, "stats": stats}


def _pose_stack(who: str, poses: torch.Tensor, B: Optional[int] = None) -> Tuple[torch.Tensor, bool]:
    """poses (B, P, 4, 4), or (B, 4, 4) for P = 1 -> ((B, P, 4, 4), whether the outputs drop the pose axis)."""
    if not torch.is_tensor(poses) or poses.dim() not in (3, 4) or tuple(poses.shape[-2:]) != (4, 4) or \
            (B is not None and int(poses.shape[0]) != B):
        raise ValueError(f"{who}: poses must be (B, P, 4, 4) or (B, 4, 4){'' if B is None else f' with B = {B}'}, got "
                         f"{tuple(poses.shape) if torch.is_tensor(poses) else type(poses).__name__}")
    single = poses.dim() == 3
    poses = poses[:, None] if single else poses
    top = _hip.CONSTANTS["POSE_EVAL_MAX"]
    if not 1 <= int(poses.shape[0]) <= 32767 or not 1 <= int(poses.shape[1]) <= top:
        raise ValueError(f"{who}: need 1 <= B <= 32767 pairs of 1 <= P <= {top} poses, got {tuple(poses.shape)}")
    return poses, single


@torch.no_grad()
def pose_errors(poses: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """cpn_pose_errors (round 25 of the header): poses (B, P, 4, 4) fp32 - or (B, 4, 4): P is 1 and the output drops that axis -
    against gt (B, 4, 4) fp32 -> (B, P, 3) float64: the rotation angle in radians, atan2 of the sine from the antisymmetric part of
    R R_gt^T and the cosine from its trace; the translation distance in scene units; the angle between the two translation
    directions in radians, atan2(|t x t_gt|, t . t_gt), NaN for a zero translation.  A pose with a value that is not finite has
    three NaNs.  One launch, one thread per (pair, pose), float64 inside.  evaluate.pose_metrics is the reference's fp32 acos, whose
    angle comes in steps of 0.02 degrees near 0; this one resolves 1e-6 degrees and 179.9999."""
    poses, single = _pose_stack("pose_errors", poses)
    B, P = int(poses.shape[0]), int(poses.shape[1])
    device_tensors("pose_errors", (("poses", poses, torch.float32, None), ("gt", gt, torch.float32, (B, 4, 4))))
    out = torch.empty(B, P, 3, dtype=torch.float64, device=poses.device)
    with torch.cuda.device(poses.device):
        _hip.call("cpn_pose_errors", poses.data_ptr(), gt.data_ptr(), B, P, out.data_ptr(), _hip.stream_handle())
    return out[:, 0] if single else out


_LEVELS: Dict = {}


def _levels(who: str, what: str, values: Sequence[float], top: float):
    """The quantiles or thresholds of residual_stats as the C array cpn_residual_stats takes; checked and built once per values."""
    key = (what, tuple(float(v) for v in values))
    arr = _LEVELS.get(key)
    if arr is None:
        n = _hip.CONSTANTS["POSE_EVAL_MAX"]
        if not 1 <= len(key[1]) <= n or not all(0.0 <= v <= top for v in key[1]):
            raise ValueError(f"{who}: {what} must hold 1 .. {n} values in [0, {top}], got {tuple(values)}")
        arr = _LEVELS[key] = (ctypes.c_double * len(key[1]))(*key[1])
    return arr


@torch.no_grad()
def residual_stats(matches: Matches, intrinsics: torch.Tensor, poses: torch.Tensor, q: Sequence[float] = (0.5,),
                   thresholds: Sequence[float] = (1.0,)) -> Dict[str, torch.Tensor]:
    """cpn_residual_stats (round 25 of the header): the distribution of the matches' Sampson residuals |r| in pixels under each of
    `poses` (B, P, 4, 4) fp32 - or (B, 4, 4): P is 1 and the outputs drop that axis -, E = [t]x R of the pose; with the ground-truth
    pose it is the evidence inlier_px, sigma_px and scale_px should be set by.  One launch, one workgroup per (pose, pair), float64
    inside, nothing read on the host -> `usable` (B, P) int32, the matches whose residual counts; `quant` (B, P, Q) float64, for
    each of `q` (1 .. 8 values in [0, 1]) the usable |r| of rank floor(q (usable - 1)) in ascending order - one of the residuals in
    its bits, never an interpolation; 0.5 is torch.median's lower middle -, NaN without a usable match; `within` (B, P, T) int32,
    the usable matches with |r| <= each of `thresholds` (1 .. 8 finite values >= 0); `sigma` (B, P, 2) float64: [0] Rousseeuw's
    LMedS scale 1.4826 (1 + 5 / (usable - 5)) median (NaN up to 5 usable matches), [1] sqrt(sum r^2 / (n_in - 5)) over the n_in
    usable matches within 2.5 [0] (NaN up to 5 of them); `status` (B, P) int32: 0 ok, 1 no usable match, 2 a pose that is not
    finite or has no translation.  The order statistics are exact: a radix descent on the bit pattern of |r| with the residual
    recomputed in every pass, no sort, no boolean indexing.  sigma is reported, not fed back: ransac_pose and model_gric take one
    threshold by value for all pairs.  The rank rule, the LMedS factor with p = 5 and the 2.5 sigma cut are this package's
    definitions and untried on a trained checkpoint."""
    xy, count = matches.xy, matches.count
    B, N = _matches_args("residual_stats", matches)
    poses, single = _pose_stack("residual_stats", poses, B)
    device_tensors("residual_stats", (("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None),
                                      ("poses", poses, torch.float32, None)))
    _cameras("residual_stats", intrinsics, None, B)
    if N > 2 ** 24:
        raise ValueError(f"residual_stats: need N <= 2^24, got N = {N}")
    qs, ts = _levels("residual_stats", "q", q, 1.0), _levels("residual_stats", "thresholds", thresholds, float(np.finfo(np.float64).max))
    P, Q, T, dev = int(poses.shape[1]), len(qs), len(ts), xy.device
    usable = torch.empty(B, P, dtype=torch.int32, device=dev)
    quant = torch.empty(B, P, Q, dtype=torch.float64, device=dev)
    within = torch.empty(B, P, T, dtype=torch.int32, device=dev)
    sigma = torch.empty(B, P, 2, dtype=torch.float64, device=dev)
    status = torch.empty(B, P, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_residual_stats", xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), poses.data_ptr(), qs, ts, B, N, P, Q, T,
                  usable.data_ptr(), quant.data_ptr(), within.data_ptr(), sigma.data_ptr(), status.data_ptr(), _hip.stream_handle())
    out = {"usable": usable, "quant": quant, "within": within, "sigma": sigma, "status": status}
    return {k: v[:, 0] for k, v in out.items()} if single else out


@torch.no_grad()
def select_pose(matches: Matches, intrinsics: torch.Tensor, rel_pose: Optional[torch.Tensor] = None, hypotheses: int = 1024,
                inlier_px: float = 1.0, seed: int = 0, solver: str = "8pt", sigma_px: float = 0.5, iters: int = 10,
                scale_px: float = 2.0, **lo_msac) -> Dict:
    """The pose of two photos without knowing whether they show a room, a wall or a turn on a tripod: ransac_pose and refine_pose
    from its pose (E); homography_pose with min_baseline 0 and refine_homography in both modes from its H (the plane, the rotation
    alone); cpn_ransac_score_h and cpn_ransac_finish_h on ONE slot, the refined plane, for its decomposition, vote and twin;
    model_gric; the picked model's pose by torch.where.  Twelve launches, nothing read on the host.  A model takes part where its
    producers' statuses say it exists (built on the device): E where ransac_pose's is 0 and refine_pose's 0 or 1; the plane where
    homography_pose's is 0 or 3, its refinement's 0 or 1 and the one-slot finish's 0; the rotation where homography_pose's is 0 or 3
    and its refinement's 0 or 1 -> `pose` (B, 4, 4) fp32 (rel_pose, or the identity without one, where no model is in), `model`
    (B) int32 (0 E, 1 plane, 2 rotation, -1 none), `gric`, `label`, `stats` (model_gric's), `avail` (B, 3) uint8, and the
    producers' dicts: `ransac`, `refined`, `homography`, `plane` (the one-slot finish's dict - pose, twin, H with sigma_2 = 1,
    inlier, stats - with `H_refined`, the unit h, and `refine_stats` beside it) and `rotation` (refine_homography's).
    The verdict is only as good as the refinement: on the unrefined RANSAC winners GRIC misreads the pure rotation (README, round
    23).  sigma_px is this package's choice and untried on a trained checkpoint.  ransac_pose's score, lo, lo_iters and lo_scale_px
    (round 24) are handed on to it: two more launches with lo > 0, and `ransac` gains its keys `score` and `lo`."""
    if solver not in _SOLVERS:
        raise ValueError(f"select_pose: solver must be one of {_SOLVERS}, got {solver!r}")
    if set(lo_msac) - _LO_KEYWORDS:
        raise ValueError(f"select_pose: unknown keywords {sorted(set(lo_msac) - _LO_KEYWORDS)}")
    if not 0.0 < float(sigma_px) < float("inf"):
        raise ValueError(f"select_pose: need a finite sigma_px > 0, got {sigma_px}")
    found = ransac_pose(matches, intrinsics, rel_pose, hypotheses=hypotheses, inlier_px=inlier_px, seed=seed, solver=solver, **lo_msac)
    refined = refine_pose(matches, intrinsics, found["pose"], iters=iters, scale_px=scale_px)
    homog = homography_pose(matches, intrinsics, rel_pose, hypotheses=hypotheses, inlier_px=inlier_px, seed=seed, min_baseline=0.0)
    flat = refine_homography(matches, intrinsics, homog["H"], model="plane", iters=iters, scale_px=scale_px)
    turn = refine_homography(matches, intrinsics, homog["H"], model="rotation", iters=iters, scale_px=scale_px)
    xy, count = matches.xy, matches.count
    B, N = int(xy.shape[0]), int(xy.shape[1])
    dev, px = xy.device, float(inlier_px)
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    one = torch.ones(B, 1, dtype=torch.uint8, device=dev)
    partial = torch.empty(B, chunks, 1, dtype=torch.int32, device=dev)
    plane = {"pose": torch.empty(B, 4, 4, dtype=torch.float32, device=dev), "twin": torch.empty(B, 4, 4, dtype=torch.float32, device=dev),
             "H": torch.empty(B, 9, dtype=torch.float64, device=dev), "inlier": torch.empty(B, N, dtype=torch.uint8, device=dev),
             "stats": torch.empty(B, 12, dtype=torch.float64, device=dev)}
    rel = 0 if rel_pose is None else rel_pose.data_ptr()
    with torch.cuda.device(dev):
        s = _hip.stream_handle()
        _hip.call("cpn_ransac_score_h", flat["H"].data_ptr(), one.data_ptr(), xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), B, N,
                  1, px, partial.data_ptr(), s)
        _hip.call("cpn_ransac_finish_h", flat["H"].data_ptr(), one.data_ptr(), partial.data_ptr(), xy.data_ptr(), count.data_ptr(),
                  intrinsics.data_ptr(), rel, B, N, 1, px, 0.0, plane["pose"].data_ptr(), plane["twin"].data_ptr(), plane["H"].data_ptr(),
                  plane["inlier"].data_ptr(), plane["stats"].data_ptr(), s)
    plane["H_refined"], plane["refine_stats"] = flat["H"], flat["stats"]
    h_ok = (homog["stats"][:, 11] == 0) | (homog["stats"][:, 11] == 3)
    avail = torch.stack(((found["stats"][:, 7] == 0) & (refined["stats"][:, 7] <= 1),
                         h_ok & (flat["stats"][:, 7] <= 1) & (plane["stats"][:, 11] == 0),
                         h_ok & (turn["stats"][:, 7] <= 1)), dim=1).to(torch.uint8).contiguous()
    verdict = model_gric(matches, intrinsics, refined["pose"], flat["H"], turn["H"], avail, sigma_px=sigma_px)
    model = verdict["stats"][:, 0].to(torch.int32)
    none = rel_pose if rel_pose is not None else torch.eye(4, dtype=torch.float32, device=dev).expand(B, 4, 4)
    pick = model[:, None, None]
    pose = torch.where(pick == 0, refined["pose"], torch.where(pick == 1, plane["pose"], torch.where(pick == 2, turn["pose"], none)))
    return {"pose": pose.contiguous(), "model": model, "gric": verdict["gric"], "label": verdict["label"], "stats": verdict["stats"],
            "avail": avail, "ransac": found, "refined": refined, "homography": homog, "plane": plane, "rotation": turn}


_STARTS = ("network", "ransac", "best")
_S_STARTS = ("network", "selected")
_H_STARTS = ("network", "homography")
_SOLVERS = ("8pt", "5pt")
_SCORES = ("inliers", "msac")
_LO_KEYWORDS = {"score", "lo", "lo_iters", "lo_scale_px"}


def _ransac_keywords(who: str, ransac: Dict) -> Tuple[Dict, str]:
    if not isinstance(ransac, dict):
        raise ValueError(f"{who}: ransac must be None or a dict of ransac_pose's keywords and `start`, got {type(ransac).__name__}")
    kw = dict(ransac)
    start = kw.pop("start", "network")
    if start not in _STARTS:
        raise ValueError(f"{who}: ransac['start'] must be one of {_STARTS}, got {start!r}")
    unknown = set(kw) - {"hypotheses", "inlier_px", "seed", "solver"} - _LO_KEYWORDS
    if unknown:
        raise ValueError(f"{who}: ransac holds unknown keywords {sorted(unknown)}")
    if kw.get("solver", "8pt") not in _SOLVERS:
        raise ValueError(f"{who}: ransac['solver'] must be one of {_SOLVERS}, got {kw['solver']!r}")
    return kw, start


def _homography_keywords(who: str, homography: Dict) -> Tuple[Dict, str]:
    if not isinstance(homography, dict):
        raise ValueError(f"{who}: homography must be None or a dict of homography_pose's keywords and `start`, got "
                         f"{type(homography).__name__}")
    kw = dict(homography)
    start = kw.pop("start", "network")
    if start not in _H_STARTS:
        raise ValueError(f"{who}: homography['start'] must be one of {_H_STARTS}, got {start!r}")
    unknown = set(kw) - {"hypotheses", "inlier_px", "seed", "min_baseline"}
    if unknown:
        raise ValueError(f"{who}: homography holds unknown keywords {sorted(unknown)}")
    return kw, start


def _select_keywords(who: str, select_kw: Dict) -> Tuple[Dict, str]:
    if not isinstance(select_kw, dict):
        raise ValueError(f"{who}: select must be None or a dict of select_pose's keywords and `start`, got {type(select_kw).__name__}")
    kw = dict(select_kw)
    start = kw.pop("start", "network")
    if start not in _S_STARTS:
        raise ValueError(f"{who}: select['start'] must be one of {_S_STARTS}, got {start!r}")
    unknown = set(kw) - {"hypotheses", "inlier_px", "seed", "solver", "sigma_px", "iters", "scale_px"} - _LO_KEYWORDS
    if unknown:
        raise ValueError(f"{who}: select holds unknown keywords {sorted(unknown)}")
    if kw.get("solver", "8pt") not in _SOLVERS:
        raise ValueError(f"{who}: select['solver'] must be one of {_SOLVERS}, got {kw['solver']!r}")
    return kw, start


def _triangulate_keywords(who: str, triangulate: Dict, refine: bool, ransac: Optional[Dict], select_kw: Optional[Dict]):
    if not isinstance(triangulate, dict):
        raise ValueError(f"{who}: triangulate must be None or a dict of `pose`, `images` and `adjust`, got {type(triangulate).__name__}")
    unknown = set(triangulate) - {"pose", "images", "adjust"}
    if unknown:
        raise ValueError(f"{who}: triangulate holds unknown keywords {sorted(unknown)}")
    pose = triangulate.get("pose", "network")
    asked = {"network": True, "refined": bool(refine), "ransac": ransac is not None, "selected": select_kw is not None}
    if pose not in asked:
        raise ValueError(f"{who}: triangulate['pose'] must be one of {tuple(asked)}, got {pose!r}")
    if not asked[pose]:
        raise ValueError(f"{who}: triangulate['pose'] = {pose!r} needs that estimator to run (refine=True, ransac={{..}} or select={{..}})")
    adjust = triangulate.get("adjust")
    if adjust is not None:
        if not isinstance(adjust, dict):
            raise ValueError(f"{who}: triangulate['adjust'] must be None or a dict of bundle_adjust's keywords, got {type(adjust).__name__}")
        unknown = set(adjust) - {"iters", "scale_px", "ftol", "min_rows", "inliers_only"}
        if unknown:
            raise ValueError(f"{who}: triangulate['adjust'] holds unknown keywords {sorted(unknown)}")
        if adjust.get("inliers_only") and pose not in ("ransac", "selected"):
            raise ValueError(f"{who}: triangulate['adjust']['inliers_only'] needs triangulate['pose'] \"ransac\" or \"selected\", got {pose!r}")
    return pose, triangulate.get("images"), adjust


@torch.no_grad()
def from_flows(flow: Sequence[torch.Tensor], intrinsics: torch.Tensor, rel_pose: torch.Tensor, S: int = 256, refine: bool = True,
               max_cycle_px: float = 10.0, max_epi_px: Optional[float] = None, stride: int = 4, iters: int = 10,
               scale_px: float = 2.0, ransac: Optional[Dict] = None, homography: Optional[Dict] = None,
               select: Optional[Dict] = None, triangulate: Optional[Dict] = None) -> Dict:
    """from_pair's second half, for flows and a pose that get_z has already returned: four launches and the mask between them,
    no host read.  ransac: None, or a dict of ransac_pose's keywords (hypotheses, inlier_px, seed, solver, and round 24's score, lo,
    lo_iters, lo_scale_px: two more launches with lo > 0) and `start`: three more
    launches, and the result gains the key `ransac` (ransac_pose's dict).  start="network" (the default) refines from rel_pose
    as without it, "ransac" from RANSAC's pose, "best" per pair from the one with more inliers under ransac_pose's rule (a tie
    and a status other than 0 go to rel_pose; chosen by torch.where on the device).
    homography: None, or a dict of homography_pose's keywords (hypotheses, inlier_px, seed, min_baseline) and `start`: three more
    launches, and the result gains the key `homography` (homography_pose's dict).  start="homography" refines from its pose where
    its status is 0 and from rel_pose elsewhere (torch.where on the device); a start other than "network" in both dicts is a
    ValueError.  Without the keyword nothing changes: no launch, no key.
    select: None, or a dict of select_pose's keywords (hypotheses, inlier_px, seed, solver, sigma_px, iters, scale_px) and `start`:
    select_pose's twelve launches, and the result gains the key `select` (select_pose's dict).  start="selected" refines from the
    selected pose where model_gric's status is 0 and from rel_pose elsewhere; a second start other than "network" among ransac,
    homography and select is the same ValueError.  Without the keyword nothing changes: no launch, no key.
    triangulate: None, or a dict of `pose` ("network", the default, "refined", "ransac" or "selected": rel_pose, refine_pose's,
    ransac_pose's or select_pose's pose, each of which must have been asked for) and `images` (None, or the pair's photos
    (B, 2, S, S, 3) fp32): one more launch, and the result gains the key `points`, coponerf_amd.triangulate.points' dict of the
    matches under that pose (round 26 of the header), and `adjust` (None, or a dict of coponerf_amd.triangulate.bundle_adjust's
    keywords iters, scale_px, ftol, min_rows and `inliers_only`, which hands it ransac_pose's mask): one launch more, and the
    result gains the key `adjust`, bundle_adjust's dict from those points and that pose (round 27).  Without the keyword nothing
    changes: no launch, no key."""
    if triangulate is not None:
        tri_pose, tri_images, tri_adjust = _triangulate_keywords("from_flows", triangulate, refine, ransac, select)
    if ransac is not None:
        ransac_kw, start = _ransac_keywords("from_flows", ransac)
    if homography is not None:
        homography_kw, h_start = _homography_keywords("from_flows", homography)
        if h_start != "network" and ransac is not None and start != "network":
            raise ValueError(f"from_flows: ransac['start'] = {start!r} and homography['start'] = {h_start!r} both name a start; "
                             "one of them must be \"network\"")
    if select is not None:
        select_kw, s_start = _select_keywords("from_flows", select)
        named = [f"{k}['start'] = {v!r}" for k, v in (("ransac", start if ransac is not None else "network"),
                                                      ("homography", h_start if homography is not None else "network"),
                                                      ("select", s_start)) if v != "network"]
        if s_start != "network" and len(named) > 1:
            raise ValueError(f"from_flows: {' and '.join(named)} all name a start; only one of them may differ from \"network\"")
    fields = match_fields(flow, intrinsics, rel_pose, S)
    matches = _select_matches(fields, max_cycle_px=max_cycle_px, max_epi_px=max_epi_px, stride=stride)
    result = {"matches": matches, "rel_pose": rel_pose, "pose": None, "stats": None, "fields": fields}
    begin = rel_pose
    if ransac is not None:
        found = result["ransac"] = ransac_pose(matches, intrinsics, rel_pose, **ransac_kw)
        st = found["stats"]
        if start == "ransac":
            begin = found["pose"]
        elif start == "best":
            better = (st[:, 7] == 0) & (st[:, 0] > st[:, 4])
            begin = torch.where(better[:, None, None], found["pose"], rel_pose)
    if homography is not None:
        plane = result["homography"] = homography_pose(matches, intrinsics, rel_pose, **homography_kw)
        if h_start == "homography":
            begin = torch.where((plane["stats"][:, 11] == 0)[:, None, None], plane["pose"], rel_pose)
    if select is not None:
        chosen = result["select"] = select_pose(matches, intrinsics, rel_pose, **select_kw)
        if s_start == "selected":
            begin = torch.where((chosen["stats"][:, 6] == 0)[:, None, None], chosen["pose"], rel_pose)
    if refine:
        result.update(refine_pose(matches, intrinsics, begin, iters=iters, scale_px=scale_px))
    if triangulate is not None:
        from . import triangulate as _triangulate                   # it imports this module
        under = {"network": rel_pose, "refined": result["pose"], "ransac": result["ransac"]["pose"] if ransac is not None else None,
                 "selected": result["select"]["pose"] if select is not None else None}[tri_pose]
        under = under.contiguous()
        result["points"] = _triangulate.points(matches, intrinsics, under, tri_images)
        if tri_adjust is not None:
            kw = dict(tri_adjust)
            mask = None
            if kw.pop("inliers_only", False):
                mask = (result["ransac"] if tri_pose == "ransac" else result["select"]["ransac"])["inlier"]
            result["adjust"] = _triangulate.bundle_adjust(result["points"], matches, intrinsics, under, inlier=mask, **kw)
    return result


@torch.no_grad()
def from_pair(model, model_input: Dict, S: int = 256, refine: bool = True, **select_and_refine_keywords) -> Dict:
    """The matches of the pair(s) in model_input (prepare_pair's dict, or any dict get_z takes).  get_z runs once; its flows
    and its rel_pose - the ones novel_views.render_path hands on - go through match_fields, select and, with refine=True,
    refine_pose.  Keywords: select's max_cycle_px, max_epi_px, stride, refine_pose's iters, scale_px and from_flows' ransac,
    homography, select and triangulate (with a dict the result gains the key `ransac`, `homography`, `select` or `points`).  Returns `matches` (a
    Matches), `rel_pose` (B, 4, 4) as estimated, `pose` and `stats` as refine_pose returns them (None with refine=False) and
    `fields`, match_fields' dict.  Nothing is read on the host; Matches.numpy is the read."""
    _, rel_pose, flow = model.get_z(model_input)
    flows = (flow[0].float().contiguous(), flow[1].float().contiguous())
    intrinsics = model_input["context"]["intrinsics"].float().contiguous()
    return from_flows(flows, intrinsics, rel_pose.float().contiguous(), S=S, refine=refine, **select_and_refine_keywords)


def photo_coords(xy, Hi, Wi, size: int) -> np.ndarray:
    """Matches (n, 4) = (x0, y0, x1, y1) in the pixels of the size x size model images -> the same in the pixels of the original
    photos of Hi x Wi pixels (two ints, or a pair of ints each where the photos differ): the inverse of the centre square crop
    and the scale of novel_views.fit_intrinsics, x_photo = x / s + (Wi - side) / 2 with s = size / side.  float64, host."""
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 4:
        raise ValueError(f"photo_coords: xy must be (n, 4), got {xy.shape}")
    Hs = (int(Hi), int(Hi)) if np.ndim(Hi) == 0 else tuple(int(v) for v in Hi)
    Ws = (int(Wi), int(Wi)) if np.ndim(Wi) == 0 else tuple(int(v) for v in Wi)
    if len(Hs) != 2 or len(Ws) != 2:
        raise ValueError("photo_coords: Hi and Wi are ints or pairs of ints (view 0, view 1)")
    out = np.empty_like(xy)
    for v in range(2):
        _, _, side = crop_window(Hs[v], Ws[v])
        s = size / side
        out[:, 2 * v + 0] = xy[:, 2 * v + 0] / s + (Ws[v] - side) / 2.0
        out[:, 2 * v + 1] = xy[:, 2 * v + 1] / s + (Hs[v] - side) / 2.0
    return out
