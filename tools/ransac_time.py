"""What the pose from the matches alone costs (coponerf_amd/matches.py: ransac_pose), on one MI355X, in one
process: two 256 x 256 pairs with 64 x 64 flows and about 6 000 matches each (round 16's workload), 1024 hypotheses, 1 px.

The flows are those of two cameras looking at smooth surfaces that are NO planes (tools/matches_time.py's tilted plane is the
degenerate case of the linear 8-point solver: nearly every hypothesis would fail the rank test and the score kernel would have
nothing to do), one surface per direction, ray-cast in float64 at the flow cells' centres; every match inside the image is kept
(the two surfaces do not agree, so the cycle error says nothing here).  rel_pose is the true pose turned by 30 degrees (these matches are exact, so
refine_pose still converges from it: what it does with outliers is tests/test_ransac_ref.py's subject, not this script's).

  (a) the three kernels of csrc/ransac.hip on the Matches of the default stride (cap = 2 S S rows per pair, about 6 000 below
      the count), ransac_pose as a whole, from_flows without `ransac` (the parent's call, re-measured here) and with
      ransac={"start": "ransac"}: HIP events around `iters` back-to-back calls, the median of `rounds` such windows.
  (b) the same rule from stock operators, in the same process: the 8 x 9 systems of the kernel's own samples, their null vectors
      by a batched torch.linalg.svd, an (Hn, n) float64 residual matrix per pair, the counts and argmax.  The counts of the pairs
      are read once before the timing (boolean shapes need them on the host).
  (c) what came out: inliers of the winner against rel_pose's, degrees from the truth before and after refine_pose, and the
      winner's count of the stock form.

  (d) the 5-point solver (csrc/ransac5.hip) in the same process, written to --out5: cpn_ransac_hypotheses5 on
      its own; cpn_ransac_score and cpn_ransac_finish at 10 HN slots - with the solver's own validity, with the valid slots
      packed to the front of the buffer (what the invalid lanes between them cost: a wave is busy while one of its lanes is)
      and with every slot invalid (the launch's fixed part); ransac_pose(solver="5pt") at HN and at HN / 4 samples and
      from_flows with it, beside the 8-point figures of (a); and what came out.

  (e) the homography model (csrc/ransac_h.hip) in the same process, written to --outh, on the curved pairs of
      (a) and on two pairs of about 6 000 exact matches on a wall in buffers of the same N rows: its three kernels; the score
      kernel once more with every slot declared valid (the 8-point score kernel of (a) has nearly every slot to count, the
      homographies' own validity leaves about half: this is the like-for-like figure, and its ratio to (a)'s is recorded);
      homography_pose as a whole beside ransac_pose 8-point and 5-point on the same Matches; the same rule from stock operators
      (batched torch.linalg.svd null vectors of the kernel's own samples, an (Hn, n) float64 transfer-error matrix in both
      views, argmax); and what came out of all three models.

There is no pass / fail time: the numbers are recorded.

    python tools/ransac_time.py [--rounds 5] [--iters 20] [--out profiles/r20_ransac.json] [--out5 profiles/r21_ransac5.json]
                                [--outh profiles/r22_homography.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matches_time import angle_deg, dir_deg, rodrigues       # noqa: E402
from summaries_time import spread, time_form                  # noqa: E402
from coponerf_amd import _hip, matches as mt                   # noqa: E402

S, HF, B = 256, 64, 2
HN, PX, SEED = 1024, 1.0, 0


def curved_pairs(dev):
    """(flow0, flow1 (B, 2, 64, 64), intrinsics (B, 2, 4, 4), rel_pose (B, 4, 4) 30 degrees off, true (B, 4, 4)) fp32 on the device."""
    s = S / HF
    c = (torch.arange(HF, dtype=torch.float64) + 0.5) * s - 0.5
    y, x = torch.meshgrid(c, c, indexing="ij")
    f0, f1, Ks, P0, Pt = [], [], [], [], []
    for b in range(B):
        f = 210.0 + 15.0 * b
        R, t = rodrigues((0.2, 1.0, 0.1), 7.0 + 2.0 * b), torch.tensor([0.45, 0.04, 0.1 + 0.05 * b], dtype=torch.float64)
        ray = torch.stack(((x - S / 2) / f, (y - S / 2) / f, torch.ones_like(x)), -1)
        z0 = 3.0 + torch.sin(x / 40.0) + 0.8 * torch.cos(y / 32.0) + 0.006 * x
        z1 = 3.5 + 0.9 * torch.cos(x / 48.0 + 1.0) + torch.sin(y / 24.0) - 0.005 * y
        X1 = (ray * z0[..., None] - t) @ R                          # view 0's pixels seen from view 1
        X0 = (ray * z1[..., None]) @ R.T + t                        # view 1's pixels seen from view 0
        for X, out in ((X1, f0), (X0, f1)):
            out.append(torch.stack((f * X[..., 0] / X[..., 2] + S / 2 - x, f * X[..., 1] / X[..., 2] + S / 2 - y)) / s)
        K = torch.eye(4, dtype=torch.float64)
        K[0, 0] = K[1, 1] = f
        K[0, 2] = K[1, 2] = S / 2
        Ks.append(torch.stack((K, K)))
        true, start = torch.eye(4, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
        true[:3, :3], true[:3, 3] = R, t
        start[:3, :3] = rodrigues((1.0, -0.5, 0.7), 30.0) @ R
        start[:3, 3] = rodrigues(torch.linalg.cross(t, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).tolist(), 30.0) @ t
        Pt.append(true)
        P0.append(start)
    return tuple(torch.stack(v).float().contiguous().to(dev) for v in (f0, f1, Ks, P0, Pt))


def stock_ransac(xy, counts, intr, sample, px=PX):
    """The rule from stock operators, one pair after the other -> (winner index, winner count) per pair, on the device."""
    out = []
    for b, n in enumerate(counts):
        rows = xy[b, :n].double()
        k0, k1 = intr[b, 0].double(), intr[b, 1].double()
        a = torch.stack(((rows[:, 0] - k0[0, 2]) / k0[0, 0], (rows[:, 1] - k0[1, 2]) / k0[1, 1], torch.ones_like(rows[:, 0])), -1)
        bb = torch.stack(((rows[:, 2] - k1[0, 2]) / k1[0, 0], (rows[:, 3] - k1[1, 2]) / k1[1, 1], torch.ones_like(rows[:, 0])), -1)
        f0, f1 = torch.stack((k0[0, 0], k0[1, 1])), torch.stack((k1[0, 0], k1[1, 1]))
        idx = sample[b].long()
        A = (a[idx][..., :, None] * bb[idx][..., None, :]).reshape(-1, 8, 9)
        Em = torch.linalg.svd(A, full_matrices=True)[2][:, 8].reshape(-1, 3, 3)
        Eb, Ea = torch.einsum("hij,nj->hni", Em, bb), torch.einsum("hij,ni->hnj", Em, a)
        num = (a[None] * Eb).sum(-1)
        g = torch.cat((Eb[..., :2] / f0, Ea[..., :2] / f1), -1)
        r = num / (g * g).sum(-1).sqrt()
        cnt = (r.abs() <= px).sum(1)
        win = cnt.argmax()
        out.append(torch.stack((win, cnt[win])))
    return torch.stack(out)


def windows(fn, rounds, iters):
    fn()
    fn()
    return spread([time_form(fn, iters)[0] for _ in range(rounds)])


def five_point(m, flows, intr, pose, true, counts, sel, args, eight):
    """(d) of the module's docstring -> the dict written to --out5; `eight` holds (a)'s kernels and calls."""
    dev, N, SL = intr.device, int(m.xy.shape[1]), 10 * HN
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    E = torch.empty(B, SL, 9, dtype=torch.float64, device=dev)
    sample = torch.empty(B, HN, 5, dtype=torch.int32, device=dev)
    valid = torch.empty(B, SL, dtype=torch.uint8, device=dev)
    partial = torch.empty(B, chunks, SL + 1, dtype=torch.int32, device=dev)
    po, inl = torch.empty(B, 4, 4, device=dev), torch.empty(B, N, dtype=torch.uint8, device=dev)
    st = torch.empty(B, 8, dtype=torch.float64, device=dev)
    s = _hip.stream_handle()
    xy, cn, K, P = m.xy.data_ptr(), m.count.data_ptr(), intr.data_ptr(), pose.data_ptr()
    hyp = lambda: _hip.call("cpn_ransac_hypotheses5", xy, cn, K, B, N, HN, SEED, E.data_ptr(), sample.data_ptr(), valid.data_ptr(), s)
    hyp()
    order = torch.argsort(valid, dim=1, descending=True, stable=True)
    packed_E = torch.gather(E, 1, order[..., None].expand(-1, -1, 9)).contiguous()
    packed_v, none_v = torch.gather(valid, 1, order).contiguous(), torch.zeros_like(valid)

    def score(Eb, vb):
        return lambda: _hip.call("cpn_ransac_score", Eb.data_ptr(), vb.data_ptr(), xy, cn, K, P, B, N, SL, PX, partial.data_ptr(), s)
    kernels = {"ransac_hypotheses5_ms": hyp, "ransac_score_10x_slots_ms": score(E, valid),
               "ransac_score_valid_slots_packed_ms": score(packed_E, packed_v), "ransac_score_no_valid_slot_ms": score(E, none_v)}
    out = {"kernels": {k: windows(fn, args.rounds, args.iters) for k, fn in kernels.items()}}
    score(E, valid)()
    out["kernels"]["ransac_finish_10x_slots_ms"] = windows(
        lambda: _hip.call("cpn_ransac_finish", E.data_ptr(), valid.data_ptr(), partial.data_ptr(), xy, cn, K, P, B, N, SL, PX,
                          po.data_ptr(), inl.data_ptr(), st.data_ptr(), s), args.rounds, args.iters)
    opts = {"hypotheses": HN, "inlier_px": PX, "seed": SEED, "start": "ransac", "solver": "5pt"}
    forms = {"ransac_pose_5pt_ms": lambda: mt.ransac_pose(m, intr, pose, HN, PX, SEED, solver="5pt"),
             "ransac_pose_5pt_quarter_samples_ms": lambda: mt.ransac_pose(m, intr, pose, HN // 4, PX, SEED, solver="5pt"),
             "refine_pose_ms": lambda: mt.refine_pose(m, intr, pose),
             "from_flows_with_ransac_5pt_ms": lambda: mt.from_flows(flows, intr, pose, S, ransac=opts, **sel)}
    out["calls"] = {k: windows(fn, args.rounds, args.iters) for k, fn in forms.items()}
    out["eight_point_same_process"] = eight
    ours = mt.from_flows(flows, intr, pose, S, ransac=opts, **sel)
    quarter = mt.ransac_pose(m, intr, pose, HN // 4, PX, SEED, solver="5pt")

    def off(Pm):
        return [[angle_deg(Pm[b, :3, :3], true[b, :3, :3]), dir_deg(Pm[b, :3, 3], true[b, :3, 3])] for b in range(B)]
    out["result"] = {"valid_slots_of": SL, "valid_slots": [int(v) for v in valid.sum(1).cpu()],
                     "valid_samples": [int(v) for v in valid.view(B, HN, 10).any(2).sum(1).cpu()],
                     "ransac_stats": [[float(v) for v in row] for row in ours["ransac"]["stats"].cpu()],
                     "ransac_stats_quarter_samples": [[float(v) for v in row] for row in quarter["stats"].cpu()],
                     "matches_per_pair": counts,
                     "degrees_from_truth": {"ransac_5pt": off(ours["ransac"]["pose"]), "refined_from_ransac_5pt": off(ours["pose"]),
                                            "ransac_5pt_quarter_samples": off(quarter["pose"])}}
    return out


def wall_matches(dev, N, n=6000):
    """B pairs of about n exact matches on the plane (0.25, -0.1, 1) . X0 = 3 seen by curved_pairs' cameras, in N-row buffers
    -> (Matches, true (B, 4, 4) float64 on the host)."""
    gen = torch.Generator().manual_seed(22)
    xy, counts, Pt = torch.zeros(B, N, 4, dtype=torch.float64), [], []
    for b in range(B):
        f = 210.0 + 15.0 * b
        R, t = rodrigues((0.2, 1.0, 0.1), 7.0 + 2.0 * b), torch.tensor([0.45, 0.04, 0.1 + 0.05 * b], dtype=torch.float64)
        p0 = torch.rand(n, 2, generator=gen, dtype=torch.float64) * S
        ray = torch.cat(((p0 - S / 2) / f, torch.ones(n, 1, dtype=torch.float64)), 1)
        depth = 3.0 / (ray @ torch.tensor([0.25, -0.1, 1.0], dtype=torch.float64))
        X1 = (ray * depth[:, None] - t) @ R
        p1 = f * X1[:, :2] / X1[:, 2:] + S / 2
        keep = ((p1 >= 0) & (p1 <= S - 1)).all(1)
        rows = torch.cat((p0, p1), 1)[keep]
        xy[b, :len(rows)] = rows
        counts.append(len(rows))
        true = torch.eye(4, dtype=torch.float64)
        true[:3, :3], true[:3, 3] = R, t
        Pt.append(true)
    return mt.Matches(xy.float().contiguous().to(dev), None, torch.tensor(counts, dtype=torch.int32, device=dev)), torch.stack(Pt), counts


def stock_homography(xy, counts, intr, sample, px=PX):
    """homography_pose's rule from stock operators, one pair after the other -> (winner index, winner count) per pair, on the
    device: the 8 x 9 systems of the kernel's own samples, their null vectors by a batched torch.linalg.svd, an (Hn, n) float64
    transfer-error matrix in both views, the counts and argmax.  (It does not drop the hypotheses that map their own sample
    behind a camera: they count few inliers.)"""
    out = []
    for b, n in enumerate(counts):
        rows = xy[b, :n].double()
        k0, k1 = intr[b, 0].double(), intr[b, 1].double()
        a = torch.stack(((rows[:, 0] - k0[0, 2]) / k0[0, 0], (rows[:, 1] - k0[1, 2]) / k0[1, 1], torch.ones_like(rows[:, 0])), -1)
        bb = torch.stack(((rows[:, 2] - k1[0, 2]) / k1[0, 0], (rows[:, 3] - k1[1, 2]) / k1[1, 1], torch.ones_like(rows[:, 0])), -1)
        f0, f1 = torch.stack((k0[0, 0], k0[1, 1])), torch.stack((k1[0, 0], k1[1, 1]))
        idx = sample[b].long()
        sa, sb = a[idx], bb[idx]                                    # (Hn, 4, 3)
        zero = torch.zeros_like(sb)
        A = torch.stack((torch.cat((sb, zero, -sa[..., 0:1] * sb), -1), torch.cat((zero, sb, -sa[..., 1:2] * sb), -1)), 2).reshape(-1, 8, 9)
        Hm = torch.linalg.svd(A, full_matrices=True)[2][:, 8].reshape(-1, 3, 3)
        Hm = Hm * torch.sign(torch.linalg.det(Hm))[:, None, None]
        Hb, Ga = torch.einsum("hij,nj->hni", Hm, bb), torch.einsum("hij,nj->hni", torch.linalg.inv(Hm), a)
        d0 = ((Hb[..., :2] / Hb[..., 2:] - a[None, :, :2]) * f0).norm(dim=-1)
        d1 = ((Ga[..., :2] / Ga[..., 2:] - bb[None, :, :2]) * f1).norm(dim=-1)
        cnt = ((Hb[..., 2] > 0) & (Ga[..., 2] > 0) & (d0 <= px) & (d1 <= px)).sum(1)
        win = cnt.argmax()
        out.append(torch.stack((win, cnt[win])))
    return torch.stack(out)


def homography(m, intr, pose, true, counts, args, other):
    """(e) of the module's docstring -> the dict written to --outh; `other` holds the 8-point and 5-point figures of this process."""
    dev, N = intr.device, int(m.xy.shape[1])
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    wall, wall_true, wall_counts = wall_matches(dev, N)
    s = _hip.stream_handle()
    K, P = intr.data_ptr(), pose.data_ptr()
    out = {"rows_per_pair_N": N, "matches_per_pair": {"curved": counts, "wall": wall_counts}, "kernels": {}, "calls": {}, "result": {}}

    def off(Pm, truth):
        return [[angle_deg(Pm[b, :3, :3].double().cpu(), truth[b, :3, :3].double().cpu()),
                 dir_deg(Pm[b, :3, 3].double().cpu(), truth[b, :3, 3].double().cpu())] for b in range(B)]
    for name, mm, truth, cnts in (("curved", m, true, counts), ("wall", wall, wall_true, wall_counts)):
        Hm = torch.empty(B, HN, 9, dtype=torch.float64, device=dev)
        sample = torch.empty(B, HN, 4, dtype=torch.int32, device=dev)
        valid = torch.empty(B, HN, dtype=torch.uint8, device=dev)
        partial = torch.empty(B, chunks, HN, dtype=torch.int32, device=dev)
        po, tw = torch.empty(B, 4, 4, device=dev), torch.empty(B, 4, 4, device=dev)
        Ho, st = torch.empty(B, 9, dtype=torch.float64, device=dev), torch.empty(B, 12, dtype=torch.float64, device=dev)
        inl = torch.empty(B, N, dtype=torch.uint8, device=dev)
        xy, cn = mm.xy.data_ptr(), mm.count.data_ptr()
        kernels = {
            "ransac_homographies_ms": lambda: _hip.call("cpn_ransac_homographies", xy, cn, K, B, N, HN, SEED, Hm.data_ptr(), sample.data_ptr(),
                                                        valid.data_ptr(), s),
            "ransac_score_h_ms": lambda: _hip.call("cpn_ransac_score_h", Hm.data_ptr(), valid.data_ptr(), xy, cn, K, B, N, HN, PX,
                                                   partial.data_ptr(), s),
            "ransac_finish_h_ms": lambda: _hip.call("cpn_ransac_finish_h", Hm.data_ptr(), valid.data_ptr(), partial.data_ptr(), xy, cn, K, P, B,
                                                    N, HN, PX, 0.0, po.data_ptr(), tw.data_ptr(), Ho.data_ptr(), inl.data_ptr(), st.data_ptr(), s)}
        out["kernels"][name] = {k: windows(fn, args.rounds, args.iters) for k, fn in kernels.items()}
        # the slots with something to count decide the score kernel's time: the same kernel with every slot valid, the invalid
        # ones filled with copies of the valid ones
        order = torch.argsort(valid, dim=1, descending=True, stable=True)
        nv = valid.sum(1, keepdim=True).clamp(min=1).long()
        pick = torch.gather(order, 1, torch.arange(HN, device=dev)[None].expand(B, -1) % nv)
        Hall, every = torch.gather(Hm, 1, pick[..., None].expand(-1, -1, 9)).contiguous(), torch.ones_like(valid)
        out["kernels"][name]["ransac_score_h_every_slot_valid_ms"] = windows(
            lambda: _hip.call("cpn_ransac_score_h", Hall.data_ptr(), every.data_ptr(), xy, cn, K, B, N, HN, PX, partial.data_ptr(), s),
            args.rounds, args.iters)
        forms = {"homography_pose_ms": lambda: mt.homography_pose(mm, intr, pose, HN, PX, SEED),
                 "ransac_pose_8pt_ms": lambda: mt.ransac_pose(mm, intr, pose, HN, PX, SEED),
                 "ransac_pose_5pt_ms": lambda: mt.ransac_pose(mm, intr, pose, HN, PX, SEED, solver="5pt"),
                 "stock_homography_ms": lambda: stock_homography(mm.xy, cnts, intr, sample)}
        out["calls"][name] = {k: windows(fn, args.rounds, args.iters if "stock" not in k else max(args.iters // 4, 2))
                              for k, fn in forms.items()}
        got = mt.homography_pose(mm, intr, pose, HN, PX, SEED)
        eight, five = mt.ransac_pose(mm, intr, pose, HN, PX, SEED), mt.ransac_pose(mm, intr, pose, HN, PX, SEED, solver="5pt")
        out["result"][name] = {"homography_stats": [[float(v) for v in row] for row in got["stats"].cpu()],
                               "valid_hypotheses": [int(v) for v in valid.sum(1).cpu()],
                               "stock_winner_and_count": stock_homography(mm.xy, cnts, intr, sample).cpu().tolist(),
                               "inliers_8pt_5pt": [[float(eight["stats"][b, 0]), float(five["stats"][b, 0])] for b in range(B)],
                               "degrees_from_truth": {"homography": off(got["pose"], truth), "twin": off(got["twin"], truth),
                                                      "ransac_8pt": off(eight["pose"], truth), "ransac_5pt": off(five["pose"], truth)}}
    # the score kernels on the same matches and the same number of slots with something to count: (nearly) all HN for the
    # 8-point solver on the curved pairs, all HN here once every slot is declared valid
    out["score_h_every_slot_over_score_8pt"] = round(out["kernels"]["curved"]["ransac_score_h_every_slot_valid_ms"]["median"] /
                                                     other["eight_point"]["kernels"]["ransac_score_ms"]["median"], 3)
    out["eight_and_five_point_same_process"] = other
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--out5", default=None)
    ap.add_argument("--outh", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ransac_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = curved_pairs(dev)
    sel = dict(max_cycle_px=1e9)
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "side": S, "flow_side": HF, "hypotheses": HN, "inlier_px": PX,
           "seed": SEED, "rounds": args.rounds, "iters": args.iters, "ms": "HIP events per call, windows of `iters` back-to-back calls"}

    m = mt.select(mt.match_fields((f0, f1), intr, pose, S), **sel)
    counts = [int(c) for c in m.count.cpu()]
    res["matches_per_pair"] = counts
    N = int(m.xy.shape[1])
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    E = torch.empty(B, HN, 9, dtype=torch.float64, device=dev)
    sample = torch.empty(B, HN, 8, dtype=torch.int32, device=dev)
    valid = torch.empty(B, HN, dtype=torch.uint8, device=dev)
    partial = torch.empty(B, chunks, HN + 1, dtype=torch.int32, device=dev)
    po = torch.empty(B, 4, 4, device=dev)
    inl = torch.empty(B, N, dtype=torch.uint8, device=dev)
    st = torch.empty(B, 8, dtype=torch.float64, device=dev)
    s = _hip.stream_handle()
    xy, cn, K, P = m.xy.data_ptr(), m.count.data_ptr(), intr.data_ptr(), pose.data_ptr()
    kernels = {
        "ransac_hypotheses_ms": lambda: _hip.call("cpn_ransac_hypotheses", xy, cn, K, B, N, HN, SEED, E.data_ptr(), sample.data_ptr(),
                                                  valid.data_ptr(), s),
        "ransac_score_ms": lambda: _hip.call("cpn_ransac_score", E.data_ptr(), valid.data_ptr(), xy, cn, K, P, B, N, HN, PX,
                                             partial.data_ptr(), s),
        "ransac_finish_ms": lambda: _hip.call("cpn_ransac_finish", E.data_ptr(), valid.data_ptr(), partial.data_ptr(), xy, cn, K, P, B, N,
                                              HN, PX, po.data_ptr(), inl.data_ptr(), st.data_ptr(), s)}
    res["rows_per_pair_N"] = N
    res["kernels"] = {k: windows(fn, args.rounds, args.iters) for k, fn in kernels.items()}
    # the same three on Matches cut to the rows in use: what a caller with a tight buffer pays
    tight = mt.Matches(m.xy[:, :max(counts)].contiguous(), None, m.count)
    forms = {
        "ransac_pose_ms": lambda: mt.ransac_pose(m, intr, pose, HN, PX, SEED),
        "ransac_pose_tight_rows_ms": lambda: mt.ransac_pose(tight, intr, pose, HN, PX, SEED),
        "from_flows_ms": lambda: mt.from_flows((f0, f1), intr, pose, S, **sel),
        "from_flows_with_ransac_ms": lambda: mt.from_flows((f0, f1), intr, pose, S, ransac={"hypotheses": HN, "inlier_px": PX, "seed": SEED,
                                                                                         "start": "ransac"}, **sel),
        "stock_ransac_ms": lambda: stock_ransac(m.xy, counts, intr, sample)}
    res["calls"] = {k: windows(fn, args.rounds, args.iters if "stock" not in k else max(args.iters // 4, 2)) for k, fn in forms.items()}

    # ---- what came out
    ours = mt.from_flows((f0, f1), intr, pose, S, ransac={"hypotheses": HN, "inlier_px": PX, "seed": SEED, "start": "ransac"}, **sel)
    plain = mt.from_flows((f0, f1), intr, pose, S, **sel)
    stock = stock_ransac(m.xy, counts, intr, sample).cpu().tolist()

    def off(Pm):
        return [[angle_deg(Pm[b, :3, :3], true[b, :3, :3]), dir_deg(Pm[b, :3, 3], true[b, :3, 3])] for b in range(B)]
    res["result"] = {"ransac_stats": [[float(v) for v in row] for row in ours["ransac"]["stats"].cpu()],
                     "valid_hypotheses": [int(v) for v in valid.sum(1).cpu()],
                     "stock_winner_and_count": stock,
                     "degrees_from_truth": {"rel_pose": off(pose), "refined_from_rel_pose": off(plain["pose"]),
                                            "ransac": off(ours["ransac"]["pose"]), "refined_from_ransac": off(ours["pose"])}}
    print(json.dumps(res, indent=1))
    res5 = dict({k: res[k] for k in ("device", "pairs", "side", "flow_side", "hypotheses", "inlier_px", "seed", "rounds", "iters", "ms")},
                **five_point(m, (f0, f1), intr, pose, true, counts, sel, args, {"kernels": res["kernels"], "calls": res["calls"]}))
    print(json.dumps(res5, indent=1))
    resh = dict({k: res[k] for k in ("device", "pairs", "side", "flow_side", "hypotheses", "inlier_px", "seed", "rounds", "iters", "ms")},
                **homography(m, intr, pose, true, counts, args,
                             {"eight_point": {"kernels": res["kernels"], "calls": res["calls"],
                                              "valid_hypotheses": res["result"]["valid_hypotheses"]},
                              "five_point": {"kernels": res5["kernels"], "calls": res5["calls"]}}))
    print(json.dumps(resh, indent=1))
    for path, what in ((args.out, res), (args.out5, res5), (args.outh, resh)):
        if path:
            with open(path, "w") as f:
                json.dump(what, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
