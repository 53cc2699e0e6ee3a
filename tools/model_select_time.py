"""What the verdict between E, a plane and a rotation alone costs (coponerf_amd/matches.py: select_pose), on one
MI355X, in one process: the two curved 256 x 256 pairs of tools/ransac_time.py (64 x 64 flows, about 6 000 matches each, buffers of
2 S S rows), 1024 hypotheses, 1 px, sigma_px 0.5, ten passes.

  (a) the new kernels on their own: cpn_refine_homography in both modes from homography_pose's H, cpn_model_gric on the refined
      models; beside them cpn_refine_pose from ransac_pose's pose, re-measured here (the figure the plane's refinement is held
      against: the same walk over the matches with a 6-parameter Jacobian).
  (b) select_pose as a whole beside the ransac_pose + refine_pose + homography_pose it contains, and from_flows with and without
      select={...}.
  (c) the same rule from stock operators, in the same process, for the part this round adds: both refinements (the residual and its
      full derivative as tensor expressions over all matches, the normal equations by masked float64 sums, torch.linalg.solve,
      torch.linalg.svd for the nearest rotation, torch.linalg.matrix_exp for the step) and GRIC (masked float64 sums), from the
      kernels' own ransac_pose / refine_pose / homography_pose results.  It must give the same `model`.  The counts of the pairs are
      read once before the timing.
  (d) what came out: gric, the pick, the margins, the statuses.

HIP events around `iters` back-to-back calls, the median of `rounds` such windows.  There is no pass / fail time: the numbers are
recorded.

    python tools/model_select_time.py [--rounds 5] [--iters 20] [--out profiles/r23_model_select.json]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ransac_time import B, HN, PX, S, SEED, curved_pairs, windows      # noqa: E402
from coponerf_amd import matches as mt                                  # noqa: E402

SIGMA, ITERS, SCALE = 0.5, 10, 2.0


def _points(rows, k0, k1):
    return ((rows[:, 0] - k0[0, 2]) / k0[0, 0], (rows[:, 1] - k0[1, 2]) / k0[1, 1], (rows[:, 2] - k1[0, 2]) / k1[0, 0],
            (rows[:, 3] - k1[1, 2]) / k1[1, 1])


def _whitened(H, pts, f0, f1):
    """H (.., 9) broadcast against the points (n) -> (y0, y1, the pieces the derivative needs)."""
    a0, a1, b0, b1 = pts
    m = [H[..., 3 * i] * b0 + H[..., 3 * i + 1] * b1 + H[..., 3 * i + 2] for i in range(3)]
    C0, C1 = m[0] - a0 * m[2], m[1] - a1 * m[2]
    J = (-m[2] / f0[0], (H[..., 0] - a0 * H[..., 6]) / f1[0], (H[..., 1] - a0 * H[..., 7]) / f1[1], -m[2] / f0[1],
         (H[..., 3] - a1 * H[..., 6]) / f1[0], (H[..., 4] - a1 * H[..., 7]) / f1[1])
    return C0, C1, J


def stock_residual(H, pts, f0, f1, dirs=None):
    """e^2 (n) and, with dirs (NP, 9), the full derivative of y along them: (y (n, 2), Jy (n, 2, NP))."""
    C0, C1, J = _whitened(H, pts, f0, f1)
    A, Bq, Cq = J[0] * J[0] + J[1] * J[1] + J[2] * J[2], J[1] * J[4] + J[2] * J[5], J[3] * J[3] + J[4] * J[4] + J[5] * J[5]
    l00 = A.sqrt()
    l10 = Bq / l00
    l11 = (Cq - l10 * l10).sqrt()
    y0 = C0 / l00
    y1 = (C1 - l10 * y0) / l11
    e2 = y0 * y0 + y1 * y1
    if dirs is None:
        return e2
    n = len(y0)
    d = dirs[:, None, :].expand(-1, n, -1)                          # (NP, n, 9)
    dC0, dC1, dJ = _whitened(d, pts, f0, f1)
    dA = 2.0 * (J[0] * dJ[0] + J[1] * dJ[1] + J[2] * dJ[2])
    dBq = dJ[1] * J[4] + J[1] * dJ[4] + dJ[2] * J[5] + J[2] * dJ[5]
    dCq = 2.0 * (J[3] * dJ[3] + J[4] * dJ[4] + J[5] * dJ[5])
    dl00 = dA / (2.0 * l00)
    dl10 = (dBq - l10 * dl00) / l00
    dl11 = (dCq - 2.0 * l10 * dl10) / (2.0 * l11)
    dy0 = (dC0 - y0 * dl00) / l00
    dy1 = (dC1 - dl10 * y0 - l10 * dy0 - y1 * dl11) / l11
    return e2, torch.stack((y0, y1), -1), torch.stack((dy0.T, dy1.T), 1)


def _skew_rows(R):
    """(3, 9): [e_k]x R."""
    eye = torch.eye(3, dtype=R.dtype, device=R.device)
    return torch.stack([torch.linalg.cross(eye[k].expand(3, 3), R.T, dim=1).T.reshape(9) for k in range(3)])


def stock_refine(rows, k0, k1, H0, mode, iters=ITERS, scale=SCALE):
    """cpn_refine_homography's rule from stock operators for one pair -> the refined H (9)."""
    pts = _points(rows, k0, k1)
    f0, f1 = torch.stack((k0[0, 0], k0[1, 1])), torch.stack((k1[0, 0], k1[1, 1]))
    if mode == 0:
        H = H0 / H0.norm()
        H = torch.where(torch.linalg.det(H.reshape(3, 3)) < 0, -H, H)
        dirs = torch.eye(9, dtype=H.dtype, device=H.device)
    else:
        U, _, Vh = torch.linalg.svd(H0.reshape(3, 3))
        H = (U @ Vh).reshape(9)
    for _ in range(iters):
        if mode == 1:
            dirs = _skew_rows(H.reshape(3, 3))
        e2, y, Jy = stock_residual(H, pts, f0, f1, dirs)
        ok = torch.isfinite(e2)
        u = 1.0 + e2 / (scale * scale)
        w = torch.where(ok, 1.0 / (u * u), torch.zeros_like(u))
        Jy, y = torch.where(ok[:, None, None], Jy, torch.zeros_like(Jy)), torch.where(ok[:, None], y, torch.zeros_like(y))
        A = torch.einsum("n,nck,ncl->kl", w, Jy, Jy)
        g = torch.einsum("n,nck,nc->k", w, Jy, y)
        trace = A.diagonal().sum()
        A = A + 1e-3 * torch.diag(A.diagonal())
        if mode == 0:
            A = A + (trace / 9.0) * torch.outer(H, H)
        delta = -torch.linalg.solve(A, g)
        if mode == 0:
            H = (H + delta) / (H + delta).norm()
        else:
            K = torch.zeros(3, 3, dtype=H.dtype, device=H.device)
            K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -delta[2], delta[1], delta[2], -delta[0], -delta[1], delta[0]
            H = (torch.linalg.matrix_exp(K) @ H.reshape(3, 3)).reshape(9)
    return H


def stock_gric(rows, k0, k1, pose_e, Hp, Hr, sigma=SIGMA):
    """cpn_model_gric's rule from stock operators for one pair, all three models in -> (gric (3), the pick)."""
    pts = _points(rows, k0, k1)
    a0, a1, b0, b1 = pts
    f0, f1 = torch.stack((k0[0, 0], k0[1, 1])), torch.stack((k1[0, 0], k1[1, 1]))
    R, t = pose_e[:3, :3].double(), pose_e[:3, 3].double()
    Em = torch.linalg.cross(t.expand(3, 3), R.T, dim=1).T
    a, b = torch.stack((a0, a1, torch.ones_like(a0)), -1), torch.stack((b0, b1, torch.ones_like(b0)), -1)
    Eb, Ea = b @ Em.T, a @ Em
    num = (a * Eb).sum(-1)
    g = torch.cat((Eb[:, :2] / f0, Ea[:, :2] / f1), -1)
    e2 = [num * num / (g * g).sum(-1), stock_residual(Hp, pts, f0, f1), stock_residual(Hr, pts, f0, f1)]
    n = len(a0)
    out = []
    for m, (d, k) in enumerate(((3.0, 5.0), (2.0, 8.0), (2.0, 3.0))):
        cap = 2.0 * (4.0 - d)
        x = e2[m] / (sigma * sigma)
        rho = torch.where(torch.isfinite(x) & (x < cap), x, torch.full_like(x, cap))
        out.append(rho.sum() + math.log(4.0) * d * n + math.log(4.0 * n) * k)
    gric = torch.stack(out)
    order = torch.tensor([2, 1, 0], device=gric.device)
    return gric, order[gric[order].argmin()]                       # the first smallest in (rotation, plane, E) order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "model_select_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = curved_pairs(dev)
    sel = dict(max_cycle_px=1e9)
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "side": S, "hypotheses": HN, "inlier_px": PX, "seed": SEED,
           "sigma_px": SIGMA, "passes": ITERS, "scale_px": SCALE, "rounds": args.rounds, "iters": args.iters,
           "ms": "HIP events per call, windows of `iters` back-to-back calls"}
    m = mt.select(mt.match_fields((f0, f1), intr, pose, S), **sel)
    counts = [int(c) for c in m.count.cpu()]
    N = int(m.xy.shape[1])
    res["matches_per_pair"], res["rows_per_pair_N"] = counts, N

    found = mt.ransac_pose(m, intr, pose, HN, PX, SEED)
    refined = mt.refine_pose(m, intr, found["pose"], ITERS, SCALE)
    homog = mt.homography_pose(m, intr, pose, HN, PX, SEED)
    flat = mt.refine_homography(m, intr, homog["H"], "plane", ITERS, SCALE)
    turn = mt.refine_homography(m, intr, homog["H"], "rotation", ITERS, SCALE)
    ones = torch.ones(B, 3, dtype=torch.uint8, device=dev)
    opts = {"hypotheses": HN, "inlier_px": PX, "seed": SEED, "sigma_px": SIGMA, "iters": ITERS, "scale_px": SCALE}
    kernels = {"refine_pose_ms": lambda: mt.refine_pose(m, intr, found["pose"], ITERS, SCALE),
               "refine_homography_plane_ms": lambda: mt.refine_homography(m, intr, homog["H"], "plane", ITERS, SCALE),
               "refine_homography_rotation_ms": lambda: mt.refine_homography(m, intr, homog["H"], "rotation", ITERS, SCALE),
               "refine_homography_plane_one_pass_ms": lambda: mt.refine_homography(m, intr, homog["H"], "plane", 1, SCALE),
               "model_gric_ms": lambda: mt.model_gric(m, intr, refined["pose"], flat["H"], turn["H"], ones, SIGMA)}
    res["kernels"] = {k: windows(fn, args.rounds, args.iters) for k, fn in kernels.items()}
    res["plane_over_refine_pose"] = round(res["kernels"]["refine_homography_plane_ms"]["median"] / res["kernels"]["refine_pose_ms"]["median"], 3)

    def contained():
        p = mt.ransac_pose(m, intr, pose, HN, PX, SEED)
        mt.refine_pose(m, intr, p["pose"], ITERS, SCALE)
        mt.homography_pose(m, intr, pose, HN, PX, SEED)

    def stock():
        out = []
        for b, n in enumerate(counts):
            rows, k0, k1 = m.xy[b, :n].double(), intr[b, 0].double(), intr[b, 1].double()
            Hp, Hr = stock_refine(rows, k0, k1, homog["H"][b], 0), stock_refine(rows, k0, k1, homog["H"][b], 1)
            out.append(stock_gric(rows, k0, k1, refined["pose"][b], Hp, Hr))
        return out
    forms = {"select_pose_ms": lambda: mt.select_pose(m, intr, pose, **opts),
             "ransac_refine_homography_contained_ms": contained,
             "from_flows_ms": lambda: mt.from_flows((f0, f1), intr, pose, S, **sel),
             "from_flows_with_select_ms": lambda: mt.from_flows((f0, f1), intr, pose, S, select=dict(opts, start="selected"), **sel),
             "stock_refinements_and_gric_ms": stock}
    res["calls"] = {k: windows(fn, args.rounds, args.iters if "stock" not in k else max(args.iters // 4, 2)) for k, fn in forms.items()}
    res["new_part_of_select_pose_ms"] = round(res["calls"]["select_pose_ms"]["median"] -
                                              res["calls"]["ransac_refine_homography_contained_ms"]["median"], 4)

    chosen = mt.select_pose(m, intr, pose, **opts)
    st = stock()
    res["result"] = {"model": chosen["model"].cpu().tolist(), "gric": chosen["gric"].cpu().tolist(),
                     "stats": [[float(v) for v in row] for row in chosen["stats"].cpu()], "avail": chosen["avail"].cpu().tolist(),
                     "plane_refine_stats": [[float(v) for v in row] for row in flat["stats"].cpu()],
                     "rotation_refine_stats": [[float(v) for v in row] for row in turn["stats"].cpu()],
                     "stock_gric": [g.cpu().tolist() for g, _ in st], "stock_model": [int(p) for _, p in st]}
    assert res["result"]["stock_model"] == res["result"]["model"], (res["result"]["stock_model"], res["result"]["model"])
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
