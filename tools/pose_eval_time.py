"""What scoring the pose estimators costs (coponerf_amd/matches.py: pose_errors, residual_stats; Evaluator(geometry=...), DESIGN.md
§4.23).  One MI355X, one process, HIP events, the median of `rounds` windows of `iters` back-to-back calls, on the two curved
256 x 256 pairs of tools/ransac_time.py (about 6 000 matches in 131 072-row buffers):

  the two kernels: cpn_pose_errors on a stack of 5 poses per pair; cpn_residual_stats on (ground truth, network) with q = 0.5 and one
  threshold - Evaluator's call - and at P = Q = T = 8; cpn_refine_pose's ten passes beside them, the yardstick of the expectation;
  residual_stats against the same statistics from stock operators in the same process: the residual as float64 tensor expressions,
  a boolean mask, torch.sort / kthvalue per pair and pose - with the host reads that takes, counted;
  Evaluator.add per batch of two 256 x 256 images without geometry, and with {"refine"} (the default), {"ransac"} and {"select"}.

There is no pass / fail time: the numbers are recorded.

    python tools/pose_eval_time.py [--rounds 5] [--iters 20] [--out profiles/r25_pose_eval.json]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PX = 1.0


def stock_stats(xy, counts, intr, poses, q, px, reads):
    """residual_stats' numbers from stock operators, one (pair, pose) after the other -> nested lists of (usable, median, within,
    sigma0, sigma1) tensors on the device.  counts are host ints (the caller's read); reads[0] counts the reads made here: the
    boolean index and the rank that depends on its length."""
    import torch
    out = []
    for b, n in enumerate(counts):
        rows = xy[b, :n].double()
        k0, k1 = intr[b, 0].double(), intr[b, 1].double()
        one = torch.ones_like(rows[:, 0])
        a = torch.stack(((rows[:, 0] - k0[0, 2]) / k0[0, 0], (rows[:, 1] - k0[1, 2]) / k0[1, 1], one), -1)
        bb = torch.stack(((rows[:, 2] - k1[0, 2]) / k1[0, 0], (rows[:, 3] - k1[1, 2]) / k1[1, 1], one), -1)
        f0, f1 = torch.stack((k0[0, 0], k0[1, 1])), torch.stack((k1[0, 0], k1[1, 1]))
        per = []
        for p in range(poses.shape[1]):
            R, t = poses[b, p, :3, :3].double(), poses[b, p, :3, 3].double()
            tx = torch.zeros(3, 3, dtype=torch.float64, device=xy.device)
            tx[0, 1], tx[0, 2], tx[1, 0], tx[1, 2], tx[2, 0], tx[2, 1] = -t[2], t[1], t[2], -t[0], -t[1], t[0]
            Em = tx @ R
            Eb, Ea = bb @ Em.T, a @ Em
            g = torch.cat((Eb[:, :2] / f0, Ea[:, :2] / f1), -1)
            D = (g * g).sum(-1)
            r = ((a * Eb).sum(-1) / D.sqrt()).abs()
            u = r[torch.isfinite(r) & (D > 0)]                      # a host read: the length of the result
            reads[0] += 1
            n_u = int(u.shape[0])
            ranked = torch.sort(u)[0]
            med = torch.stack([ranked[int(qq * (n_u - 1))] for qq in q])
            s0 = 1.4826 * (1.0 + 5.0 / (n_u - 5)) * torch.kthvalue(u, (n_u - 1) // 2 + 1)[0]
            inl = u[u <= 2.5 * s0]                                  # and another
            reads[0] += 1
            s1 = ((inl * inl).sum() / (int(inl.shape[0]) - 5)).sqrt()
            per.append((n_u, med, (u <= px).sum(), s0, s1))
        out.append(per)
    return out


def main():
    import torch
    from ransac_time import B, S, curved_pairs, windows
    from coponerf_amd import _hip, matches as mt
    from coponerf_amd.evaluate import Evaluator
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pose_eval_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = curved_pairs(dev)
    sel = dict(max_cycle_px=1e9)
    m = mt.select(mt.match_fields((f0, f1), intr, pose, S), **sel)
    N, counts = int(m.xy.shape[1]), [int(c) for c in m.count.cpu()]
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "side": S, "rows_per_pair_N": N, "matches_per_pair": counts, "inlier_px": PX,
           "rounds": args.rounds, "iters": args.iters, "ms": "HIP events per call, windows of `iters` back-to-back calls", "kernels": {},
           "stock": {}, "evaluator_add": {}}
    s = _hip.stream_handle()
    refined = mt.refine_pose(m, intr, true)["pose"]
    stack5 = torch.stack((pose, refined, true, refined, pose), dim=1).contiguous()
    two = torch.stack((true, pose), dim=1).contiguous()
    eight = torch.stack([true, pose, refined, true, pose, refined, true, pose], dim=1).contiguous()
    errs = torch.empty(B, 5, 3, dtype=torch.float64, device=dev)

    def stats_call(poses, q, thr):
        P, Q, T = int(poses.shape[1]), len(q), len(thr)
        qa, ta = (ctypes.c_double * Q)(*q), (ctypes.c_double * T)(*thr)
        bufs = [torch.empty(B, P, dtype=torch.int32, device=dev), torch.empty(B, P, Q, dtype=torch.float64, device=dev),
                torch.empty(B, P, T, dtype=torch.int32, device=dev), torch.empty(B, P, 2, dtype=torch.float64, device=dev),
                torch.empty(B, P, dtype=torch.int32, device=dev)]
        return lambda: _hip.call("cpn_residual_stats", m.xy.data_ptr(), m.count.data_ptr(), intr.data_ptr(), poses.data_ptr(), qa, ta, B, N,
                                 P, Q, T, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                 bufs[4].data_ptr(), s), bufs

    kernels = {"pose_errors_5_poses_ms": lambda: _hip.call("cpn_pose_errors", stack5.data_ptr(), true.data_ptr(), B, 5, errs.data_ptr(), s),
               "residual_stats_P2_Q1_T1_ms": stats_call(two, (0.5,), (PX,))[0],
               "residual_stats_P8_Q8_T8_ms": stats_call(eight, tuple(i / 7 for i in range(8)), tuple(0.25 * (i + 1) for i in range(8)))[0],
               "refine_pose_10_passes_ms": lambda: mt.refine_pose(m, intr, pose)}
    for name, fn in kernels.items():
        res["kernels"][name] = windows(fn, args.rounds, args.iters)
    res["kernels"]["residual_stats_over_refine_pose"] = round(res["kernels"]["residual_stats_P2_Q1_T1_ms"]["median"] /
                                                              res["kernels"]["refine_pose_10_passes_ms"]["median"], 3)

    reads = [0]
    ours = mt.residual_stats(m, intr, two, q=(0.5,), thresholds=(PX,))
    stock = stock_stats(m.xy, counts, intr, two, (0.5,), PX, reads)
    res["stock"]["host_reads_per_call"] = reads[0] + 1              # and the counts
    res["stock"]["residual_stats_wrapper_ms"] = windows(lambda: mt.residual_stats(m, intr, two, q=(0.5,), thresholds=(PX,)), args.rounds, args.iters)
    res["stock"]["stock_operators_ms"] = windows(lambda: stock_stats(m.xy, [int(c) for c in m.count.cpu()], intr, two, (0.5,), PX, reads),
                                                 args.rounds, args.iters)
    res["stock"]["stock_over_kernel"] = round(res["stock"]["stock_operators_ms"]["median"] / res["stock"]["residual_stats_wrapper_ms"]["median"], 2)
    res["stock"]["agreement"] = [[{"usable": [int(ours["usable"][b, p]), stock[b][p][0]],
                                   "median_px": [float(ours["quant"][b, p, 0]), float(stock[b][p][1][0])],
                                   "within": [int(ours["within"][b, p, 0]), int(stock[b][p][2])],
                                   "sigma": [[float(v) for v in ours["sigma"][b, p]], [float(stock[b][p][3]), float(stock[b][p][4])]]}
                                  for p in range(2)] for b in range(B)]

    gen = torch.Generator().manual_seed(25)
    rgb, gt = (torch.rand(B, 1, S * S, 3, generator=gen) * 2 - 1).to(dev), (torch.rand(B, 1, S * S, 3, generator=gen) * 2 - 1).to(dev)
    out = {"rgb": rgb, "rel_pose": pose, "gt_rel_pose": true, "flow": (f0, f1)}
    for name, geometry in (("without_geometry", None), ("refine", dict(sel)), ("ransac", dict(sel, ransac={})), ("select", dict(sel, select={}))):
        ev = Evaluator(geometry=geometry, capacity=1 << 12)
        kw = {} if geometry is None else {"intrinsics": intr}
        res["evaluator_add"][name + "_ms"] = windows(lambda: ev.add(out, gt, None, **kw), args.rounds, args.iters)
        assert ev.host_reads == 0
        if geometry is not None:
            table, c = ev.rows(host=True)[:B], {k: i for i, k in enumerate(ev.columns)}
            res["evaluator_add"][name + "_row"] = {k: [float(v) for v in table[:, c[k]]] for k in ev.columns[8:]}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
