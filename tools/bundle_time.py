"""What two-view bundle adjustment costs (coponerf_amd/triangulate.py: bundle_adjust).  One MI355X, one process, HIP
events, the median of `rounds` windows of `iters` back-to-back calls, on the two curved 256 x 256 pairs of tools/ransac_time.py -
about 6 000 matches in 131 072-row buffers at stride 4 - and again at stride 1 (every pixel that stays inside).  The start is
refine_pose's pose (10 passes, scale 2) and the points cpn_triangulate_matches forms under it:

  the kernel: cpn_bundle_adjust at iters = 10 (at ftol = 1e-6 and at the default 1e-12, with the solves each makes) and at
  iters = 0 (the three sweeps that only measure);
  the same rule from stock float64 operators in the same process: batched Jacobians, torch.linalg.inv of the 3 x 3 blocks,
  torch.linalg.solve of the reduced system, torch.matrix_exp for the step - one pair after the other, one host read per solve for
  the accept decision, counted - checked to take the kernel's accept / reject sequence and to end at its cost;
  (ftol = 1e-6 for both: on these exact matches the gains reach round-off after a few steps, and at the default 1e-12 round-off
  decides the last accept / reject of either form - they then differ in that last decision and agree in the cost to 1e-14);
  cpn_refine_pose (10 passes) beside both, and bundle_adjust's time over it per solve, in units of one of its passes.

There is no pass / fail time: the numbers are recorded.

    python tools/bundle_time.py [--rounds 5] [--iters 20] [--out profiles/r27_bundle.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _skew(v):
    import torch
    z = torch.zeros_like(v[..., 0])
    return torch.stack((torch.stack((z, -v[..., 2], v[..., 1]), -1), torch.stack((v[..., 2], z, -v[..., 0]), -1),
                        torch.stack((-v[..., 1], v[..., 0], z), -1)), -2)


def stock_adjust(xy, counts, intr, pose, xyz, flag, iters, scale_px, ftol, reads):
    """bundle_adjust's rule from stock operators, one pair after the other -> per pair (the accept sequence as a string, the last
    cost, the pose (4, 4) float64 on the device).  counts are host ints; reads[0] counts the host reads made here."""
    import torch
    s2, out = scale_px * scale_px, []
    for b, n in enumerate(counts):
        m, K0, K1 = xy[b, :n].double(), intr[b, 0].double(), intr[b, 1].double()
        f0, c0, f1, c1 = torch.stack((K0[0, 0], K0[1, 1])), K0[:2, 2], torch.stack((K1[0, 0], K1[1, 1])), K1[:2, 2]
        R, t = pose[b, :3, :3].double(), pose[b, :3, 3].double()
        len0 = t.norm()
        t = t / len0
        X = xyz[b, :n].double() / len0
        on = (flag[b, :n] == 0) & torch.isfinite(m).all(1) & torch.isfinite(X).all(1) & (X[:, 2] > 0) & (((X - t) @ R)[:, 2] > 0)
        m, X = m[on], X[on]                                             # a host read: the length of the result
        reads[0] += 1

        def cost_of(R, t, X):
            Y = (X - t) @ R
            r = torch.cat((f0 * X[:, :2] / X[:, 2:] + c0 - m[:, :2], f1 * Y[:, :2] / Y[:, 2:] + c1 - m[:, 2:]), 1)
            e2 = (r * r).sum(1)
            u = 1 + e2 / s2
            return r, Y, ((e2 / 2) / u).sum(), 1 / (u * u)

        def proj_jac(f, Y):
            z = torch.zeros_like(Y[:, 0])
            return torch.stack((torch.stack((f[0] / Y[:, 2], z, -f[0] * Y[:, 0] / Y[:, 2] ** 2), -1),
                                torch.stack((z, f[1] / Y[:, 2], -f[1] * Y[:, 1] / Y[:, 2] ** 2), -1)), -2)

        lam, seq, solves = 1e-3, "", 0
        while solves < iters:
            r, Y, kept, w = cost_of(R, t, X)
            M = proj_jac(f1, Y) @ R.T
            Jx = torch.cat((proj_jac(f0, X), M), 1)
            Jp = torch.zeros(len(X), 4, 6, dtype=torch.float64, device=X.device)
            Jp[:, 2:, :3], Jp[:, 2:, 3:] = M @ _skew(X - t), -M
            wJx, wJp = w[:, None, None] * Jx, w[:, None, None] * Jp
            V = wJx.transpose(1, 2) @ Jx
            V = V + lam * torch.diag_embed(torch.diagonal(V, dim1=1, dim2=2))
            W, U = wJp.transpose(1, 2) @ Jx, wJp.transpose(1, 2) @ Jp
            gx, gp = (wJx.transpose(1, 2) @ r[:, :, None])[..., 0], (wJp.transpose(1, 2) @ r[:, :, None])[..., 0]
            Vi = torch.linalg.inv(V)
            T = W @ Vi
            S = (U - T @ W.transpose(1, 2)).sum(0)
            g = (gp - (T @ gx[:, :, None])[..., 0]).sum(0)
            A = S + lam * torch.diag(torch.diagonal(S))
            A[3:, 3:] += torch.trace(S) / 6 * torch.outer(t, t)
            delta = torch.linalg.solve(A, -g)
            solves += 1
            dX = -(Vi @ (gx + (W.transpose(1, 2) @ delta))[:, :, None])[..., 0]
            tn = t + delta[3:]
            ln = tn.norm()
            Rn, tn, Xn = torch.matrix_exp(_skew(delta[:3])) @ R, tn / ln, (X + dX) / ln
            _, Yn, trial, _ = cost_of(Rn, tn, Xn)
            good = bool(((Xn[:, 2] > 0) & (Yn[:, 2] > 0)).all() & (trial < kept))       # a host read: the decision
            reads[0] += 1
            if good:
                seq += "A"
                R, t, X, lam = Rn, tn, Xn, max(lam / 3, 1e-12)
                if float(kept - trial) <= ftol * float(kept):
                    break
            else:
                seq += "R"
                lam = 4 * lam
                if lam > 1e8:
                    break
        P = torch.eye(4, dtype=torch.float64, device=X.device)
        P[:3, :3], P[:3, 3] = R, len0 * t
        out.append((seq, float(cost_of(R, t, X)[2]), P))
    return out


def main():
    import torch
    from ransac_time import B, S, curved_pairs, windows
    from coponerf_amd import _hip, matches as mt, triangulate as tg
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bundle_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = curved_pairs(dev)
    fields = mt.match_fields((f0, f1), intr, pose, S)
    LM, SCALE, FTOL = 10, 2.0, 1e-6
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "side": S, "lm_iters": LM, "scale_px": SCALE, "ftol": FTOL, "rounds": args.rounds,
           "iters": args.iters, "ms": "HIP events per call, windows of `iters` back-to-back calls", "strides": {}}
    for stride in (4, 1):
        m = mt.select(fields, max_cycle_px=1e9, stride=stride)
        N, counts = int(m.xy.shape[1]), [int(c) for c in m.count.cpu()]
        refined = mt.refine_pose(m, intr, pose, iters=10, scale_px=SCALE)["pose"].contiguous()
        tri = tg.points(m, intr, refined)
        ba = tg.bundle_adjust(tri, m, intr, refined, iters=LM, scale_px=SCALE, ftol=FTOL)
        st = ba["stats"].cpu()
        row = {"rows_per_pair_N": N, "matches_per_pair": counts, "rows_used": [int(v) for v in st[:, 3]],
               "accepted": [int(v) for v in st[:, 4]], "rejected": [int(v) for v in st[:, 5]], "status": [int(v) for v in st[:, 11]],
               "cost": [[float(v) for v in st[:, 0]], [float(v) for v in st[:, 1]]], "sigma": [float(v) for v in st[:, 7]],
               "predicted_deg": [[float(v) for v in st[:, 8]], [float(v) for v in st[:, 9]]], "kernels": {}, "stock": {}}
        solves = [a + r for a, r in zip(row["accepted"], row["rejected"])]
        row["kernels"]["bundle_adjust_ms"] = windows(lambda: tg.bundle_adjust(tri, m, intr, refined, iters=LM, scale_px=SCALE, ftol=FTOL),
                                                     args.rounds, args.iters)
        loose = tg.bundle_adjust(tri, m, intr, refined, iters=LM, scale_px=SCALE)["stats"].cpu()
        row["kernels"]["default_ftol_solves"] = [int(a + r) for a, r in zip(loose[:, 4], loose[:, 5])]
        row["kernels"]["bundle_adjust_default_ftol_ms"] = windows(lambda: tg.bundle_adjust(tri, m, intr, refined, iters=LM, scale_px=SCALE),
                                                                  args.rounds, args.iters)
        row["kernels"]["bundle_adjust_measure_only_ms"] = windows(lambda: tg.bundle_adjust(tri, m, intr, refined, iters=0, scale_px=SCALE),
                                                                  args.rounds, args.iters)
        row["kernels"]["refine_pose_10_ms"] = windows(lambda: mt.refine_pose(m, intr, pose, iters=10, scale_px=SCALE), args.rounds, args.iters)
        row["kernels"]["triangulate_matches_ms"] = windows(lambda: tg.points(m, intr, refined), args.rounds, args.iters)
        one_pass = row["kernels"]["refine_pose_10_ms"]["median"] / 11.0            # ten passes and the one that measures
        per_solve = (row["kernels"]["bundle_adjust_ms"]["median"] - row["kernels"]["bundle_adjust_measure_only_ms"]["median"]) / max(max(solves), 1)
        row["kernels"]["solves"] = solves
        row["kernels"]["refine_pose_passes_per_solve"] = round(per_solve / one_pass, 2)
        few = max(2, args.iters // 10)
        reads = [0]
        theirs = stock_adjust(m.xy, counts, intr, refined, tri["xyz"], tri["flag"], LM, SCALE, FTOL, reads)
        row["stock"]["host_reads_per_call"] = reads[0] + 1              # and the counts
        row["stock"]["calls_per_window"] = few
        row["stock"]["stock_operators_ms"] = windows(lambda: stock_adjust(m.xy, [int(c) for c in m.count.cpu()], intr, refined, tri["xyz"],
                                                                          tri["flag"], LM, SCALE, FTOL, reads), args.rounds, few)
        row["stock"]["stock_over_kernel"] = round(row["stock"]["stock_operators_ms"]["median"] / row["kernels"]["bundle_adjust_ms"]["median"], 2)
        errs = mt.pose_errors(torch.stack((refined, ba["pose"], torch.stack([p for _, _, p in theirs]).float()), 1).contiguous(), true).cpu()
        row["stock"]["agreement"] = {"sequence": [s for s, _, _ in theirs],
                                     "same_counts": [s.count("A") == a and s.count("R") == r for (s, _, _), a, r in zip(theirs, row["accepted"], row["rejected"])],
                                     "cost": [[float(v) for v in st[:, 1]], [c for _, c, _ in theirs]]}
        row["errors_rot_rad_trans_angle_rad"] = {"refined": errs[:, 0].tolist(), "adjusted": errs[:, 1].tolist(), "stock": errs[:, 2].tolist()}
        res["strides"][f"stride_{stride}"] = row
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
