"""What LO-MSAC costs and what it buys (coponerf_amd/matches.py: ransac_pose(score="msac", lo=K)).  Two halves that
write into one file, each keeping the other's section:

  --accuracy   on the CPU, no device: the accuracy table of the numpy restatement (tests/lo_msac_ref.py: accuracy_rows) - the
               curved scene, the wall and the 5 %-off wall, both solvers, 16 / 64 / 256 / 1024 hypotheses, seeds 0 - 2, the four
               settings (inliers | msac) x (lo 0 | 8), pose errors to the truth in degrees of ransac_pose's pose and of
               refine_pose from it - and its summary per cell (the median over the seeds).
  (default)    on one MI355X, in one process, HIP events, the median of `rounds` windows of `iters` back-to-back calls, on the two
               curved 256 x 256 pairs of tools/ransac_time.py (about 6 000 matches in 131 072-row buffers), at 1024 and at 256
               hypotheses, for both solvers: each kernel alone (cpn_ransac_score against cpn_ransac_score_slots counting and
               graded on the same slots, cpn_ransac_polish at K = 8 and 4 passes, the K-slot score, both finishes);
               ransac_pose in the four settings; from_flows with and without; and what came out.

There is no pass / fail time: the numbers are recorded.

    python tools/lo_msac_time.py [--accuracy] [--rounds 5] [--iters 20] [--out profiles/r24_lo_msac.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K_LO, LO_ITERS, PX, SEED = 8, 4, 1.0, 0
SETTINGS = (("inliers", 0), ("msac", 0), ("inliers", K_LO), ("msac", K_LO))


def accuracy():
    from tests import lo_msac_ref as lm
    rows = lm.accuracy_rows()
    cells = {}
    for r in rows:
        cells.setdefault((r["scene"], r["solver"], r["hypotheses"], r["score"], r["lo"]), []).append(r)
    summary = []
    for (scene, solver, Hn, kind, lo), rs in cells.items():
        med = lambda f: round(statistics.median(r[f] for r in rs), 4)
        summary.append({"scene": scene, "solver": solver, "hypotheses": Hn, "score": kind, "lo": lo, "seeds": len(rs),
                        "median_deg_R": med("deg_R"), "median_deg_t": med("deg_t"), "median_refined_deg_R": med("refined_deg_R"),
                        "median_refined_deg_t": med("refined_deg_t"), "worst_deg": round(max(max(r["deg_R"], r["deg_t"]) for r in rs), 4),
                        "worst_refined_deg": round(max(max(r["refined_deg_R"], r["refined_deg_t"]) for r in rs), 4),
                        "polished_won": sum(r["polished_won"] for r in rs)})
    return {"what": "tests/lo_msac_ref.py on the CPU: 1000 matches, 0.5 px noise, 30 % outliers, inlier_px 1, lo_iters 4, lo_scale_px "
                    "None; refined = refine_pose's restatement (10 passes, 2 px) from the winner; degrees to the truth",
            "rows": rows, "summary_median_over_seeds": summary}


def timing(args):
    import torch
    from ransac_time import B, S, curved_pairs, windows
    from matches_time import angle_deg, dir_deg
    from coponerf_amd import _hip, matches as mt
    assert torch.cuda.is_available(), "lo_msac_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = curved_pairs(dev)
    sel = dict(max_cycle_px=1e9)
    m = mt.select(mt.match_fields((f0, f1), intr, pose, S), **sel)
    N = int(m.xy.shape[1])
    chunks = -(-N // _hip.CONSTANTS["RANSAC_CHUNK"])
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "side": S, "rows_per_pair_N": N, "matches_per_pair": [int(c) for c in m.count.cpu()],
           "inlier_px": PX, "seed": SEED, "lo": K_LO, "lo_iters": LO_ITERS, "rounds": args.rounds, "iters": args.iters,
           "ms": "HIP events per call, windows of `iters` back-to-back calls", "runs": []}
    s = _hip.stream_handle()
    xy, cn, K, P = m.xy.data_ptr(), m.count.data_ptr(), intr.data_ptr(), pose.data_ptr()

    def off(Pm):
        return [[angle_deg(Pm[b, :3, :3], true[b, :3, :3]), dir_deg(Pm[b, :3, 3], true[b, :3, 3])] for b in range(B)]
    for solver, per in (("8pt", 1), ("5pt", 10)):
        for HN in (1024, 256):
            SL, T = per * HN, per * HN + K_LO
            E = torch.empty(B, SL, 9, dtype=torch.float64, device=dev)
            sample = torch.empty(B, HN, 8 if per == 1 else 5, dtype=torch.int32, device=dev)
            valid = torch.empty(B, SL, dtype=torch.uint8, device=dev)
            narrow = torch.empty(B, chunks, SL + 1, dtype=torch.int32, device=dev)
            wide = torch.empty(B, chunks, T + 1, dtype=torch.int32, device=dev)
            E_lo = torch.empty(B, K_LO, 9, dtype=torch.float64, device=dev)
            valid_lo = torch.empty(B, K_LO, dtype=torch.uint8, device=dev)
            info = torch.empty(B, K_LO, 8, dtype=torch.float64, device=dev)
            po, inl = torch.empty(B, 4, 4, device=dev), torch.empty(B, N, dtype=torch.uint8, device=dev)
            st, lo_out = torch.empty(B, 8, dtype=torch.float64, device=dev), torch.empty(B, 4, dtype=torch.float64, device=dev)
            won = torch.empty(B, dtype=torch.int64, device=dev)
            _hip.call("cpn_ransac_hypotheses5" if per == 10 else "cpn_ransac_hypotheses", xy, cn, K, B, N, HN, SEED, E.data_ptr(),
                      sample.data_ptr(), valid.data_ptr(), s)
            slots = lambda graded, buf, total: (lambda: _hip.call("cpn_ransac_score_slots", E.data_ptr(), valid.data_ptr(), xy, cn, K, P, B, N,
                                                                  SL, 0, total, graded, PX, buf.data_ptr(), s))
            kernels = {
                "ransac_score_ms": lambda: _hip.call("cpn_ransac_score", E.data_ptr(), valid.data_ptr(), xy, cn, K, P, B, N, SL, PX,
                                                     narrow.data_ptr(), s),
                "ransac_score_slots_counting_ms": slots(0, narrow, SL),
                "ransac_score_slots_graded_ms": slots(1, narrow, SL),
                "ransac_score_slots_graded_wide_rows_ms": slots(1, wide, T),
                "ransac_polish_ms": lambda: _hip.call("cpn_ransac_polish", E.data_ptr(), valid.data_ptr(), wide.data_ptr(), xy, cn, K, B, N,
                                                      SL, K_LO, LO_ITERS, PX, PX, E_lo.data_ptr(), valid_lo.data_ptr(), info.data_ptr(), s),
                "ransac_polish_no_pass_ms": lambda: _hip.call("cpn_ransac_polish", E.data_ptr(), valid.data_ptr(), wide.data_ptr(), xy, cn, K,
                                                              B, N, SL, K_LO, 0, PX, PX, E_lo.data_ptr(), valid_lo.data_ptr(),
                                                              info.data_ptr(), s),
                "ransac_score_slots_polished_only_ms": lambda: _hip.call("cpn_ransac_score_slots", E_lo.data_ptr(), valid_lo.data_ptr(), xy,
                                                                         cn, K, P, B, N, K_LO, SL, T, 1, PX, wide.data_ptr(), s),
                "ransac_finish_ms": lambda: _hip.call("cpn_ransac_finish", E.data_ptr(), valid.data_ptr(), narrow.data_ptr(), xy, cn, K, P, B,
                                                      N, SL, PX, po.data_ptr(), inl.data_ptr(), st.data_ptr(), s),
                "ransac_finish_lo_ms": lambda: _hip.call("cpn_ransac_finish_lo", E.data_ptr(), valid.data_ptr(), E_lo.data_ptr(),
                                                         valid_lo.data_ptr(), info.data_ptr(), wide.data_ptr(), xy, cn, K, P, B, N, SL, K_LO, 1,
                                                         PX, po.data_ptr(), inl.data_ptr(), st.data_ptr(), won.data_ptr(), lo_out.data_ptr(), s)}
            run = {"solver": solver, "hypotheses": HN, "slots": SL, "kernels": {}, "calls": {}, "result": {}}
            for name, fn in kernels.items():                        # in the loop's own order: each finds its inputs written
                run["kernels"][name] = windows(fn, args.rounds, args.iters)
            run["graded_over_counting_score"] = round(run["kernels"]["ransac_score_slots_graded_ms"]["median"] /
                                                      run["kernels"]["ransac_score_ms"]["median"], 3)
            run["kernels"]["refine_pose_10_passes_ms"] = windows(lambda: mt.refine_pose(m, intr, pose), args.rounds, args.iters)
            for kind, lo in SETTINGS:
                kw = dict(hypotheses=HN, inlier_px=PX, seed=SEED, solver=solver, score=kind, lo=lo, lo_iters=LO_ITERS)
                tag = f"{kind}_lo{lo}"
                run["calls"][f"ransac_pose_{tag}_ms"] = windows(lambda: mt.ransac_pose(m, intr, pose, **kw), args.rounds, args.iters)
                opts = dict(kw, start="ransac")
                run["calls"][f"from_flows_{tag}_ms"] = windows(lambda: mt.from_flows((f0, f1), intr, pose, S, ransac=opts, **sel),
                                                               args.rounds, args.iters)
                got = mt.ransac_pose(m, intr, pose, **kw)
                ours = mt.from_flows((f0, f1), intr, pose, S, ransac=opts, **sel)
                run["result"][tag] = {"stats": [[float(v) for v in row] for row in got["stats"].cpu()],
                                      "score": [int(v) for v in got["score"].cpu()] if "score" in got else None,
                                      "lo": [[float(v) for v in row] for row in got["lo"].cpu()] if "lo" in got else None,
                                      "degrees_from_truth": off(got["pose"]), "refined_degrees_from_truth": off(ours["pose"])}
            run["calls"]["from_flows_without_ransac_ms"] = windows(lambda: mt.from_flows((f0, f1), intr, pose, S, **sel), args.rounds,
                                                                   args.iters)
            res["runs"].append(run)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true", help="the CPU half: the accuracy table of the restatement")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    whole = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            whole = json.load(f)
    key = "accuracy" if args.accuracy else "timing"
    whole[key] = accuracy() if args.accuracy else timing(args)
    print(json.dumps(whole[key] if not args.accuracy else whole[key]["summary_median_over_seeds"], indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(whole, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
