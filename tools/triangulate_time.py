"""What turning the matches into geometry costs (coponerf_amd/triangulate.py: points, depth_scale, from_pair).  One
MI355X, one process, HIP events, the median of `rounds` windows of `iters` back-to-back calls, on the two curved 256 x 256 pairs of
tools/ransac_time.py - about 6 000 matches in 131 072-row buffers at stride 4 - and again at stride 1 (every pixel that stays inside):

  the two kernels: cpn_triangulate_matches under the true pose, without and with the colours of two photos, and cpn_depth_scale
  against a depth map that holds the true depth at the nearest pixel of every match (so its scale must come out as |t|: recorded);
  the same rule from stock operators in the same process: the correction, the point and the ratios as batched float64 tensor
  expressions, the keep mask, torch.median per pair - with the host reads that takes, counted;
  triangulate.from_pair(pose="network", scale="depth") on the synthetic-weight model against the matches.from_pair and the one
  render_path it contains (fewer calls per window: these take tens of milliseconds).

There is no pass / fail time: the numbers are recorded.

    python tools/triangulate_time.py [--rounds 5] [--iters 20] [--out profiles/r26_triangulate.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PASSES = 3


def stock_scale(xy, counts, intr, pose, depth, S, reads):
    """depth_scale(points(..)) from stock operators: float64 tensor expressions over the whole buffers, then per pair a boolean
    index and torch.median -> (scale (B) on the device, rows used).  counts are host ints (the caller's read); reads[0] counts the
    reads made here."""
    import torch
    B, N = xy.shape[:2]
    m = xy.double()
    K0, K1 = intr[:, 0].double(), intr[:, 1].double()
    f0, c0 = torch.stack((K0[:, 0, 0], K0[:, 1, 1]), -1)[:, None], torch.stack((K0[:, 0, 2], K0[:, 1, 2]), -1)[:, None]
    f1, c1 = torch.stack((K1[:, 0, 0], K1[:, 1, 1]), -1)[:, None], torch.stack((K1[:, 0, 2], K1[:, 1, 2]), -1)[:, None]
    R, t = pose[:, :3, :3].double(), pose[:, :3, 3].double()
    th = t / t.norm(dim=1, keepdim=True)
    tx = torch.zeros(B, 3, 3, dtype=torch.float64, device=xy.device)
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -th[:, 2], th[:, 1], th[:, 2], -th[:, 0], -th[:, 1], th[:, 0]
    Em = tx @ R
    one = torch.ones_like(m[..., :1])
    a, b = torch.cat(((m[..., :2] - c0) / f0, one), -1), torch.cat(((m[..., 2:] - c1) / f1, one), -1)
    Eb, Ea = b @ Em.transpose(1, 2), a @ Em
    c = (a * Eb).sum(-1)
    p, q = Eb[..., :2] / f0, Ea[..., :2] / f1
    Ft = Em[:, :2, :2] / f0.transpose(1, 2) / f1
    n, n2 = p, q
    for _ in range(PASSES):
        A = (n * (n2 @ Ft.transpose(1, 2))).sum(-1)
        Bq = 0.5 * ((n * p).sum(-1) + (n2 * q).sum(-1))
        lam = c / (Bq + (Bq * Bq - A * c).sqrt())
        D, G = lam[..., None] * n, lam[..., None] * n2
        n, n2 = p - G @ Ft.transpose(1, 2), q - D @ Ft
    ah = torch.cat(((m[..., :2] - D - c0) / f0, one), -1)
    bh = torch.cat(((m[..., 2:] - G - c1) / f1, one), -1)
    cr = bh @ R.transpose(1, 2)
    w = torch.linalg.cross(ah, cr)
    ww = (w * w).sum(-1)
    tt = t[:, None].expand_as(cr)
    z0 = (torch.linalg.cross(tt, cr) * w).sum(-1) / ww
    z1 = (torch.linalg.cross(tt, ah) * w).sum(-1) / ww
    err = ((D * D).sum(-1) + (G * G).sum(-1)).sqrt()
    par = torch.rad2deg(torch.atan2(ww.sqrt(), (ah * cr).sum(-1)))
    u, v = (m[..., 0] + 0.5).floor(), (m[..., 1] + 0.5).floor()
    inside = (u >= 0) & (u <= S - 1) & (v >= 0) & (v <= S - 1)
    d = torch.gather(depth, 1, torch.where(inside, v * S + u, torch.zeros_like(u)).long()).double()
    keep = inside & (z0 > 0) & (z1 > 0) & (err <= 1.0) & (par >= 1.0) & (d > 0) & (d < 10)
    ratio = d / z0
    scales, used = [], []
    for b_, n_ in enumerate(counts):
        r = ratio[b_, :n_][keep[b_, :n_]]                           # a host read: the length of the result
        reads[0] += 1
        used.append(int(r.shape[0]))
        scales.append(torch.median(r))
    return torch.stack(scales), used


def main():
    import torch
    from ransac_time import B, S, curved_pairs, windows
    from coponerf_amd import CoPoNeRF, _hip, matches as mt, synthetic as syn, triangulate as tg
    from coponerf_amd.novel_views import prepare_pair, render_path
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "triangulate_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = curved_pairs(dev)
    fields = mt.match_fields((f0, f1), intr, pose, S)
    res = {"device": torch.cuda.get_device_name(0), "pairs": B, "side": S, "passes": PASSES, "rounds": args.rounds, "iters": args.iters,
           "ms": "HIP events per call, windows of `iters` back-to-back calls", "strides": {}, "from_pair": {}}
    s = _hip.stream_handle()
    gen = torch.Generator().manual_seed(26)
    images = (torch.rand(B, 2, S, S, 3, generator=gen) * 2 - 1).to(dev)
    unit = tg.rescale(true, torch.ones(B, dtype=torch.float64, device=dev))
    for stride in (4, 1):
        m = mt.select(fields, max_cycle_px=1e9, stride=stride)
        N, counts = int(m.xy.shape[1]), [int(c) for c in m.count.cpu()]
        # the true depth at the nearest pixel of every match, 0 (not valid) elsewhere
        exact = tg.points(m, intr, true)
        u, v = (m.xy[..., 0].double() + 0.5).floor().long().clamp(0, S - 1), (m.xy[..., 1].double() + 0.5).floor().long().clamp(0, S - 1)
        depth = torch.zeros(B, S * S, device=dev)
        for b in range(B):
            on = exact["flag"][b, :counts[b]] == 0
            depth[b].index_put_(((v[b, :counts[b]] * S + u[b, :counts[b]])[on],), exact["geom"][b, :counts[b], 0][on])
        tri = tg.points(m, intr, unit)
        out = {k: torch.empty_like(x) for k, x in tri.items()}
        rgb = torch.empty(B, N, 3, device=dev)
        scale, stats = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, 4, dtype=torch.float64, device=dev)
        tri_call = lambda im, col: _hip.call("cpn_triangulate_matches", m.xy.data_ptr(), m.count.data_ptr(), intr.data_ptr(), unit.data_ptr(),
                                             im, B, N, S if im else 0, out["xyz"].data_ptr(), out["geom"].data_ptr(), out["flag"].data_ptr(),
                                             col, s)
        row = {"rows_per_pair_N": N, "matches_per_pair": counts, "kernels": {}, "stock": {}}
        row["kernels"]["triangulate_matches_ms"] = windows(lambda: tri_call(None, None), args.rounds, args.iters)
        row["kernels"]["triangulate_matches_with_colours_ms"] = windows(lambda: tri_call(images.data_ptr(), rgb.data_ptr()), args.rounds, args.iters)
        row["kernels"]["depth_scale_ms"] = windows(lambda: _hip.call("cpn_depth_scale", tri["geom"].data_ptr(), tri["flag"].data_ptr(),
                                                                     m.xy.data_ptr(), m.count.data_ptr(), depth.data_ptr(), true.data_ptr(), B, N,
                                                                     S, 1.0, 1.0, 8, scale.data_ptr(), stats.data_ptr(), s), args.rounds, args.iters)
        row["kernels"]["cloud_ms"] = windows(lambda: tg.cloud(tri), args.rounds, args.iters)
        both = lambda: tg.depth_scale(tg.points(m, intr, unit), m, depth, S, rel_pose=true)
        reads = [0]
        ours = both()
        theirs, used = stock_scale(m.xy, counts, intr, unit, depth, S, reads)
        row["stock"]["host_reads_per_call"] = reads[0] + 1          # and the counts
        row["stock"]["points_and_depth_scale_ms"] = windows(both, args.rounds, args.iters)
        row["stock"]["stock_operators_ms"] = windows(lambda: stock_scale(m.xy, [int(c) for c in m.count.cpu()], intr, unit, depth, S, reads),
                                                     args.rounds, args.iters)
        row["stock"]["stock_over_kernels"] = round(row["stock"]["stock_operators_ms"]["median"] / row["stock"]["points_and_depth_scale_ms"]["median"], 2)
        row["stock"]["agreement"] = {"scale": [[float(v) for v in ours["scale"]], [float(v) for v in theirs]],
                                     "rows_used": [[int(v) for v in ours["stats"][:, 0]], used],
                                     "true_length": [float(v) for v in true[:, :3, 3].double().norm(dim=1)],
                                     "spread": [float(v) for v in ours["stats"][:, 1]], "network_over_scale": [float(v) for v in ours["stats"][:, 2]]}
        res["strides"][f"stride_{stride}"] = row

    model = CoPoNeRF.CoPoNeRF(n_view=2)
    model.load_state_dict(syn.make_full_weights({k: tuple(v.shape) for k, v in model.state_dict().items()}), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    few = max(2, args.iters // 10)
    kw = dict(max_cycle_px=1e9)
    res["from_pair"]["calls_per_window"] = few
    res["from_pair"]["triangulate_from_pair_depth_ms"] = windows(lambda: tg.from_pair(model, inp, pose="network", scale="depth", **kw), args.rounds, few)
    res["from_pair"]["triangulate_from_pair_given_ms"] = windows(lambda: tg.from_pair(model, inp, pose="network", scale="given", **kw), args.rounds, few)
    res["from_pair"]["matches_from_pair_ms"] = windows(lambda: mt.from_pair(model, inp, refine=False, **kw), args.rounds, few)
    res["from_pair"]["render_path_view0_depth_ms"] = windows(lambda: render_path(model, inp, (0.0,), return_depth=True), args.rounds, few)
    last = tg.from_pair(model, inp, pose="network", scale="depth", **kw)
    res["from_pair"]["synthetic_weights"] = {"matches": int(last["matches"]["matches"].count[0]), "depth_scale_stats": [float(v) for v in last["stats"][0]],
                                             "cloud": int(last["cloud"].count[0]),
                                             "note": "the synthetic flows carry no geometry: this shows that the path runs, nothing more"}
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
