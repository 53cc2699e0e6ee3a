"""What the matches of two photos cost (coponerf_amd/matches.py), on one MI355X, in one process.

  (a) the kernels of csrc/matches.hip on two 256 x 256 pairs with 64 x 64 flows - cpn_match_fields, cpn_compact_matches on the
      default selection, cpn_refine_pose with 10 iterations - by HIP events, and match_fields / select / refine_pose /
      from_flows (the kernels, the mask between them and their allocations; no host read) by wall clock around a synchronise.
      The flows are those of a tilted plane seen by two cameras (ray-cast here in float64, sampled at the flow cells' centres),
      so that the matches carry a geometry; rel_pose is the true pose turned by 2 degrees and its translation by 5.
  (b) the same results composed from stock operators: cycle_masks' chain (F.interpolate, utils.warp's grid_sample, torch.norm)
      with the residual in float64 torch, boolean indexing per pair - which reads the host -, and the same Gauss-Newton per
      pair with torch.linalg.cholesky_ex / cholesky_solve on the device.  Timed by wall clock like (a), alternating with it.
      The differences of the two results are recorded.
  (c) the operator calls and the host reads of both: every ATen operator that is not a view counts (each is at least one
      launch), every entry point of the library with its known number of launches; the reads are what torch's synchronisation
      debug mode reports (its own notice that the mode is a prototype is left out).
  (d) from_pair of a prepare_pair dict on the synthetic weights against the get_z it contains, alternating, wall clock.  The
      synthetic flows carry no geometry: this shows that the path runs and what it costs, nothing about the pose.

There is no pass / fail time: the numbers are recorded, and (a) is compared with (b) from the same run only.

    python tools/matches_time.py [--rounds 6] [--iters 50] [--out profiles/r16_matches.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
import warnings

import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import CoPoNeRF, _hip, matches as mt, novel_views as nv, synthetic as syn   # noqa: E402
from coponerf_amd.aux_outputs import _grid, _inside, _warp                                   # noqa: E402

S, HF, B = 256, 64, 2
ITERS, SCALE = 10, 2.0
LAUNCHES = {"cpn_match_fields": 1, "cpn_compact_matches": 2, "cpn_refine_pose": 1}
VIEWS = {"view", "_unsafe_view", "reshape", "expand", "select", "slice", "transpose", "permute", "unsqueeze", "squeeze", "alias",
         "detach", "as_strided", "t", "unbind", "split", "_reshape_alias", "expand_as", "view_as", "numpy_T", "diagonal", "unfold",
         "lift_fresh", "is_same_size", "sym_size", "sym_stride", "sym_numel", "stride", "size", "dim", "is_pinned"}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, iters):
    """Median ms of fn() between two HIP events."""
    fn()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


class Ops(TorchDispatchMode):
    """Counts the ATen operators that are not views."""

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.overloadpacket.__name__ not in VIEWS:
            self.n += 1
        return func(*args, **(kwargs or {}))


def census(fn, operators=True):
    """(ATen operators that are not views, launches of this module's entry points, host reads) of one fn()."""
    calls = []
    real = _hip.call

    def counted(name, *a):
        calls.append(name)
        return real(name, *a)
    _hip.call = counted
    torch.cuda.synchronize()
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                if operators:
                    with Ops() as ops:
                        fn()
                else:
                    ops = None
                    fn()
            finally:
                torch.cuda.set_sync_debug_mode("default")
    finally:
        _hip.call = real
    torch.cuda.synchronize()
    return {"aten_operators": ops.n if ops else None, "library_launches": sum(LAUNCHES.get(c, 0) for c in calls),
            "other_library_calls": len([c for c in calls if c not in LAUNCHES]), 
            "host_reads": len([c for c in caught if "synchroniz" in str(c.message) and "prototype" not in str(c.message)])}


# ------------------------------------------------------------------------------------------------------------- the scene
def rodrigues(axis, deg):
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    Kx = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    th = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def plane_pairs(dev):
    """(flow0, flow1 (B, 2, 64, 64), intrinsics (B, 2, 4, 4), rel_pose (B, 4, 4) the start, true (B, 4, 4)) fp32 on the device."""
    s = S / HF
    c = (torch.arange(HF, dtype=torch.float64) + 0.5) * s - 0.5
    y, x = torch.meshgrid(c, c, indexing="ij")
    f0, f1, Ks, P0, Pt = [], [], [], [], []
    for b in range(B):
        f = 210.0 + 15.0 * b
        R, t = rodrigues((0.2, 1.0, 0.1), 7.0 + 2.0 * b), torch.tensor([0.45, 0.04, 0.1 + 0.05 * b], dtype=torch.float64)
        n, cpl = torch.tensor([-0.25, -0.15, 1.0], dtype=torch.float64), 3.5
        ray = torch.stack(((x - S / 2) / f, (y - S / 2) / f, torch.ones_like(x)), -1)
        X0 = ray * (cpl / (ray @ n))[..., None]                    # view 0's pixels on the plane
        X1 = (X0 - t) @ R
        f0.append(torch.stack((f * X1[..., 0] / X1[..., 2] + S / 2 - x, f * X1[..., 1] / X1[..., 2] + S / 2 - y)) / s)
        d1 = (cpl - n @ t) / ((ray @ R.T) @ n)                     # view 1's pixels on the plane: n . (R d r + t) = c
        Y0 = (ray * d1[..., None]) @ R.T + t
        f1.append(torch.stack((f * Y0[..., 0] / Y0[..., 2] + S / 2 - x, f * Y0[..., 1] / Y0[..., 2] + S / 2 - y)) / s)
        K = torch.eye(4, dtype=torch.float64)
        K[0, 0] = K[1, 1] = f
        K[0, 2] = K[1, 2] = S / 2
        Ks.append(torch.stack((K, K)))
        true, start = torch.eye(4, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
        true[:3, :3], true[:3, 3] = R, t
        start[:3, :3], start[:3, 3] = rodrigues((1.0, -0.4, 0.6), 2.0) @ R, rodrigues((0.1, 1.0, 0.3), 5.0) @ t
        Pt.append(true)
        P0.append(start)
    return tuple(torch.stack(v).float().contiguous().to(dev) for v in (f0, f1, Ks, P0, Pt))


# ------------------------------------------------------------------------------------------------------ the stock composition
def stock_fields(f0, f1, intr, pose):
    """match_fields from stock operators: cycle_masks' chain in fp32, the residual in float64."""
    up = [F.interpolate(f, S, mode="bilinear") * (S / HF) for f in (f0, f1)]
    K0, K1 = intr[:, 0, :3, :3].double(), intr[:, 1, :3, :3].double()
    R, t = pose[:, :3, :3].double(), pose[:, :3, 3].double()
    z = torch.zeros_like(t[:, 0])
    tx = torch.stack((z, -t[:, 2], t[:, 1], t[:, 2], z, -t[:, 0], -t[:, 1], t[:, 0], z), -1).view(-1, 3, 3)
    Fm = torch.linalg.inv(K0).transpose(1, 2) @ tx @ R @ torch.linalg.inv(K1)
    out = {"q": [], "cycle": [], "epi": [], "inside": []}
    for d in (0, 1):
        g = _grid(B, S, S, f0.device)
        q = (g + up[d]).permute(0, 2, 3, 1)
        cyc = torch.norm(up[d] + _warp(up[1 - d], up[d]), dim=1)
        ones = torch.ones(B, S, S, 1, dtype=torch.float64, device=f0.device)
        p = torch.cat((g.permute(0, 2, 3, 1).double(), ones), -1).view(B, -1, 3)
        m = torch.cat((q.double(), ones), -1).view(B, -1, 3)
        x0, x1 = (p, m) if d == 0 else (m, p)
        Fx1, Ftx0 = x1 @ Fm.transpose(1, 2), x0 @ Fm
        epi = (x0 * Fx1).sum(-1) / torch.sqrt(Fx1[..., 0] ** 2 + Fx1[..., 1] ** 2 + Ftx0[..., 0] ** 2 + Ftx0[..., 1] ** 2)
        out["q"].append(q)
        out["cycle"].append(cyc)
        out["epi"].append(epi.view(B, S, S).float())
        out["inside"].append(_inside(up[d]))
    return {k: torch.stack(v) for k, v in out.items()}


def stock_select(fields, stride=4):
    """select from stock operators: boolean indexing per pair (the host read) -> lists of (n_b, 4) and (n_b, 2)."""
    on = torch.arange(S, device=fields["q"].device) % stride == stride // 2
    keep = fields["inside"] & (fields["cycle"] <= 10.0) & (on[:, None] & on[None, :])
    g = _grid(1, S, S, keep.device)[0].permute(1, 2, 0)
    xys, errs = [], []
    for b in range(B):
        rows, es = [], []
        for d in (0, 1):
            k = keep[d, b]
            p, m = g[k], fields["q"][d, b][k]
            rows.append(torch.cat((p, m) if d == 0 else (m, p), -1))
            es.append(torch.stack((fields["cycle"][d, b][k], fields["epi"][d, b][k]), -1))
        xys.append(torch.cat(rows))
        errs.append(torch.cat(es))
    return xys, errs


def _hat(v):
    z = torch.zeros_like(v[..., 0])
    return torch.stack((z, -v[..., 2], v[..., 1], v[..., 2], z, -v[..., 0], -v[..., 1], v[..., 0], z), -1).view(*v.shape[:-1], 3, 3)


def stock_refine(xys, intr, pose, iters=ITERS, scale=SCALE):
    """refine_pose from stock operators, float64, one pair after the other (their counts differ); no host read."""
    out = []
    eye = torch.eye(3, dtype=torch.float64, device=pose.device)
    for b, xy in enumerate(xys):
        xy = xy.double()
        k0, k1 = intr[b, 0].double(), intr[b, 1].double()
        a = torch.stack(((xy[:, 0] - k0[0, 2]) / k0[0, 0], (xy[:, 1] - k0[1, 2]) / k0[1, 1], torch.ones_like(xy[:, 0])), -1)
        bb = torch.stack(((xy[:, 2] - k1[0, 2]) / k1[0, 0], (xy[:, 3] - k1[1, 2]) / k1[1, 1], torch.ones_like(xy[:, 0])), -1)
        f0 = torch.stack((k0[0, 0], k0[1, 1]))
        f1 = torch.stack((k1[0, 0], k1[1, 1]))
        R, t0 = pose[b, :3, :3].double(), pose[b, :3, 3].double()
        len0 = t0.norm()
        t = t0 / len0
        for _ in range(iters):
            Em = _hat(t) @ R
            dE = torch.cat((_hat(t) @ _hat(eye) @ R, _hat(eye) @ R))                 # (6, 3, 3)
            Eb, Ea = bb @ Em.T, a @ Em
            n = (a * Eb).sum(-1)
            g = torch.cat((Eb[:, :2] / f0, Ea[:, :2] / f1), -1)
            D = (g * g).sum(-1)
            sd = D.sqrt()
            r = n / sd
            dEb, dEa = torch.einsum("kij,nj->nki", dE, bb), torch.einsum("kij,ni->nkj", dE, a)
            dn = (a[:, None, :] * dEb).sum(-1)
            dD = 2 * (torch.cat((dEb[..., :2] / f0, dEa[..., :2] / f1), -1) * g[:, None, :]).sum(-1)
            J = dn / sd[:, None] - n[:, None] * dD / (2 * D * sd)[:, None]
            w = 1 / (1 + (r / scale) ** 2) ** 2
            H = J.T @ (J * w[:, None])
            gr = J.T @ (w * r)
            A = H + 1e-3 * torch.diag(torch.diagonal(H))
            A[3:, 3:] += torch.trace(H) / 6 * torch.outer(t, t)
            L, _ = torch.linalg.cholesky_ex(A)
            x = -torch.cholesky_solve(gr[:, None], L)[:, 0]
            R = torch.linalg.matrix_exp(_hat(x[:3])) @ R
            t = (t + x[3:]) / (t + x[3:]).norm()
        P = torch.eye(4, dtype=torch.float64, device=pose.device)
        P[:3, :3], P[:3, 3] = R, len0 * t
        out.append(P.float())
    return torch.stack(out)


def angle_deg(Ra, Rb):
    return float(torch.rad2deg(2 * torch.asin(((Ra.double() - Rb.double()).norm() / (2 * math.sqrt(2))).clamp(max=1))))


def dir_deg(ta, tb):
    ta, tb = ta.double() / ta.double().norm(), tb.double() / tb.double().norm()
    return float(torch.rad2deg(2 * torch.asin(((ta - tb).norm() / 2).clamp(max=1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    f0, f1, intr, pose, true = plane_pairs(dev)
    res = {"pairs": B, "side": S, "flow_side": HF, "refine_iters": ITERS, "scale_px": SCALE, "rounds": args.rounds, "iters": args.iters}

    # ---- (a) the kernels by events
    fields = mt.match_fields((f0, f1), intr, pose, S)
    m = mt.select(fields)
    keep = ((fields["inside"] != 0) & (fields["cycle"] <= 10.0) & mt._stride_mask(S, 4, dev)).to(torch.uint8)
    stream = _hip.stream_handle()
    q, cyc, epi, ins = fields["q"], fields["cycle"], fields["epi"], fields["inside"]
    scratch = torch.empty(_hip.lib().cpn_compact_matches_scratch(B, S), dtype=torch.int32, device=dev)
    po, st = torch.empty(B, 4, 4, device=dev), torch.empty(B, 8, dtype=torch.float64, device=dev)
    cap = 2 * S * S
    kern = {}
    kern["match_fields_ms"] = events(lambda: _hip.call("cpn_match_fields", f0.data_ptr(), f1.data_ptr(), intr.data_ptr(), pose.data_ptr(),
                                                       B, S, HF, q.data_ptr(), cyc.data_ptr(), epi.data_ptr(), ins.data_ptr(), stream),
                                     args.iters)
    kern["compact_matches_ms"] = events(lambda: _hip.call("cpn_compact_matches", keep.data_ptr(), q.data_ptr(), cyc.data_ptr(),
                                                          epi.data_ptr(), B, S, scratch.data_ptr(), m.xy.data_ptr(), m.err.data_ptr(),
                                                          m.count.data_ptr(), stream), args.iters)
    kern["refine_pose_ms"] = events(lambda: _hip.call("cpn_refine_pose", m.xy.data_ptr(), m.count.data_ptr(), intr.data_ptr(),
                                                      pose.data_ptr(), B, cap, ITERS, SCALE, po.data_ptr(), st.data_ptr(), stream),
                                    args.iters)
    res["kernels"] = kern
    res["matches_per_pair"] = [int(c) for c in m.count.cpu()]

    # ---- (a) against (b), by wall clock, alternating
    state = {}

    def s_fields():
        state["fields"] = stock_fields(f0, f1, intr, pose)

    def s_select():
        state["sel"] = stock_select(state["fields"])

    def s_refine():
        state["pose"] = stock_refine(state["sel"][0], intr, pose)

    def s_all():
        s_fields()
        s_select()
        s_refine()
    forms = {"match_fields_ms": lambda: mt.match_fields((f0, f1), intr, pose, S), "stock_fields_ms": s_fields,
             "select_ms": lambda: mt.select(fields), "stock_select_ms": s_select,
             "refine_pose_ms": lambda: mt.refine_pose(m, intr, pose, ITERS, SCALE), "stock_refine_ms": s_refine,
             "from_flows_ms": lambda: mt.from_flows((f0, f1), intr, pose, S), "stock_all_ms": s_all}
    for fn in forms.values():
        fn()
        fn()
    runs = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            runs[name].append(wall(fn))
    res["wall"] = runs
    res["median"] = {k: statistics.median(v) for k, v in runs.items()}
    res["census"] = {name[:-3]: census(fn) for name, fn in forms.items()}

    # ---- what the two results differ by
    ours = mt.from_flows((f0, f1), intr, pose, S)
    s_all()
    sf, (sxy, serr), spose = state["fields"], state["sel"], state["pose"]
    omask = (ours["fields"]["inside"] != 0) & (ours["fields"]["cycle"] <= 10.0)
    smask = sf["inside"] & (sf["cycle"] <= 10.0)
    fin = torch.isfinite(ours["fields"]["epi"]) & torch.isfinite(sf["epi"])
    diff = {"q_largest": float((ours["fields"]["q"] - sf["q"]).abs().max()),
            "cycle_largest": float((ours["fields"]["cycle"] - sf["cycle"]).abs().max()),
            "epi_largest": float((ours["fields"]["epi"] - sf["epi"])[fin].abs().max()),
            "mask_pixels_that_differ": int((omask != smask).sum()), "mask_share": float(omask.float().mean()),
            "counts": [int(c) for c in ours["matches"].count.cpu()], "stock_counts": [int(x.shape[0]) for x in sxy]}
    stats = ours["stats"].cpu()
    diff["pose_largest"] = float((ours["pose"] - spose).abs().max())
    diff["stats"] = [[float(v) for v in row] for row in stats]
    diff["degrees_from_truth"] = {
        "start": [[angle_deg(pose[b, :3, :3], true[b, :3, :3]), dir_deg(pose[b, :3, 3], true[b, :3, 3])] for b in range(B)],
        "refined": [[angle_deg(ours["pose"][b, :3, :3], true[b, :3, :3]), dir_deg(ours["pose"][b, :3, 3], true[b, :3, 3])] for b in range(B)],
        "stock": [[angle_deg(spose[b, :3, :3], true[b, :3, :3]), dir_deg(spose[b, :3, 3], true[b, :3, 3])] for b in range(B)]}
    res["difference"] = diff

    # ---- (d) from_pair against the get_z it contains
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = nv.prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    whole_forms = {"get_z_ms": lambda: model.get_z(inp), "from_pair_ms": lambda: mt.from_pair(model, inp)}
    for fn in whole_forms.values():
        fn()
        fn()
    whole = {name: [] for name in whole_forms}
    for _ in range(args.rounds):
        for name, fn in whole_forms.items():
            whole[name].append(wall(fn))
    res["from_pair"] = dict(whole, pairs=1)
    res["from_pair"]["median"] = {k: statistics.median(v) for k, v in whole.items()}
    res["from_pair"]["median"]["from_pair_less_get_z_ms"] = res["from_pair"]["median"]["from_pair_ms"] - res["from_pair"]["median"]["get_z_ms"]
    res["from_pair"]["census"] = census(whole_forms["from_pair_ms"], operators=False)
    res["from_pair"]["stats"] = [float(v) for v in mt.from_pair(model, inp)["stats"][0].cpu()]

    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
