"""Calibration of RenderEngine.auto_threshold (precision = "auto"): the attention-sharpness sweep of
tests/test_gpu_range.py (B = 1, 64 x 64, S = 32, key_map_2 / query_embed_2 / query_repeat_embed_2 scaled by the gain) rendered
in the reference-arithmetic mode and in auto mode with auto_threshold = inf (= the fp16 default, plus every ray's guard score).
Per ray: the guard score sum_i w_i (1 - w_i) |l_i| (csrc/guard.hip) against |rgb_f16 - rgb_f32| (max over channels) and the largest |at_wt_f16 - at_wt_f32| over its 2 S samples.

The seeds are NOT test_gpu_range's (21 / 22, weights 7): those are exactly tests/golden/peaked_val.npz at gain 64, which together
with the held-out sweep of tests/test_gpu_auto.py (other seeds again) tests the threshold chosen here.

    python tools/auto_calibrate.py [--rays 1024] [--margin 2] [--json out.json]"""
import argparse, json, math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import CoPoNeRF, synthetic as syn      # noqa: E402
from tests.helpers import to_device                       # noqa: E402

GAINS = (1.0, 16.0, 24.0, 32.0, 48.0, 64.0)
RGB_BAR, WT_BAR = 5e-4, 1e-3              # half of the 1e-3 / 2e-3 bars the auto mode is held to
SEEDS = dict(inputs=41, latents=42, weights=13)

ap = argparse.ArgumentParser()
ap.add_argument("--rays", type=int, default=1024)
ap.add_argument("--margin", type=float, default=2.0, help="threshold = smallest score of a bad ray / margin")
ap.add_argument("--json", default="")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, H, S, R = 1, 64, 32, a.rays
inp = to_device(syn.make_inputs(B, H, H, R, seed=SEEDS["inputs"]), dev)
z, rel, flow = syn.make_latents(B, H, H, seed=SEEDS["latents"])
z = to_device(syn.latents_at_getz_statistics(z), dev)
rel, flow = rel.to(dev), to_device(flow, dev)
scores, e_rgb, e_wt, gains = [], [], [], []
for g in GAINS:
    model = CoPoNeRF.CoPoNeRF(n_view=2, npoints=S)
    model.load_state_dict(syn.peaked_weights(syn.make_render_weights(seed=SEEDS["weights"]), g), strict=False)
    model = model.to(dev).eval()
    eng = model._engine
    with torch.no_grad():
        eng.precision, eng.auto_threshold = "auto", float("inf")
        o16 = model(inp, z=z, rel_pose=rel, val=True, flow=flow, debug=True)
        eng.precision = "f32"
        o32 = model(inp, z=z, rel_pose=rel, val=True, flow=flow)
    sc = o16["_core"]["guard_score"].reshape(-1).cpu().double()
    er = (o16["rgb"] - o32["rgb"]).abs().reshape(B * R, 3).max(dim=1).values.cpu().double()
    at = lambda o: o["at_wt"].view(B, 2, R, S).permute(0, 2, 1, 3).reshape(B * R, 2 * S)
    ew = (at(o16) - at(o32)).abs().max(dim=1).values.cpu().double()
    scores.append(sc), e_rgb.append(er), e_wt.append(ew), gains.append(torch.full_like(sc, g))
sc, er, ew, gn = (torch.cat(x) for x in (scores, e_rgb, e_wt, gains))
bad = (er > RGB_BAR) | (ew > WT_BAR)
min_bad = float(sc[bad].min()) if bool(bad.any()) else math.inf
tau = min_bad / a.margin
print(f"rays per gain {R} (seeds {SEEDS}); bad = rgb err > {RGB_BAR:g} or weight err > {WT_BAR:g}")
print("gain  score p50     p90      max   | rgb err max  weight err max | bad rays  smallest bad score | flagged at tau")
for g in GAINS:
    m = gn == g
    s_, r_, w_, b_ = sc[m], er[m], ew[m], bad[m]
    print("%4.0f  %8.3f %8.3f %8.3f | %11.2e  %14.2e | %8d  %18s | %6.3f" % (
        g, float(s_.median()), float(s_.quantile(0.9)), float(s_.max()), float(r_.max()), float(w_.max()), int(b_.sum()),
        "%.3f" % float(s_[b_].min()) if bool(b_.any()) else "-", float((s_ > tau).double().mean())))
edges = [0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, math.inf]
print("score bin          rays   rgb err max   weight err max   bad")
for lo, hi in zip(edges[:-1], edges[1:]):
    m = (sc >= lo) & (sc < hi)
    if bool(m.any()):
        print("[%5.2f, %5.2f)  %6d   %11.2e   %14.2e   %4d" % (lo, hi, int(m.sum()), float(er[m].max()), float(ew[m].max()),
                                                          int(bad[m].sum())))
print(f"smallest score of a bad ray: {min_bad:.4f}; threshold at margin {a.margin:g}: {tau:.4f}")
for mg in (1.5, 2.0, 3.0):
    print(f"margin {mg:g} (threshold {min_bad / mg:.4f}): flagged per gain " +
          ", ".join("%g: %.3f" % (g, float((sc[gn == g] > min_bad / mg).double().mean())) for g in GAINS))
if a.json:
    with open(a.json, "w") as f:
        json.dump({"seeds": SEEDS, "rays": R, "min_bad_score": min_bad, "margin": a.margin, "threshold": tau,
                   "score": sc.tolist(), "rgb_err": er.tolist(), "wt_err": ew.tolist(), "gain": gn.tolist()}, f)
