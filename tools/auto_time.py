"""One 256 x 256 x 64 image (65 536 rays, B = 1) in precision = "auto" at attention gains 1, 32, 48, 64 (synthetic.peaked_weights,
latents at get_z's statistics), with the flagged fraction at each gain, and the fp16 default / reference-arithmetic mode on the
same image.  Engine defaults otherwise (two call lanes).   python tools/auto_time.py [--steps 3] [--gains 1,32,48,64]"""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import CoPoNeRF, synthetic as syn      # noqa: E402
from tests.helpers import to_device                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--gains", default="1,32,48,64")
a = ap.parse_args()
dev = torch.device("cuda:0")
H, S = 256, 64
inp = to_device(syn.make_inputs(1, H, H, H * H, seed=3), dev)
z, rel, flow = syn.make_latents(1, H, H, seed=4)
z, rel, flow = to_device(syn.latents_at_getz_statistics(z), dev), rel.to(dev), to_device(flow, dev)


def timed(model, steps):
    with torch.no_grad():
        model(inp, z=z, rel_pose=rel, val=True, flow=flow)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model(inp, z=z, rel_pose=rel, val=True, flow=flow)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


for g in (float(x) for x in a.gains.split(",")):
    model = CoPoNeRF.CoPoNeRF(n_view=2, npoints=S)
    model.load_state_dict(syn.peaked_weights(syn.make_render_weights(), g), strict=False)
    model = model.to(dev).eval()
    eng = model._engine
    res = {}
    for mode in ("f16", "auto", "f32"):
        eng._ws.clear()                     # each mode sizes its own workspaces (no allocator retries behind another's)
        torch.cuda.empty_cache()
        eng.precision = mode
        res[mode] = timed(model, a.steps if mode != "f32" else max(1, a.steps // 2 + 1))
    eng.precision = "auto"
    with torch.no_grad():
        model(inp, z=z, rel_pose=rel, val=True, flow=flow)
    k, n = eng.last_exact_rays
    print(f"gain {g:4.0f}: auto {res['auto'] * 1e3:7.2f} ms  {H * H / res['auto'] / 1e6:5.3f} M rays/s  flagged {k}/{n} "
          f"({k / n:.3f}) | f16 {res['f16'] * 1e3:7.2f} ms  {H * H / res['f16'] / 1e6:5.3f} M rays/s | "
          f"f32 {res['f32'] * 1e3:7.2f} ms  {H * H / res['f32'] / 1e6:5.3f} M rays/s | auto / f16 {res['auto'] / res['f16']:.3f}",
          flush=True)
    del model, eng                          # its workspaces (tens of GB) before the next gain's
    torch.cuda.empty_cache()
