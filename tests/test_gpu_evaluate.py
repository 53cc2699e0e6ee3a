"""coponerf_amd.evaluate.Evaluator on the MI355X (`pytest -m gpu`): the device-resident table against the plain-Python
bookkeeping of tests/metrics_ref.summary_ref fed with float64 metrics of the same rendered images."""
import math

import numpy as np
import pytest
import torch

from coponerf_amd import synthetic as syn
from tests import metrics_ref as mr
from tests.helpers import to_device

pytestmark = pytest.mark.gpu

SSIM_BAR, MSE_REL, PSNR_DB, ANGLE, TRANS_REL = 5e-5, 1e-6, 1e-5, 1e-5, 1e-6       # tests/test_gpu_metrics.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=torch.float32)


def _rel_poses(B, first):
    """Estimated poses 0.1 .. 0.4 rad and 10 .. 40 degrees of direction away from the rig's: angles the acos bars hold for."""
    rel = torch.eye(4).repeat(B, 1, 1)
    for b in range(B):
        k = first + b
        rel[b, :3, :3] = _rot_y(-0.2 - 0.06 * k)
        rel[b, :3, 3] = torch.tensor([0.3, 0.06 * (k + 1), 0.05 - 0.03 * k])
    return rel


def _fake_output(B, H, W, seed, dev):
    """A joined output dict without a model: smooth images plus noise, poses as above."""
    pred, target = mr.make_case("textured", B, H, W, seed=seed)
    gt_rel = torch.eye(4).repeat(B, 1, 1)
    gt_rel[:, :3, :3] = _rot_y(-0.1)
    gt_rel[:, 0, 3] = 0.3
    out = {"rgb": torch.from_numpy(pred).to(dev).view(B, 1, H * W, 3), "rel_pose": _rel_poses(B, seed).to(dev),
           "gt_rel_pose": gt_rel.to(dev)}
    return out, torch.from_numpy(target).to(dev).view(B, 1, H * W, 3)


def _rows64(out, gt, H, W, overlaps):
    B = out["rel_pose"].shape[0]
    pred, target = out["rgb"].cpu().numpy().reshape(B, H, W, 3), gt.cpu().numpy().reshape(B, H, W, 3)
    mse, ssim = mr.mse64(pred, target), mr.ssim64(pred, target)
    pose = mr.pose64(out["rel_pose"].cpu().numpy(), out["gt_rel_pose"].cpu().numpy())
    return [dict(mse=float(mse[b]), psnr=float(mr.psnr64(mse[b])), ssim=float(ssim[b]), rot=float(pose[b, 0]),
                 trans=float(pose[b, 1]), angle_trans=float(pose[b, 2]), overlap=overlaps[b]) for b in range(B)]


def _close(name, got, want):
    if isinstance(want, float) and math.isnan(want):
        return math.isnan(got)
    base = name.split("_")[0] if not name.startswith("angle_trans") else "angle"
    tol = {"psnr": PSNR_DB, "ssim": SSIM_BAR, "mse": MSE_REL * abs(want), "rot": ANGLE, "angle": ANGLE,
           "trans": TRANS_REL * (max(abs(want), 1.0) if name.endswith("_std") else abs(want))}[base]
    return abs(got - want) <= tol


def test_add_end_to_end_against_python_bookkeeping(dev):
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.evaluate import Evaluator
    H = 64
    model = CoPoNeRF.CoPoNeRF(n_view=2, npoints=32)
    model.load_state_dict(syn.make_render_weights(), strict=False)
    model = model.to(dev).eval()
    # every bucket, and both thresholds exactly: 0.75 is still medium, 0.5 already medium
    overlaps = [[0.75, 0.76], [0.5], [0.49, 0.9]]
    as_given = [overlaps[0], torch.tensor(overlaps[1], dtype=torch.float64), torch.tensor(overlaps[2], dtype=torch.float64, device=dev)]
    ev = Evaluator()
    rows, first = [], 0
    for i, ov in enumerate(overlaps):
        B = len(ov)
        inp = to_device(syn.make_inputs(B, H, H, 0, seed=140 + i, full_image=True), dev)
        z, _, flow = (to_device(t, dev) for t in syn.make_latents(B, H, H, seed=150 + i))
        with torch.no_grad():
            out = model(inp, z=z, rel_pose=_rel_poses(B, first).to(dev), val=True, flow=flow)
        gt = {"rgb": inp["query"]["rgb"]}                                  # the loader's gt dict
        ev.add(out, gt, as_given[i], image_shape=(H, H) if i else None)    # (B, 1, 4096, 3): square when not told
        assert ev.host_reads == 0
        rows += _rows64(out, gt["rgb"], H, H, ov)
        first += B
    assert len(ev) == 5
    want = mr.summary_ref(rows, [2, 1, 2])
    got = ev.summary()
    assert ev.host_reads == 1
    table = ev.rows(host=True)
    assert table.shape == (5, 8) and table[:, 7].tolist() == [0, 0, 1, 2, 2] and table[:, 6].tolist() == sum(overlaps, [])
    assert list(got) == ["all", "small", "medium", "large"]
    assert {k: v["n"] for k, v in got.items()} == {"all": 3, "small": 1, "medium": 2, "large": 2}
    col = {"rot": 3, "trans": 4, "angle_trans": 5}
    members = {"all": list(range(5)), **{b: [i for i, r in enumerate(rows) if mr.bucket(r["overlap"]) == b] for b in ("small", "medium", "large")}}
    for key, w in want.items():
        g = got[key]
        print(key, {k: (round(g[k], 6), round(w[k], 6)) for k in ("psnr", "ssim", "mse", "rot_mean", "trans_mean", "angle_trans_mean")})
        for name, v in w.items():
            if name.endswith("_median_at") or name == "n":
                continue
            assert _close(name, g[name], v), (key, name, g[name], v)
        for name in ("rot", "trans") + (() if key == "all" else ("angle_trans",)):
            # the median is one of the table's own values: the same image the float64 bookkeeping picks
            picked = members[key][w[name + "_median_at"]]
            assert g[name + "_median"] == float(table[picked, col[name]]), (key, name)
    line = ev.format_summary(got)
    assert line.splitlines()[0].startswith("all: PSNR: ") and "Rot_median: " in line and "std_Trans_angle: " in line
    assert f"SSIM: {got['large']['ssim']:.4f}" in line.splitlines()[3]


def test_add_reads_nothing_on_the_host(dev):
    """`host_reads` is the counter the tree's other zero-read tests assert on (TrainStep, dist); here the runtime is asked as
    well: with torch's sync debug mode on `error`, any blocking device -> host read or pageable copy inside add raises."""
    from coponerf_amd.evaluate import Evaluator
    ev = Evaluator(extra={"l1": lambda p, t: (p - t).abs().mean(dim=(1, 2, 3))}, capacity=2)
    out, gt = _fake_output(2, 24, 40, 1, dev)
    ev.add(out, gt, [0.3, 0.8], image_shape=(24, 40))                      # first call: the table's allocation
    on_host, on_device = torch.tensor([0.6, 0.7], dtype=torch.float64), torch.tensor([0.6, 0.7], device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add(out, gt, [0.3, 0.8], image_shape=(24, 40))                   # grows the table 2 -> 4
        ev.add(out, gt, on_host, image_shape=(24, 40))                      # 4 -> 8
        ev.add(out, gt, on_device, image_shape=(24, 40))
        ev.add(out, gt, None, image_shape=(24, 40))
        with pytest.raises(TypeError, match="device tensors"):              # float() of each would be a read per image
            ev.add(out, gt, list(on_device), image_shape=(24, 40))
        device_rows = ev.rows()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.host_reads == 0 and device_rows.is_cuda and device_rows.shape == (10, 9)
    s = ev.summary()
    assert ev.host_reads == 1 and s["all"]["n"] == 5
    assert s["small"]["n"] == 2 and s["medium"]["n"] == 4 and s["large"]["n"] == 2      # the last call joined no bucket
    assert Evaluator(device=dev).rows().is_cuda and Evaluator(device=dev).rows().shape == (0, 8)     # empty, still on the device


def test_run_equals_add(dev):
    """One batch of two full 256 x 256 images from a (model_input, gt, overlap) loader, get_z included."""
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.evaluate import Evaluator
    from coponerf_amd.pipeline import render_images
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    inp = syn.make_inputs(2, 256, 256, 0, seed=160, full_image=True)
    overlap = torch.tensor([0.6, 0.8], dtype=torch.float64)
    loader = [(inp, {"rgb": inp["query"]["rgb"]}, overlap)]                # host tensors, as a DataLoader yields them
    ev = Evaluator().run(model, loader)
    assert ev.host_reads == 0 and len(ev) == 2
    got = ev.rows()
    assert bool(torch.isfinite(got).all()), got
    other = Evaluator()
    inp_dev = to_device(inp, dev)
    with torch.no_grad():
        for _, out in render_images(model, [inp_dev]):
            other.add(out, inp_dev["query"]["rgb"], overlap)
    assert torch.equal(got, other.rows())
    t = got.cpu()
    print("rows", t.tolist())
    assert bool((t[:, 0] > 0).all()) and bool((t[:, 2].abs() <= 1).all()) and t[:, 6].tolist() == [0.6, 0.8]
    assert sorted(ev.summary()) == ["all", "large", "medium"]


def test_extra_metric_lands_in_rows_and_summary(dev):
    from coponerf_amd.evaluate import Evaluator
    seen = []

    def stub(p, t):
        seen.append((tuple(p.shape), tuple(t.shape), float(p.abs().max()), p.is_cuda))
        return (p - t).abs().mean(dim=(1, 2, 3))

    ev = Evaluator(extra={"lpips": stub})
    assert ev.columns[-1] == "lpips"
    H, W = 16, 20
    values = []
    for i, B in enumerate((2, 1)):
        out, gt = _fake_output(B, H, W, 3 + i, dev)
        out["rgb"] = out["rgb"] * 1.5                                      # leaves [-1, 1]: the callable gets the clamped image
        ev.add(out, gt, [0.2] * B, image_shape=(H, W))
        p = out["rgb"].view(B, H, W, 3).clamp(-1, 1)
        values += (p - gt.view(B, H, W, 3)).abs().mean(dim=(1, 2, 3)).double().tolist()
    assert [s[:2] for s in seen] == [((2, 3, H, W), (2, 3, H, W)), ((1, 3, H, W), (1, 3, H, W))]
    assert all(s[2] <= 1.0 and s[3] for s in seen)
    assert ev.rows(host=True)[:, 8].tolist() == values
    s = ev.summary()
    assert s["small"]["lpips"] == pytest.approx(sum(values) / 3, rel=1e-12)
    assert s["all"]["lpips"] == pytest.approx(((values[0] + values[1]) / 2 + values[2]) / 2, rel=1e-12)      # per call, as the reference
    assert "LPIPS: " in ev.format_summary(s)
    with pytest.raises(ValueError, match="collides"):
        Evaluator(extra={"ssim": stub})


def test_growing_the_table_keeps_earlier_rows(dev):
    from coponerf_amd.evaluate import Evaluator
    small, big = Evaluator(capacity=2), Evaluator(capacity=64)
    snapshots = []
    for i, B in enumerate((2, 1, 2)):                                      # 5 images through a table that starts at 2 rows
        out, gt = _fake_output(B, 16, 20, 7 + i, dev)
        for ev in (small, big):
            ev.add(out, gt, [0.1 * (i + 1)] * B, image_shape=(16, 20))
        snapshots.append(small.rows())
    assert small._capacity == 8 and big._capacity == 64 and len(small) == 5
    final = small.rows()
    assert torch.equal(final, big.rows())
    assert torch.equal(final[:2], snapshots[0]) and torch.equal(final[:3], snapshots[1])
    assert final[:, 7].tolist() == [0, 0, 1, 2, 2]
    with pytest.raises(ValueError, match="poses"):
        small.add({**out, "rel_pose": out["rel_pose"][:1], "gt_rel_pose": out["gt_rel_pose"][:1]}, gt, None, image_shape=(16, 20))
    assert len(small) == 5
