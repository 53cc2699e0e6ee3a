"""The LPIPS training term through losses.loss_terms and TrainStep on the MI355X (`pytest -m gpu`): B = 2, 1 024 rays on a
64 x 64 image, host mask [1, 0], LPIPS.synthetic.  Pair 0's rays cover a 32 x 32 window in a shuffled order, pair 1's are
scattered.  The renderer is an elementwise stand-in with the drop-in model's call contract (tests/test_gpu_full_loss.py explains
why: its step is bit-reproducible); one step of the real model at 256 x 256 follows.  Values and gradients are held to the
end-to-end bars of tests/test_gpu_lpips_grad.py (float64 and a stock-op composition measured here)."""
import numpy as np
import pytest
import torch

from coponerf_amd import losses, shards
from coponerf_amd import lpips as cl
from coponerf_amd import synthetic as syn
from tests.helpers import to_device
from tests.test_gpu_lpips import CAP
from tests.test_gpu_lpips_grad import SEED, img_max, reference_and_bars

pytestmark = pytest.mark.gpu

B, SIDE, PATCH = 2, 64, 32
R = PATCH * PATCH
WEIGHT = 0.25
X0, Y0 = 19, 7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lp(dev):
    return cl.LPIPS.synthetic(SEED).to(dev)


class _TinyRenderer(torch.nn.Module):
    """rgb as a smooth function of uv alone: elementwise, so a step is bit-reproducible and a ray's colour does not depend on
    the order of the rays."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor([0.9, -0.7, 0.4]))
        self.b = torch.nn.Parameter(torch.tensor([-0.5, 0.8, 0.6]))
        self.c = torch.nn.Parameter(torch.tensor([0.0, 0.3, -0.3]))

    def forward(self, inp, val=False):
        uv = inp["query"]["uv"] / 8.0
        rgb = 1.2 * torch.sin(uv[..., :1] * self.a + uv[..., 1:] * self.b + self.c)       # leaves [-1, 1] in places
        return {"rgb": rgb, "at_wt": rgb.detach()[..., :1]}


def case(mask=(1, 0)):
    """(model_input with the query alone, gt (B, 1, R, 3)) on the host."""
    ys, xs = np.meshgrid(np.arange(PATCH), np.arange(PATCH), indexing="ij")
    window = (Y0 + ys.reshape(-1)) * SIDE + X0 + xs.reshape(-1)
    pix = np.stack((window[syn.permutation(R, 5)], syn.permutation(SIDE * SIDE, 6)[:R]))
    uv = torch.from_numpy(np.stack((pix % SIDE, pix // SIDE), -1).astype(np.float32)).view(B, 1, R, 2)
    gt = syn.uniform((B, 1, R, 3), 9, -1.0, 1.0, stream=2).float()
    return {"query": {"uv": uv, "rgb": gt, "mask": torch.tensor(mask, dtype=torch.int64)}}, gt


def on_device(inp, gt, dev):
    q = {k: (v if k == "mask" else v.to(dev)) for k, v in inp["query"].items()}      # the mask stays on the host
    return {"query": q}, gt.to(dev)


def patches(rgb, gt, inp):
    """Pair 0's prediction and target as (1, 3, 32, 32) images, on the host."""
    uv = inp["query"]["uv"][:1, 0].cpu()
    return (losses.patch_from_rays(rgb[:1].reshape(1, R, 3).detach().cpu(), uv, PATCH).contiguous(),
            losses.patch_from_rays(gt[:1].reshape(1, R, 3).cpu(), uv, PATCH).contiguous())


def test_term_value_and_gradient(dev, lp):
    inp, gt = on_device(*case(), dev)
    model = _TinyRenderer().to(dev)
    rgb = model(inp)["rgb"].detach().requires_grad_(True)
    terms = losses.loss_terms(losses.LossConfig(lpips=WEIGHT), inp, {"rgb": rgb}, gt, perceptual=lp)
    assert list(terms) == ["img_loss", "lpips_loss"]
    terms["lpips_loss"].backward()
    pp, pt = patches(rgb, gt, inp)
    assert float(pp.abs().max()) > 1.0
    want, gwant, bar, gbar = reference_and_bars(pp, pt, dev, "pair 0's patch")
    # the value: weight x differentiable of pair 0's patch
    ppd = pp.to(dev).requires_grad_(True)
    direct = lp.differentiable(ppd, pt.to(dev))
    direct.sum().backward()
    got = terms["lpips_loss"].detach().cpu().double()
    d_term, d_direct = abs(float(got) / WEIGHT - float(want[0])), abs(float(direct.detach()[0]) - float(want[0]))
    print(f"lpips_loss / weight {float(got) / WEIGHT:.7f}  differentiable {float(direct.detach()[0]):.7f}  lpips64 {float(want[0]):.7f}  "
          f"bar {float(bar[0]):.2e}")
    assert d_term <= float(bar[0]) + 2.0 ** -24 * float(want[0]) and d_direct <= float(bar[0])      # + the weight's rounding
    assert d_term <= CAP
    # the gradient to rgb: the direct gradient scattered back to the rays, and zero on pair 1
    uv = inp["query"]["uv"][0, 0].long().cpu()
    at_ray = lambda g: g[0][:, uv[:, 1] - Y0, uv[:, 0] - X0].t()                        # (3, 32, 32) -> (R, 3)
    g = rgb.grad.cpu().double()
    e_term = float((g[0, 0] / WEIGHT - at_ray(gwant)).abs().max())
    e_direct = float((at_ray(ppd.grad.cpu().double()) - at_ray(gwant)).abs().max())
    print(f"max |d lpips_loss / d rgb / weight - f64| {e_term:.2e}  max |direct - f64| {e_direct:.2e}  bar {float(gbar[0]):.2e}  "
          f"max |grad64| {float(img_max(gwant)[0]):.3e}")
    assert e_term <= float(gbar[0]) and e_direct <= float(gbar[0])
    assert bool((g[1] == 0).all()) and float(g[0].abs().max()) > 0


def test_step_with_the_term_sorted_and_unsorted(dev, lp):
    from coponerf_amd.train_step import TrainStep
    inp, gt = on_device(*case(), dev)
    res = []
    for sort in (True, False):
        model = _TinyRenderer().to(dev)
        with torch.no_grad():
            pp, pt = patches(model(inp)["rgb"], gt, inp)
        step = TrainStep(model, lr=1e-3, loss=losses.LossConfig(lpips=WEIGHT), perceptual=lp)
        step.sort_rays = sort
        r = step(inp, gt)
        assert (r["ray_order"] is not None) == sort
        assert list(r["losses"]) == ["img_loss", "lpips_loss"] and r["host_reads"] == 0 and bool(r["stepped"])
        assert torch.equal(r["loss"], r["losses"]["img_loss"] + r["losses"]["lpips_loss"])
        assert not torch.equal(model.a.detach().cpu(), _TinyRenderer().a.detach())      # the step did update
        res.append(float(r["losses"]["lpips_loss"]) / WEIGHT)
    want, _, bar, _ = reference_and_bars(pp, pt, dev, "pair 0's patch")
    print(f"lpips_loss / weight with the rays sorted {res[0]:.7f}, as given {res[1]:.7f}  lpips64 {float(want[0]):.7f}  "
          f"bar {float(bar[0]):.2e}")
    for v in res:                                                                       # the same patch either way
        assert abs(v - float(want[0])) <= float(bar[0]) + 2.0 ** -24 * float(want[0]) and abs(v - float(want[0])) <= CAP


def test_no_patch_pair_is_an_exact_zero(dev, lp):
    from coponerf_amd.train_step import TrainStep
    inp, gt = on_device(*case(mask=(0, 0)), dev)
    rgb = _TinyRenderer().to(dev)(inp)["rgb"]
    term = losses.loss_terms(losses.LossConfig(lpips=WEIGHT), inp, {"rgb": rgb}, gt, perceptual=lp)["lpips_loss"]
    assert term.is_cuda and float(term) == 0.0 and not term.requires_grad
    r = TrainStep(_TinyRenderer().to(dev), loss=losses.LossConfig(lpips=WEIGHT), perceptual=lp)(inp, gt)
    assert float(r["losses"]["lpips_loss"]) == 0.0 and torch.equal(r["loss"], r["losses"]["img_loss"]) and bool(r["stepped"])


def test_weight_zero_is_todays_step_bit_for_bit(dev):
    from coponerf_amd.train_step import TrainStep
    inp, gt = on_device(*case(), dev)
    a, b = _TinyRenderer().to(dev), _TinyRenderer().to(dev)
    sa, sb = TrainStep(a, lr=1e-2), TrainStep(b, lr=1e-2, loss=losses.LossConfig(lpips=0.0))
    for _ in range(2):
        ra, rb = sa(inp, gt), sb(inp, gt)
        assert torch.equal(ra["loss"], rb["loss"]) and list(ra["losses"]) == list(rb["losses"]) == ["img_loss"]
        assert sorted(ra) == sorted(rb)
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)


def test_what_the_term_refuses(dev, lp):
    from coponerf_amd.train_step import TrainStep
    inp, gt = on_device(*case(), dev)
    cfg = losses.LossConfig(lpips=WEIGHT)
    with pytest.raises(ValueError, match="perceptual"):
        TrainStep(_TinyRenderer().to(dev), loss=cfg)(inp, gt)                           # no network: the first step raises
    bare = {"query": {k: v for k, v in inp["query"].items() if k != "mask"}}
    with pytest.raises(ValueError, match="mask"):
        TrainStep(_TinyRenderer().to(dev), loss=cfg, perceptual=lp)(bare, gt)
    moved = {"query": dict(inp["query"], mask=inp["query"]["mask"].to(dev))}
    with pytest.raises(ValueError, match="on the host"):
        TrainStep(_TinyRenderer().to(dev), loss=cfg, perceptual=lp)(moved, gt)


def test_assembler_hands_the_mask_over_on_the_host(dev, tmp_path):
    rng = np.random.default_rng(5)
    n, Hs, Ws = 3, 256, 455
    frames = rng.integers(0, 256, size=(n, Hs, Ws, 3), dtype=np.uint8)
    c2w = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    intr = np.tile(np.array([0.5, 0.89, 0.5, 0.5], dtype=np.float32), (n, 1))
    path = str(tmp_path / "scene.cpnshard")
    shards.write_shard(path, frames, np.arange(n), c2w, intr)
    sh = shards.Shard(path)
    asm = shards.BatchAssembler(4, Hs, Ws, R, dev, lpips=True)
    draw = np.random.default_rng(17)
    for b in range(4):
        asm.fill(b, sh, (0, 1, 2), draw)
    inp, gt = asm.to_model_input()
    mask = inp["query"]["mask"]
    assert mask.dtype == torch.int64 and tuple(mask.shape) == (4,) and not mask.is_cuda and torch.equal(mask, asm.mask)
    assert 0 < int(mask.sum()) < 4                                                      # both branches among the four
    assert inp["query"]["uv"].shape == (4, 1, R, 2) and gt["rgb"].shape == (4, 1, R, 3)
    uv = inp["query"]["uv"][:, 0].cpu()
    for b in range(4):
        if int(mask[b]):                                                                # a patch: rebuilt from its rays, it is the crop's window
            x0, y0 = int(uv[b, :, 0].min()), int(uv[b, :, 1].min())
            got = losses.patch_from_rays(gt["rgb"][b:b + 1, 0].cpu(), uv[b:b + 1], PATCH)[0].permute(1, 2, 0)
            crop = torch.from_numpy(frames[2, asm.y0 + y0:asm.y0 + y0 + PATCH, asm.x0 + x0:asm.x0 + x0 + PATCH].astype(np.float32))
            assert torch.equal(got, crop / 127.5 - 1)
    plain = shards.BatchAssembler(1, Hs, Ws, R, dev)
    plain.fill(0, sh, (0, 1, 2), draw)
    assert "mask" not in plain.to_model_input()[0]["query"]                             # everything else is unchanged


def test_one_step_of_the_real_model(dev, lp):
    """256 x 256, B = 2, 1 024 rays, pair 0 a patch: the term joins the loss, the step is taken, the host reads nothing."""
    from coponerf_amd.train_step import TrainStep
    from tests.test_gpu_full_loss import make_model
    inp = syn.make_inputs(B, 256, 256, R, seed=71)
    ys, xs = np.meshgrid(np.arange(PATCH), np.arange(PATCH), indexing="ij")
    inp["query"]["uv"][0, 0] = torch.from_numpy(np.stack((100 + xs.reshape(-1), 60 + ys.reshape(-1)), -1).astype(np.float32))
    gt = inp["query"]["rgb"].clone()
    inp, gt = to_device(inp, dev), gt.to(dev)
    inp["query"]["mask"] = torch.tensor([1, 0], dtype=torch.int64)
    r = TrainStep(make_model(dev), loss=losses.LossConfig(lpips=WEIGHT), perceptual=lp)(inp, gt)
    t = r["losses"]
    print("real model: " + ", ".join(f"{k} {float(v):.6f}" for k, v in t.items()) + f", stepped {bool(r['stepped'])}")
    assert list(t) == ["img_loss", "lpips_loss"] and r["host_reads"] == 0
    assert bool(torch.isfinite(t["lpips_loss"])) and float(t["lpips_loss"]) > 0
    assert torch.equal(r["loss"], t["img_loss"] + t["lpips_loss"])
    assert bool(r["stepped"])
