"""The reference's full loss through the product on the MI355X: coponerf_amd.losses.loss_terms in place of the restatement in
tests/step_case.py, against upstream's own gradients of the whole step (tests/golden/step.npz, case `full`), and one
TrainStep with every switch of LossConfig on."""
import pytest
import torch

from coponerf_amd import losses
from coponerf_amd import synthetic as syn
from tests import step_case as sc
from tests.helpers import to_device
from tests.test_gpu_step import REL_L2, REL_MAX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def make_model(dev):
    from coponerf_amd import CoPoNeRF
    m = CoPoNeRF.CoPoNeRF(n_view=2, npoints=sc.CFG["S"])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(syn.make_full_weights(shapes), strict=True)
    return m.to(dev)


def test_product_loss_terms_match_upstream_gradients(dev):
    fx = sc.fixture()
    model = make_model(dev)
    inp, gt = sc.inputs()
    inp, gt = to_device(inp, dev), gt.to(dev)
    out = model(inp, val=False)
    terms = losses.loss_terms(losses.LossConfig(cycle=True, pose=True), inp, out, gt)
    assert set(terms) == {"img_loss", "cycle_loss", "pose_loss"}
    for name, t in terms.items():
        want = float(fx[f"full|loss|{name}"])
        assert abs(float(t.detach()) - want) <= 1e-3 * max(1.0, abs(want)), (name, float(t.detach()), want)
    sum(terms.values()).backward()
    rows, bad = sc.compare("full", {n: p.grad for n, p in model.named_parameters()}, fx, rel_l2=REL_L2, rel_max=REL_MAX)
    print("[full, product loss] worst tensors vs the upstream gradients:\n" + sc.report(rows, 12))
    assert not bad, sc.report(bad, 40)


class _TinyRenderer(torch.nn.Module):
    """Stand-in with the drop-in model's call contract, elementwise only: its step is bit-reproducible run to run (the real
    model's is not: its backward accumulates with atomics and the trunk's batch statistics follow), so two TrainSteps that
    claim to be the same computation can be held to the same bits."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor([0.3, -0.2, 0.1]))
        self.b = torch.nn.Parameter(torch.tensor([-0.1, 0.25, 0.05]))
        self.c = torch.nn.Parameter(torch.tensor([0.0, 0.1, -0.1]))

    def forward(self, inp, val=False):
        uv = inp["query"]["uv"] / 64.0
        rgb = torch.tanh(uv[..., :1] * self.a + uv[..., 1:] * self.b + self.c)
        return {"rgb": rgb, "at_wt": rgb.detach()[..., :1]}


def test_default_config_is_todays_step_bit_for_bit(dev):
    """TrainStep(model) and TrainStep(model, loss=LossConfig()): the same loss bits and the same updated parameters over two
    steps, and the loss is today's expression (train_step.py before the argument existed) on the same output."""
    from coponerf_amd.train_step import TrainStep
    inp, gt = sc.inputs()
    inp, gt = to_device(inp, dev), gt.to(dev)
    gt[0, 0, 3, 1] = float("nan")                                           # loss_function.py:66-69 zeroes NaNs
    a, b = _TinyRenderer().to(dev), _TinyRenderer().to(dev)
    sa, sb = TrainStep(a, lr=1e-2), TrainStep(b, lr=1e-2, loss=losses.LossConfig())
    for _ in range(2):
        ra, rb = sa(inp, gt), sb(inp, gt)
        assert torch.equal(ra["loss"], rb["loss"]) and bool(torch.isfinite(rb["loss"]))
        assert list(rb["losses"]) == ["img_loss"] and torch.equal(rb["losses"]["img_loss"], rb["loss"])
        assert ra["host_reads"] == 0 and rb["host_reads"] == 0 and bool(ra["stepped"]) and bool(rb["stepped"])
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)
    with torch.no_grad():
        sorted_inp, sorted_gt, _ = TrainStep._rays_by_tile(inp, gt)
        out = b(sorted_inp)
        zero = lambda t: torch.where(torch.isnan(t), torch.zeros_like(t), t)
        today = (zero(sorted_gt) - zero(out["rgb"])).abs().mean()
        assert torch.equal(today, losses.loss_terms(losses.LossConfig(), sorted_inp, out, sorted_gt)["img_loss"])
    assert not torch.equal(a.a.detach().cpu(), _TinyRenderer().a.detach())           # the steps did update


def test_train_step_with_every_term(dev):
    """One step of the real model with cycle, pose and ssim on: the four terms come back as detached device scalars, their sum
    is the step's loss and the host reads nothing.  Either outcome of `stepped` is legal: on synthetic weights the flows' own
    masks may be empty, which makes the SSIM term NaN (as upstream's 0 / 0), and then the guard skips the step."""
    from coponerf_amd.train_step import TrainStep
    inp, gt = sc.inputs()
    inp, gt = to_device(inp, dev), gt.to(dev)
    res = TrainStep(make_model(dev), loss=losses.LossConfig(cycle=True, pose=True, ssim=True))(inp, gt)
    assert list(res["losses"]) == ["img_loss", "ssim_loss", "cycle_loss", "pose_loss"]
    assert all(t.is_cuda and t.dim() == 0 and not t.requires_grad for t in res["losses"].values())
    assert res["host_reads"] == 0
    t = res["losses"]
    total = t["img_loss"] + t["ssim_loss"] + t["cycle_loss"] + t["pose_loss"]
    assert torch.equal(torch.nan_to_num(total, nan=-1.0), torch.nan_to_num(res["loss"], nan=-1.0))
    for name in ("img_loss", "cycle_loss", "pose_loss"):
        assert bool(torch.isfinite(t[name])), name
    stepped = bool(res["stepped"])
    ssim = float(t["ssim_loss"])
    print(f"stepped {stepped}, losses " + ", ".join(f"{k} {float(v):.6f}" for k, v in t.items()))
    assert stepped == (ssim == ssim)                       # NaN (empty masks) <=> the guard skipped the step
