"""coponerf_amd.novel_views on the MI355X (`pytest -m gpu`): the three kernels of csrc/novel_views.hip against the float64 /
numpy-float32 forms of tests/novel_views_ref.py, and render_path against plain forward(val=True) calls.

Bounds (U = 2^-24; derived in tests/novel_views_ref.py from operation counts, none from a run):
  fitted images   |kernel - float64| <= fit_bound = (8 T + 11) U to first order, T the taps per axis: 2.2e-5 at 45 taps, where
                  half a grey level is 3.9e-3.  A crop that already has the model's size gives float(u8) / 127.5f - 1.0f exactly.
  camera path     |kernel - float64| <= U max(1, |entry|): the fp32 store.
  frames          exactly the numpy float32 rule.
  render_path     frames exactly the pack rule of its own rgb; rgb bit for bit that of a plain forward(val=True) with the same
                  pose (the same kernels on the same inputs).
"""
import numpy as np
import pytest
import torch

from coponerf_amd import synthetic as syn
from tests import novel_views_ref as nr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _fit(img0, img1, size, antialias, dev):
    from coponerf_amd.novel_views import prepare_pair
    return prepare_pair(img0, img1, hfov_deg=60.0, size=size, antialias=antialias, device=dev)["context"]["rgb"]


# ---------------------------------------------------------------------------------------------------------- fitted images
@pytest.mark.parametrize("shape,size", nr.FIT_CASES)
def test_fit_images_against_float64(dev, shape, size):
    """View 0 is seeded noise, view 1 constant images (one launch for both: they have one size), B = 3, host inputs."""
    noise, const, ref = nr.fit_case(*shape, size)
    for aa in (True, False):
        got = _fit(noise, const, size, aa, dev)
        assert got.shape == (3, 2, size, size, 3) and got.dtype == torch.float32 and got.is_cuda
        got = got.cpu().numpy().astype(np.float64)
        bound = nr.fit_bound(*shape, size, aa)
        err_noise = float(np.abs(got[:, 0] - ref[("noise", aa)]).max())
        err_const = float(np.abs(got[:, 1] - ref[("const", aa)]).max())
        spread = float(np.ptp(got[:, 1], axis=(1, 2)).max())                    # per image and channel
        print(shape, size, aa, "noise", err_noise, "const", err_const, "spread", spread, "bound", bound)
        assert err_noise <= bound and err_const <= bound
        assert spread <= 2 * bound                                              # a constant image stays constant to the bound
        if nr.crop(noise).shape[1] == size:                                     # identity: the loader's values, bit for bit
            want = nr.crop(noise).astype(np.float32) / np.float32(127.5) - np.float32(1.0)
            assert np.array_equal(got[:, 0].astype(np.float32), want)


def test_fit_images_identity_equals_prepare_input(dev):
    """At a crop of the model's size the kernel writes what cpn_prepare_input writes (coponerf_amd/shards.py)."""
    from coponerf_amd import _hip
    frames = nr.fit_case(16, 16, 16)[0]                                          # (3, 16, 16, 3): context 0, context 1, query
    got = _fit(frames[0], frames[1], 16, True, dev)
    f = torch.from_numpy(frames.copy()).to(dev).view(1, 3, 16, 16, 3)
    pix = torch.zeros(1, 1, dtype=torch.int32, device=dev)
    ctx = torch.empty(1, 2, 16, 16, 3, dtype=torch.float32, device=dev)
    q = torch.empty(1, 1, 1, 3, dtype=torch.float32, device=dev)
    _hip.call("cpn_prepare_input", f.data_ptr(), 1, 16, 16, 0, 0, 16, 16, 1, pix.data_ptr(), ctx.data_ptr(), q.data_ptr(),
              _hip.stream_handle())
    assert torch.equal(got, ctx)


def test_fit_images_batching_devices_and_mixed_sizes(dev):
    a, _, ref_a = nr.fit_case(37, 53, 16)
    b, _, ref_b = nr.fit_case(9, 12, 16)
    whole = _fit(a, b, 16, True, dev)                                            # two sizes: one launch each
    for got, ref, shape in ((whole[:, 0], ref_a, (37, 53)), (whole[:, 1], ref_b, (9, 12))):
        assert float(np.abs(got.cpu().numpy() - ref[("noise", True)]).max()) <= nr.fit_bound(*shape, 16, True)
    alone = _fit(a[0], b[0], 16, True, dev)                                      # B = 1, (Hi, Wi, 3) inputs
    assert alone.shape == (1, 2, 16, 16, 3) and torch.equal(alone, whole[:1])
    ta, tb = torch.from_numpy(a.copy()), torch.from_numpy(b.copy())
    assert torch.equal(_fit(ta.to(dev), tb.to(dev), 16, True, dev), whole)      # device inputs: the same bits
    assert torch.equal(_fit(ta, tb.to(dev), 16, True, dev), whole)              # one of each
    same = _fit(a, a, 16, False, dev)                                            # one size, one launch
    assert torch.equal(_fit(ta.to(dev), ta.to(dev), 16, False, dev), same) and torch.equal(same[:, 0], same[:, 1])


def test_prepare_pair_returns_the_input_dict(dev):
    from coponerf_amd.novel_views import fit_intrinsics, prepare_pair
    a, b = nr.fit_case(37, 53, 16)[0], nr.fit_case(9, 12, 16)[0]
    K = np.array([[[50.0, 0, 26.0], [0, 51.0, 18.0], [0, 0, 1]], [[11.0, 0, 6.5], [0, 11.5, 4.0], [0, 0, 1]]])
    inp = prepare_pair(a, b, intrinsics=K, size=16, device=dev)
    ctx, qry = inp["context"], inp["query"]
    want = np.stack([fit_intrinsics(K[0], 37, 53, 16), fit_intrinsics(K[1], 9, 12, 16)]).astype(np.float32)
    assert np.array_equal(ctx["intrinsics"].cpu().numpy(), np.broadcast_to(want, (3, 2, 4, 4)))
    assert np.array_equal(qry["intrinsics"].cpu().numpy(), np.broadcast_to(want[:1], (3, 1, 4, 4)))
    eye = torch.eye(4, device=dev)
    assert torch.equal(ctx["cam2world"], eye.expand(3, 2, 4, 4)) and torch.equal(qry["cam2world"], eye.expand(3, 1, 4, 4))
    assert qry["rgb"].shape == (3, 1, 256, 3) and not bool(qry["rgb"].any())
    uv = qry["uv"].cpu().numpy()
    assert uv.shape == (3, 1, 256, 2) and np.array_equal(uv[1, 0, 35], (3.0, 2.0))         # pixel 35 = row 2, column 3
    assert all(t.is_contiguous() and t.dtype == torch.float32 for d in (ctx, qry) for t in d.values())


# ------------------------------------------------------------------------------------------------------------ camera path
@pytest.mark.parametrize("sway", (0.0, 0.05))
def test_camera_path_against_float64(dev, sway):
    from coponerf_amd.novel_views import camera_path
    rel = nr.path_poses()
    ts = (-0.25, 0.0, 0.5, 1.0, 1.5)
    rel_d = torch.from_numpy(rel).to(dev)
    got = camera_path(rel_d, ts, sway=sway)
    assert got.shape == (5, 3, 4, 4) and got.dtype == torch.float32 and got.is_cuda
    ref = nr.path64(rel, ts, sway=sway)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print("sway", sway, "largest error / bound", float((err / nr.path_bound(ref)).max()))
    assert (err <= nr.path_bound(ref)).all()
    if sway == 0.0:                                          # the ends: the identity and rel_pose, to one fp32 rounding
        eye = np.broadcast_to(np.eye(4), (3, 4, 4))
        assert (np.abs(got[1].cpu().numpy() - eye) <= nr.U).all()
        assert (np.abs(got[3].cpu().numpy().astype(np.float64) - rel) <= nr.U * np.maximum(1.0, np.abs(rel))).all()
        assert torch.equal(got[0, 0], torch.from_numpy(nr.path64(rel[:1], [-0.25])[0, 0].astype(np.float32)).to(dev))
    assert torch.equal(camera_path(rel_d, torch.tensor(ts, dtype=torch.float64, device=dev), sway=sway), got)


# ------------------------------------------------------------------------------------------------------------- the frames
@pytest.mark.parametrize("with_depth", (False, True))
def test_pack_frames_is_the_float32_rule(dev, with_depth):
    from coponerf_amd.novel_views import pack_frames
    special, ties = nr.pack_values()
    B, h, w = 2, 7, 45
    n = B * h * w * 3
    x = syn.uniform((n,), 3, -1.2, 1.2, stream=1).numpy()
    x[:len(special)] = special
    x[len(special):len(special) + len(ties)] = ties
    rgb = x.reshape(B, h * w, 3)
    depth = None
    if with_depth:
        depth = syn.uniform((B, h * w), 3, -1.0, 12.0, stream=2).numpy()
        depth[0, :6] = (np.nan, 0.0, 10.0, -0.0, 5.0, np.inf)
        depth[1, 10:266] = (np.arange(256) / 25.6).astype(np.float32)            # every d with d / 10 * 256 near an integer
    out = torch.full((3, B, h, 2 * w if with_depth else w, 3), 77, dtype=torch.uint8, device=dev)
    pack_frames(torch.from_numpy(rgb).to(dev), out[1], None if depth is None else torch.from_numpy(depth).to(dev))
    assert np.array_equal(out[1].cpu().numpy(), nr.pack_rule(rgb, h, w, depth))
    assert bool((out[0] == 77).all()) and bool((out[2] == 77).all())            # only its own frame is written


# ------------------------------------------------------------------------------------------------------------ render_path
@pytest.fixture(scope="module")
def scene(dev):
    """The synthetic-weight model of the other GPU tests and one pair of 256 x 455 noise photos."""
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.novel_views import prepare_pair
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    return model, prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)


def _plain(model, inp, pose, uv, latents):
    """forward(val=True) with `pose` (B, 4, 4) as the query camera on the pixels uv."""
    z, rel_pose, flow = latents
    B, R = uv.shape[0], uv.shape[2]
    query = {"uv": uv, "rgb": torch.zeros(B, 1, R, 3, device=uv.device), "intrinsics": inp["query"]["intrinsics"],
             "cam2world": pose.unsqueeze(1).contiguous()}
    with torch.no_grad():
        return model({"context": inp["context"], "query": query}, z=z, rel_pose=rel_pose, val=True, flow=flow)


def test_render_path_window(dev, scene):
    from coponerf_amd.novel_views import render_path
    model, inp = scene
    y0, x0, h, w = 100, 37, 16, 24
    ts = (0.0, 0.5, 1.0)
    res = render_path(model, inp, ts, window=(y0, x0, h, w), return_rgb=True)
    frames, rgb, poses = res["frames"], res["rgb"], res["poses"]
    assert frames.shape == (3, 1, h, w, 3) and frames.dtype == torch.uint8 and frames.is_cuda
    assert rgb.shape == (3, 1, h * w, 3) and poses.shape == (3, 1, 4, 4) and res["rel_pose"].shape == (1, 4, 4)
    with torch.no_grad():
        latents = model.get_z(inp)
    assert torch.equal(latents[1], res["rel_pose"])
    assert torch.equal(poses[2], res["rel_pose"])            # t = 1: the query camera is rel_pose itself
    assert torch.equal(poses[0], torch.eye(4, device=dev)[None])
    uv = inp["query"]["uv"].view(1, 1, 256, 256, 2)[:, :, y0:y0 + h, x0:x0 + w].reshape(1, 1, h * w, 2).contiguous()
    assert np.array_equal(uv[0, 0, w + 1].cpu().numpy(), (x0 + 1.0, y0 + 1.0))
    for k in range(3):
        assert np.array_equal(frames[k].cpu().numpy(), nr.pack_rule(rgb[k].cpu().numpy(), h, w)), k
        pose = res["rel_pose"] if k == 2 else poses[k]
        plain = _plain(model, inp, pose, uv, latents)["rgb"]
        assert torch.equal(rgb[k], plain.view(1, h * w, 3)), k
    assert bool(rgb.isfinite().all()) and float(rgb.std()) > 0 and not torch.equal(rgb[0], rgb[2])
    again = render_path(model, inp, ts, window=(y0, x0, h, w))
    assert "rgb" not in again and torch.equal(again["frames"], frames)
    quiet = render_path(model, inp, ts, window=(y0, x0, h, w), announce=False)
    assert torch.equal(quiet["frames"], frames)


def test_render_path_full_image_with_depth(dev, scene):
    from coponerf_amd.novel_views import render_path
    model, inp = scene
    ts = (0.25, 1.0)
    res = render_path(model, inp, ts, sway=0.02, depth=True, return_rgb=True)
    frames, rgb, poses = res["frames"], res["rgb"], res["poses"]
    assert frames.shape == (2, 1, 256, 512, 3) and rgb.shape == (2, 1, 65536, 3)
    with torch.no_grad():
        latents = model.get_z(inp)
    for k in range(2):
        plain = _plain(model, inp, poses[k], inp["query"]["uv"], latents)
        assert torch.equal(rgb[k], plain["rgb"].view(1, 65536, 3)), k
        want = nr.pack_rule(rgb[k].cpu().numpy(), 256, 256, plain["depth_ray"].view(1, 65536).cpu().numpy())
        assert np.array_equal(frames[k].cpu().numpy(), want), k
    assert torch.equal(render_path(model, inp, ts, sway=0.02, depth=True)["frames"], frames)
